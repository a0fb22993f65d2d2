"""CPU tests of the X-mode boundary (gpt_sgld_session_create_x, gpt_sgld_session_staging,
gpt_sgld_regression_chains_x): bad arguments fail with GPT_ERR_BAD_DIMS before any device call,
the header declares the entries, the library exports them and the Julia shim binds the host form."""
import ctypes as C
import os

import numpy as np
import pytest

try:
    from tests.test_capi import header_functions
    from tests.test_julia_shim import all_calls, header_prototypes
except ImportError:            # a foreign `tests` package on the path: the modules beside this one
    from test_capi import header_functions
    from test_julia_shim import all_calls, header_prototypes

SYMS = ["gpt_sgld_session_create_x", "gpt_sgld_session_staging", "gpt_sgld_regression_chains_x"]
n, D, N, r, Q, m = 24, 3, 29, 3, 10, 8


def _problem(nch=3):
    from gpt_amd import GPT_SGLD as G
    rng = np.random.default_rng(5)
    return dict(X=np.asfortranarray(rng.standard_normal((N, D))),
                Z=np.asfortranarray(rng.standard_normal((n, D))),
                b=np.asfortranarray(rng.random((n, D))), y=rng.standard_normal(N),
                ls=np.ascontiguousarray(1.0 + 0.1 * rng.random((max(nch, 1), D))),
                sg=np.ones(max(nch, 1)), I=G.samplenz(r, D, Q, 1),
                cfg=G.make_config(n, D, N, r, Q, m, 1e-4, 1e-6, 0.05, 1.0, 0, 1, 0))


def _chains_x(p, nch=3, ls_len=D, **null):
    """Raw gpt_sgld_regression_chains_x call; the arrays named in `null` are passed as NULL."""
    from gpt_amd import _lib
    P_D, P_I32, P_U64 = _lib.P_D, _lib.P_I32, _lib.P_U64
    k = max(nch, 1)
    ptr = lambda name: None if null.get(name) else p[name].ctypes.data_as(P_D)
    seeds = np.arange(1, k + 1, dtype=np.uint64)
    ys = (P_D * k)(*[p["y"].ctypes.data_as(P_D)] * k)
    st = np.zeros(k, dtype=np.int32)
    return _lib.lib().gpt_sgld_regression_chains_x(
        C.byref(p["cfg"]), nch, seeds.ctypes.data_as(P_U64), ptr("X"), ys, ptr("ls"), ls_len,
        ptr("sg"), 1.0, ptr("Z"), ptr("b"), p["I"].ctypes.data_as(P_I32), None, None, None, None,
        None, st.ctypes.data_as(P_I32))


def _create_x(p, nch=3, ls_len=D, **null):
    """Raw gpt_sgld_session_create_x call.  The device pointers are the host arrays' addresses:
    the argument checks must reject the call before anything reads through them."""
    from gpt_amd import _lib
    k = max(nch, 1)
    ptr = lambda name: None if null.get(name) else C.c_void_p(p[name].ctypes.data)
    seeds = np.arange(1, k + 1, dtype=np.uint64)
    ys = (C.c_void_p * k)(*[p["y"].ctypes.data] * k)
    h = C.c_void_p()
    rc = _lib.lib().gpt_sgld_session_create_x(
        C.byref(p["cfg"]), nch, seeds.ctypes.data_as(_lib.P_U64), ptr("X"), ys, ptr("ls"), ls_len,
        None if null.get("sg") else p["sg"].ctypes.data_as(_lib.P_D), 1.0, ptr("Z"), ptr("b"),
        p["I"].ctypes.data_as(_lib.P_I32), 1, None, C.byref(h))
    assert h.value is None
    return rc


BAD = [dict(ls_len=2), dict(ls_len=0), dict(ls_len=D + 1), dict(X=True), dict(Z=True),
       dict(sg=True), dict(nch=0), dict(nch=-1)]


@pytest.mark.parametrize("call", [_chains_x, _create_x], ids=["chains_x", "create_x"])
@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_arguments_raise_without_a_device(call, bad):
    from gpt_amd import _lib
    p = _problem()
    rc = call(p, **bad)
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS


def test_python_wrapper_rejects_bad_length_scales_without_a_device():
    """GPTregression_chains_x with a length-scale row of the wrong width reaches the library's
    ls_len check and raises GPTError."""
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPTError
    p = _problem()
    with pytest.raises(GPTError):
        G.GPTregression_chains_x(p["X"], p["y"], p["ls"][:, :2], 1.0, 1.0, p["Z"], p["b"], 0.05,
                                 p["I"], r, Q, m, 1e-4, 1e-6, 0, 1, [1, 2, 3])


def test_header_declares_and_library_exports_the_x_entries():
    from gpt_amd import _lib
    names = header_functions()
    lib = _lib.lib()
    for s in SYMS:
        assert s in names, s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert len(_lib.SIGNATURES[s][1]) == len(header_prototypes()[s][1]), s


def test_staging_rejects_null_arguments():
    from gpt_amd import _lib
    assert _lib.lib().gpt_sgld_session_staging(None, None) == _lib.GPT_ERR_BAD_DIMS


def test_julia_shim_binds_the_host_form():
    calls = [c for c in all_calls() if c[1] == "gpt_sgld_regression_chains_x"]
    assert len(calls) == 1 and calls[0][0] == "GPT_SGLD_HIP.jl"
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "julia",
                            "GPT_SGLD_HIP.jl")).read()
    # exported, and its size checks precede the ccall
    assert "GPTregression_chains_x" in src.split("module GPT_SGLD_HIP")[1].split("const LIB")[0]
    body = src.split("function GPTregression_chains_x")[1]
    assert body.index("one column of length scales per chain") < body.index("ccall(")
