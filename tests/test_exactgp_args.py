"""CPU tests of the exact-GP boundary: bad arguments fail with GPT_ERR_BAD_DIMS before any device
call, the header declares the entries, the library exports them with matching signatures and the
Julia shim binds the host forms."""
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

SYMS = ["gpt_egp_create", "gpt_egp_eval", "gpt_egp_eval_timed", "gpt_egp_predict",
        "gpt_egp_destroy", "gpt_gp_nlogmarginal", "gpt_gp_predict"]
N, D, NT = 12, 3, 5


def _problem():
    rng = np.random.default_rng(3)
    return dict(X=np.asfortranarray(rng.standard_normal((N, D))), y=rng.standard_normal(N),
                Xt=np.asfortranarray(rng.standard_normal((NT, D))), yt=rng.standard_normal(NT),
                h=np.array([1.0, 1.2, 0.8, 0.9, 0.04]), val=np.ones(1), grad=np.ones(D + 2),
                fmu=np.ones(NT), fs2=np.ones(NT), lp=np.ones(NT))


def _p(p, name, null):
    from gpt_amd import _lib
    return None if null.get(name) else p[name].ctypes.data_as(_lib.P_D)


def _nlogmarginal(p, n=N, d=D, lh=D + 2, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gp_nlogmarginal(_p(p, "X", null), n, d, _p(p, "y", null),
                                          _p(p, "h", null), lh, 1, _p(p, "val", null),
                                          _p(p, "grad", null))


def _predict(p, n=N, d=D, lh=D + 2, nt=NT, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gp_predict(_p(p, "X", null), n, d, _p(p, "y", null), _p(p, "h", null),
                                     lh, _p(p, "Xt", null), nt, _p(p, "yt", null),
                                     _p(p, "fmu", null), _p(p, "fs2", null), _p(p, "lp", null))


def _create(p, n=N, d=D, **null):
    from gpt_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().gpt_egp_create(_p(p, "X", null), n, d, _p(p, "y", null), C.byref(h))
    assert h.value is None
    return rc


def _fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert text in str(ei.value), (text, str(ei.value))


BAD_DIMS = [dict(n=16385), dict(n=0), dict(d=17), dict(d=0), dict(X=True), dict(y=True)]
BAD_DIMS_TEXT = ["exact GP: N must be in 1..16384"] * 2 + ["exact GP: D must be in 1..16"] * 2 + \
                ["exact GP: null input array"] * 2
BAD_HYPER = [dict(lh=4), dict(lh=2), dict(lh=D + 3), dict(h=True)]
BAD_HYPER_TEXT = ["exact GP: hyperparams must have 3 or D + 2 entries"] * 3 + \
                 ["exact GP: null hyperparams"]
BAD_VALUE_TEXT = "exact GP: hyperparams must be positive and finite"


@pytest.mark.parametrize("call", [_nlogmarginal, _predict, _create],
                         ids=["nlogmarginal", "predict", "create"])
@pytest.mark.parametrize("bad", BAD_DIMS, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_dimensions_fail_without_a_device(call, bad):
    from gpt_amd import _lib
    rc = call(_problem(), **bad)
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    _fails(call(_problem(), **bad), BAD_DIMS_TEXT[BAD_DIMS.index(bad)])


@pytest.mark.parametrize("call", [_nlogmarginal, _predict], ids=["nlogmarginal", "predict"])
@pytest.mark.parametrize("bad", BAD_HYPER, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_hyper_vector_fails_without_a_device(call, bad):
    from gpt_amd import _lib
    assert call(_problem(), **bad) == _lib.GPT_ERR_BAD_DIMS
    _fails(call(_problem(), **bad), BAD_HYPER_TEXT[BAD_HYPER.index(bad)])


@pytest.mark.parametrize("call", [_nlogmarginal, _predict], ids=["nlogmarginal", "predict"])
@pytest.mark.parametrize("value", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("k", range(D + 2))
def test_bad_hyper_values_fail_without_a_device(call, value, k):
    from gpt_amd import _lib
    p = _problem()
    p["h"][k] = value
    assert call(p) == _lib.GPT_ERR_BAD_DIMS
    _fails(call(p), BAD_VALUE_TEXT)
    p["h"] = np.array([1.0, value, 0.04]) if k == 1 else p["h"]
    assert call(p, lh=p["h"].size) == _lib.GPT_ERR_BAD_DIMS
    _fails(call(p, lh=p["h"].size), BAD_VALUE_TEXT)


def test_null_outputs_and_handles_fail_without_a_device():
    from gpt_amd import _lib
    lib, P = _lib.lib(), _lib.P_D
    p = _problem()
    assert _nlogmarginal(p, val=True) == _lib.GPT_ERR_BAD_DIMS
    assert _nlogmarginal(p, grad=True) == _lib.GPT_ERR_BAD_DIMS
    for name in ("Xt", "fmu", "fs2", "yt"):             # lp without ytest
        assert _predict(p, **{name: True}) == _lib.GPT_ERR_BAD_DIMS
    assert _predict(p, nt=0) == _lib.GPT_ERR_BAD_DIMS
    assert lib.gpt_egp_create(p["X"].ctypes.data_as(P), N, D, p["y"].ctypes.data_as(P),
                              None) == _lib.GPT_ERR_BAD_DIMS
    h = p["h"].ctypes.data_as(P)
    assert lib.gpt_egp_eval(None, h, D + 2, 0, p["val"].ctypes.data_as(P), None,
                            None) == _lib.GPT_ERR_BAD_DIMS
    assert lib.gpt_egp_eval_timed(None, h, D + 2, 0, p["val"].ctypes.data_as(P), None,
                                  None) == _lib.GPT_ERR_BAD_DIMS
    assert lib.gpt_egp_predict(None, h, D + 2, p["Xt"].ctypes.data_as(P), NT, None, 0,
                               p["fmu"].ctypes.data_as(P), p["fs2"].ctypes.data_as(P),
                               None) == _lib.GPT_ERR_BAD_DIMS
    assert lib.gpt_egp_destroy(None) == _lib.GPT_OK
    _fails(_nlogmarginal(p, val=True), "exact GP: null output")
    _fails(_nlogmarginal(p, grad=True), "exact GP: null output")
    for name in ("Xt", "fmu", "fs2"):
        _fails(_predict(p, **{name: True}), "exact GP: null test input or output")
    _fails(_predict(p, yt=True), "exact GP: lp needs ytest")
    _fails(_predict(p, nt=0), "exact GP: Ntest must be in 1..2^31-1")
    _fails(lib.gpt_egp_create(p["X"].ctypes.data_as(P), N, D, p["y"].ctypes.data_as(P), None),
           "exact GP: null handle pointer")
    _fails(lib.gpt_egp_eval(None, h, D + 2, 0, p["val"].ctypes.data_as(P), None, None),
           "exact GP: null handle or output")
    _fails(lib.gpt_egp_eval_timed(None, h, D + 2, 0, p["val"].ctypes.data_as(P), None, None),
           "exact GP: null phase_ms")
    _fails(lib.gpt_egp_eval_timed(None, h, D + 2, 0, p["val"].ctypes.data_as(P), None,
                                  p["grad"].ctypes.data_as(P)), "exact GP: null handle or output")
    _fails(lib.gpt_egp_predict(None, h, D + 2, p["Xt"].ctypes.data_as(P), NT, None, 0,
                               p["fmu"].ctypes.data_as(P), p["fs2"].ctypes.data_as(P), None),
           "exact GP: null handle")


def test_python_wrappers_raise_without_a_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    p = _problem()
    with pytest.raises(GPTError) as ei:
        G.ExactGP(np.zeros((3, 17)), np.zeros(3))
    assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(GPTError):
        G.GP_nlogmarginal(p["X"], p["y"], 0.04, 0.81, [1.0, 1.0])       # 2 length scales, D = 3
    with pytest.raises(GPTError):
        G.GP_nlogmarginal(p["X"], p["y"], -0.04, 0.81, 1.0)
    with pytest.raises(ValueError):
        G.ExactGP(p["X"], p["y"][:-1])
    assert G.GPPrediction._fields == ("ymu", "ys2", "fmu", "fs2", "lp")      # GPkit's order


def test_header_declares_and_library_exports_the_entries():
    from gpt_amd import _lib
    names = header_functions()
    protos = header_prototypes()
    lib = _lib.lib()
    for s in SYMS:
        assert s in names, s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert len(_lib.SIGNATURES[s][1]) == len(protos[s][1]), s


def test_julia_shim_binds_the_host_forms():
    calls = {c[1]: c[0] for c in all_calls()}
    assert calls.get("gpt_gp_nlogmarginal") == "GPT_SGLD_HIP.jl"
    assert calls.get("gpt_gp_predict") == "GPT_SGLD_HIP.jl"
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "julia",
                            "GPT_SGLD_HIP.jl")).read()
    exported = src.split("module GPT_SGLD_HIP")[1].split("const LIB")[0]
    for name in ("GP_nlogmarginal", "GP_gradnlogmarginal", "GP_predict"):
        assert name in exported, name
