"""CPU tests of the function-draw boundary: bad arguments fail with GPT_ERR_BAD_DIMS and their own
message before any device call, the header declares the entries, the library exports them with
matching signatures and the Julia shim binds them."""
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

SYMS = ["gpt_gp_rand", "gpt_gp_post_rand", "gpt_gpnt_draw_theta", "gpt_egp_draw_prior",
        "gpt_egp_draw_posterior", "gpt_nlml_draw_theta", "gpt_gpdraw_last_timing"]
N, D, NT, S = 12, 3, 5, 2
HANDLE = C.c_void_p(None)        # no handle exists without a device: the checks that need none run first


def _problem():
    rng = np.random.default_rng(5)
    return dict(X=np.asfortranarray(rng.standard_normal((N, D))),
                Xt=np.asfortranarray(rng.standard_normal((NT, D))),
                h=np.array([1.0, 1.2, 0.8, 0.9, 0.04]), F=np.ones(N * S), fmu=np.ones(NT),
                Fp=np.ones(NT * S), cov=np.ones(NT * NT))


def _p(p, name, null):
    from gpt_amd import _lib
    return None if null.get(name) else p[name].ctypes.data_as(_lib.P_D)


def _rand(p, n=N, d=D, lh=D + 2, jitter=1e-6, s=S, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gp_rand(_p(p, "X", null), n, d, _p(p, "h", null), lh, jitter, s, 7,
                                  _p(p, "F", null))


def _prior(p, jitter=1e-6, s=S, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_egp_draw_prior(HANDLE, _p(p, "h", null), D + 2, jitter, s, 7, None,
                                         _p(p, "F", null), None)


def _posterior(p, nt=NT, jitter=1e-6, observed=0, s=S, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_egp_draw_posterior(HANDLE, _p(p, "h", null), D + 2, _p(p, "Xt", null), nt,
                                             jitter, observed, s, 7, None, _p(p, "fmu", null),
                                             _p(p, "Fp", null), _p(p, "cov", null), None)


def _theta(p, s=S, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_nlml_draw_theta(HANDLE, _p(p, "h", null), D + 2, s, 7, None,
                                          _p(p, "F", null), None)


def _fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert text in str(ei.value), (text, str(ei.value))


BAD_JITTER = [-1e-9, float("nan"), float("inf"), -float("inf")]


@pytest.mark.parametrize("call", [_rand, _prior, _posterior], ids=["rand", "prior", "posterior"])
@pytest.mark.parametrize("jitter", BAD_JITTER)
def test_bad_jitter_fails_without_a_device(call, jitter):
    _fails(call(_problem(), jitter=jitter), "jitter must be >= 0 and finite")


@pytest.mark.parametrize("call", [_rand, _prior, _posterior, _theta],
                         ids=["rand", "prior", "posterior", "theta"])
@pytest.mark.parametrize("s", [0, -1, 4097])
def test_bad_draw_count_fails_without_a_device(call, s):
    _fails(call(_problem(), s=s), "S must be in")


def test_posterior_without_samples_takes_zero_draws_but_no_other_bad_count():
    p = _problem()
    _fails(_posterior(p, s=0, Fp=True), "null handle")          # S = 0 passes with F NULL
    _fails(_posterior(p, s=-1, Fp=True), "S must be in 0..4096")
    _fails(_posterior(p, s=4097, Fp=True), "S must be in 0..4096")


@pytest.mark.parametrize("nt", [0, -3, 8193])
def test_bad_test_count_fails_without_a_device(nt):
    _fails(_posterior(_problem(), nt=nt), "Ntest must be in 1..8192")


@pytest.mark.parametrize("observed", [-1, 2])
def test_bad_observed_flag_fails_without_a_device(observed):
    _fails(_posterior(_problem(), observed=observed), "observed must be 0 or 1")


def test_null_handles_and_outputs_fail_without_a_device():
    p = _problem()
    _fails(_prior(p), "null handle or output")
    _fails(_posterior(p), "null handle")
    _fails(_posterior(p, Xt=True), "null test input")
    _fails(_posterior(p, fmu=True, Fp=True, cov=True, s=0), "no output asked for")
    _fails(_theta(p), "null handle or output")
    _fails(_rand(p, F=True), "null output")
    _fails(_rand(p, X=True), "null input array")
    _fails(_rand(p, h=True), "null hyperparams")


@pytest.mark.parametrize("bad", [dict(n=16385), dict(n=0), dict(d=17), dict(d=0), dict(lh=4),
                                 dict(lh=2), dict(lh=D + 3)],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_one_shot_bad_dimensions_fail_without_a_device(bad):
    from gpt_amd import _lib
    assert _rand(_problem(), **bad) == _lib.GPT_ERR_BAD_DIMS


@pytest.mark.parametrize("value", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("k", range(D + 2))
def test_one_shot_bad_hyper_values_fail_without_a_device(value, k):
    p = _problem()
    p["h"][k] = value
    _fails(_rand(p), "hyperparams must be positive and finite")


def test_python_wrappers_raise_without_a_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    p = _problem()
    for kw in (dict(S=0), dict(S=4097), dict(jitter=-1.0), dict(jitter=float("nan"))):
        with pytest.raises(GPTError) as ei:
            G.GPrand(p["X"], [1.0, 1.2, 0.8], 0.9, **kw)
        assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(GPTError):
        G.GPrand(p["X"], [1.0, 1.2], 0.9)                  # 2 length scales, D = 3
    with pytest.raises(GPTError):
        G.GPrand(p["X"], 1.0, -0.9)
    with pytest.raises(GPTError) as ei:
        G._draw_z(np.zeros((N, 3)), N, 2)
    assert ei.value.code == GPT_ERR_BAD_DIMS
    assert G._draw_z(np.zeros(N), N, 1).shape == (N, 1) and G._draw_z(None, N, 1) is None
    assert G.GPPosteriorDraw._fields == ("fmu", "samples", "cov", "z")
    for name in ("draw_prior", "draw_posterior", "predict_cov"):
        assert callable(getattr(G.ExactGP, name))
    assert callable(G.NoTensorMarginal.draw_theta) and callable(G.gp_posterior_draw_oneshot)


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


def test_julia_shim_binds_the_entries():
    calls = {c[1]: c[0] for c in all_calls()}
    for s in SYMS[:3]:                 # the host-pointer forms: the shim keeps no handles
        assert calls.get(s) == "GPT_SGLD_HIP.jl", s
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "julia",
                            "GPT_SGLD_HIP.jl")).read()
    exported = src.split("module GPT_SGLD_HIP")[1].split("const LIB")[0]
    for name in ("GPrand", "GPpost_rand", "GPNT_draw_theta", "fhatdraw", "createmesh"):
        assert name in exported, name
