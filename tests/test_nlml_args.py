"""CPU tests of the RFF-marginal boundary (gpt_nlml_*, its one-shot forms and gpt_rff_kernel_error):
every single bad argument fails with GPT_ERR_BAD_DIMS and its own message before any device call,
the header declares the entries and the library exports them with matching signatures."""
import ctypes as C

import numpy as np
import pytest

try:
    from tests.test_capi import header_functions
    from tests.test_julia_shim import all_calls, header_prototypes
except ImportError:            # a foreign `tests` package on the path: the modules beside this one
    from test_capi import header_functions
    from test_julia_shim import all_calls, header_prototypes

SYMS = ["gpt_nlml_create", "gpt_nlml_eval", "gpt_nlml_eval_timed", "gpt_nlml_features",
        "gpt_nlml_predict", "gpt_nlml_draw_theta", "gpt_nlml_destroy", "gpt_gpnt_nlogmarginal",
        "gpt_gpnt_predict", "gpt_gpnt_draw_theta", "gpt_rff_kernel_error"]
N, D, NF, NT, S = 12, 3, 6, 5, 2
HANDLE = C.c_void_p(None)        # no handle exists without a device: the checks that need none run first


def _problem():
    rng = np.random.default_rng(11)
    return dict(X=np.asfortranarray(rng.standard_normal((N, D))), y=rng.standard_normal(N),
                Z=np.asfortranarray(rng.standard_normal((NF, D))), b=rng.random(NF),
                Xt=np.asfortranarray(rng.standard_normal((NT, D))), yt=rng.standard_normal(NT),
                h=np.array([1.0, 1.2, 0.8, 0.9, 0.04]), val=np.ones(1), grad=np.ones(D + 2),
                fmu=np.ones(NT), fs2=np.ones(NT), lp=np.ones(NT), theta=np.ones(NF * S),
                out3=np.ones(3), ms=np.ones(16))


def _p(p, name, null):
    from gpt_amd import _lib
    return None if null.get(name) else p[name].ctypes.data_as(_lib.P_D)


def _head(p, N_, d, n, null):
    return [_p(p, "X", null), N_, d, _p(p, "y", null), _p(p, "Z", null), _p(p, "b", null), n]


def _nlogmarginal(p, N_=N, d=D, n=NF, lh=D + 2, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_nlogmarginal(*_head(p, N_, d, n, null), _p(p, "h", null), lh, 1,
                                            _p(p, "val", null), _p(p, "grad", null))


def _predict(p, N_=N, d=D, n=NF, lh=D + 2, nt=NT, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_predict(*_head(p, N_, d, n, null), _p(p, "h", null), lh,
                                       _p(p, "Xt", null), nt, _p(p, "yt", null), _p(p, "fmu", null),
                                       _p(p, "fs2", null), _p(p, "lp", null))


def _draw(p, N_=N, d=D, n=NF, lh=D + 2, s=S, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_draw_theta(*_head(p, N_, d, n, null), _p(p, "h", null), lh, s, 7,
                                          None, _p(p, "theta", null))


def _create(p, N_=N, d=D, n=NF, **null):
    from gpt_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().gpt_nlml_create(*_head(p, N_, d, n, null), C.byref(h))
    assert h.value is None
    return rc


def _kerr(p, N_=N, d=D, n=NF, lh=D + 2, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_rff_kernel_error(_p(p, "X", null), N_, d, _p(p, "Z", null),
                                           _p(p, "b", null), n, _p(p, "h", null), lh,
                                           _p(p, "out3", null))


def _fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert text in str(ei.value), (text, str(ei.value))


ONE_SHOTS = [_nlogmarginal, _predict, _draw]
ONE_SHOT_IDS = ["nlogmarginal", "predict", "draw_theta"]
_ids = lambda v: "-".join("%s=%s" % kv for kv in v[0].items()) if isinstance(v, tuple) else None
BAD_DIMS = [(dict(n=1025), "nlml: n must be in 1..1024"), (dict(n=0), "nlml: n must be in 1..1024"),
            (dict(N_=0), "nlml: N must be in 1..2^31-1"),
            (dict(N_=2 ** 31), "nlml: N must be in 1..2^31-1"),
            (dict(d=17), "nlml: D must be in 1..16"), (dict(d=0), "nlml: D must be in 1..16"),
            (dict(X=True), "nlml: null input array"), (dict(y=True), "nlml: null input array"),
            (dict(Z=True), "nlml: null input array"), (dict(b=True), "nlml: null input array")]
BAD_HYPER = [(dict(lh=4), "nlml: hyperparams must have 3 or D + 2 entries"),
             (dict(lh=2), "nlml: hyperparams must have 3 or D + 2 entries"),
             (dict(lh=D + 3), "nlml: hyperparams must have 3 or D + 2 entries"),
             (dict(h=True), "nlml: null hyperparams")]


@pytest.mark.parametrize("call", ONE_SHOTS + [_create], ids=ONE_SHOT_IDS + ["create"])
@pytest.mark.parametrize("bad", BAD_DIMS, ids=_ids)
def test_bad_dimensions_fail_without_a_device(call, bad):
    _fails(call(_problem(), **bad[0]), bad[1])


@pytest.mark.parametrize("call", ONE_SHOTS + [_kerr], ids=ONE_SHOT_IDS + ["kernel_error"])
@pytest.mark.parametrize("bad", BAD_HYPER, ids=_ids)
def test_bad_hyper_vector_fails_without_a_device(call, bad):
    _fails(call(_problem(), **bad[0]), bad[1])


@pytest.mark.parametrize("call", ONE_SHOTS + [_kerr], ids=ONE_SHOT_IDS + ["kernel_error"])
@pytest.mark.parametrize("value", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("k", range(D + 2))
def test_bad_hyper_values_fail_without_a_device(call, value, k):
    p = _problem()
    p["h"][k] = value
    _fails(call(p), "nlml: hyperparams must be positive and finite")
    if k < 3:                                            # the iso form's three entries
        p["h"] = np.array([1.0, 0.9, 0.04])
        p["h"][k] = value
        _fails(call(p, lh=3), "nlml: hyperparams must be positive and finite")


def test_one_shot_outputs_and_test_arguments_fail_without_a_device():
    p = _problem()
    _fails(_nlogmarginal(p, val=True), "nlml: null output")
    _fails(_nlogmarginal(p, grad=True), "nlml: null output")
    for name in ("Xt", "fmu", "fs2"):
        _fails(_predict(p, **{name: True}), "nlml: null test input or output")
    _fails(_predict(p, yt=True), "nlml: lp needs ytest")
    for nt in (0, -2, 2 ** 31):
        _fails(_predict(p, nt=nt), "nlml: Ntest must be in 1..2^31-1")
    for s in (0, -1, 4097):
        _fails(_draw(p, s=s), "nlml draw: S must be in 1..4096")
    _fails(_draw(p, theta=True), "nlml draw: null output")


def test_handle_entries_fail_without_a_device():
    from gpt_amd import _lib
    lib, P = _lib.lib(), _lib.P_D
    p = _problem()
    q = lambda name: p[name].ctypes.data_as(P)
    _fails(lib.gpt_nlml_create(q("X"), N, D, q("y"), q("Z"), q("b"), NF, None),
           "nlml: null handle pointer")
    _fails(lib.gpt_nlml_eval(HANDLE, q("h"), D + 2, 0, q("val"), None, None),
           "nlml: null handle or output")
    _fails(lib.gpt_nlml_eval_timed(HANDLE, q("h"), D + 2, 0, q("val"), None, q("ms")),
           "nlml: null handle or output")
    _fails(lib.gpt_nlml_eval_timed(HANDLE, q("h"), D + 2, 0, q("val"), None, None),
           "nlml: null phase_ms")
    _fails(lib.gpt_nlml_features(HANDLE, q("fmu"), None), "nlml: null handle or output")
    _fails(lib.gpt_nlml_predict(HANDLE, q("h"), D + 2, q("Xt"), NT, None, 0, q("fmu"), q("fs2"),
                                None), "nlml: null handle")
    for s in (0, -1, 4097):
        _fails(lib.gpt_nlml_draw_theta(HANDLE, q("h"), D + 2, s, 7, None, q("theta"), None),
               "nlml draw: S must be in 1..4096")
    _fails(lib.gpt_nlml_draw_theta(HANDLE, q("h"), D + 2, S, 7, None, q("theta"), None),
           "nlml draw: null handle or output")
    assert lib.gpt_nlml_destroy(None) == _lib.GPT_OK


KERR_BAD = [(dict(X=True), "rff_kernel_error: null argument"),
            (dict(Z=True), "rff_kernel_error: null argument"),
            (dict(b=True), "rff_kernel_error: null argument"),
            (dict(out3=True), "rff_kernel_error: null argument"),
            (dict(n=0), "rff_kernel_error: n must be in 1..8192"),
            (dict(n=8193), "rff_kernel_error: n must be in 1..8192"),
            (dict(N_=0), "rff_kernel_error: N must be in 1..65536"),
            (dict(N_=65537), "rff_kernel_error: N must be in 1..65536"),
            (dict(d=0), "rff_kernel_error: D must be in 1..16"),
            (dict(d=17), "rff_kernel_error: D must be in 1..16"),
            (dict(n=8192, N_=65536), "rff_kernel_error: phi (n x N doubles) must not exceed 2 GiB")]


@pytest.mark.parametrize("bad", KERR_BAD, ids=_ids)
def test_kernel_error_arguments_fail_without_a_device(bad):
    _fails(_kerr(_problem(), **bad[0]), bad[1])


def test_python_wrappers_raise_without_a_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    p = _problem()
    with pytest.raises(GPTError) as ei:
        G.NoTensorMarginal(np.zeros((3, 17)), np.zeros(3), np.zeros((2, 17)), np.zeros(2))
    assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(ValueError):
        G.NoTensorMarginal(p["X"], p["y"][:-1], p["Z"], p["b"])
    with pytest.raises(GPTError):
        G.gpnt_nlogmarginal_oneshot(p["X"], p["y"], p["Z"], p["b"], [1.0, 1.0, 0.9, 0.04])
    with pytest.raises(GPTError) as ei:                   # a GPTError, not ExactGP's ValueError
        G.gpnt_predict_oneshot(p["X"], p["y"], p["Z"], p["b"], p["h"], p["Xt"][:, :2])
    assert ei.value.code == GPT_ERR_BAD_DIMS and not isinstance(ei.value, ValueError)
    for name in ("nlogmarginal", "gradnlogmarginal", "value_and_grad", "theta_mean", "features",
                 "predict", "draw_theta", "close"):
        assert callable(getattr(G.NoTensorMarginal, name)), name


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
    for s in ("gpt_gpnt_nlogmarginal", "gpt_gpnt_predict", "gpt_gpnt_draw_theta",
              "gpt_rff_kernel_error"):
        assert calls.get(s) == "GPT_SGLD_HIP.jl", s
