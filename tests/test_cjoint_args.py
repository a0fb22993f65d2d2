"""CPU tests of the softmax-joint boundary (gpt_cjoint_create and the one-shot forms): every single
bad argument fails with GPT_ERR_BAD_DIMS and its own message before any device call, the header
declares the entries and the library exports them with matching signatures."""
import ctypes as C

import numpy as np
import pytest

try:
    from tests.test_capi import header_functions
    from tests.test_julia_shim import all_calls, header_prototypes
except ImportError:            # a foreign `tests` package on the path: the modules beside this one
    from test_capi import header_functions
    from test_julia_shim import all_calls, header_prototypes

SYMS = ["gpt_cjoint_create", "gpt_cjoint_eval", "gpt_cjoint_set_theta", "gpt_cjoint_get_theta",
        "gpt_cjoint_steps", "gpt_cjoint_langevin", "gpt_chmc_run", "gpt_chmc_leapfrog",
        "gpt_cjoint_scores", "gpt_cjoint_destroy", "gpt_gpnt_neglogjoint",
        "gpt_gpnt_joint_langevin", "gpt_gpnt_joint_hmc", "gpt_gpnt_joint_scores"]
N, D, NF, NC, NT = 12, 3, 6, 3, 5
HANDLE = C.c_void_p(None)        # no handle exists without a device: the checks that need none run first


def _problem():
    rng = np.random.default_rng(13)
    return dict(X=np.asfortranarray(rng.standard_normal((N, D))),
                y=rng.integers(1, NC + 1, N).astype(np.float64),
                Z=np.asfortranarray(rng.standard_normal((NF, D))), b=rng.random(NF),
                theta=0.1 * rng.standard_normal(NF * NC), h=np.array([1.0, 1.2, 0.8, 0.9]),
                val=np.ones(1), grad=np.ones(NF * NC + D + 1), scores=np.ones(N * NC),
                store=np.ones(NF * NC * 2), acc=np.ones(2, dtype=np.int32), dH=np.ones(2),
                U=np.ones(2))


def _p(p, name, null):
    from gpt_amd import _lib
    return None if null.get(name) else p[name].ctypes.data_as(_lib.P_D)


def _head(p, N_, d, c, n, null):
    return [_p(p, "X", null), N_, d, _p(p, "y", null), c, _p(p, "Z", null), _p(p, "b", null), n]


def _create(p, N_=N, d=D, c=NC, n=NF, **null):
    from gpt_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().gpt_cjoint_create(*_head(p, N_, d, c, n, null), C.byref(h))
    assert h.value is None
    return rc


def _neglogjoint(p, N_=N, d=D, c=NC, n=NF, lh=D + 1, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_neglogjoint(*_head(p, N_, d, c, n, null), _p(p, "theta", null),
                                           _p(p, "h", null), lh, 1, _p(p, "val", null),
                                           _p(p, "grad", null))


def _langevin(p, N_=N, d=D, c=NC, n=NF, lh=D + 1, t0=0, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_joint_langevin(*_head(p, N_, d, c, n, null), _p(p, "theta", null),
                                              _p(p, "h", null), lh, 1e-3, 2, 7, t0)


def _hmc(p, N_=N, d=D, c=NC, n=NF, lh=D + 1, t0=0, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_joint_hmc(*_head(p, N_, d, c, n, null), _p(p, "theta", null),
                                         _p(p, "h", null), lh, 1e-3, 2, 0, 2, 1, 7, t0,
                                         _p(p, "store", null),
                                         p["acc"].ctypes.data_as(_lib.P_I32), _p(p, "dH", null),
                                         _p(p, "U", null), None)


def _scores(p, N_=N, d=D, c=NC, n=NF, lh=D + 1, **null):
    from gpt_amd import _lib
    return _lib.lib().gpt_gpnt_joint_scores(_p(p, "X", null), N_, d, c, _p(p, "Z", null),
                                            _p(p, "b", null), n, _p(p, "theta", null),
                                            _p(p, "h", null), lh, _p(p, "scores", null))


def _fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert text in str(ei.value), (text, str(ei.value))


ONE_SHOTS = [_neglogjoint, _langevin, _hmc, _scores]
ONE_SHOT_IDS = ["neglogjoint", "langevin", "hmc", "scores"]
_ids = lambda v: "-".join("%s=%s" % kv for kv in v[0].items()) if isinstance(v, tuple) else None
BAD_DIMS = [(dict(n=1025), "cjoint: n must be in 1..1024"), (dict(n=0), "cjoint: n must be in 1..1024"),
            (dict(N_=0), "cjoint: N must be in 1..2^31-1"),
            (dict(N_=2 ** 31), "cjoint: N must be in 1..2^31-1"),
            (dict(d=17), "cjoint: D must be in 1..16"), (dict(d=0), "cjoint: D must be in 1..16"),
            (dict(c=0), "cjoint: the number of classes must be in 1..32"),
            (dict(c=33), "cjoint: the number of classes must be in 1..32"),
            (dict(X=True), "cjoint: null input array"), (dict(Z=True), "cjoint: null input array"),
            (dict(b=True), "cjoint: null input array")]
BAD_HYPER = [(dict(lh=3), "cjoint: hyperparams must have 2 or D + 1 entries"),
             (dict(lh=1), "cjoint: hyperparams must have 2 or D + 1 entries"),
             (dict(lh=D + 2), "cjoint: hyperparams must have 2 or D + 1 entries"),
             (dict(h=True), "cjoint: null hyperparams")]


@pytest.mark.parametrize("call", ONE_SHOTS + [_create], ids=ONE_SHOT_IDS + ["create"])
@pytest.mark.parametrize("bad", BAD_DIMS, ids=_ids)
def test_bad_dimensions_fail_without_a_device(call, bad):
    _fails(call(_problem(), **bad[0]), bad[1])


@pytest.mark.parametrize("call", ONE_SHOTS, ids=ONE_SHOT_IDS)
@pytest.mark.parametrize("bad", BAD_HYPER, ids=_ids)
def test_bad_hyper_vector_fails_without_a_device(call, bad):
    _fails(call(_problem(), **bad[0]), bad[1])


@pytest.mark.parametrize("call", ONE_SHOTS, ids=ONE_SHOT_IDS)
@pytest.mark.parametrize("value", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("k", range(D + 1))
def test_bad_hyper_values_fail_without_a_device(call, value, k):
    p = _problem()
    p["h"][k] = value
    _fails(call(p), "cjoint: hyperparams must be positive and finite")
    if k < 2:                                            # the scalar form's two entries
        p["h"] = np.array([1.0, 0.9])
        p["h"][k] = value
        _fails(call(p, lh=2), "cjoint: hyperparams must be positive and finite")


@pytest.mark.parametrize("call", [_create, _neglogjoint, _langevin, _hmc],
                         ids=["create"] + ONE_SHOT_IDS[:3])
@pytest.mark.parametrize("label", [1.5, 0.0, NC + 1.0, -1.0, float("nan")])
def test_bad_labels_fail_without_a_device(call, label):
    p = _problem()
    p["y"][N // 2] = label
    _fails(call(p), "cjoint: labels must be integers in 1..C")


@pytest.mark.parametrize("call", [_create, _neglogjoint, _langevin, _hmc],
                         ids=["create"] + ONE_SHOT_IDS[:3])
def test_null_labels_fail_without_a_device(call):
    _fails(call(_problem(), y=True), "cjoint: null input array")


def test_one_shot_outputs_fail_without_a_device():
    p = _problem()
    for name in ("theta", "val", "grad"):
        _fails(_neglogjoint(p, **{name: True}), "cjoint: null theta or output")
    for call in (_langevin, _hmc):
        _fails(call(p, theta=True), "cjoint: null theta or negative t0")
        _fails(call(p, t0=-1), "cjoint: null theta or negative t0")
    for name in ("theta", "scores"):
        _fails(_scores(p, **{name: True}), "cjoint: null theta or output")


def test_handle_entries_fail_without_a_device():
    from gpt_amd import _lib
    lib, P = _lib.lib(), _lib.P_D
    p = _problem()
    q = lambda name: p[name].ctypes.data_as(P)
    _fails(lib.gpt_cjoint_create(q("X"), N, D, q("y"), NC, q("Z"), q("b"), NF, None),
           "cjoint: null handle pointer")
    _fails(lib.gpt_cjoint_eval(HANDLE, q("h"), D + 1, None, 0, q("val"), None, None),
           "cjoint: null handle or output")
    _fails(lib.gpt_cjoint_set_theta(HANDLE, q("theta")), "cjoint: null handle or theta")
    _fails(lib.gpt_cjoint_get_theta(HANDLE, q("theta")), "cjoint: null handle or output")
    _fails(lib.gpt_cjoint_langevin(HANDLE, q("h"), D + 1, 1e-3, 2, 7, 0), "cjoint: null handle")
    _fails(lib.gpt_chmc_run(HANDLE, q("h"), D + 1, 1e-3, 2, 0, 2, 1, 7, 0, None, None, None, None,
                            None), "cjoint: null handle")
    _fails(lib.gpt_chmc_leapfrog(HANDLE, q("h"), D + 1, 1e-3, 2, q("theta"), None, None),
           "cjoint: null handle or momentum")
    _fails(lib.gpt_cjoint_scores(HANDLE, q("h"), D + 1, q("X"), N, q("scores")),
           "cjoint: bad scores arguments")
    assert lib.gpt_cjoint_destroy(None) == _lib.GPT_OK


def test_python_wrappers_raise_without_a_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    p = _problem()
    with pytest.raises(GPTError) as ei:
        G.SoftmaxJoint(p["X"], p["y"], p["Z"], p["b"], C=33)
    assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(GPTError):
        G.SoftmaxJoint(p["X"], p["y"] + 0.5, p["Z"], p["b"], C=NC)
    with pytest.raises(ValueError):
        G.SoftmaxJoint(p["X"], p["y"][:-1], p["Z"], p["b"])
    with pytest.raises(GPTError):
        G.gpnt_neglogjoint_oneshot(p["X"], p["y"], p["Z"], p["b"], p["theta"], [1.0, 1.0, 0.9], C=NC)
    for name in ("neglogjointlkhd", "gradneglogjointlkhd", "value_and_grad", "hyper_value_and_grad",
                 "theta", "set_theta", "langevin", "hmc", "mala", "leapfrog", "scores", "evaluate",
                 "close"):
        assert callable(getattr(G.SoftmaxJoint, name)), name
    assert isinstance(G.SoftmaxJoint.steps, property)


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
    for s in SYMS[-4:]:
        assert calls.get(s) == "GPT_SGLD_HIP.jl", s
