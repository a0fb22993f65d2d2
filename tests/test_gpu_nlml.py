"""GPU tests of the device marginal likelihood and gradient (gpt_amd/csrc/nlml.hip) against the
50-digit golden tests/golden/nlml_mp.npz and the fp64 restatements of tests/nlml_ref.py.

Parity rule (per gradient component): the device's relative error against the mp value is at
most 32 x the larger of the two fp64 restatements' errors against mp for that component, with a
floor of 1e-12.  The factor 32 covers the different summation order of the MFMA K loop and of
the blocked Cholesky (O(log2 n · eps) effects on the same conditioning); the yardstick is the
restatement's own error, never the device's.  The value is held to 1e-12 relative.
"""
import os
import sys

import numpy as np
import pytest

import nlml_ref as NR

pytestmark = pytest.mark.gpu

FLOOR = 1e-12


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@pytest.fixture(scope="module")
def golden():
    return NR.load_golden()


@pytest.fixture(scope="module")
def yard(golden):
    return {(nm, p): NR.yardstick(g, p)[0] for nm, g in golden.items() for p in range(3)}


def marginal(g):
    return G().NoTensorMarginal(g["X"], g["y"], g["Z"], g["b"])


def check_parity(val, grad, gold_val, gold_grad, yard_k, tag):
    ev, eg = NR.rel_errors(val, grad, gold_val, gold_grad)
    bound = np.maximum(32 * yard_k, FLOOR)
    ratio = eg / bound
    print("%s: value %.2e; worst component error %.2e, worst error/bound %.3f"
          % (tag, ev, eg.max(), ratio.max()))
    assert ev <= 1e-12, (tag, ev)
    assert (eg <= bound).all(), (tag, eg, bound)


@pytest.mark.parametrize("case", NR.CASES, ids=NR.case_name)
def test_value_and_gradient_parity(golden, yard, case):
    nm = NR.case_name(case)
    g = golden[nm]
    m = marginal(g)
    for p in range(3):
        val, grad = m.value_and_grad(g["H"][p])
        check_parity(val, grad, g["val"][p], g["grad"][p], yard[(nm, p)], "%s point %d" % (nm, p))
        assert np.array_equal(np.array(G().GPNT_gradnlogmarginal(g["y"], case[0], g["H"][p], m, m)),
                              grad)
        assert G().GPNT_nlogmarginal(g["y"], case[0], g["H"][p], m) == val
    m.close()


@pytest.mark.parametrize("nm", ["n33_N130_D2_Lh4", "n100_N517_D4_Lh3", "n65_N1030_D16_Lh18"])
def test_features_equal_feature_notensor(golden, nm):
    g = golden[nm]
    m = marginal(g)
    h = g["H"][1]
    m.value_and_grad(h)
    phi, S = m.features(sin=True)
    D = g["X"].shape[1]
    ls = h[:D] if h.size == D + 2 else h[0]
    want = G().featureNotensor(g["X"], ls, h[-2], g["Z"], g["b"])
    assert np.array_equal(phi, want)
    c2 = 2.0 / g["Z"].shape[0] * h[-2] ** 2
    assert np.abs(phi ** 2 + S ** 2 - c2).max() <= 1e-14 * c2
    m.nlogmarginal(h)
    assert np.array_equal(m.features(), want)


@pytest.mark.parametrize("nm", ["n40_N203_D4_Lh6", "n48_N30_D3_Lh5", "n128_N259_D8_Lh10"])
def test_theta_mean(golden, nm):
    g = golden[nm]
    m = marginal(g)
    for p in range(3):
        h = g["H"][p]
        ls, sigma, s2 = NR.split(h, g["X"].shape[1])
        phi = NR.feature_notensor(g["X"], ls, sigma, g["Z"], g["b"])
        want = np.linalg.solve(phi @ phi.T + s2 * np.eye(phi.shape[0]), phi @ g["y"])
        got = m.theta_mean(h)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("nm", ["n33_N130_D2_Lh4", "n65_N1030_D16_Lh18", "n100_N517_D4_Lh3"])
def test_determinism_and_one_shot(golden, nm):
    g = golden[nm]
    m = marginal(g)
    h = g["H"][1]
    v1, g1 = m.value_and_grad(h)
    m.value_and_grad(g["H"][0])                      # other work on the handle in between
    v2, g2 = m.value_and_grad(h)
    assert v1 == v2 and np.array_equal(g1, g2)
    v3, g3 = G().gpnt_nlogmarginal_oneshot(g["X"], g["y"], g["Z"], g["b"], h)
    assert v1 == v3 and np.array_equal(g1, g3)
    # value-only evaluations: the same nlml bits
    assert m.nlogmarginal(h) == v1
    assert G().gpnt_nlogmarginal_oneshot(g["X"], g["y"], g["Z"], g["b"], h, want_grad=False) == v1


def test_size_limit():
    """n = 1024 (the blocked Cholesky's limit) with N = 80, against the fused fp64 restatement
    under the parity rule with the restatement's error taken as 1e-10; n = 1025 is rejected."""
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    rng = np.random.default_rng(5)
    n, N, D = 1024, 80, 3
    X, y = rng.standard_normal((N, D)), rng.standard_normal(N)
    Z, b = rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    h = np.array([1.0, 1.0, 1.0, 0.9, 0.04])
    val, grad = G().NoTensorMarginal(X, y, Z, b).value_and_grad(h)
    rv, rg, _ = NR.value_and_grad_fused(X, y, Z, b, h)
    assert np.abs(rg).min() >= 1e-4 * np.abs(rg[:-1]).max()
    err = np.abs(grad - rg) / np.abs(rg)
    print("n = 1024: value %.2e, gradient %s" % (abs(val - rv) / abs(rv), err))
    assert abs(val - rv) <= 1e-12 * abs(rv)
    assert (err <= 32 * 1e-10).all(), err
    with pytest.raises(GPTError) as ei:
        G().NoTensorMarginal(X, y, rng.standard_normal((1025, D)), rng.random(1025))
    assert ei.value.code == GPT_ERR_BAD_DIMS


def test_bad_hyperparameters_rejected(golden):
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    g = golden["n33_N130_D2_Lh4"]
    m = marginal(g)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        for k in range(4):
            h = g["H"][0].copy()
            h[k] = bad
            with pytest.raises(GPTError) as ei:
                m.value_and_grad(h)
            assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(GPTError):
        m.nlogmarginal([1.0, 1.0, 1.0, 0.9, 0.04])    # Lh = 5 with D = 2
    val, _ = m.value_and_grad(g["H"][0])              # the handle still works
    assert abs(val - g["val"][0]) <= 1e-12 * abs(g["val"][0])


def test_nan_input_is_a_status_not_a_fault(golden):
    """A NaN in X fails the Cholesky's pivot test: GPT_ERR_NOT_SPD, NaN outputs, and the next
    evaluation on a fresh handle is good."""
    from gpt_amd import _lib
    g = golden["n40_N203_D4_Lh6"]
    X = np.asfortranarray(g["X"].copy())
    X[7, 2] = np.nan
    N, D = X.shape
    n = g["Z"].shape[0]
    y, Z, b = (np.asfortranarray(g[k]) for k in ("y", "Z", "b"))
    h = np.ascontiguousarray(g["H"][0])
    P = _lib.P_D
    lib = _lib.lib()
    for want_grad in (1, 0):
        handle = _lib.C.c_void_p()
        assert lib.gpt_nlml_create(X.ctypes.data_as(P), N, D, y.ctypes.data_as(P),
                                   Z.ctypes.data_as(P), b.ctypes.data_as(P), n,
                                   _lib.C.byref(handle)) == _lib.GPT_OK
        val = _lib.C.c_double(1.0)
        grad, theta = np.ones(h.size), np.ones(n)
        rc = lib.gpt_nlml_eval(handle, h.ctypes.data_as(P), h.size, want_grad, _lib.C.byref(val),
                               grad.ctypes.data_as(P), theta.ctypes.data_as(P))
        assert rc == _lib.GPT_ERR_NOT_SPD
        assert np.isnan(val.value) and np.isnan(theta).all()
        assert np.isnan(grad).all() if want_grad else (grad == 1.0).all()
        assert lib.gpt_nlml_destroy(handle) == _lib.GPT_OK
    val = np.array([1.0])
    grad = np.ones(h.size)
    rc = lib.gpt_gpnt_nlogmarginal(X.ctypes.data_as(P), N, D, y.ctypes.data_as(P),
                                   Z.ctypes.data_as(P), b.ctypes.data_as(P), n,
                                   h.ctypes.data_as(P), h.size, 1, val.ctypes.data_as(P),
                                   grad.ctypes.data_as(P))
    assert rc == _lib.GPT_ERR_NOT_SPD and np.isnan(val[0]) and np.isnan(grad).all()
    good, gg = marginal(g).value_and_grad(h)
    assert abs(good - g["val"][0]) <= 1e-12 * abs(g["val"][0]) and np.isfinite(gg).all()


def test_optimiser_on_the_device(golden):
    pytest.importorskip("scipy")
    g = golden["n40_N203_D4_Lh6"]
    start = np.array([1.0, 1.0, 1.0, 1.0, 0.2, 0.04])
    ftol = 1e-3
    m = marginal(g)
    ref = NR.RefMarginal(g["X"], g["y"], g["Z"], g["b"])
    f0 = m.nlogmarginal(start)
    dx, df = G().GPNT_hyperparameters(m.nlogmarginal, m.gradnlogmarginal, start, 0.001, ftol=ftol)
    cx, cf = G().GPNT_hyperparameters(ref.nlogmarginal, ref.gradnlogmarginal, start, 0.001, ftol=ftol)
    print("device: nlml %.6f at %s; restatement: %.6f at %s" % (df, dx, cf, cx))
    assert df < f0
    assert df <= cf + 10 * ftol * max(1.0, abs(cf))
    assert (dx >= 0.001 * (1 - 1e-12)).all()
    # the parity rule at the result: its mp value is computed here (about 3 s at this size),
    # since the point depends on the run
    sys.path.insert(0, os.path.dirname(NR.GOLDEN))
    from make_nlml_golden import mp_value_grad
    mv, mg = mp_value_grad(g["X"], g["y"], g["Z"], g["b"], dx)
    here = dict(g, H=dx[None, :], val=np.array([mv]), grad=mg[None, :])
    val, got = m.value_and_grad(dx)
    check_parity(val, got, mv, mg, NR.yardstick(here, 0)[0], "optimiser result")
