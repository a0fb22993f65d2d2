"""GPU tests of exact GP regression on the device (gpt_amd/csrc/exactgp.hip) against the golden
tests/golden/exactgp_mp.npz (50-digit mpmath up to N = 259, long double above) and the fp64
restatements of tests/exactgp_ref.py.

Parity rule (tests/test_gpu_nlml.py's): for each quantity the yardstick is the larger error of the
two fp64 restatements against the golden, and the device's error may be at most
max(32 x yardstick, 1e-12).  Value: relative; gradient: per component, relative; fmu: over
max|fmu|; fs2 and ys2: over sigma_RBF^2; lp: over max|lp|.  alpha is held to 1e-9 of max|alpha|
against the literal restatement (test_theta_mean's bar).
"""
import os
import sys

import numpy as np
import pytest

import exactgp_ref as ER

pytestmark = pytest.mark.gpu

FLOOR = 1e-12


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@pytest.fixture(scope="module")
def golden():
    return ER.load_golden()


_YARD = {}


def yard(golden, nm, p):
    if (nm, p) not in _YARD:
        _YARD[(nm, p)] = ER.yardstick(golden[nm], p)[0]
    return _YARD[(nm, p)]


def device_result(gp, g, h):
    val, grad = gp.value_and_grad(h)
    pr = gp.predict(h, g["Xtest"], g["ytest"])
    assert pr.ymu is pr.fmu or np.array_equal(pr.ymu, pr.fmu)
    assert np.array_equal(pr.ys2, pr.fs2 + h[-1])
    return ER.Result(val, grad, None, pr.fmu, pr.fs2, pr.lp)


def check_parity(res, gold, yd, h, tag):
    err = ER.errors(res, gold, h)
    for q in ER.QUANT:
        bound = np.maximum(32 * yd[q], FLOOR)
        print("%s %-4s error %.2e, yardstick %.2e, worst error/bound %.3f"
              % (tag, q, np.max(err[q]), np.max(yd[q]), np.max(err[q] / bound)))
    for q in ER.QUANT:
        assert (err[q] <= np.maximum(32 * yd[q], FLOOR)).all(), (tag, q, err[q], yd[q])


@pytest.mark.parametrize("case", ER.CASES, ids=ER.case_name)
def test_parity(golden, case):
    nm = ER.case_name(case)
    g = golden[nm]
    gp = G().ExactGP(g["X"], g["y"])
    for p in range(3):
        h = g["H"][p]
        res = device_result(gp, g, h)
        check_parity(res, ER.point(g, p), yard(golden, nm, p), h, "%s point %d" % (nm, p))
        want = ER.literal(g["X"], g["y"], h).alpha
        got = gp.alpha(h)
        ea = np.abs(got - want).max() / np.abs(want).max()
        print("%s point %d alpha error %.2e" % (nm, p, ea))
        assert ea <= 1e-9
        nl = h.size - 2
        v = G().GP_nlogmarginal(g["X"], g["y"], h[-1], h[-2] ** 2, h[:nl] if nl > 1 else h[0])
        assert abs(v - res.val) <= 1e-12 * abs(res.val)      # sqrt(sigma^2) may differ by an ulp
    gp.close()


BITS = ["N33_D2_Lh4_T33", "N130_D4_Lh3_T64", "N259_D8_Lh10_T100", "N1100_D4_Lh6_T300"]


@pytest.mark.parametrize("nm", BITS)
def test_determinism_and_one_shot(golden, nm):
    g = golden[nm]
    gp = G().ExactGP(g["X"], g["y"])
    h = g["H"][1]
    v1, g1 = gp.value_and_grad(h)
    a1 = gp.alpha(h)
    gp.value_and_grad(g["H"][0])                     # other work on the handle in between
    v2, g2 = gp.value_and_grad(h)
    assert v1 == v2 and np.array_equal(g1, g2) and np.array_equal(a1, gp.alpha(h))
    v3, g3 = G().gp_nlogmarginal_oneshot(g["X"], g["y"], h)
    assert v1 == v3 and np.array_equal(g1, g3)
    assert gp.nlogmarginal(h) == v1                  # value-only: the same bits
    assert G().gp_nlogmarginal_oneshot(g["X"], g["y"], h, want_grad=False) == v1


@pytest.mark.parametrize("nm", ["N259_D8_Lh10_T100", "N1100_D4_Lh6_T300"])
def test_prediction_does_not_depend_on_the_chunking(golden, nm):
    g = golden[nm]
    h = g["H"][1]
    Nt = g["Xtest"].shape[0]
    gp = G().ExactGP(g["X"], g["y"])
    base = gp.predict(h, g["Xtest"], g["ytest"], chunk=Nt)          # predict alone: it fits
    for chunk in (64, 17, None):
        pr = gp.predict(h, g["Xtest"], g["ytest"], chunk=chunk)
        for a, b in zip(base, pr):
            assert np.array_equal(a, b), chunk
    gp2 = G().ExactGP(g["X"], g["y"])
    gp2.value_and_grad(h)                                           # predict right after eval
    pr = gp2.predict(h, g["Xtest"], g["ytest"], chunk=Nt)
    for a, b in zip(base, pr):
        assert np.array_equal(a, b)
    one = G().gp_predict_oneshot(g["X"], g["y"], h, g["Xtest"], g["ytest"])
    for a, b in zip(base, one):
        assert np.array_equal(a, b)
    nolp = gp.predict(h, g["Xtest"])
    assert nolp.lp is None and np.array_equal(nolp.fmu, base.fmu) and np.array_equal(nolp.fs2, base.fs2)


def test_failed_factorisation_is_a_status(golden):
    """X = 0 makes every K_ij = 1, and 1 + 1e-20 = 1: the second pivot is exactly 1 - 1 = 0."""
    from gpt_amd import _lib
    X = np.zeros((8, 2), order="F")
    y = np.arange(8.0)
    h = np.array([1.0, 1.0, 1.0, 1e-20])
    gp = G().ExactGP(X, y)
    with pytest.raises(_lib.GPTError) as ei:
        gp.value_and_grad(h)
    assert ei.value.code == _lib.GPT_ERR_NOT_SPD
    P = _lib.P_D
    val = _lib.C.c_double(1.0)
    grad, alpha = np.ones(4), np.ones(8)
    rc = _lib.lib().gpt_egp_eval(gp._h, h.ctypes.data_as(P), 4, 1, _lib.C.byref(val),
                                 grad.ctypes.data_as(P), alpha.ctypes.data_as(P))
    assert rc == _lib.GPT_ERR_NOT_SPD
    assert np.isnan(val.value) and np.isnan(grad).all() and np.isnan(alpha).all()
    Xt = np.zeros((3, 2), order="F")
    fmu, fs2, lp = np.ones(3), np.ones(3), np.ones(3)
    rc = _lib.lib().gpt_egp_predict(gp._h, h.ctypes.data_as(P), 4, Xt.ctypes.data_as(P), 3,
                                    y.ctypes.data_as(P), 0, fmu.ctypes.data_as(P),
                                    fs2.ctypes.data_as(P), lp.ctypes.data_as(P))
    assert rc == _lib.GPT_ERR_NOT_SPD
    assert np.isnan(fmu).all() and np.isnan(fs2).all() and np.isnan(lp).all()
    # the handle stays usable: the next evaluation on it passes the parity rule, measured against
    # the long-double evaluation of that point (the length-scale derivatives are exactly zero)
    with pytest.raises(_lib.GPTError) as ei:
        gp.value_and_grad(np.array([1.0, 1.0, 1.0, float("nan")]))
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    sys.path.insert(0, os.path.dirname(ER.GOLDEN))
    from make_exactgp_golden import ld_eval
    hg = np.array([1.0, 1.0, 1.0, 0.5])
    yt = np.array([0.5, -1.0, 2.0])
    ld = [np.asarray(a, dtype=np.float64) for a in ld_eval(X, y, hg, Xt, yt)]
    g = dict(X=X, y=y, Xtest=Xt, ytest=yt, H=hg[None, :], val=ld[0][None], grad=ld[1][None],
             fmu=ld[2][None], fs2=ld[3][None], lp=ld[4][None])
    res = device_result(gp, g, hg)
    assert (res.grad[:2] == 0.0).all()
    check_parity(res, ER.point(g, 0), ER.yardstick(g, 0)[0], hg, "after a failure")


def test_optimiser_on_the_device(golden):
    """GPNT_hyperparameters driven by the device object and by the restatement (optinf's
    counterpart); the gradient at the device's end point against its long-double evaluation."""
    pytest.importorskip("scipy")
    nm = "N130_D4_Lh6_T64"
    g = golden[nm]
    start = np.array([1.0, 1.0, 1.0, 1.0, 0.5, 0.1])
    gp = G().ExactGP(g["X"], g["y"])
    ref = ER.RefExact(g["X"], g["y"])
    kw = dict(xtol=1e-9, ftol=1e-12)
    dx, df = G().GPNT_hyperparameters(gp.nlogmarginal, gp.gradnlogmarginal, start, 1e-4, **kw)
    cx, cf = G().GPNT_hyperparameters(ref.nlogmarginal, ref.gradnlogmarginal, start, 1e-4, **kw)
    print("device: nlml %.9f at %s; restatement: %.9f at %s" % (df, dx, cf, cx))
    assert df < gp.nlogmarginal(start)
    assert abs(df - cf) <= 1e-6 * abs(cf)
    sys.path.insert(0, os.path.dirname(ER.GOLDEN))
    from make_exactgp_golden import ld_eval
    ld = [np.asarray(a, dtype=np.float64) for a in ld_eval(g["X"], g["y"], dx, g["Xtest"], g["ytest"])]
    here = dict(g, H=dx[None, :], val=ld[0][None], grad=ld[1][None], fmu=ld[2][None],
                fs2=ld[3][None], lp=ld[4][None])
    res = device_result(gp, g, dx)
    check_parity(res, ER.point(here, 0), ER.yardstick(here, 0)[0], dx, "optimiser result")
