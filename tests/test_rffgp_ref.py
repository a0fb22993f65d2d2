"""CPU tests of tests/rffgp_ref.py (the fp64 restatements of the RFF GP's closed-form predictive
and of the kernel approximation error) against tests/golden/rffgp_mp.npz, of the golden's own
inputs, and of the new entries' declarations.  Bounds: the predictive restatements are
double-precision Cholesky / LU solves with A, held to n eps cond(A) in the parity measures (the
first-order bound of a backward-stable solve); the kernel-error restatements involve no solve and
are held to the device tests' floor, 1e-12 relative.
"""
import os

import numpy as np
import pytest

import nlml_ref as NR
import rffgp_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return RR.load_golden()


def _solve_bound(g, p):
    """n eps cond(A): the first-order bound of a backward-stable solve with A."""
    n = g["Z"].shape[0]
    ls, sigma, s2 = NR.split(g["H"][p], g["X"].shape[1])
    phi = NR.feature_notensor(g["X"], ls, sigma, g["Z"], g["b"])
    return n * np.finfo(np.float64).eps * np.linalg.cond(phi @ phi.T + s2 * np.eye(n))


def test_golden_inputs_and_size(golden):
    assert os.path.getsize(RR.GOLDEN) < 500 * 1024
    assert float(np.load(RR.GOLDEN)["ld_vs_mp"]) <= 1e-14
    for ci, case in enumerate(RR.CASES):
        g = golden[RR.case_name(case)]
        X, y, Z, b = NR.case_inputs(case, RR.CASE_IDX[ci])
        assert np.array_equal(X, g["X"]) and np.array_equal(y, g["y"])
        assert np.array_equal(Z, g["Z"]) and np.array_equal(b, g["b"])
        Xt, yt = RR.make_test_inputs(X, y, RR.CASE_IDX[ci])
        assert Xt.shape == (RR.NTEST, case[2])
        assert np.array_equal(Xt, g["Xtest"]) and np.array_equal(yt, g["ytest"])
        assert g["fmu"].shape == g["fs2"].shape == g["lp"].shape == (3, RR.NTEST)
        assert g["kerr"].shape == (2, 3)
        assert (g["fs2"] > 0).all() and (g["kerr"] > 0).all()


@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_name)
def test_predictive_restatements_against_golden(golden, case):
    g = golden[RR.case_name(case)]
    for p in range(3):
        yard, e1, e2 = RR.pred_yardstick(g, p)
        print("%s point %d: chol %s, lu %s" % (RR.case_name(case), p, e1, e2))
        bound = _solve_bound(g, p)
        for k in RR.PRED_QUANT:
            assert yard[k] <= bound, (p, k, e1[k], e2[k], bound)
        res = RR.predict_chol(g["X"], g["y"], g["Z"], g["b"], g["H"][p], g["Xtest"], g["ytest"])
        assert np.array_equal(res.ys2, res.fs2 + g["H"][p][-1]) and res.ymu is res.fmu
        assert (res.fs2 > 0).all()
        assert RR.predict_chol(g["X"], g["y"], g["Z"], g["b"], g["H"][p], g["Xtest"]).lp is None


@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_name)
def test_kernel_error_restatements_against_golden(golden, case):
    g = golden[RR.case_name(case)]
    for q in range(len(RR.KERR_POINTS)):
        yard, e1, e2 = RR.kerr_yardstick(g, q)
        print("%s point %d: literal %s, blocked %s" % (RR.case_name(case), RR.KERR_POINTS[q], e1, e2))
        assert (yard <= 1e-12).all(), (q, e1, e2)


@pytest.mark.parametrize("case", [c for c in RR.CASES if c[0] <= c[1]], ids=RR.case_name)
def test_push_through_identity(golden, case):
    """phi*'(phi phi' + s2 I)^-1 phi y = k*'(K_rff + s2 I)^-1 y: the feature-space mean is the
    kernel-space mean of the approximate kernel."""
    g = golden[RR.case_name(case)]
    for p in range(3):
        fmu = g["fmu"][p]
        alt = RR.push_through_mean(g["X"], g["y"], g["Z"], g["b"], g["H"][p], g["Xtest"])
        assert np.abs(alt - fmu).max() <= 1e-8 * np.abs(fmu).max(), (p, np.abs(alt - fmu).max())


def test_kernel_error_small_shapes_agree():
    rng = np.random.default_rng(3)
    for N, n in ((1, 1), (5, 2), (70, 31)):
        X, Z, b = rng.standard_normal((N, 3)), rng.standard_normal((n, 3)), 2 * np.pi * rng.random(n)
        h = np.array([0.8, 1.1, 1.7, 0.9, 0.04])
        a, c = RR.kernel_error_literal(X, Z, b, h), RR.kernel_error_blocked(X, Z, b, h, rows=16)
        assert np.allclose(a, c, rtol=1e-13, atol=0)
    # one point, one feature: K = sigma^2, K_rff = 2 sigma^2 cos^2(b)
    e = RR.kernel_error_literal(np.zeros((1, 1)), np.ones((1, 1)), np.array([0.3]), [1.0, 2.0, 0.1])
    assert abs(e.norm_K - 4.0) <= 1e-15 and abs(e.frob - abs(4.0 - 8.0 * np.cos(0.3) ** 2)) <= 1e-14
    assert e.max_abs == e.frob


def test_new_entries_are_declared():
    from gpt_amd import _lib
    from test_julia_shim import all_calls, header_prototypes
    protos = header_prototypes()
    for name in ("gpt_nlml_predict", "gpt_gpnt_predict", "gpt_rff_kernel_error", "gpt_rff_last_timing"):
        assert name in protos and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(protos[name][1]), name
        assert hasattr(_lib.lib(), name), name
    bound = {c[1] for c in all_calls()}
    assert {"gpt_gpnt_predict", "gpt_rff_kernel_error"} <= bound
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## Julia")[0]
    for name in ("gpt_gpnt_predict", "gpt_rff_kernel_error"):
        assert "`%s`" % name in text, name
