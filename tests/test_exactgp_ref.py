"""CPU tests of the exact-GP restatements (tests/exactgp_ref.py) against the golden
tests/golden/exactgp_mp.npz: the two fp64 forms agree with it to within each other's error, the
gradient is the derivative of the value, and GPkit's log-space relation holds."""
import numpy as np
import pytest

import exactgp_ref as ER

FLOOR = 1e-12
SMALL = [c for c in ER.CASES if c[0] <= ER.MP_MAX_N]


@pytest.fixture(scope="module")
def golden():
    return ER.load_golden()


def test_golden_is_complete(golden):
    z = np.load(ER.GOLDEN)
    assert float(z["ld_vs_mp"]) <= 1e-14
    for case in ER.CASES:
        g = golden[ER.case_name(case)]
        N, D, Lh, Nt = case
        assert g["X"].shape == (N, D) and g["Xtest"].shape == (Nt, D) and g["H"].shape == (3, Lh)
        assert (np.abs(g["val"]) >= 1.0).all()
        X, y, Xt, yt = ER.case_inputs(case, ER.CASES.index(case))
        assert np.array_equal(X, g["X"]) and np.array_equal(yt, g["ytest"])
        assert np.array_equal(g["H"], np.stack(ER.hyper_points(D, Lh)))


@pytest.mark.parametrize("case", ER.CASES, ids=ER.case_name)
def test_restatements_agree_with_the_golden(golden, case):
    g = golden[ER.case_name(case)]
    for p in range(3):
        _, e1, e2 = ER.yardstick(g, p)
        for q in ER.QUANT:
            assert (e1[q] <= np.maximum(32 * e2[q], FLOOR)).all(), (p, q, e1[q], e2[q])
            assert (e2[q] <= np.maximum(32 * e1[q], FLOOR)).all(), (p, q, e1[q], e2[q])


@pytest.mark.parametrize("case", SMALL, ids=ER.case_name)
def test_gradient_is_the_derivative_of_the_value(golden, case):
    g = golden[ER.case_name(case)]
    for p in range(3):
        h = g["H"][p]
        grad = ER.fused(g["X"], g["y"], h).grad
        fd = ER.central_diff(lambda hh: ER.literal(g["X"], g["y"], hh).val, h)
        # relative to the largest component: the difference quotient's own rounding error,
        # eps |value| / step, is absolute and exceeds 1e-6 of the smallest components at D = 16
        assert np.abs(grad - fd).max() <= 1e-6 * np.abs(grad).max(), (p, grad, fd)


@pytest.mark.parametrize("case", SMALL[1:7], ids=ER.case_name)
def test_gpkit_log_space_relation(golden, case):
    """dnlZ = grad * [l..., sigma_RBF, 2 signal_var] is the derivative with respect to
    [log l; log sigma_RBF; log sqrt(signal_var)]."""
    g = golden[ER.case_name(case)]
    h = g["H"][1]
    lh = np.log(h)
    lh[-1] = 0.5 * np.log(h[-1])
    dn = ER.dnlz_log(ER.literal(g["X"], g["y"], h).grad, h)
    fd = np.empty(h.size)
    for k in range(h.size):
        d = 1e-5
        up, dn_ = lh.copy(), lh.copy()
        up[k] += d
        dn_[k] -= d
        fd[k] = (ER.nlz_log(g["X"], g["y"], up, case[1]) - ER.nlz_log(g["X"], g["y"], dn_, case[1])) / (2 * d)
    assert np.abs(dn - fd).max() <= 1e-6 * np.abs(dn).max(), (dn, fd)


@pytest.mark.parametrize("case", SMALL[:8], ids=ER.case_name)
def test_gp_nlogmarginal_signature(golden, case):
    g = golden[ER.case_name(case)]
    for p in range(3):
        h = g["H"][p]
        nl = h.size - 2
        v = ER.GP_nlogmarginal(g["X"], g["y"], h[-1], h[-2] ** 2, h[:nl] if nl > 1 else h[0])
        assert abs(v - g["val"][p]) <= 1e-12 * abs(g["val"][p])
