"""CPU tests of the hyper-parameter learning layer: the fp64 restatements of tests/nlml_ref.py
against the 50-digit golden (tests/golden/nlml_mp.npz), the optimiser wrappers on restatement
callables, and the argument checks of the new entry points that need no device.

Bounds.  A = phi phi' + s2 I has cond(A) <= 1 + 2 sigma_RBF^2 N / s2 (||phi phi'|| <= its trace,
phi^2 <= 2 sigma_RBF^2 / n).  A backward-stable fp64 solve carries a relative error of about
cond(A) eps, and every gradient entry is a sum of terms of the size of the largest entry, so
  |g_k - gold_k| <= 64 cond(A) eps max|gold|   (eps = 2^-53; 64 for the n-term accumulations)
for both restatements; the value, whose terms do not cancel, is held to 1e-12 relative.  The
messages of these assertions carry the measured errors per case and component.
"""
import math

import numpy as np
import pytest

import nlml_ref as NR

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    return NR.load_golden()


def cond_bound(g, h):
    return 1.0 + 2.0 * h[-2] ** 2 * g["y"].size / h[-1]


@pytest.mark.parametrize("case", NR.CASES, ids=NR.case_name)
def test_restatements_match_the_mp_golden(golden, case):
    g = golden[NR.case_name(case)]
    assert g["H"].shape == (3, case[3])
    report = []
    for p in range(3):
        h = g["H"][p]
        args = (g["X"], g["y"], g["Z"], g["b"], h)
        val = NR.nlogmarginal(*args)
        vf, _, _ = NR.value_and_grad_fused(*args)
        _, e_lit, e_fus = NR.yardstick(g, p)
        gold = g["grad"][p]
        assert np.abs(gold).min() >= 1e-4 * np.abs(gold[:-1]).max()
        ev = max(abs(val - g["val"][p]), abs(vf - g["val"][p])) / abs(g["val"][p])
        report.append("point %d: value %.1e, literal %s, fused %s" % (
            p, ev, np.array2string(e_lit, precision=1), np.array2string(e_fus, precision=1)))
        bound = 64 * cond_bound(g, h) * EPS * np.abs(gold).max() / np.abs(gold)
        msg = "%s %s" % (NR.case_name(case), "; ".join(report))
        assert ev <= 1e-12, msg
        assert (e_lit <= bound).all() and (e_fus <= bound).all(), msg
    print("\n".join(report))


@pytest.mark.parametrize("case", NR.CASES, ids=NR.case_name)
def test_value_against_central_differences(golden, case):
    """The golden gradient is the derivative of the value restatement: central differences with
    a relative step 1e-5, bound 1e-5 max|g| truncation plus the rounding of the difference."""
    g = golden[NR.case_name(case)]
    for p in range(3):
        h = g["H"][p]

        def fun(hh):
            return NR.nlogmarginal(g["X"], g["y"], g["Z"], g["b"], hh)
        cd = NR.central_diff(fun, h)
        gold = g["grad"][p]
        tol = 1e-5 * np.abs(gold).max() + 64 * cond_bound(g, h) * EPS * abs(g["val"][p]) / (1e-5 * h)
        assert (np.abs(cd - gold) <= tol).all(), (p, np.abs(cd - gold) / np.abs(gold).max())


def test_log_space_chain_rule():
    """Both optimiser wrappers minimise over log h with the gradient g h: on
    f(h) = sum (log h - a)^2 they must land on h = exp(a)."""
    pytest.importorskip("scipy")
    from gpt_amd import GPT_SGLD as G
    a = np.array([0.3, -1.2, 2.0])
    calls = []

    def f(h):
        calls.append(np.array(h))
        return float(((np.log(h) - a) ** 2).sum())

    def gr(h):
        return 2 * (np.log(h) - a) / h
    for run in (lambda: G.GPNT_hyperparameters_optim(f, gr, [1.0, 1.0, 1.0], 1e-8, 1e-14),
                lambda: G.GPNT_hyperparameters(f, gr, [1.0, 1.0, 1.0], 1e-3, xtol=1e-8, ftol=1e-14)):
        minx, minf = run()
        assert np.abs(np.log(minx) - a).max() < 1e-6 and minf < 1e-11
    assert all((c > 0).all() for c in calls)
    # an active bound: the third entry stops at its lower bound exp(2.5) > exp(a_3)
    lb = [1e-3, 1e-3, math.exp(2.5)]
    minx, _ = G.GPNT_hyperparameters(f, gr, [1.0, 1.0, 20.0], lb, xtol=1e-8, ftol=1e-14)
    assert abs(minx[2] - lb[2]) < 1e-9 * lb[2] and np.abs(np.log(minx[:2]) - a[:2]).max() < 1e-6
    with pytest.raises(ValueError):
        G.GPNT_hyperparameters(f, gr, [1.0, 1.0, 1.0], [0.0, 1e-3, 1e-3])


START = np.array([1.0, 1.0, 1.0, 1.0, 0.2, 0.04])


def test_hyperparameters_on_the_restatement(golden):
    pytest.importorskip("scipy")
    from gpt_amd import GPT_SGLD as G
    g = golden["n40_N203_D4_Lh6"]
    ref = NR.RefMarginal(g["X"], g["y"], g["Z"], g["b"])
    f0 = ref.nlogmarginal(START)
    minx, minf = G.GPNT_hyperparameters(ref.nlogmarginal, ref.gradnlogmarginal, START, 0.001)
    assert minf < f0 and (minx >= 0.001 * (1 - 1e-12)).all()
    assert abs(minf - ref.nlogmarginal(minx)) <= 1e-12 * abs(minf)
    # run to convergence: the projected log-space gradient falls under the gradient tolerance
    minx, minf2 = G.GPNT_hyperparameters(ref.nlogmarginal, ref.gradnlogmarginal, START, 0.001,
                                         xtol=1e-5, ftol=1e-15)
    gl = ref.gradnlogmarginal(minx) * minx
    at_bound = (minx <= 0.001 * (1 + 1e-9)) & (gl > 0)
    assert minf2 <= minf and (minx >= 0.001 * (1 - 1e-12)).all()
    assert np.abs(gl[~at_bound]).max() <= 1e-3 * max(1.0, abs(minf2)), gl


def test_wrappers_reject_other_objects():
    from gpt_amd import GPT_SGLD as G
    h = [1.0, 0.9, 0.04]
    with pytest.raises(TypeError):
        G.GPNT_nlogmarginal(np.zeros(4), 3, h, lambda hh: None)
    with pytest.raises(TypeError):
        G.GPNT_gradnlogmarginal(np.zeros(4), 3, h, object(), object())


def test_bad_arguments_fail_without_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    rng = np.random.default_rng(0)

    def code(n, N, D, h):
        X, y = rng.standard_normal((N, D)), rng.standard_normal(N)
        Z, b = rng.standard_normal((n, D)), rng.random(n)
        with pytest.raises(_lib.GPTError) as ei:
            G.gpnt_nlogmarginal_oneshot(X, y, Z, b, h)
        return ei.value.code
    good = [1.0, 1.0, 0.9, 0.04]
    assert code(1025, 8, 2, good) == _lib.GPT_ERR_BAD_DIMS            # n > 1024
    assert code(4, 8, 17, [1.0, 0.9, 0.04]) == _lib.GPT_ERR_BAD_DIMS  # D > 16
    assert code(4, 8, 2, [1.0, 1.0, 1.0, 0.9, 0.04]) == _lib.GPT_ERR_BAD_DIMS   # Lh not 3 or D + 2
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for k in range(4):
            h = list(good)
            h[k] = bad
            assert code(4, 8, 2, h) == _lib.GPT_ERR_BAD_DIMS
    handle = _lib.C.c_void_p()
    X, Z = np.zeros((8, 2), order="F"), np.zeros((1025, 2), order="F")
    rc = _lib.lib().gpt_nlml_create(X.ctypes.data_as(_lib.P_D), 8, 2, X.ctypes.data_as(_lib.P_D),
                                    Z.ctypes.data_as(_lib.P_D), Z.ctypes.data_as(_lib.P_D), 1025,
                                    _lib.C.byref(handle))
    assert rc == _lib.GPT_ERR_BAD_DIMS and not handle.value
