"""CPU checks of tests/cjoint_ref.py and tests/golden/cjoint_mp.npz: both fp64 restatements of the
softmax joint likelihood against the 50-digit golden, against each other and against central
differences, and the generator's component rule on the stored points."""
import numpy as np
import pytest

import cjoint_ref as CR


@pytest.fixture(scope="module")
def golden():
    return CR.load_golden()


@pytest.mark.parametrize("case", CR.CASES, ids=CR.case_name)
def test_restatements_against_the_golden(golden, case):
    """fp64 against the true value at the same inputs: 1e-13 for the value; for the gradients
    1e-10, which leaves four digits for components up to 1e4 times smaller than the largest (the
    generator's rule) at n*N <= 3e4 summands."""
    g = golden[CR.case_name(case)]
    n, C = g["theta"].shape
    largest = case[5] == "x40"
    for p in range(3):
        args = (g["X"], g["y"], g["Z"], g["b"], g["theta"], g["H"][p])
        assert g["H"][p].size == CR.hyper_len(case)
        lit_v = CR.neglogjoint_literal(*args)
        lit = CR.gradneglogjoint_literal(*args)
        fv, ft, fh = CR.value_and_grad_fused(*args)
        for v in (lit_v, fv):
            assert abs(v - g["val"][p]) <= 1e-13 * abs(g["val"][p])
        for gh in (lit[n * C:], fh):
            assert (CR.hyper_errors(gh, g["gh"][p], largest) <= 1e-10).all()
        for gt in (lit[:n * C].reshape((n, C), order="F"), ft):
            assert CR.theta_error(gt, g["gtheta"][p]) <= 1e-13
        # the fused form against the literal one
        assert abs(fv - lit_v) <= 1e-13 * abs(lit_v)
        assert CR.theta_error(ft, lit[:n * C].reshape((n, C), order="F")) <= 1e-13
        assert (CR.hyper_errors(fh, lit[n * C:], largest) <= 1e-10).all()


def test_component_rule_holds_for_the_stored_points(golden):
    for case in CR.CASES:
        g = golden[CR.case_name(case)]
        for p in range(3):
            assert np.isfinite(g["gh"][p]).all() and np.isfinite(g["gtheta"][p]).all()
            if case[5] != "x40":
                assert CR.component_rule(g["gh"][p]), (case, p, g["gh"][p])


def test_cases_are_what_they_claim(golden):
    for case in CR.CASES:
        n, N, D, C, form, variant = case
        g = golden[CR.case_name(case)]
        assert g["X"].shape == (N, D) and g["Z"].shape == (n, D) and g["theta"].shape == (n, C)
        present = set(g["y"].astype(int))
        if variant == "absent5":
            assert present == set(range(1, C + 1)) - {5}
        else:
            assert present == set(range(1, C + 1))
        if variant == "x40":
            phi = CR.NR.feature_notensor(g["X"], *CR.split(g["H"][0], D), g["Z"], g["b"])
            assert np.abs(g["theta"].T @ phi).max() > 100.0


def test_central_differences(golden):
    case = CR.CASES[1]
    g = golden[CR.case_name(case)]
    n, C = g["theta"].shape
    args = (g["X"], g["y"], g["Z"], g["b"])
    h = g["H"][1]
    _, ft, fh = CR.value_and_grad_fused(*args, g["theta"], h)
    cd = CR.central_diff(lambda x: CR.value_and_grad_fused(*args, g["theta"], x)[0], h)
    assert (np.abs(cd - fh) <= 1e-6 * np.abs(fh).max()).all()
    sel = [0, 7, n * C - 1]
    tv = g["theta"].ravel(order="F")
    for e in sel:
        def f(x):
            t = tv.copy()
            t[e] = x[0]
            return CR.value_and_grad_fused(*args, t.reshape((n, C), order="F"), h)[0]
        cd = CR.central_diff(f, tv[e:e + 1])
        assert abs(cd[0] - ft.ravel(order="F")[e]) <= 1e-6 * np.abs(ft).max()


def test_langevin_restatements_agree(golden):
    """The step with the literal and with the fused gradient: three steps, and a non-zero t0
    draws other noise."""
    g = golden[CR.case_name(CR.CASES[0])]
    args = (g["X"], g["y"], g["Z"], g["b"], g["theta"], g["H"][1], 2e-3, 3, 11)
    a = CR.langevin(*args, t0=0, gradtheta=CR.gradtheta_literal)
    b = CR.langevin(*args, t0=0, gradtheta=CR.gradtheta_fused)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    c = CR.langevin(*args, t0=5)
    assert np.abs(c - b).max() > 1e-3
    one = g["theta"]
    for t in range(3):
        one = CR.langevin(g["X"], g["y"], g["Z"], g["b"], one, g["H"][1], 2e-3, 1, 11, t0=t)
    assert np.array_equal(one, b)
