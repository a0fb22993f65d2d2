"""CPU tests of the draw restatements (tests/gpdraw_ref.py) against the mpmath golden
tests/golden/gpdraw_mp.npz, and of createmesh / fhatdraw's host-side contracts.

The bound on the restatements' own error: every quantity goes through a Cholesky factor of a
matrix M + 1e-6 I with |M| <= sigma_RBF^2 N, so its relative error is within a modest multiple of
cond * 2^-53 <= (1.69 * 259 / 1e-6) * 1.1e-16 = 4.9e-8; 1e-6 leaves a factor 20 for the growth
constants.  (The device is not held to this bound but to 32 x the error measured here.)"""
import numpy as np
import pytest

import gpdraw_ref as R

BOUND = 1e-6


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_name(c) for c in R.CASES])
def test_golden_holds_the_cases_inputs(golden, idx):
    g = golden[R.case_name(R.CASES[idx])]
    N, D, Lh, Nt = R.CASES[idx]
    for k, v in R.case_inputs(idx).items():
        assert np.array_equal(g[k], v), k
    assert g["X"].shape == (N, D) and g["Xtest"].shape == (Nt, D) and g["h"].size == Lh
    assert np.array_equal(g["Xtest"][-5:], g["X"][:5])
    assert g["Fprior"].shape == (N, R.S) and g["Fpost"].shape == (Nt, R.S)
    assert ("cov" in g) == (Nt <= R.COV_MAX_NT)
    assert ("theta" in g) == bool(R.RFF_N[idx])
    if R.RFF_N[idx]:
        assert g["theta"].shape == (R.RFF_N[idx], R.S)


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[R.case_name(c) for c in R.CASES])
def test_restatements_against_mpmath(golden, idx):
    g = golden[R.case_name(R.CASES[idx])]
    yd = R.yardstick(g)
    for q, e in yd.items():
        print("%s %-5s restatement error %.2e" % (R.case_name(R.CASES[idx]), q, e))
    assert set(yd) >= {"prior", "fmu", "post"}
    for q, e in yd.items():
        assert e <= BOUND, (q, e)


def test_restatement_columns_are_independent(golden):
    g = golden[R.case_name(R.CASES[0])]
    F = R.prior(g["X"], g["h"], R.JITTER, g["Zprior"])
    F3 = R.prior(g["X"], g["h"], R.JITTER, g["Zprior"][:, 2:3])
    assert np.abs(F[:, 2:3] - F3).max() <= 1e-13 * np.abs(F).max()
    obs = R.posterior(g["X"], g["y"], g["h"], g["Xtest"], R.JITTER, True, g["Zpost"])
    fun = R.posterior(g["X"], g["y"], g["h"], g["Xtest"], R.JITTER, False, g["Zpost"])
    assert np.array_equal(obs.fmu, fun.fmu) and np.array_equal(obs.cov, fun.cov)
    # observations scatter more than function values: the noise variance joins the factor
    assert (obs.F - obs.fmu[:, None]).std() > (fun.F - fun.fmu[:, None]).std()


def test_createmesh_order_and_shape():
    from gpt_amd import GPT_SGLD as G
    x, y, grid = G.createmesh(-1.0, 2.0, 4)
    assert np.array_equal(x, np.linspace(-1.0, 2.0, 4)) and np.array_equal(x, y)
    assert grid.shape == (16, 2)
    k = 0
    for i in range(4):                 # the reference's loop: x outer, y inner
        for j in range(4):
            assert grid[k, 0] == x[i] and grid[k, 1] == y[j]
            k += 1
    x50, _, g50 = G.createmesh(0, 1, 50)
    assert g50.shape == (2500, 2) and g50[49, 1] == 1.0 and g50[50, 0] == x50[1]


def test_fhatdraw_rejects_a_wrong_length_scale_before_any_device_call():
    from gpt_amd import GPT_SGLD as G
    X = np.zeros((7, 3))
    with pytest.raises(ValueError, match="dimensions of X and length_scale do not match"):
        G.fhatdraw(X, 5, [1.0, 2.0], 1.0, 2, 8)
    with pytest.raises(ValueError):
        G.fhatdraw(np.zeros(7), 5, 1.0, 1.0, 2, 8)
