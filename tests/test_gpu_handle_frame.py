"""GPU tests of the frame the resident hyper-parameter handles share (gpt_amd/csrc/gp_handle.h): the
key of the resident factor, its invalidation, and the scratch block that grows on demand, walked on
ExactGP and NoTensorMarginal at the smallest shapes that take every branch.

ExactGP: N = 70, D = 2, Ntest = 9 (two 64-row panels: the blocked Cholesky and egp_trsm's update
run).  NoTensorMarginal: N = 40, D = 2, n = 18 and 17 (the even and the odd V2 route), Ntest = 9.
Every assertion is bitwise equality of results that are the same computation.

Of the transitions of the frame, these are held bitwise elsewhere at comparable shapes and not
repeated here:
  - predict on a fresh handle against value_and_grad then predict:
    test_gpu_exactgp.py::test_prediction_does_not_depend_on_the_chunking (N = 259) and
    test_gpu_rffgp.py::test_factor_reuse (n = 33, 100, 128);
  - the one-shot forms against the handle: gp_predict_oneshot in
    test_gpu_exactgp.py::test_prediction_does_not_depend_on_the_chunking, gpnt_predict_oneshot in
    test_gpu_rffgp.py::test_factor_reuse, gp_nlogmarginal_oneshot and gpnt_nlogmarginal_oneshot in
    the two test_determinism_and_one_shot (test_gpu_exactgp.py, test_gpu_nlml.py);
  - draw_theta before and after a gradient evaluation at even n:
    test_gpu_gpdraw.py::test_bits_do_not_depend_on_S_or_the_other_columns (n = 40, 100, 300); the
    odd n is here.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, NT = 2, 9
H1 = np.array([1.3, 0.8, 0.9, 0.05])          # ARD: D + 2 entries
H2 = np.array([0.9, 1.1, 0.02])               # iso


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def problem(N, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((N, D)))
    Xt = np.asfortranarray(rng.standard_normal((NT, D)))
    f = lambda A: np.sin(A[:, 0]) + 0.5 * A[:, 1]
    return dict(X=X, y=f(X) + 0.1 * rng.standard_normal(N), Xt=Xt,
                yt=f(Xt) + 0.1 * rng.standard_normal(NT))


def not_spd(call):
    from gpt_amd._lib import GPT_ERR_NOT_SPD, GPTError
    with pytest.raises(GPTError) as ei:
        call()
    assert ei.value.code == GPT_ERR_NOT_SPD, ei.value


# ---------------------------------------------------------------------------------- ExactGP
@pytest.fixture(scope="module")
def gp_case():
    """The data and, computed once on fresh handles, predict at H1 and at H2."""
    p = problem(70, 1)
    p["new"] = lambda: G().ExactGP(p["X"], p["y"])
    for nm, h in (("fresh1", H1), ("fresh2", H2)):
        gp = p["new"]()
        p[nm] = gp.predict(h, p["Xt"], p["yt"])
        gp.close()
    assert np.isfinite(p["fresh1"].lp).all() and not same(p["fresh1"], p["fresh2"])
    return p


def test_exact_gp_refits_when_the_hyper_parameters_change(gp_case):
    p = gp_case
    gp = p["new"]()
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    assert same(gp.predict(H2, p["Xt"], p["yt"]), p["fresh2"])
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])         # and on the kept factor
    gp.close()


def test_exact_gp_scratch_block_regrows(gp_case):
    p = gp_case
    gp = p["new"]()
    assert same(gp.predict(H1, p["Xt"], p["yt"], chunk=2), p["fresh1"])    # 2 columns
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])             # regrown to Ntest
    assert same(gp.predict(H1, p["Xt"], p["yt"], chunk=2), p["fresh1"])    # 2 of the larger block
    assert same(gp.predict(H1, p["Xt"], p["yt"], chunk=5), p["fresh1"])
    gp.close()


def test_exact_gp_failed_factorisation_clears_the_key():
    """test_gpu_exactgp.py::test_failed_factorisation_is_a_status's input at N = 70: X = 0 makes
    every K_ij = 1, and 1 + 1e-20 = 1, so the second pivot is exactly 1 - 1 = 0; K + 0.5 I is
    positive definite."""
    N = 70
    X, y = np.zeros((N, D), order="F"), np.arange(N, dtype=np.float64)
    Xt = problem(N, 2)["Xt"]
    yt = np.linspace(-1.0, 1.0, NT)
    bad, ok = np.array([1.0, 1.0, 1.0, 1e-20]), np.array([1.0, 1.0, 1.0, 0.5])
    gp = G().ExactGP(X, y)
    fresh = gp.predict(ok, Xt, yt)
    gp.close()
    assert np.isfinite(fresh.fmu).all() and np.isfinite(fresh.lp).all()
    gp = G().ExactGP(X, y)
    not_spd(lambda: gp.value_and_grad(bad))                 # the first call of the handle fails
    assert same(gp.predict(ok, Xt, yt), fresh)
    not_spd(lambda: gp.predict(bad, Xt, yt))                # a failure after a kept factor
    not_spd(lambda: gp.predict(bad, Xt, yt))                # no stale key: it fails again
    assert same(gp.predict(ok, Xt, yt), fresh)
    gp.close()


def test_exact_gp_prior_draw_overwrites_the_factor(gp_case):
    p = gp_case
    gp = p["new"]()
    F = gp.draw_prior(H1, S=3, seed=5)
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])         # the same h: refit
    assert np.array_equal(gp.draw_prior(H1, S=3, seed=5), F)           # over predict's factor
    assert same(gp.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    gp.close()


# ------------------------------------------------------------------------- NoTensorMarginal
_NT = {}


def nt_problem(n):
    """The data at n features and, computed once on fresh handles, predict at H1 and at H2."""
    if n in _NT:
        return _NT[n]
    p = problem(40, 3)
    rng = np.random.default_rng(4)
    p["Z"] = np.asfortranarray(rng.standard_normal((n, D)))
    p["b"] = 2 * np.pi * rng.random(n)
    p["n"] = n
    p["new"] = lambda: G().NoTensorMarginal(p["X"], p["y"], p["Z"], p["b"])
    for nm, h in (("fresh1", H1), ("fresh2", H2)):
        m = p["new"]()
        p[nm] = m.predict(h, p["Xt"], p["yt"])
        m.close()
    assert np.isfinite(p["fresh1"].lp).all() and not same(p["fresh1"], p["fresh2"])
    _NT[n] = p
    return p


@pytest.fixture(params=[18, 17], ids=["n18", "n17"])
def nt_case(request):
    return nt_problem(request.param)


def test_marginal_refits_when_the_hyper_parameters_change(nt_case):
    p = nt_case
    m = p["new"]()
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    assert same(m.predict(H2, p["Xt"], p["yt"]), p["fresh2"])
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])           # and on the kept factor
    m.close()


def test_marginal_scratch_block_regrows(nt_case):
    p = nt_case
    m = p["new"]()
    assert same(m.predict(H1, p["Xt"], p["yt"], chunk=2), p["fresh1"])     # 2 columns
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])              # regrown to Ntest
    assert same(m.predict(H1, p["Xt"], p["yt"], chunk=2), p["fresh1"])     # 2 of the larger block
    assert same(m.predict(H1, p["Xt"], p["yt"], chunk=5), p["fresh1"])
    m.close()


def test_marginal_failed_cholesky_clears_the_key(nt_case):
    """Two failing inputs.  test_gpu_rffgp.py::test_failed_cholesky_leaves_the_handle_usable's is a
    NaN in X, which no later call on that handle can get past: there a handle that has failed
    answers as a fresh one does, the status and NaN-filled outputs.  For the handle to recover the
    failure has to come from the hyper-parameters: sigma_RBF = 1e200 makes phi phi' overflow, the
    first pivot is inf, its column inf/inf, and the second pivot is not positive."""
    from gpt_amd._lib import GPT_ERR_NOT_SPD, P_D, lib
    p = nt_case
    X = p["X"].copy()
    X[7, 1] = np.nan
    h = H1.ctypes.data_as(P_D)

    def raw(m):
        out = [np.ones(NT), np.ones(NT), np.ones(NT)]
        rc = lib().gpt_nlml_predict(m._h, h, H1.size, p["Xt"].ctypes.data_as(P_D), NT,
                                    p["yt"].ctypes.data_as(P_D), 0, *[o.ctypes.data_as(P_D) for o in out])
        return rc, out

    fresh = G().NoTensorMarginal(X, p["y"], p["Z"], p["b"])
    rc0, out0 = raw(fresh)
    fresh.close()
    assert rc0 == GPT_ERR_NOT_SPD and all(np.isnan(o).all() for o in out0)
    poisoned = G().NoTensorMarginal(X, p["y"], p["Z"], p["b"])
    not_spd(lambda: poisoned.value_and_grad(H1))
    rc1, out1 = raw(poisoned)                               # no stale factor is taken
    poisoned.close()
    assert rc1 == rc0 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out0, out1))

    over = H1.copy()
    over[-2] = 1e200
    m = p["new"]()
    not_spd(lambda: m.value_and_grad(over))                 # the first call of the handle fails
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    not_spd(lambda: m.predict(over, p["Xt"], p["yt"]))      # a failure after a kept factor
    not_spd(lambda: m.predict(over, p["Xt"], p["yt"]))      # no stale key: it fails again
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])
    m.close()


def test_theta_draws_on_the_lazy_and_on_the_gradient_inverse():
    p = nt_problem(17)                                      # the odd n (the even ones: see above)
    z = np.asfortranarray(np.random.default_rng(6).standard_normal((p["n"], 3)))
    m = p["new"]()
    lazy = m.draw_theta(H1, S=3, z=z)                       # Xt built by the draw
    assert np.isfinite(lazy).all()
    m.value_and_grad(H1)
    assert np.array_equal(m.draw_theta(H1, S=3, z=z), lazy)             # Xt left by the gradient
    m.nlogmarginal(H1)                                                  # no Xt after this one
    assert np.array_equal(m.draw_theta(H1, S=3, z=z), lazy)
    assert same(m.predict(H1, p["Xt"], p["yt"]), p["fresh1"])           # Xt left by the draw
    m.close()
