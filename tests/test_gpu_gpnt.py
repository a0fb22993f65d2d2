"""The full-theta regression chains on the device (gpt_amd/csrc/gpnt.hip) and the evaluation of
their samples, against the restatements and yardsticks of tests/gpnt_ref.py.

Cases (tests/gpnt_ref.py CASES; workgroup = 512 threads = 8 waves): A n = 70 with the whole batch
staged and a last batch of 3 rows; B n = 1100 with several row groups per step and a short last
group; C n = 10 300, where not one row fits beside theta; D batches of one row; E m > N; F n = 6000,
where two rows fit, which is too few to be worth staging unless asked for.

Bounds: parity with the oracle at relative 1e-9 (the bar of test_gpu_parity's GPNT_SGLD test);
three steps within min(8·u, 1e-13)·max|theta| of mpmath, u the numpy restatement's own error on the
same inputs (tests/test_gpnt_ref.py); a score within (n + 2)·2^-53·sum_j|phi_ji·theta_js| (one fma
chain of length n); an RMSE within relative (Ntest + 8)·2^-53 of the mpmath RMSE of the returned
values (a sum of non-negative terms with two roundings each, at most Ntest - 1 additions in any
order, a division, a square root and the scale); a window mean within (S + 1)·2^-53·sum_s|f_is|/S.
"""
import numpy as np
import pytest

import gpnt_ref as GR
from oracle import gpt_sgld_ref as R

pytestmark = pytest.mark.gpu

ROWS_ENV = "GPTSGLD_GPNT_ROWS"


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def run_chains(name, ks=(0, 1, 2), store_every=1, eps=None, phi_y=None):
    n, N, m, burnin, maxepoch, decay = GR.CASES[name]
    phi, y = GR.inputs(name) if phi_y is None else phi_y
    eps = GR.EPS if eps is None else eps
    pick = lambda v: [v[k] for k in ks]
    return G().GPNT_SGLD_chains(phi, y, pick(GR.SIGNAL_VAR), pick(GR.SIGMA_THETA), m, pick(eps), decay,
                                burnin, maxepoch, pick(GR.SEEDS), store_every=store_every)


@pytest.fixture(autouse=True)
def no_rows_cap(monkeypatch):
    monkeypatch.delenv(ROWS_ENV, raising=False)


# ------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_chains_match_the_oracle(name):
    n, N, m, burnin, maxepoch, decay = GR.CASES[name]
    phi, y = GR.inputs(name)
    store, status = run_chains(name)
    total = (burnin + maxepoch) * (-(-N // m))
    assert not status.any() and store.shape == (n, total, 3)
    for k in range(3):
        want = R.GPNT_SGLD(phi, y, GR.SIGNAL_VAR[k], GR.SIGMA_THETA[k], m, GR.EPS[k], decay, burnin,
                           maxepoch, GR.SEEDS[k])
        r = GR.rel(store[:, :, k], want)
        print("case %s chain %d: rel = %.3g" % (name, k, r))
        assert r < 1e-9, (k, r)


@pytest.mark.parametrize("name", GR.STEP_CASES)
def test_three_steps_against_mpmath(name):
    phi, y, sv, sth, m, eps, decay, seed = GR.step_problem(name)
    store, status = G().GPNT_SGLD_chains(phi, y, sv, sth, m, eps, decay, 0, 2, [seed])
    assert not status.any()
    err, bar = GR.max_err_mp(store[:, :3, 0], GR.step_reference(name)), GR.step_bar(name)
    print("case %s: three-step error / max|theta| = %.3g, bar = %.3g, error / bar = %.3f" % (
        name, err, bar, err / bar))
    assert err <= bar, err / bar


def test_routes():
    n, N, m = GR.CASES["A"][:3]
    run_chains("A", ks=(0,))
    route = G().gpnt_last_route()
    assert route["rows"] == m and route["groups"] == 1, route
    m = GR.CASES["B"][2]
    run_chains("B", ks=(0,))
    route = G().gpnt_last_route()
    assert 0 < route["rows"] < m and route["groups"] > 1 and m % route["rows"] != 0, route
    assert route["lds_bytes"] <= 160 * 1024
    run_chains("C", ks=(0,))
    route = G().gpnt_last_route()
    assert route["rows"] == 0 and route["groups"] == 0, route
    assert 8 * GR.CASES["C"][0] <= route["lds_bytes"] <= 160 * 1024


def test_groups_of_fewer_rows_than_half_the_waves_are_staged_only_on_request(monkeypatch):
    base, status = run_chains("F")
    route = G().gpnt_last_route()
    assert not status.any() and route["rows"] == 0, route
    monkeypatch.setenv(ROWS_ENV, "5")                      # two rows are what fits
    got, status = run_chains("F")
    route = G().gpnt_last_route()
    assert not status.any() and route["rows"] == 2 and route["groups"] == 3, route
    assert np.array_equal(got, base)


@pytest.mark.parametrize("name", ["A", "B"])
def test_results_do_not_depend_on_the_group_size(name, monkeypatch):
    base, status = run_chains(name)
    assert not status.any()
    m = GR.CASES[name][2]
    for cap, rows in (("1", 1), ("7", 7), ("0", 0)):
        monkeypatch.setenv(ROWS_ENV, cap)
        got, status = run_chains(name)
        route = G().gpnt_last_route()
        assert route["rows"] == rows and route["groups"] == (-(-m // rows) if rows else 0), route
        assert not status.any()
        assert np.array_equal(got, base), cap


def test_chains_are_independent_and_store_every_thins():
    name = "A"
    n, N, m, burnin, maxepoch, decay = GR.CASES[name]
    store, status = run_chains(name)
    assert not status.any()
    for k in range(3):
        one, st = run_chains(name, ks=(k,))
        assert not st.any() and np.array_equal(one[:, :, 0], store[:, :, k]), k
    nb = -(-N // m)
    total = (burnin + maxepoch) * nb
    ends, status = run_chains(name, store_every=nb)
    assert not status.any() and ends.shape == (n, burnin + maxepoch, 3)
    assert np.array_equal(ends, store[:, nb - 1::nb, :])
    assert total % 4 != 0
    some, status = run_chains(name, store_every=4)
    assert some.shape == (n, total // 4, 3)
    assert np.array_equal(some, store[:, 3::4, :][:, :total // 4, :])


def test_an_epoch_of_two_launches():
    """nb = 4100 batches of one row: the epoch takes launches of 4096 and 4 steps, so theta goes to
    HBM and comes back and the second launch starts mid-epoch.  With m = 1 the step is contractive
    while eps·N/(2·signal_var) is well below 1 (0.041 here); the oracle's max|theta| is 2.63 and a
    relative 1e-15 perturbation of phi moves its result by 1.0e-15, so the 1e-9 bar of
    test_chains_match_the_oracle holds over the 4100 steps too."""
    n, N, m, decay, sv, sth, eps = 64, 4100, 1, 0.1, 0.05, 1.0, 1e-6
    seeds = [5, 2 ** 40 + 9]
    phi, y = GR.inputs("D", N=N)
    chains = lambda s, **kw: G().GPNT_SGLD_chains(phi, y, sv, sth, m, eps, decay, 0, 1, s, **kw)
    store, status = chains(seeds)
    assert not status.any() and store.shape == (n, N, 2)
    for k, seed in enumerate(seeds):
        r = GR.rel(store[:, :, k], R.GPNT_SGLD(phi, y, sv, sth, m, eps, decay, 0, 1, seed))
        print("4100 steps, chain %d: rel = %.3g" % (k, r))
        assert r < 1e-9, (k, r)
        one, st = chains([seed])
        assert not st.any() and np.array_equal(one[:, :, 0], store[:, :, k]), k
    last, status = chains(seeds, store_every=N)
    assert not status.any() and last.shape == (n, 1, 2)
    assert np.array_equal(last[:, 0, :], store[:, -1, :])


def test_nan_chain_is_zero_filled_and_leaves_its_siblings():
    from gpt_amd import _lib
    eps = [GR.EPS[0], 1e300, GR.EPS[2]]
    store, status = run_chains("A", eps=eps)
    assert list(status) == [0, _lib.GPT_ERR_NAN_THETA, 0]
    assert not store[:, :, 1].any()
    for k in (0, 2):
        one, st = run_chains("A", ks=(k,))
        assert not st.any() and np.array_equal(one[:, :, 0], store[:, :, k]), k


def test_x_form_equals_the_phi_form():
    n, N, m, burnin, maxepoch, decay = GR.CASES["A"]
    rng = np.random.default_rng(31)
    X = np.asfortranarray(rng.standard_normal((N, 3)))
    Z = np.asfortranarray(rng.standard_normal((n, 3)))
    b = 2 * np.pi * rng.random(n)
    ls, sigma = [1.4, 0.9, 2.1], 1.3
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N)
    phi = G().featureNotensor(X, ls, sigma, Z, b)
    args = (GR.SIGNAL_VAR, GR.SIGMA_THETA, m, GR.EPS, decay, burnin, maxepoch, GR.SEEDS)
    want, st0 = G().GPNT_SGLD_chains(phi, y, *args)
    got, st1 = G().GPNT_SGLD_chains_x(X, y, ls, sigma, Z, b, *args)
    assert not st0.any() and not st1.any() and want.any()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------- evaluation
@pytest.fixture(scope="module")
def evaluation():
    theta, phitest, ytest = GR.eval_inputs()
    ev = G().GPNT_pred(theta, phitest, ytest, window=GR.EVAL["window"], scale=GR.EVAL["scale"],
                       scores=True)
    return ev, GR.scores_mp(phitest, theta)


def test_scores_against_mpmath(evaluation):
    ev, (smp, mag) = evaluation
    n, Nt, T = GR.EVAL["n"], GR.EVAL["Ntest"], GR.EVAL["T"]
    assert ev.scores.shape == (Nt, T)
    worst = 0.0
    for i in range(Nt):
        for t in range(T):
            bound = (n + 2) * GR.U * mag[i, t]
            err = GR.abs_err_mp(ev.scores[i, t], smp[i][t])
            worst = max(worst, err / bound)
            assert err <= bound, (i, t, err / bound)
    print("scores: worst error / bound = %.4f" % worst)


def test_rmse_and_window_mean_against_mpmath(evaluation):
    ev, _ = evaluation
    _, _, ytest = GR.eval_inputs()
    Nt, T, scale, window = (GR.EVAL[k] for k in ("Ntest", "T", "scale", "window"))
    rb = (Nt + 8) * GR.U
    assert ev.sample_rmse.shape == (T,) and ev.mean_fhat.shape == (Nt,) and ev.window == window
    for t in range(T):
        e = GR.rel_err_mp(ev.sample_rmse[t], GR.rmse_mp(ev.scores[:, t], ytest, scale))
        print("sample %d: rmse = %.6f, relative error / bound = %.4f" % (t, ev.sample_rmse[t], e / rb))
        assert e <= rb, (t, e / rb)
    S = window[1] - window[0]
    mmp = GR.mean_mp(ev.scores, *window)
    bound = (S + 1) * GR.U * np.abs(ev.scores[:, window[0]:window[1]]).sum(axis=1) / S
    worst = 0.0
    for i in range(Nt):
        err = GR.abs_err_mp(ev.mean_fhat[i], mmp[i])
        worst = max(worst, err / bound[i])
        assert err <= bound[i], (i, err / bound[i])
    e = GR.rel_err_mp(ev.rmse, GR.rmse_mp(ev.mean_fhat, ytest, scale))
    print("window mean: worst error / bound = %.4f; rmse = %.6f, relative error / bound = %.4f" % (
        worst, ev.rmse, e / rb))
    assert e <= rb, e / rb
    ref = GR.eval_np(*GR.eval_inputs(), window, scale)              # and nothing is far off
    assert abs(ev.rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]
    assert np.abs(ev.sample_rmse - ref["sample_rmse"]).max() <= 1e-12 * ref["sample_rmse"].max()


def test_evaluation_bit_for_bit_properties(evaluation):
    ev, _ = evaluation
    theta, phitest, ytest = GR.eval_inputs()
    T, scale = GR.EVAL["T"], GR.EVAL["scale"]
    for t in range(T):
        one = G().GPNT_pred(theta[:, t], phitest, ytest, scale=scale, scores=True)
        assert one.sample_rmse[0] == ev.sample_rmse[t], t
        assert np.array_equal(one.scores[:, 0], ev.scores[:, t]), t
        assert np.array_equal(one.mean_fhat, ev.scores[:, t])     # the mean of one sample is exact
        assert one.rmse == ev.sample_rmse[t] and one.window == (0, 1)
    cols = [T - 1, 0, 2]
    a = G().GPNT_pred(theta, phitest, ytest, cols=cols, window=(1, 3), scale=scale, scores=True)
    b = G().GPNT_pred(theta[:, cols], phitest, ytest, window=(1, 3), scale=scale, scores=True)
    for q in ("sample_rmse", "mean_fhat", "scores"):
        assert np.array_equal(getattr(a, q), getattr(b, q)), q
    assert a.rmse == b.rmse
    assert np.array_equal(a.scores, ev.scores[:, cols])
    assert G().GPNT_pred(theta, phitest, ytest, scale=scale).scores is None


def test_pred_x_equals_pred_on_the_device_features():
    theta, _, ytest = GR.eval_inputs()
    Xtest, ls, sigma, Z, b = GR.eval_x_inputs()
    phitest = G().featureNotensor(Xtest, ls, sigma, Z, b)
    kw = dict(window=GR.EVAL["window"], scale=GR.EVAL["scale"], scores=True)
    a = G().GPNT_pred_x(theta, Xtest, ytest, ls, sigma, Z, b, **kw)
    c = G().GPNT_pred(theta, phitest, ytest, **kw)
    assert c.scores.any()
    for q in ("sample_rmse", "mean_fhat", "scores"):
        assert np.array_equal(getattr(a, q), getattr(c, q)), q
    assert a.rmse == c.rmse
