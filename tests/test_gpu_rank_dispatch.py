"""Every entry of the launch tables (gpt_amd/csrc/launch_util.h) reaches its own kernel.

The host picks a kernel instantiation from a run-time value (the rank r, the classifier's padded
class count CC, ...).  The parity tests hold most (family, value) pairs to the oracle already; this
file holds the pairs they leave out, each at the smallest shape the family takes at that value,
against the restatement its family's parity test uses and at that test's bar.  A launch that
reached another rank's kernel reads U with the wrong stride and misses these bars by many orders.

Held elsewhere (tests/<file>::<test>):
  grid step, temp_init, r in Ranks   test_gpu_step.py::test_step_against_mpmath[sgld_stiefel-*-grid]
  chain R 1..5, J 1 4 8, WV 4 8      test_gpu_step.py::test_step_against_mpmath[sgld_stiefel-*-chain]
  chain J 2 (64 < n <= 128)          test_gpu_parity.py::test_sampler_trajectory_matches_oracle[
                                     batch256-chain]
  wave R in WaveRanks, J 1..4        test_gpu_step.py::test_step_against_mpmath[sgld_stiefel-*-wave]
                                     (J = 3: 130-4-16-120-64-11)
  RMSprop, w-only, class r 2 3 5     test_gpu_step.py::test_step_against_mpmath[rmsprop-* | wonly-* |
                                     cls_*], test_gpu_parity.py::test_rmsprop_trajectory_matches_oracle,
                                     ::test_sgldermw_matches_oracle, ::test_classification_matches_oracle
  pred_kernel r 1 5 20               test_gpu_pred.py::test_pred_direct_kernels
  pred_x_kernel r 1 5 20             the same (gpt_pred_mean_x launches it under GPTSGLD_PRED=direct only)
  pairs NT 1..8, rows-pf D cases     test_gpu_pred.py::test_pred_golden_parity and
                                     oracle/pred_cases.py HELD_ELSEWHERE
  tgp_temp r 3 5                     test_gpu_tgp.py::test_gibbs_matches_oracle; r 2 3 5 against mpmath:
                                     test_gpu_gibbs.py::test_sampler_against_mpmath[tgp-*]
  GMC kick, geodesic r 2 5           test_gpu_parity.py::test_gmc_matches_oracle; r 1 2 3 5 against
                                     mpmath: test_gpu_gibbs.py::test_sampler_against_mpmath[gmc-*]
  cf_epoch domove 2 r 1 4 15 20      test_gpu_movielens.py::test_fullw_sideinfo_matches_oracle,
                                     ::test_fullw_sideinfo_lazy_move_wide_batches,
                                     ::test_fullw_sideinfo_live_config_full_fold,
                                     ::test_fullw_sideinfo_lazy_equals_eager_move
  cf_epoch domove 0, cf_move r 4 5 20   ::test_fullw_no_side_matches_oracle, ::..._lazy_equals_eager_move
  cf_epoch domove 1 r 3 4            ::test_fullw_sideinfo_matches_oracle[sgd_stiefel | sgld_stiefel]
  cf_eval                            every run of the above
  cfg_rows, cfg_wsystem r 3 4 15     ::test_fullw_gibbs_matches_oracle; r 3 4 8 10 against mpmath:
                                     test_gpu_gibbs.py::test_sampler_against_mpmath[mlg-*]
  ntc CC 2 4 8 16                    test_gpu_cls.py::test_sampler_matches_the_restatement
  cjoint value, full, CC 2..32       test_gpu_cjoint.py::test_value_and_gradient_parity
  cjoint theta CC 4 8                test_gpu_cjoint.py::test_langevin_steps
  cjoint scores CC 4 8 32            test_gpu_cjoint.py::test_determinism_and_one_shot,
                                     ::test_scores_with_identity_theta_are_the_features
  expm check (mode, nn)              test_gpu_expm.py::test_device_expm_against_mpmath
The cjoint features mode (a timing diagnostic) writes nothing that a test could read.
"""
import numpy as np
import pytest

import cjoint_ref as CJ
import cls_ref as CLS
from oracle import gpt_sgld_ref as R
from oracle import movielens_ref as M
from oracle import pred_cases as PC
from test_gpu_movielens import problem as ml_problem
from test_gpu_parity import _gmc_problem, make_problem, rel
from test_gpu_pred import route
from test_gpu_tgp import data as tgp_data, oracle_b

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 16, 20)


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def others(*held):
    return [r for r in RANKS if r not in held]


def shape(r):
    """(n, D, N, Q, m): two steps of one epoch, 3r core entries (r² where that is fewer).  A column
    of U that no core entry names has no gradient, and RMSprop divides that column's rounding noise
    by the root of its own mean square: at Q = 4 the oracle itself turns a 1e-15 relative change
    of U_init into 2.6e-8 (r = 15), 2.6e-9 (r = 12), 1.5e-9 (r = 10) in these two steps; at Q = 3r
    into 1.4e-14 at the most over the twelve ranks."""
    return max(24, r + 4), 2, 16, min(3 * r, r * r), 8


# ------------------------------------------------------------------- grid engine's step variants
@pytest.mark.parametrize("r", others(2, 3, 5))
def test_rmsprop_rank(r):
    n, D, N, Q, m = shape(r)
    p = make_problem(n, D, N, r, Q, seed=13)
    a = (p["phi"], p["y"], 0.05, p["I"], r, Q, m, 1e-6, 0.9, 0, 1, 29)
    ws, Us = G().GPT_SGLDERM_RMSprop(*a)
    wo, Uo, info = R.GPT_SGLDERM_RMSprop(*a)
    assert info["status"] == 0
    print("rmsprop r = %d: w %.3g U %.3g" % (r, rel(ws, wo), rel(Us, Uo)))
    assert rel(ws, wo) < 1e-8 and rel(Us, Uo) < 1e-8


@pytest.mark.parametrize("r", others(2, 3, 5))
def test_wonly_rank(r):
    n, D, N, Q, m = shape(r)
    p = make_problem(n, D, N, r, Q, seed=17)
    a = (p["phi"], p["y"], 0.05, p["I"], r, Q, m, 1e-4, 0, 1, 31)
    ws, U, gn = G().GPT_SGLDERMw(*a, diag=True)
    wo, Uo, info = R.GPT_SGLDERMw(*a, record=True)
    print("w-only r = %d: w %.3g" % (r, rel(ws, wo)))
    assert rel(U, Uo) < 1e-14
    assert rel(ws, wo) < 1e-9
    assert rel(gn, np.array(info["gradw_norm"])) < 1e-9


@pytest.mark.parametrize("r", others(2, 3, 5))
def test_classification_rank(r):
    n, D, N, Q, m = shape(r)
    p = make_problem(n, D, N, r, Q, seed=23)
    y = 1.0 + (p["y"] > np.median(p["y"]))
    a = (p["phi"], y, p["I"], r, Q, m, 1e-4, 1e-6, 0, 1, 41)
    ws, Us = G().GPTclassification(*a)
    wo, Uo, info = R.GPTclassification(*a)
    assert info["status"] == 0
    print("classification r = %d: w %.3g U %.3g" % (r, rel(ws, wo), rel(Us, Uo)))
    assert rel(ws, wo) < 1e-8 and rel(Us, Uo) < 1e-8


# ---------------------------------------------------------------------------- direct prediction
@pytest.mark.parametrize("r", others(1, 5, 20))
def test_pred_direct_rank(r, monkeypatch):
    """pred_kernel (GPTSGLD_PRED=direct) and pred_x_kernel, two samples, 70 rows (a ragged tile)."""
    n, D, Nt, Q, S = max(24, r + 4), 2, 70, min(4, r * r), 2
    rng = np.random.default_rng(r)
    X, Z, b = rng.standard_normal((Nt, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random((n, D))
    ls = 1 + 0.2 * rng.standard_normal(D)
    phi = R.feature(X, ls, 1.1, 2.0, Z, b)
    I = R.samplenz(r, D, Q, 3)
    ws = rng.standard_normal((Q, S))
    Us = np.stack([R.init_state(n, r, D, Q, 10 + s)[1] for s in range(S)], axis=3)
    f = np.stack([R.pred(ws[:, s], Us[..., s], I, phi) for s in range(S)])
    monkeypatch.setenv("GPTSGLD_PRED", "direct")       # read by every call; both kernels need it
    got = G().pred(ws[:, 1], Us[..., 1], I, phi)
    assert route() == dict(kind=PC.DIRECT, tdim=0, npw=0, grid=2, tiles=2, passes=1, first=1)
    assert rel(got, f[1]) < 1e-12, rel(got, f[1])
    mean = G().pred_mean_x(ws, Us.reshape((n, r, D * S), order="F"), I, X, rng.standard_normal(Nt),
                           ls, 1.1, 2.0, Z, b)[0]
    # pred_x_kernel records no route; the stacked-sample path it replaces would have (first = S)
    assert route()["kind"] == PC.DIRECT and route()["first"] == 1
    assert rel(mean, f.mean(axis=0)) < 1e-12, rel(mean, f.mean(axis=0))


# ------------------------------------------------------------------------------ tensor GP, GMC
@pytest.mark.parametrize("r", others(3, 5))
def test_tgp_gibbs_rank(r):
    from gpt_amd import TGP
    n, D, N, q, sigma, gen, srbf = r + 4, 2, 40, min(6, r * r), 0.3, 123, 1.4332
    X, y = tgp_data(N, D, 7)
    W, U, I = TGP.GPT_inf(X, y, sigma, n, r, srbf, q, gen, 2, 0)
    b = oracle_b(R.datawhitening(X), n, srbf, gen)
    Wo, Uo, Io = R.GPT_inf(b, R.datawhitening(y), sigma, n, r, q, 2, 0, gen)
    assert (I == Io).all()
    print("tgp r = %d: W %.3g U %.3g" % (r, rel(W, Wo), rel(U, Uo)))
    assert rel(W, Wo) < 1e-8 and rel(U, Uo) < 1e-8


@pytest.mark.parametrize("r", others(2, 5))
def test_gmc_rank(r):
    n, D, N, Q = r + 4, 2, 16, min(4, r * r)
    phi, y, I = _gmc_problem(n, D, N, r, Q)
    a = (phi, y, 1.0, I, r, Q, 1e-2, 1e-2, 0, 2, 2, 7)
    ws, Us, acc = G().GPT_GMC(*a)
    wo, Uo, acco = R.GPT_GMC(*a)
    print("gmc r = %d: w %.3g U %.3g" % (r, rel(ws, wo), rel(Us, Uo)))
    assert rel(ws, wo) < 1e-8 and rel(Us, Uo) < 1e-8
    assert np.all(np.abs(acc - acco) <= 1e-7 * np.maximum(np.abs(acco), 1e-3))


# ------------------------------------------------------------------------------------ MovieLens
def check_cf(got, want):
    for g, w_ in zip(got[:3], want[:3]):
        assert rel(g, w_) < 1e-8, rel(g, w_)
    assert np.abs(got[3] - want[3]).max() < 1e-8
    assert np.all(np.abs(got[4] - want[4]) <= 1e-9 * want[4])
    assert np.all(np.abs(got[5] - want[5]) <= 1e-9 * want[5])


CF_MOVES = {   # cf_epoch_kernel's domove: (langevin, stiefel, epsU, ranks the parity tests hold)
    2: (False, False, 1e-6, (1, 4, 15, 20)),      # the lazy SGD move
    0: (True, False, 1e-6, (4, 5, 20)),           # batch phase, then cf_move_kernel
    1: (False, True, 1e-4, (3, 4)),               # the Stiefel move inside the epoch kernel
}


@pytest.mark.parametrize("domove,r", [(dm, r) for dm, v in CF_MOVES.items() for r in others(*v[3])])
def test_cf_epoch_rank(domove, r):
    """One epoch of three batches over 48 ratings (cf_epoch, cf_move, cf_eval)."""
    from gpt_amd import movielens
    lang, stf, epsU, _ = CF_MOVES[domove]
    tr, te, ud, md, mu, sd = ml_problem(48, 12)
    w0 = np.random.default_rng(5).standard_normal((r, r))
    args = (tr, ud, md, te, 0.8, 0.1, 1.0, w0, 16, 1e-4, epsU, 0.5, 0.25, 0.5, 0, 1, 17, mu, sd)
    got = movielens.GPT_fullw_sideinfo(*args, langevin=lang, stiefel=stf, avg=False)
    assert movielens.last_timing()["mode"] == domove          # the route the host took
    check_cf(got, M.GPT_fullw_sideinfo(*args, langevin=lang, stiefel=stf, avg=False))


@pytest.mark.parametrize("r", others(3, 4, 15))
def test_cf_gibbs_rank(r):
    """One sweep over 48 ratings (cfg_rows, cfg_wsystem)."""
    from gpt_amd import movielens
    tr, te, ud, md, mu, sd = ml_problem(48, 12)
    w0 = np.random.default_rng(9).standard_normal((r, r))
    args = (tr, ud, md, te, 0.8, 0.5, 1.0, w0, 0, 1, 1, 17, mu, sd)
    check_cf(movielens.GPT_fullw_gibbs(*args, avg=False, rotated_w=False),
             M.GPT_fullw_gibbs(*args, avg=False, rotated_w=False))


# ------------------------------------------------------------------------------ the classifiers
def test_ntc_cc32():
    """GPNT_SGLDclass at 20 classes (CC = 32)."""
    case = (40, 60, 20, 25, 0, 1, 0.0, 1.0)
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, eps = CLS.sampler_inputs(case, 7)
    got = G().GPNT_SGLDclass(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
    want = CLS.gpnt_sgld_class(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
    assert got.shape == want.shape == (n, C, 3)
    assert CLS.rel(got, want) < 1e-9, CLS.rel(got, want)


@pytest.mark.parametrize("idx", [2, 3, 5], ids=["cc2", "cc16", "cc32"])
def test_cjoint_theta_and_scores_cc(idx):
    """The Langevin step (mode theta) and the scores at the class counts tests/test_gpu_cjoint.py
    runs neither at: C = 2, 16 and 32 of its golden cases."""
    case = CJ.CASES[idx]
    g = CJ.load_golden()[CJ.case_name(case)]
    h = g["H"][1]
    j = G().SoftmaxJoint(g["X"], g["y"], g["Z"], g["b"], C=g["theta"].shape[1])
    j.set_theta(g["theta"])
    D = g["X"].shape[1]
    phi = G().featureNotensor(g["X"][:9], h[:D] if case[4] == "ard" else h[0], h[-1], g["Z"], g["b"])
    want = phi.T @ g["theta"]
    got = j.scores(h, g["X"][:9])
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    want = CJ.langevin(g["X"], g["y"], g["Z"], g["b"], g["theta"], h, 2e-3, 1, 11, 0)
    j.langevin(h, 2e-3, 1, 11, t0=0)
    assert CLS.rel(j.theta(), want) < 1e-9, CLS.rel(j.theta(), want)
    j.close()
