"""The posterior predictive of stored samples on the device (gpt_amd/csrc/predictive.hip) against
the mpmath reference and the yardsticks of tests/predictive_ref.py, its exact properties, its
independence of everything but a row's own values, and the tensor and full-theta routes.

Bar of fmu, fs2, lp, lp_mix (error relative to the column's max |value|):
max(8 × the numpy restatement's own error against mpmath, (S + 16)·2^-53); tests/
test_predictive_ref.py holds the restatement itself.  Measured on the MI355X, device error /
bar (numpy's error in units of 2^-53 in brackets):

    case   fmu             fs2             lp              lp_mix
    a      0      (0)      0      (0)      0.0635 (1.08)   0.0635  (1.08)
    b      0.0366 (0.659)  0.0892 (1.61)   0.125  (2.33)   0.125   (3)
    c      0.0489 (1.03)   0.0993 (2.08)   0.125  (3.06)   0.0276  (1.18)
    d      0.0598 (4.85)   0.0597 (4.83)   0.0548 (4.44)   0.00864 (0.7)
    e      0.0308 (4.84)   0.0504 (7.91)   0.0649 (10.2)   0.013   (2.06)
    f      0.0487 (2.39)   0.0562 (2.75)   0.125  (7.79)   0.015   (0.736)
    g      0.091  (4.46)   0      (0)      0.125  (12.7)   0.0825  (4.04)
    h      0.0893 (4.38)   0.0508 (2.49)   0.125  (8.32)   0.0604  (2.96)
"""
import numpy as np
import pytest

import gpnt_ref as GR
import predictive_ref as PR
from oracle import pred_cases as PC

pytestmark = pytest.mark.gpu

TENSOR_SHAPE = (8, 2, 65, 3, 5, 5)       # n, D, Ntest, r, Q, S


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def rows(ev):
    return dict(fmu=ev.gp.fmu, fs2=ev.gp.fs2, lp=ev.gp.lp, lp_mix=ev.lp_mix)


def same_bits(a, b):
    ra, rb = rows(a), rows(b)
    return (all(np.array_equal(ra[q], rb[q]) for q in PR.QUANTITIES)
            and np.array_equal(a.gp.ys2, b.gp.ys2) and np.array_equal(a.gp.ymu, b.gp.ymu)
            and (a.mnlp, a.mnlp_mix, a.coverage95) == (b.mnlp, b.mnlp_mix, b.coverage95))


def run_case(name):
    F, y, window, nv = PR.inputs(name)
    return G().predictive(F, y, nv, window=window)


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_predictive_against_mpmath(name):
    pytest.importorskip("mpmath")
    F, y, (a, b), nv = PR.inputs(name)
    ev, ref, ys = run_case(name), PR.reference(name), PR.yardstick(name)
    got = rows(ev)
    line = []
    for q in PR.QUANTITIES:
        err = PR.col_err(got[q], ref[q])
        line.append("%s %.3g (%.3g)" % (q, err / PR.bar(name, q), ys[q] / PR.U))
    print("case %s: device error / bar (numpy error / 2^-53): %s" % (name, ", ".join(line)))
    for q in PR.QUANTITIES:
        assert PR.col_err(got[q], ref[q]) <= PR.bar(name, q), (name, q)
    Nt = y.size
    rb = (Nt + 8) * PR.U
    assert PR.rel_err(ev.mnlp, -PR.sum_mp(ev.gp.lp) / Nt) <= rb
    assert PR.rel_err(ev.mnlp_mix, -PR.sum_mp(ev.lp_mix) / Nt) <= rb
    assert ev.coverage95 * Nt == ref["covered"]
    assert (ev.gp.fs2 >= 0).all()
    assert np.array_equal(ev.gp.ys2, ev.gp.fs2 + nv) and ev.gp.ymu is ev.gp.fmu
    assert ev.mean_fhat is ev.gp.fmu and ev.window == (a, b)


@pytest.mark.parametrize("name", ["a", "g"])
def test_equal_columns_have_zero_variance(name):
    _, _, _, nv = PR.inputs(name)
    ev = run_case(name)
    assert (ev.gp.fs2 == 0.0).all() and (ev.gp.ys2 == nv).all()


def test_log_density_survives_underflow():
    F, y, (a, b), nv = PR.inputs("f")
    # the unshifted sum is exactly 0 on the rows whose nearest sample is over 0.04 away
    assert (np.exp(-(y[:, None] - F) ** 2 / (2 * nv)).sum(axis=1) == 0.0).sum() >= 10
    assert np.isfinite(run_case("f").lp_mix).all()


def test_scale_enters_the_scalars_only():
    F, y, window, nv = PR.inputs("c")
    a, b = G().predictive(F, y, nv, window=window), G().predictive(F, y, nv, window=window, scale=17.3)
    assert all(np.array_equal(rows(a)[q], rows(b)[q]) for q in PR.QUANTITIES)
    assert b.mnlp == a.mnlp + np.log(17.3) and b.mnlp_mix == a.mnlp_mix + np.log(17.3)
    assert np.array_equal(b.sample_rmse, a.sample_rmse * 17.3) and b.rmse == a.rmse * 17.3
    assert np.allclose(b.sample_loglik, a.sample_loglik, rtol=1e-14, atol=0)


# --------------------------------------------------------------------------- independence
def test_rows_do_not_depend_on_the_other_rows():
    F, y, window, nv = PR.inputs("e")
    full, part = run_case("e"), G().predictive(F[:40], y[:40], nv, window=window)
    for q in PR.QUANTITIES:
        assert np.array_equal(rows(full)[q][:40], rows(part)[q]), q


def test_rows_do_not_depend_on_where_the_window_sits():
    F, y, (a, b), nv = PR.inputs("e")
    full, cut = run_case("e"), G().predictive(np.asfortranarray(F[:, a:b]), y, nv)
    assert same_bits(full, cut)


def test_a_repeated_call_gives_the_same_bits():
    assert same_bits(run_case("e"), run_case("e"))


# --------------------------------------------------------------------------- routes
def test_tensor_routes():
    p = PC._inputs(TENSOR_SHAPE, 0)
    n, D, Nt, r, Q, S = TENSOR_SHAPE
    nv, window, scale = 0.05, (1, 5), 3.1
    fhat = np.asfortranarray(np.stack([G().pred(p["w"][:, s], p["U"][..., s], p["I"], p["phi"])
                                       for s in range(S)], axis=1))
    want = G().predictive(fhat, p["y"], nv, window=window, scale=scale)
    got = G().pred_predictive(p["w"], p["U"], p["I"], p["phi"], p["y"], nv, window=window, scale=scale)
    assert same_bits(got, want)
    assert np.array_equal(got.sample_rmse, want.sample_rmse) and got.rmse == want.rmse
    mean, _ = G().pred_mean(p["w"][:, 1:5], p["U"][..., 1:5], p["I"], p["phi"], p["y"])
    assert np.array_equal(got.gp.fmu, mean)
    cols = G().pred_predictive(p["w"], p["U"], p["I"], p["phi"], p["y"], nv, cols=range(1, 5), scale=scale)
    assert same_bits(cols, got)
    phi = G().feature(p["X"], p["ls"], 1.0, p["scale"], p["Z"], p["b"])
    on_phi = G().pred_predictive(p["w"], p["U"], p["I"], phi, p["y"], nv, window=window, scale=scale)
    on_x = G().pred_predictive_x(p["w"], p["U"], p["I"], p["X"], p["y"], p["ls"], 1.0, p["scale"],
                                 p["Z"], p["b"], nv, window=window, scale=scale)
    assert same_bits(on_x, on_phi)
    assert np.array_equal(on_x.sample_rmse, on_phi.sample_rmse) and on_x.rmse == on_phi.rmse


def test_full_theta_routes():
    n, N, m, burnin, maxepoch, decay = GR.CASES["A"]
    phi, y = GR.inputs("A")
    store, status = G().GPNT_SGLD_chains(phi, y, GR.SIGNAL_VAR, GR.SIGMA_THETA, m, GR.EPS, decay,
                                         burnin, maxepoch, GR.SEEDS)
    assert not status.any()
    theta, nv, scale = store[:, :, 0], GR.SIGNAL_VAR[0], 17.3
    T = theta.shape[1]
    window = (T // 2, T)
    ref = G().GPNT_pred(theta, phi, y, window=window, scale=scale, scores=True)
    want = G().predictive(ref.scores, y, nv, window=window, scale=scale)
    got = G().GPNT_predictive(theta, phi, y, nv, window=window, scale=scale)
    assert same_bits(got, want)
    assert np.array_equal(got.gp.fmu, ref.mean_fhat) and got.mean_fhat is got.gp.fmu
    for ev in (got, want):
        assert ev.rmse == ref.rmse and np.array_equal(ev.sample_rmse, ref.sample_rmse)
        sse = y.size * (ev.sample_rmse / scale) ** 2
        formula = -sse / (2 * nv) - 0.5 * y.size * np.log(2 * np.pi * nv)
        assert (np.abs(ev.sample_loglik - formula) <= 4 * PR.U * np.abs(formula)).all()
    cols = np.arange(T // 2, T)
    assert same_bits(G().GPNT_predictive(theta, phi, y, nv, cols=cols, scale=scale), got)
    X, ls, sigma, Z, b = GR.eval_x_inputs()
    th, _, yt = GR.eval_inputs()
    phit = G().featureNotensor(X, ls, sigma, Z, b)
    w = GR.EVAL["window"]
    on_phi = G().GPNT_predictive(th, phit, yt, nv, window=w, scale=scale)
    on_x = G().GPNT_predictive_x(th, X, yt, ls, sigma, Z, b, nv, window=w, scale=scale)
    assert same_bits(on_x, on_phi)
    assert np.array_equal(on_x.sample_rmse, on_phi.sample_rmse) and on_x.rmse == on_phi.rmse


def test_fs2_of_exact_posterior_draws_is_the_posterior_variance():
    theta, phitest, ytest, var = PR.posterior_draws()
    ev = G().GPNT_predictive(theta, phitest, ytest, PR.DRAWS["signal_var"])
    assert ev.gp.fs2.shape == (PR.DRAWS["Ntest"],)
    assert (np.abs(ev.gp.fs2 / var - 1) <= PR.draws_band()).all()


def test_device_entry_equals_the_host_entry():
    import torch
    from gpt_amd.session import predictive_device
    F, y, window, nv = PR.inputs("e")
    want = run_case("e")
    fhat = torch.from_numpy(np.array(F.T, order="C")).cuda()
    fmu, fs2, lp, lpmix, s_lp, s_mix, covered = predictive_device(fhat, torch.from_numpy(y.copy()).cuda(),
                                                                  nv, window=window)
    got = dict(fmu=fmu, fs2=fs2, lp=lp, lp_mix=lpmix)
    for q in PR.QUANTITIES:
        assert np.array_equal(got[q].cpu().numpy(), rows(want)[q]), q
    assert -s_lp / y.size == want.mnlp and -s_mix / y.size == want.mnlp_mix
    assert covered == round(want.coverage95 * y.size)
    none = predictive_device(fhat, torch.from_numpy(y.copy()).cuda(), nv, window=window, rows=False)
    assert none[:4] == (None,) * 4 and none[4:] == (s_lp, s_mix, covered)
