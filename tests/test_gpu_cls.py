"""Classification on the device (gpt_amd/csrc/cls.hip) against the restatements and yardsticks of
tests/cls_ref.py: the GPNT_SGLDclass step engine, the evaluation kernel against mpmath, the
full-theta and tensor evaluation paths, and ImageNoTensorExperiment.jl's configuration on the
segment data.

Bounds (tests/cls_ref.py): a row's nlp is held to E_i = eps·(2|a_i| + |x_{i,y_i}| + C + 4), a mean
of Ntest rows to mean_i E_i + eps·Ntest·mean_i|nlp_i|.  Where the scores themselves differ from the
reference's by at most d_i in row i, nlp_i = lse(x_i) − x_{i,y} moves by at most 2·d_i (lse is
1-Lipschitz in the maximum norm), which is added to the row's bound.
"""
import numpy as np
import pytest

import cls_ref as CR
import gpnt_ref as GR
from oracle import gpt_sgld_ref as R

pytestmark = pytest.mark.gpu

EPS = CR.EPS


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def run_single(case, idx, seed, eps=None):
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, e0 = CR.sampler_inputs(case, idx)
    return G().GPNT_SGLDclass(phi, y, sth, m, e0 if eps is None else eps, decay, burnin, maxepoch,
                              seed)


# ----------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("idx", range(len(CR.SAMPLER_CASES)),
                         ids=[CR.case_name(c) for c in CR.SAMPLER_CASES])
def test_sampler_matches_the_restatement(idx):
    case = CR.SAMPLER_CASES[idx]
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, eps = CR.sampler_inputs(case, idx)
    got = G().GPNT_SGLDclass(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
    want = CR.gpnt_sgld_class(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
    assert got.shape == want.shape == (n, C, (burnin + maxepoch) * (-(-N // m)))
    print("%s: rel = %.3g" % (CR.case_name(case), CR.rel(got, want)))
    assert CR.rel(got, want) < 1e-9, CR.rel(got, want)


def test_chains_equal_single_runs_bit_for_bit():
    case = CR.SAMPLER_CASES[0]
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, _ = CR.sampler_inputs(case, 0)
    seeds, epss = [5, 11, 5], [2e-3, 1e-3, 4e-3]
    store, status = G().GPNT_SGLDclass_chains(phi, y, sth, m, epss, decay, burnin, maxepoch, seeds)
    assert not status.any()
    for k in range(3):
        assert np.array_equal(store[..., k], run_single(case, 0, seeds[k], epss[k])), k
    nb = -(-N // m)
    ends, status = G().GPNT_SGLDclass_chains(phi, y, sth, m, epss, decay, burnin, maxepoch, seeds,
                                             store_every=nb)
    assert not status.any() and ends.shape == (n, C, burnin + maxepoch, 3)
    assert np.array_equal(ends, store[:, :, nb - 1::nb, :])


def test_nan_chain_is_zero_filled_and_leaves_its_siblings(capsys):
    from gpt_amd import _lib
    case = CR.SAMPLER_CASES[0]
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, _ = CR.sampler_inputs(case, 0)
    seeds, epss = [5, 6, 7], [2e-3, 1e300, 1e-3]
    store, status = G().GPNT_SGLDclass_chains(phi, y, sth, m, epss, decay, burnin, maxepoch, seeds)
    assert list(status) == [0, _lib.GPT_ERR_NAN_THETA, 0]
    assert not store[..., 1].any()
    for k in (0, 2):
        assert np.array_equal(store[..., k], run_single(case, 0, seeds[k], epss[k])), k
    capsys.readouterr()
    out = run_single(case, 0, 6, 1e300)
    assert out.shape == (n,) and not out.any()
    assert "Get NaN in theta. Try smaller epsilon" in capsys.readouterr().out


# -------------------------------------------------------------------------- evaluation kernel
def check_rows(nlp_got, nlp_mp, E, what):
    err = np.array([abs(float(g - w)) for g, w in zip(nlp_got, nlp_mp)])
    ratio = float((err / E).max())
    assert (err <= E).all(), (what, ratio)
    return ratio


def check_mean(got, nlp_mp, E, what, extra=0.0):
    bound = CR.mean_bound(E, nlp_mp) + extra
    err = abs(float(got - CR.mp_mean(nlp_mp)))
    assert err <= bound, (what, err / bound)
    return err / bound


@pytest.mark.parametrize("scale", CR.EVAL_SCALES)
@pytest.mark.parametrize("shape", CR.EVAL_SHAPES, ids=CR.case_name)
def test_evaluation_kernel_per_sample(shape, scale):
    """Every sample against mpmath: the miss count exactly, mean_nlp within the mean bound, the
    rows' nlp (the optional output of a one-sample call) within E_i; and the figures of sample t
    bit for bit the same from the call on all T samples and from the call on sample t alone."""
    Nt, C, T = shape
    s, y, per = CR.eval_reference(shape, scale)
    ev = G().class_eval(s, y)
    wr = wm = 0.0
    for t, (pred, nlp, E) in enumerate(per):
        assert ev.prop_missed[t] == 1 - np.sum(pred == y) / Nt, t
        wm = max(wm, check_mean(ev.mean_nlp[t], nlp, E, t))
        one = G().class_eval(s[:, :, t], y)
        assert one.prop_missed[0] == ev.prop_missed[t] and one.mean_nlp[0] == ev.mean_nlp[t]
        assert np.array_equal(one.mean_fhat, s[:, :, t])          # the mean of one sample is exact
        assert np.array_equal(one.prediction, pred)
        assert (one.avg_prop_missed, one.avg_mean_nlp) == (ev.prop_missed[t], ev.mean_nlp[t])
        wr = max(wr, check_rows(one.nlp, nlp, E, t))
    print("eval %s scale %g: worst row error / E = %.3f, worst mean error / bound = %.4f" % (
        CR.case_name(shape), scale, wr, wm))


@pytest.mark.parametrize("scale", CR.EVAL_SCALES)
@pytest.mark.parametrize("shape", CR.EVAL_SHAPES, ids=CR.case_name)
def test_evaluation_kernel_windows(shape, scale):
    """mean_scores within W·eps·mean|x| of the window's mean; prediction, miss rate and nlp of the
    averaged scores against mpmath on the restated mean, rows whose top-two gap there is below
    1e-9·(1 + max|mean|) left out (at most 1 %; the cases have none, tests/test_cls_ref.py)."""
    Nt, C, T = shape
    s, y = CR.eval_scores(shape, scale, plant=T > 1)
    for window in CR.eval_windows(T):
        W = window[1] - window[0]
        ev = G().class_eval(s, y, window=window)
        mean = CR.window_mean(s, window)
        tol = W * EPS * np.abs(s[:, :, window[0]:window[1]]).mean(axis=2)
        assert (np.abs(ev.mean_fhat - mean) <= tol).all(), window
        keep = CR.top_two_gap(mean) >= 1e-9 * (1 + np.abs(mean).max())
        assert (~keep).sum() <= 0.01 * Nt
        pred, nlp = CR.rows_eval_mp(mean, y)
        assert np.array_equal(ev.prediction[keep], pred[keep]), window
        if keep.all():
            assert ev.avg_prop_missed == 1 - np.sum(pred == y) / Nt, window
        d = 2 * tol.max(axis=1)
        E = CR.row_bound(ev.mean_fhat, y) + d
        check_rows(ev.nlp, nlp, E, window)
        check_mean(ev.avg_mean_nlp, nlp, E, window)
        full = G().class_eval(s, y)                                # the window does not touch these
        assert np.array_equal(full.prop_missed, ev.prop_missed)
        assert np.array_equal(full.mean_nlp, ev.mean_nlp)


def same_figures(a, b):
    return (np.array_equal(a.prop_missed, b.prop_missed) and np.array_equal(a.mean_nlp, b.mean_nlp)
            and a.avg_prop_missed == b.avg_prop_missed and a.avg_mean_nlp == b.avg_mean_nlp
            and np.array_equal(a.mean_fhat, b.mean_fhat) and np.array_equal(a.nlp, b.nlp)
            and np.array_equal(a.prediction, b.prediction))


def test_device_pointer_evaluation_equals_the_host_form():
    """gpt_class_eval_dev on torch tensors, required outputs only and with the optional ones: the
    same bits as gpt_class_eval; a label outside 1..C on the device is refused."""
    import torch
    from gpt_amd import _lib
    shape = (257, 16, 3)
    Nt, C, T = shape
    s, y = CR.eval_scores(shape, 50.0)
    window = (1, 3)
    ev = G().class_eval(s, y, window=window)
    ds = torch.from_numpy(np.ascontiguousarray(s.T)).cuda()
    dy = torch.from_numpy(y).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    pm, nl, avg = torch.zeros(T, **f64), torch.zeros(T, **f64), torch.zeros(2, **f64)
    ms, nlp = torch.zeros((C, Nt), **f64), torch.zeros(Nt, **f64)
    pr = torch.zeros(Nt, dtype=torch.int32, device="cuda")
    P = lambda t: _lib.C.c_void_p(t.data_ptr())
    for opt in (False, True):
        pm.zero_(); nl.zero_(); avg.zero_()
        _lib.check(_lib.lib().gpt_class_eval_dev(P(ds), P(dy), Nt, C, T, window[0], window[1], P(pm),
                                                 P(nl), P(avg), P(ms) if opt else None,
                                                 P(pr) if opt else None, P(nlp) if opt else None,
                                                 None))
        torch.cuda.synchronize()
        assert np.array_equal(pm.cpu().numpy(), ev.prop_missed)
        assert np.array_equal(nl.cpu().numpy(), ev.mean_nlp)
        assert tuple(avg.cpu().numpy()) == (ev.avg_prop_missed, ev.avg_mean_nlp)
    assert np.array_equal(ms.cpu().numpy().T, ev.mean_fhat)
    assert np.array_equal(pr.cpu().numpy(), ev.prediction)
    assert np.array_equal(nlp.cpu().numpy(), ev.nlp)
    dy[5] = C + 1
    rc = _lib.lib().gpt_class_eval_dev(P(ds), P(dy), Nt, C, T, 0, T, P(pm), P(nl), P(avg), None,
                                       None, None, None)
    assert rc == _lib.GPT_ERR_BAD_DIMS


# ------------------------------------------------------------------------ full-theta evaluation
@pytest.mark.parametrize("dims", [(70, 130, 3, 4), (150, 257, 7, 3), (16, 64, 2, 1), (33, 65, 16, 5),
                                  (20, 70, 32, 3)])
def test_full_theta_evaluation(dims):
    """(n, Ntest, C, T): ragged K, row and column tiles of nt_scores_kernel; the last has S = C·T = 96,
    two column tiles with a ragged second.  Every score is one fma chain over j, so it is held to
    (n + 2)·2^-53·sum_j |phitest[j, i]·theta[j, s]| of the 50-digit dot product (the bound of
    tests/test_gpu_gpnt.py::test_scores_against_mpmath), beside the 1e-13·max|want| of the einsum."""
    n, Nt, C, T = dims
    rng = np.random.default_rng(n + Nt)
    theta = rng.standard_normal((n, C, T))
    phitest = np.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, Nt)))
    y = rng.integers(1, C + 1, Nt)
    window = (T // 2, T)
    ev = G().GPNT_pred_class(theta, phitest, y, window=window, scores=True)
    want = np.einsum("ji,jct->ict", phitest, theta)
    assert ev.scores.shape == (Nt, C, T)
    assert np.abs(ev.scores - want).max() <= 1e-13 * np.abs(want).max()
    smp, mag = GR.scores_mp(phitest, theta.reshape((n, C * T), order="F"))
    got = ev.scores.reshape((Nt, C * T), order="F")
    worst = max(GR.abs_err_mp(got[i, s], smp[i][s]) / ((n + 2) * GR.U * mag[i, s])
                for i in range(Nt) for s in range(C * T))
    print("scores %s: worst error / bound = %.3f" % (dims, worst))
    assert worst <= 1.0
    assert same_figures(ev, G().class_eval(ev.scores, y, window=window))
    cols = [T - 1, 0]
    sub = G().GPNT_pred_class(theta, phitest, y, cols=cols, scores=True)
    assert np.array_equal(sub.scores, ev.scores[:, :, cols])


# --------------------------------------------------------------------------- tensor evaluation
@pytest.mark.parametrize("shape,rows", [((16, 3, 130, 5, 30, 3, 4), False),
                                        ((24, 4, 200, 6, 40, 2, 3), True)])
def test_tensor_evaluation(shape, rows):
    import torch
    from gpt_amd.session import pred_device, pred_last_route
    n, D, Nt, r, Q, C, T = shape
    S = C * T
    rng = np.random.default_rng(Nt)
    w = np.asfortranarray(rng.standard_normal((Q, C, T)))
    U = np.asfortranarray(rng.standard_normal((n, r, D, C, T)) / np.sqrt(n))
    I = R.samplenz(r, D, Q, 3)
    phitest = np.asfortranarray(rng.standard_normal((n, D, Nt)) * 0.7)
    y = rng.integers(1, C + 1, Nt)
    window = (1, T)
    ev = G().pred_class(w, U, I, phitest, y, window=window, scores=True)
    kind = pred_last_route()["kind"]
    assert (kind in (1, 2)) if rows else (kind == 0), kind

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).cuda()
    out = torch.full((S, Nt), float("nan"), dtype=torch.float64, device="cuda")
    dw, dU, dI, dphi = dev(w), dev(U), dev((I - 1).astype(np.int32)), dev(phitest)
    pred_device(dw.data_ptr(), dU.data_ptr(), dI, dphi, n, D, Nt, r, Q, S, out)
    torch.cuda.synchronize()
    assert pred_last_route()["kind"] == kind
    f = out.cpu().numpy().T.reshape((Nt, C, T), order="F")
    assert np.array_equal(ev.scores, f)
    assert same_figures(ev, G().class_eval(ev.scores, y, window=window))


def test_tensor_classifier_end_to_end():
    """GPTclassification on the small problem of tests/test_gpu_parity.py's CLS_CASES, two
    epochs, evaluated at the epoch ends against R.pred on the device's own (w, U) plus the
    restated evaluation: scores at 1e-12·max|f|, figures at the bounds with that score error."""
    from test_gpu_parity import CLS_CASES, make_problem
    n, D, N, r, Q, m, ncls, burnin, maxepoch, lang, stf = CLS_CASES["binary_sgld_stiefel"]
    p = make_problem(n, D, N, r, Q, seed=23)
    f = p["y"] - np.median(p["y"])
    y = (1 + np.clip(np.floor((f - f.min()) / (np.ptp(f) + 1e-12) * ncls), 0, ncls - 1)).astype(int)
    ws, Us = G().GPTclassification(p["phi"], y.astype(float), p["I"], r, Q, m, 1e-4, 1e-6, burnin,
                                   maxepoch, 41)
    nb = -(-N // m)
    cols = [nb * e - 1 for e in range(1, maxepoch + 1)]
    ev = G().pred_class(ws, Us, p["I"], p["phi"], y, cols=cols, scores=True)
    want = np.empty((N, ncls, len(cols)))
    for k, col in enumerate(cols):
        for c in range(ncls):
            want[:, c, k] = R.pred(ws[:, c, col], Us[:, :, :, c, col], p["I"], p["phi"])
    d = 1e-12 * np.abs(want).max()
    assert np.abs(ev.scores - want).max() <= d
    ref = CR.class_eval_np(want, y)
    for k in range(len(cols)):
        assert CR.top_two_gap(want[:, :, k]).min() > 2 * d        # no prediction can flip
        assert ev.prop_missed[k] == ref["prop_missed"][k]
        pred, nlp = CR.rows_eval_mp(want[:, :, k], y)
        check_mean(ev.mean_nlp[k], nlp, CR.row_bound(want[:, :, k], y) + 2 * d, k)
    assert CR.top_two_gap(ref["mean_fhat"]).min() > 2 * d
    assert ev.avg_prop_missed == ref["avg_prop_missed"]
    assert np.array_equal(ev.prediction, ref["prediction"])
    pred, nlp = CR.rows_eval_mp(ref["mean_fhat"], y)
    check_mean(ev.avg_mean_nlp, nlp, CR.row_bound(ref["mean_fhat"], y) + 2 * d + 2 * len(cols) * EPS *
               np.abs(want).max(), "window")


# -------------------------------------------------------------------------------- segment data
def test_segment_data_experiment():
    """ImageNoTensorExperiment.jl's configuration (n = 150, m = 50, eps_theta = 0.001, seed 2,
    features of seed 17) for 2 + 10 epochs: theta_store at 1e-9, then the ten epoch ends with the
    last five as the window.  For orientation the restatement's miss rate is about 0.14 after
    epoch 1 and 0.06 after epoch 6; nothing but equality with the restatement is asserted."""
    c = CR.SEG
    Xtr, ytr, Xte, yte = CR.segment_problem()
    phitr = G().featureNotensor_seeded(Xtr, c["n"], CR.SEG_LS, CR.SEG_SIGMA_RBF, c["feature_seed"])
    phite = G().featureNotensor_seeded(Xte, c["n"], CR.SEG_LS, CR.SEG_SIGMA_RBF, c["feature_seed"])
    args = (c["sigma_theta"], c["m"], c["eps_theta"], c["decay_rate"], c["burnin"], c["maxepoch"],
            c["seed"])
    got = G().GPNT_SGLDclass(phitr, ytr, *args)
    want = CR.gpnt_sgld_class(phitr, ytr, *args)
    assert got.shape == want.shape == (150, 7, 312)
    print("segment: theta_store rel = %.3g" % CR.rel(got, want))
    assert CR.rel(got, want) < 1e-9
    nb = 26
    cols = [nb * e - 1 for e in range(c["burnin"] + 1, c["burnin"] + c["maxepoch"] + 1)]
    window = (5, 10)
    ev = G().GPNT_pred_class(got, phite, yte, cols=cols, window=window)
    sref = np.einsum("ji,jct->ict", phite, want[:, :, cols])
    ref = CR.class_eval_np(sref, yte, window=window)
    Nt = yte.size
    # the 1e-9 parity of theta moves a score of row i by at most 1e-9·max|theta|·|phitest[:, i]|_1
    d = 1e-9 * np.abs(want).max() * np.abs(phite).sum(axis=0)
    worst = 0.0
    for k in range(len(cols)):
        out = int((CR.top_two_gap(sref[:, :, k]) < 1e-6).sum())
        assert out <= 0.01 * Nt
        assert abs(ev.prop_missed[k] - ref["prop_missed"][k]) <= out / Nt + (0 if out == 0 else EPS)
        pred, nlp = CR.rows_eval_mp(sref[:, :, k], yte)
        worst = max(worst, check_mean(ev.mean_nlp[k], nlp, CR.row_bound(sref[:, :, k], yte) + 2 * d, k))
    out = int((CR.top_two_gap(ref["mean_fhat"]) < 1e-6).sum())
    assert out <= 0.01 * Nt
    assert abs(ev.avg_prop_missed - ref["avg_prop_missed"]) <= out / Nt + (0 if out == 0 else EPS)
    pred, nlp = CR.rows_eval_mp(ref["mean_fhat"], yte)
    check_mean(ev.avg_mean_nlp, nlp, CR.row_bound(ref["mean_fhat"], yte) + 2 * d + 2 * 5 * EPS *
               np.abs(sref).max(), "window")
    print("segment: prop_missed %s, mean_nlp %s, window %.4f / %.4f, worst mean error / bound %.3g" % (
        np.round(ev.prop_missed, 4), np.round(ev.mean_nlp, 4), ev.avg_prop_missed, ev.avg_mean_nlp,
        worst))
