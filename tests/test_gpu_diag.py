"""The chain diagnostics on the device (gpt_amd/csrc/diag.hip) against the mpmath reference and the
yardsticks of tests/diag_ref.py, their independence of everything but a parameter's (and a chain's)
own values, bit for bit, the sampler routes, and the device-tensor entry.

Bar of every quantity (error relative to the column's max |value|; acf and chain_acf in units of
rho): max(8 × the numpy restatement's own error against mpmath, (S + 16)·2^-53); tests/
test_diag_ref.py holds the restatement itself.  truncated, the Geyer stop index and the NaN rows are
compared exactly.  Measured on the MI355X, device error / bar (numpy's error in units of 2^-53 in
brackets):

    case           mean           sd             rhat           ess            mcse           tau            chain_mean     chain_var      acf            chain_acf
    antithetic     0.0115 (2.48)  0.0148 (3.2)   0.00405 (0.876)0.103 (22.2)   0.0555 (12.7)  0.0954 (21.4)  0.0176 (3.81)  0.0361 (7.8)   0.0267 (4.5)   0.0264 (5.71)
    constant_row   0.00499 (0.28) 0.0356 (2)     0.0193 (1.08)  0.125 (7.67)   0.0784 (4.39)  0.11 (6.16)    0.00836 (0.468)0.049 (2.89)   0.107 (5.99)   0.0786 (4.4)
    k_3groups      0.0192 (2.99)  0.0133 (1.95)  0.00555 (0.865)0.0437 (7.27)  0.032 (4.99)   0.0387 (7.3)   0.0223 (3.48)  0.0305 (4.8)   0.025 (3.89)   0.0387 (5.52)
    k_kb           0.0273 (2.18)  0.0232 (1.86)  0.0104 (0.833) 0.0627 (3.44)  0.0388 (3.01)  0.0391 (4.55)  0.0285 (2.28)  0.0525 (3.77)  0.0374 (2.48)  0.0519 (3.15)
    k_kg           0.0367 (4.26)  0.0142 (1.65)  0.00691 (0.801)0.0673 (7.81)  0.11 (12.7)    0.125 (23.9)   0.0169 (1.96)  0.0257 (2.98)  0.0297 (3.44)  0.03 (3.48)
    k_kg+1         0.029 (3.36)   0.0189 (2.19)  0.00814 (0.944)0.0545 (6.32)  0.0215 (2.51)  0.0298 (5.45)  0.0232 (2.69)  0.0424 (4.92)  0.0328 (3.54)  0.0299 (3.54)
    offset         0.0396 (3.21)  0.02 (1.69)    0.0236 (1.91)  0.0545 (4.42)  0.0251 (2.03)  0.0356 (5.7)   0.0607 (4.92)  0.0211 (2.35)  0.0293 (2.34)  0.0352 (3.33)
    p1_s4_k1       0.049 (0.981)  0.0128 (0.255) 0.0796 (1.59)  0.00419 (0.0839)0.00874 (0.175)0.0225 (0.451) 0.049 (0.981)  0.0095 (0.19)  0.0709 (1.42)  0.0069 (0.138)
    p257_s65_kb-1  0.0343 (2.78)  0.0436 (3.53)  0.0194 (1.57)  0.063 (5.1)    0.031 (2.46)   0.0463 (4.55)  0.0343 (2.78)  0.0612 (4.96)  0.0722 (4.83)  0.0772 (5.25)
    p3_m64         0.0809 (5.18)  0.0197 (1.26)  0.00772 (0.494)0.051 (3.26)   0.0241 (1.84)  0.0439 (3.07)  0.0478 (3.06)  0.062 (3.97)   0.0441 (2.5)   0.063 (4.03)
    p63_s5         0.0429 (0.9)   0.0689 (1.45)  0.125 (3.1)    0.125 (6.7)    0.0895 (1.88)  0.0849 (1.78)  0.0581 (1.22)  0.125 (2.72)   0.125 (4.67)   0.0864 (2.47)
    p65_s200_trunc 0.0347 (7.49)  0.022 (4.75)   0.0108 (2.34)  0.0268 (7.5)   0.0422 (10.6)  0.0504 (11.3)  0.0337 (7.28)  0.0516 (10.1)  0.0612 (12.2)  0.0847 (16.3)
    p65_s64_halo   0.0486 (3.89)  0.0208 (2.08)  0.0177 (1.41)  0.125 (15.4)   0.0785 (6.28)  0.096 (7.56)   0.0518 (4.14)  0.0399 (3.19)  0.0792 (6.34)  0.0513 (4.37)
    s_tc+1_keven   0.0469 (2.3)   0.00644 (0.316)0.013 (0.636)  0.0675 (3.49)  0.0313 (1.54)  0.0575 (2.82)  0.0469 (2.3)   0.0201 (0.706) 0.0358 (1.75)  0.0347 (1.7)
    s_tc-1_kb+1    0.0441 (2.07)  0.0471 (1.22)  0.0135 (0.636) 0.125 (7.45)   0.15 (7.41)    0.125 (12.3)   0.0364 (1.71)  0.0364 (2.96)  0.0887 (3.44)  0.0369 (2.74)
    s_tc_kfull     0.0482 (2.31)  0.0337 (1.62)  0.0263 (1.26)  0.0613 (2.94)  0.0375 (1.8)   0.0268 (1.29)  0.0404 (1.94)  0.0717 (3.44)  0.0492 (2.24)  0.0745 (3.58)
    shifted_chain  0.0361 (4.19)  0.0165 (1.92)  0.0106 (1.23)  0.0511 (5.93)  0.0371 (4.31)  0.0435 (4.53)  0.0391 (4.54)  0.0461 (5.35)  0.0269 (3.95)  0.0238 (2.69)
    window         0.0394 (3.15)  0.0445 (3.56)  0.0164 (1.31)  0.102 (8.99)   0.125 (17.1)   0.125 (25)     0.0344 (2.75)  0.0462 (3.72)  0.069 (5.52)   0.0313 (2.73)
"""
import numpy as np
import pytest

import diag_ref as DR
import gpnt_ref as GR

pytestmark = pytest.mark.gpu


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def run_case(name, **kw):
    x, window, max_lag = DR.inputs(name)
    return G().chain_diagnostics(x, window=window, max_lag=max_lag, acf=True, chain_acf=True, **kw)


def same_bits(a, b, names=DR.QUANTITIES + ("truncated",)):
    return all(np.array_equal(getattr(a, q), getattr(b, q), equal_nan=True) for q in names)


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_diagnostics_against_mpmath(name):
    pytest.importorskip("mpmath")
    d, ref, ys = run_case(name), DR.reference(name), DR.yardstick(name)
    err = DR.errors(DR.as_dict(d), name)
    print("case %s: device error / bar (numpy error / 2^-53): %s" % (name, ", ".join(
        "%s %.3g (%.3g)" % (q, err[q] / DR.bar(name, q), ys[q] / DR.U) for q in DR.QUANTITIES)))
    assert d.max_lag == ref["K"]
    assert np.array_equal(d.truncated, ref["truncated"])
    assert np.array_equal(DR.stops(d.acf, d.max_lag), ref["stop"])
    for q in DR.QUANTITIES:
        assert err[q] <= DR.bar(name, q), (name, q, err[q] / DR.bar(name, q))
    live = ~np.isnan(d.rhat)
    assert d.n_truncated == int(ref["truncated"].sum())
    assert d.max_rhat == d.rhat[live].max() and d.min_ess == d.ess[live].min()


def test_a_constant_row_is_nan_and_leaves_its_neighbours_alone():
    x, window, max_lag = DR.inputs("constant_row")
    d = run_case("constant_row")
    r = DR.CONST_ROW
    for q in ("rhat", "ess", "mcse", "tau"):
        assert np.isnan(getattr(d, q)[r]) and np.isfinite(np.delete(getattr(d, q), r)).all()
    assert np.isnan(d.acf[r]).all() and np.isnan(d.chain_acf[r]).all()
    assert d.truncated[r] == 0 and d.sd[r] == 0.0 and abs(d.mean[r] - x[r, 0, 0]) <= 4 * DR.U * 3.7
    assert (d.chain_var[r] == 0.0).all()
    live = np.array(x)
    live[r] = DR.ar1(np.random.default_rng(1), 1, x.shape[1], x.shape[2], 0.5)[0]
    e = G().chain_diagnostics(live, window=window, max_lag=max_lag, acf=True, chain_acf=True)
    keep = np.arange(x.shape[0]) != r
    for q in DR.QUANTITIES + ("truncated",):
        assert np.array_equal(getattr(d, q)[keep], getattr(e, q)[keep]), q
    zero = G().chain_diagnostics(np.zeros((3, 8, 1)))       # the store of a NaN-bailed chain alone
    assert np.isnan(zero.rhat).all() and np.isnan(zero.max_rhat) and np.isnan(zero.min_ess)
    assert zero.n_truncated == 0


# --------------------------------------------------------------------------- independence
def test_rows_do_not_depend_on_the_other_rows():
    x, window, max_lag = DR.inputs("p65_s200_trunc")
    full = run_case("p65_s200_trunc")
    part = G().chain_diagnostics(x[:40], window=window, max_lag=max_lag, acf=True, chain_acf=True)
    for q in DR.QUANTITIES + ("truncated",):
        assert np.array_equal(getattr(full, q)[:40], getattr(part, q)), q


def test_rows_do_not_depend_on_where_the_window_sits():
    x, (a, b), max_lag = DR.inputs("window")
    cut = G().chain_diagnostics(np.asfortranarray(x[:, a:b]), max_lag=max_lag, acf=True, chain_acf=True)
    assert same_bits(run_case("window"), cut)


@pytest.mark.parametrize("name,k", [("k_3groups", 20), ("k_3groups", 65), ("p65_s200_trunc", 15)])
def test_acf_does_not_depend_on_max_lag(name, k):
    x, window, _ = DR.inputs(name)
    S = window[1] - window[0]
    runs = [G().chain_diagnostics(x, window=window, max_lag=lag, acf=True, chain_acf=True)
            for lag in (k, 2 * k, S - 1)]
    for d in runs[1:]:
        assert np.array_equal(d.acf[:, :k + 1], runs[0].acf)
        assert np.array_equal(d.chain_acf[:, :k + 1], runs[0].chain_acf)
        assert same_bits(d, runs[0], ("mean", "sd", "rhat", "chain_mean", "chain_var"))


@pytest.mark.parametrize("name", ["s_tc_kfull", "p3_m64"])
def test_a_chain_does_not_depend_on_the_other_chains(name):
    x, window, max_lag = DR.inputs(name)
    full = run_case(name)
    for m in (0, x.shape[2] - 1):
        one = G().chain_diagnostics(x[:, :, m], window=window, max_lag=max_lag, chain_acf=True)
        assert np.array_equal(one.chain_mean[:, 0], full.chain_mean[:, m])
        assert np.array_equal(one.chain_var[:, 0], full.chain_var[:, m])
        assert np.array_equal(one.chain_acf[:, :, 0], full.chain_acf[:, :, m])


def test_a_repeated_call_gives_the_same_bits():
    assert same_bits(run_case("k_3groups"), run_case("k_3groups"))


def test_input_forms_agree():
    x, window, max_lag = DR.inputs("s_tc_kfull")
    kw = dict(window=window, max_lag=max_lag, acf=True, chain_acf=True)
    want = G().chain_diagnostics(x, **kw)
    assert same_bits(G().chain_diagnostics([x[:, :, m] for m in range(x.shape[2])], **kw), want)
    assert same_bits(G().chain_diagnostics(np.ascontiguousarray(x), **kw), want)
    # an HMCResult.theta_store (n, C, T) is one chain whose leading axes are flattened column-major
    th = DR.ar1(np.random.default_rng(2), 12, 40, 1, 0.4)[:, :, 0].reshape((4, 3, 40), order="F")
    a = G().chain_diagnostics([th], acf=True, chain_acf=True)
    b = G().chain_diagnostics(th.reshape((12, 40), order="F"), acf=True, chain_acf=True)
    assert same_bits(a, b) and a.window == (0, 40) and a.max_lag == 39


# --------------------------------------------------------------------------- routes
def close_to_np(d, x, window, max_lag):
    want = DR.diag_np(x, window[0], window[1], max_lag)
    for q in DR.QUANTITIES:
        g, w = getattr(d, q), want[q]
        assert np.array_equal(np.isnan(g), np.isnan(w)), q
        assert np.nanmax(np.abs(g - w)) <= 1e-12 * max(1.0, np.nanmax(np.abs(w))), q
    assert np.array_equal(d.truncated, want["truncated"])


def test_full_theta_route():
    n, N, m, burnin, maxepoch, decay = GR.CASES["A"]
    phi, y = GR.inputs("A")
    store, status = G().GPNT_SGLD_chains(phi, y, GR.SIGNAL_VAR, GR.SIGMA_THETA, m, GR.EPS, decay,
                                         burnin, maxepoch, GR.SEEDS)
    assert not status.any() and store.shape[0] == n and store.shape[2] == 3
    T = store.shape[1]
    window = (T // 3, T)
    d = G().chain_diagnostics(store, window=window, acf=True, chain_acf=True)
    assert d.max_lag == window[1] - window[0] - 1 and d.rhat.shape == (n,)
    close_to_np(d, store, window, d.max_lag)


def test_tensor_route():
    from test_gpu_parity import make_problem
    n, D, N, r, Q, m, burnin, maxepoch = 16, 3, 40, 2, 6, 8, 1, 2     # tests/test_gpu_bigseed.py's
    p = make_problem(n, D, N, r, Q, seed=11)
    res = G().GPTregression_chains(p["phi"], p["y"], 0.05, p["I"], r, Q, m, 1e-4, 1e-6, burnin,
                                   maxepoch, [3, 4])
    assert all(st == 0 for _, _, st in res)
    ws = [w for w, U, st in res]
    d = G().chain_diagnostics(ws, acf=True, chain_acf=True)
    assert d.chain_mean.shape == (Q, 2)
    close_to_np(d, np.stack(ws, axis=2), (0, ws[0].shape[1]), d.max_lag)


# --------------------------------------------------------------------------- device entry
def test_device_entry_equals_the_host_entry():
    import torch
    from gpt_amd.session import diagnostics_device
    x, window, max_lag = DR.inputs("k_3groups")
    want = run_case("k_3groups")
    P, T, M = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 1, 0))).cuda()      # (M, T, P)
    # the same chains at a stride larger than T·P: a view into a padded allocation
    padded = torch.full((M, T + 3, P), float("nan"), dtype=torch.float64, device="cuda")
    padded[:, :T] = xt
    for src in (xt, padded[:, :T]):
        d = diagnostics_device(src, window=window, max_lag=max_lag, acf=True, chain_acf=True)
        for q in DR.ROWS + ("truncated",):
            assert np.array_equal(getattr(d, q).cpu().numpy(), getattr(want, q)), q
        assert np.array_equal(d.chain_mean.cpu().numpy().T, want.chain_mean)
        assert np.array_equal(d.chain_var.cpu().numpy().T, want.chain_var)
        assert np.array_equal(d.acf.cpu().numpy().T, want.acf)
        assert np.array_equal(d.chain_acf.cpu().numpy().transpose(2, 1, 0), want.chain_acf)
        assert (d.max_rhat, d.min_ess, d.n_truncated) == (want.max_rhat, want.min_ess, want.n_truncated)
        assert d.window == want.window and d.max_lag == want.max_lag
    lean = diagnostics_device(xt, window=window, max_lag=max_lag)
    assert lean.acf is None and lean.chain_acf is None
    assert np.array_equal(lean.ess.cpu().numpy(), want.ess)
