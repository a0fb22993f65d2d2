"""Device tests of Hamiltonian Monte Carlo on the resident theta of the softmax classifier
(gpt_amd/csrc/chmc.hip) against the numpy restatement of tests/chmc_ref.py.

A device decision is compared with the restatement's only where the restatement's own margin
|log u - (H0 - H1)| is at least chmc_ref.MARGIN_MIN on every transition; each parity case asserts
that first, from the restatement alone.  Tolerances: theta within cls_ref.rel < 1e-9, the bar
test_langevin_steps holds the Langevin step to; dH and value within 1e-9 * max(|H0|, 1).
"""
import numpy as np
import pytest

import chmc_ref as H
import cjoint_ref as CR
import cls_ref as CLS

pytestmark = pytest.mark.gpu

TOL = 1e-9


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def joint_of(g, theta=None):
    j = G().SoftmaxJoint(g["X"], g["y"], g["Z"], g["b"], C=g["theta"].shape[1])
    if theta is not None:
        j.set_theta(theta)
    return j


def same(a, b):
    """Equal bits in every field of two HMCResults."""
    return (np.array_equal(a.theta_store, b.theta_store) and np.array_equal(a.accept, b.accept)
            and np.array_equal(a.dH, b.dH) and np.array_equal(a.value, b.value))


def joined(parts):
    return (np.concatenate([p.theta_store for p in parts], axis=2),
            np.concatenate([p.accept for p in parts]), np.concatenate([p.dH for p in parts]),
            np.concatenate([p.value for p in parts]))


def fields(r):
    return r.theta_store, r.accept, r.dH, r.value


def equal_fields(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("idx,L,eps", H.PARITY, ids=lambda v: str(v))
def test_trajectory_parity(idx, L, eps):
    g, theta0, h, want = H.run(idx, L, eps, 3)
    assert want["margin"].min() >= H.MARGIN_MIN, want["margin"]
    j = joint_of(g, theta0)
    got = j.hmc(h, eps, L, 3, H.SEED, t0=0)
    assert j.steps == 3 and got.theta_store.shape == theta0.shape + (3,)
    scale = np.maximum(np.abs(want["H0"]), 1.0)
    e_th = CLS.rel(got.theta_store, want["store"])
    e_dh = (np.abs(got.dH - want["dH"]) / scale).max()
    e_val = (np.abs(got.value - want["value"]) / scale).max()
    print("hmc %s L=%d: accept %s, theta rel %.3g, dH err %.3g, value err %.3g (of |H0| ~ %.3g)"
          % (CR.case_name(CR.CASES[idx]), L, got.accept, e_th, e_dh, e_val, scale.max()))
    assert np.array_equal(got.accept, want["accept"])
    assert e_th < TOL and e_dh <= TOL and e_val <= TOL
    assert np.array_equal(j.theta(), got.theta_store[:, :, -1])
    assert got.ndivergent == 0 and got.accept_rate == want["accept"].mean()
    assert CLS.rel(got.theta_store[:, :, 0], theta0) > 1e-3                 # it moved
    again = joint_of(g, theta0).hmc(h, eps, L, 3, H.SEED, t0=0)             # equal inputs, equal bits
    assert same(got, again)
    other = joint_of(g, theta0).hmc(h, eps, L, 3, H.SEED + 1, t0=0)
    assert not np.array_equal(other.theta_store, got.theta_store)


def test_mala_is_hmc_with_one_step_and_the_oneshot_entry_agrees():
    g, theta0, h, _ = H.run(0, 1, 1e-2, 3)
    a = joint_of(g, theta0).hmc(h, 1e-2, 1, 3, H.SEED, t0=0)
    b = joint_of(g, theta0).mala(h, 1e-2, 3, H.SEED, t0=0)
    assert same(a, b)
    th, c = G().gpnt_joint_hmc_oneshot(g["X"], g["y"], g["Z"], g["b"], theta0, h, 1e-2, 1, 3, H.SEED,
                                       C=theta0.shape[1])
    assert same(a, c) and np.array_equal(th, a.theta_store[:, :, -1])


def test_both_outcomes():
    c = H.BOTH
    g, theta0, h, want = H.run(c["idx"], c["L"], c["eps"], c["ntrans"], c["scale"])
    assert want["margin"].min() >= H.MARGIN_MIN and 0 < want["accept"].sum() < c["ntrans"]
    j = joint_of(g, theta0)
    got = j.hmc(h, c["eps"], c["L"], c["ntrans"], H.SEED, t0=0)
    print("both outcomes: accept %s, theta rel %.3g" % (got.accept, CLS.rel(got.theta_store, want["store"])))
    assert np.array_equal(got.accept, want["accept"])
    k = int(np.flatnonzero(got.accept == 0)[0])
    assert k > 0
    assert np.array_equal(got.theta_store[:, :, k], got.theta_store[:, :, k - 1])
    assert got.value[k] == got.value[k - 1]
    assert not np.array_equal(got.theta_store[:, :, k + 1], got.theta_store[:, :, k])
    assert got.accept_rate == 11 / 12


def test_rejections_keep_theta():
    c = H.ALL_REJECTED
    g, theta0, h, want = H.run(c["idx"], c["L"], c["eps"], c["ntrans"], c["scale"])
    assert want["margin"].min() >= H.MARGIN_MIN and not want["accept"].any()
    j = joint_of(g, theta0)
    got = j.hmc(h, c["eps"], c["L"], c["ntrans"], H.SEED, t0=0)
    print("all rejected: dH %.3f .. %.3f" % (got.dH.min(), got.dH.max()))
    assert not got.accept.any() and got.accept_rate == 0 and got.ndivergent == 0
    assert np.array_equal(j.theta(), theta0)
    for k in range(c["ntrans"]):
        assert np.array_equal(got.theta_store[:, :, k], theta0)
    assert (got.value == got.value[0]).all()
    assert (np.abs(got.dH - want["dH"]) <= TOL * np.maximum(np.abs(want["H0"]), 1.0)).all()


@pytest.mark.parametrize("idx", [0, 4])
def test_integrator(idx):
    g = H.golden_case(idx)
    h, eps, L = g["H"][H.POINT], 1e-2, 4
    n, C = g["theta"].shape
    p0 = H.momentum(n, C, 3, 0)
    wq, wp, wH0, wH1, _, _ = H.leapfrog(g["X"], g["y"], g["Z"], g["b"], g["theta"], h, eps, L, p0)
    j = joint_of(g, g["theta"])
    q, p1, H0, H1 = j.leapfrog(h, eps, L, p0)
    errs = (CLS.rel(q, wq), CLS.rel(p1, wp), abs(H0 - wH0) / max(abs(wH0), 1), abs(H1 - wH1) / max(abs(wH0), 1))
    print("leapfrog %s: q %.3g, p %.3g, H0 %.3g, H1 %.3g" % ((CR.case_name(CR.CASES[idx]),) + errs))
    assert max(errs) < TOL
    assert np.array_equal(j.theta(), g["theta"])                       # the resident theta stays
    q2, p2, K0, K1 = j.leapfrog(h, eps, L, p0)                          # and so does the result
    assert np.array_equal(q, q2) and np.array_equal(p1, p2) and (H0, H1) == (K0, K1)
    j.set_theta(q)
    back, pb, B0, B1 = j.leapfrog(h, eps, L, -p1)
    assert CLS.rel(back, g["theta"]) < TOL and CLS.rel(-pb, p0) < TOL
    assert abs(B0 - H1) <= TOL * abs(H1) and abs(B1 - H0) <= TOL * abs(H0)
    assert np.array_equal(j.theta(), q)


def test_cuts_and_the_cache():
    idx, L, eps = 4, 3, 1e-2
    g = H.golden_case(idx)
    th0, h1, h2 = g["theta"], g["H"][1], g["H"][2]
    whole = fields(joint_of(g, th0).hmc(h1, eps, L, 6, H.SEED, t0=0))
    j = joint_of(g, th0)
    ones = [j.hmc(h1, eps, L, 1, H.SEED, t0=0)] + [j.hmc(h1, eps, L, 1, H.SEED) for _ in range(5)]
    assert j.steps == 6 and equal_fields(joined(ones), whole)
    j = joint_of(g, th0)
    assert equal_fields(joined([j.hmc(h1, eps, L, 2, H.SEED, t0=0), j.hmc(h1, eps, L, 4, H.SEED)]), whole)
    # set_theta(theta()) in between drops the cache: U and grad U are recomputed to the same bits
    j = joint_of(g, th0)
    a = j.hmc(h1, eps, L, 2, H.SEED, t0=0)
    j.set_theta(j.theta())
    assert equal_fields(joined([a, j.hmc(h1, eps, L, 4, H.SEED)]), whole)
    # another hyper point: from the second part on, a fresh handle started at that theta with h2
    j = joint_of(g, th0)
    j.hmc(h1, eps, L, 2, H.SEED, t0=0)
    mid = j.theta()
    b = j.hmc(h2, eps, L, 3, H.SEED)
    fresh = joint_of(g, mid).hmc(h2, eps, L, 3, H.SEED, t0=2)
    assert same(b, fresh) and not np.array_equal(b.theta_store, whole[0][:, :, 2:5])
    # and back at h1, the cache of h2 is not used
    c = j.hmc(h1, eps, L, 2, H.SEED)
    assert same(c, joint_of(g, b.theta_store[:, :, -1]).hmc(h1, eps, L, 2, H.SEED, t0=5))
    # a langevin call in between moves theta and the counter; the run after it starts from there
    j = joint_of(g, th0)
    j.hmc(h1, eps, L, 2, H.SEED, t0=0)
    j.langevin(h1, 2e-3, 1, H.SEED)
    mid = j.theta()
    d = j.hmc(h1, eps, L, 2, H.SEED)
    assert j.steps == 5
    assert same(d, joint_of(g, mid).hmc(h1, eps, L, 2, H.SEED, t0=3))
    # an evaluation with a theta makes that theta resident; one without leaves the cache valid
    j = joint_of(g, th0)
    j.hmc(h1, eps, L, 2, H.SEED, t0=0)
    j.neglogjointlkhd(None, h2)
    j.gradneglogjointlkhd(None, h2)
    assert equal_fields(joined([a, j.hmc(h1, eps, L, 4, H.SEED)]), whole)
    j.neglogjointlkhd(th0, h1)
    assert equal_fields(fields(j.hmc(h1, eps, L, 6, H.SEED, t0=0)), whole)


def test_thinning_and_burn_in():
    idx, L, eps = 0, 2, 1e-2
    g = H.golden_case(idx)
    h = g["H"][H.POINT]
    full = joint_of(g, g["theta"]).hmc(h, eps, L, 9, H.SEED, t0=0)
    thin = joint_of(g, g["theta"]).hmc(h, eps, L, 7, H.SEED, burnin=2, thin=3, t0=0)
    assert thin.theta_store.shape[2] == 2 and thin.accept.size == 9
    after = full.theta_store[:, :, 2:]
    assert np.array_equal(thin.theta_store, after[:, :, 2:7:3])        # columns 2 and 5 past burn-in
    assert np.array_equal(thin.accept, full.accept) and np.array_equal(thin.dH, full.dH)
    assert np.array_equal(thin.value, full.value)
    last = joint_of(g, g["theta"])
    kept = last.hmc(h, eps, L, 1, H.SEED, burnin=8, t0=0)               # the E step's form
    assert np.array_equal(kept.theta_store[:, :, 0], full.theta_store[:, :, 8])
    assert np.array_equal(last.theta(), full.theta_store[:, :, 8])
    none = joint_of(g, g["theta"]).hmc(h, eps, L, 0, H.SEED, t0=0)
    assert none.theta_store.shape[2] == 0 and none.accept.size == 0


def test_divergence_and_errors():
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPT_ERR_NAN_THETA, GPTError
    c = H.DIVERGENT
    g, theta0, h, want = H.run(c["idx"], c["L"], c["eps"], c["ntrans"])
    assert want["divergent"].all()
    j = joint_of(g, theta0)
    got = j.hmc(h, c["eps"], c["L"], c["ntrans"], H.SEED, t0=0)           # no exception: GPT_OK
    assert not got.accept.any() and got.ndivergent == c["ntrans"]
    assert np.array_equal(j.theta(), theta0)
    for k in range(c["ntrans"]):
        assert np.array_equal(got.theta_store[:, :, k], theta0)
    ok = j.hmc(h, 1e-2, 1, 2, H.SEED, t0=0)                               # the handle goes on
    assert same(ok, joint_of(g, theta0).hmc(h, 1e-2, 1, 2, H.SEED, t0=0))

    bad = theta0.copy()
    bad[3, 1] = np.inf
    j.set_theta(bad)
    with pytest.raises(GPTError) as ei:
        j.hmc(h, 1e-2, 2, 2, H.SEED, t0=0)
    assert ei.value.code == GPT_ERR_NAN_THETA
    with pytest.raises(GPTError) as ei:
        j.leapfrog(h, 1e-2, 2, np.zeros_like(theta0))
    assert ei.value.code == GPT_ERR_NAN_THETA
    j.set_theta(theta0)
    assert same(j.hmc(h, 1e-2, 1, 2, H.SEED, t0=0), ok)

    t_before, th_before = j.steps, j.theta()
    calls = [dict(eps=0.0), dict(eps=-1e-2), dict(eps=np.inf), dict(eps=np.nan), dict(L=0),
             dict(L=1025), dict(thin=0), dict(nsamples=-1), dict(burnin=-1),
             dict(t0=2 ** 32 - 1), dict(h=np.append(h[:-1], 0.0)), dict(h=h[:-1][:1]),
             dict(h=np.append(h[:-1], np.nan))]
    for kw in calls:
        a = dict(h=h, eps=1e-2, L=2, nsamples=2, seed=H.SEED, burnin=0, thin=1, t0=0)
        a.update(kw)
        with pytest.raises(GPTError) as ei:
            j.hmc(a["h"], a["eps"], a["L"], a["nsamples"], a["seed"], burnin=a["burnin"],
                  thin=a["thin"], t0=a["t0"])
        assert ei.value.code == GPT_ERR_BAD_DIMS, kw
    for kw in (dict(eps=0.0), dict(L=0), dict(L=1025)):
        a = dict(eps=1e-2, L=2)
        a.update(kw)
        with pytest.raises(GPTError) as ei:
            j.leapfrog(h, a["eps"], a["L"], np.zeros_like(theta0))
        assert ei.value.code == GPT_ERR_BAD_DIMS, kw
    assert j.steps == t_before and np.array_equal(j.theta(), th_before)     # refused before any work


def planted():
    """N = 400, D = 2, C = 3, n = 64: labels drawn from the softmax of a planted theta at l = 1,
    sigma = 2 (the problem of test_gpu_cjoint.py's stochastic EM tests)."""
    rng = np.random.default_rng(12)
    N, D, C, n = 400, 2, 3, 64
    X, Z, b = rng.standard_normal((N, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    theta = rng.standard_normal((n, C))
    phi = CR.NR.feature_notensor(X, np.ones(D), 2.0, Z, b)
    s = (theta.T @ phi).T
    P = np.exp(s - s.max(axis=1, keepdims=True))
    P /= P.sum(axis=1, keepdims=True)
    y = np.array([rng.choice(C, p=P[i]) + 1 for i in range(N)], dtype=np.float64)
    return X, y, Z, b, C, n


def test_stochastic_em_with_the_hmc_e_step():
    pytest.importorskip("scipy")
    from scipy.optimize import minimize
    X, y, Z, b, C, n = planted()
    init = [3.0, 3.0, 1.0]
    kw = dict(epsilon=1e-2, num_sgld_iter=4, num_cg_iter=5, seed=4, max_iter=2, tol=0.0)
    j = G().SoftmaxJoint(X, y, Z, b, C=C)
    got = G().GPNT_hyperparameters_ng(np.zeros(n * C), init, j.neglogjointlkhd, j.gradneglogjointlkhd,
                                      Z, b, e_step="hmc", num_leapfrog=3, **kw)
    theta_got = j.theta()

    k = G().SoftmaxJoint(X, y, Z, b, C=C)                  # the same two rounds by hand
    k.set_theta(np.zeros(n * C))
    lh = np.log(np.array(init))

    def fun(x):
        hx = np.exp(x)
        val, gh = k.hyper_value_and_grad(hx)
        return val, gh * hx
    rates = []
    for r in range(2):
        res = k.hmc(np.exp(lh), 1e-2, 3, 1, 4, burnin=3, t0=4 * r)
        rates.append(res.accept_rate)
        lh = np.asarray(minimize(fun, lh, jac=True, method="CG", options={"maxiter": 5}).x)
    print("EM with hmc: accept rates %s, h %s" % (rates, np.exp(lh)))
    assert np.array_equal(got, np.exp(lh)) and np.array_equal(theta_got, k.theta())
    assert k.steps == 8 and theta_got.any()

    # e_step="langevin" is the call without the argument
    a = G().SoftmaxJoint(X, y, Z, b, C=C)
    ha = G().GPNT_hyperparameters_ng(np.zeros(n * C), init, a.neglogjointlkhd, a.gradneglogjointlkhd,
                                     Z, b, **kw)
    c = G().SoftmaxJoint(X, y, Z, b, C=C)
    hc = G().GPNT_hyperparameters_ng(np.zeros(n * C), init, c.neglogjointlkhd, c.gradneglogjointlkhd,
                                     Z, b, e_step="langevin", **kw)
    assert np.array_equal(ha, hc) and np.array_equal(a.theta(), c.theta())
    assert not np.array_equal(ha, got)
    with pytest.raises(ValueError):
        G().GPNT_hyperparameters_ng(np.zeros(n * C), init, c.neglogjointlkhd, c.gradneglogjointlkhd,
                                    Z, b, e_step="nuts")
