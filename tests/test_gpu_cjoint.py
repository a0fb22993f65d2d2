"""GPU tests of the device joint likelihood of the softmax classifier (gpt_amd/csrc/cjoint.hip),
its Langevin step and the stochastic EM driver against the 50-digit golden
tests/golden/cjoint_mp.npz and the fp64 restatements of tests/cjoint_ref.py.

Parity rule (tests/test_gpu_nlml.py's): per hyper-gradient component the device's relative error
against the mp value is at most 32 x the larger of the two fp64 restatements' errors against mp
for that component, with a floor of 1e-12; grad theta goes by the same rule on
max |error| / max |entry|; the value is held to 1e-12 relative.  The yardstick is the
restatements' own error, never the device's.  In the theta-times-40 case the softmax saturates and
hyper-gradient components nearly cancel, so the generator's component rule cannot be expected to
hold: there the errors (the device's and the restatements') are measured against the largest
hyper-gradient component.
"""
import functools

import numpy as np
import pytest

import cjoint_ref as CR
import cls_ref as CLS

pytestmark = pytest.mark.gpu

FLOOR = 1e-12


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@functools.lru_cache(maxsize=None)
def golden():
    return CR.load_golden()


@functools.lru_cache(maxsize=None)
def yard(nm, p, largest):
    return CR.yardstick(golden()[nm], p, largest)


def joint_of(g):
    return G().SoftmaxJoint(g["X"], g["y"], g["Z"], g["b"], C=g["theta"].shape[1])


@pytest.mark.parametrize("case", CR.CASES, ids=CR.case_name)
def test_value_and_gradient_parity(case):
    nm = CR.case_name(case)
    g = golden()[nm]
    n, C = g["theta"].shape
    largest = case[5] == "x40"
    j = joint_of(g)
    for p in range(3):
        h = g["H"][p]
        val, grad = j.value_and_grad(g["theta"].ravel(order="F"), h)
        assert grad.shape == (n * C + h.size,)
        ev = abs(val - g["val"][p]) / abs(g["val"][p])
        eh = CR.hyper_errors(grad[n * C:], g["gh"][p], largest)
        et = CR.theta_error(grad[:n * C].reshape((n, C), order="F"), g["gtheta"][p])
        yh, yt = yard(nm, p, largest)
        bh, bt = np.maximum(32 * yh, FLOOR), max(32 * yt, FLOOR)
        print("%s point %d: value %.2e; hyper worst error %.2e, worst error/bound %.3f; "
              "grad theta error %.2e, error/bound %.3f"
              % (nm, p, ev, eh.max(), (eh / bh).max(), et, et / bt))
        assert ev <= 1e-12, (nm, p, ev)
        assert (eh <= bh).all(), (nm, p, eh, bh)
        assert et <= bt, (nm, p, et, bt)
        # value bits: a value-only evaluation returns those of the gradient evaluation
        assert j.neglogjointlkhd(None, h) == val
        assert np.array_equal(j.gradneglogjointlkhd(None, h), grad)
    j.close()


@pytest.mark.parametrize("idx", [0, 4, 5])
def test_determinism_and_one_shot(idx):
    case = CR.CASES[idx]
    g = golden()[CR.case_name(case)]
    j = joint_of(g)
    h = g["H"][1]
    th = g["theta"].ravel(order="F")
    v1, g1 = j.value_and_grad(th, h)
    j.value_and_grad(None, g["H"][0])                 # other work on the handle in between
    j.scores(g["H"][2], g["X"][:9])
    v2, g2 = j.value_and_grad(None, h)
    assert v1 == v2 and np.array_equal(g1, g2)
    assert np.array_equal(j.theta(), g["theta"])
    v3, g3 = G().gpnt_neglogjoint_oneshot(g["X"], g["y"], g["Z"], g["b"], th, h,
                                          C=g["theta"].shape[1])
    assert v1 == v3 and np.array_equal(g1, g3)
    assert G().gpnt_neglogjoint_oneshot(g["X"], g["y"], g["Z"], g["b"], th, h,
                                        C=g["theta"].shape[1], want_grad=False) == v1
    hv, hg = j.hyper_value_and_grad(h)
    assert hv == v1 and np.array_equal(hg, g1[th.size:])


@pytest.mark.parametrize("n,N,D,form", [(24, 50, 3, "ard"), (32, 131, 16, "ard"), (7, 33, 4, "scalar")])
def test_scores_with_identity_theta_are_the_features(n, N, D, form):
    """theta = identity columns (C = n <= 32): scores equal featureNotensor bit for bit."""
    rng = np.random.default_rng(n + N)
    X, Z, b = rng.standard_normal((N, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    y = (np.arange(N) % n) + 1.0
    j = G().SoftmaxJoint(X, y, Z, b, C=n)
    j.set_theta(np.eye(n))
    ls = np.array([1.3]) if form == "scalar" else 0.5 + rng.random(D)
    h = np.concatenate([ls, [1.7]])
    got = j.scores(h, X)
    want = G().featureNotensor(X, ls if form == "ard" else ls[0], 1.7, Z, b)
    assert got.shape == (N, n)
    assert np.array_equal(got, want.T)


def test_scores_and_evaluate_against_the_host():
    case = CR.CASES[4]
    g = golden()[CR.case_name(case)]
    j = joint_of(g)
    j.set_theta(g["theta"])
    h = g["H"][1]
    rng = np.random.default_rng(3)
    Xt = rng.standard_normal((77, 16))
    yt = rng.integers(1, 8, 77)
    phi = G().featureNotensor(Xt, h[:16], h[-1], g["Z"], g["b"])
    want = phi.T @ g["theta"]
    got = j.scores(h, Xt)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    ev = j.evaluate(h, Xt, yt)
    assert np.array_equal(ev.scores[:, :, 0], got)
    ref = G().class_eval(got, yt)
    assert ev.prop_missed[0] == ref.prop_missed[0] and ev.mean_nlp[0] == ref.mean_nlp[0]
    assert ev.avg_prop_missed == ref.avg_prop_missed and ev.avg_mean_nlp == ref.avg_mean_nlp
    assert np.array_equal(ev.prediction, ref.prediction) and np.array_equal(ev.nlp, ref.nlp)


def test_size_limit():
    """n = 1024 with N = 40, D = 3, C = 2 against the fused fp64 restatement under the parity rule
    with the restatement's error taken as 1e-10 (test_gpu_nlml.py::test_size_limit's way);
    n = 1025, D = 17 and C = 33 are rejected."""
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    rng = np.random.default_rng(5)
    n, N, D, C = 1024, 40, 3, 2
    X, Z, b = rng.standard_normal((N, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    y = (np.arange(N) % C) + 1.0
    theta = 0.3 * rng.standard_normal((n, C))
    h = np.array([1.0, 1.0, 1.0, 1.0])
    val, grad = G().SoftmaxJoint(X, y, Z, b).value_and_grad(theta, h)
    rv, rt, rh = CR.value_and_grad_fused(X, y, Z, b, theta, h)
    assert CR.component_rule(rh)
    eh = np.abs(grad[n * C:] - rh) / np.abs(rh)
    et = CR.theta_error(grad[:n * C].reshape((n, C), order="F"), rt)
    print("n = 1024: value %.2e, hyper gradient %s, grad theta %.2e" % (abs(val - rv) / abs(rv), eh, et))
    assert abs(val - rv) <= 1e-12 * abs(rv)
    assert (eh <= 32 * 1e-10).all() and et <= 32 * 1e-10
    for bad in (dict(n=1025), dict(D=17), dict(C=33)):
        n2, D2, C2 = bad.get("n", 8), bad.get("D", 3), bad.get("C", 2)
        with pytest.raises(GPTError) as ei:
            G().SoftmaxJoint(rng.standard_normal((N, D2)), y, rng.standard_normal((n2, D2)),
                             rng.random(n2), C=C2)
        assert ei.value.code == GPT_ERR_BAD_DIMS, bad


def test_bad_labels_and_hyperparameters_rejected():
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    g = golden()[CR.case_name(CR.CASES[0])]
    for k, v in ((3, 0.0), (3, 4.0), (5, 1.5), (7, float("nan"))):
        y = g["y"].copy()
        y[k] = v
        with pytest.raises(GPTError) as ei:
            G().SoftmaxJoint(g["X"], y, g["Z"], g["b"], C=3)
        assert ei.value.code == GPT_ERR_BAD_DIMS
    j = joint_of(g)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        for k in range(3):
            h = g["H"][0].copy()
            h[k] = bad
            with pytest.raises(GPTError) as ei:
                j.value_and_grad(g["theta"], h)
            assert ei.value.code == GPT_ERR_BAD_DIMS
    with pytest.raises(GPTError):
        j.neglogjointlkhd(g["theta"], [1.0, 1.0, 1.0, 1.0])       # Lh = 4 with D = 2
    val = j.neglogjointlkhd(g["theta"], g["H"][0])                # the handle still works
    assert abs(val - g["val"][0]) <= 1e-12 * abs(g["val"][0])


@pytest.mark.parametrize("idx,t0", [(1, 0), (4, 5)])
def test_langevin_steps(idx, t0):
    """Three Langevin steps against the restatement at CLS.rel < 1e-9, the tolerance at which
    tests/test_gpu_cls.py:45 holds GPNT_SGLDclass's theta to its restatement (its 64_96_2 case
    runs three steps); the same seed gives equal bits, and one run of three steps equals three
    runs of one."""
    g = golden()[CR.case_name(CR.CASES[idx])]
    h = g["H"][1]
    eps, seed = 2e-3, 11
    want = CR.langevin(g["X"], g["y"], g["Z"], g["b"], g["theta"], h, eps, 3, seed, t0)
    j = joint_of(g)
    j.set_theta(g["theta"])
    j.langevin(h, eps, 3, seed, t0=t0)
    got = j.theta()
    assert j.steps == t0 + 3
    print("langevin %s: rel = %.3g" % (CR.case_name(CR.CASES[idx]), CLS.rel(got, want)))
    assert CLS.rel(got, want) < 1e-9
    assert CLS.rel(got, g["theta"]) > 1e-3                        # it moved
    j.set_theta(g["theta"])
    j.langevin(h, eps, 3, seed, t0=t0)
    assert np.array_equal(j.theta(), got)
    j.set_theta(g["theta"])
    j.langevin(h, eps, 1, seed, t0=t0)
    j.langevin(h, eps, 1, seed)
    j.langevin(h, eps, 1, seed)
    assert np.array_equal(j.theta(), got)
    j.set_theta(g["theta"])
    j.langevin(h, eps, 3, seed + 1, t0=t0)
    assert not np.array_equal(j.theta(), got)


def test_langevin_nan_is_an_error_code():
    from gpt_amd._lib import GPT_ERR_NAN_THETA, GPTError
    g = golden()[CR.case_name(CR.CASES[0])]
    j = joint_of(g)
    j.set_theta(g["theta"])
    with pytest.raises(GPTError) as ei:
        j.langevin(g["H"][0], 1e300, 4, 3, t0=0)
    assert ei.value.code == GPT_ERR_NAN_THETA
    j.set_theta(g["theta"])                                       # the handle still works
    assert abs(j.neglogjointlkhd(None, g["H"][0]) - g["val"][0]) <= 1e-12 * abs(g["val"][0])


@functools.lru_cache(maxsize=None)
def planted():
    """N = 400, D = 2, C = 3, n = 64: labels drawn from the softmax of a planted theta at
    l = 1, sigma = 2."""
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


def run_em(seed, **kw):
    X, y, Z, b, C, n = planted()
    j = G().SoftmaxJoint(X, y, Z, b, C=C)
    out = G().GPNT_hyperparameters_ng(np.zeros(n * C), [3.0, 3.0, 1.0], j.neglogjointlkhd,
                                      j.gradneglogjointlkhd, Z, b, seed=seed, trace=True, **kw)
    return j, out


def test_stochastic_em_on_a_planted_problem():
    pytest.importorskip("scipy")
    j, (h1, tr1) = run_em(4, max_iter=4)
    assert len(tr1) == 4 and np.isfinite(h1).all() and (h1 > 0).all()     # max_iter is honoured
    for before, after, hyper in tr1:
        print("EM round: f before %.6f, after %.6f, hyper %s" % (before, after, hyper))
        assert after <= before
    _, (h2, tr2) = run_em(4, max_iter=4)
    assert np.array_equal(h1, h2) and all(a[:2] == c[:2] for a, c in zip(tr1, tr2))
    _, (h3, _) = run_em(5, max_iter=4)
    assert not np.array_equal(h1, h3)
    _, (_, tr5) = run_em(4, max_iter=2)
    assert len(tr5) == 2


def test_em_without_e_step_is_scipy_cg_on_the_handle():
    pytest.importorskip("scipy")
    from scipy.optimize import minimize
    X, y, Z, b, C, n = planted()
    theta0 = 0.1 * np.random.default_rng(1).standard_normal(n * C)
    j = G().SoftmaxJoint(X, y, Z, b, C=C)
    init = np.array([3.0, 3.0, 1.0])
    got = G().GPNT_hyperparameters_ng(theta0, init, j.neglogjointlkhd, j.gradneglogjointlkhd, Z, b,
                                      num_sgld_iter=0, num_cg_iter=10, max_iter=1)
    assert np.array_equal(j.theta().ravel(order="F"), theta0)

    def fun(lh):
        h = np.exp(lh)
        return j.neglogjointlkhd(theta0, h), j.gradneglogjointlkhd(theta0, h)[-3:] * h
    res = minimize(fun, np.log(init), jac=True, method="CG", options={"maxiter": 10})
    assert np.array_equal(got, np.exp(res.x))
    with pytest.raises(TypeError):
        G().GPNT_hyperparameters_ng(theta0, init, fun, j.gradneglogjointlkhd, Z, b)
    other = G().SoftmaxJoint(X, y, Z, b, C=C)
    with pytest.raises(TypeError):
        G().GPNT_hyperparameters_ng(theta0, init, j.neglogjointlkhd, other.gradneglogjointlkhd, Z, b)


def test_segment_data_three_rounds():
    """Three rounds from l = ones(16), sigma = 1 on the segment training rows
    (ImageExperiment.jl's n = 150 and feature seed): finite hyper-parameters, and evaluate on the
    1010 test rows equals class_eval of featureNotensor(Xtest)'theta computed on the host.  No
    quality figure is asserted (the reference recorded none for this loop)."""
    pytest.importorskip("scipy")
    Xtr, ytr, Xte, yte = CLS.segment_problem()
    n, C = CLS.SEG["n"], 7
    Z, b = G().feature_inputs(n, 16, CLS.SEG["feature_seed"])
    j = G().SoftmaxJoint(Xtr, ytr.astype(np.float64), Z, b[:, 0], C=C)
    h, tr = G().GPNT_hyperparameters_ng(np.zeros(n * C), np.ones(17), j.neglogjointlkhd,
                                        j.gradneglogjointlkhd, Z, b[:, 0], seed=2, max_iter=3,
                                        trace=True)
    assert len(tr) == 3 and h.shape == (17,) and np.isfinite(h).all() and (h > 0).all()
    ev = j.evaluate(h, Xte, yte)
    phi = G().featureNotensor(Xte, h[:16], h[-1], Z, b[:, 0])
    want = phi.T @ j.theta()
    assert np.abs(ev.scores[:, :, 0] - want).max() <= 1e-12 * np.abs(want).max()
    ref = G().class_eval(ev.scores[:, :, 0], yte)
    assert ev.prop_missed[0] == ref.prop_missed[0] and ev.mean_nlp[0] == ref.mean_nlp[0]
    hostref = CLS.class_eval_np(want, yte)
    assert abs(ev.mean_nlp[0] - hostref["mean_nlp"][0]) <= 1e-9 * max(1.0, abs(hostref["mean_nlp"][0]))
    print("segment after 3 rounds: prop_missed %.4f, mean_nlp %.4f, f %.3f -> %.3f, sigma %.4f"
          % (ev.prop_missed[0], ev.mean_nlp[0], tr[0][0], tr[-1][1], h[-1]))
