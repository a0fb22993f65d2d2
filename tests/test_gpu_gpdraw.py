"""GPU tests of the function draws (gpt_amd/csrc/gpdraw.hip and the draw entries of exactgp.hip and
nlml.hip) against the mpmath golden tests/golden/gpdraw_mp.npz and the fp64 restatements of
tests/gpdraw_ref.py.

Parity rule (tests/test_gpu_exactgp.py's): the yardstick is the error of the fp64 restatement
against the golden, and the device's error may be at most max(32 x yardstick, 1e-12).  Prior F over
max|F|, fmu over max|fmu|, posterior F over max|F - fmu|, cov over sigma_RBF^2, theta over
max|theta - l|.
"""
import math

import numpy as np
import pytest

import gpdraw_ref as R
from oracle import fastmath_cases as FC
from oracle import philox as P

pytestmark = pytest.mark.gpu

FLOOR = 1e-12
EPS = 2.0 ** -53
NAMES = [R.case_name(c) for c in R.CASES]
RFF = [nm for nm, n in zip(NAMES, R.RFF_N) if n]


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


_YARD, _DEV = {}, {}


def yard(golden, nm):
    if nm not in _YARD:
        _YARD[nm] = R.yardstick(golden[nm])
    return _YARD[nm]


def dev(golden, nm):
    """The device's S = 17 results of a case with the golden's injected normals, computed once."""
    if nm not in _DEV:
        g = golden[nm]
        gp = G().ExactGP(g["X"], g["y"])
        d = dict(Fprior=gp.draw_prior(g["h"], S=R.S, z=g["Zprior"]),
                 post=gp.draw_posterior(g["h"], g["Xtest"], S=R.S, z=g["Zpost"], return_cov=True))
        gp.close()
        if "Ztheta" in g:
            nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
            d["theta"] = nt.draw_theta(g["h"], R.S, z=g["Ztheta"])
            d["l"] = nt.theta_mean(g["h"])
            nt.close()
        _DEV[nm] = d
    return _DEV[nm]


def held(tag, err, yd):
    worst = 0.0
    for q in sorted(err):
        bound = max(32 * yd[q], FLOOR)
        worst = max(worst, err[q] / bound)
        print("%s %-5s error %.2e, yardstick %.2e, error/bound %.3f" % (tag, q, err[q], yd[q],
                                                                         err[q] / bound))
    for q in err:
        assert err[q] <= max(32 * yd[q], FLOOR), (tag, q, err[q], yd[q])
    return worst


# --------------------------------------------------------------------------------- 1. the noise
@pytest.mark.parametrize("seed", [1, 2 ** 63 + 5])
def test_noise_is_the_documented_philox_stream(golden, seed):
    """Zout against oracle.philox.normals(M, seed, s, 25, kind) under normal_at's bar of
    tests/test_gpu_fastmath.py: (2 + T_POLY + 1) 2^-52 times the pair's radius."""
    g = golden[NAMES[0]]
    gp = G().ExactGP(g["X"], g["y"])
    nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
    zs = [gp.draw_prior(g["h"], S=3, seed=seed, return_z=True)[1],
          gp.draw_posterior(g["h"], g["Xtest"], S=3, seed=seed, return_z=True).z,
          nt.draw_theta(g["h"], 3, seed=seed, return_z=True)[1]]
    for kind, z in enumerate(zs):
        M = z.shape[0]
        assert z.shape == (M, 3) and np.isfinite(z).all()
        for s in range(3):
            want = P.normals(M + (M & 1), seed, s, 25, kind)
            rad = np.repeat(np.hypot(want[0::2], want[1::2]), 2)[:M]
            worst = (np.abs(z[:, s] - want[:M]) / (2.0 ** -52 * rad)).max()
            print("kind %d column %d: worst %.3f units of 2^-52 rad" % (kind, s, worst))
            assert worst <= 2 + FC.T_POLY + 1
        assert np.abs(z[:, 0] - z[:, 1]).max() > 1e-3           # columns are different streams
    gp.close()
    nt.close()


# ---------------------------------------------------------------------- 2. parity, injected Z
@pytest.mark.parametrize("S", [1, 3, 17])
@pytest.mark.parametrize("nm", NAMES)
def test_parity_with_injected_normals(golden, nm, S):
    g, yd = golden[nm], yard(golden, nm)
    cols = slice(0, S)
    if S == R.S:
        d = dev(golden, nm)
        Fp, post, th = d["Fprior"], d["post"], d.get("theta")
    else:
        gp = G().ExactGP(g["X"], g["y"])
        Fp = gp.draw_prior(g["h"], S=S, z=g["Zprior"][:, cols])
        post = gp.draw_posterior(g["h"], g["Xtest"], S=S, z=g["Zpost"][:, cols], return_cov=True)
        gp.close()
        th = None
        if "Ztheta" in g:
            nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
            th = nt.draw_theta(g["h"], S, z=g["Ztheta"][:, cols])
            nt.close()
    assert Fp.shape == (g["X"].shape[0], S) and post.samples.shape == (g["Xtest"].shape[0], S)
    err = R.errors(g, Fprior=Fp, fmu=post.fmu, Fpost=post.samples, cov=post.cov, th=th, cols=cols)
    assert np.array_equal(post.cov, post.cov.T)
    worst = held("%s S=%d" % (nm, S), err, yd)
    print("%s S=%d worst error/bound %.3f" % (nm, S, worst))


# ------------------------------------------------------------------- 3. the factors themselves
def _resid(L, A, unit):
    return np.abs(L @ L.T - A).max() / unit


@pytest.mark.parametrize("nm", NAMES)
def test_factors_reproduce_their_matrices(golden, nm):
    """Zin = I gives F - mu = L: L L' against K + jitter I and against cov + jitter I, held to
    32 x the residual of numpy's factor of the same matrix."""
    g = golden[nm]
    h, N, Nt = g["h"], g["X"].shape[0], g["Xtest"].shape[0]
    unit = h[-2] ** 2
    gp = G().ExactGP(g["X"], g["y"])
    L = gp.draw_prior(h, S=N, z=np.eye(N))
    A = R.kern(g["X"], g["X"], h) + R.JITTER * np.eye(N)
    assert np.array_equal(L, np.tril(L))
    got, ref = _resid(L, A, unit), _resid(np.linalg.cholesky(A), A, unit)
    print("%s prior factor residual %.2e, numpy's %.2e" % (nm, got, ref))
    assert got <= max(32 * ref, FLOOR)
    post = gp.draw_posterior(h, g["Xtest"], S=Nt, z=np.eye(Nt), return_cov=True)
    gp.close()
    Ls = post.samples - post.fmu[:, None]
    Sg = post.cov + R.JITTER * np.eye(Nt)
    got, ref = _resid(Ls, Sg, unit), _resid(np.linalg.cholesky(Sg), Sg, unit)
    print("%s posterior factor residual %.2e, numpy's %.2e" % (nm, got, ref))
    assert got <= max(32 * ref, FLOOR)       # the floor covers F = fmu + L rounding L to F's grid


@pytest.mark.parametrize("nm", RFF)
def test_theta_factor_inverts_the_system(golden, nm):
    """Zin = I: W = (theta - l)/sigma = L^-T, and A W W' = I, held to 32 x numpy's residual."""
    import scipy.linalg as sla
    g = golden[nm]
    h = g["h"]
    n = g["Zf"].shape[0]
    nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
    th = nt.draw_theta(h, n, z=np.eye(n))
    l = nt.theta_mean(h)
    nt.close()
    W = (th - l[:, None]) / math.sqrt(h[-1])
    assert np.array_equal(W, np.triu(W))
    _, A = R.rff_system(g["X"], h, g["Zf"], g["bf"])
    Wn = sla.solve_triangular(np.linalg.cholesky(A).T, np.eye(n), lower=False)
    got, ref = np.abs(A @ W @ W.T - np.eye(n)).max(), np.abs(A @ Wn @ Wn.T - np.eye(n)).max()
    print("%s A W W' - I: %.2e, numpy's %.2e" % (nm, got, ref))
    assert got <= max(32 * ref, FLOOR)


# ------------------------------------------------------------------------ 4. ties to what exists
@pytest.mark.parametrize("nm", NAMES)
def test_posterior_mean_and_marginals_are_predicts(golden, nm):
    g, yd = golden[nm], yard(golden, nm)
    h = g["h"]
    gp = G().ExactGP(g["X"], g["y"])
    pr = gp.predict(h, g["Xtest"])
    post = dev(golden, nm)["post"]
    assert np.array_equal(post.fmu, pr.fmu)
    cov = gp.predict_cov(h, g["Xtest"])
    assert np.array_equal(cov, post.cov)
    assert np.array_equal(gp.predict(h, g["Xtest"]).fmu, pr.fmu)
    gp.close()
    assert (pr.fs2 > 0).all()                                      # not clamped
    e = np.abs(np.diag(cov) - pr.fs2).max() / h[-2] ** 2
    bound = max(32 * yd.get("cov", 0.0), FLOOR)
    print("%s diag(cov) vs fs2: %.2e (bound %.2e)" % (nm, e, bound))
    assert e <= bound


def _moment_tol(fmu, fs2, M):
    """Rounding of the moments of 2M samples mu +- sqrt(M) L e_i: every sample carries
    2^-53 (|mu| + sqrt(M) sd) of rounding, the variance its square; 64 covers the 2M-term sums."""
    scale = np.abs(fmu).max() + math.sqrt(M * fs2.max())
    return 64 * EPS * scale, 64 * EPS * scale * scale


@pytest.mark.parametrize("nm", RFF)
def test_symmetric_theta_draws_reproduce_the_closed_form_predictive(golden, nm):
    """Zin = sqrt(n) [I, -I]: the 2n draws have mean l and covariance signal_var A^-1 exactly, so
    GPNT_predictive over them is NoTensorMarginal.predict."""
    g = golden[nm]
    h = g["h"]
    n, Nt = g["Zf"].shape[0], g["Xtest"].shape[0]
    ytest = np.sin(g["Xtest"].sum(axis=1))
    nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
    z = math.sqrt(n) * np.hstack([np.eye(n), -np.eye(n)])
    theta = nt.draw_theta(h, 2 * n, z=z)
    pr = nt.predict(h, g["Xtest"], ytest)
    nt.close()
    phitest = G().featureNotensor(g["Xtest"], h[:-2] if h.size > 3 else h[0], h[-2], g["Zf"], g["bf"])
    ev = G().GPNT_predictive(theta, phitest, ytest, h[-1])
    tm, tv = _moment_tol(pr.fmu, pr.fs2, n)
    em, evr = np.abs(ev.gp.fmu - pr.fmu).max(), np.abs(ev.gp.fs2 - pr.fs2).max()
    print("%s fmu %.2e (tol %.2e), fs2 %.2e (tol %.2e)" % (nm, em, tm, evr, tv))
    assert em <= tm and evr <= tv


def test_symmetric_posterior_draws_reproduce_predict(golden):
    nm = NAMES[1]                                                   # Ntest = 64
    g = golden[nm]
    h, Nt = g["h"], g["Xtest"].shape[0]
    assert Nt == 64
    ytest = np.sin(g["Xtest"].sum(axis=1))
    gp = G().ExactGP(g["X"], g["y"])
    z = math.sqrt(Nt) * np.hstack([np.eye(Nt), -np.eye(Nt)])
    F = gp.draw_posterior(h, g["Xtest"], S=2 * Nt, z=z).samples
    pr = gp.predict(h, g["Xtest"], ytest)
    gp.close()
    ev = G().predictive(F, ytest, h[-1])
    tm, tv = _moment_tol(pr.fmu, pr.fs2 + R.JITTER, Nt)
    em = np.abs(ev.gp.fmu - pr.fmu).max()
    evr = np.abs(ev.gp.fs2 - (pr.fs2 + R.JITTER)).max()             # L L' = cov + jitter I
    print("%s fmu %.2e (tol %.2e), fs2 %.2e (tol %.2e)" % (nm, em, tm, evr, tv))
    assert em <= tm and evr <= tv


# ------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("nm", NAMES)
def test_bits_do_not_depend_on_S_or_the_other_columns(golden, nm):
    g, d = golden[nm], dev(golden, nm)
    h = g["h"]
    gp = G().ExactGP(g["X"], g["y"])
    assert np.array_equal(gp.draw_prior(h, S=R.S, z=g["Zprior"]), d["Fprior"])      # equal calls
    s = 16
    assert np.array_equal(gp.draw_prior(h, S=1, z=g["Zprior"][:, s])[:, 0], d["Fprior"][:, s])
    one = gp.draw_posterior(h, g["Xtest"], S=1, z=g["Zpost"][:, s])
    assert np.array_equal(one.samples[:, 0], d["post"].samples[:, s])
    assert np.array_equal(one.fmu, d["post"].fmu) and one.cov is None and one.z is None
    # a Philox call's columns do not depend on S
    a, b = gp.draw_prior(h, S=2, seed=9), gp.draw_prior(h, S=19, seed=9)
    assert np.array_equal(a, b[:, :2]) and not np.array_equal(b[:, 0], b[:, 1])
    a = gp.draw_posterior(h, g["Xtest"], S=2, seed=9, observed=True).samples
    b = gp.draw_posterior(h, g["Xtest"], S=19, seed=9, observed=True).samples
    assert np.array_equal(a, b[:, :2])
    assert not np.array_equal(a, gp.draw_posterior(h, g["Xtest"], S=2, seed=9).samples)
    prior19 = gp.draw_prior(h, S=19, seed=9)
    gp.close()
    # the one-shot forms
    ls = h[:-2] if h.size > 3 else h[0]
    assert np.array_equal(G().GPrand(g["X"], ls, h[-2], S=19, seed=9), prior19)
    o = G().gp_posterior_draw_oneshot(g["X"], g["y"], h, g["Xtest"], S=R.S, z=g["Zpost"],
                                      return_cov=True)
    for x, y in zip(o[:3], d["post"][:3]):
        assert np.array_equal(x, y)
    if "Ztheta" in g:
        nt = G().NoTensorMarginal(g["X"], g["y"], g["Zf"], g["bf"])
        assert np.array_equal(nt.draw_theta(h, R.S, z=g["Ztheta"]), d["theta"])
        assert np.array_equal(nt.draw_theta(h, 1, z=g["Ztheta"][:, s])[:, 0], d["theta"][:, s])
        a, b = nt.draw_theta(h, 2, seed=9), nt.draw_theta(h, 19, seed=9)
        assert np.array_equal(a, b[:, :2])
        nt.value_and_grad(h)                                         # Xt left by the gradient
        assert np.array_equal(nt.draw_theta(h, R.S, z=g["Ztheta"]), d["theta"])
        nt.close()
        assert np.array_equal(G().gpnt_draw_theta_oneshot(g["X"], g["y"], g["Zf"], g["bf"], h, R.S,
                                                          z=g["Ztheta"]), d["theta"])


def test_interleaved_calls_return_what_each_returns_alone(golden):
    nm = NAMES[2]
    g, d = golden[nm], dev(golden, nm)
    h = g["h"]
    h2 = h.copy()
    h2[-1] *= 2.0
    fresh = G().ExactGP(g["X"], g["y"])
    want_pred = fresh.predict(h2, g["Xtest"])
    fresh.close()
    fresh = G().ExactGP(g["X"], g["y"])
    want_vg = fresh.value_and_grad(h)
    fresh.close()
    gp = G().ExactGP(g["X"], g["y"])
    assert np.array_equal(gp.draw_prior(h, S=R.S, z=g["Zprior"]), d["Fprior"])
    got = gp.predict(h2, g["Xtest"])
    assert np.array_equal(got.fmu, want_pred.fmu) and np.array_equal(got.fs2, want_pred.fs2)
    p1 = gp.draw_posterior(h, g["Xtest"], S=R.S, z=g["Zpost"], return_cov=True)
    v, gr = gp.value_and_grad(h)
    assert v == want_vg[0] and np.array_equal(gr, want_vg[1])
    p2 = gp.draw_posterior(h, g["Xtest"], S=R.S, z=g["Zpost"], return_cov=True)
    gp.close()
    for p in (p1, p2):
        for x, y in zip(p[:3], d["post"][:3]):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------- 6. failure is a status
def test_failed_factorisation_is_a_status():
    """X = 0, sigma_RBF = 1, jitter = 0: K is all ones and the second pivot is exactly 1 - 1 = 0."""
    from gpt_amd._lib import GPT_ERR_NOT_SPD, GPTError, P_D, lib
    Gm = G()
    N, S = 70, 3
    X, y = np.zeros((N, 2), order="F"), np.arange(N, dtype=np.float64)
    h = np.array([1.0, 1.0, 0.5])
    gp = Gm.ExactGP(X, y)
    with pytest.raises(GPTError) as ei:
        gp.draw_prior(h, S=S, jitter=0.0)
    assert ei.value.code == GPT_ERR_NOT_SPD and "K + jitter*I" in str(ei.value)
    F, Z = np.zeros((N, S), order="F"), np.zeros((N, S), order="F")
    rc = lib().gpt_egp_draw_prior(gp._h, h.ctypes.data_as(P_D), 3, 0.0, S, 1, None,
                                  F.ctypes.data_as(P_D), Z.ctypes.data_as(P_D))
    assert rc == GPT_ERR_NOT_SPD and np.isnan(F).all() and np.isnan(Z).all()
    with pytest.raises(GPTError) as ei:
        Gm.GPrand(X, 1.0, 1.0, S=S, jitter=0.0)
    assert ei.value.code == GPT_ERR_NOT_SPD
    # the handle is still usable: K + 0.5 I is positive definite, and so is K + 1e-6 I
    pr = gp.predict(h, X[:4])
    assert np.isfinite(pr.fmu).all() and np.isfinite(pr.fs2).all()
    assert np.isfinite(gp.draw_prior(h, S=S, jitter=1e-6)).all()
    assert np.isfinite(gp.draw_posterior(h, X[:4] + 1.0, S=S).samples).all()
    gp.close()


# -------------------------------------------------------------------- 7. fhatdraw end to end
def test_fhatdraw_end_to_end():
    Gm = G()
    n, D, r, Q, N = 5, 5, 2, 32, 100                               # the TensorSynthData shape
    X = np.random.default_rng(11).standard_normal((N, D))
    y, w, U, I, phi = Gm.fhatdraw(X, n, 1.5, 1.2, r, Q, seed=3)
    assert y.shape == (N,) and w.shape == (Q,) and U.shape == (n, r, D)
    assert I.shape == (Q, D) and phi.shape == (n, D, N)
    assert np.array_equal(Gm.pred(w, U, I, phi), y)
    for k in range(D):
        assert np.abs(U[:, :, k].T @ U[:, :, k] - np.eye(r)).max() <= 1e-12
    again = Gm.fhatdraw(X, n, 1.5, 1.2, r, Q, seed=3)
    for a, b in zip(again, (y, w, U, I, phi)):
        assert np.array_equal(a, b)
    other = Gm.fhatdraw(X, n, 1.5, 1.2, r, Q, seed=4)
    assert not np.array_equal(other[0], y) and not np.array_equal(other[1], w)
    vec = Gm.fhatdraw(X, n, [1.5] * D, 1.2, r, Q, seed=3)
    assert np.array_equal(vec[0], y)
    _, _, grid = Gm.createmesh(-1, 1, 5)
    assert Gm.fhatdraw(grid, n, 1.0, 1.0, r, 4, seed=1)[0].shape == (25,)
