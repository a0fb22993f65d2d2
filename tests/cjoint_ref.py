"""fp64 numpy restatements of the joint likelihood of the full-theta softmax classifier and its
gradient, an mpmath evaluation, a restatement of the Langevin step on theta, the test cases of
tests/golden/cjoint_mp.npz and the error yardstick of the device parity tests.

    neglogjoint_literal / gradneglogjoint_literal   ImageExperiment.jl:135-204 (per-row loops and
                                                    the n x N x (Lh) gradfeatureNotensor array)
    value_and_grad_fused                            the one-pass form the device runs
    mp_value_grad                                   the same quantities at 50 digits
    langevin                                        the E step of GPNT_hyperparameters_ng
                                                    (GPT_SGLD.jl:1031-1033)

Hyper-parameters are h = [length_scale (D entries, or one: the scalar form); sigma_RBF]; theta is
(n, C); labels are 1..C.  The gradient is the reference's [vec(gradtheta); gradl; gradsigma].

RNG contract of the Langevin step (cls_ref.py's THETA_NOISE contract): the noise of 0-based step t
and class c is normals(n, seed, t, THETA_NOISE, c), and theta <- theta - (eps/2 grad + sqrt(eps) xi)
as GPT_SGLD.jl:1032 and GPNT_SGLDclass subtract it.
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import math
import os

import numpy as np

import nlml_ref as NR
from oracle import philox as px

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cjoint_mp.npz")

# (n, N, D, C, form, variant)
CASES = [
    (33, 130, 2, 3, "ard", ""),          # n < 64 and no multiple of 16; N no multiple of a tile
    (70, 130, 5, 3, "scalar", ""),       # scalar length scale with D > 1
    (64, 96, 1, 2, "scalar", ""),        # D = 1, Lh = 2, binary
    (40, 17, 3, 16, "ard", ""),          # N smaller than one tile; many classes
    (150, 203, 16, 7, "ard", ""),        # the experiment's n, C and D = 16
    (330, 70, 4, 32, "ard", ""),         # C at the limit; theta does not fit beside the tile
    (150, 203, 16, 7, "ard", "absent5"),  # class 5 absent, C passed explicitly
    (70, 130, 5, 3, "ard", "x40"),       # theta scaled by 40: scores in the hundreds
]
LS_CYCLE = [1.3978, 0.5, 2.8966, 7.5565]      # PowerPlantDataExperiment.jl:83-116, cyclically


def case_name(case):
    n, N, D, C, form, variant = case
    return "n%d_N%d_D%d_C%d_%s%s" % (n, N, D, C, form, "_" + variant if variant else "")


def hyper_len(case):
    return 2 if case[4] == "scalar" else case[2] + 1


def hyper_points(case):
    """The three points of every case."""
    nl = hyper_len(case) - 1
    return [np.array([1.0] * nl + [1.0]),
            np.array([LS_CYCLE[k % 4] for k in range(nl)] + [0.9129]),
            np.array([0.6] * nl + [2.0])]


def case_inputs(case, idx):
    """X (N, D), y (N, 1..C as float64), Z (n, D), b (n), theta (n, C): seeded normals, b = 2 pi
    rand; every class present except in the absent-class variant."""
    n, N, D, C, _, variant = case
    rng = np.random.default_rng(7000 + idx)
    X = rng.standard_normal((N, D))
    Z = rng.standard_normal((n, D))
    b = 2 * math.pi * rng.random(n)
    theta = rng.standard_normal((n, C))
    if variant == "x40":
        theta = 40.0 * theta
    classes = np.array([c for c in range(1, C + 1) if not (variant == "absent5" and c == 5)])
    y = classes[np.arange(N) % classes.size]
    rng.shuffle(y)
    return X, y.astype(np.float64), Z, b, theta


def split(h, D):
    h = np.asarray(h, dtype=np.float64)
    if h.size not in (2, D + 1):
        raise ValueError("hyperparams must have 2 or D + 1 entries")
    ls = np.full(D, h[0]) if h.size == 2 else h[:D].copy()
    return ls, float(h[-1])


def labels0(y, C):
    yv = np.asarray(y, dtype=np.float64).ravel()
    yi = yv.astype(np.int64)
    if not np.array_equal(yi, yv) or yi.min() < 1 or yi.max() > C:
        raise ValueError("labels must be integers in 1..C")
    return yi - 1


def logsumexp(x):
    """ImageExperiment.jl:129-132."""
    a = np.max(x)
    return a + math.log(np.sum(np.exp(x - a)))


# --------------------------------------------------------------------------- literal form
def neglogjoint_literal(X, y, Z, b, theta, h):
    n, C = theta.shape
    ls, sigma = split(h, X.shape[1])
    yi = labels0(y, C)
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    phi_theta = theta.T @ phi
    L = 0.0
    for i in range(X.shape[0]):
        L += logsumexp(phi_theta[:, i]) - phi_theta[yi[i], i]
    return L + np.sum(theta ** 2) / 2


def gradneglogjoint_literal(X, y, Z, b, theta, h):
    """[vec(gradtheta); gradlength_scale; gradsigma_RBF] with the loops of :152-204 and the
    (n, N, Lh) array of gradfeatureNotensor."""
    n, C = theta.shape
    N, D = X.shape
    h = np.asarray(h, dtype=np.float64)
    ls, sigma = split(h, D)
    yi = labels0(y, C)
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    phi_theta = theta.T @ phi
    gradtheta = np.zeros((n, C))
    for c in range(C):
        for i in range(N):
            gradtheta[:, c] += math.exp(phi_theta[c, i] - logsumexp(phi_theta[:, i])) * phi[:, i]
    for i in range(N):
        gradtheta[:, yi[i]] -= phi[:, i]
    gradtheta += theta
    gradfeature = NR.gradfeature_notensor(X, np.concatenate([h, [1.0]]), Z, b)   # (n, N, Lh)
    Lh = h.size
    gh = np.zeros(Lh)
    for i in range(N):
        p = np.exp(phi_theta[:, i] - logsumexp(phi_theta[:, i]))
        for k in range(Lh):
            gf = gradfeature[:, i, k]
            gh[k] += np.sum(p * (theta.T @ gf)) - np.sum(theta[:, yi[i]] * gf)
    return np.concatenate([gradtheta.ravel(order="F"), gh])


# --------------------------------------------------------------------------- fused form
def value_and_grad_fused(X, y, Z, b, theta, h):
    """value, gradtheta (n, C), gradh (Lh): no n x N x D array."""
    n, C = theta.shape
    N, D = X.shape
    h = np.asarray(h, dtype=np.float64)
    ls, sigma = split(h, D)
    yi = labels0(y, C)
    Zt, f = NR._arg(X, ls, Z, b)
    c = math.sqrt(2.0 / n) * sigma
    phi, S = c * np.cos(f), c * np.sin(f)
    s = theta.T @ phi
    a = s.max(axis=0)
    lse = a + np.log(np.exp(s - a).sum(axis=0))
    R = np.exp(s - lse)
    R[yi, np.arange(N)] -= 1.0
    val = np.sum(lse - s[yi, np.arange(N)]) + np.sum(theta ** 2) / 2
    gtheta = phi @ R.T + theta
    T = S * (theta @ R)
    gl = (Zt * (T @ X)).sum(axis=0) / ls
    gh = np.empty(h.size)
    if h.size == 2:
        gh[0] = gl.sum()
    else:
        gh[:D] = gl
    gh[-1] = np.sum(R * s) / sigma
    return val, gtheta, gh


def gradtheta_literal(X, y, Z, b, theta, h):
    n, C = theta.shape
    return gradneglogjoint_literal(X, y, Z, b, theta, h)[:n * C].reshape((n, C), order="F")


def gradtheta_fused(X, y, Z, b, theta, h):
    return value_and_grad_fused(X, y, Z, b, theta, h)[1]


# --------------------------------------------------------------------------- Langevin step
def langevin(X, y, Z, b, theta, h, eps, nsteps, seed, t0=0, gradtheta=gradtheta_fused):
    """nsteps steps from the 0-based step counter t0; returns the new theta (n, C)."""
    theta = np.array(theta, dtype=np.float64, copy=True)
    n, C = theta.shape
    for t in range(t0, t0 + nsteps):
        g = gradtheta(X, y, Z, b, theta, h)
        noise = np.empty((n, C))
        for c in range(C):
            noise[:, c] = px.normals(n, seed, t, px.THETA_NOISE, c)
        theta = theta - (eps * g / 2 + math.sqrt(eps) * noise)
    return theta


# --------------------------------------------------------------------------- mpmath
def mp_value_grad(X, y, Z, b, theta, h):
    """value (float), gradtheta (n, C) and gradh (Lh) from a 50-digit evaluation.  Zt = Z / l is
    formed in mp from the float64 inputs, so this is the true value at those inputs."""
    import mpmath as mp
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        M = mp.mpf
        n, C = theta.shape
        N, D = X.shape
        Lh = len(h)
        hh = [M(float(v)) for v in h]
        ls = [hh[0]] * D if Lh == 2 else hh[:D]
        sig = hh[-1]
        yi = labels0(y, C)
        Xm = [[M(float(X[i, k])) for k in range(D)] for i in range(N)]
        Xc = [[Xm[i][k] for i in range(N)] for k in range(D)]
        Zt = [[M(float(Z[j, k])) / ls[k] for k in range(D)] for j in range(n)]
        th = [[M(float(theta[j, c])) for c in range(C)] for j in range(n)]      # th[j][c]
        thc = [[th[j][c] for j in range(n)] for c in range(C)]
        cc = mp.sqrt(M(2) / n) * sig
        f = [[mp.fdot(Xm[i], Zt[j]) + M(float(b[j])) for i in range(N)] for j in range(n)]
        phi = [[cc * mp.cos(v) for v in row] for row in f]                      # phi[j][i]
        S = [[cc * mp.sin(v) for v in row] for row in f]
        phic = [[phi[j][i] for j in range(n)] for i in range(N)]
        val = M(0)
        rs = M(0)
        R = [[None] * N for _ in range(C)]                                      # R[c][i]
        for i in range(N):
            s = [mp.fdot(thc[c], phic[i]) for c in range(C)]
            a = max(s)
            lse = a + mp.log(mp.fsum(mp.exp(v - a) for v in s))
            val += lse - s[yi[i]]
            for c in range(C):
                r = mp.exp(s[c] - lse) - (1 if c == yi[i] else 0)
                R[c][i] = r
                rs += r * s[c]
        val += mp.fsum(v * v for row in th for v in row) / 2
        gtheta = np.empty((n, C))
        for j in range(n):
            for c in range(C):
                gtheta[j, c] = float(mp.fdot(phi[j], R[c]) + th[j][c])
        Rcol = [[R[c][i] for c in range(C)] for i in range(N)]
        gl = [M(0)] * D
        for j in range(n):
            T = [S[j][i] * mp.fdot(th[j], Rcol[i]) for i in range(N)]
            for k in range(D):
                gl[k] += Zt[j][k] * mp.fdot(T, Xc[k])
        gl = [gl[k] / ls[k] for k in range(D)]
        gh = [mp.fsum(gl)] if Lh == 2 else list(gl)
        gh.append(rs / sig)
        return float(val), gtheta, np.array([float(v) for v in gh])
    finally:
        mp.mp.dps = old


# --------------------------------------------------------------------------- golden and yardstick
KEYS = ("X", "y", "Z", "b", "theta", "H", "val", "gtheta", "gh")


def load_golden():
    """{case name: dict(X, y, Z, b, theta, H (3, Lh), val (3), gtheta (3, n, C), gh (3, Lh))}"""
    z = np.load(GOLDEN)
    return {case_name(c): {k: z["%s_%s" % (case_name(c), k)] for k in KEYS} for c in CASES}


def component_rule(gh):
    """The generator's rule: every hyper-gradient component at least 1e-4 of the largest."""
    return np.abs(gh).min() >= 1e-4 * np.abs(gh).max()


def hyper_errors(got, gold, against_largest=False):
    """Relative error per hyper-gradient component; with ``against_largest`` (the x40 case, where
    the component rule cannot be expected to hold) the errors are taken against the largest
    component."""
    den = np.abs(gold).max() if against_largest else np.abs(gold)
    return np.abs(np.asarray(got) - gold) / den


def theta_error(got, gold):
    return float(np.abs(np.asarray(got) - gold).max() / np.abs(gold).max())


def yardstick(g, p, against_largest=False):
    """(per hyper-gradient component, for gradtheta): the larger of the two fp64 restatements'
    errors against mp at point p of golden case g.  The device parity bound is 32 x this with a
    floor of 1e-12."""
    args = (g["X"], g["y"], g["Z"], g["b"], g["theta"], g["H"][p])
    n, C = g["theta"].shape
    lit = gradneglogjoint_literal(*args)
    _, ft, fh = value_and_grad_fused(*args)
    eh = np.maximum(hyper_errors(lit[n * C:], g["gh"][p], against_largest),
                    hyper_errors(fh, g["gh"][p], against_largest))
    et = max(theta_error(lit[:n * C].reshape((n, C), order="F"), g["gtheta"][p]),
             theta_error(ft, g["gtheta"][p]))
    return eh, et


def central_diff(fun, x, rel=1e-6):
    x = np.asarray(x, dtype=np.float64)
    g = np.empty(x.size)
    for k in range(x.size):
        d = rel * max(abs(x[k]), 1.0)
        xp, xm = x.copy(), x.copy()
        xp[k] += d
        xm[k] -= d
        g[k] = (fun(xp) - fun(xm)) / (xp[k] - xm[k])
    return g
