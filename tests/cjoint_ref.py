"""fp64 numpy restatements of the joint likelihood of the full-theta softmax classifier and its
gradient, an mpmath evaluation, a restatement of the Langevin step on theta, the test cases of
tests/golden/cjoint_mp.npz and the error yardstick of the device parity tests.

    neglogjoint_literal / gradneglogjoint_literal   ImageExperiment.jl:135-204 (per-row loops and
                                                    the n x N x (Lh) gradfeatureNotensor array)
    value_and_grad_fused                            the one-pass form the device runs
    mp_value_grad                                   the same quantities at 50 digits (mp_core
                                                    keeps them as mpf, mp_features is its phi, S)
    ld_value_grad                                   the fused form in long double
    cjoint_layout                                   the device's tile layout restated
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
MP_DIGITS = 50


def mp_features(X, Z, b, h, want_S=True):
    """phi = c cos f and S = c sin f (n rows of N mpf) at 50 digits from the float64 inputs, with
    Zt = Z / l formed in mp; a leapfrog evaluates many theta on one of these.  Call under
    mp.workdps(MP_DIGITS)."""
    import mpmath as mp
    M = mp.mpf
    N, D = X.shape
    n = Z.shape[0]
    Lh = len(h)
    hh = [M(float(v)) for v in h]
    ls = [hh[0]] * D if Lh == 2 else hh[:D]
    sig = hh[-1]
    Xm = [[M(float(X[i, k])) for k in range(D)] for i in range(N)]
    Zt = [[M(float(Z[j, k])) / ls[k] for k in range(D)] for j in range(n)]
    cc = mp.sqrt(M(2) / n) * sig
    f = [[mp.fdot(Xm[i], Zt[j]) + M(float(b[j])) for i in range(N)] for j in range(n)]
    phi = [[cc * mp.cos(v) for v in row] for row in f]                          # phi[j][i]
    S = [[cc * mp.sin(v) for v in row] for row in f] if want_S else None
    return dict(n=n, N=N, D=D, Lh=Lh, ls=ls, sig=sig, Xm=Xm, Zt=Zt, phi=phi, S=S,
                phic=[[phi[j][i] for j in range(n)] for i in range(N)])


def mp_theta(theta):
    """theta (n, C) of doubles as th[j][c] of mpf (exact)."""
    import mpmath as mp
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(theta, dtype=np.float64)]


def mp_core(F, y, th, want_h=True):
    """value, gradtheta (gt[j][c]) and gradh (list, or None) as mpf at the mpf theta th[j][c] on
    mp_features' F: nothing is rounded to double, so an integrator can chain evaluations.  Call
    under mp.workdps(MP_DIGITS)."""
    import mpmath as mp
    M = mp.mpf
    n, N, D, Lh = F["n"], F["N"], F["D"], F["Lh"]
    C = len(th[0])
    phi, phic = F["phi"], F["phic"]
    yi = labels0(y, C)
    thc = [[th[j][c] for j in range(n)] for c in range(C)]
    val = M(0)
    rs = M(0)
    R = [[None] * N for _ in range(C)]                                          # R[c][i]
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
    gt = [[mp.fdot(phi[j], R[c]) + th[j][c] for c in range(C)] for j in range(n)]
    if not want_h:
        return val, gt, None
    S, Zt, ls = F["S"], F["Zt"], F["ls"]
    Xc = [[F["Xm"][i][k] for i in range(N)] for k in range(D)]
    Rcol = [[R[c][i] for c in range(C)] for i in range(N)]
    gl = [M(0)] * D
    for j in range(n):
        T = [S[j][i] * mp.fdot(th[j], Rcol[i]) for i in range(N)]
        for k in range(D):
            gl[k] += Zt[j][k] * mp.fdot(T, Xc[k])
    gl = [gl[k] / ls[k] for k in range(D)]
    gh = [mp.fsum(gl)] if Lh == 2 else list(gl)
    gh.append(rs / F["sig"])
    return val, gt, gh


def mp_value_grad(X, y, Z, b, theta, h):
    """value (float), gradtheta (n, C) and gradh (Lh) from a 50-digit evaluation.  Zt = Z / l is
    formed in mp from the float64 inputs, so this is the true value at those inputs."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        val, gt, gh = mp_core(mp_features(X, Z, b, h), y, mp_theta(theta))
        gtheta = np.array([[float(v) for v in row] for row in gt])
        return float(val), gtheta, np.array([float(v) for v in gh])


def ld_value_grad(X, y, Z, b, theta, h):
    """value, gradtheta (n, C), gradh (Lh) in np.longdouble (x87 80-bit where numpy has it): the
    fused form on the float64 inputs, the reference of the tile-walk cases whose mpmath evaluation
    takes too long (tests/golden/make_exactgp_golden.py's way above N = 259)."""
    L = np.longdouble
    n, C = theta.shape
    N, D = X.shape
    h = np.asarray(h, dtype=np.float64)
    ls, sigma = split(h, D)
    yi = labels0(y, C)
    Xl, th = X.astype(L), theta.astype(L)
    lsl = ls.astype(L)
    Zt = Z.astype(L) / lsl
    f = Zt @ Xl.T + b.astype(L)[:, None]
    c = np.sqrt(L(2) / L(n)) * L(sigma)
    phi, S = c * np.cos(f), c * np.sin(f)
    s = th.T @ phi
    a = s.max(axis=0)
    lse = a + np.log(np.exp(s - a).sum(axis=0))
    R = np.exp(s - lse)
    R[yi, np.arange(N)] -= L(1)
    val = np.sum(lse - s[yi, np.arange(N)]) + np.sum(th * th) / L(2)
    gtheta = phi @ R.T + th
    T = S * (th @ R)
    gl = (Zt * (T @ Xl)).sum(axis=0) / lsl
    gh = np.empty(h.size, dtype=L)
    if h.size == 2:
        gh[0] = gl.sum()
    else:
        gh[:D] = gl
    gh[-1] = np.sum(R * s) / L(sigma)
    return val, gtheta, gh


# --------------------------------------------------------------------------- device layout
CJ_LDS, CJ_MAX_BLOCKS, NW = 160 * 1024, 256, 8


def _al16(x):
    return (x + 15) & ~15


def cjoint_layout(n, N, C):
    """gpt_amd/csrc/cjoint.hip's cjoint_layout restated (the C ABI has no query for it): dict(CC,
    TI, ntiles, nblk, theta_lds, bytes).  Workgroup w of nblk walks the tiles w, w + nblk, ..."""
    CC = 2 if C <= 2 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32
    TI = 32
    while True:
        o = _al16(8 * CC * TI)
        o = _al16(o + 8 * 16 * TI)
        o = _al16(o + 8 * 16)
        o = _al16(o + 8 * NW)
        o = _al16(o + 8 * n * TI)
        o = _al16(o + 8 * n * TI)
        if o <= CJ_LDS or TI == 8:
            break
        TI //= 2
    with_theta = _al16(o + 8 * n * CC)
    theta_lds = with_theta <= CJ_LDS
    ntiles = -(-N // TI)
    return dict(CC=CC, TI=TI, ntiles=ntiles, nblk=min(ntiles, CJ_MAX_BLOCKS),
                theta_lds=bool(theta_lds), bytes=with_theta if theta_lds else o)


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
