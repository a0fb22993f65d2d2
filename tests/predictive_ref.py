"""Restatements, yardsticks and cases of the posterior predictive of stored samples
(gpt_amd/csrc/predictive.hip).  A helper of tests/test_predictive_ref.py (CPU) and
tests/test_gpu_predictive.py; nothing under gpt_amd/ imports it.

predictive_np is the device's order of operations in numpy fp64: per row, over the
window's S columns in sample order,
    fmu = (Σ f)/S;  p = the first f, ebar = (Σ (f − p))/S, fs2 = (Σ ((f − p) − ebar)²)/S;
    ys2 = fs2 + v;  lp = −(y − fmu)²/(2 ys2) − ½ log(2π ys2);
    m = min (y − f)²,  lpmix = ((−½ log(2π v) − log S) − m/(2v)) + log Σ exp((m − (y − f)²)/(2v)),
with 1/(2v) formed once.  predictive_mp is the mathematics on the same doubles at 50 digits (the
variance about the exact mean, the mixture density by its definition).  yardstick(case) is the
error of the first against the second: the device is held to a multiple of it, never to its own
output."""
import functools
import math

import numpy as np

U = 2.0 ** -53
Z95 = 1.959963984540054
QUANTITIES = ("fmu", "fs2", "lp", "lp_mix")

# name -> (k, Ntest, T, window, noise_var, kind)
CASES = {
    "a": (0, 1, 1, (0, 1), 0.05, "normal"),        # one row, one sample: fs2 == 0, ys2 == noise_var
    "b": (1, 63, 2, (0, 2), 0.05, "normal"),       # short of a wave
    "c": (2, 65, 7, (2, 7), 0.2299 ** 2, "normal"),  # one row past a wave; window not at column 0
    "d": (3, 257, 65, (0, 65), 0.0476, "normal"),  # rows past 256, samples past 64
    "e": (4, 1031, 200, (59, 200), 0.05, "normal"),  # prime rows over several tiles; window 60:end
    "f": (5, 130, 33, (0, 33), 1e-6, "normal"),    # every exponent underflows without the shift
    "g": (6, 130, 33, (0, 33), 0.05, "equal"),     # all columns equal: fs2 == 0 exactly
    "h": (7, 130, 33, (0, 33), 0.05, "offset"),    # f = 1e3 + 1e-2 z: one-pass variance fails
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(F (Ntest, T) column-major, y, window, noise_var) of a case, read-only."""
    k, Nt, T, window, nv, kind = CASES[name]
    rng = np.random.default_rng(9100 + k)
    g = rng.standard_normal(Nt)
    z = rng.standard_normal((Nt, T))
    zy = rng.standard_normal(Nt)
    if kind == "equal":
        F = np.repeat((g + 0.3 * z[:, 0])[:, None], T, axis=1)
    elif kind == "offset":
        F = 1e3 + 1e-2 * z
    else:
        F = g[:, None] + 0.3 * z
    F = np.asfortranarray(F)
    y = g + math.sqrt(nv + 0.09) * zy
    F.setflags(write=False)
    y.setflags(write=False)
    return F, y, window, nv


def predictive_np(F, y, first, last, nv):
    """dict of fmu, fs2, lp, lp_mix (Ntest), sum_lp, sum_lp_mix, covered in the device's order."""
    W = np.asarray(F)[:, first:last]
    y = np.asarray(y, dtype=np.float64)
    S = W.shape[1]
    p = W[:, 0]
    m = np.zeros(y.size)
    se = np.zeros(y.size)
    dmin = np.full(y.size, np.inf)
    for s in range(S):
        v = W[:, s]
        m = m + v
        se = se + (v - p)
        d = y - v
        dmin = np.minimum(dmin, d * d)
    m = m / S
    ebar = se / S
    inv2v = 1.0 / (2.0 * nv)
    q = np.zeros(y.size)
    es = np.zeros(y.size)
    for s in range(S):
        v = W[:, s]
        e = (v - p) - ebar
        q = q + e * e
        d = y - v
        es = es + np.exp((dmin - d * d) * inv2v)
    fs2 = q / S
    ys2 = fs2 + nv
    r = y - m
    lp = -(r * r) / (2.0 * ys2) - 0.5 * np.log(2.0 * np.pi * ys2)
    lpmix = ((-0.5 * math.log(2.0 * math.pi * nv) - math.log(float(S))) - dmin * inv2v) + np.log(es)
    return dict(fmu=m, fs2=fs2, lp=lp, lp_mix=lpmix, sum_lp=float(lp.sum()),
                sum_lp_mix=float(lpmix.sum()), covered=int((np.abs(r) <= Z95 * np.sqrt(ys2)).sum()))


def onepass_fs2_np(F, first, last):
    """The one-pass variance (Σ f² − S·fmu²)/S the kernel does not use (case h)."""
    W = np.asarray(F)[:, first:last]
    S = W.shape[1]
    s1 = np.zeros(W.shape[0])
    s2 = np.zeros(W.shape[0])
    for s in range(S):
        s1 = s1 + W[:, s]
        s2 = s2 + W[:, s] * W[:, s]
    fmu = s1 / S
    return (s2 - S * fmu * fmu) / S


def _mp():
    import mpmath
    return mpmath


def predictive_mp(F, y, first, last, nv):
    """The same quantities as lists of mpf at 50 digits, the sums of the two densities, the
    covered count and ``margin`` = min_i | |y − ymu|/(Z95·sqrt(ys2)) − 1 |."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        W = np.asarray(F)[:, first:last]
        S = W.shape[1]
        v = mp.mpf(float(nv))
        c0 = -mp.log(2 * mp.pi * v) / 2 - mp.log(S)
        out = dict(fmu=[], fs2=[], lp=[], lp_mix=[])
        covered, margin = 0, mp.inf
        for i in range(W.shape[0]):
            f = [mp.mpf(float(x)) for x in W[i]]
            yi = mp.mpf(float(y[i]))
            fmu = mp.fsum(f) / S
            fs2 = mp.fsum((x - fmu) ** 2 for x in f) / S
            ys2 = fs2 + v
            ex = [-(yi - x) ** 2 / (2 * v) for x in f]
            top = max(ex)
            out["fmu"].append(fmu)
            out["fs2"].append(fs2)
            out["lp"].append(-(yi - fmu) ** 2 / (2 * ys2) - mp.log(2 * mp.pi * ys2) / 2)
            out["lp_mix"].append(c0 + top + mp.log(mp.fsum(mp.exp(e - top) for e in ex)))
            ratio = abs(yi - fmu) / (mp.mpf(Z95) * mp.sqrt(ys2))
            covered += ratio <= 1
            margin = min(margin, abs(ratio - 1))
        out["sum_lp"] = mp.fsum(out["lp"])
        out["sum_lp_mix"] = mp.fsum(out["lp_mix"])
        out["covered"] = int(covered)
        out["margin"] = float(margin)
        return out
    finally:
        mp.mp.dps = old


@functools.lru_cache(maxsize=None)
def reference(name):
    F, y, (a, b), nv = inputs(name)
    return predictive_mp(F, y, a, b, nv)


def col_err(got, ref):
    """max_i |got_i − ref_i| / max_i |ref_i| against a list of mpf (0/0 = 0, x/0 = inf)."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        num = max(abs(mp.mpf(float(g)) - r) for g, r in zip(np.asarray(got).ravel(), ref))
        den = max(abs(r) for r in ref)
        if den == 0:
            return 0.0 if num == 0 else math.inf
        return float(num / den)
    finally:
        mp.mp.dps = old


def rel_err(got, ref):
    """|got − ref|/|ref| of a double against an mpf."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return float(abs(mp.mpf(float(got)) - ref) / abs(ref))
    finally:
        mp.mp.dps = old


def sum_mp(rows):
    """The exact sum of doubles as an mpf."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return mp.fsum(mp.mpf(float(x)) for x in np.asarray(rows).ravel())
    finally:
        mp.mp.dps = old


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """{quantity: the numpy restatement's col_err against mpmath} of a case."""
    F, y, (a, b), nv = inputs(name)
    got, ref = predictive_np(F, y, a, b, nv), reference(name)
    return {q: col_err(got[q], ref[q]) for q in QUANTITIES}


def bar(name, q):
    """The device's bar: max(8 × the yardstick, (S + 16)·2^-53)."""
    a, b = CASES[name][3]
    return max(8.0 * yardstick(name)[q], (b - a + 16) * U)


# --------------------------------------------------------------------------- the meaning of fs2
DRAWS = dict(n=16, N=40, S=4000, Ntest=65, signal_var=0.05, sigma_theta=1.3, seed=9190)


@functools.lru_cache(maxsize=None)
def posterior_draws():
    """Exact draws of the full-theta model's Gaussian posterior: theta (n, S) = mean + L^-T z with
    the precision A = phi phi'/v + I/sigma_theta^2 = L L'; phitest (n, Ntest), ytest, and
    var (Ntest) = phi*' A^-1 phi*, the variance fs2 estimates from the S draws."""
    d = DRAWS
    n, N, S, Nt, v = d["n"], d["N"], d["S"], d["Ntest"], d["signal_var"]
    rng = np.random.default_rng(d["seed"])
    phi = math.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, N)))
    y = phi.T @ rng.standard_normal(n) + math.sqrt(v) * rng.standard_normal(N)
    phitest = np.asfortranarray(math.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, Nt))))
    A = phi @ phi.T / v + np.eye(n) / d["sigma_theta"] ** 2
    L = np.linalg.cholesky(A)
    mean = np.linalg.solve(A, phi @ y / v)
    theta = np.asfortranarray(mean[:, None] + np.linalg.solve(L.T, rng.standard_normal((n, S))))
    var = (np.linalg.solve(L, phitest) ** 2).sum(axis=0)
    ytest = phitest.T @ mean + math.sqrt(v) * rng.standard_normal(Nt)
    return theta, phitest, ytest, var


def draws_band():
    """5·sqrt(2/S): five standard deviations of a variance estimated from S Gaussian draws."""
    return 5.0 * math.sqrt(2.0 / DRAWS["S"])
