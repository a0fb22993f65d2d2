"""fp64 numpy restatements of exact GP regression (squared-exponential kernel, iso or ARD, Gaussian
noise, zero mean), the test cases of tests/golden/exactgp_mp.npz and the error yardstick of the
device parity tests.

    K_ij = sigma_RBF^2 exp(-1/2 sum_k ((x_ik - x_jk)/l_k)^2),  A = K + signal_var I = L L',
    alpha = A^-1 y,  nlml = sum log L_ii + y'alpha/2 + (N/2) log 2 pi        (GP_nlogmarginal)
    grad  = 1/2 sum_ij Q_ij dA_ij/dh,  Q = A^-1 - alpha alpha'
    fmu = Ks'alpha, fs2 = max(sigma_RBF^2 - colsum((L^-1 Ks)^2), 0), ys2 = fs2 + signal_var,
    lp = -(y - fmu)^2/(2 ys2) - log(2 pi ys2)/2                              (prediction)

    literal     cholesky, Q by solves, one sum(Q o dK)/2 per hyper-parameter, v = L \\ Ks
    fused       P = W'W through W = L^-1, a single pass over (P - alpha alpha') o K,
                fs2 = sigma^2 - diag(Ks'P Ks) with P applied as W'W (the product P Ks loses
                cond(A) eps against sigma^2 and would only slacken the yardstick): the arrangement
                the device runs

Hyper-parameters are h = [length_scale (D entries, or one); sigma_RBF; signal_var].
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import math
import os
from collections import namedtuple

import numpy as np

from nlml_ref import central_diff, whiten  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "exactgp_mp.npz")
NB = 64                      # the device Cholesky's panel width (gpt_amd/csrc/exactgp.hip kEgpNB)

# (N, D, Lh, Ntest)
CASES = [
    (1, 1, 3, 3),
    (15, 2, 4, 5),
    (16, 1, 3, 16),
    (17, 3, 5, 7),
    (33, 2, 4, 33),
    (130, 4, 6, 64),
    (130, 4, 3, 64),
    (200, 16, 18, 40),
    (259, 8, 10, 100),
    (517, 4, 6, 130),
    (1100, 4, 6, 300),
    (NB - 1, 4, 6, 20),
    (NB, 4, 6, 20),
    (NB + 1, 4, 6, 20),
]
MP_MAX_N = 259               # mpmath up to here, long double above
EXACT = [1.4426, 0.5, 4.0272, 7.3516, 0.8296, 0.0205]     # DataRecords.txt:384, l_2 set to 0.5

Result = namedtuple("Result", "val grad alpha fmu fs2 lp")


def case_name(case):
    return "N%d_D%d_Lh%d_T%d" % tuple(case)


def hyper_points(D, Lh):
    """The three points of every case, trimmed or extended (cyclically) to Lh - 2 length scales."""
    nl = Lh - 2
    ls = [EXACT[k % 4] for k in range(nl)]
    return [np.array([1.0] * nl + [0.9, 0.04]),
            np.array(ls + EXACT[4:]),
            np.array([0.3] * nl + [1.5, 0.001])]


def case_inputs(case, idx):
    """X (N, D), y (N), Xtest (Ntest, D), ytest (Ntest): PowerPlant rows whitened with the train
    rows' statistics when D <= 4 and N >= 16, seeded normals otherwise; the test rows come from
    the same pool and are disjoint from the train rows."""
    N, D, _, Nt = case
    rng = np.random.default_rng(2003 + idx)     # 2003: |y| = 1.34 at N = 1, so that |nlml| >= 1 there
    if D <= 4 and N >= 16:
        pp = np.load(os.path.join(HERE, "golden", "powerplant.npz"))["data"]
        rows = rng.permutation(pp.shape[0])[:N + Nt]
        Xa, ya = pp[rows, :D], pp[rows, 4]
        mu, sd = Xa[:N].mean(axis=0), Xa[:N].std(axis=0, ddof=1)
        ym, ys = ya[:N].mean(), ya[:N].std(ddof=1)
        Xa, ya = (Xa - mu) / sd, (ya - ym) / ys
    else:
        Xa = rng.standard_normal((N + Nt, D))
        ya = rng.standard_normal(N + Nt)
    return Xa[:N].copy(), ya[:N].copy(), Xa[N:].copy(), ya[N:].copy()


def split(h, D):
    h = np.asarray(h, dtype=np.float64)
    if h.size not in (3, D + 2):
        raise ValueError("hyperparams must have 3 or D + 2 entries")
    ls = np.full(D, h[0]) if h.size == 3 and D != 1 else h[:D].copy()
    return ls, float(h[-2]), float(h[-1])


def sqdiff(Xa, Xb):
    """(D, Na, Nb): (x_ik - x_jk)^2"""
    return np.stack([(Xa[:, None, k] - Xb[None, :, k]) ** 2 for k in range(Xa.shape[1])])


def kernel(Xa, Xb, ls, sigma):
    s = np.zeros((Xa.shape[0], Xb.shape[0]))
    for k in range(Xa.shape[1]):
        d = (Xa[:, None, k] - Xb[None, :, k]) / ls[k]
        s = s + d * d
    return sigma ** 2 * np.exp(-0.5 * s)


def _lp(ytest, fmu, ys2):
    return -(ytest - fmu) ** 2 / (2 * ys2) - 0.5 * np.log(2 * math.pi * ys2)


def _pack(h, D, gl, gs, gv):
    g = np.empty(np.asarray(h).size)
    if g.size == D + 2:
        g[:D] = gl
    else:
        g[0] = gl.sum()
    g[-2], g[-1] = gs, gv
    return g


def literal(X, y, h, Xtest=None, ytest=None):
    N, D = X.shape
    ls, sigma, s2 = split(h, D)
    K = kernel(X, X, ls, sigma)
    L = np.linalg.cholesky(K + s2 * np.eye(N))
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    val = np.log(np.diag(L)).sum() + 0.5 * (y @ alpha) + 0.5 * N * math.log(2 * math.pi)
    Q = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(N))) - np.outer(alpha, alpha)
    d2 = sqdiff(X, X)
    gl = np.array([(Q * (K * d2[k] / ls[k] ** 3)).sum() / 2 for k in range(D)])
    gs = (Q * (2 * K / sigma)).sum() / 2
    gv = np.trace(Q) / 2
    fmu = fs2 = lp = None
    if Xtest is not None:
        Ks = kernel(X, Xtest, ls, sigma)
        v = np.linalg.solve(L, Ks)
        fmu = Ks.T @ alpha
        fs2 = np.maximum(sigma ** 2 - (v * v).sum(axis=0), 0.0)
        if ytest is not None:
            lp = _lp(ytest, fmu, fs2 + s2)
    return Result(val, _pack(h, D, gl, gs, gv), alpha, fmu, fs2, lp)


def fused(X, y, h, Xtest=None, ytest=None):
    N, D = X.shape
    ls, sigma, s2 = split(h, D)
    K = kernel(X, X, ls, sigma)
    L = np.linalg.cholesky(K + s2 * np.eye(N))
    W = np.linalg.solve(L, np.eye(N))
    P = W.T @ W
    z = W @ y
    alpha = W.T @ z
    val = np.log(np.diag(L)).sum() + 0.5 * (z @ z) + 0.5 * N * math.log(2 * math.pi)
    QK = (P - np.outer(alpha, alpha)) * K
    d2 = sqdiff(X, X)
    gl = np.array([0.5 * (QK * d2[k]).sum() / ls[k] ** 3 for k in range(D)])
    gs = QK.sum() / sigma
    gv = 0.5 * (np.trace(P) - alpha @ alpha)
    fmu = fs2 = lp = None
    if Xtest is not None:
        Ks = kernel(X, Xtest, ls, sigma)
        fmu = Ks.T @ alpha
        V = W @ Ks                       # diag(Ks'P Ks) through P's factor, P = W'W
        fs2 = np.maximum(sigma ** 2 - (V * V).sum(axis=0), 0.0)
        if ytest is not None:
            lp = _lp(ytest, fmu, fs2 + s2)
    return Result(val, _pack(h, D, gl, gs, gv), alpha, fmu, fs2, lp)


def dnlz_log(grad, h):
    """GPkit's dnlZ: the gradient with respect to log l, log sigma_RBF and log sqrt(signal_var)."""
    h = np.asarray(h, dtype=np.float64)
    f = h.copy()
    f[-1] = 2 * h[-1]
    return np.asarray(grad) * f


def nlz_log(X, y, lh, D):
    """The value as a function of GPkit's log hyper-parameters [log l; log sf; log sn]."""
    lh = np.asarray(lh, dtype=np.float64)
    h = np.exp(lh)
    h[-1] = math.exp(2 * lh[-1])
    return literal(X, y, h).val


def GP_nlogmarginal(X, y, signal_var, sigma_RBF2, length_scale):
    """GPT_SGLD.jl:905-915's signature on the literal restatement."""
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    return literal(X, y, np.concatenate([ls, [math.sqrt(sigma_RBF2), signal_var]])).val


class RefExact:
    """The callables GPNT_hyperparameters takes, on the fp64 restatement."""

    def __init__(self, X, y):
        self.X, self.y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def nlogmarginal(self, h):
        return literal(self.X, self.y, np.asarray(h, dtype=np.float64)).val

    def gradnlogmarginal(self, h):
        return fused(self.X, self.y, np.asarray(h, dtype=np.float64)).grad


QUANT = ("val", "grad", "fmu", "fs2", "ys2", "lp")


def errors(res, gold, h):
    """The error of each quantity of a Result against a golden point, in the parity rule's
    measures: value relative, gradient per component relative (absolute where the golden component
    is exactly zero: the length-scale derivative at N = 1), fmu over max|fmu|, fs2 and ys2 over
    sigma_RBF^2, lp over max|lp|."""
    s2, sg2 = float(h[-1]), float(h[-2]) ** 2
    return {
        "val": abs(res.val - gold["val"]) / abs(gold["val"]),
        "grad": np.abs(res.grad - gold["grad"]) / np.where(gold["grad"] == 0, 1.0, np.abs(gold["grad"])),
        "fmu": np.abs(res.fmu - gold["fmu"]).max() / np.abs(gold["fmu"]).max(),
        "fs2": np.abs(res.fs2 - gold["fs2"]).max() / sg2,
        "ys2": np.abs((res.fs2 + s2) - (gold["fs2"] + s2)).max() / sg2,
        "lp": np.abs(res.lp - gold["lp"]).max() / np.abs(gold["lp"]).max(),
    }


def load_golden():
    """{case name: dict(X, y, Xtest, ytest, H (3, Lh), val (3), grad (3, Lh), fmu, fs2, lp (3, Ntest))}"""
    z = np.load(GOLDEN)
    keys = ("X", "y", "Xtest", "ytest", "H", "val", "grad", "fmu", "fs2", "lp")
    return {case_name(c): {k: z["%s_%s" % (case_name(c), k)] for k in keys} for c in CASES}


def point(g, p):
    return {k: g[k][p] for k in ("val", "grad", "fmu", "fs2", "lp")}


def yardstick(g, p):
    """Per quantity: the larger of the two fp64 restatements' errors against the golden at point p
    of case g (the device bound is 32 x this, floor 1e-12), and the two errors."""
    h = g["H"][p]
    gold = point(g, p)
    e1 = errors(literal(g["X"], g["y"], h, g["Xtest"], g["ytest"]), gold, h)
    e2 = errors(fused(g["X"], g["y"], h, g["Xtest"], g["ytest"]), gold, h)
    return {k: np.maximum(e1[k], e2[k]) for k in QUANT}, e1, e2
