"""fp64 numpy restatements of the no-tensor GP marginal likelihood and its gradient, the test
cases of tests/golden/nlml_mp.npz and the error yardstick of the device parity tests.

    feature_notensor / gradfeature_notensor     GPT_SGLD.jl:109-120, :142-177
    nlogmarginal                                GPT_SGLD.jl:921-933
    gradnlogmarginal_literal                    GPT_SGLD.jl:939-962 (B, C, d, tmp, eigvalsh)
    value_and_grad_fused                        the one-GEMM form the device runs

Hyper-parameters are [length_scale (D, or 1 for the scalar form); sigma_RBF; signal_var].
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlml_mp.npz")

# (n, N, D, Lh)
CASES = [
    (33, 130, 2, 4),        # n = 1 mod 16, ragged N
    (40, 203, 4, 6),
    (48, 30, 3, 5),         # n > N: N - n < 0, rank-deficient phi phi'
    (16, 64, 1, 3),         # exact tiles, D = 1
    (100, 517, 4, 6),
    (100, 517, 4, 3),       # scalar length scale
    (128, 259, 8, 10),
    (65, 1030, 16, 18),     # maximum D, several column blocks
]
EXPERIMENT = [1.3978, 0.5, 2.8966, 7.5565, 0.9129, 0.0195]   # PowerPlantDataExperiment.jl:83-116


def case_name(case):
    return "n%d_N%d_D%d_Lh%d" % tuple(case)


def hyper_points(D, Lh):
    """The three points of every case, trimmed or extended to D (cyclically) length scales."""
    nl = Lh - 2
    exp_ls = [EXPERIMENT[k % 4] for k in range(nl)]
    return [np.array([1.0] * nl + [0.9, 0.04]),
            np.array(exp_ls + EXPERIMENT[4:]),
            np.array([0.3] * nl + [1.5, 0.001])]


def whiten(X):
    X = np.array(X, dtype=np.float64, copy=True)
    if X.ndim == 1:
        return (X - X.mean()) / X.std(ddof=1)
    return (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)


def case_inputs(case, idx):
    """X (N, D), y (N), Z (n, D), b (n): whitened PowerPlant rows for D <= 4, seeded normals
    otherwise; Z = randn, b = 2 pi rand."""
    n, N, D, _ = case
    rng = np.random.default_rng(1000 + idx)
    if D <= 4:
        pp = np.load(os.path.join(os.path.dirname(GOLDEN), "powerplant.npz"))["data"]
        rows = rng.permutation(pp.shape[0])[:N]
        X = whiten(pp[rows, :D])
        y = whiten(pp[rows, 4])
    else:
        X = rng.standard_normal((N, D))
        y = rng.standard_normal(N)
    Z = rng.standard_normal((n, D))
    b = 2 * math.pi * rng.random(n)
    return X, y, Z, b


def split(h, D):
    h = np.asarray(h, dtype=np.float64)
    if h.size not in (3, D + 2):
        raise ValueError("hyperparams must have 3 or D + 2 entries")
    ls = np.full(D, h[0]) if h.size == 3 and D != 1 else h[:D].copy()
    return ls, float(h[-2]), float(h[-1])


def _arg(X, ls, Z, b):
    Zt = Z * (1.0 / ls)[None, :]
    s = np.zeros((Z.shape[0], X.shape[0]))
    for k in range(X.shape[1]):                   # sum(X[i,:].*Zt[j,:]) left to right
        s = s + Zt[:, k:k + 1] * X[None, :, k]
    return Zt, s + b.reshape(-1, 1)


def feature_notensor(X, ls, sigma, Z, b):
    n = Z.shape[0]
    _, f = _arg(X, ls, Z, b)
    return math.sqrt(2.0 / n) * sigma * np.cos(f)


def gradfeature_notensor(X, h, Z, b):
    """(n, N, Lh - 1): d phi / d length_scale (one slice, or D of them), then d phi / d sigma_RBF."""
    n, D = Z.shape
    ls, sigma, _ = split(h, D)
    Zt, f = _arg(X, ls, Z, b)
    phisin = math.sqrt(2.0 / n) * sigma * np.sin(f)
    out = []
    if len(h) == 3:                               # scalar length scale (:142-154)
        out.append(phisin * (Zt @ X.T) / h[0])
    else:
        for k in range(D):
            out.append(phisin * np.outer(Zt[:, k], X[:, k]) / ls[k])
    out.append(math.sqrt(2.0 / n) * np.cos(f))
    return np.stack(out, axis=2)


def nlogmarginal(X, y, Z, b, h):
    n, D = Z.shape
    N = y.size
    ls, sigma, s2 = split(h, D)
    phi = feature_notensor(X, ls, sigma, Z, b)
    A = phi @ phi.T + s2 * np.eye(n)
    L = np.linalg.cholesky(A)
    bv = phi @ y
    l = np.linalg.solve(L.T, np.linalg.solve(L, bv))
    logdet = 2 * np.log(np.diag(L)).sum()
    sum1 = (N - n) * math.log(s2) / 2 + logdet / 2
    sum2 = (y @ y - bv @ l) / (2 * s2)
    return sum1 + sum2 + N * math.log(2 * math.pi) / 2


def gradnlogmarginal_literal(X, y, Z, b, h):
    n, D = Z.shape
    N = y.size
    h = np.asarray(h, dtype=np.float64)
    ls, sigma, s2 = split(h, D)
    phi = feature_notensor(X, ls, sigma, Z, b)
    A = phi @ phi.T + s2 * np.eye(n)
    L = np.linalg.cholesky(A)
    gradphi = gradfeature_notensor(X, h, Z, b)
    Lh = h.size
    grad = np.empty(Lh)
    bv = phi @ y

    def solve(v):
        return np.linalg.solve(L.T, np.linalg.solve(L, v))
    l = solve(bv)
    for k in range(Lh - 1):
        gphi = gradphi[:, :, k]
        B = gphi @ phi.T
        C = solve(B)
        d = B @ l - gphi @ y
        tmp = solve(d)
        grad[k] = np.trace(C) + (bv @ tmp) / s2
    lam = np.linalg.eigvalsh(A)
    grad[Lh - 1] = ((N - n) / (2 * s2) + (1.0 / lam).sum() / 2 + (l @ bv - y @ y) / (2 * s2 ** 2)
                    + (l @ l) / (2 * s2))
    return grad


def value_and_grad_fused(X, y, Z, b, h):
    """The rearrangement the device runs: P = A^-1, e = phi'l - y, W = P phi,
    T = S o (W + l e'/s2), d/dl_k = sum_j Zt[j,k] (T X)[j,k] / l_k."""
    n, D = Z.shape
    N = y.size
    h = np.asarray(h, dtype=np.float64)
    ls, sigma, s2 = split(h, D)
    Zt, f = _arg(X, ls, Z, b)
    c = math.sqrt(2.0 / n) * sigma
    phi, S = c * np.cos(f), c * np.sin(f)
    A = phi @ phi.T + s2 * np.eye(n)
    L = np.linalg.cholesky(A)
    bv = phi @ y
    l = np.linalg.solve(L.T, np.linalg.solve(L, bv))
    Xi = np.linalg.solve(L, np.eye(n))
    P = Xi.T @ Xi
    trP = (Xi * Xi).sum()
    yy, bl, ll = y @ y, bv @ l, l @ l
    val = ((N - n) / 2 * math.log(s2) + np.log(np.diag(L)).sum() + (yy - bl) / (2 * s2)
           + N / 2 * math.log(2 * math.pi))
    e = phi.T @ l - y
    T = S * (P @ phi + np.outer(l, e) / s2)
    gl = (Zt * (T @ X)).sum(axis=0) / ls
    grad = np.empty(h.size)
    if h.size == 3:
        grad[0] = gl.sum()
    else:
        grad[:D] = gl
    grad[-2] = (n - s2 * trP) / sigma - ll / sigma
    grad[-1] = (N - n) / (2 * s2) + trP / 2 + (bl - yy) / (2 * s2 ** 2) + ll / (2 * s2)
    return val, grad, l


class RefMarginal:
    """The callables GPNT_hyperparameters takes, on the fp64 restatement."""

    def __init__(self, X, y, Z, b):
        self.X, self.y, self.Z, self.b = (np.asarray(a, dtype=np.float64) for a in (X, y, Z, b))

    def nlogmarginal(self, h):
        return nlogmarginal(self.X, self.y, self.Z, self.b, np.asarray(h, dtype=np.float64))

    def gradnlogmarginal(self, h):
        return value_and_grad_fused(self.X, self.y, self.Z, self.b, h)[1]


def central_diff(fun, h, rel=1e-5):
    h = np.asarray(h, dtype=np.float64)
    g = np.empty(h.size)
    for k in range(h.size):
        d = rel * h[k]
        hp, hm = h.copy(), h.copy()
        hp[k] += d
        hm[k] -= d
        g[k] = (fun(hp) - fun(hm)) / (hp[k] - hm[k])
    return g


def load_golden():
    """{case name: dict(X, y, Z, b, H (3, Lh), val (3), grad (3, Lh))}"""
    z = np.load(GOLDEN)
    out = {}
    for case in CASES:
        nm = case_name(case)
        out[nm] = {k: z["%s_%s" % (nm, k)] for k in ("X", "y", "Z", "b", "H", "val", "grad")}
    return out


def rel_errors(got_val, got_grad, gold_val, gold_grad):
    """Relative error of the value and of each gradient component against the mp golden."""
    ev = abs(got_val - gold_val) / abs(gold_val)
    eg = np.abs(np.asarray(got_grad) - gold_grad) / np.abs(gold_grad)
    return ev, eg


def yardstick(g, p):
    """Per component: the larger of the two fp64 restatements' relative errors against mp at
    point p of golden case g (the bound of the device parity rule is 32 x this, floor 1e-12)."""
    args = (g["X"], g["y"], g["Z"], g["b"], g["H"][p])
    lit = gradnlogmarginal_literal(*args)
    _, fus, _ = value_and_grad_fused(*args)
    e1 = np.abs(lit - g["grad"][p]) / np.abs(g["grad"][p])
    e2 = np.abs(fus - g["grad"][p]) / np.abs(g["grad"][p])
    return np.maximum(e1, e2), e1, e2
