"""fp64 numpy restatements of the closed-form predictive of the no-tensor RFF GP and of the
kernel approximation error, the test cases of tests/golden/rffgp_mp.npz and the error yardstick
of the device parity tests.

    model (GPT_SGLD.jl:921-933)   y = phi(x)'theta + eps, theta ~ N(0, I), eps ~ N(0, s2)
    predict_chol                  A = phi phi' + s2 I = L L', l = A^-1 phi y,
                                  fmu = phi*'l, fs2 = s2 colsum((L^-1 phi*)^2)
    predict_lu                    fs2 = s2 diag(phi*' solve(A, phi*))
    kernel_error_literal          K - phi.T @ phi  (PowerPlantDataExperiment.jl:47-97)
    kernel_error_blocked          the same in 64-row blocks, summed block by block

Hyper-parameters are [length_scale (D, or 1 for the scalar form); sigma_RBF; signal_var].  The
train inputs and hyper points are those of tests/golden/nlml_mp.npz.
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import collections
import math
import os

import numpy as np

import nlml_ref as NR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rffgp_mp.npz")

# the cases of nlml_ref.CASES this model is tested on (index there, for case_inputs' seed)
CASE_IDX = [0, 2, 3, 5, 6, 7]
CASES = [NR.CASES[i] for i in CASE_IDX]
NTEST = 77
MP_MAX_N = 259            # mpmath up to this N, long double above
KERR_POINTS = (0, 1)      # the hyper points of the kernel-error golden

Prediction = collections.namedtuple("Prediction", "ymu ys2 fmu fs2 lp")
KernelError = collections.namedtuple("KernelError", "frob norm_K max_abs")


def case_name(case):
    return NR.case_name(case)


def make_test_inputs(X, y, idx):
    """Xtest (77, D), ytest (77): jittered train rows."""
    rng = np.random.default_rng(7000 + idx)
    N, D = X.shape
    rows = rng.integers(0, N, NTEST)
    Xtest = X[rows] + 0.3 * rng.standard_normal((NTEST, D))
    ytest = y[rows] + 0.1 * rng.standard_normal(NTEST)
    return Xtest, ytest


def _lp(ytest, ymu, ys2):
    return -(ytest - ymu) ** 2 / (2 * ys2) - 0.5 * np.log(2 * math.pi * ys2)


def _fit(X, y, Z, b, h):
    n, D = Z.shape
    ls, sigma, s2 = NR.split(h, D)
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    A = phi @ phi.T + s2 * np.eye(n)
    return ls, sigma, s2, phi, A


def predict_chol(X, y, Z, b, h, Xtest, ytest=None):
    ls, sigma, s2, phi, A = _fit(X, y, Z, b, h)
    L = np.linalg.cholesky(A)
    l = np.linalg.solve(L.T, np.linalg.solve(L, phi @ y))
    ps = NR.feature_notensor(Xtest, ls, sigma, Z, b)
    fmu = ps.T @ l
    V = np.linalg.solve(L, ps)
    fs2 = s2 * (V * V).sum(axis=0)
    lp = _lp(ytest, fmu, fs2 + s2) if ytest is not None else None
    return Prediction(fmu, fs2 + s2, fmu, fs2, lp)


def predict_lu(X, y, Z, b, h, Xtest, ytest=None):
    ls, sigma, s2, phi, A = _fit(X, y, Z, b, h)
    l = np.linalg.solve(A, phi @ y)
    ps = NR.feature_notensor(Xtest, ls, sigma, Z, b)
    fmu = ps.T @ l
    fs2 = s2 * (ps * np.linalg.solve(A, ps)).sum(axis=0)
    lp = _lp(ytest, fmu, fs2 + s2) if ytest is not None else None
    return Prediction(fmu, fs2 + s2, fmu, fs2, lp)


def push_through_mean(X, y, Z, b, h, Xtest):
    """fmu = k*'(K_rff + s2 I)^-1 y, the N x N form of the same mean."""
    ls, sigma, s2 = NR.split(h, Z.shape[1])
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    ps = NR.feature_notensor(Xtest, ls, sigma, Z, b)
    return (ps.T @ phi) @ np.linalg.solve(phi.T @ phi + s2 * np.eye(y.size), y)


def se_kernel(Xa, Xb, ls, sigma):
    s = np.zeros((Xa.shape[0], Xb.shape[0]))
    for k in range(Xa.shape[1]):
        d = (Xa[:, None, k] - Xb[None, :, k]) / ls[k]
        s = s + d * d
    return sigma ** 2 * np.exp(-0.5 * s)


def kernel_error_literal(X, Z, b, h):
    ls, sigma, _ = NR.split(h, Z.shape[1])
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    K = se_kernel(X, X, ls, sigma)
    d = K - phi.T @ phi
    return KernelError(math.sqrt((d ** 2).sum()), math.sqrt((K ** 2).sum()), np.abs(d).max())


def kernel_error_blocked(X, Z, b, h, rows=64):
    ls, sigma, _ = NR.split(h, Z.shape[1])
    phi = NR.feature_notensor(X, ls, sigma, Z, b)
    sd = sk = mx = 0.0
    for i0 in range(0, X.shape[0], rows):
        K = se_kernel(X[i0:i0 + rows], X, ls, sigma)
        d = K - phi[:, i0:i0 + rows].T @ phi
        sd += (d * d).sum()
        sk += (K * K).sum()
        mx = max(mx, np.abs(d).max())
    return KernelError(math.sqrt(sd), math.sqrt(sk), mx)


def load_golden():
    """{case name: dict(X, y, Z, b, H (3, Lh) from nlml_mp.npz; Xtest, ytest, fmu, fs2, lp
    (3, 77), kerr (2, 3): frob, norm_K, max_abs at hyper points 0 and 1)}"""
    z = np.load(GOLDEN)
    train = NR.load_golden()
    out = {}
    for case in CASES:
        nm = case_name(case)
        g = {k: train[nm][k] for k in ("X", "y", "Z", "b", "H")}
        g.update({k: z["%s_%s" % (nm, k)] for k in ("Xtest", "ytest", "fmu", "fs2", "lp", "kerr")})
        out[nm] = g
    return out


PRED_QUANT = ("fmu", "fs2", "lp")


def pred_errors(res, g, p):
    """fmu over max|fmu|, fs2 over sigma_RBF^2, lp over max|lp| against golden point p."""
    sg2 = float(g["H"][p][-2]) ** 2
    return {"fmu": np.abs(res.fmu - g["fmu"][p]).max() / np.abs(g["fmu"][p]).max(),
            "fs2": np.abs(res.fs2 - g["fs2"][p]).max() / sg2,
            "lp": np.abs(res.lp - g["lp"][p]).max() / np.abs(g["lp"][p]).max()}


def pred_yardstick(g, p):
    """Per quantity: the larger of the two restatements' errors against the golden (the device
    bound is 32 x this, floor 1e-12), and the two errors."""
    args = (g["X"], g["y"], g["Z"], g["b"], g["H"][p], g["Xtest"], g["ytest"])
    e1 = pred_errors(predict_chol(*args), g, p)
    e2 = pred_errors(predict_lu(*args), g, p)
    return {k: max(e1[k], e2[k]) for k in PRED_QUANT}, e1, e2


def kerr_errors(res, g, q):
    """Relative errors of (frob, norm_K, max_abs) against the golden's row q (point KERR_POINTS[q])."""
    return np.abs(np.asarray(res, dtype=np.float64) - g["kerr"][q]) / np.abs(g["kerr"][q])


def kerr_yardstick(g, q):
    args = (g["X"], g["Z"], g["b"], g["H"][KERR_POINTS[q]])
    e1 = kerr_errors(kernel_error_literal(*args), g, q)
    e2 = kerr_errors(kernel_error_blocked(*args), g, q)
    return np.maximum(e1, e2), e1, e2
