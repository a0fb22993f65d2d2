"""Generates tests/golden/exactgp_mp.npz: the exact-GP value, gradient and predictions of every
case and hyper point of tests/exactgp_ref.py.

    N <= 259     mpmath at 50 digits (minutes; never run by a test)
    N  > 259     np.longdouble (x87 80-bit) with the hand-written Cholesky below

The long-double path is also evaluated on every mp case; the worst relative disagreement is stored
(`ld_vs_mp`) and must stay under 1e-14, two decades under the parity floor, or the large cases
would have to take mp as well.  Every stored value has |value| >= 1 so relative errors mean
something.  Usage: python tests/golden/make_exactgp_golden.py [processes]
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import exactgp_ref as ER  # noqa: E402


# ------------------------------------------------------------------ generic dense algebra
# Works on any numpy dtype whose scalars carry +, -, *, / (object arrays of mpf, longdouble).
def chol_lower(A, sqrt):
    A = A.copy()
    n = A.shape[0]
    for j in range(n):
        A[j, j] = sqrt(A[j, j])
        if j + 1 < n:
            A[j + 1:, j] = A[j + 1:, j] / A[j, j]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(A[j + 1:, j], A[j + 1:, j])
        A[j, j + 1:] = A[j, j + 1:] * 0
    return A


def tri_solve(L, B):
    """L^-1 B by forward substitution, all columns at once."""
    X = B.copy()
    for j in range(L.shape[0]):
        if j:
            X[j] = X[j] - np.dot(L[j, :j], X[:j])
        X[j] = X[j] / L[j, j]
    return X


def evaluate(X, y, h, Xtest, ytest, dt, fn):
    """Value, gradient, fmu, fs2, lp in the arithmetic of dt / fn (exp, log, sqrt, pi)."""
    N, D = X.shape
    cv = np.vectorize(dt, otypes=[object]) if dt is not np.longdouble else (lambda a: np.asarray(a, dtype=np.longdouble))
    Xh, yh, Xt, yt, hh = cv(X), cv(y), cv(Xtest), cv(ytest), cv(np.asarray(h, dtype=np.float64))
    nl = hh.size - 2
    ls = [hh[k if nl == D else 0] for k in range(D)]
    sigma, s2 = hh[-2], hh[-1]
    vexp = np.vectorize(fn["exp"], otypes=[object]) if dt is not np.longdouble else np.exp
    vlog = np.vectorize(fn["log"], otypes=[object]) if dt is not np.longdouble else np.log
    half = dt(1) / dt(2)

    def kern(Xa, Xb):
        s = (Xa[:, None, 0] - Xb[None, :, 0]) * 0
        for k in range(D):
            d = (Xa[:, None, k] - Xb[None, :, k]) / ls[k]
            s = s + d * d
        return sigma * sigma * vexp(-half * s)
    K = kern(Xh, Xh)
    A = K.copy()
    for i in range(N):
        A[i, i] = A[i, i] + s2
    L = chol_lower(A, fn["sqrt"])
    eye = K * 0
    for i in range(N):
        eye[i, i] = dt(1)
    W = tri_solve(L, eye)
    z = np.dot(W, yh)
    alpha = np.dot(W.T, z)
    val = vlog(np.diagonal(L)).sum() + half * np.dot(z, z) + dt(N) * half * fn["log"](2 * fn["pi"])
    P = np.dot(W.T, W)
    QK = (P - np.outer(alpha, alpha)) * K
    gl = []
    for k in range(D):
        d = Xh[:, None, k] - Xh[None, :, k]
        gl.append(half * (QK * d * d).sum() / (ls[k] * ls[k] * ls[k]))
    grad = ([sum(gl)] if nl != D else gl) + [QK.sum() / sigma,
                                              half * (np.trace(P) - np.dot(alpha, alpha))]
    Ks = kern(Xh, Xt)
    V = np.dot(W, Ks)
    fmu = np.dot(Ks.T, alpha)
    fs2 = sigma * sigma - (V * V).sum(axis=0)
    fs2 = np.where(fs2 > 0, fs2, fs2 * 0)
    ys2 = fs2 + s2
    lp = -(yt - fmu) * (yt - fmu) / (2 * ys2) - half * vlog(2 * fn["pi"] * ys2)
    return val, np.array(grad), fmu, fs2, lp


def ld_eval(X, y, h, Xtest, ytest):
    """The long-double evaluation (also the optimiser test's reference at its end point)."""
    fn = {"exp": np.exp, "log": np.log, "sqrt": np.sqrt, "pi": np.longdouble(np.pi) +
          np.longdouble(1.2246467991473532e-16)}       # pi to 80 bits: the double and its remainder
    return evaluate(X, y, h, Xtest, ytest, np.longdouble, fn)


def mp_eval(X, y, h, Xtest, ytest):
    import mpmath as mp
    mp.mp.dps = 50
    fn = {"exp": mp.exp, "log": mp.log, "sqrt": mp.sqrt, "pi": mp.pi}
    return evaluate(X, y, h, Xtest, ytest, mp.mpf, fn)


def _to_f64(r):
    return tuple(np.array(a, dtype=object).astype(np.float64) if np.ndim(a) else float(a) for a in r)


def _rel(a, b):
    """Worst disagreement of a long-double result with an mp one, each quantity in the measure of
    exactgp_ref.errors."""
    import mpmath as mp
    out = [abs(mp.mpf(float(a[0])) + mp.mpf(float(a[0] - np.longdouble(float(a[0])))) - b[0]) / abs(b[0])]
    for q, scale in ((1, None), (2, "max"), (3, "max"), (4, "max")):
        d = [abs(mp.mpf(float(x)) + mp.mpf(float(x - np.longdouble(float(x)))) - yv)
             for x, yv in zip(a[q], b[q])]
        if scale is None:
            out.append(max(dd / abs(yv) if yv != 0 else dd for dd, yv in zip(d, b[q])))   # N = 1: d/dl = 0
        else:
            out.append(max(d) / max(max(abs(yv) for yv in b[q]), mp.mpf(10) ** -300))
    return float(max(out))


def work(job):
    ci, p = job
    case = ER.CASES[ci]
    X, y, Xt, yt = ER.case_inputs(case, ci)
    h = ER.hyper_points(case[1], case[2])[p]
    ld = ld_eval(X, y, h, Xt, yt)
    if case[0] <= ER.MP_MAX_N:
        m = mp_eval(X, y, h, Xt, yt)
        return ci, p, _to_f64(m), _rel(ld, m)
    return ci, p, _to_f64(ld), 0.0


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, (os.cpu_count() or 2) - 1)
    jobs = [(ci, p) for ci in range(len(ER.CASES)) for p in range(3)]
    jobs.sort(key=lambda j: -ER.CASES[j[0]][0])
    with Pool(procs) as pool:
        done = pool.map(work, jobs, chunksize=1)
    out, worst = {}, 0.0
    for ci, case in enumerate(ER.CASES):
        nm = ER.case_name(case)
        X, y, Xt, yt = ER.case_inputs(case, ci)
        res = {p: r for c, p, r, _ in done if c == ci}
        out.update({nm + "_X": X, nm + "_y": y, nm + "_Xtest": Xt, nm + "_ytest": yt,
                    nm + "_H": np.stack(ER.hyper_points(case[1], case[2]))})
        for q, key in enumerate(("val", "grad", "fmu", "fs2", "lp")):
            out[nm + "_" + key] = np.stack([np.asarray(res[p][q]) for p in range(3)])
        assert (np.abs(out[nm + "_val"]) >= 1.0).all(), (nm, out[nm + "_val"])
    for c, p, _, dis in done:
        print("%s point %d: long double vs mp %.2e" % (ER.case_name(ER.CASES[c]), p, dis))
        worst = max(worst, dis)
    assert worst <= 1e-14, worst
    out["ld_vs_mp"] = np.array(worst)
    np.savez_compressed(ER.GOLDEN, **out)
    print("wrote %s, worst long double vs mp disagreement %.2e" % (ER.GOLDEN, worst))


if __name__ == "__main__":
    main()
