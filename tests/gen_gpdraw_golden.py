"""Makes tests/golden/gpdraw_mp.npz: the function draws of tests/gpdraw_ref.py's cases evaluated with
mpmath at 50 digits from the fp64 inputs of case_inputs (kernel, features, Cholesky factors, solves
and products all in mpmath), rounded to fp64 at the end.  Per case: the inputs, Fprior, fmu, Fpost
(observed = 0), cov (Ntest <= 100), and for the cases with an RFF model l and theta.

    python tests/gen_gpdraw_golden.py            (a few minutes, pure-Python mpmath)
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpdraw_ref as R  # noqa: E402

mp.dps = 50


def M(a):
    """fp64 array -> nested lists of mpf (exact)."""
    a = np.asarray(a, dtype=np.float64)
    return [mpf(float(v)) for v in a] if a.ndim == 1 else [[mpf(float(v)) for v in row] for row in a]


def dot(a, b):
    return mp.fdot(a, b)


def kern(Xa, Xb, ls, sig2):
    return [[sig2 * mp.exp(-sum(((p - q) / l) ** 2 for p, q, l in zip(xa, xb, ls)) / 2)
             for xb in Xb] for xa in Xa]


def chol(A):
    """Rows of the lower Cholesky factor of A (rows of its lower triangle suffice)."""
    n = len(A)
    L = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(i):
            Li[j] = (A[i][j] - dot(Li[:j], L[j][:j])) / L[j][j]
        d = A[i][i] - dot(Li[:i], Li[:i])
        assert d > 0, (i, d)
        Li[i] = mp.sqrt(d)
    return L


def fwd(L, b):
    """L^-1 b."""
    x = []
    for i in range(len(L)):
        x.append((b[i] - dot(L[i][:i], x)) / L[i][i])
    return x


def bwd(L, b):
    """L^-T b."""
    n = len(L)
    x = [mpf(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - sum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
    return x


def cols(Z):
    return [list(c) for c in zip(*Z)]


def tri_times(L, Zc):
    """Columns of L Z from the columns of Z."""
    return [[dot(L[i][:i + 1], z[:i + 1]) for i in range(len(L))] for z in Zc]


def F64(colmajor_cols):
    return np.array([[float(v) for v in c] for c in colmajor_cols]).T


def one_case(idx):
    N, D, Lh, Nt = R.CASES[idx]
    c = R.case_inputs(idx)
    h = c["h"]
    ls = [mpf(float(h[k if Lh == D + 2 else 0])) for k in range(D)]
    sig, s2, jit = mpf(float(h[-2])), mpf(float(h[-1])), mpf(R.JITTER)
    X, y, Xt = M(c["X"]), M(c["y"]), M(c["Xtest"])
    out = dict(c)
    K = kern(X, X, ls, sig * sig)
    Kj = [row[:] for row in K]
    for i in range(N):
        Kj[i][i] += jit
    out["Fprior"] = F64(tri_times(chol(Kj), cols(M(c["Zprior"]))))
    for i in range(N):
        K[i][i] += s2
    L = chol(K)
    alpha = bwd(L, fwd(L, y))
    Ks = kern(Xt, X, ls, sig * sig)                    # row a: k(x*_a, X)
    fmu = [dot(r, alpha) for r in Ks]
    V = [fwd(L, r) for r in Ks]                        # row a: column a of L^-1 Ks
    Kss = kern(Xt, Xt, ls, sig * sig)
    cov = [[Kss[a][b] - dot(V[a], V[b]) for b in range(Nt)] for a in range(Nt)]
    out["fmu"] = np.array([float(v) for v in fmu])
    if Nt <= R.COV_MAX_NT:
        out["cov"] = np.array([[float(v) for v in r] for r in cov])
    for a in range(Nt):
        cov[a][a] += jit
    LZ = tri_times(chol(cov), cols(M(c["Zpost"])))
    out["Fpost"] = F64([[m + v for m, v in zip(fmu, col)] for col in LZ])
    if R.RFF_N[idx]:
        n = R.RFF_N[idx]
        Zf, bf = M(c["Zf"]), M(c["bf"])
        cf = mp.sqrt(mpf(2) / n) * sig
        phi = [[cf * mp.cos(sum(zf / l * x for zf, l, x in zip(Zf[j], ls, X[i])) + bf[j])
                for i in range(N)] for j in range(n)]
        A = [[dot(phi[a], phi[b]) if b <= a else mpf(0) for b in range(n)] for a in range(n)]
        for a in range(n):
            A[a][a] += s2
        La = chol(A)
        l = bwd(La, fwd(La, [dot(r, y) for r in phi]))
        sq = mp.sqrt(s2)
        th = [[m + sq * v for m, v in zip(l, bwd(La, z))] for z in cols(M(c["Ztheta"]))]
        out["l"] = np.array([float(v) for v in l])
        out["theta"] = F64(th)
    return out


def main():
    store = {}
    for idx, case in enumerate(R.CASES):
        for k, v in one_case(idx).items():
            store["%s/%s" % (R.case_name(case), k)] = v
        print("case", R.case_name(case), "done", flush=True)
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **store)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
