"""Regenerate nlml_mp.npz: the no-tensor GP negative log marginal likelihood and its gradient
(GPT_SGLD.jl:109-120, :142-177, :921-962) in mpmath at 50 digits, for every case of
tests/nlml_ref.py at three hyper-parameter points each.

    python tests/golden/make_nlml_golden.py [processes]

The literal formulas: A = phi phi' + s2 I, its Cholesky factor, l = A \\ (phi y), and per
hyper-parameter B = dphi phi', C = A \\ B, d = B l - dphi y, tmp = A \\ d, grad = tr C + b'tmp/s2.
The reference's sum(1 ./ eigvals(A)) is taken as tr(A^-1) from the same factor (equal to every
digit kept; a 50-digit symmetric eigen-solve of n = 128 takes far longer than the rest).
Zt = Z / l is formed in mp from the float64 inputs, so the golden is the true value at those
inputs; the float64 restatements round the feature argument.

Every gradient component must be at least 1e-4 of the largest feature hyper-parameter component
(so that a relative test means something): a point that fails has its length scales multiplied
by 1.25 until it passes, and the script says so.  Per case the file holds X, y, Z, b, H (3, Lh),
val (3) and grad (3, Lh) as float64.  Data only; about two CPU-minutes on 8 processes.
"""
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nlml_ref as NR  # noqa: E402


def mp_value_grad(X, y, Z, b, h):
    import mpmath as mp
    mp.mp.dps = 50
    M = mp.mpf
    n, D = Z.shape
    N = y.size
    Lh = len(h)
    hh = [M(float(v)) for v in h]
    ls = [hh[0]] * D if (Lh == 3 and D != 1) else hh[:D]
    sig, s2 = hh[-2], hh[-1]
    Xm = [[M(float(X[i, k])) for k in range(D)] for i in range(N)]
    ym = [M(float(v)) for v in y]
    Zt = [[M(float(Z[j, k])) / ls[k] for k in range(D)] for j in range(n)]
    c = mp.sqrt(M(2) / n)
    f = [[mp.fdot(Xm[i], Zt[j]) + M(float(b[j])) for i in range(N)] for j in range(n)]
    cosf = [[mp.cos(v) for v in row] for row in f]
    sinf = [[mp.sin(v) for v in row] for row in f]
    phi = [[c * sig * v for v in row] for row in cosf]
    phisin = [[c * sig * v for v in row] for row in sinf]
    A = [[None] * n for _ in range(n)]
    for j in range(n):
        for j2 in range(j + 1):
            A[j][j2] = A[j2][j] = mp.fdot(phi[j], phi[j2])
        A[j][j] += s2
    L = [[M(0)] * n for _ in range(n)]
    for j in range(n):
        d = mp.sqrt(A[j][j] - mp.fdot(L[j][:j], L[j][:j]))
        L[j][j] = d
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], L[j][:j])) / d
    Lt = [[L[i][j] for i in range(n)] for j in range(n)]        # rows of L'

    def solve(v):
        w = [None] * n
        for i in range(n):
            w[i] = (v[i] - mp.fdot(L[i][:i], w[:i])) / L[i][i]
        x = [None] * n
        for i in range(n - 1, -1, -1):
            x[i] = (w[i] - mp.fdot(Lt[i][i + 1:], x[i + 1:])) / L[i][i]
        return x
    bv = [mp.fdot(phi[j], ym) for j in range(n)]
    l = solve(bv)
    yy = mp.fdot(ym, ym)
    logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(n))
    val = ((N - n) * mp.log(s2) / 2 + logdet / 2 + (yy - mp.fdot(bv, l)) / (2 * s2)
           + N * mp.log(2 * mp.pi) / 2)
    grad = []
    for k in range(Lh - 1):
        if k == Lh - 2:
            gphi = [[c * v for v in row] for row in cosf]
        elif Lh == 3 and D != 1:
            gphi = [[phisin[j][i] * mp.fdot(Zt[j], Xm[i]) / hh[0] for i in range(N)]
                    for j in range(n)]
        else:
            gphi = [[phisin[j][i] * Zt[j][k] * Xm[i][k] / ls[k] for i in range(N)]
                    for j in range(n)]
        B = [[mp.fdot(gphi[j], phi[j2]) for j2 in range(n)] for j in range(n)]
        trC = M(0)
        for j2 in range(n):
            trC += solve([B[j][j2] for j in range(n)])[j2]
        d = [mp.fdot(B[j], l) - mp.fdot(gphi[j], ym) for j in range(n)]
        tmp = solve(d)
        grad.append(trC + mp.fdot(bv, tmp) / s2)
    trP = M(0)
    for j in range(n):
        ej = [M(1) if i == j else M(0) for i in range(n)]
        trP += solve(ej)[j]
    grad.append((N - n) / (2 * s2) + trP / 2 + (mp.fdot(l, bv) - yy) / (2 * s2 ** 2)
                + mp.fdot(l, l) / (2 * s2))
    return float(val), np.array([float(g) for g in grad])


def task(arg):
    idx, p = arg
    case = NR.CASES[idx]
    n, N, D, Lh = case
    X, y, Z, b = NR.case_inputs(case, idx)
    h = NR.hyper_points(D, Lh)[p]
    note = ""
    # the cheap fp64 form picks the point; mp then evaluates it once
    for _ in range(12):
        g = NR.value_and_grad_fused(X, y, Z, b, h)[1]
        if np.abs(g).min() >= 1e-4 * np.abs(g[:Lh - 1]).max():
            break
        h = h.copy()
        h[:Lh - 2] *= 1.25
        note = " (point replaced: length scales now %s)" % h[:Lh - 2]
    val, grad = mp_value_grad(X, y, Z, b, h)
    assert np.abs(grad).min() >= 1e-4 * np.abs(grad[:Lh - 1]).max(), (case, p, grad)
    print("%s point %d: nlml %.6f%s" % (NR.case_name(case), p, val, note), flush=True)
    return idx, p, h, val, grad


def main(procs):
    jobs = [(idx, p) for idx in range(len(NR.CASES)) for p in range(3)]
    jobs.sort(key=lambda a: -NR.CASES[a[0]][0] ** 2 * NR.CASES[a[0]][1] * NR.CASES[a[0]][3])
    with multiprocessing.Pool(procs) as pool:
        res = pool.map(task, jobs, chunksize=1)
    out = {}
    for idx, case in enumerate(NR.CASES):
        nm = NR.case_name(case)
        X, y, Z, b = NR.case_inputs(case, idx)
        mine = sorted((r for r in res if r[0] == idx), key=lambda r: r[1])
        out.update({nm + "_X": X, nm + "_y": y, nm + "_Z": Z, nm + "_b": b,
                    nm + "_H": np.stack([r[2] for r in mine]),
                    nm + "_val": np.array([r[3] for r in mine]),
                    nm + "_grad": np.stack([r[4] for r in mine])})
    np.savez_compressed(NR.GOLDEN, **out)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
