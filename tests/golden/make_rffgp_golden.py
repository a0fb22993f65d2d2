"""Generates tests/golden/rffgp_mp.npz: the closed-form predictive of the no-tensor RFF GP (fmu,
fs2, lp at three hyper points) and the kernel approximation error (frob, norm_K, max_abs at hyper
points 0 and 1) of every case of tests/rffgp_ref.py.

    N <= 259     mpmath at 50 digits from the double inputs (minutes; never run by a test)
    N  > 259     np.longdouble (x87 80-bit) with make_exactgp_golden's Cholesky

The train inputs X, y, Z, b and the hyper points H are those stored in nlml_mp.npz (checked here
against nlml_ref.case_inputs), so this file holds only Xtest, ytest and results.  The long-double
path is also evaluated on every mp case; the worst disagreement, in the measures of
rffgp_ref.pred_errors / kerr_errors, is stored (`ld_vs_mp`) and must stay under 1e-14.
Usage: python tests/golden/make_rffgp_golden.py [processes]
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import nlml_ref as NR  # noqa: E402
import rffgp_ref as RR  # noqa: E402
from make_exactgp_golden import chol_lower, tri_solve  # noqa: E402


def _arith(kind):
    """dt, the array converter and the elementary functions of one arithmetic."""
    if kind == "ld":
        pi = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)
        return (np.longdouble, lambda a: np.asarray(a, dtype=np.longdouble),
                dict(cos=np.cos, exp=np.exp, log=np.log, sqrt=np.sqrt, pi=pi))
    import mpmath as mp
    mp.mp.dps = 50
    v = lambda f: np.vectorize(f, otypes=[object])  # noqa: E731
    return (mp.mpf, lambda a: v(lambda x: mp.mpf(float(x)))(np.asarray(a, dtype=np.float64)),
            dict(cos=v(mp.cos), exp=v(mp.exp), log=v(mp.log), sqrt=mp.sqrt, pi=mp.pi))


def _features(Xh, ls, sigma, Zh, bh, dt, fn):
    n, D = Zh.shape
    f = bh[:, None] + Xh[None, :, 0] * 0
    for k in range(D):
        f = f + (Zh[:, k] / ls[k])[:, None] * Xh[None, :, k]
    return fn["sqrt"](dt(2) / dt(n)) * sigma * fn["cos"](f)


def _hyper(h, D, cv):
    hh = cv(h)
    nl = hh.size - 2
    return [hh[k if nl == D else 0] for k in range(D)], hh[-2], hh[-1]


def predict(kind, X, y, Z, b, h, Xtest, ytest):
    dt, cv, fn = _arith(kind)
    n, D = Z.shape
    Xh, yh, Zh, bh, Xt, yt = cv(X), cv(y), cv(Z), cv(b), cv(Xtest), cv(ytest)
    ls, sigma, s2 = _hyper(h, D, cv)
    phi = _features(Xh, ls, sigma, Zh, bh, dt, fn)
    A = np.dot(phi, phi.T)
    for j in range(n):
        A[j, j] = A[j, j] + s2
    L = chol_lower(A, fn["sqrt"])
    w = tri_solve(L, np.dot(phi, yh)[:, None])
    ps = _features(Xt, ls, sigma, Zh, bh, dt, fn)
    V = tri_solve(L, ps)
    fmu = np.dot(V.T, w)[:, 0]                     # phi*' L^-T L^-1 phi y
    fs2 = s2 * (V * V).sum(axis=0)
    ys2 = fs2 + s2
    half = dt(1) / dt(2)
    lp = -(yt - fmu) * (yt - fmu) / (2 * ys2) - half * fn["log"](2 * fn["pi"] * ys2)
    return fmu, fs2, lp


def kernel_error(kind, X, Z, b, h):
    dt, cv, fn = _arith(kind)
    N, D = X.shape
    Xh, Zh, bh = cv(X), cv(Z), cv(b)
    ls, sigma, _ = _hyper(h, D, cv)
    phi = _features(Xh, ls, sigma, Zh, bh, dt, fn)
    half = dt(1) / dt(2)
    sd = sk = mx = dt(0)
    for i0 in range(0, N, 64):                     # row blocks bound the memory of the large cases
        Xa = Xh[i0:i0 + 64]
        s = (Xa[:, None, 0] - Xh[None, :, 0]) * 0
        for k in range(D):
            d = (Xa[:, None, k] - Xh[None, :, k]) / ls[k]
            s = s + d * d
        K = sigma * sigma * fn["exp"](-half * s)
        d = K - np.dot(phi[:, i0:i0 + 64].T, phi)
        sd = sd + (d * d).sum()
        sk = sk + (K * K).sum()
        mx = max(mx, abs(d).max())
    return np.array([fn["sqrt"](sd), fn["sqrt"](sk), mx], dtype=object)


def _f64(a):
    return np.array([float(x) for x in np.ravel(a)]).reshape(np.shape(a))


def _diff(ld, m, scale):
    """max |ld - m| / scale with the long double kept to its 80 bits."""
    import mpmath as mp
    worst = mp.mpf(0)
    for x, yv in zip(np.ravel(ld), np.ravel(m)):
        hi = float(x)
        worst = max(worst, abs(mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi))) - yv))
    return float(worst / scale)


def work(job):
    what, ci, p = job
    case = RR.CASES[ci]
    idx = RR.CASE_IDX[ci]
    g = NR.load_golden()[RR.case_name(case)]
    X, y, Z, b = NR.case_inputs(case, idx)
    assert all(np.array_equal(a, g[k]) for a, k in ((X, "X"), (y, "y"), (Z, "Z"), (b, "b")))
    h = g["H"][p]
    use_mp = case[1] <= RR.MP_MAX_N
    if what == "pred":
        Xt, yt = RR.make_test_inputs(X, y, idx)
        ld = predict("ld", X, y, Z, b, h, Xt, yt)
        if not use_mp:
            return what, ci, p, tuple(_f64(a) for a in ld), 0.0
        m = predict("mp", X, y, Z, b, h, Xt, yt)
        sg2 = float(h[-2]) ** 2
        dis = max(_diff(ld[0], m[0], max(abs(v) for v in m[0])), _diff(ld[1], m[1], sg2),
                  _diff(ld[2], m[2], max(abs(v) for v in m[2])))
        return what, ci, p, tuple(_f64(a) for a in m), dis
    ld = kernel_error("ld", X, Z, b, h)
    if not use_mp:
        return what, ci, p, _f64(ld), 0.0
    m = kernel_error("mp", X, Z, b, h)
    dis = max(_diff(ld[q:q + 1], m[q:q + 1], m[q]) for q in range(3))
    return what, ci, p, _f64(m), dis


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, (os.cpu_count() or 2) - 1)
    jobs = [("pred", ci, p) for ci in range(len(RR.CASES)) for p in range(3)]
    jobs += [("kerr", ci, p) for ci in range(len(RR.CASES)) for p in RR.KERR_POINTS]
    cost = lambda j: RR.CASES[j[1]][1] ** 2 * RR.CASES[j[1]][0] * (1 if j[0] == "kerr" else 0.3)  # noqa: E731
    jobs.sort(key=lambda j: -cost(j))
    with Pool(procs) as pool:
        done = pool.map(work, jobs, chunksize=1)
    out, worst = {}, 0.0
    for ci, case in enumerate(RR.CASES):
        nm = RR.case_name(case)
        X, y, _, _ = NR.case_inputs(case, RR.CASE_IDX[ci])
        Xt, yt = RR.make_test_inputs(X, y, RR.CASE_IDX[ci])
        pred = {p: r for w, c, p, r, _ in done if w == "pred" and c == ci}
        kerr = {p: r for w, c, p, r, _ in done if w == "kerr" and c == ci}
        out.update({nm + "_Xtest": Xt, nm + "_ytest": yt})
        for q, key in enumerate(("fmu", "fs2", "lp")):
            out[nm + "_" + key] = np.stack([pred[p][q] for p in range(3)])
        out[nm + "_kerr"] = np.stack([kerr[p] for p in RR.KERR_POINTS])
    for w, c, p, _, dis in done:
        print("%s %s point %d: long double vs mp %.2e" % (w, RR.case_name(RR.CASES[c]), p, dis))
        worst = max(worst, dis)
    assert worst <= 1e-14, worst
    out["ld_vs_mp"] = np.array(worst)
    np.savez_compressed(RR.GOLDEN, **out)
    print("wrote %s, worst long double vs mp disagreement %.2e" % (RR.GOLDEN, worst))


if __name__ == "__main__":
    main()
