"""Regenerate gibbs_mp.npz: the mpmath (50 digits) references of every case of oracle.gibbs_cases
(tensor-GP Gibbs, geodesic Monte Carlo, MovieLens Gibbs, the Gaussian draw alone) and the CPU-only
measurements that go with them: the high-precision side of tests/test_gpu_gibbs.py and
tests/test_gibbs_cases.py.

    python tests/golden/make_gibbs_golden.py [processes]

Per case `key` (oracle.gibbs_cases.key): key_digest (SHA-256 of the case and its inputs, which are
regenerated from shape and seed, not stored); key_<quantity>_hi / _lo for the family's quantities
(oracle.gibbs_cases.QUANTITIES; the stored sweep or epoch first), hi float64 + lo float32 = the true
value to about 2^-77; key_numpy and key_f64 (the errors of the numpy restatement of record and of
this suite's own float64 run against mpmath, in the order of QUANTITIES, NaN where a case has none)
and key_seconds.  Per family: u_family = the largest key_numpy over the family's cases and
bar_family = MARGIN·u, the device's bar.  Data only; nothing comes from the device.

About 15 s on eight cores, a minute on one (the 100 × 100 precision of w at r = 10 over 592 ratings
and the 180 × 180 precision of U_k take 10 s each).
"""
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import gibbs_cases as GC  # noqa: E402


def _one(c):
    t0 = time.time()
    packed = GC.pack(c, GC.compute(c))
    sec = time.time() - t0
    qs = GC.QUANTITIES[c.family]
    ref = {q: (packed[q + "_hi"], packed[q + "_lo"].astype(np.float64)) for q in qs if q + "_hi" in packed}
    e_np, e_64 = GC.rel_err(c, GC.run_numpy(c), ref), GC.rel_err(c, GC.run_f64(c), ref)
    nan = float("nan")
    return (GC.key(c), GC.digest(c), packed, np.array([e_np.get(q, nan) for q in qs]),
            np.array([e_64.get(q, nan) for q in qs]), sec)


def _cost(c):
    if c.family == "tgp":
        return (c.n * c.r) ** 2 * c.N * c.D * c.sweeps
    if c.family == "mlg":
        return c.r ** 4 * 600 * (c.burnin + c.maxepoch) * c.n_samples
    if c.family == "gmc":
        return c.n * c.r * c.N * c.D * c.L * c.epochs * 50
    return c.p ** 3


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    cases = sorted(GC.CASES, key=lambda c: -_cost(c))
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out, meas = {}, {}
    for c, (k, dg, packed, e_np, e_64, sec) in zip(cases, results):
        out[k + "_digest"] = np.array(dg)
        for s, a in packed.items():
            out[k + "_" + s] = a
        out[k + "_numpy"], out[k + "_f64"], out[k + "_seconds"] = e_np, e_64, np.array(sec)
        meas[k] = e_np
        print("%-28s %6.1f s  numpy %s   f64 %s" % (GC.case_id(c), sec, " ".join("%.1e" % v for v in e_np),
                                                  " ".join("%.1e" % v for v in e_64)), flush=True)
    for fam in GC.FAMILIES:
        u = np.zeros(len(GC.QUANTITIES[fam]))
        for c in GC.CASES:
            if c.family == fam:
                u = np.fmax(u, meas[GC.key(c)])
        out["u_" + fam] = u
        out["bar_" + fam] = GC.MARGIN * u
        print("%-5s u = %s   B = %s" % (fam, " ".join("%.1e" % v for v in u),
                                       " ".join("%.1e" % v for v in GC.MARGIN * u)))
    np.savez_compressed(GC.GOLDEN, **out)
    print("%s: %d bytes, %.0f s" % (GC.GOLDEN, os.path.getsize(GC.GOLDEN), time.time() - t0))


if __name__ == "__main__":
    main()
