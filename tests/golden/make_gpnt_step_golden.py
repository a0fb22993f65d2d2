"""Regenerate gpnt_step_mp.npz: the mpmath (50 digits) references of every case of
tests/gpnt_step_cases.py (the full-theta regression sampler GPNT_SGLD, every held step) and the
CPU-only measurements that go with them: the high-precision side of tests/test_gpu_gpnt_step.py and
tests/test_gpnt_step_cases.py.

    python tests/golden/make_gpnt_step_golden.py [processes]

Per case `name`: name_digest (SHA-256 of the case and its inputs, which are regenerated from shape
and seed, not stored); name_hi (held steps, kept entries) float64 + name_lo float32 = the true value
to about 2^-77; name_scale, max|theta| of each whole held step; name_u, the error of the numpy
restatement (oracle.gpt_sgld_ref.GPNT_SGLD thinned as gpnt_ref.gpnt_sgld_chains does) against the
reference in gpnt_step_cases.error's measure (the device's bar is B = MARGIN·u); name_share and
name_share_g, the step-1 shares of the gradient and of its data term (gpnt_step_cases.shares);
name_seconds.  Data only; nothing comes from the device.

Two caps on B are conditions of the cases, not measurements: B <= 1e-14 for a case of at most ten
steps and B <= 1e-13 for every case.  The maker refuses to write a fixture that misses one, or a
case whose share is under SHARE_MIN: then the case's inputs change, never the cap.
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import gpnt_step_cases as T  # noqa: E402


def _one(c):
    t0 = time.time()
    packed = T.pack(c, T.compute(c))
    sec = time.time() - t0
    ref = dict(hi=packed["hi"], lo=packed["lo"].astype(np.float64), scale=packed["scale"],
               sel=T.select(c.n, c.n))
    return c.name, T.digest(c), packed, T.error(T.run_numpy(c), ref), T.shares(c), sec


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    cases = sorted(T.CASES, key=lambda c: -(c.n * T.steps(c) * (c.m + 8)))
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out = {}
    for name, dg, packed, u, (share, share_g), sec in results:
        out[name + "_digest"] = np.array(dg)
        for s, a in packed.items():
            out[name + "_" + s] = a
        out[name + "_u"], out[name + "_seconds"] = np.array(u), np.array(sec)
        out[name + "_share"], out[name + "_share_g"] = np.array(share), np.array(share_g)
    missed = []
    for c in T.CASES:
        u, bar = float(out[c.name + "_u"]), T.MARGIN * float(out[c.name + "_u"])
        print("%-18s %6.1f s  steps %4d held %2d  route %-24s share %.3f (data %.3f)  u = %.2e  B = %.2e" % (
            c.name, out[c.name + "_seconds"], T.steps(c), T.kept(c), tuple(T.route(c)),
            out[c.name + "_share"], out[c.name + "_share_g"], u, bar), flush=True)
        if not bar <= (T.CAP_SHORT if T.steps(c) <= T.SHORT_STEPS else T.CAP):
            missed.append(c.name + ": B over its cap")
        if not min(out[c.name + "_share"], out[c.name + "_share_g"]) >= T.SHARE_MIN:
            missed.append(c.name + ": share under SHARE_MIN")
    if missed:
        sys.exit("not written: " + "; ".join(missed))
    np.savez_compressed(T.GOLDEN, **out)
    print("%s: %d bytes, %.0f s" % (T.GOLDEN, os.path.getsize(T.GOLDEN), time.time() - t0))


if __name__ == "__main__":
    main()
