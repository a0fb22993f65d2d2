"""Regenerate cls_step_mp.npz: the mpmath (50 digits) references of every case of
tests/cls_step_cases.py (the full-theta softmax sampler GPNT_SGLDclass, every stored step) and the
CPU-only measurement that goes with them: the high-precision side of tests/test_gpu_cls_step.py and
tests/test_cls_step_cases.py.

    python tests/golden/make_cls_step_golden.py [processes]

Per case `name`: name_digest (SHA-256 of the case and its inputs, which are regenerated from shape
and seed, not stored); name_hi (stored steps, kept entries) float64 + name_lo float32 = the true value
to about 2^-77; name_scale, max|theta| of each whole stored step; name_u, the error of the numpy
restatement cls_ref.gpnt_sgld_class against the reference in cls_step_cases.error's measure (the
device's bar is MARGIN·u); name_seconds.  Data only; nothing comes from the device.

About 8 s on eight processes, 20 s on one (two_launches' 4097 steps take 6 s, theta_fills_lds'
80 000 normals in mpmath 4 s).
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import cls_step_cases as T  # noqa: E402


def _one(c):
    t0 = time.time()
    packed = T.pack(c, T.compute(c))
    sec = time.time() - t0
    ref = dict(hi=packed["hi"], lo=packed["lo"].astype(np.float64), scale=packed["scale"],
               sel=T.select(c.n, c.n * c.C))
    return c.name, T.digest(c), packed, T.error(T.run_numpy(c), ref), sec


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    cases = sorted(T.CASES, key=lambda c: -(c.n * c.C * T.total(c) * (c.m + 8)))
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out = {}
    for name, dg, packed, u, sec in results:
        out[name + "_digest"] = np.array(dg)
        for s, a in packed.items():
            out[name + "_" + s] = a
        out[name + "_u"], out[name + "_seconds"] = np.array(u), np.array(sec)
    for c in T.CASES:
        print("%-30s %6.1f s  steps %4d kept %2d  u = %.2e  B = %.2e" % (
            c.name, out[c.name + "_seconds"], T.total(c), T.kept(c), out[c.name + "_u"],
            T.MARGIN * out[c.name + "_u"]), flush=True)
    np.savez_compressed(T.GOLDEN, **out)
    print("%s: %d bytes, %.0f s" % (T.GOLDEN, os.path.getsize(T.GOLDEN), time.time() - t0))


if __name__ == "__main__":
    main()
