"""Regenerate pred_mp.npz: the mpmath (50 digits) references and derived error bounds of
oracle.pred_cases, the high-precision side of tests/test_gpu_pred.py and tests/test_pred_cases.py.

    python tests/golden/make_pred_golden.py [processes]

Per distinct case shape `key` (oracle.pred_cases.key): key_digest (SHA-256 of the case's inputs,
which are regenerated from the shape and seed, not stored), key_hi (float64) and key_lo (float32)
with hi + lo = the true f to about 2^-77 relative, key_E (float64) the bound, each (S, Ntest).
Data only; a few minutes on one core.  tests/test_pred_cases.py recomputes a subset where mpmath
is importable.
"""
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import pred_cases as PC  # noqa: E402


def _one(c):
    return PC.key(c), PC.digest(c), PC.compute(c)


def main():
    cases = list({PC.key(c): c for c in PC.CASES}.values())
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out = {}
    for k, dg, (hi, lo, E) in results:
        out[k + "_digest"] = np.array(dg)
        out[k + "_hi"] = hi
        out[k + "_lo"] = lo.astype(np.float32)
        out[k + "_E"] = E
        print("%s: %d values, max E / max|f| = %.3g" % (k, hi.size, E.max() / np.abs(hi).max()),
              flush=True)
    np.savez_compressed(PC.GOLDEN, **out)
    print("%s: %d bytes" % (PC.GOLDEN, os.path.getsize(PC.GOLDEN)))


if __name__ == "__main__":
    main()
