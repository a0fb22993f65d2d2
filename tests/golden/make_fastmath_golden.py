"""Regenerate fastmath_mp.npz: the mpmath (50 digits) references of oracle.fastmath_cases, the
high-precision side of tests/test_gpu_fastmath.py and tests/test_fastmath_cases.py.

    python tests/golden/make_fastmath_golden.py

Per reference set `key` (oracle.fastmath_cases.KEYS): key_digest (SHA-256 of the input set),
key_hi (float64) and key_lo (float32) with hi + lo = the true value to about 2^-77 relative.  Data
only; about a minute.  tests/test_fastmath_cases.py recomputes them where mpmath is importable.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import fastmath_cases as FC  # noqa: E402


def main():
    out = {}
    for key in FC.KEYS:
        hi, lo = FC._compute(key)
        out[key + "_digest"] = np.array(FC.digest(key))
        out[key + "_hi"] = hi
        out[key + "_lo"] = lo.astype(np.float32)
        print("%s: %d values" % (key, hi.size), flush=True)
    np.savez_compressed(FC.GOLDEN, **out)
    print("%s: %d bytes" % (FC.GOLDEN, os.path.getsize(FC.GOLDEN)))


if __name__ == "__main__":
    main()
