"""Regenerate expm_mp_nnXX.npz: mpmath.expm (60 digits) of every matrix of oracle.expm_cases.cases(nn),
the high-precision reference of tests/test_gpu_expm.py.

    python tests/golden/make_expm_golden.py [nn ...]

Per file: digest (SHA-256 of the float64 input matrix), hi (float64) and lo (float32) with
hi + lo = exp(X) to about 1e-23 relative.  Data only; a few minutes for all sizes (mpmath takes
seconds per matrix from nn = 30 up, which is why the results are committed).
tests/test_oracle.py recomputes a sample of them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import expm_cases as XC  # noqa: E402


def main(sizes):
    for nn in sizes:
        cs = XC.cases(nn)
        refs = [XC.expm_mp(X) for _, _, X in cs]
        np.savez_compressed(XC.golden_path(nn),
                            digest=np.array([XC.digest(X) for _, _, X in cs]),
                            hi=np.stack([h for h, _ in refs]),
                            lo=np.stack([l for _, l in refs]).astype(np.float32))
        print("nn = %d: %d matrices" % (nn, len(cs)), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or XC.ALL_SIZES)
