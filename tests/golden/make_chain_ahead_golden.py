"""tests/golden/chain_ahead_control.npz: the stored samples of tests/test_gpu_chain_ahead.py's control
case (the WV = 4 build of the chain engine, seven steps, two chains), recorded on the device from the
library of the commit BEFORE the draw-ahead of the U noise (GPTSGLD_LIB names that build):

    GPTSGLD_LIB=/path/to/parent/libgptsgld.so python tests/golden/make_chain_ahead_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_chain_ahead as T  # noqa: E402

if __name__ == "__main__":
    out = T.run_chunks(T.CONTROL, [T.STEPS])
    assert out["status"] == [0, 0] and out["done"] == T.STEPS
    dst = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    np.savez(dst, w=out["w"], U=out["U"])
    print("wrote %s: w %s, U %s" % (dst, out["w"].shape, out["U"].shape))
