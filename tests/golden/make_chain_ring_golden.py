"""tests/golden/chain_ring_parent.npz: what tests/test_gpu_chain_ring.py's cases store over seven
chain-engine steps of two chains (the w of every step, the U of the last step, the SHA-256 of every
(chain, step) U block), recorded on the device from the library of the commit BEFORE the batch
loop's row staging became a two-buffer ring (GPTSGLD_LIB names that build):

    GPTSGLD_LIB=/path/to/parent/libgptsgld.so python tests/golden/make_chain_ring_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_chain_ring as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    for shape in T.SHAPES:
        o = T.whole(shape)
        print(shape, "status", o["status"], "done", o["done"], flush=True)
        assert o["status"] == [0, 0] and o["done"] == T.STEPS
        assert np.isfinite(o["w"]).all() and np.isfinite(o["U"]).all()
        k = T.key(shape)
        out["w_" + k], out["Ulast_" + k], out["Usha_" + k] = o["w"], o["U"][..., -1], T.digests(o["U"])
    dst = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    np.savez(dst, **out)
    print("wrote %s (%d bytes): %s" % (dst, os.path.getsize(dst), {k: v.shape for k, v in out.items()}))
