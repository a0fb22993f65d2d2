"""tests/golden/chain_glue_parent.npz: the final (w, U, status) of tests/test_gpu_chain_glue.py's
parent cases (seven chain-engine steps, two chains, the WV = 8 and the WV = 4 build), recorded on
the device from the library of the commit BEFORE the step bookkeeping changed (GPTSGLD_LIB names
that build):

    GPTSGLD_LIB=/path/to/parent/libgptsgld.so python tests/golden/make_chain_glue_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_chain_glue as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    for shape in T.PARENT_SHAPES:
        w, U, status = T.parent_run(shape)
        assert not status.any() and np.isfinite(w).all() and np.isfinite(U).all()
        key = "_".join(map(str, shape))
        out["w_" + key], out["U_" + key], out["status_" + key] = w, U, status
    dst = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    np.savez(dst, **out)
    print("wrote %s: %s" % (dst, {k: v.shape for k, v in out.items()}))
