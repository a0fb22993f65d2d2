"""Regenerate tests/golden/segment.npz from the reference's data file segment.dat (the image
segmentation data of ImageExperiment.jl / ImageNoTensorExperiment.jl):

    python tests/golden/make_segment_golden.py /path/to/reference

Output (data only): ``data``, one float64 array of 2310 rows x 20 columns exactly as the file
holds them: 19 attributes and the class label 1..7 in the last column.  The column selection
[1, 2, 6:20] and the 1300 / 1010 split of ImageNoTensorExperiment.jl:9-26 are applied by the
tests (tests/cls_ref.py segment_problem), not here.
"""
import os
import sys

import numpy as np


def main(ref):
    out = os.path.dirname(os.path.abspath(__file__))
    data = np.loadtxt(os.path.join(ref, "segment.dat"), dtype=np.float64)
    assert data.shape == (2310, 20), data.shape
    np.savez_compressed(os.path.join(out, "segment.npz"), data=data)
    print("segment.npz: %s, labels %s" % (data.shape, sorted(set(data[:, -1].astype(int)))))


if __name__ == "__main__":
    main(sys.argv[1])
