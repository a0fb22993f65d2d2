"""Regenerate cjoint_mp.npz: the negative log joint likelihood of the full-theta softmax classifier
and its gradient with respect to theta and [length_scale; sigma_RBF] (ImageExperiment.jl:135-204)
in mpmath at 50 digits, for every case of tests/cjoint_ref.py at three hyper-parameter points.

    python tests/golden/make_cjoint_golden.py [processes]

Every hyper-gradient component must be at least 1e-4 of the largest (so that a relative test means
something): a point that fails has its length scales multiplied by 1.25 until it passes, and the
script says so.  The theta-times-40 case is exempt (a saturated softmax leaves components that
nearly cancel); its errors are measured against the largest component.  Per case the file holds
X, y, Z, b, theta, H (3, Lh), val (3), gtheta (3, n, C) and gh (3, Lh) as float64.  Data only; a
few CPU-minutes on 8 processes.
"""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import cjoint_ref as CR  # noqa: E402


def task(arg):
    idx, p = arg
    case = CR.CASES[idx]
    X, y, Z, b, theta = CR.case_inputs(case, idx)
    h = CR.hyper_points(case)[p]
    nl = h.size - 1
    exempt = case[5] == "x40"
    note = ""
    # the cheap fp64 form picks the point; mp then evaluates it once
    for _ in range(12):
        if exempt or CR.component_rule(CR.value_and_grad_fused(X, y, Z, b, theta, h)[2]):
            break
        h = h.copy()
        h[:nl] *= 1.25
        note = " (point replaced: length scales now %s)" % h[:nl]
    val, gtheta, gh = CR.mp_value_grad(X, y, Z, b, theta, h)
    assert exempt or CR.component_rule(gh), (case, p, gh)
    print("%s point %d: value %.6f%s" % (CR.case_name(case), p, val, note), flush=True)
    return idx, p, h, val, gtheta, gh


def main(procs):
    jobs = [(idx, p) for idx in range(len(CR.CASES)) for p in range(3)]
    jobs.sort(key=lambda a: -CR.CASES[a[0]][0] * CR.CASES[a[0]][1] * (CR.CASES[a[0]][2] + CR.CASES[a[0]][3]))
    with multiprocessing.Pool(procs) as pool:
        res = pool.map(task, jobs, chunksize=1)
    out = {}
    for idx, case in enumerate(CR.CASES):
        nm = CR.case_name(case)
        X, y, Z, b, theta = CR.case_inputs(case, idx)
        mine = sorted((r for r in res if r[0] == idx), key=lambda r: r[1])
        out.update({nm + "_X": X, nm + "_y": y, nm + "_Z": Z, nm + "_b": b, nm + "_theta": theta,
                    nm + "_H": np.stack([r[2] for r in mine]),
                    nm + "_val": np.array([r[3] for r in mine]),
                    nm + "_gtheta": np.stack([r[4] for r in mine]),
                    nm + "_gh": np.stack([r[5] for r in mine])})
    np.savez_compressed(CR.GOLDEN, **out)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
