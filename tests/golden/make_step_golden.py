"""Regenerate step_mp.npz: the mpmath (50 digits) references of three SGLD steps of every case of
oracle.step_cases, and the CPU-only measurements that go with them: the high-precision side of
tests/test_gpu_step.py and tests/test_step_cases.py.

    make -C oracle && python tests/golden/make_step_golden.py [processes]

Per case `key` (oracle.step_cases.key): key_digest (SHA-256 of the inputs, the initial state and the
step sizes, all regenerated from shape and seed, not stored); key_w_hi / key_w_lo (steps, Q[, C]),
key_n_hi / key_n_lo (steps, [C,] 1 + D: ‖gradw‖, ‖gradU_k‖) and key_U_hi / key_U_lo (kept steps,
kept entries: oracle.step_cases.u_select), hi float64 + lo float32 = the true value to about 2^-77;
key_expm_norms (‖·‖₁ of every expm argument of the numpy restatement) and key_meas (MEAS below).
Per family: u_family = the largest error of the two fp64 restatements (oracle/gpt_sgld_ref.py, and
the C++ one of oracle/cpu_lib.py for SGLD + Stiefel regression) against mpmath over the family's
cases for (w, U, norms, colnorm: oracle.step_cases.QUANTITIES), and bar_family = MARGIN·u, the
device's bar.  Data only; 165 s on eight cores (the r = 20, D = 12 case is one process for all of
that), 500 s of mpmath in all.
"""
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import step_cases as SC  # noqa: E402

MEAS = ("share_w", "share_U", "cond_w", "cond_U", "cond_norms", "numpy_w", "numpy_U", "numpy_norms",
        "numpy_colnorm", "cpp_w", "cpp_U", "cpp_colnorm", "seconds")
PERTURBATIONS = 3


def as_reference(c, packed):
    out = dict(w=(packed["w_hi"], packed["w_lo"].astype(np.float64)),
               norms=(packed["n_hi"], packed["n_lo"].astype(np.float64)), sel=SC.u_select(c))
    if "U_hi" in packed:
        out["U"] = (packed["U_hi"], packed["U_lo"].astype(np.float64))
    return out


def conditioning(c):
    """The worst move of each stored quantity of the numpy restatement under perturbed inputs."""
    base = SC.run_numpy(c)
    worst = {}
    for s in range(PERTURBATIONS):
        for q, v in SC.rel_err(SC.run_numpy(c, SC.perturbed(c, s)), base).items():
            worst[q] = max(worst.get(q, 0.0), v)
    return worst


def _one(c):
    t0 = time.time()
    packed = SC.pack(c, SC.compute(c))
    sec = time.time() - t0
    ref = as_reference(c, packed)
    p = SC.inputs(c)
    m = dict.fromkeys(MEAS, float("nan"))
    m.update(share_w=p["share_w"], share_U=p["share_U"], seconds=sec)
    run = SC.run_numpy(c)
    assert run["status"] == 0, SC.case_id(c)
    for q, v in SC.rel_err(run, ref, SC.on_manifold(c)).items():
        m["numpy_" + q] = v
    for q, v in conditioning(c).items():
        m["cond_" + q] = v
    if c.family == SC.REG:
        e = SC.rel_err(SC.run_cpp(c), ref, True)
        m.update(cpp_w=e["w"], cpp_U=e["U"], cpp_colnorm=e["colnorm"])
    return SC.key(c), SC.digest(c), packed, SC.expm_norms(c), np.array([m[k] for k in MEAS])


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    cases = sorted(SC.CASES, key=lambda c: -c.shape[0] * c.shape[1] * c.shape[2] ** 2)
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out = {}
    u = {fam: np.zeros(len(SC.QUANTITIES)) for fam in SC.FAMILIES}
    for c, (k, dg, packed, norms, meas) in zip(cases, results):
        out[k + "_digest"] = np.array(dg)
        for s, a in packed.items():
            out[k + "_" + s] = a
        out[k + "_expm_norms"] = norms
        out[k + "_meas"] = meas
        m = dict(zip(MEAS, meas))
        for i, q in enumerate(SC.QUANTITIES):
            u[c.family][i] = np.nanmax([u[c.family][i], m["numpy_" + q], m.get("cpp_" + q, np.nan)])
        print("%-44s %6.1f s  expm norm <= %-8.3g shares %.2f %.2f  cond %.1e  numpy %.1e %.1e %.1e %.1e"
              "  C++ %.1e %.1e %.1e" % (SC.case_id(c), m["seconds"], norms.max() if len(norms) else 0.0,
                                   m["share_w"], m["share_U"],
                                   np.nanmax([m["cond_w"], m["cond_U"], m["cond_norms"]]),
                                   m["numpy_w"], m["numpy_U"], m["numpy_norms"], m["numpy_colnorm"], m["cpp_w"],
                                   m["cpp_U"], m["cpp_colnorm"]),
              flush=True)
    for fam in SC.FAMILIES:
        out["u_" + fam] = u[fam]
        out["bar_" + fam] = SC.MARGIN * u[fam]
        print("%-18s u = %s   B = %s" % (fam, " ".join("%.2e" % v for v in u[fam]),
                                        " ".join("%.2e" % v for v in SC.MARGIN * u[fam])))
    np.savez_compressed(SC.GOLDEN, **out)
    print("%s: %d bytes, %.0f s" % (SC.GOLDEN, os.path.getsize(SC.GOLDEN), time.time() - t0))


if __name__ == "__main__":
    main()
