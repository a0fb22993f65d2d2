"""Regenerate cf_step_mp.npz: the mpmath (50 digits) references of the stored epochs of every case of
oracle.cf_cases, and the CPU-only measurements that go with them: the high-precision side of
tests/test_gpu_cf_step.py and tests/test_cf_cases.py.

    python tests/golden/make_cf_golden.py [processes]

Per reference `key` (oracle.cf_cases.key; cases that differ in the launch path only share one):
key_digest (SHA-256 of the inputs, the initial state and the step sizes, all regenerated from shape
and seed, not stored); key_w_hi / key_w_lo (epochs, r, r; not for the fixed-w entries), key_U_*
(epochs, n1 + D1, r), key_V_*, key_testpred_* (epochs, Ntest), key_rmse_* (epochs, 2: train, test),
hi float64 + lo float32 = the true value to about 2^-77; key_expm_norms (‖·‖₁ of every expm argument
of the numpy restatement, Stiefel cases) and key_meas (MEAS below).  Per family: u_family = the
largest error of the fp64 numpy restatement (oracle/movielens_ref.py from the injected U0 / V0)
against mpmath over the family's cases for oracle.cf_cases.QUANTITIES, and bar_family = MARGIN·u,
the device's bar.  Data only.
"""
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import cf_cases as CC  # noqa: E402

Q6 = CC.QUANTITIES[:-1]
MEAS = (("share_w", "share_U", "decay", "sigma_u", "pred_rms") + tuple("cond_" + q for q in Q6)
        + tuple("numpy_" + q for q in CC.QUANTITIES) + tuple("f64_" + q for q in CC.QUANTITIES)
        + ("seconds",))
PERTURBATIONS = 3


def conditioning(c):
    """The worst move of each stored quantity of the numpy restatement under perturbed inputs."""
    base = CC.run_numpy(c)
    worst = {}
    for s in range(PERTURBATIONS):
        for q, v in CC.rel_err(CC.run_numpy(c, CC.perturbed(c, s)), base).items():
            worst[q] = max(worst.get(q, 0.0), v)
    return worst


def _one(c):
    t0 = time.time()
    packed = CC.pack(c, CC.compute(c))
    sec = time.time() - t0
    ref = {q: (packed[q + "_hi"], packed[q + "_lo"].astype(np.float64)) for q in CC.STORED
           if q + "_hi" in packed}
    p = CC.inputs(c)
    m = dict.fromkeys(MEAS, float("nan"))
    m.update({k: p[k] for k in ("share_w", "share_U", "decay", "sigma_u", "pred_rms")}, seconds=sec)
    for q, v in CC.rel_err(CC.run_numpy(c), ref, CC.on_manifold(c)).items():
        m["numpy_" + q] = v
    for q, v in CC.rel_err(CC.run_f64(c), ref, CC.on_manifold(c)).items():
        m["f64_" + q] = v
    for q, v in conditioning(c).items():
        m["cond_" + q] = v
    norms = CC.expm_norms(c) if c.stiefel else np.zeros(0)
    return CC.key(c), CC.digest(c), packed, norms, np.array([m[k] for k in MEAS])


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    uniq = {}
    for c in CC.CASES:
        uniq.setdefault(CC.key(c), c)
    cases = sorted(uniq.values(), key=lambda c: -(c.r ** 3 * (30 if c.stiefel else 1) + c.m * c.r * c.r))
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            results = pool.map(_one, cases, chunksize=1)
    else:
        results = [_one(c) for c in cases]
    out, meas = {}, {}
    for c, (k, dg, packed, norms, ms) in zip(cases, results):
        out[k + "_digest"] = np.array(dg)
        for s, a in packed.items():
            out[k + "_" + s] = a
        out[k + "_expm_norms"] = norms
        out[k + "_meas"] = ms
        meas[k] = m = dict(zip(MEAS, ms))
        print("%-20s %6.1f s  sigma_u %-8.3g shares %.2f %.2f  expm norm <= %-6.3g cond %.1e  numpy %s"
              "  f64 %.1e" % (c.name, m["seconds"], m["sigma_u"], m["share_w"], m["share_U"],
                              norms.max() if len(norms) else 0.0,
                              np.nanmax([m["cond_" + q] for q in Q6]),
                              " ".join("%.1e" % m["numpy_" + q] for q in CC.QUANTITIES),
                              np.nanmax([m["f64_" + q] for q in CC.QUANTITIES])), flush=True)
    for fam in CC.FAMILIES:
        u = np.zeros(len(CC.QUANTITIES))
        for c in CC.CASES:
            if c.family == fam:
                u = np.fmax(u, [meas[CC.key(c)]["numpy_" + q] for q in CC.QUANTITIES])
        out["u_" + fam] = u
        out["bar_" + fam] = CC.MARGIN * u
        print("%-14s u = %s   B = %s" % (fam, " ".join("%.1e" % v for v in u),
                                        " ".join("%.1e" % v for v in CC.MARGIN * u)))
    np.savez_compressed(CC.GOLDEN, **out)
    print("%s: %d bytes, %.0f s" % (CC.GOLDEN, os.path.getsize(CC.GOLDEN), time.time() - t0))


if __name__ == "__main__":
    main()
