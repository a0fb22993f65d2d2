"""Time the device joint likelihood of the softmax classifier (gpt_amd/csrc/cjoint.hip) against the
fp64 numpy restatements of ImageExperiment.jl:135-204.

    python scripts/time_cjoint.py [--runs 11] [--reps 20] [--threads 16]
                                  [--out profiles/cjoint_bench.json]

Shapes: the segment shape (n = 150, N = 1300, D = 16, C = 7, the data of tests/golden/segment.npz)
and an MNIST-like n = 1000, N = 60000, D = 16, C = 10 of seeded normals.  Per shape, on a resident
handle after two warm-up calls: the device-event time per evaluation of the value, of the value
with the theta gradient (a Langevin step's evaluation), of the full gradient and of the tiles'
phi and S alone (gpt_cjoint_time: --reps back-to-back evaluations between two events, median of
--runs), the host time of one value / value + gradient call (a host clock around a call that ends
in a synchronise and the copy of the results) and of one Langevin step.  `sincos_share` is the
features-alone time over the full-gradient time.  Beside them the fused numpy restatement on
--threads BLAS threads (median of three; one run at the large shape) and, at the segment shape
only, the literal restatement with its n x N x 17 array (at the large shape that array is 7.7 GB,
which is the point).  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = [("value", 0), ("value_grad_theta", 1), ("value_grad", 2), ("features_only", 4)]


def inputs(name):
    import numpy as np
    import cls_ref as CLS
    from gpt_amd import GPT_SGLD as G
    rng = np.random.default_rng(21)
    if name == "segment":
        X, y, _, _ = CLS.segment_problem()
        n, C = 150, 7
        Z, b = G.feature_inputs(n, 16, CLS.SEG["feature_seed"])
        b = b[:, 0]
        h = np.array(CLS.SEG_LS + [CLS.SEG_SIGMA_RBF])
        y = y.astype(np.float64)
    else:
        N, D, n, C = 60000, 16, 1000, 10
        X = rng.standard_normal((N, D))
        y = rng.integers(1, C + 1, N).astype(np.float64)
        Z, b = rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
        h = np.array([4.0] * D + [2.0])
    theta = rng.standard_normal((n, C))
    return X, y, Z, b, theta, h, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cjoint_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)
    import numpy as np
    import cjoint_ref as CR
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import C as CT, P_D, check, lib
    assert lib().gpt_device_count() > 0, "time_cjoint.py needs a GPU"
    rows = []
    for name in ("segment", "mnist_like"):
        X, y, Z, b, theta, h, ncls = inputs(name)
        N, D = X.shape
        n = Z.shape[0]
        j = G.SoftmaxJoint(X, y, Z, b, C=ncls)
        j.set_theta(theta)
        hp = np.ascontiguousarray(h)
        row = {"shape": name, "N": N, "D": D, "n": n, "C": ncls, "hyper": h.tolist(),
               "reps_per_event_window": a.reps}
        ms = CT.c_double()
        dev = {}
        for key, mode in MODES:
            ts = []
            for it in range(a.runs + 2):
                check(lib().gpt_cjoint_time(j._h, hp.ctypes.data_as(P_D), h.size, mode, a.reps,
                                            CT.byref(ms)))
                if it >= 2:
                    ts.append(ms.value)
            dev[key] = {"device_ms": float(np.median(ts)), "device_ms_min": float(np.min(ts)),
                        "device_ms_max": float(np.max(ts))}
        row["device"] = dev
        row["sincos_share"] = dev["features_only"]["device_ms"] / dev["value_grad"]["device_ms"]
        host = {}
        for key, fun in (("value", lambda: j.neglogjointlkhd(None, h)),
                         ("value_grad", lambda: j.value_and_grad(None, h)),
                         ("langevin_step", lambda: j.langevin(h, 1e-6, 1, 3))):
            ts = []
            for it in range(a.runs + 2):
                t0 = time.perf_counter()
                fun()
                if it >= 2:
                    ts.append((time.perf_counter() - t0) * 1e3)
            host[key + "_ms"] = float(np.median(ts))
        row["host"] = host
        j.set_theta(theta)
        val, grad = j.value_and_grad(None, h)
        row["value"] = val
        j.close()
        if not a.no_cpu:
            def med(fun, k):
                ts = []
                for _ in range(k):
                    t0 = time.perf_counter()
                    out = fun()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return float(np.median(ts)), out
            k = 3 if name == "segment" else 1
            row["numpy_threads"] = a.threads
            row["numpy_fused_value_grad_ms"], (rv, rt, rh) = med(
                lambda: CR.value_and_grad_fused(X, y, Z, b, theta, h), k)
            row["speedup_value_grad_vs_fused_numpy"] = (row["numpy_fused_value_grad_ms"]
                                                        / host["value_grad_ms"])
            row["rel_diff_vs_fused_numpy"] = {
                "value": abs(val - rv) / abs(rv),
                "grad_theta": CR.theta_error(grad[:n * ncls].reshape((n, ncls), order="F"), rt),
                "grad_hyper_max": float((np.abs(grad[n * ncls:] - rh) / np.abs(rh).max()).max())}
            if name == "segment":
                row["numpy_literal_value_ms"], _ = med(
                    lambda: CR.neglogjoint_literal(X, y, Z, b, theta, h), 3)
                row["numpy_literal_grad_ms"], _ = med(
                    lambda: CR.gradneglogjoint_literal(X, y, Z, b, theta, h), 1)
                row["literal_gradfeature_bytes"] = 8 * n * N * (D + 1)
                row["speedup_value_grad_vs_literal_numpy"] = (
                    (row["numpy_literal_value_ms"] + row["numpy_literal_grad_ms"])
                    / host["value_grad_ms"])
            else:
                row["literal_gradfeature_bytes"] = 8 * n * N * (D + 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": a.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
