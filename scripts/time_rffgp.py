"""Time the RFF GP's closed-form predictive and the kernel approximation error on the device
(gpt_amd/csrc/nlml.hip) against numpy restatements that are not the code under test.

    python scripts/time_rffgp.py [--runs 7] [--threads 16] [--out profiles/rffgp_bench.json]

predict: PowerPlant's 5000 / 4568 split at n = 100 and 800 and kin40k's 10000 / 30000 at n = 1024,
at the hyper-parameters GPNT_hyperparameters finds on the device from the experiment's start.  Per
shape: the device-event time of the call's chunks (gpt_rff_last_timing) and the host time of the
call on a resident handle that holds the factor, medians of --runs runs after two warm-up runs;
the Cholesky-form numpy restatement of the same prediction (the factor given) on --threads BLAS
threads; test RMSE (x ytrainStd) and mean lp, beside ExactGP's on the PowerPlant split.

rff_kernel_error: PowerPlantDataExperiment.jl:83-97's loop on all 9568 whitened rows, n in
{100, ..., 3200} x three (Z, b) seeds at the script's hyper-parameters and again with l_2 = 0.5:
frob, frob / norm_K, the tile pass's device time and its rate on the MFMA flops (N^2 n for the
lower tiles computed in full); the literal numpy form at n = 800.  `headline_ab` in the output
(bench.py's figure, alternating with the parent commit's library) is kept from the existing file.
Needs the GPU; no fallback.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCRIPT_LS = [1.3978, 0.0028, 2.8966, 7.5565]     # PowerPlantDataExperiment.jl:83
SIGMA_RBF2 = 0.8333
NS = [100, 200, 400, 800, 1600, 3200]
CHOL_TRAILING_TFLOPS = 11.1                      # DESIGN §6d, the exact GP's trailing update


def whiten_pair(Xa, ya, Xb, yb):
    mu, sd = Xa.mean(axis=0), Xa.std(axis=0, ddof=1)
    ym, ys = ya.mean(), ya.std(ddof=1)
    return (Xa - mu) / sd, (ya - ym) / ys, (Xb - mu) / sd, (yb - ym) / ys, float(ys)


def predict_inputs(name):
    import numpy as np
    import nlml_ref as NR
    gold = os.path.join(ROOT, "tests", "golden")
    if name == "powerplant":
        pp = np.load(os.path.join(gold, "powerplant.npz"))["data"]
        tr, te = pp[:5000], pp[5000:]
        return whiten_pair(tr[:, :4], tr[:, 4], te[:, :4], te[:, 4]) + (np.array(NR.EXPERIMENT),)
    z = np.load(os.path.join(gold, "kin40k.npz"))
    return whiten_pair(z["Xtrain"][:10000], z["ytrain"][:10000], z["Xtest"], z["ytest"]) + (
        np.array([1.5] * 8 + [1.0, 0.05]),)


def med(ts):
    import numpy as np
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rffgp_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)
    import numpy as np
    import exactgp_ref as ER
    import nlml_ref as NR
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import lib
    assert lib().gpt_device_count() > 0, "time_rffgp.py needs a GPU"
    out = {"runs": a.runs, "threads": a.threads, "predict": [], "kernel_error": {}}

    # ------------------------------------------------------------------ predict
    for name, n in (("powerplant", 100), ("powerplant", 800), ("kin40k", 1024)):
        X, y, Xt, yt, ystd, start = predict_inputs(name)
        D = X.shape[1]
        rng = np.random.default_rng(n)
        Z, b = rng.standard_normal((n, D)), 2 * math.pi * rng.random(n)
        m = G.NoTensorMarginal(X, y, Z, b)
        t0 = time.perf_counter()
        h, nlml = G.GPNT_hyperparameters(m.nlogmarginal, m.gradnlogmarginal, start, 0.001)
        row = {"shape": name, "n": n, "N": X.shape[0], "Ntest": Xt.shape[0], "D": D,
               "hyper": h.tolist(), "nlml": nlml, "optimiser_s": time.perf_counter() - t0}
        m.nlogmarginal(h)                         # the factor the predictions reuse
        dev, host = [], []
        for it in range(a.runs + 2):
            t0 = time.perf_counter()
            pr = m.predict(h, Xt, yt)
            if it >= 2:
                host.append((time.perf_counter() - t0) * 1e3)
                dev.append(float(G.rff_last_timing()[2]))
        row["predict_device_ms"], row["predict_host_ms"] = med(dev), med(host)
        row["test_rmse"] = float(ystd * np.sqrt(np.mean((yt - pr.ymu) ** 2)))
        row["mean_lp"] = float(pr.lp.mean())
        row["min_fs2"] = float(pr.fs2.min())
        if not a.no_cpu:
            from scipy.linalg import solve_triangular
            ls, sigma, s2 = NR.split(h, D)
            phi = NR.feature_notensor(X, ls, sigma, Z, b)
            L = np.linalg.cholesky(phi @ phi.T + s2 * np.eye(n))
            l = m.theta_mean(h)
            t0 = time.perf_counter()
            ps = NR.feature_notensor(Xt, ls, sigma, Z, b)
            fmu = ps.T @ l
            V = solve_triangular(L, ps, lower=True, check_finite=False)
            fs2 = s2 * np.einsum("ij,ij->j", V, V)
            row["numpy_predict_ms"] = (time.perf_counter() - t0) * 1e3
            row["numpy_fmu_vs_device"] = float(np.abs(fmu - pr.fmu).max() / np.abs(fmu).max())
            row["numpy_fs2_vs_device"] = float(np.abs(fs2 - pr.fs2).max() / sigma ** 2)
            row["speedup_vs_numpy_device_time"] = row["numpy_predict_ms"] / row["predict_device_ms"]["median"]
            row["speedup_vs_numpy_host_time"] = row["numpy_predict_ms"] / row["predict_host_ms"]["median"]
        m.close()
        if name == "powerplant":
            gp = G.ExactGP(X, y)
            ep = gp.predict(np.array(ER.EXACT), Xt, yt)
            row["exactgp_test_rmse"] = float(ystd * np.sqrt(np.mean((yt - ep.ymu) ** 2)))
            row["exactgp_mean_lp"] = float(ep.lp.mean())
            gp.close()
        print(json.dumps(row), flush=True)
        out["predict"].append(row)

    # ------------------------------------------------------------------ kernel error
    pp = np.load(os.path.join(ROOT, "tests", "golden", "powerplant.npz"))["data"]
    X = NR.whiten(pp[:, :4])
    N = X.shape[0]
    for tag, l2 in (("script_hyper", SCRIPT_LS[1]), ("l2_0p5", 0.5)):
        h = np.array([SCRIPT_LS[0], l2, SCRIPT_LS[2], SCRIPT_LS[3], math.sqrt(SIGMA_RBF2), 0.0195])
        rows = []
        for n in NS:
            for seed in (1, 2, 3):
                rng = np.random.default_rng(1000 * seed + n)
                Z, b = rng.standard_normal((n, 4)), 2 * math.pi * rng.random(n)
                G.rff_kernel_error(X, Z, b, h)                    # warm-up
                ms, wall = [], []
                for _ in range(3):
                    t0 = time.perf_counter()
                    e = G.rff_kernel_error(X, Z, b, h)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(G.rff_last_timing()[:2].copy())
                feat, tile = np.median(np.stack(ms), axis=0)
                rows.append({"n": n, "seed": seed, "frob": e.frob, "norm_K": e.norm_K,
                             "frob_over_norm_K": e.frob / e.norm_K, "max_abs": e.max_abs,
                             "features_ms": float(feat), "tiles_ms": float(tile),
                             "call_ms": float(np.median(wall)),
                             "mfma_tflops": N * (N + 64.0) * n / (tile * 1e-3) / 1e12})
                print(json.dumps(rows[-1]), flush=True)
        out["kernel_error"][tag] = {"hyper": h.tolist(), "N": N, "rows": rows}
    out["kernel_error"]["cholesky_trailing_update_tflops"] = CHOL_TRAILING_TFLOPS
    if not a.no_cpu:
        import rffgp_ref as RR
        n = 800
        rng = np.random.default_rng(1000 + n)
        Z, b = rng.standard_normal((n, 4)), 2 * math.pi * rng.random(n)
        h = np.array(out["kernel_error"]["l2_0p5"]["hyper"])
        t0 = time.perf_counter()
        ref = RR.kernel_error_literal(X, Z, b, h)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        dev = next(r for r in out["kernel_error"]["l2_0p5"]["rows"] if r["n"] == n and r["seed"] == 1)
        out["kernel_error"]["numpy_literal_n800"] = {
            "ms": cpu_ms, "frob": ref.frob, "device_call_ms": dev["call_ms"],
            "frob_vs_device_rel": abs(ref.frob - dev["frob"]) / ref.frob,
            "speedup_call": cpu_ms / dev["call_ms"]}
        print(json.dumps(out["kernel_error"]["numpy_literal_n800"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if os.path.exists(a.out):                    # the headline A/B record is entered by hand
        old = json.load(open(a.out))
        if "headline_ab" in old:
            out["headline_ab"] = old["headline_ab"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
