"""Time exact GP regression on the device (gpt_amd/csrc/exactgp.hip) against two yardsticks that
are not the code under test.

    python scripts/time_exactgp.py [--runs 11] [--threads 16] [--out profiles/exactgp_bench.json]

Shapes: PowerPlant N = 1000, 5000, 9568 at D = 4 (tests/exactgp_ref.py's EXACT: the ARD
hyper-parameters of DataRecords.txt:384 with l_2 = 0.5; the rows past N, or the first 1000 rows at N = 9568, are the test set) and kin40k N = 10000 at D = 8
with its 30000 test rows.  Per shape: the host time of a value-only evaluation, of a value +
gradient evaluation and of a prediction at the fitted point on a resident handle (a host clock
around the call, which ends in a stream synchronise and the copy of the results), each the median
of --runs runs after two warm-up runs, and the device-event time of each phase from
gpt_egp_eval_timed.  The Cholesky's rate is N^3/3 flops over its phase time, set against the fp64
matrix peak.  Yardsticks: (a) the scipy fp64 restatement (Cholesky + solves; the triangular solve
of the test block) on --threads BLAS threads, one run; (b) torch.linalg.cholesky and
torch.cholesky_solve of the same matrix on the same device, median of --runs: what the vendor
factorisation does.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ["build", "cholesky", "solves", "inverse", "P", "grad_pass"]
FP64_MATRIX_PEAK = 78.6e12          # MI355X fp64 matrix flop/s


def shapes():
    return [("powerplant", 1000), ("powerplant", 5000), ("powerplant", 9568), ("kin40k", 10000)]


def inputs(name, N):
    import numpy as np
    import exactgp_ref as ER
    gold = os.path.join(ROOT, "tests", "golden")
    if name == "powerplant":
        pp = np.load(os.path.join(gold, "powerplant.npz"))["data"]
        tr = pp[:N]
        te = pp[N:] if N < pp.shape[0] else pp[:1000]
        h = np.array(ER.EXACT)
        Xa, ya, Xb, yb = tr[:, :4], tr[:, 4], te[:, :4], te[:, 4]
    else:
        z = np.load(os.path.join(gold, "kin40k.npz"))
        Xa, ya, Xb, yb = z["Xtrain"][:N], z["ytrain"][:N], z["Xtest"], z["ytest"]
        h = np.array([1.5] * 8 + [1.0, 0.05])
    mu, sd = Xa.mean(axis=0), Xa.std(axis=0, ddof=1)
    ym, ys = ya.mean(), ya.std(ddof=1)
    return (Xa - mu) / sd, (ya - ym) / ys, (Xb - mu) / sd, (yb - ym) / ys, h


def kernel(Xa, Xb, h):
    import numpy as np
    from scipy.spatial.distance import cdist
    ls = h[:-2]
    return h[-2] ** 2 * np.exp(-0.5 * cdist(Xa / ls, Xb / ls, "sqeuclidean"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exactgp_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)
    import numpy as np
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import C, P_D, check, lib
    assert lib().gpt_device_count() > 0, "time_exactgp.py needs a GPU"

    def med(fun, runs):
        ts = []
        for it in range(runs + 2):
            t0 = time.perf_counter()
            fun()
            if it >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}

    rows = []
    for name, N in shapes():
        X, y, Xt, yt, h = inputs(name, N)
        gp = G.ExactGP(X, y)
        hp = np.ascontiguousarray(h)
        row = {"shape": name, "N": N, "D": X.shape[1], "Ntest": Xt.shape[0], "hyper": h.tolist()}
        val = C.c_double()
        grad = np.empty(h.size)
        ph = np.empty(len(PHASES))
        for want_grad, key in ((0, "value"), (1, "value_grad")):
            row[key] = med(lambda: check(lib().gpt_egp_eval(
                gp._h, hp.ctypes.data_as(P_D), h.size, want_grad, C.byref(val),
                grad.ctypes.data_as(P_D), None)), a.runs)
            phases = []
            for _ in range(a.runs):
                check(lib().gpt_egp_eval_timed(gp._h, hp.ctypes.data_as(P_D), h.size, want_grad,
                                               C.byref(val), grad.ctypes.data_as(P_D),
                                               ph.ctypes.data_as(P_D)))
                phases.append(ph.copy())
            m = np.median(np.stack(phases), axis=0)
            row[key]["device_ms"] = float(m.sum())
            row[key]["phase_ms"] = dict(zip(PHASES, m.tolist()))
        row["nlml"] = val.value
        chol = row["value_grad"]["phase_ms"]["cholesky"] * 1e-3
        row["cholesky_gflops"] = N ** 3 / 3.0 / chol / 1e9
        row["cholesky_share_of_fp64_matrix_peak"] = N ** 3 / 3.0 / chol / FP64_MATRIX_PEAK
        gp.nlogmarginal(h)                       # the prediction reuses this factor
        row["predict"] = med(lambda: gp.predict(h, Xt, yt), max(3, a.runs // 3))
        pr = gp.predict(h, Xt, yt)
        row["test_rmse_whitened"] = float(np.sqrt(np.mean((yt - pr.fmu) ** 2)))
        row["fit_predict_ms"] = row["value"]["ms"] + row["predict"]["ms"]
        gp.close()
        if not a.no_torch:
            import torch
            K = kernel(X, X, h)
            K[np.diag_indices_from(K)] += h[-1]
            Kd = torch.from_numpy(K).cuda()
            yd = torch.from_numpy(y).cuda()[:, None]
            Ksd = torch.from_numpy(kernel(X, Xt, h)).cuda()

            def sync(fun):
                fun()
                torch.cuda.synchronize()
            row["torch_cholesky"] = med(lambda: sync(lambda: torch.linalg.cholesky(Kd)), a.runs)
            Ld = torch.linalg.cholesky(Kd)
            row["torch_cholesky_solve_y"] = med(lambda: sync(lambda: torch.cholesky_solve(yd, Ld)),
                                                a.runs)
            try:
                row["torch_triangular_solve_Ks"] = med(lambda: sync(
                    lambda: torch.linalg.solve_triangular(Ld, Ksd, upper=False)), max(3, a.runs // 3))
            except RuntimeError as e:            # the vendor trsm's workspace allocation can fail
                row["torch_triangular_solve_Ks"] = {"error": str(e).splitlines()[0]}
            row["torch_cholesky_gflops"] = N ** 3 / 3.0 / (row["torch_cholesky"]["ms"] * 1e-3) / 1e9
            al = torch.cholesky_solve(yd, Ld)[:, 0].cpu().numpy()
            row["torch_alpha_vs_device"] = float(np.abs(al - G.ExactGP(X, y).alpha(h)).max()
                                                 / np.abs(al).max())
            del Kd, Ksd, Ld
            torch.cuda.empty_cache()
        if not a.no_cpu:
            from scipy.linalg import cho_solve, cholesky, solve_triangular
            t0 = time.perf_counter()
            K = kernel(X, X, h)
            K[np.diag_indices_from(K)] += h[-1]
            L = cholesky(K, lower=True, overwrite_a=True, check_finite=False)
            al = cho_solve((L, True), y, check_finite=False)
            t1 = time.perf_counter()
            Ks = kernel(X, Xt, h)
            fmu = Ks.T @ al
            V = solve_triangular(L, Ks, lower=True, overwrite_b=True, check_finite=False)
            fs2 = h[-2] ** 2 - np.einsum("ij,ij->j", V, V)
            t2 = time.perf_counter()
            row["scipy_threads"] = a.threads
            row["scipy_value_ms"] = (t1 - t0) * 1e3
            row["scipy_predict_ms"] = (t2 - t1) * 1e3
            row["scipy_fmu_vs_device"] = float(np.abs(fmu - pr.fmu).max() / np.abs(fmu).max())
            row["scipy_fs2_vs_device"] = float(np.abs(np.maximum(fs2, 0) - pr.fs2).max() / h[-2] ** 2)
            row["speedup_value"] = row["scipy_value_ms"] / row["value"]["ms"]
            row["speedup_predict"] = row["scipy_predict_ms"] / row["predict"]["ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": a.runs, "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "rows": rows}, f,
                  indent=1)


if __name__ == "__main__":
    main()
