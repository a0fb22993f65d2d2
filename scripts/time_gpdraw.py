"""Time the function draws on the device (gpt_amd/csrc/gpdraw.hip and the draw entries of
exactgp.hip / nlml.hip) against two yardsticks that are not the code under test.

    python scripts/time_gpdraw.py [--runs 5] [--threads 16] [--out profiles/gpdraw_bench.json]

Shapes: draw_prior at N = 2500 (the reference's 50 x 50 mesh), 10000 (MakeSynthData's size) and
16384, D = 2, S = 1 and 256; draw_posterior on PowerPlant's first 5000 rows at Ntest = 1024 and
4568 (the remaining rows), S = 256; draw_theta at n = 800 on the same rows, S = 256.  Per shape:
the host time of the call on a resident handle (a host clock around it; it ends in a stream
synchronise and the copy of the results), median of --runs after two warm-up runs, and the
device-event time of each phase from gpt_gpdraw_last_timing, median over the same runs.  Derived:
the triangular product's GB/s on one read of the triangle (S = 1) and the covariance pass's
TFLOP/s (2 N Ntest^2 / 2 flops for the lower blocks).  Yardsticks: (a) numpy / scipy on --threads
BLAS threads, one run; (b) torch.linalg.cholesky + torch.matmul on the same device, median of
--runs.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ["noise", "assembly", "solve", "covariance", "cholesky", "product"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpdraw_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--max-n", type=int, default=16384)
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)
    import numpy as np
    from scipy.linalg import cholesky, solve_triangular
    from scipy.spatial.distance import cdist
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import P_D, check, lib
    assert lib().gpt_device_count() > 0, "time_gpdraw.py needs a GPU"

    def kernel(Xa, Xb, h):
        ls = h[:-2]
        return h[-2] ** 2 * np.exp(-0.5 * cdist(Xa / ls, Xb / ls, "sqeuclidean"))

    def timed(fun, runs):
        """Host ms (median, min, max) and the median device phases of fun over runs."""
        ts, ph = [], []
        buf = np.zeros(len(PHASES))
        for it in range(runs + 2):
            t0 = time.perf_counter()
            fun()
            dt = (time.perf_counter() - t0) * 1e3
            check(lib().gpt_gpdraw_last_timing(buf.ctypes.data_as(P_D), len(PHASES)))
            if it >= 2:
                ts.append(dt)
                ph.append(buf.copy())
        m = np.median(np.stack(ph), axis=0)
        return {"ms": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
                "device_ms": float(m.sum()), "phase_ms": dict(zip(PHASES, m.tolist()))}

    def torch_med(fun, runs):
        import torch
        ts = []
        for it in range(runs + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fun()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"runs": a.runs, "rows": rows}, f, indent=1)

    # ---- prior draws
    for N in (2500, 10000, 16384):
        if N > a.max_n:
            continue
        rng = np.random.default_rng(N)
        X = rng.uniform(-3, 3, (N, 2))
        h = np.array([1.0, 1.0, 0.05])
        gp = G.ExactGP(X, np.zeros(N))
        for S in (1, 256):
            row = {"what": "draw_prior", "N": N, "D": 2, "S": S}
            row.update(timed(lambda: gp.draw_prior(h, S=S, seed=1), a.runs))
            if S == 1:
                row["product_GBps_one_triangle_read"] = 8.0 * N * (N + 1) / 2 / (
                    row["phase_ms"]["product"] * 1e-3) / 1e9
            row["cholesky_gflops"] = N ** 3 / 3.0 / (row["phase_ms"]["cholesky"] * 1e-3) / 1e9
            if not a.no_torch:
                import torch
                K = kernel(X, X, h)
                K[np.diag_indices_from(K)] += 1e-6
                Kd = torch.from_numpy(K).cuda()
                Zd = torch.randn(N, S, dtype=torch.float64, device="cuda")
                row["torch_cholesky_ms"] = torch_med(lambda: torch.linalg.cholesky(Kd), a.runs)
                Ld = torch.linalg.cholesky(Kd)
                row["torch_matmul_ms"] = torch_med(lambda: torch.matmul(Ld, Zd), a.runs)
                del Kd, Ld, Zd
                torch.cuda.empty_cache()
            if not a.no_cpu and S == 1:
                t0 = time.perf_counter()
                K = kernel(X, X, h)
                K[np.diag_indices_from(K)] += 1e-6
                t1 = time.perf_counter()
                L = cholesky(K, lower=True, overwrite_a=True, check_finite=False)
                t2 = time.perf_counter()
                L @ rng.standard_normal((N, 256))
                t3 = time.perf_counter()
                row["numpy_threads"] = a.threads
                row["numpy_ms"] = {"assembly": (t1 - t0) * 1e3, "cholesky": (t2 - t1) * 1e3,
                                   "product_S256": (t3 - t2) * 1e3}
            emit(row)
        gp.close()

    # ---- posterior draws and theta draws on PowerPlant
    import exactgp_ref as ER
    pp = np.load(os.path.join(ROOT, "tests", "golden", "powerplant.npz"))["data"]
    tr, te = pp[:5000], pp[5000:]
    mu, sd = tr[:, :4].mean(axis=0), tr[:, :4].std(axis=0, ddof=1)
    X, Xte = (tr[:, :4] - mu) / sd, (te[:, :4] - mu) / sd
    y = (tr[:, 4] - tr[:, 4].mean()) / tr[:, 4].std(ddof=1)
    h = np.array(ER.EXACT)
    N, S = X.shape[0], 256
    gp = G.ExactGP(X, y)
    gp.nlogmarginal(h)                                   # the draws reuse this factor
    for Nt in (1024, Xte.shape[0]):
        Xt = Xte[:Nt]
        row = {"what": "draw_posterior", "N": N, "D": 4, "Ntest": Nt, "S": S}
        row.update(timed(lambda: gp.draw_posterior(h, Xt, S=S, seed=1), a.runs))
        row["covariance_tflops"] = N * Nt * (Nt + 1.0) / (row["phase_ms"]["covariance"] * 1e-3) / 1e12
        if not a.no_torch:
            import torch
            K = kernel(X, X, h)
            K[np.diag_indices_from(K)] += h[-1]
            Ld = torch.linalg.cholesky(torch.from_numpy(K).cuda())
            Ksd = torch.from_numpy(kernel(X, Xt, h)).cuda()
            Kss = torch.from_numpy(kernel(Xt, Xt, h)).cuda()
            Zd = torch.randn(Nt, S, dtype=torch.float64, device="cuda")
            try:
                row["torch_solve_ms"] = torch_med(
                    lambda: torch.linalg.solve_triangular(Ld, Ksd, upper=False), a.runs)
                Vd = torch.linalg.solve_triangular(Ld, Ksd, upper=False)
                row["torch_covariance_ms"] = torch_med(lambda: Kss - Vd.T @ Vd, a.runs)
                Sg = Kss - Vd.T @ Vd + 1e-6 * torch.eye(Nt, dtype=torch.float64, device="cuda")
                row["torch_cholesky_ms"] = torch_med(lambda: torch.linalg.cholesky(Sg), a.runs)
                Ls = torch.linalg.cholesky(Sg)
                row["torch_matmul_ms"] = torch_med(lambda: torch.matmul(Ls, Zd), a.runs)
            except RuntimeError as e:
                row["torch_error"] = str(e).splitlines()[0]
            torch.cuda.empty_cache()
        if not a.no_cpu:
            K = kernel(X, X, h)
            K[np.diag_indices_from(K)] += h[-1]
            L = cholesky(K, lower=True, overwrite_a=True, check_finite=False)
            t0 = time.perf_counter()
            Ks = kernel(X, Xt, h)
            t1 = time.perf_counter()
            V = solve_triangular(L, Ks, lower=True, overwrite_b=True, check_finite=False)
            t2 = time.perf_counter()
            Sg = kernel(Xt, Xt, h) - V.T @ V
            Sg[np.diag_indices_from(Sg)] += 1e-6
            t3 = time.perf_counter()
            Ls = cholesky(Sg, lower=True, overwrite_a=True, check_finite=False)
            t4 = time.perf_counter()
            Ls @ np.random.default_rng(0).standard_normal((Nt, S))
            t5 = time.perf_counter()
            row["numpy_threads"] = a.threads
            row["numpy_ms"] = {"assembly": (t1 - t0) * 1e3, "solve": (t2 - t1) * 1e3,
                               "covariance": (t3 - t2) * 1e3, "cholesky": (t4 - t3) * 1e3,
                               "product": (t5 - t4) * 1e3}
        emit(row)
    gp.close()

    n = 800
    Zf, bf = G.feature_inputs(n, 4, 1)
    nt = G.NoTensorMarginal(X, y, Zf, bf[:, 0])
    nt.nlogmarginal(h)
    nt.predict(h, Xte[:8])                               # leaves L^-T on the device
    row = {"what": "draw_theta", "n": n, "N": N, "S": S}
    row.update(timed(lambda: nt.draw_theta(h, S, seed=1), a.runs))
    row1 = timed(lambda: nt.draw_theta(h, 1, seed=1), a.runs)
    row["S1"] = row1
    row["product_GBps_one_triangle_read_S1"] = 8.0 * n * (n + 1) / 2 / (
        row1["phase_ms"]["product"] * 1e-3) / 1e9
    nt.close()
    emit(row)


if __name__ == "__main__":
    main()
