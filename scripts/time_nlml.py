"""Time the device marginal likelihood (gpt_amd/csrc/nlml.hip) against the literal numpy
restatement of GPT_SGLD.jl:921-962.

    python scripts/time_nlml.py [--runs 11] [--threads 16] [--out profiles/nlml_bench.json]

Shapes: PowerPlant at full size (N = 9568, D = 4, n in {100, 200, 400, 800}) and a kin40k-like
N = 10000, D = 8, n = 500.  Per shape and for value-only / value + gradient evaluations: the host
time of one evaluation on a resident handle (a host clock around the call, which ends in a
stream synchronise and the copy of the results) and the device-event time of each phase, each the
median of --runs runs after two warm-up runs.  Beside them the fp64 numpy restatement (value:
nlogmarginal; gradient: gradnlogmarginal_literal, which repeats the value's work as the reference
does) on --threads BLAS threads, median of three.  The gradient GEMM's rate is 2 n^2 N flops over
its phase time, set against the fp64 matrix peak.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ["features", "syrk", "gemv", "cholesky", "trsv", "inv_factor", "inverse", "residual",
          "grad_gemm", "grad_finish", "scalars"]
FP64_MATRIX_PEAK = 78.6e12          # MI355X fp64 matrix flop/s


def shapes():
    out = [("powerplant", 9568, 4, n) for n in (100, 200, 400, 800)]
    out.append(("kin40k_like", 10000, 8, 500))
    return out


def inputs(name, N, D, n):
    import numpy as np
    import nlml_ref as NR
    rng = np.random.default_rng(11)
    if name == "powerplant":
        pp = np.load(os.path.join(ROOT, "tests", "golden", "powerplant.npz"))["data"]
        X, y = NR.whiten(pp[:N, :D]), NR.whiten(pp[:N, 4])
        h = np.array(NR.EXPERIMENT)
    else:
        X = rng.standard_normal((N, D))
        y = np.sin(X).sum(axis=1) + 0.1 * rng.standard_normal(N)
        h = np.array([1.5] * D + [1.0, 0.05])
    Z = rng.standard_normal((n, D))
    b = 2 * np.pi * rng.random(n)
    return X, y, Z, b, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlml_bench.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)
    import numpy as np
    import nlml_ref as NR
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import C, P_D, check, lib
    assert lib().gpt_device_count() > 0, "time_nlml.py needs a GPU"
    rows = []
    for name, N, D, n in shapes():
        X, y, Z, b, h = inputs(name, N, D, n)
        m = G.NoTensorMarginal(X, y, Z, b)
        hp = np.ascontiguousarray(h)
        row = {"shape": name, "N": N, "D": D, "n": n, "hyper": h.tolist()}
        for want_grad, key in ((0, "value"), (1, "value_grad")):
            val = C.c_double()
            grad = np.empty(h.size)
            ph = np.empty(len(PHASES))
            host, phases = [], []
            for it in range(a.runs + 2):
                t0 = time.perf_counter()
                check(lib().gpt_nlml_eval(m._h, hp.ctypes.data_as(P_D), h.size, want_grad,
                                          C.byref(val), grad.ctypes.data_as(P_D), None))
                t1 = time.perf_counter()
                check(lib().gpt_nlml_eval_timed(m._h, hp.ctypes.data_as(P_D), h.size, want_grad,
                                                C.byref(val), grad.ctypes.data_as(P_D),
                                                ph.ctypes.data_as(P_D)))
                if it >= 2:
                    host.append((t1 - t0) * 1e3)
                    phases.append(ph.copy())
            med = np.median(np.stack(phases), axis=0)
            row[key] = {"host_ms": float(np.median(host)), "host_ms_min": float(np.min(host)),
                        "host_ms_max": float(np.max(host)), "device_ms": float(med.sum()),
                        "phase_ms": dict(zip(PHASES, med.tolist())),
                        "phase_share": dict(zip(PHASES, (med / med.sum()).tolist()))}
            if want_grad:
                flops = 2.0 * n * n * N
                gemm = med[PHASES.index("grad_gemm")] * 1e-3
                row[key]["grad_gemm_tflops"] = flops / gemm / 1e12
                row[key]["grad_gemm_share_of_fp64_matrix_peak"] = flops / gemm / FP64_MATRIX_PEAK
                row["nlml"] = val.value
        m.close()
        if not a.no_cpu:
            def med3(fun):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fun()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return float(np.median(ts))
            row["numpy_threads"] = a.threads
            row["numpy_value_ms"] = med3(lambda: NR.nlogmarginal(X, y, Z, b, h))
            row["numpy_literal_grad_ms"] = med3(lambda: NR.gradnlogmarginal_literal(X, y, Z, b, h))
            row["speedup_value"] = row["numpy_value_ms"] / row["value"]["host_ms"]
            row["speedup_value_grad"] = ((row["numpy_value_ms"] + row["numpy_literal_grad_ms"])
                                         / row["value_grad"]["host_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": a.runs, "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "rows": rows}, f,
                  indent=1)


if __name__ == "__main__":
    main()
