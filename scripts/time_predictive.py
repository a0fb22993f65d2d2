"""Device time of the posterior-predictive evaluator (gpt_amd/csrc/predictive.hip) at the two
experiment shapes, written to profiles/predictive_bench.json:

    PowerPlantNoTensor   Ntest = 4568,  T = 100, window 60:100 (S = 41)
    kin40k               Ntest = 30000, T = S = 224

Per shape: the evaluator's device-event time on device predictions (gpt_predictive_last_timing,
median of --reps calls) and its GB/s on one read of 8·Ntest·S bytes; the scores and the two
mean/SSE launches of GPNT_pred on full-theta samples of n features (gpt_gpnt_last_timing "eval")
beside the evaluator inside GPNT_predictive of the same samples; and the numpy restatement
(tests/predictive_ref.py) with the rows split over 16 threads.

    python scripts/time_predictive.py [--reps 7] [--headline-ab FILE]

--headline-ab merges a json list of alternating bench.py results of this library and the parent
commit's (GPTSGLD_LIB) into the output as `headline_ab`; an existing one is kept otherwise."""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = {"PowerPlantNoTensor": dict(Ntest=4568, T=100, window=(59, 100), n=100, noise_var=0.0529),
          "kin40k": dict(Ntest=30000, T=224, window=(0, 224), n=1000, noise_var=0.0476)}


def numpy_16_threads(F, y, a, b, nv):
    import predictive_ref as PR
    cuts = np.linspace(0, y.size, 17).astype(int)
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda k: PR.predictive_np(F[cuts[k]:cuts[k + 1]], y[cuts[k]:cuts[k + 1]], a, b, nv),
                    range(16)))
    return 1e3 * (time.perf_counter() - t0)


def one_shape(name, s, reps):
    import torch
    from gpt_amd import GPT_SGLD as G
    from gpt_amd.session import predictive_device
    Nt, T, (a, b), n, nv = s["Ntest"], s["T"], s["window"], s["n"], s["noise_var"]
    rng = np.random.default_rng(5)
    theta = np.asfortranarray(rng.standard_normal((n, T)) / np.sqrt(n))
    phitest = np.asfortranarray(np.sqrt(2.0) * np.cos(rng.uniform(0, 2 * np.pi, (n, Nt))))
    y = phitest.T @ theta.mean(axis=1) + np.sqrt(nv) * rng.standard_normal(Nt)
    ev = G.GPNT_pred(theta, phitest, y, window=(a, b), scores=True)
    fhat, yd = torch.from_numpy(np.ascontiguousarray(ev.scores.T)).cuda(), torch.from_numpy(y).cuda()
    dev, pred_eval, inside = [], [], []
    for _ in range(reps + 1):                       # the first call carries the module load
        predictive_device(fhat, yd, nv, window=(a, b))
        dev.append(G.predictive_last_timing())
        G.GPNT_pred(theta, phitest, y, window=(a, b))
        pred_eval.append(G.gpnt_last_timing()["eval"])
        G.GPNT_predictive(theta, phitest, y, nv, window=(a, b))
        inside.append(G.predictive_last_timing())
    ms = statistics.median(dev[1:])
    out = dict(Ntest=Nt, T=T, window=[a, b], n=n, evaluator_ms=ms, evaluator_ms_min=min(dev[1:]),
               evaluator_gbps=8e-6 * Nt * (b - a) / ms,
               gpnt_pred_scores_and_mean_sse_ms=statistics.median(pred_eval[1:]),
               evaluator_inside_gpnt_predictive_ms=statistics.median(inside[1:]),
               numpy_16_threads_ms=numpy_16_threads(ev.scores, y, a, b, nv))
    print(name, json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--headline-ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_bench.json"))
    args = ap.parse_args()
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out = {"shapes": {k: one_shape(k, s, args.reps) for k, s in SHAPES.items()}}
    if args.headline_ab:
        out["headline_ab"] = json.load(open(args.headline_ab))
    elif "headline_ab" in old:
        out["headline_ab"] = old["headline_ab"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
