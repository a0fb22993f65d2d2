"""Timing of the classification side on the device: GPNT_SGLDclass steps per second at the
segment shape for 1 and 256 chains beside the numpy restatement on 16 threads, and the time of an
evaluation call (full-theta and tensor path, the latter split into prediction and evaluation) at
the experiment's size and at a larger one.

    python scripts/time_class.py [--out profiles/class_bench.json]

Device times are device events inside the library (gpt_class_last_timing) around the kernels of a
call; call times are wall clock around the whole host-pointer call (uploads, kernels, downloads).
Every figure is the median over a window of repeated calls of at least 0.2 s, after a warm-up call.
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")

import argparse
import json
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cls_ref as CR  # noqa: E402
from gpt_amd import GPT_SGLD as G  # noqa: E402
from gpt_amd import _lib  # noqa: E402

WINDOW_S = 0.2


def last_ms():
    ms = np.zeros(3)
    _lib.check(_lib.lib().gpt_class_last_timing(ms.ctypes.data_as(_lib.P_D)))
    return ms


def timed(fn, slots):
    """Median wall seconds and median device ms of the slots over a window >= WINDOW_S."""
    fn()                                                   # warm-up
    wall, dev = [], []
    t_end = time.perf_counter() + WINDOW_S
    while len(wall) < 3 or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        dev.append(last_ms()[slots])
    return float(np.median(wall)), np.median(np.array(dev), axis=0), len(wall)


def sampler(out):
    c = CR.SEG
    Xtr, ytr, _, _ = CR.segment_problem()
    phi = G.featureNotensor_seeded(Xtr, c["n"], CR.SEG_LS, CR.SEG_SIGMA_RBF, c["feature_seed"])
    n, N = phi.shape
    nb = -(-N // c["m"])
    epochs = 12
    steps = epochs * nb
    res = dict(n=n, N=N, C=7, m=c["m"], steps_per_call=steps)
    for nch in (1, 256):
        seeds = list(range(1, nch + 1))
        eps = [c["eps_theta"]] * nch

        def call():
            G.GPNT_SGLDclass_chains(phi, ytr, 1.0, c["m"], eps, 0.0, 0, epochs, seeds, store_every=nb)
        wall, dev, reps = timed(call, [0])
        res["chains_%d" % nch] = dict(
            chain_steps_per_s_device=nch * steps / (dev[0] * 1e-3), device_ms=float(dev[0]),
            chain_steps_per_s_call=nch * steps / wall, call_s=wall, calls=reps)
    t0 = time.perf_counter()
    reps = 0
    while reps < 2 or time.perf_counter() - t0 < WINDOW_S:
        CR.gpnt_sgld_class(phi, ytr, 1.0, c["m"], c["eps_theta"], 0.0, 0, epochs, 1)
        reps += 1
    res["numpy_restatement"] = dict(steps_per_s=reps * steps / (time.perf_counter() - t0),
                                    threads=int(os.environ["OMP_NUM_THREADS"]), calls=reps)
    out["sampler"] = res


def evaluation(out):
    res = {}
    for (Nt, C, T) in ((1010, 7, 100), (30000, 10, 200)):
        rng = np.random.default_rng(Nt)
        y = rng.integers(1, C + 1, Nt)
        window = (T // 2, T)
        n = 150
        theta = np.asfortranarray(rng.standard_normal((n, C, T)))
        phite = np.asfortranarray(np.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, Nt))))
        wall, dev, reps = timed(lambda: G.GPNT_pred_class(theta, phite, y, window=window), [1, 2])
        key = "Ntest%d_C%d_T%d" % (Nt, C, T)
        res[key] = dict(full_theta=dict(n=n, call_s=wall, scores_ms=float(dev[0]),
                                        evaluation_ms=float(dev[1]), calls=reps))
        n, D, r, Q = 5, 16, 10, 200                       # ImageExperiment.jl:13-34
        w = np.asfortranarray(rng.standard_normal((Q, C, T)))
        U = np.asfortranarray(rng.standard_normal((n, r, D, C, T)) / np.sqrt(n))
        I = G.samplenz(r, D, Q, 1)
        ph = np.asfortranarray(rng.standard_normal((n, D, Nt)) * 0.6)
        wall, dev, reps = timed(lambda: G.pred_class(w, U, I, ph, y, window=window), [1, 2])
        res[key]["tensor"] = dict(n=n, D=D, r=r, Q=Q, call_s=wall, prediction_ms=float(dev[0]),
                                  evaluation_ms=float(dev[1]), calls=reps)
    out["evaluation"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_bench.json"))
    a = ap.parse_args()
    import torch
    out = dict(device=torch.cuda.get_device_name(0), window_s=WINDOW_S)
    sampler(out)
    evaluation(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
