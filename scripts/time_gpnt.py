"""Timing of the full-theta regression chains (GPNT_SGLD_chains) and of GPNT_pred on the device.

    python scripts/time_gpnt.py [--out profiles/gpnt_bench.json]

config1   PowerPlantNoTensorExperiment.jl's shape (n = 2000, N = 5000, m = 50, 100 epochs, seed 1,
          eps = 0.00011): whole-call wall time of GPNT_SGLD against GPNT_SGLD_chains with one chain,
          at store_every = 1 and at store_every = numbatches.
sweep     256 chains at that shape: chain-steps/s, sampler kernel time per step of all chains, and
          bytes/s on the algorithmic traffic 8·n·m per chain-step (one read of the batch) over that
          kernel time; GPTSGLD_GPNT_ROWS=0 (rows read twice, no staging) and groups of 4, 2 and 1
          rows against the default.
kin40k    kin40kNoTensorExperiment.jl's shape (n = 8000, N = 10 000, m = 50), features formed from
          X on the device, 1 and 64 chains, the same figures; the one row that fits beside theta is
          not staged by default, GPTSGLD_GPNT_ROWS=1 stages it.
eval      GPNT_pred on the 100 epoch ends of the 4568 PowerPlant test rows: the call time, the RMSE
          of the 60:100 average, and its difference from the numpy evaluation of the same theta.

The versions of a comparison alternate inside this one process, three rounds after a warm-up call
of each; the median and the spread (max - min) of the rounds are reported.  Wall times are around
whole host-pointer calls (uploads, kernels, downloads); kernel times are device events inside the
library (gpt_gpnt_last_timing).
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "16")

import argparse
import json
import math
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import kin40k, powerplant  # noqa: E402
from gpt_amd import GPT_SGLD as G  # noqa: E402

ROUNDS = 3
ROWS_ENV = "GPTSGLD_GPNT_ROWS"


def alternate(versions):
    """versions: name -> callable.  One warm-up call each, then ROUNDS rounds in turn.  Returns
    name -> dict(wall_s, sampler_ms: median and spread, route) and the last result of each."""
    last = {}
    for name, fn in versions.items():
        last[name] = fn()
    wall = {k: [] for k in versions}
    dev = {k: [] for k in versions}
    route = {}
    for _ in range(ROUNDS):
        for name, fn in versions.items():
            t0 = time.perf_counter()
            last[name] = fn()
            wall[name].append(time.perf_counter() - t0)
            dev[name].append(G.gpnt_last_timing()["sampler"])
            route[name] = G.gpnt_last_route()
    stat = lambda v: dict(median=float(np.median(v)), spread=float(max(v) - min(v)))
    return {k: dict(wall_s=stat(wall[k]), sampler_ms=stat(dev[k]), route=route[k]) for k in versions}, last


def with_rows(cap, fn):
    def run():
        old = os.environ.pop(ROWS_ENV, None)
        if cap is not None:
            os.environ[ROWS_ENV] = str(cap)
        try:
            return fn()
        finally:
            os.environ.pop(ROWS_ENV, None)
            if old is not None:
                os.environ[ROWS_ENV] = old
    return run


def rates(res, n, m, nchains, steps):
    """chain-steps/s, ms per step of all chains and bytes/s on 8·n·m per chain-step, from the
    median sampler kernel time."""
    ms = res["sampler_ms"]["median"]
    res["chain_steps_per_s"] = nchains * steps / (ms * 1e-3)
    res["ms_per_step_all_chains"] = ms / steps
    res["algorithmic_TB_per_s"] = 8.0 * n * m * nchains * steps / (ms * 1e-3) / 1e12
    res["algorithmic_GB_per_s_per_chain"] = 8.0 * n * m * steps / (ms * 1e-3) / 1e9
    return res


def config1(out):
    Xtr, ytr, Xte, yte, ysd = powerplant(4)
    n, m, eps, epochs, sv = 2000, 50, 0.00011, 100, 0.2299 ** 2
    phi = G.featureNotensor(Xtr, n, 1.4332, 1.0, 17)
    phite = G.featureNotensor(Xte, n, 1.4332, 1.0, 17)
    N = phi.shape[1]
    nb = -(-N // m)
    steps = epochs * nb
    res, last = alternate({
        "GPNT_SGLD": lambda: G.GPNT_SGLD(phi, ytr, sv, 1.0, m, eps, 0, 0, epochs, 1),
        "chains_1_store_every_1": lambda: G.GPNT_SGLD_chains(phi, ytr, sv, 1.0, m, eps, 0, 0, epochs, [1]),
        "chains_1_store_every_nb": lambda: G.GPNT_SGLD_chains(phi, ytr, sv, 1.0, m, eps, 0, 0, epochs, [1],
                                                            store_every=nb),
    })
    res["GPNT_SGLD"].pop("sampler_ms")                       # not a chains call: no such figure
    res["GPNT_SGLD"].pop("route")
    for k in ("chains_1_store_every_1", "chains_1_store_every_nb"):
        rates(res[k], n, m, 1, steps)
    old, (new, st) = last["GPNT_SGLD"], last["chains_1_store_every_1"]
    ends = last["chains_1_store_every_nb"][0]
    res["shape"] = dict(n=n, N=N, m=m, epochs=epochs, steps=steps)
    res["chains_vs_GPNT_SGLD_rel"] = float(np.abs(new[:, :, 0] - old).max() / np.abs(old).max())
    res["store_every_nb_equals_columns"] = bool(np.array_equal(ends, new[:, nb - 1::nb, :]))
    a, b = res["chains_1_store_every_1"]["wall_s"], res["GPNT_SGLD"]["wall_s"]
    res["one_chain_condition"] = bool(a["median"] <= b["median"] + b["spread"] and not st.any())
    res["speedup_store_every_1"] = b["median"] / a["median"]
    res["speedup_store_every_nb"] = b["median"] / res["chains_1_store_every_nb"]["wall_s"]["median"]
    out["config1"] = res
    return phi, ytr, phite, yte, ysd, ends[:, :, 0]


def sweep(out, phi, ytr):
    n, N = phi.shape
    m, eps, sv, epochs, nch = 50, 0.00011, 0.2299 ** 2, 10, 256
    nb = -(-N // m)
    steps = epochs * nb
    seeds = list(range(1, nch + 1))
    call = lambda: G.GPNT_SGLD_chains(phi, ytr, sv, 1.0, m, eps, 0, 0, epochs, seeds, store_every=nb)
    versions = {"default": with_rows(None, call), "rows_0": with_rows(0, call)}
    for cap in (4, 2, 1):                                  # what a group of fewer rows than waves costs
        versions["rows_%d" % cap] = with_rows(cap, call)
    res, last = alternate(versions)
    for k in versions:
        rates(res[k], n, m, nch, steps)
    res["shape"] = dict(n=n, N=N, m=m, epochs=epochs, steps=steps, chains=nch)
    res["same_bits"] = bool(all(np.array_equal(last["default"][0], last[k][0]) for k in versions))
    res["staging_speedup"] = res["rows_0"]["sampler_ms"]["median"] / res["default"]["sampler_ms"]["median"]
    out["sweep"] = res


def kin40k_shape(out):
    Xtr, ytr, _, _, _ = kin40k(8)
    n, m, eps, sv, epochs = 8000, 50, 0.0001, 0.065, 2
    N = Xtr.shape[0]
    nb = -(-N // m)
    steps = epochs * nb
    Z, b = G.feature_inputs(n, 8, 17)
    res = dict(shape=dict(n=n, N=N, m=m, epochs=epochs, steps=steps))
    for nch in (1, 64):
        seeds = list(range(1, nch + 1))
        call = lambda: G.GPNT_SGLD_chains_x(Xtr, ytr, 1.5905, 1.1812, Z, b[:, 0], sv, 1.0, m, eps, 0.0,
                                            0, epochs, seeds, store_every=nb)
        # one row fits beside theta here: the default does not stage it, rows_1 does
        r, last = alternate({"default": with_rows(None, call), "rows_1": with_rows(1, call)})
        for k in ("default", "rows_1"):
            rates(r[k], n, m, nch, steps)
        r["same_bits"] = bool(np.array_equal(last["default"][0], last["rows_1"][0]))
        r["finite"] = bool(np.isfinite(last["default"][0]).all() and not last["default"][1].any())
        res["chains_%d" % nch] = r
    out["kin40k_notensor"] = res


def evaluation(out, phite, yte, ysd, ends):
    window = (59, 100)
    ev = G.GPNT_pred(ends, phite, yte, window=window, scale=ysd)          # warm-up
    wall, dev = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        ev = G.GPNT_pred(ends, phite, yte, window=window, scale=ysd)
        wall.append(time.perf_counter() - t0)
        dev.append(G.gpnt_last_timing()["eval"])
    fh = phite.T @ ends
    want = ysd * math.sqrt(np.mean((fh[:, window[0]:window[1]].mean(axis=1) - yte) ** 2))
    want_s = ysd * np.sqrt(np.mean((fh - yte[:, None]) ** 2, axis=0))
    out["evaluation"] = dict(
        Ntest=int(yte.size), T=int(ends.shape[1]), window=list(window),
        call_s=dict(median=float(np.median(wall)), spread=float(max(wall) - min(wall))),
        kernels_ms=dict(median=float(np.median(dev)), spread=float(max(dev) - min(dev))),
        rmse_60_100=ev.rmse, rmse_first_epoch=float(ev.sample_rmse[0]),
        rmse_last_epoch=float(ev.sample_rmse[-1]),
        rmse_vs_numpy_rel=abs(ev.rmse - want) / want,
        sample_rmse_vs_numpy_rel=float(np.abs(ev.sample_rmse - want_s).max() / want_s.max()),
        in_band_3p95_4p35=bool(3.95 <= ev.rmse <= 4.35))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpnt_bench.json"))
    a = ap.parse_args()
    import torch
    out = dict(device=torch.cuda.get_device_name(0), rounds=ROUNDS)
    phi, ytr, phite, yte, ysd, ends = config1(out)
    evaluation(out, phite, yte, ysd, ends)
    sweep(out, phi, ytr)
    kin40k_shape(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    ok = (out["config1"]["one_chain_condition"] and out["evaluation"]["in_band_3p95_4p35"]
          and out["evaluation"]["rmse_vs_numpy_rel"] <= 1e-12)
    if not ok:
        sys.exit("a condition of the measurement does not hold (see the figures above)")


if __name__ == "__main__":
    main()
