"""Time X-mode sessions (features staged per minibatch from X) against phi-mode sessions.

    python scripts/time_xmode.py [--shape bench|kin40k_ref] [--chains 256] [--seconds 1.0]
                                 [--repeats 5] [--spans 8] [--legs phi,x] [--out FILE.json]

Two legs on the same seeded inputs (kin40k, every chain its own length scales and sigma_RBF, the
sweep block of kin40kExperiment.jl:67-74), alternated `--repeats` times, each timed window at
least `--seconds` of whole epochs (graph replays), host clock around run() + sync() after a
two-epoch warm-up:
  phi   SGLDSession on one feature_device() phi per chain (the existing API only)
  x     SGLDSession.from_X; with several --spans (chain engine: 4,8,16) one x leg per span cap
        (GPTSGLD_XSPAN)
and, in the same call, gpt_feature_dev on nchains*m rows: the stager's yardstick (the same
arithmetic on the same number of elements).  The stager's own kernel time comes from a separate
run under `rocprofv3 --kernel-trace --stats -- python scripts/time_xmode.py --legs x --repeats 1`
(kernel stage_batches_kernel; one launch covers up to `span` steps).  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"bench": dict(n=500, r=5, epsw=1e-5, epsU=1e-8, engine="chain"),
          "kin40k_ref": dict(n=150, r=20, epsw=1e-4, epsU=1e-7, engine="wave")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="bench", choices=sorted(SHAPES))
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--Q", type=int, default=200)
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--N", type=int, default=0, help="training rows (default: all of kin40k)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spans", default="8", help="chain engine: X-mode span caps to time (4,8,16)")
    ap.add_argument("--legs", default="phi,x")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import ctypes as CT

    import torch
    import bench
    from gpt_amd._lib import check, lib
    from gpt_amd import GPT_SGLD as G
    from gpt_amd.session import SGLDSession, feature_device
    assert torch.cuda.is_available(), "time_xmode.py needs a GPU"
    dev = torch.device("cuda", 0)
    sh = SHAPES[a.shape]
    n, r, D, Q, m, C = sh["n"], sh["r"], 8, a.Q, a.m, a.chains
    Xtr, ytr, _, _, _ = bench.kin40k(D)
    if a.N:
        Xtr, ytr = Xtr[:a.N], ytr[:a.N]
    N = Xtr.shape[0]
    nb = -(-N // m)
    I = G.samplenz(r, D, Q, 17)
    Z, b = G.feature_inputs(n, D, 17)
    scale = math.sqrt(n / Q ** (1.0 / D))
    rng = np.random.default_rng(1)
    ls = np.array(bench.KIN40K_LS)[None, :] * (1.0 + 0.2 * rng.random((C, D)))     # distinct rows
    sg = 1.0420 * (1.0 + 0.1 * rng.random(C))
    seeds = list(range(1, C + 1))
    Xd = torch.from_numpy(np.ascontiguousarray(Xtr.T)).to(dev)
    Zd = torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev)
    bd = torch.from_numpy(np.ascontiguousarray(b.T)).to(dev)
    lsd = torch.from_numpy(np.ascontiguousarray(ls)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(ytr)).to(dev)
    common = dict(store=False, engine=sh["engine"])
    hyper = (I, r, Q, m, sh["epsw"], sh["epsU"], 0.0476, 0, 1000000, seeds)

    legs = {}
    names = a.legs.split(",")
    if "phi" in names:
        phis = [feature_device(Xd, lsd[c], float(sg[c]), scale, Zd, bd) for c in range(C)]
        torch.cuda.synchronize()
        legs["phi"] = SGLDSession(phis, yd, *hyper, **common)
    spans = [int(s) for s in a.spans.split(",")] if sh["engine"] == "chain" else [1]
    staging = {}
    if "x" in names:
        for sp in spans:
            os.environ["GPTSGLD_XSPAN"] = str(sp)
            key = "x" if len(spans) == 1 else "x_span%d" % sp
            legs[key] = SGLDSession.from_X(Xd, yd, lsd, sg, scale, Zd, bd, *hyper, **common)
            staging[key] = legs[key].staging()
        os.environ.pop("GPTSGLD_XSPAN", None)

    # warm-up: two epochs (captures the epoch graph), then size the window from a timed epoch
    steps = {}
    for k, s in legs.items():
        assert s.info()["engine"] == sh["engine"]
        s.run(2 * nb)
        s.sync()
        t0 = time.perf_counter()
        s.run(nb)
        s.sync()
        per = (time.perf_counter() - t0) / nb
        steps[k] = max(1, math.ceil(a.seconds / per / nb)) * nb
    ms = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, s in legs.items():                 # alternate the legs
            t0 = time.perf_counter()
            s.run(steps[k])
            s.sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps[k])
    for k, s in legs.items():
        assert all(s.status(c) in (0, 1) for c in range(min(C, 4)))

    # the stager's yardstick: gpt_feature_dev on nchains*m rows, same element count as one step
    rows = C * m
    Xs = Xd[:, :min(rows, N)].repeat(1, -(-rows // min(rows, N)))[:, :rows].contiguous()
    feature_device(Xs, lsd[0], float(sg[0]), scale, Zd, bd)
    torch.cuda.synchronize()
    reps = 20
    fms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = torch.empty((rows, D, n), dtype=torch.float64, device=dev)
        e0.record()
        for _ in range(reps):
            check(lib().gpt_feature_dev(CT.c_void_p(Xs.data_ptr()), rows, D,
                                        CT.c_void_p(lsd[0].data_ptr()), D, float(sg[0]), scale,
                                        CT.c_void_p(Zd.data_ptr()), CT.c_void_p(bd.data_ptr()), n,
                                        CT.c_void_p(out.data_ptr()), None))
        e1.record()
        torch.cuda.synchronize()
        fms.append(e0.elapsed_time(e1) / reps)

    elems = float(C) * m * n * D
    med = lambda v: float(np.median(v))
    res = dict(script="time_xmode", shape=a.shape, engine=sh["engine"], n=n, D=D, N=N, r=r, Q=Q,
               m=m, chains=C, repeats=a.repeats, timed_steps=steps,
               ms_per_step={k: med(v) for k, v in ms.items()},
               ms_per_step_all={k: [round(x, 5) for x in v] for k, v in ms.items()},
               staging=staging, phi_bytes_per_chain=8 * n * D * N,
               elements_per_step=elems,
               feature_dev_ms=med(fms), feature_dev_ms_all=[round(x, 5) for x in fms],
               feature_dev_gelem_s=elems / med(fms) / 1e6)
    if "phi" in ms:
        for k in ms:
            if k != "phi":
                res.setdefault("ratio_x_over_phi", {})[k] = med(ms[k]) / med(ms["phi"])
                d = med(ms[k]) - med(ms["phi"])
                res.setdefault("step_time_added_ms", {})[k] = d
                res.setdefault("stager_gelem_s_from_added_time", {})[k] = (
                    elems / d / 1e6 if d > 0 else None)
    for s in legs.values():
        s.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
