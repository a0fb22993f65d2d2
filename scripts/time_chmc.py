"""Time Hamiltonian Monte Carlo on the softmax classifier's theta (gpt_amd/csrc/chmc.hip) beside the
Langevin steps of the same handle, and record its acceptance rates and test quality.

    python scripts/time_chmc.py [--runs 11] [--out profiles/chmc_bench.json] [--headline FILE]

Shapes: the segment shape (n = 150, N = 1300, D = 16, C = 7, tests/golden/segment.npz) and an
MNIST-like n = 1000, N = 60000, D = 16, C = 10 of seeded normals (scripts/time_cjoint.py's).  Per
shape and L in {1, 8}: device-event windows around one SoftmaxJoint.hmc call of T and of 3T
transitions and, from the same handle in the same session, around T*L and 3T*L Langevin steps;
median, min and max of --runs windows after two warm-up windows each, the four alternating.  The
events are recorded on the null stream, which the library runs on, around the whole call, so a
window also holds what a call costs once: the upload of the length scales, the evaluation that
forms U and grad U of the starting theta (set_theta before every window drops the cache), the
allocation and the copy of the store and the records.  `per_transition` is therefore the slope
(t(3T) - t(T)) / 2T, `per_call` the intercept, and `whole_call` t(3T) / 3T.  `ratio` is the hmc slope
over the Langevin slope; `spread` is (max - min) / median of the 3T Langevin windows.  With U and
grad U of the state cached, a transition runs L evaluations and L + 4 small kernels, a Langevin
step one evaluation and one small kernel.

Also: the acceptance rate of 200 transitions at eps in {1e-4, 1e-3, 1e-2, 4e-2} (segment shape,
from the state after 300 Langevin steps of eps = 1e-3 from zero), and the window-averaged test
miss rate and NLP of an HMC store beside a GPNT_SGLDclass store of the same length on the segment split, through
GPNT_pred_class.  --headline names a JSON file with the benchmark's alternating A/B lines, stored
as `headline_ab`.  Needs the GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_cjoint import inputs  # noqa: E402


def stats(ts, per):
    import numpy as np
    ts = np.asarray(ts) / per
    return {"device_ms": float(np.median(ts)), "device_ms_min": float(ts.min()),
            "device_ms_max": float(ts.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chmc_bench.json"))
    ap.add_argument("--headline", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import cls_ref as CLS
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import lib
    assert lib().gpt_device_count() > 0 and torch.cuda.is_available(), "time_chmc.py needs a GPU"

    def window(fun):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.default_stream())
        fun()
        e1.record(torch.cuda.default_stream())
        e1.synchronize()
        return e0.elapsed_time(e1)

    def slope(t1, t3, T):
        t1, t3 = np.asarray(t1), np.asarray(t3)
        return {"per_transition": {"device_ms": float(np.median(t3) - np.median(t1)) / (2 * T)},
                "per_call_ms": float(1.5 * np.median(t1) - 0.5 * np.median(t3)),
                "whole_call": stats(t3, 3 * T), "windows_ms": {"T": stats(t1, 1), "3T": stats(t3, 1)}}

    rows = []
    eps = 1e-6
    for name, T in (("segment", 200), ("mnist_like", 10)):
        X, y, Z, b, theta, h, ncls = inputs(name)
        j = G.SoftmaxJoint(X, y, Z, b, C=ncls)
        row = {"shape": name, "N": X.shape[0], "D": X.shape[1], "n": Z.shape[0], "C": ncls,
               "T": T, "eps": eps, "by_L": {}}
        for L in (1, 8):
            t = {k: [] for k in ("h1", "h3", "l1", "l3")}
            acc = []
            for it in range(a.runs + 2):
                got = {}
                for key, mult in (("h1", 1), ("l1", 1), ("h3", 3), ("l3", 3)):
                    j.set_theta(theta)
                    if key[0] == "h":
                        res = []
                        got[key] = window(lambda: res.append(j.hmc(h, eps, L, mult * T, 3, t0=0)))
                        rate = res[0].accept_rate
                    else:
                        got[key] = window(lambda: j.langevin(h, eps, mult * T * L, 3, t0=0))
                if it >= 2:
                    for key in t:
                        t[key].append(got[key])
                    acc.append(rate)
            r = {"hmc": slope(t["h1"], t["h3"], T), "langevin_L_steps": slope(t["l1"], t["l3"], T),
                 "accept_rate": float(np.mean(acc))}
            r["ratio"] = (r["hmc"]["per_transition"]["device_ms"]
                          / r["langevin_L_steps"]["per_transition"]["device_ms"])
            r["ratio_whole_call"] = (r["hmc"]["whole_call"]["device_ms"]
                                     / r["langevin_L_steps"]["whole_call"]["device_ms"])
            w = r["langevin_L_steps"]["windows_ms"]["3T"]
            r["spread"] = (w["device_ms_max"] - w["device_ms_min"]) / w["device_ms"]
            row["by_L"][str(L)] = r
        print(json.dumps(row), flush=True)
        rows.append(row)
        j.close()

    # acceptance rates and test quality on the segment split
    Xtr, ytr, Xte, yte = CLS.segment_problem()
    S = CLS.SEG
    n, C = S["n"], 7
    Z, b = G.feature_inputs(n, 16, S["feature_seed"])
    b = b[:, 0]
    h = np.array(CLS.SEG_LS + [CLS.SEG_SIGMA_RBF])
    j = G.SoftmaxJoint(Xtr, ytr.astype(np.float64), Z, b, C=C)
    accept = {}
    j.set_theta(np.zeros((n, C)))
    j.langevin(h, 1e-3, 300, S["seed"], t0=0)
    start = j.theta()
    for L in (1, 8):
        for eps in (1e-4, 1e-3, 1e-2, 4e-2):
            j.set_theta(start)
            r = j.hmc(h, eps, L, 200, S["seed"], t0=300)
            accept["L%d_eps%g" % (L, eps)] = {"accept_rate": r.accept_rate, "ndivergent": r.ndivergent,
                                              "mean_abs_dH": float(np.abs(r.dH).mean())}
    phitr = G.featureNotensor(Xtr, h[:16], h[-1], Z, b)
    phite = G.featureNotensor(Xte, h[:16], h[-1], Z, b)
    nb = -(-S["Ntrain"] // S["m"])
    sgld = G.GPNT_SGLDclass(phitr, ytr, S["sigma_theta"], S["m"], S["eps_theta"], S["decay_rate"],
                            S["burnin"], S["maxepoch"], S["seed"])
    nburn, nkeep = S["burnin"] * nb, S["maxepoch"] * nb
    ev = G.GPNT_pred_class(sgld, phite, yte, window=(nburn, nburn + nkeep))
    quality = {"samples": nkeep, "burnin": nburn,
               "GPNT_SGLDclass": {"eps_theta": S["eps_theta"], "m": S["m"],
                                  "avg_prop_missed": ev.avg_prop_missed, "avg_mean_nlp": ev.avg_mean_nlp}}
    for L, eps in ((1, 1e-3), (8, 2.5e-4)):
        j.set_theta(sgld[:, :, 0])
        r = j.hmc(h, eps, L, nkeep, S["seed"], burnin=nburn, t0=0)
        ev = G.GPNT_pred_class(r.theta_store, phite, yte, window=(0, nkeep))
        quality["hmc_L%d_eps%g" % (L, eps)] = {"accept_rate": r.accept_rate,
                                               "avg_prop_missed": ev.avg_prop_missed,
                                               "avg_mean_nlp": ev.avg_mean_nlp}
    print(json.dumps({"accept": accept, "quality": quality}), flush=True)
    out = {"runs": a.runs, "rows": rows, "segment_accept": accept, "segment_quality": quality}
    if a.headline and os.path.exists(a.headline):
        with open(a.headline) as f:
            out["headline_ab"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
