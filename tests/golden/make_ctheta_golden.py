"""Regenerate ctheta_mp.npz: the 50-digit references of tests/ctheta_cases.py (the joint evaluator on
the tile-walk shapes, three steps of the class sampler, the joint's Langevin steps, the leapfrog
forward and back, and the HMC transitions) with the CPU-only measurements that go with them: the
high-precision side of tests/test_gpu_ctheta.py and tests/test_ctheta_cases.py.

    python tests/golden/make_ctheta_golden.py [processes]

Per entry `key` (ctheta_cases.key): key_digest (SHA-256 of the regenerated inputs), key_<name>_hi /
key_<name>_lo (hi float64 + lo float32; states at ctheta_cases.entry_select's entries), the plain
arrays accept, margin, H0 (hmc) and start (leapfrog: the doubles the back leapfrog starts from), and
key_meas (MEAS below).  Per family: u_family, the largest error of the fp64 restatements against the
references per quantity (ctheta_cases.FAMILIES), and bar_family = MARGIN·u.  The walk case
n = 330, N = 4100 is evaluated in long double (mpmath takes about 160 s for it); everything else is
mpmath.  Data only.  Two leapfrog passes: the back leapfrog's restatement needs the stored start, so
the measurements run after the references are written.
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import ctheta_cases as T  # noqa: E402

MEAS = ("seconds", "share", "cond", "fused", "literal")
PERTURBATIONS = 3


def _ref(e):
    t0 = time.time()
    packed = T.pack(e, T.compute(e))
    return T.key(e), T.digest(e), packed, time.time() - t0


def share(e):
    if e[0] == "cls":
        return min(T.cls_share(e[1], c) for c in range(len(T.CLS_CHAINS)))
    if e[0] == "lang":
        return T.lang_eps(e[1])[1]
    return float("nan")


def conditioning(e):
    base = T.run_numpy(e)
    return max(max(T.moves(e, base, T.run_numpy(e, perturb_seed=s)).values())
               for s in range(PERTURBATIONS))


def _measure(e):
    """(fused / vectorised errors, literal errors, conditioning) of a sampler entry."""
    ref = T.reference(e)
    if e[0] == "cls":
        a, b = T.errors(e, T.run_numpy(e), ref), T.errors(e, T.run_numpy(e, literal=True), ref)
    else:
        a = T.errors(e, T.run_numpy(e), ref)
        b = T.errors(e, T.run_numpy(e, pot=T.pot_literal), ref) if literal_too(e) else {}
    return a, b, conditioning(e)


def literal_too(e):
    """The literal form is left out of the 12-transition run (97 evaluations of it)."""
    return not (e[0] == "hmc" and e[4] > 3)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    t0 = time.time()
    cost = lambda e: -{"walk": 5, "hmc": 4, "leap": 2, "lang": 1, "cls": 1}[e[0]] * (  # noqa: E731
        1 if e[0] == "cls" else T.problem("w%d" % e[1] if e[0] == "walk" else e[1]).X.shape[0])
    entries = sorted(T.ENTRIES, key=cost)
    with multiprocessing.Pool(procs) as pool:
        refs = pool.map(_ref, entries, chunksize=1)
        out, secs = {}, {}
        for e, (k, dg, packed, sec) in zip(entries, refs):
            out[k + "_digest"] = np.array(dg)
            secs[e] = sec
            for s, a in packed.items():
                out[k + "_" + s] = a
        np.savez_compressed(T.GOLDEN, **out)
        T._stored.cache_clear()
        samplers = [e for e in entries if e[0] != "walk"]
        meas = pool.map(_measure, samplers, chunksize=1)
    u = {f: np.zeros(len(q)) for f, q in T.FAMILIES.items()}
    for e, (a, b, cond) in zip(samplers, meas):
        f = T.family(e)
        for i, q in enumerate(T.FAMILIES[f]):
            u[f][i] = max(u[f][i], a[q], b.get(q, 0.0) if f[0] != "w" else 0.0)
        m = dict(seconds=secs[e], share=share(e), cond=cond, fused=max(a.values()),
                 literal=max(b.values()) if b else float("nan"))
        out[T.key(e) + "_meas"] = np.array([m[k] for k in MEAS])
        print("%-28s %6.1f s  share %.2f  cond %.1e  restatements %s | %s"
              % (T.key(e), m["seconds"], m["share"], cond,
                 " ".join("%s %.1e" % kv for kv in a.items()),
                 " ".join("%s %.1e" % kv for kv in b.items())), flush=True)
    for e in entries:
        if e[0] == "walk":
            out[T.key(e) + "_meas"] = np.array([secs[e]] + [float("nan")] * (len(MEAS) - 1))
            print("%-28s %6.1f s" % (T.key(e), secs[e]))
    for f in T.FAMILIES:
        out["u_" + f] = u[f]
        out["bar_" + f] = T.MARGIN * u[f]
        print("%-8s %s  u = %s   B = %s" % (f, " ".join(T.FAMILIES[f]), " ".join("%.2e" % v for v in u[f]),
                                          " ".join("%.2e" % v for v in T.MARGIN * u[f])))
    out["seconds"] = np.array([time.time() - t0, sum(secs.values())])
    np.savez_compressed(T.GOLDEN, **out)
    print("%s: %d bytes, %.0f s (%.0f s of references)" % (T.GOLDEN, os.path.getsize(T.GOLDEN),
                                                          time.time() - t0, sum(secs.values())))


if __name__ == "__main__":
    main()
