"""bench.py's plain line, its --full line and --dump-outputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
                 "warmup", "n_gpus", "config", "roofline"}
FULL_ONLY_KEYS = {"cpu_baseline", "test_rmse", "quality", "pred", "single_chain", "allreduce_ms"}


def _timed_namespace():
    args = types.SimpleNamespace(workload="kin40k", steps=20, warmup=5, epsw=1e-5, epsU=1e-8,
                                 signal_var=0.0476)
    return dict(args=args, value=2.9e6, world=1, world_seen=1, warm_ms=1000.0, ms_per_step=0.088,
                wdesc="kin40k", N=10000, Nte=30000, D=8, n=500, r=5, Q=200, m=50, C=256, alive=256,
                info=dict(engine="chain", workgroups=256, threads=512, lds_bytes=73600),
                roof={"bound": "hbm", "achieved": 5800.0, "peak": 8000.0, "unit": "GB/s",
                      "frac": 0.72}, traffic=4.2e8, traffic_src="t", k_us=85.2, k_us_ranks=[85.2],
                dataset="kin40k", bytes_launch=4.94e8, host_us={}, steps_run=1025)


def test_plain_line_is_the_headline_of_the_full_line():
    """A plain run's line has the headline fields with the meaning of the --full line, and none of
    the fields whose legs take runs of their own."""
    import bench
    timed = _timed_namespace()
    plain = bench.headline(types.SimpleNamespace(**timed))
    full = bench.compose_line(types.SimpleNamespace(
        cpu=dict(value=17000.0, cores=16, kind="port"), quality=dict(test_rmse=0.28, note="x"),
        allreduce_ms=0.05, npred=256, pred_ms=6.9, pred_flop=3.07e11, gemm_ms=5.4, vphase_ms=1.0,
        rmse_final=0.28, vphase_kernel="pred_vphase_pairs_kernel",
        single=dict(steps_per_s=2e4, kernel_us=50.0), **timed))
    assert HEADLINE_KEYS <= set(plain) and not FULL_ONLY_KEYS & set(plain)
    assert FULL_ONLY_KEYS <= set(full)
    assert all(full[k] == plain[k] for k in plain)
    assert plain["metric"] == bench.METRICS["kin40k"] and plain["unit"] == "chain-steps/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["ms_per_step"] == 0.088 and plain["steps"] == 20 and plain["warmup"] == 5
    json.dumps(plain)


def test_dump_outputs_writes_float64_npy(tmp_path):
    import bench
    w = np.arange(12, dtype=np.float32).reshape(3, 4)
    U = np.linspace(0.0, 1.0, 30).reshape(3, 10)
    bench.dump_outputs(str(tmp_path / "d"), {"w": w, "U": U})
    assert sorted(os.listdir(tmp_path / "d")) == ["U.npy", "w.npy"]
    gw, gU = np.load(tmp_path / "d" / "w.npy"), np.load(tmp_path / "d" / "U.npy")
    assert gw.dtype == np.float64 and gU.dtype == np.float64
    assert np.array_equal(gw, w) and np.array_equal(gU, U)


def test_dump_outputs_over_the_limit_is_a_fixed_sample(tmp_path):
    """Past the byte limit every array is cut to the same seeded sample of its elements: the
    files fit the limit, and two dumps hold the same elements of their arrays."""
    import bench
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((50, 40)), rng.standard_normal(500)
    limit = 8192
    for d, shift in (("x", 0.0), ("y", 1.0)):
        bench.dump_outputs(str(tmp_path / d), {"a": a + shift, "b": b + shift}, limit=limit)
    size = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert size <= limit
    xa, ya = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "y" / "a.npy")
    xb = np.load(tmp_path / "x" / "b.npy")
    assert 0 < xa.size < a.size and 0 < xb.size < b.size
    assert np.array_equal(ya, xa + 1.0)                  # the same elements in both dumps
    assert np.isin(xa, a).all() and np.isin(xb, b).all()
    assert abs(xa.size / a.size - xb.size / b.size) < 0.01


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_chains_state(tmp_path):
    """`bench.py --dump-outputs` at a tiny setting: the plain line, and (w, U) of every chain after
    warmup + steps steps equal to a session of the same chains stepped the same number of times."""
    import math
    import torch
    import bench
    from gpt_amd import GPT_SGLD as G
    from gpt_amd.session import SGLDSession, feature_device
    C, steps, warmup = 3, 4, 2
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--chains", str(C), "--epochs", "1",
                        "--clock-warm-ms", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert HEADLINE_KEYS <= set(line) and not FULL_ONLY_KEYS & set(line)
    assert line["steps"] == steps and line["ms_per_step"] > 0
    # ms_per_step is the time of one timed step of all C chains
    assert line["value"] == pytest.approx(C / (line["ms_per_step"] * 1e-3), rel=1e-9)
    w, U, st = (np.load(out / (k + ".npy")) for k in ("w", "U", "status"))
    _, D, m, ls, srbf, sv, _, n, r, epsw, epsU = bench.WORKLOADS["kin40k"]
    Q = 200
    assert w.dtype == U.dtype == np.float64
    assert w.shape == (C, Q) and U.shape == (C, n * r * D) and not st.any()

    dev = torch.device("cuda", 0)
    Xtr, ytr, _, _, _ = bench.kin40k(D)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z, b = G.feature_inputs(n, D, 17)
    phi = feature_device(tt(Xtr.T), tt(np.array(ls)), srbf, math.sqrt(n / Q ** (1.0 / D)),
                         tt(Z.T), tt(b.T))
    y = tt(ytr)
    nb = -(-Xtr.shape[0] // m)
    # the kernels sum in a fixed order without atomics, so the same chains stepped the same way
    # give the same bits
    sess = SGLDSession(phi, y, G.samplenz(r, D, Q, 17), r, Q, m, epsw, epsU, sv, 0, 2,
                       bench.chain_seeds(0, C), store_every=nb, store=True)
    sess.run(warmup)
    sess.prepare(steps)
    sess.run(steps)
    w2 = torch.empty((C, Q), dtype=torch.float64, device=dev)
    U2 = torch.empty((C, n * r * D), dtype=torch.float64, device=dev)
    sess.gather_state(0, C, w2, U2)
    sess.sync()
    sess.close()
    assert np.array_equal(w, w2.cpu().numpy()) and np.array_equal(U, U2.cpu().numpy())
