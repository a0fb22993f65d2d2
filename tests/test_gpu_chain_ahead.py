"""What a chain-engine step order that carries state from one step into the next has to keep
(gpt_amd/csrc/chain.hip, WV = 8 build).  Written for the draw-ahead of the U noise (waves k >= 4
drawing ξ(t + 1) at the end of step t into the gradient accumulator of step t + 1), which was
measured and not merged; the kernel as it is passes all of it, and a later
attempt has to.

Shapes, inputs and step sizes are those of oracle/step_cases.py, the smallest at which the WV = 8
kernel's edges show: D = 5 (a single wave with a SIMD partner), D = 6, and D = 8 with n and Q at
their maxima.  The sessions train on N = 2·m + tail rows, two chains of different seeds,
store_every = 1: seven steps pass two full batches, the ragged last batch, the epoch boundary, and
end inside the third epoch.  What is held:

  chunks    run(7), seven run(1), and run(3); prepare(4); run(4) store bitwise-equal w and U and
            equal status: a sample does not depend on how steps are split into launches and graphs;
  ending    a launch that ends on the chain's last step (total_steps = 7) and launches that end
            mid-epoch (total_steps = 9: run(5), run(4)) store the same first seven samples, and the
            nine samples of run(5); run(4) are those of run(9);
  diag      diagnostics on and off store bitwise-equal w and U, and the gradient norms of the
            three-step cases stay within SC.bars() of the mpmath reference SC.reference(c) (the
            yardstick of tests/test_gpu_step.py, reused);
  control   the D <= 4 case (64, 4, 5, 30, 8, 1) runs the WV = 4 build (one wave per SIMD): its
            samples are those recorded from the library before this file's commit
            (tests/golden/chain_ahead_control.npz, written by make_chain_ahead_golden.py).
"""
import functools
import os

import numpy as np
import pytest

from oracle import step_cases as SC

pytestmark = pytest.mark.gpu

SHAPES = [(200, 5, 3, 70, 20, 7), (258, 6, 4, 130, 15, 4), (512, 8, 5, 256, 33, 5)]
CONTROL = (64, 4, 5, 30, 8, 1)
SEEDS = [23, 1009]
STEPS = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_ahead_control.npz")


def case(shape):
    (c,) = [c for c in SC.CASES if c.family == SC.REG and c.shape == shape and c.epsU == 1e-6]
    return c


@functools.lru_cache(maxsize=None)
def problem(shape):
    """The case's generator and tuned step sizes on N = 2·m + tail rows, on the device."""
    import torch
    c = case(shape)
    n, D, r, Q, m, tail = shape
    p = SC.make_problem(n, D, 2 * m + tail, r, Q, seed=11 + 100 * c.seed)
    t = SC.inputs(c)
    phi = torch.from_numpy(np.ascontiguousarray(p["phi"].transpose(2, 1, 0))).cuda()
    return dict(phi=phi, y=torch.from_numpy(p["y"]).cuda(), I=p["I"], epsw=t["epsw"], epsU=t["epsU"],
                signal_var=t["signal_var"])


def run_chunks(shape, chunks, total=STEPS, diag=False):
    """Stored (w, U) of both chains, their statuses and the diagnostics after the given calls:
    an int n is run(n), ("prepare", n) is prepare(n)."""
    from gpt_amd.session import SGLDSession
    n, D, r, Q, m, tail = shape
    p = problem(shape)
    s = SGLDSession(p["phi"], p["y"], p["I"], r, Q, m, p["epsw"], p["epsU"], p["signal_var"], 0, 3,
                    SEEDS, store_every=1, max_steps=total, diag=diag, engine="chain")
    assert s.info()["engine"] == "chain"
    for ch in chunks:
        if isinstance(ch, tuple):
            s.prepare(ch[1])
        else:
            s.run(ch)
    s.sync()
    done = s.steps_done
    out = [s.fetch(c, diag=diag) for c in range(len(SEEDS))]
    s.close()
    return dict(w=np.stack([o[0][:, :done] for o in out]), U=np.stack([o[1][..., :done] for o in out]),
                status=[o[2] for o in out], diag=np.stack([o[3][:, :done] for o in out]) if diag else None,
                done=done)


@functools.lru_cache(maxsize=None)
def whole(shape):
    """run(7) of a seven-step chain: the one reference of every comparison, left unchanged."""
    out = run_chunks(shape, [STEPS])
    assert out["done"] == STEPS and out["status"] == [0, 0]
    assert np.isfinite(out["w"]).all() and np.isfinite(out["U"]).all()
    assert not np.array_equal(out["U"][0], out["U"][1])         # two seeds, two trajectories
    for a in (out["w"], out["U"]):
        a.setflags(write=False)
    return out


def same(a, b, steps=None):
    sl = slice(None) if steps is None else slice(0, steps)
    assert a["status"] == b["status"]
    assert np.array_equal(a["w"][..., sl], b["w"][..., sl])
    assert np.array_equal(a["U"][..., sl], b["U"][..., sl])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_chunk_invariance(shape):
    ref = whole(shape)
    for chunks in ([1] * STEPS, [3, ("prepare", 4), 4]):
        out = run_chunks(shape, chunks)
        assert out["done"] == STEPS
        same(out, ref)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_launch_ending(shape):
    """total_steps = 7: the launch of `whole` ends on the chain's last step.  total_steps = 9: run(5)
    ends mid-epoch, run(4) on the last step; run(9) passes both points inside one call."""
    ref = whole(shape)
    split = run_chunks(shape, [5, 4], total=9)
    assert split["done"] == 9
    same(split, ref, STEPS)
    same(run_chunks(shape, [9], total=9), split)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_diag_leaves_samples(shape):
    out = run_chunks(shape, [STEPS], diag=True)
    same(out, whole(shape))
    assert np.isfinite(out["diag"]).all() and (out["diag"] > 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_diag_norms_against_mpmath(shape):
    """The three steps of tests/test_gpu_step.py on the chain engine (injected initial state, diag
    on): every gradient norm within SC.bars() of the 50-digit reference."""
    from gpt_amd import GPT_SGLD as G
    c = case(shape)
    n, D, r, Q, m, tail = shape
    p = SC.inputs(c)
    ws, Us, dg = G.GPTregression(p["phi"], p["y"], p["signal_var"], p["I"], r, Q, m, p["epsw"],
                                 p["epsU"], 0, 2, SC.RUN_SEED, max_steps=SC.STEPS, engine="chain",
                                 w_init=p["w0"], U_init=p["U0"], diag=True)
    out = SC.standard(ws, Us, dg.T)
    err, B = SC.rel_err(out, SC.reference(c), SC.on_manifold(c)), SC.bars()[c.family]
    print("%s: worst / B: %s" % (SC.case_id(c), "  ".join(
        "%s %.3f (%.2e)" % (q, err[q] / B[q], err[q]) for q in SC.QUANTITIES if q in err)))
    assert np.isfinite(out["norms"]).all()
    assert err["norms"] <= B["norms"], (err["norms"], B["norms"])


def test_control_wv4_build_unchanged():
    g = np.load(GOLDEN)
    out = run_chunks(CONTROL, [STEPS])
    assert out["status"] == [0, 0]
    assert np.array_equal(out["w"], g["w"]) and np.array_equal(out["U"], g["U"])
