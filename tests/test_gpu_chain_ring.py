"""What a row-staging schedule of the chain engine's batch loop has to keep (gpt_amd/csrc/chain.hip).
Written for the two-buffer staging ring of the J = 8, WV = 8 build: row group g of a batch in buffer
g & 1, group g + 2 issued behind group g's (b) phase, the second buffer laid over the waves'
post-batch scratch.  Whatever stages the rows, every double of a step is formed by the same
operations in the same order, so the stored samples are held bitwise to those recorded from the
library of the commit before the ring (tests/golden/chain_ring_parent.npz, written by
tests/golden/make_chain_ring_golden.py with GPTSGLD_LIB naming that build).

Problems are SC.make_problem on N = 2·m + tail rows with the step sizes of the existing REG case of
the same n (SC.inputs), two chains of different seeds, store_every = 1, seven steps: two full
batches, the ragged tail batch, the epoch boundary, and an end inside the third epoch.  A row group
is G = 2 batch rows; the shapes are the smallest that reach the ring's edges in the J = 8 wide build:

  (258, 5, 5, 100, 33, 5)   n = 258: six of the eight row blocks are padding; D = 5; r = 5, where the
                            post-batch scratch nearly fills its slice of the second buffer;
                            17 groups (odd >= 5), tail batch 3 groups
  (512, 8, 3, 120, 15, 4)   n = 512, D = 8, r = 3; 8 groups (even >= 4), tail batch 2 groups
  (258, 8, 5, 200, 4, 1)    2 groups per batch (no refill inside the loop), tail batch 1 group
  (512, 5, 4, 100, 2, 1)    1 group per batch (the second buffer never filled), r = 4

and two builds that keep one buffer or need no aliasing, from oracle/step_cases.py as they stand:

  (64, 4, 5, 30, 8, 1)      the WV = 4 build (D <= 4)
  (200, 5, 3, 70, 20, 7)    J = 4, WV = 8

What is held, bitwise:
  parent    run(7) stores the w of every step, the U of the last step and the SHA-256 of every
            (chain, step) U block that the parent's library stored, with status 0 (the digests keep
            the fixture under 1 MB: the full U of the n = 512, D = 8 case alone is 1.4 MB);
  chunks    seven run(1) and run(3); prepare(4); run(4) store what run(7) stores;
  diag      diagnostics on and off store the same samples.
"""
import functools
import hashlib
import os

import numpy as np
import pytest

from oracle import step_cases as SC

pytestmark = pytest.mark.gpu

RING_SHAPES = [(258, 5, 5, 100, 33, 5), (512, 8, 3, 120, 15, 4), (258, 8, 5, 200, 4, 1),
               (512, 5, 4, 100, 2, 1)]
CONTROL_SHAPES = [(64, 4, 5, 30, 8, 1), (200, 5, 3, 70, 20, 7)]
SHAPES = RING_SHAPES + CONTROL_SHAPES
# the existing REG case whose tuned step sizes a shape runs with: the one of the same n
STEP_SIZES_OF = {258: (258, 6, 4, 130, 15, 4), 512: (512, 8, 5, 256, 33, 5),
                 64: (64, 4, 5, 30, 8, 1), 200: (200, 5, 3, 70, 20, 7)}
SEEDS = [23, 1009]
STEPS = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_ring_parent.npz")


def step_case(shape):
    (c,) = [c for c in SC.CASES
            if c.family == SC.REG and c.shape == STEP_SIZES_OF[shape[0]] and c.epsU == 1e-6]
    return c


@functools.lru_cache(maxsize=None)
def problem(shape):
    import torch
    n, D, r, Q, m, tail = shape
    c = step_case(shape)
    p = SC.make_problem(n, D, 2 * m + tail, r, Q, seed=11 + 100 * c.seed)
    t = SC.inputs(c)
    phi = torch.from_numpy(np.ascontiguousarray(p["phi"].transpose(2, 1, 0))).cuda()
    return dict(phi=phi, y=torch.from_numpy(p["y"]).cuda(), I=p["I"], epsw=t["epsw"], epsU=t["epsU"],
                signal_var=t["signal_var"])


def run_chunks(shape, chunks, diag=False):
    """Stored (w, U) of both chains and their statuses after the given calls: an int n is run(n),
    ("prepare", n) is prepare(n)."""
    from gpt_amd.session import SGLDSession
    n, D, r, Q, m, tail = shape
    p = problem(shape)
    s = SGLDSession(p["phi"], p["y"], p["I"], r, Q, m, p["epsw"], p["epsU"], p["signal_var"], 0, 3,
                    SEEDS, store_every=1, max_steps=STEPS, diag=diag, engine="chain")
    assert s.info()["engine"] == "chain"
    for ch in chunks:
        if isinstance(ch, tuple):
            s.prepare(ch[1])
        else:
            s.run(ch)
    s.sync()
    done = s.steps_done
    out = [s.fetch(c) for c in range(len(SEEDS))]
    s.close()
    return dict(w=np.stack([o[0][:, :done] for o in out]), U=np.stack([o[1][..., :done] for o in out]),
                status=[o[2] for o in out], done=done)


@functools.lru_cache(maxsize=None)
def whole(shape):
    """run(7): the one reference of every comparison, left unchanged."""
    out = run_chunks(shape, [STEPS])
    for a in (out["w"], out["U"]):
        a.setflags(write=False)
    return out


def digests(U):
    """SHA-256 of every (chain, step) block of the stored U (chains, n, r, D, steps)."""
    return np.array([[hashlib.sha256(np.ascontiguousarray(U[c, ..., s]).tobytes()).hexdigest()
                      for s in range(U.shape[-1])] for c in range(U.shape[0])])


def key(shape):
    return "_".join(map(str, shape))


def same(a, b):
    assert a["done"] == b["done"] and a["status"] == b["status"]
    assert np.array_equal(a["w"], b["w"])
    assert np.array_equal(a["U"], b["U"])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parent_samples(shape):
    g = np.load(GOLDEN)
    out = whole(shape)
    assert out["done"] == STEPS and out["status"] == [0, 0]
    assert not np.array_equal(out["U"][0], out["U"][1])         # two seeds, two trajectories
    assert np.array_equal(out["w"], g["w_" + key(shape)])
    assert np.array_equal(out["U"][..., -1], g["Ulast_" + key(shape)])
    d, dg = digests(out["U"]), g["Usha_" + key(shape)]
    assert d.shape == dg.shape
    assert (d == dg).all(), "first U sample that differs (chain, step): %s" % (np.argwhere(d != dg)[0],)


@pytest.mark.parametrize("shape", RING_SHAPES, ids=str)
def test_chunk_invariance(shape):
    ref = whole(shape)
    for chunks in ([1] * STEPS, [3, ("prepare", 4), 4]):
        same(run_chunks(shape, chunks), ref)


@pytest.mark.parametrize("shape", RING_SHAPES, ids=str)
def test_diag_leaves_samples(shape):
    same(run_chunks(shape, [STEPS], diag=True), whole(shape))
