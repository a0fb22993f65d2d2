"""The chain engine's step bookkeeping (gpt_amd/csrc/chain.hip): the batch position and the store
schedule are carried from step to step instead of divided out of the step counter, the row indices
of the batch after next arrive by LDS-DMA in a second index slot, the next targets are gathered
across the w update, and the U write-back sits behind one uniform guard.  None of it may change a
sample, and none of it may depend on how steps are split into launches.

Sessions as in tests/test_gpu_chain_ahead.py: oracle/step_cases.py problems on N = 2·m + tail rows
(nb = 3, the last batch ragged), two chains of different seeds.  Shapes:

  (200, 5, 3, 70, 20, 7)    one wave with a SIMD partner;
  (512, 8, 5, 256, 33, 5)   the maxima, m odd: the index DMA of the second batch starts 4-byte
                            aligned only;
  (64, 4, 5, 30, 8, 1)      the WV = 4 build, J = 1, a one-row tail (the first-row staging of the
                            last batch has fewer rows than a group).

What is held, everything bitwise:

  schedule  burn-in of one epoch, store_every in {1, 2, 3, nb}, nine steps (two epoch ends and the
            ragged batch inside): the nstore samples stored at store_every = s are samples
            s, 2s, .. of the store_every = 1 run, whether the steps run as run(9), run(4); run(5)
            or nine run(1);
  state     gather_state and status after each of these splits equal the unsplit run's (the
            launch-end write of U and w);
  parent    the final (w, U, status) after seven steps of the first and the third shape are those
            of the library before this change (tests/golden/chain_glue_parent.npz, written by
            tests/golden/make_chain_glue_golden.py);
  x mode    a chain session built from X with four steps per launch at most, nine steps in one
            call, equals the same session run one step per call.
"""
import functools
import os

import numpy as np
import pytest

import test_gpu_chain_ahead as A

pytestmark = pytest.mark.gpu

SHAPES = [(200, 5, 3, 70, 20, 7), (512, 8, 5, 256, 33, 5), (64, 4, 5, 30, 8, 1)]
PARENT_SHAPES = [SHAPES[0], SHAPES[2]]
SEEDS = A.SEEDS
NB = 3                              # N = 2·m + tail
STEPS = 9                           # burn-in epoch + two stored epochs
SPLITS = [[9], [4, 5], [1] * 9]
PARENT_STEPS = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_glue_parent.npz")


def final_state(s):
    """(w, U, status) of every chain as the session holds them now."""
    import torch
    w = torch.empty((s.nchains, s.Q), dtype=torch.float64, device="cuda")
    U = torch.empty((s.nchains, s.n * s.r * s.D), dtype=torch.float64, device="cuda")
    s.gather_state(0, s.nchains, w, U)
    s.sync()
    return w.cpu().numpy(), U.cpu().numpy(), [s.status(c) for c in range(s.nchains)]


def run_split(shape, store_every, chunks, burnin=1, maxepoch=2, total=STEPS):
    from gpt_amd.session import SGLDSession
    n, D, r, Q, m, tail = shape
    p = A.problem(shape)
    s = SGLDSession(p["phi"], p["y"], p["I"], r, Q, m, p["epsw"], p["epsU"], p["signal_var"], burnin,
                    maxepoch, SEEDS, store_every=store_every, max_steps=total, engine="chain")
    assert s.info()["engine"] == "chain" and s.numbatches == NB
    for ch in chunks:
        s.run(ch)
    s.sync()
    assert s.steps_done == total
    gw, gU, status = final_state(s)
    out = [s.fetch(c) for c in range(len(SEEDS))]
    nstore = s.nstore
    s.close()
    assert [o[2] for o in out] == status
    return dict(w=np.stack([o[0] for o in out]), U=np.stack([o[1] for o in out]), status=status,
                gw=gw, gU=gU, nstore=nstore)


@functools.lru_cache(maxsize=None)
def whole(shape, store_every):
    """run(9) at this store_every: the reference of the split runs, left unchanged."""
    out = run_split(shape, store_every, [STEPS])
    assert out["status"] == [0, 0]
    for a in (out["w"], out["U"], out["gw"], out["gU"]):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    assert not np.array_equal(out["gU"][0], out["gU"][1])       # two seeds, two trajectories
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_store_schedule(shape):
    every = whole(shape, 1)
    stored = STEPS - NB                                         # steps after the burn-in epoch
    assert every["nstore"] == stored and every["w"].shape[-1] == stored
    # every sample is a step of its own: no slot written twice or left at its zero fill
    for k in range(stored):
        assert np.abs(every["w"][..., k]).max() > 0
        assert k == 0 or not np.array_equal(every["w"][..., k], every["w"][..., k - 1])
    # the last sample is the state the launch left behind
    assert np.array_equal(every["w"][..., -1], every["gw"])
    assert np.array_equal(every["U"][..., -1].reshape(len(SEEDS), -1, order="F"), every["gU"])
    for s in sorted({1, 2, 3, NB}):
        for chunks in SPLITS:
            out = whole(shape, s) if chunks == [STEPS] else run_split(shape, s, chunks)
            assert out["status"] == every["status"]
            assert out["nstore"] == stored // s and out["w"].shape[-1] == stored // s
            assert np.array_equal(out["w"], every["w"][..., s - 1::s][..., :stored // s]), (s, chunks)
            assert np.array_equal(out["U"], every["U"][..., s - 1::s][..., :stored // s]), (s, chunks)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_state_after_split_launches(shape):
    for s in (1, NB):
        ref = whole(shape, s)
        for chunks in SPLITS[1:]:
            out = run_split(shape, s, chunks)
            assert out["status"] == ref["status"]
            assert np.array_equal(out["gw"], ref["gw"]), (s, chunks)
            assert np.array_equal(out["gU"], ref["gU"]), (s, chunks)


def parent_run(shape):
    """Seven steps in one call, no burn-in (ends inside the third epoch): the final state."""
    out = run_split(shape, 1, [PARENT_STEPS], burnin=0, maxepoch=3, total=PARENT_STEPS)
    return out["gw"], out["gU"], np.array(out["status"], dtype=np.int32)


@pytest.mark.parametrize("shape", PARENT_SHAPES, ids=str)
def test_parent_final_state(shape):
    g = np.load(GOLDEN)
    key = "_".join(map(str, shape))
    w, U, status = parent_run(shape)
    assert np.array_equal(status, g["status_" + key]) and not status.any()
    assert np.array_equal(w, g["w_" + key])
    assert np.array_equal(U, g["U_" + key])


def test_x_mode_span_four(monkeypatch):
    """An X session whose launches stop after four steps (ring of five batch slots), inside one
    epoch of ten batches: run(9) is launches of 4, 4 and 1 steps."""
    import test_gpu_xmode as X
    monkeypatch.setenv("GPTSGLD_XSPAN", "4")
    shape = (24, 3, 29, 3, 10, 3)                               # nb = 10
    n, D, N, r, Q, m = shape
    p = X.make_problem(n, D, N, r, Q, seed=33)
    ls, sg = X.sweeps(D)
    res = []
    for chunks in ([9], [1] * 9):
        s = X.x_session(p, ls, sg, shape, "chain", max_steps=9)
        assert s.info()["engine"] == "chain" and s.staging()["slots"] == 5 and s.numbatches == 10
        for ch in chunks:
            s.run(ch)
        s.sync()
        assert s.steps_done == 9
        res.append(final_state(s))
        s.close()
    (w9, U9, st9), (w1, U1, st1) = res
    assert st9 == st1 == [0] * len(X.SEEDS)
    assert np.isfinite(w9).all() and np.isfinite(U9).all()
    assert np.array_equal(w9, w1) and np.array_equal(U9, U1)
    assert not np.array_equal(w9[0], w9[1])
