"""The callers of the session's launch loop (gpt_amd/csrc/api_session.hip session_launches) next to
gpt_sgld_session_run: gpt_sgld_session_time_steps, gpt_sgld_session_stamps and
gpt_sgld_session_timeline.  Each runs the same steps as run(), with events or diagnostics buffers
around the launches, so what it leaves behind must be run()'s, bit for bit: the gathered (w, U),
the status, steps_done and the fetched stores.

Sessions as in tests/test_gpu_chain_glue.py: the (64, 4, 5, 30, 8, 1) problem of
tests/test_gpu_chain_ahead.py (nb = 3, a one-row last batch), two seeds, a burn-in epoch and two
stored epochs, nine steps; the wave engine runs test_gpu_parity's wave shape (40, 3, 40, 6, 30, 8).
The X session is test_x_mode_span_four's: launches of at most four steps, where the stager's call
has to sit before the event pair and before the launch.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_chain_ahead as A
from test_gpu_chain_glue import final_state

pytestmark = pytest.mark.gpu

SHAPE = (64, 4, 5, 30, 8, 1)                    # (n, D, r, Q, m, tail): N = 2·m + tail
WAVE_SHAPE = (40, 3, 40, 6, 30, 8)              # (n, D, N, r, Q, m)
X_SHAPE = (24, 3, 29, 3, 10, 3)                 # nb = 10
SEEDS = A.SEEDS
STEPS = 9


def session(engine, total=STEPS):
    from gpt_amd.session import SGLDSession
    if engine == "wave":
        import torch
        import test_gpu_parity as P
        n, D, N, r, Q, m = WAVE_SHAPE
        p = P.make_problem(n, D, N, r, Q, seed=11)
        phi = torch.from_numpy(np.ascontiguousarray(p["phi"].transpose(2, 1, 0))).cuda()
        s = SGLDSession(phi, torch.from_numpy(p["y"]).cuda(), p["I"], r, Q, m, 1e-4, 1e-6, 0.05, 1,
                        2, SEEDS, max_steps=total, engine="wave")
    else:
        n, D, r, Q, m, tail = SHAPE
        p = A.problem(SHAPE)
        s = SGLDSession(p["phi"], p["y"], p["I"], r, Q, m, p["epsw"], p["epsU"], p["signal_var"], 1,
                        2, SEEDS, max_steps=total, engine=engine)
        assert s.numbatches == 3
    assert s.info()["engine"] == engine
    return s


def x_session(monkeypatch):
    import test_gpu_xmode as X
    monkeypatch.setenv("GPTSGLD_XSPAN", "4")
    n, D, N, r, Q, m = X_SHAPE
    p = X.make_problem(n, D, N, r, Q, seed=33)
    ls, sg = X.sweeps(D)
    s = X.x_session(p, ls, sg, X_SHAPE, "chain", max_steps=STEPS)
    assert s.info()["engine"] == "chain" and s.staging()["slots"] == 5 and s.numbatches == 10
    return s


def snapshot(s, done):
    """Everything a run leaves behind; closes the session."""
    s.sync()
    assert s.steps_done == done
    w, U, status = final_state(s)
    out = [s.fetch(c) for c in range(s.nchains)]
    s.close()
    assert [o[2] for o in out] == status
    return dict(w=w, U=U, status=status, ws=np.stack([o[0] for o in out]),
                Us=np.stack([o[1] for o in out]))


def same(a, b):
    assert a["status"] == b["status"] == [0] * len(a["status"])
    for k in ("w", "U", "ws", "Us"):
        assert np.isfinite(b[k]).all()
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(b["w"][0], b["w"][1])             # two seeds, two trajectories


@functools.lru_cache(maxsize=None)
def ran(engine, steps=STEPS):
    """run(steps) on a fresh session: the reference, left unchanged."""
    s = session(engine)
    s.run(steps)
    out = snapshot(s, steps)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def timed(s, calls):
    """The (kind, n) calls on s; every time_steps mean must be a finite positive time."""
    for kind, k in calls:
        if kind == "run":
            s.run(k)
        else:
            us = s.time_steps(k)
            assert np.isfinite(us) and us > 0, us


CALLS = [[("time", 9)], [("time", 4), ("run", 5)]]


@pytest.mark.parametrize("calls", CALLS, ids=["time9", "time4_run5"])
@pytest.mark.parametrize("engine", ["grid", "chain", "wave"])
def test_time_steps_leaves_what_run_leaves(engine, calls):
    s = session(engine)
    timed(s, calls)
    same(snapshot(s, STEPS), ran(engine))


def test_time_steps_on_an_x_session(monkeypatch):
    res = []
    for calls in [[("run", 9)]] + CALLS:
        s = x_session(monkeypatch)
        timed(s, calls)
        res.append(snapshot(s, STEPS))
    same(res[1], res[0])
    same(res[2], res[0])


def _stamps(s, nsteps):
    from gpt_amd import _lib
    out = np.zeros(nsteps * (s.D + 1) * s.nchains * 16, dtype=np.int64)
    return _lib.lib().gpt_sgld_session_stamps(s._h, nsteps, out.ctypes.data_as(C.POINTER(C.c_int64)))


def test_stamps_leave_what_run_leaves():
    from gpt_amd import _lib
    s = session("grid")
    assert _stamps(s, STEPS) == _lib.GPT_OK
    same(snapshot(s, STEPS), ran("grid"))


def test_stamps_rejected_on_an_x_session(monkeypatch):
    from gpt_amd import _lib
    s = x_session(monkeypatch)
    assert _stamps(s, STEPS) == _lib.GPT_ERR_BAD_DIMS
    assert s.steps_done == 0
    s.close()


def _timeline(s, nsteps):
    from gpt_amd import _lib
    out = np.zeros(s.nchains * _lib.lib().gpt_sgld_timeline_slots(), dtype=np.int64)
    us = C.c_double(0.0)
    return _lib.lib().gpt_sgld_session_timeline(s._h, nsteps, out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                C.byref(us))


def test_timeline_is_one_launch_of_the_epoch():
    from gpt_amd import _lib
    s = session("chain")
    assert _timeline(s, 4) == _lib.GPT_ERR_BAD_DIMS             # crosses the epoch's end at nb = 3
    assert s.steps_done == 0
    assert _timeline(s, 2) == _lib.GPT_OK
    same(snapshot(s, 2), ran("chain", 2))


def test_timeline_rejected_on_the_grid_engine():
    from gpt_amd import _lib
    s = session("grid")
    assert _timeline(s, 2) == _lib.GPT_ERR_BAD_DIMS
    assert s.steps_done == 0
    s.close()
