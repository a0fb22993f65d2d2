"""CPU tests of the tensor-sampler session's boundary (gpt_sgld_session_create and the host samplers
on top of it): every argument error is GPT_ERR_BAD_DIMS before any device call, the engine requests
a shape cannot serve included, and the Python wrappers' own checks and step counts.

The device pointers of the raw calls are host addresses: the checks must reject the call before
anything reads through them.
"""
import ctypes as C

import numpy as np
import pytest

n, D, N, r, Q, m = 24, 3, 29, 3, 10, 8
STORE, CHAIN, SPLIT, WAVE = 1, 8, 64, 128       # store_flags bits (include/gptsgld.h)


def _problem(shape=(n, D, N, r, Q, m)):
    from gpt_amd import GPT_SGLD as G
    n_, D_, N_, r_, Q_, m_ = shape
    rng = np.random.default_rng(7)
    return dict(phi=np.asfortranarray(rng.standard_normal((n_, D_, N_))), y=rng.standard_normal(N_),
                I=G.samplenz(r_, D_, Q_, 1),
                cfg=G.make_config(n_, D_, N_, r_, Q_, m_, 1e-4, 1e-6, 0.05, 1.0, 0, 1, 0))


def _create(p, nch=2, flags=STORE, out=True, **null):
    """Raw gpt_sgld_session_create call -> (return code, last error); the arguments named in `null`
    are passed as NULL.  The handle stays null."""
    from gpt_amd import _lib
    k = max(nch, 1)
    seeds = np.arange(1, k + 1, dtype=np.uint64)
    phis = (C.c_void_p * k)(*[p["phi"].ctypes.data] * k)
    ys = (C.c_void_p * k)(*[p["y"].ctypes.data] * k)
    h = C.c_void_p()
    rc = _lib.lib().gpt_sgld_session_create(
        C.byref(p["cfg"]), nch, None if null.get("seeds") else seeds.ctypes.data_as(_lib.P_U64),
        None if null.get("phi") else phis, ys, p["I"].ctypes.data_as(_lib.P_I32), flags, None,
        C.byref(h) if out else None)
    assert h.value is None
    return rc, _lib.lib().gpt_last_error().decode(errors="replace")


def test_null_out():
    from gpt_amd import _lib
    assert _create(_problem(), out=False)[0] == _lib.GPT_ERR_BAD_DIMS


@pytest.mark.parametrize("bad", [dict(nch=0), dict(seeds=True), dict(phi=True)],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_chain_arguments(bad):
    from gpt_amd import _lib
    assert _create(_problem(), **bad)[0] == _lib.GPT_ERR_BAD_DIMS


@pytest.mark.parametrize("entry", [0, r + 1])
def test_core_index_outside_its_range(entry):
    from gpt_amd import _lib
    p = _problem()
    p["I"][Q // 2, D - 1] = entry
    assert _create(p)[0] == _lib.GPT_ERR_BAD_DIMS


@pytest.mark.parametrize("shape,flag,text", [
    ((n, D, N, r, Q, m), SPLIT, "split engine"),
    ((n, D, N, r, Q, m), WAVE, "wave engine does not support"),
    ((40, 3, N, 6, 30, 8), CHAIN, "chain engine does not support"),
], ids=["split", "wave", "chain"])
def test_engine_request_the_shape_cannot_serve(shape, flag, text):
    from gpt_amd import _lib
    rc, msg = _create(_problem(shape), flags=STORE | flag)
    assert rc == _lib.GPT_ERR_BAD_DIMS, (rc, msg)
    assert text in msg, msg


def test_split_engine_in_the_environment(monkeypatch):
    from gpt_amd import _lib
    monkeypatch.setenv("GPTSGLD_ENGINE", "split")
    rc, msg = _create(_problem())
    assert rc == _lib.GPT_ERR_BAD_DIMS, (rc, msg)
    assert "split engine" in msg, msg


def _host_sampler(name, p, *lead):
    from gpt_amd import _lib
    ws = np.zeros((Q, -(-N // m)), order="F")
    ptr = lambda a: a.ctypes.data_as(_lib.P_D)
    return getattr(_lib.lib(), name)(C.byref(p["cfg"]), *lead, ptr(p["phi"]), ptr(p["y"]),
                                     p["I"].ctypes.data_as(_lib.P_I32), None, None, ptr(ws), None, None)


def test_rmsprop_needs_a_positive_epsilon():
    from gpt_amd import _lib
    assert _host_sampler("gpt_sgld_rmsprop", _problem(), 0.0, 0.9) == _lib.GPT_ERR_BAD_DIMS


def test_wonly_needs_the_stiefel_path():
    from gpt_amd import _lib
    p = _problem()
    p["cfg"].stiefel = 0
    assert _host_sampler("gpt_sgld_wonly", p) == _lib.GPT_ERR_BAD_DIMS


# ----------------------------------------------------------------- the Python wrappers
def test_wrappers_reject_disagreeing_inputs():
    from gpt_amd import GPT_SGLD as G
    p = _problem()
    phi, y, I = p["phi"], p["y"], p["I"]
    a = (r, Q, m, 1e-4, 1e-6, 0, 1)
    with pytest.raises(ValueError, match="phi and y disagree on N"):
        G.GPTregression(phi, y[:-1], 0.05, I, *a)
    with pytest.raises(ValueError, match=r"I must be \(Q, D\)"):
        G.GPTregression(phi, y, 0.05, I[:-1], *a)
    with pytest.raises(ValueError, match="every phi must have the same"):
        G.GPTregression_chains([phi, phi[:, :, :-1]], y, 0.05, I, *a, [1, 2])
    with pytest.raises(ValueError, match="one phi per chain, or one shared phi"):
        G.GPTregression_chains([phi, phi], y, 0.05, I, *a, [1, 2, 3])
    with pytest.raises(ValueError, match="phi and y disagree on N"):
        G.GPTregression_chains(phi, y[:-1], 0.05, I, *a, [1, 2])
    with pytest.raises(ValueError, match="phi and y disagree on N"):
        G.GPT_SGLDERMw(phi, y[:-1], 0.05, I, r, Q, m, 1e-4, 0, 1)
    with pytest.raises(ValueError, match=r"I must be \(Q, D\)"):
        G.GPT_SGLDERMw(phi, y, 0.05, I[:, :-1], r, Q, m, 1e-4, 0, 1)
    with pytest.raises(ValueError, match="phi and y disagree on N"):
        G.GPT_GMC(phi, y[:-1], 0.05, I, r, Q, 1e-3, 1e-3, 0, 1, 2)
    with pytest.raises(ValueError, match=r"I must be \(Q, D\)"):
        G.GPT_GMC(phi, y, 0.05, I[:-1], r, Q, 1e-3, 1e-3, 0, 1, 2)


@pytest.mark.parametrize("N_,m_", [(29, 8), (16, 8), (1, 8)])
@pytest.mark.parametrize("store_every", [1, 3])
@pytest.mark.parametrize("max_steps", [0, 5])
def test_run_counts(N_, m_, store_every, max_steps):
    from gpt_amd.GPT_SGLD import _run_counts
    burnin, maxepoch = 1, 2
    nb = (N_ + m_ - 1) // m_
    total = (burnin + maxepoch) * nb
    want = (nb, min(total, max_steps) if max_steps > 0 else total, maxepoch * nb // store_every)
    assert _run_counts(N_, m_, burnin, maxepoch, store_every, max_steps) == want
    assert _run_counts(N_, m_, burnin, maxepoch) == (nb, total, maxepoch * nb)
