"""X mode (gpt_sgld_session_create_x / gpt_sgld_regression_chains_x): sessions that train from X,
with each minibatch's features staged on the device, against phi mode and against the oracle.

"phi mode" is the existing entry fed ``G().feature(X, ls_c, sigma_c, scale, Z, b)``.  The stager
forms each feature with feature_kernel's arithmetic and the same device cos, and the same engine
code reads the same doubles in the same order, so X mode equals phi mode exactly: the comparisons
are ``np.array_equal`` on every stored w and U plus equal status, and a non-zero status on either
side fails.  The oracle comparison (independent of the device features) holds the project's
trajectory bar, 1e-8 relative.
"""
import math

import numpy as np
import pytest

from oracle import gpt_sgld_ref as R

pytestmark = pytest.mark.gpu

SEEDS = [3, 4, 5]
# the order-ring test's setting: ragged last batch (nb = 4), seven epochs, the ring wraps
RING = dict(burnin=1, maxepoch=6, store_every=2, epsw=1e-4, epsU=1e-6)
SHAPES = {"grid": (25, 3, 29, 3, 10, 8), "chain": (24, 3, 29, 3, 10, 8),
          "wave": (24, 3, 29, 6, 10, 8)}


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def rel(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_problem(n, D, N, r, Q, seed=0):
    """tests/test_gpu_parity.py make_problem's recipe (without its oracle phi)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    Z = rng.standard_normal((n, D))
    b = 2 * np.pi * rng.random((n, D))
    ls = 1.0 + 0.2 * rng.standard_normal(D)
    scale = math.sqrt(n / Q ** (1.0 / D))
    phi = R.feature(X, ls, 1.0, scale, Z, b)
    I = R.samplenz(r, D, Q, seed + 1)
    w, U = R.init_state(n, r, D, Q, seed + 2)
    y = R.pred(w, U, I, phi) + 0.05 * rng.standard_normal(N)
    return dict(X=X, Z=Z, b=b, ls=ls, scale=scale, I=I, y=y)


def sweeps(D, seeds=SEEDS, scalar=False):
    """Per chain its own length scales (D of them, or one) and sigma_RBF."""
    ls, sg = [], []
    for c in seeds:
        g = np.random.default_rng(100 + c)
        ls.append(1.0 + 0.2 * g.standard_normal(1 if scalar else D))
        sg.append(1.0 + 0.1 * g.standard_normal())
    return np.array(ls), np.array(sg)


def device_phis(p, ls, sg):
    return [G().feature(p["X"], ls[c] if ls.shape[1] > 1 else float(ls[c, 0]), sg[c], p["scale"],
                        p["Z"], p["b"]) for c in range(len(sg))]


def assert_same(got, want):
    assert len(got) == len(want)
    for c, ((gw, gU, gs), (ww, wU, ws)) in enumerate(zip(got, want)):
        assert gs == 0 and ws == 0, (c, gs, ws)
        assert np.array_equal(gw, ww) and np.array_equal(gU, wU), (c, rel(gw, ww), rel(gU, wU))
        assert np.abs(ww).max() > 0 and np.abs(wU).max() > 0


def assert_chains_differ(res):
    for a in range(len(res)):
        for b in range(a + 1, len(res)):
            assert not np.array_equal(res[a][0], res[b][0])


# ----------------------------------------------------------------- 1. bitwise, per engine
@pytest.mark.parametrize("engine", ["grid", "chain", "wave"])
def test_x_mode_equals_phi_mode_bitwise(engine):
    n, D, N, r, Q, m = SHAPES[engine]
    p = make_problem(n, D, N, r, Q, seed=31)
    ls, sg = sweeps(D)
    phis = device_phis(p, ls, sg)
    a = (r, Q, m, RING["epsw"], RING["epsU"], RING["burnin"], RING["maxepoch"], SEEDS)
    want = G().GPTregression_chains(phis, p["y"], 0.05, p["I"], *a,
                                    store_every=RING["store_every"], engine=engine)
    got = G().GPTregression_chains_x(p["X"], p["y"], ls, sg, p["scale"], p["Z"], p["b"], 0.05,
                                     p["I"], *a, store_every=RING["store_every"], engine=engine)
    assert_same(got, want)
    assert_chains_differ(got)


# ----------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("engine,shape", [("wave", (40, 3, 40, 6, 30, 8)),
                                          ("chain", (64, 4, 40, 5, 30, 8))])
def test_x_mode_matches_oracle(engine, shape):
    """R.feature + R.GPTregression per chain: nothing of the device's features is on the
    reference side.  Seeds and step sizes of test_regression_chains_per_chain_phi_matches_oracle."""
    n, D, N, r, Q, m = shape
    p = make_problem(n, D, N, r, Q, seed=11)
    ls, sg = sweeps(D)
    got = G().GPTregression_chains_x(p["X"], p["y"], ls, sg, p["scale"], p["Z"], p["b"], 0.05,
                                     p["I"], r, Q, m, 1e-4, 1e-6, 0, 2, SEEDS, engine=engine)
    for c, sd in enumerate(SEEDS):
        phi = R.feature(p["X"], ls[c], sg[c], p["scale"], p["Z"], p["b"])
        wo, Uo, info = R.GPTregression(phi, p["y"], 0.05, p["I"], r, Q, m, 1e-4, 1e-6, 0, 2, sd)
        ws, Us, st = got[c]
        assert st == 0 and info["status"] == 0
        print("chain %d: rel w %.3e  rel U %.3e" % (c, rel(ws, wo), rel(Us, Uo)))
        assert rel(ws, wo) < 1e-8, (c, rel(ws, wo))
        assert rel(Us, Uo) < 1e-8, (c, rel(Us, Uo))


# ----------------------------------------------------------------- sessions
def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def phi_session(p, phis, shape, engine, **kw):
    from gpt_amd.session import SGLDSession
    n, D, N, r, Q, m = shape
    dphi = [to_dev(np.transpose(x, (2, 1, 0))) for x in phis]
    return SGLDSession(dphi, to_dev(p["y"]), p["I"], r, Q, m, RING["epsw"], RING["epsU"], 0.05,
                       RING["burnin"], RING["maxepoch"], SEEDS, store_every=RING["store_every"],
                       engine=engine, **kw)


def x_session(p, ls, sg, shape, engine, **kw):
    from gpt_amd.session import SGLDSession
    n, D, N, r, Q, m = shape
    return SGLDSession.from_X(p["X"], to_dev(p["y"]), ls, sg, p["scale"], p["Z"], p["b"], p["I"],
                              r, Q, m, RING["epsw"], RING["epsU"], 0.05, RING["burnin"],
                              RING["maxepoch"], SEEDS, store_every=RING["store_every"],
                              engine=engine, **kw)


def run_all(s, pieces=None, prepare=False):
    total = s.total_steps
    if prepare:
        s.prepare(total)
    for k in (pieces or []):
        s.run(k)
    s.run(total)                       # the rest (run() stops at total_steps)
    s.sync()
    assert s.steps_done == total
    out = [s.fetch(c) for c in range(s.nchains)]
    s.close()
    return out


# ----------------------------------------------------------------- 3. epoch longer than the span
def test_chain_engine_epoch_longer_than_span_cap():
    shape = (24, 3, 29, 3, 10, 3)                      # nb = 10
    n, D, N, r, Q, m = shape
    p = make_problem(n, D, N, r, Q, seed=33)
    ls, sg = sweeps(D)
    sx = x_session(p, ls, sg, shape, "chain")
    assert sx.info()["engine"] == "chain"
    KR = sx.staging()["slots"]
    assert sx.numbatches > KR - 1, (sx.numbatches, KR)  # a chain launch cannot cover the epoch
    got = run_all(sx)
    want = run_all(phi_session(p, device_phis(p, ls, sg), shape, "chain"))
    assert_same(got, want)
    assert_chains_differ(got)


# ----------------------------------------------------------------- 4. sessions run in pieces
@pytest.fixture(scope="module")
def pieces_ref():
    """Per engine: the problem and its phi-mode stores, computed once and left unchanged."""
    out = {}
    for engine in ("chain", "wave"):
        shape = SHAPES[engine]
        n, D, N, r, Q, m = shape
        p = make_problem(n, D, N, r, Q, seed=35)
        ls, sg = sweeps(D)
        phis = device_phis(p, ls, sg)
        out[engine] = (shape, p, ls, sg, phis, run_all(phi_session(p, phis, shape, engine)))
    return out


@pytest.mark.parametrize("engine", ["chain", "wave"])
def test_sessions_run_in_pieces(engine, pieces_ref):
    shape, p, ls, sg, phis, want = pieces_ref[engine]
    a = run_all(x_session(p, ls, sg, shape, engine), pieces=[3, 5])
    b = run_all(x_session(p, ls, sg, shape, engine), prepare=True)
    assert_same(a, want)
    assert_same(b, want)
    assert_same(a, b)


@pytest.mark.parametrize("engine", ["chain", "wave", "grid"])
def test_run_ending_mid_epoch(engine):
    """max_steps = nb + 1 ends one step into the second epoch: the third epoch's order is never
    built, and the lookahead must not stage from it."""
    shape = SHAPES[engine]
    n, D, N, r, Q, m = shape
    p = make_problem(n, D, N, r, Q, seed=35)
    ls, sg = sweeps(D)
    nb = -(-N // m)
    kw = dict(max_steps=nb + 1)
    sx = x_session(p, ls, sg, shape, engine, **kw)
    sp = phi_session(p, device_phis(p, ls, sg), shape, engine, **kw)
    assert sx.total_steps == nb + 1
    states = []
    for s in (sx, sp):
        s.run(s.total_steps)
        s.sync()
        st = [s.status(c) for c in range(s.nchains)]
        assert st == [0] * s.nchains
        import torch
        w = torch.empty((s.nchains, Q), dtype=torch.float64, device="cuda")
        U = torch.empty((s.nchains, n * r * D), dtype=torch.float64, device="cuda")
        s.gather_state(0, s.nchains, w, U)
        s.sync()
        states.append((w.cpu().numpy(), U.cpu().numpy()))
        s.close()
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    assert not np.array_equal(states[0][0][0], states[0][0][1])


# ----------------------------------------------------------------- 5. scalar length scale
def test_scalar_length_scale():
    shape = SHAPES["chain"]
    n, D, N, r, Q, m = shape
    p = make_problem(n, D, N, r, Q, seed=37)
    ls, sg = sweeps(D, scalar=True)
    assert ls.shape == (3, 1)
    phis = device_phis(p, ls, sg)
    a = (r, Q, m, 1e-4, 1e-6, 0, 2, SEEDS)
    want = G().GPTregression_chains(phis, p["y"], 0.05, p["I"], *a, engine="chain")
    got = G().GPTregression_chains_x(p["X"], p["y"], ls, sg, p["scale"], p["Z"], p["b"], 0.05,
                                     p["I"], *a, engine="chain")
    assert_same(got, want)
    assert_chains_differ(got)


# ----------------------------------------------------------------- 6. footprint
@pytest.mark.parametrize("engine", ["chain", "wave", "grid"])
def test_staging_footprint(engine):
    n, D, _, r, Q, m = SHAPES[engine]
    slots = []
    for N in (29, 290):
        shape = (n, D, N, r, Q, m)
        p = make_problem(n, D, N, r, Q, seed=39)
        ls, sg = sweeps(D)
        s = x_session(p, ls, sg, shape, engine)
        st = s.staging()
        s.close()
        assert st["xmode"] == 1
        KR = st["slots"]
        assert KR >= 2
        assert st["bytes_per_chain"] == KR * m * (8 * n * D + 8 + 4) + 4 * 2 * N
        slots.append(KR)
    assert slots[0] == slots[1]
    shape = (n, D, 29, r, Q, m)
    p = make_problem(n, D, 29, r, Q, seed=39)
    ls, sg = sweeps(D)
    s = phi_session(p, device_phis(p, ls, sg), shape, engine)
    st = s.staging()
    s.close()
    assert st["xmode"] == 0


# ----------------------------------------------------------------- 7. rejections
def test_rmsprop_rejected_on_x_session():
    from gpt_amd._lib import GPTError
    shape = SHAPES["grid"]
    n, D, N, r, Q, m = shape
    p = make_problem(n, D, N, r, Q, seed=41)
    ls, sg = sweeps(D)
    s = x_session(p, ls, sg, shape, "grid")
    with pytest.raises(GPTError):
        s.set_rmsprop(1e-4, 0.9)
    s.close()
