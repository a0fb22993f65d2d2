"""Seeds above 2^32, end to end.  The Philox key's second word is seed >> 32; a seed narrowed to 32
bits anywhere on its way (a params struct, a ctypes signature, a kernel argument) would make chains
share streams in silence.  One small shape per path, run under SEED = (0x299f31d0 << 32) |
0xa4093822 and under its low word alone: each run matches the oracle under the same seed at the
path's existing bar, and the two runs differ.  (The host-only draws are in tests/test_capi.py, the
Philox words themselves in tests/test_gpu_fastmath.py.)"""
import functools
import math

import numpy as np
import pytest

from oracle import gpt_sgld_ref as R
from oracle.fastmath_cases import BIG_SEED as SEED

pytestmark = pytest.mark.gpu
LOW = SEED & 0xFFFFFFFF
SEEDS = [SEED, LOW]


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def rel(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ------------------------------------------------------------------------------ sampler engines
# the "small" and "w_r6_d3" shapes of tests/test_gpu_parity.py: (n, D, N, r, Q, m, burnin, maxepoch)
PHI_SHAPES = {"grid": (16, 3, 40, 2, 6, 8, 1, 2), "chain": (16, 3, 40, 2, 6, 8, 1, 2),
              "wave": (40, 3, 70, 6, 30, 16, 0, 2)}
# the shapes of tests/test_gpu_xmode.py: (n, D, N, r, Q, m)
X_SHAPES = {"grid": (25, 3, 29, 3, 10, 8), "chain": (24, 3, 29, 3, 10, 8), "wave": (24, 3, 29, 6, 10, 8)}
EPSW, EPSU, SV = 1e-4, 1e-6, 0.05


@functools.lru_cache(maxsize=None)
def phi_problem(shape):
    from test_gpu_parity import make_problem
    n, D, N, r, Q, m, burnin, maxepoch = shape
    return make_problem(n, D, N, r, Q, seed=11)


@functools.lru_cache(maxsize=None)
def phi_oracle(shape, seed):
    """Computed once per (shape, seed), shared by the engines, left unchanged."""
    n, D, N, r, Q, m, burnin, maxepoch = shape
    p = phi_problem(shape)
    wo, Uo, info = R.GPTregression(p["phi"], p["y"], SV, p["I"], r, Q, m, EPSW, EPSU, burnin,
                                   maxepoch, seed, record=True)
    assert info["status"] == 0
    return wo, Uo


@pytest.mark.parametrize("engine", ["grid", "chain", "wave"])
def test_phi_sessions_take_the_whole_seed(engine):
    """The seed in gpt_sgld_config (gpt_sgld_regression) and in the seeds array
    (gpt_sgld_regression_chains)."""
    shape = PHI_SHAPES[engine]
    n, D, N, r, Q, m, burnin, maxepoch = shape
    p = phi_problem(shape)
    single = [G().GPTregression(p["phi"], p["y"], SV, p["I"], r, Q, m, EPSW, EPSU, burnin, maxepoch,
                                s, engine=engine) for s in SEEDS]
    chains = G().GPTregression_chains(p["phi"], p["y"], SV, p["I"], r, Q, m, EPSW, EPSU, burnin,
                                      maxepoch, SEEDS, engine=engine)
    for c, s in enumerate(SEEDS):
        wo, Uo = phi_oracle(shape, s)
        assert chains[c][2] == 0
        for ws, Us in (single[c], chains[c][:2]):
            assert rel(ws, wo) < 1e-8, (c, rel(ws, wo))
            assert rel(Us, Uo) < 1e-8, (c, rel(Us, Uo))
    assert rel(single[0][0], single[1][0]) > 1e-3
    assert rel(chains[0][0], chains[1][0]) > 1e-3


@pytest.mark.parametrize("engine", ["grid", "chain", "wave"])
def test_x_sessions_take_the_whole_seed(engine):
    from test_gpu_xmode import make_problem
    n, D, N, r, Q, m = X_SHAPES[engine]
    p = make_problem(n, D, N, r, Q, seed=31)
    ls = np.tile(p["ls"], (2, 1))
    got = G().GPTregression_chains_x(p["X"], p["y"], ls, 1.0, p["scale"], p["Z"], p["b"], SV, p["I"],
                                     r, Q, m, EPSW, EPSU, 0, 2, SEEDS, engine=engine)
    phi = R.feature(p["X"], p["ls"], 1.0, p["scale"], p["Z"], p["b"])
    for c, s in enumerate(SEEDS):
        wo, Uo, info = R.GPTregression(phi, p["y"], SV, p["I"], r, Q, m, EPSW, EPSU, 0, 2, s)
        ws, Us, st = got[c]
        assert st == 0 and info["status"] == 0
        assert rel(ws, wo) < 1e-8, (c, rel(ws, wo))
        assert rel(Us, Uo) < 1e-8, (c, rel(Us, Uo))
    assert rel(got[0][0], got[1][0]) > 1e-3


# ---------------------------------------------------------------------- the other Philox consumers
def _ml_problem(ntr, nte):
    from test_gpu_movielens import problem
    return problem(ntr, nte)


def test_cf_fullw_sideinfo_takes_the_whole_seed():
    from gpt_amd import movielens
    from oracle import movielens_ref as M
    tr, te, ud, md, mu, sd = _ml_problem(600, 200)
    w0 = np.random.default_rng(5).standard_normal((3, 3))
    runs = []
    for s in SEEDS:
        args = (tr, ud, md, te, 0.8, 0.1, 1.0, w0, 64, 1e-4, 1e-4, 0.5, 0.25, 0.5, 0, 1, s, mu, sd)
        got = movielens.GPT_fullw_sideinfo(*args, langevin=True, stiefel=True, avg=True)
        want = M.GPT_fullw_sideinfo(*args, langevin=True, stiefel=True, avg=True)
        for g, w_ in zip(got[:3], want[:3]):
            assert rel(g, w_) < 1e-8, rel(g, w_)
        assert np.abs(got[3] - want[3]).max() < 1e-8
        runs.append(got)
    assert rel(runs[0][1], runs[1][1]) > 1e-3


def test_cf_fullw_gibbs_takes_the_whole_seed():
    from gpt_amd import movielens
    from oracle import movielens_ref as M
    tr, te, ud, md, mu, sd = _ml_problem(800, 300)
    w0 = np.random.default_rng(9).standard_normal((3, 3))
    runs = []
    for s in SEEDS:
        args = (tr, ud, md, te, 0.8, 0.5, 1.0, w0, 0, 1, 1, s, mu, sd)
        got = movielens.GPT_fullw_gibbs(*args)
        want = M.GPT_fullw_gibbs(*args)
        for g, w_ in zip(got[:3], want[:3]):
            assert rel(g, w_) < 1e-8, rel(g, w_)
        assert np.abs(got[3] - want[3]).max() < 1e-8
        runs.append(got)
    assert rel(runs[0][0], runs[1][0]) > 1e-3


def test_tgp_gibbs_takes_the_whole_seed():
    from gpt_amd import TGP
    from test_gpu_tgp import data, oracle_b
    n, D, N, r, q, sigma, iters, burnin = 7, 3, 131, 3, 20, 0.3, 2, 0
    X, y = data(N, D, 7)
    runs = []
    for s in SEEDS:
        W, U, I = TGP.GPT_inf(X, y, sigma, n, r, 1.4332, q, s, iters, burnin)
        b = oracle_b(R.datawhitening(X), n, 1.4332, s)
        Wo, Uo, Io = R.GPT_inf(b, R.datawhitening(y), sigma, n, r, q, iters, burnin, s)
        assert (I == Io).all()
        assert rel(W, Wo) < 1e-8 and rel(U, Uo) < 1e-8, (rel(W, Wo), rel(U, Uo))
        runs.append(W)
    assert rel(runs[0], runs[1]) > 1e-3


def test_gmc_takes_the_whole_seed():
    from test_gpu_parity import _gmc_problem
    n, D, N, r, Q, L = 8, 3, 40, 2, 5, 5
    phi, y, I = _gmc_problem(n, D, N, r, Q)
    runs = []
    for s in SEEDS:
        ws, Us, acc = G().GPT_GMC(phi, y, 1.0, I, r, Q, 1e-2, 1e-2, 1, 3, L, s)
        wo, Uo, acco = R.GPT_GMC(phi, y, 1.0, I, r, Q, 1e-2, 1e-2, 1, 3, L, s)
        assert rel(ws, wo) < 1e-8 and rel(Us, Uo) < 1e-8, (rel(ws, wo), rel(Us, Uo))
        assert np.all(np.abs(acc - acco) <= 1e-7 * np.maximum(np.abs(acco), 1e-3))
        runs.append(ws)
    assert rel(runs[0], runs[1]) > 1e-3


def test_gpnt_sgld_takes_the_whole_seed():
    rng = np.random.default_rng(12)
    N, D, n = 120, 4, 80
    X = rng.standard_normal((N, D)); Z = rng.standard_normal((n, D)); b = 2 * np.pi * rng.random(n)
    phi = R.featureNotensor(X, 1.4, 1.0, Z, b)
    y = rng.standard_normal(N)
    runs = []
    for s in SEEDS:
        got = G().GPNT_SGLD(phi, y, 0.05, 1.0, 25, 1e-4, 0.1, 1, 2, s)
        want = R.GPNT_SGLD(phi, y, 0.05, 1.0, 25, 1e-4, 0.1, 1, 2, s)
        assert got.shape == want.shape and rel(got, want) < 1e-9
        runs.append(got)
    assert rel(runs[0], runs[1]) > 1e-3


@pytest.mark.parametrize("N", [97, 14000])
def test_epoch_orders_take_the_whole_seed(N):
    """Both forms of the device shuffle: in LDS, and in the global workspace past 13 632 rows."""
    from oracle import philox as px
    runs = []
    for s in SEEDS:
        got = G().epoch_orders(N, s, 2)
        order = np.arange(N)
        for e in range(2):
            order = order[px.randperm(N, s, e)]
            assert np.array_equal(got[:, e], order), (s, e)
        runs.append(got)
    assert not np.array_equal(runs[0], runs[1])
