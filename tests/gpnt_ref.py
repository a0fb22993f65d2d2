"""Restatements, cases and yardsticks of the full-theta regression chains (GPNT_SGLD_chains,
GPNT_pred) for tests/test_gpnt_ref.py and tests/test_gpu_gpnt.py.

    gpnt_sgld_chains        per chain oracle.gpt_sgld_ref.GPNT_SGLD thinned by store_every
    three_steps_mp          GPT_SGLD.jl:826-843 at 50 digits on the same doubles
    yardstick               the numpy restatement's own error against three_steps_mp
    scores_mp / rmse_mp / mean_mp   PowerPlantNoTensorExperiment.jl:51-63 at 50 digits

RNG contract (GPNT_SGLD's): theta0 = sigma_theta·normals(n, seed, 0, THETA_INIT, 0), the noise of
1-based step t is normals(n, seed, t-1, THETA_NOISE, 0), epoch orders are the cumulative
randperm(N, seed, epoch-1).  Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import functools
import math

import numpy as np

from oracle import gpt_sgld_ref as R
from oracle import philox as px

U = 2.0 ** -53
NAN_THETA = 4                       # GPT_ERR_NAN_THETA

# name -> (n, N, m, burnin, maxepoch, decay_rate); the workgroup is 512 threads = 8 waves
CASES = {
    "A": (70, 103, 25, 1, 2, 0.1),     # n not a multiple of 64; whole batch staged; last batch of 3
    "B": (1100, 60, 20, 0, 2, 0.0),    # n past 2 x 512; row groups with a short last one; m | N
    "C": (10300, 24, 5, 0, 2, 0.0),    # one row does not fit beside theta: not staged
    "D": (64, 5, 1, 0, 2, 0.0),        # B = 1
    "E": (64, 10, 25, 0, 2, 0.5),      # m > N: one short batch per epoch
    "F": (6000, 12, 6, 0, 1, 0.0),     # two rows fit beside theta: fewer than half the waves, so
                                       # not staged unless asked for (and then 12 carry registers)
}
# three sibling chains: different seeds, step sizes, signal_var and sigma_theta; two share a seed
SEEDS = [5, 11, 5]
EPS = [1e-4, 5e-5, 2e-4]
SIGNAL_VAR = [0.05, 0.1, 0.02]
SIGMA_THETA = [1.0, 0.7, 1.3]


def inputs(name, N=None):
    """phi (n, N) with entries of RFF size and y = phi'w + noise; N replaces the case's own."""
    n, N0 = CASES[name][:2]
    N = N0 if N is None else N
    rng = np.random.default_rng(7000 + ord(name))
    phi = np.asfortranarray(math.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, N))))
    y = phi.T @ rng.standard_normal(n) + 0.1 * rng.standard_normal(N)
    return phi, y


def gpnt_sgld_chains(phi, y, signal_vars, sigma_thetas, m, eps_thetas, decay_rate, burnin, maxepoch,
                     seeds, store_every=1):
    """(theta_store (n, kept, nchains), status): chain k is GPNT_SGLD of its own arguments with the
    1-based steps divisible by store_every kept; a chain that met a NaN has a zero store."""
    n, N = phi.shape
    total = (burnin + maxepoch) * (-(-N // m))
    kept = total // store_every
    k = len(seeds)
    store = np.zeros((n, kept, k), order="F")
    status = np.zeros(k, dtype=np.int32)
    for c in range(k):
        with np.errstate(all="ignore"):
            full = R.GPNT_SGLD(phi, y, signal_vars[c], sigma_thetas[c], m, eps_thetas[c], decay_rate,
                               burnin, maxepoch, seeds[c])
        if full.ndim == 1:
            status[c] = NAN_THETA
        else:
            store[:, :, c] = full[:, store_every - 1::store_every][:, :kept]
    return store, status


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# --------------------------------------------------------------------------- three steps, mpmath
def _mp():
    import mpmath as mp
    return mp


def three_steps_mp(phi, y, signal_var, sigma_theta, m, eps_theta, decay_rate, seed, steps=3):
    """theta after each of the first `steps` steps, (n, steps) of mpf, on the doubles phi, y, theta0
    and noise: everything else (dot products, the gradient, eps_t and its root) at 50 digits."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        n, N = phi.shape
        nb = -(-N // m)
        f = lambda v: mp.mpf(float(v))
        theta = [f(v) for v in sigma_theta * px.normals(n, seed, 0, px.THETA_INIT, 0)]
        out = []
        order = np.arange(N)
        t = 0
        for epoch in range(1, -(-steps // nb) + 1):
            order = order[px.randperm(N, seed, epoch - 1)]
            for batch in range(1, nb + 1):
                if t == steps:
                    break
                t += 1
                idx = order[m * (batch - 1): min(m * batch, N)]
                B = len(idx)
                eps = f(eps_theta) * mp.mpf(t) ** (-f(decay_rate))
                res = [f(y[i]) - mp.fsum(f(phi[j, i]) * theta[j] for j in range(n)) for i in idx]
                noise = px.normals(n, seed, t - 1, px.THETA_NOISE, 0)
                cN = mp.mpf(N) / B
                new = []
                for j in range(n):
                    g = mp.fsum(f(phi[j, i]) * r for i, r in zip(idx, res))
                    grad = -theta[j] / f(sigma_theta) ** 2 + cN * g / f(signal_var)
                    new.append(theta[j] + eps * grad / 2 + mp.sqrt(eps) * f(noise[j]))
                theta = new
                out.append(theta)
        return out
    finally:
        mp.mp.dps = old


def max_err_mp(got, ref):
    """max |got - ref| / max |ref| over the columns of ref (a list of columns of mpf)."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        top = max(abs(v) for col in ref for v in col)
        err = max(abs(mp.mpf(float(got[j, s])) - v) for s, col in enumerate(ref) for j, v in enumerate(col))
        return float(err / top)
    finally:
        mp.mp.dps = old


STEP_CASES = ("A", "B")


def step_problem(name):
    """Cases A and B at N = m + 3: a full batch, the short batch of 3, the next epoch's first."""
    n, _, m, _, _, decay = CASES[name]
    phi, y = inputs(name, N=m + 3)
    return phi, y, SIGNAL_VAR[0], SIGMA_THETA[1], m, EPS[0], decay, SEEDS[1]


@functools.lru_cache(maxsize=None)
def step_reference(name):
    return three_steps_mp(*step_problem(name))


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """u: the error of the numpy restatement's first three steps against mpmath, relative to
    max|theta|.  The device's bar is min(8·u, 1e-13)."""
    phi, y, sv, sth, m, eps, decay, seed = step_problem(name)
    full = R.GPNT_SGLD(phi, y, sv, sth, m, eps, decay, 0, 2, seed)
    return max_err_mp(full[:, :3], step_reference(name))


def step_bar(name):
    return min(8.0 * yardstick(name), 1e-13)


# --------------------------------------------------------------------------- evaluation
EVAL = dict(n=70, Ntest=130, T=5, scale=17.3, window=(1, 4))


@functools.lru_cache(maxsize=None)
def eval_inputs():
    n, Nt, T = EVAL["n"], EVAL["Ntest"], EVAL["T"]
    rng = np.random.default_rng(811)
    theta = np.asfortranarray(rng.standard_normal((n, T)))
    phitest = np.asfortranarray(math.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, Nt))))
    ytest = phitest.T @ theta.mean(axis=1) + 0.3 * rng.standard_normal(Nt)
    for a in (theta, phitest, ytest):
        a.setflags(write=False)
    return theta, phitest, ytest


def eval_x_inputs():
    """Xtest (Ntest, 3), length scales, sigma_RBF, Z, b for the X form (D = 3)."""
    rng = np.random.default_rng(812)
    n, Nt = EVAL["n"], EVAL["Ntest"]
    return (np.asfortranarray(rng.standard_normal((Nt, 3))), np.array([1.4, 0.9, 2.1]), 1.3,
            np.asfortranarray(rng.standard_normal((n, 3))), 2 * np.pi * rng.random(n))


def scores_mp(phitest, theta):
    """(scores[i][t] as mpf, mag[i, t] = sum_j |phitest[j, i]·theta[j, t]|)."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        n, Nt = phitest.shape
        T = theta.shape[1]
        P = [[mp.mpf(float(phitest[j, i])) for j in range(n)] for i in range(Nt)]
        Th = [[mp.mpf(float(theta[j, t])) for j in range(n)] for t in range(T)]
        s = [[mp.fsum(a * b for a, b in zip(P[i], Th[t])) for t in range(T)] for i in range(Nt)]
        return s, np.abs(phitest).T @ np.abs(theta)
    finally:
        mp.mp.dps = old


def rmse_mp(f, ytest, scale):
    """scale·sqrt(sum_i (ytest_i - f_i)^2 / Ntest) at 50 digits on the doubles f, ytest."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        sse = mp.fsum((mp.mpf(float(y)) - mp.mpf(float(v))) ** 2 for y, v in zip(ytest, f))
        return mp.mpf(float(scale)) * mp.sqrt(sse / len(ytest))
    finally:
        mp.mp.dps = old


def mean_mp(scores, first, last):
    """Per row the mean of the doubles scores[i, first:last] at 50 digits."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return [mp.fsum(mp.mpf(float(v)) for v in row[first:last]) / (last - first) for row in scores]
    finally:
        mp.mp.dps = old


def rel_err_mp(got, want):
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return float(abs(mp.mpf(float(got)) - want) / abs(want))
    finally:
        mp.mp.dps = old


def abs_err_mp(got, want):
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return float(abs(mp.mpf(float(got)) - want))
    finally:
        mp.mp.dps = old


def eval_np(theta, phitest, ytest, window, scale):
    """The script's own evaluation in numpy (PowerPlantNoTensorExperiment.jl:51-63)."""
    f = phitest.T @ theta
    Nt = len(ytest)
    sample = scale * np.linalg.norm(ytest[:, None] - f, axis=0) / math.sqrt(Nt)
    mean = f[:, window[0]:window[1]].mean(axis=1)
    return dict(scores=f, sample_rmse=sample, mean_fhat=mean,
                rmse=scale * np.linalg.norm(ytest - mean) / math.sqrt(Nt))
