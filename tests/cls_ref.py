"""fp64 numpy restatements of the classification side, its evaluation in numpy and in mpmath, the
test cases and the error yardsticks of tests/test_cls_ref.py and tests/test_gpu_cls.py.

    gpnt_sgld_class / gpnt_sgld_class_literal   GPNT_SGLDclass, GPT_SGLD.jl:851-901
    class_eval_np / class_eval_mp               ImageNoTensorExperiment.jl:56-73 (indmax, logsumexp)
    row_bound / mean_bound                      what fp64 can hold of nlp_i and of its mean

RNG contract of the sampler (it extends GPNT_SGLD's with class tags, as init_state_cls does):
theta[:, c] = sigma_theta·normals(n, seed, 0, THETA_INIT, c); the noise of 1-based step t and class
c is normals(n, seed, t-1, THETA_NOISE, c); epoch orders are the cumulative randperm(N, seed,
epoch-1).  Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import functools
import math
import os

import numpy as np

from oracle import philox as px

EPS = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment.npz")

# (n, N, C, m, burnin, maxepoch, decay_rate, sigma_theta)
SAMPLER_CASES = [
    (70, 130, 3, 25, 1, 2, 0.1, 1.0),     # n not a multiple of 64; ragged last batch of 5
    (150, 203, 7, 50, 0, 2, 0.0, 1.0),    # the experiment's n, m, C; last batch of 3
    (64, 96, 2, 96, 0, 3, 0.5, 0.7),      # one batch of > 64 columns; binary; unscaled +theta
    (33, 64, 16, 7, 0, 1, 0.0, 1.0),      # n < 64; many classes
    (20, 10, 2, 50, 0, 2, 0.0, 1.0),      # m > N
    (330, 70, 2, 64, 0, 2, 0.0, 1.0),     # 8·n·m = 169 KB: the batch's phi is re-read, not staged
]
# (Ntest, C, T)
EVAL_SHAPES = [(130, 3, 4), (1010, 7, 5), (64, 2, 1), (257, 16, 3)]
EVAL_SCALES = [1.0, 50.0, 700.0]


def case_name(case):
    return "_".join("%g" % v for v in case)


def sampler_inputs(case, idx=0):
    """phi (n, N) with entries of RFF size, labels 1..C with every class present, eps_theta."""
    n, N, C = case[:3]
    rng = np.random.default_rng(4000 + idx)
    phi = np.asfortranarray(math.sqrt(2.0 / n) * np.cos(rng.uniform(0, 2 * np.pi, (n, N))))
    y = (np.arange(N) % C) + 1
    rng.shuffle(y)
    return phi, y.astype(np.float64), 2e-3


def check_labels(y, C=None):
    yv = np.asarray(y, dtype=np.float64).ravel()
    yi = yv.astype(np.int64)
    if C is None:
        C = int(yv.max() - yv.min() + 1)
    if not np.array_equal(yi, yv) or yi.min() < 1 or yi.max() > C:
        raise ValueError("labels must be integers in 1..C")
    return yi, C


def logsumexp(x):
    """GPT_SGLD.jl:8-11."""
    a = np.max(x)
    return a + math.log(np.sum(np.exp(x - a)))


def gpnt_sgld_class(phi, y, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch, param_seed,
                    store_every=1, ncls=None):
    """GPT_SGLD.jl:851-901, vectorised.  theta_store (n, C, kept), or zeros(n) on NaN."""
    phi = np.asarray(phi, dtype=np.float64)
    n, N = phi.shape
    yi, C = check_labels(y, ncls)
    numbatches = -(-N // m)
    theta = np.empty((n, C))
    for c in range(C):
        theta[:, c] = sigma_theta * px.normals(n, param_seed, 0, px.THETA_INIT, c)
    total = (maxepoch + burnin) * numbatches
    store = np.zeros((n, C, total // store_every), order="F")
    order = np.arange(N)
    t = 0
    for epoch in range(1, maxepoch + burnin + 1):
        order = order[px.randperm(N, param_seed, epoch - 1)]
        for batch in range(1, numbatches + 1):
            t += 1
            idx = order[m * (batch - 1): min(m * batch, N)]
            pb = phi[:, idx]
            B = len(idx)
            eps = eps_theta * float(t) ** (-decay_rate)
            x = theta.T @ pb                                        # C x B
            a = x.max(axis=0)
            lse = a + np.log(np.exp(x - a).sum(axis=0))
            P = np.exp(x - lse)
            P[yi[idx] - 1, np.arange(B)] -= 1.0
            gradtheta = (N / B) * (pb @ P.T) + theta                # no sigma_theta here (:888)
            noise = np.empty((n, C))
            for c in range(C):
                noise[:, c] = px.normals(n, param_seed, t - 1, px.THETA_NOISE, c)
            theta = theta - (eps * gradtheta / 2 + math.sqrt(eps) * noise)
            if t % store_every == 0:
                store[:, :, t // store_every - 1] = theta
            if np.isnan(theta).any():
                return np.zeros(n)
    return store


def gpnt_sgld_class_literal(phi, y, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch,
                            param_seed, ncls=None):
    """The same with the loops of :877-892 transcribed one to one (``ncls``: C where the labels do
    not span it)."""
    phi = np.asarray(phi, dtype=np.float64)
    n, N = phi.shape
    yi, C = check_labels(y, ncls)
    numbatches = -(-N // m)
    theta = np.empty((n, C))
    for c in range(C):
        theta[:, c] = sigma_theta * px.normals(n, param_seed, 0, px.THETA_INIT, c)
    store = np.zeros((n, C, (maxepoch + burnin) * numbatches), order="F")
    order = np.arange(N)
    t = 0
    for epoch in range(1, maxepoch + burnin + 1):
        order = order[px.randperm(N, param_seed, epoch - 1)]
        for batch in range(1, numbatches + 1):
            t += 1
            idx = order[m * (batch - 1): min(m * batch, N)]
            phi_batch = phi[:, idx]
            y_batch = yi[idx]
            batch_size = len(idx)
            epsilon = eps_theta * float(t) ** (-decay_rate)
            phi_theta = theta.T @ phi_batch
            gradtheta = np.zeros((n, C))
            for c in range(C):
                for i in range(batch_size):
                    gradtheta[:, c] += math.exp(phi_theta[c, i] - logsumexp(phi_theta[:, i])) * phi_batch[:, i]
            for i in range(batch_size):
                gradtheta[:, y_batch[i] - 1] -= phi_batch[:, i]
            gradtheta *= N / batch_size
            gradtheta += theta
            grad = epsilon * gradtheta / 2
            noise = np.empty((n, C))
            for c in range(C):
                noise[:, c] = math.sqrt(epsilon) * px.normals(n, param_seed, t - 1, px.THETA_NOISE, c)
            theta = theta - (grad + noise)
            store[:, :, t - 1] = theta
            if np.isnan(theta).any():
                return np.zeros(n)
    return store


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# --------------------------------------------------------------------------- evaluation
def _as3(scores):
    s = np.asarray(scores, dtype=np.float64)
    return s.reshape(s.shape + (1,)) if s.ndim == 2 else s


def rows_eval_np(x, yi):
    """x (Ntest, C): prediction (1-based, first index of the maximum) and nlp per row."""
    a = x.max(axis=1)
    lse = a + np.log(np.exp(x - a[:, None]).sum(axis=1))
    return np.argmax(x, axis=1) + 1, lse - x[np.arange(x.shape[0]), yi - 1]


def window_mean(scores, window):
    """Mean over the samples of the half-open 0-based window: the exactly rounded sum (fsum)
    over W, so within 2^-52 relative of the true mean."""
    s = _as3(scores)
    first, last = window
    out = np.empty(s.shape[:2])
    for i in range(s.shape[0]):
        for c in range(s.shape[1]):
            out[i, c] = math.fsum(s[i, c, first:last]) / (last - first)
    return out


def class_eval_np(scores, ytest, window=None):
    s = _as3(scores)
    Nt, C, T = s.shape
    yi, _ = check_labels(ytest, C)
    window = (0, T) if window is None else window
    if not 0 <= window[0] < window[1] <= T:
        raise ValueError("bad window")
    pm, nl = np.empty(T), np.empty(T)
    for t in range(T):
        pr, nlp = rows_eval_np(s[:, :, t], yi)
        pm[t] = 1 - np.sum(pr == yi) / Nt
        nl[t] = nlp.mean()
    mean = window_mean(s, window)
    pr, nlp = rows_eval_np(mean, yi)
    return dict(prop_missed=pm, mean_nlp=nl, avg_prop_missed=1 - np.sum(pr == yi) / Nt,
                avg_mean_nlp=nlp.mean(), mean_fhat=mean, prediction=pr, nlp=nlp)


def rows_eval_mp(x, yi):
    """The same at 50 digits on the given doubles: prediction (int array) and nlp (list of mpf).
    The comparisons of the maximum act on the doubles, so the prediction is exact."""
    import mpmath as mp
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        pred = np.argmax(x, axis=1) + 1
        nlp = []
        for i in range(x.shape[0]):
            row = [mp.mpf(float(v)) for v in x[i]]
            a = max(row)
            lse = a + mp.log(mp.fsum(mp.exp(v - a) for v in row))
            nlp.append(lse - row[int(yi[i]) - 1])
        return pred, nlp
    finally:
        mp.mp.dps = old


def mp_mean(vals):
    import mpmath as mp
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        return mp.fsum(vals) / len(vals)
    finally:
        mp.mp.dps = old


def row_bound(x, yi):
    """E_i = eps·(2|a_i| + |x_{i,y_i}| + C + 4): a + log(sum exp) - x_y with exp and log correct to
    1 ulp; the sum of C terms lies in [1, C]."""
    a = np.abs(x.max(axis=1))
    xy = np.abs(x[np.arange(x.shape[0]), yi - 1])
    return EPS * (2 * a + xy + x.shape[1] + 4)


def mean_bound(E, nlp):
    """mean_i E_i + eps·Ntest·mean_i|nlp_i|: any summation order of the Ntest terms."""
    nl = np.array([abs(float(v)) for v in nlp])
    return float(np.mean(E) + EPS * len(nl) * nl.mean())


def eval_windows(T):
    """All samples, one sample, a strict sub-window; none but the first holds sample 0."""
    if T == 1:
        return [(0, 1)]
    w = [(0, T), (T - 1, T)]
    if T >= 3:
        w.append((1, T - 1))
    return w


def eval_scores(shape, scale, plant=True):
    """Random scores scale·randn and labels; with ``plant``, sample 0 holds, in rows 0-11, exact
    ties of the maximum (the first of the tied indices is the label, the last, or neither), rows
    with all scores equal (nlp = log C) and rows whose true class is 1000 below the maximum.
    Sample 0 lies in no window of eval_windows(T) but the all-samples one, where the other samples
    break the ties of the mean."""
    Nt, C, T = shape
    rng = np.random.default_rng(int(97 * Nt + 13 * C + T + scale))
    s = np.asfortranarray(scale * rng.standard_normal((Nt, C, T)))
    y = rng.integers(1, C + 1, Nt)
    if plant:
        for i in range(12):
            k = i % 4
            if k == 0:                       # tie of the maximum at indices 0 and C-1, label first
                s[i, :, 0] = np.minimum(s[i, :, 0], 0.25 * scale)
                s[i, 0, 0] = s[i, C - 1, 0] = 0.5 * scale
                y[i] = 1
            elif k == 1:                     # the same, label the last of the tied: a miss
                s[i, :, 0] = np.minimum(s[i, :, 0], 0.25 * scale)
                s[i, 0, 0] = s[i, C - 1, 0] = 0.5 * scale
                y[i] = C
            elif k == 2:                     # all equal
                s[i, :, 0] = 0.375 * scale
            else:                            # true class 1000 below the maximum
                top = s[i, :, 0].max()
                y[i] = int(np.argmin(s[i, :, 0])) + 1
                s[i, y[i] - 1, 0] = top - 1000.0
    return s, y.astype(np.int32)


def top_two_gap(x):
    p = np.sort(x, axis=1)
    return p[:, -1] - p[:, -2]


@functools.lru_cache(maxsize=None)
def eval_reference(shape, scale, plant=True):
    """scores, labels and, per sample, (prediction, nlp in mpmath, E) — computed once per case."""
    s, y = eval_scores(shape, scale, plant)
    per = []
    for t in range(shape[2]):
        pred, nlp = rows_eval_mp(s[:, :, t], y)
        per.append((pred, nlp, row_bound(s[:, :, t], y)))
    return s, y, per


# --------------------------------------------------------------------------- segment data
SEG_LS = [5.1212, 1.4029, 5.0614, 5.8121, 6.1082, 4.7774, 1.7421, 1.6444, 1.8365, 1.7417, 1.8233,
          2.8132, 1.2788, 1.8477, 2.0961, 1.1489]
SEG_SIGMA_RBF = 11.4468
SEG = dict(n=150, m=50, eps_theta=0.001, decay_rate=0.0, sigma_theta=1.0, seed=2, feature_seed=17,
           burnin=2, maxepoch=10, Ntrain=1300)


def segment_problem():
    """ImageNoTensorExperiment.jl:8-26: columns [1, 2, 6:20] of segment.dat, 1300 training rows
    whitened by their own mean and std, the other 1010 by the training rows' statistics."""
    data = np.load(GOLDEN)["data"]
    data = data[:, [0, 1] + list(range(5, 20))]
    D, Ntr = 16, SEG["Ntrain"]
    Xtr, ytr = data[:Ntr, :D], data[:Ntr, D].astype(np.int64)
    mu, sd = Xtr.mean(axis=0), Xtr.std(axis=0, ddof=1)
    Xte, yte = (data[Ntr:, :D] - mu) / sd, data[Ntr:, D].astype(np.int64)
    return (Xtr - mu) / sd, ytr, Xte, yte
