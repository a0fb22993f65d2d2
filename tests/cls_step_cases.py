"""Cases, inputs, the 50-digit reference and the CPU-side measurements of the full-theta softmax
sampler's step tests (tests/test_gpu_cls_step.py on the device, tests/test_cls_step_cases.py on the
CPU): GPNT_SGLDclass (GPT_SGLD.jl:851-901), ntc_chain_kernel of gpt_amd/csrc/cls.hip, at every
class width CC, on both sides of the staging edge, with theta filling LDS, with saturated logits,
across the 4096-step launch boundary and with a store stride that leaves a tail.

A case is a Case tuple; its phi and labels are built like cls_ref.sampler_inputs (the six
cls_ref.SAMPLER_CASES are here under old_*, with the very inputs tests/test_gpu_cls.py gives them).

The reference (compute) is GPT_SGLD.jl:869-899 on the exact doubles of phi, theta0 =
sigma·philox.normals, eps and the labels, with everything else at MP_DIGITS digits: the dot products,
the max-shifted log-sum-exp, the softmax, the gradient, eps_t = eps·t^(-decay), its square root and
the update, for every stored step.  The step noise is oracle.step_cases._mp_normals: the project's
50-digit Box–Muller on the Philox integers (as the Gibbs and step goldens draw), not the doubles of
philox.normals, so no allowance for the device's own draw is added to any bar.  Nothing is rounded
between steps.

Storage (tests/golden/cls_step_mp.npz, maker tests/golden/make_cls_step_golden.py): per case `name`
name_digest (SHA-256 of the case and its regenerated inputs), name_hi (kept, entries) float64 +
name_lo float32, name_scale (kept,) = max|theta| of the whole step, name_u and name_seconds.  A step
of more than KEEP entries (theta_fills_lds alone) is kept at select()'s entries: every S-th in
column-major order, S the smallest stride coprime to n that leaves at most KEEP, and the first and
last EDGE entries.

Error of a run: max|run − ref| over the kept entries of a stored step over that step's max|theta|,
the largest over the stored steps.  Bar per case: B = MARGIN·u, u that error of the numpy restatement
cls_ref.gpnt_sgld_class as the maker measured it.  Nothing here comes from the device.
Test infrastructure: numpy / mpmath, no GPU.
"""
import collections
import functools
import hashlib
import math
import os

import numpy as np

import cls_ref as CLS
from oracle import philox as px
from oracle import step_cases as SC

MP_DIGITS = SC.MP_DIGITS
MARGIN = SC.MARGIN       # device bar B = MARGIN·u (tests/test_gpu_step.py explains the factor)
CAP_SHORT, CAP = 1e-14, 1e-13            # on B: cases of at most SHORT_STEPS steps, every case
SHORT_STEPS = 10
OLD_BAR = 1e-9           # tests/test_gpu_cls.py::test_sampler_matches_the_restatement
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cls_step_mp.npz")
KEEP, EDGE = 2048, 64
NW = 8                   # kNW: waves of a workgroup
LDS = 160 * 1024
LAUNCH_STEPS = 4096      # gpt_gpnt_sgld_class_chains: steps of one launch, within an epoch
EPS0 = 2e-3              # cls_ref.sampler_inputs' step size
EPS_LARGE = 0.5          # where the gradient's part of the move is to show beside the noise's
SEED = 5
SATURATION = 800.0       # max|x| the saturated case has to exceed at step 1
SHARE_MIN = 0.1

# labels: None = cls_ref.sampler_inputs' (1..C, every class present when N >= C); (lo, hi) = the
# values lo..hi in turn, shuffled, with C given to the chains entry as ncls
Case = collections.namedtuple("Case", "name n N C m epochs decay sigma store_every eps idx labels")


def _cases():
    def new(k, name, n, N, C, m, epochs, decay=0.0, sigma=1.0, store_every=1, eps=EPS0, labels=None):
        return Case(name, n, N, C, m, epochs, decay, sigma, store_every, eps, 20 + k, labels)
    out = [
        new(0, "cc32_min", 70, 53, 17, 25, 2, decay=0.1, eps=EPS_LARGE),
        new(1, "cc32_full", 33, 40, 32, 7, 1),
        new(2, "one_class", 20, 10, 1, 4, 2),
        new(3, "absent_classes", 40, 30, 5, 8, 1, labels=(2, 3)),
        new(4, "stage_last", 307, 67, 2, 64, 1),
        new(5, "stage_first_off", 308, 67, 2, 64, 1),
        new(6, "theta_fills_lds", 630, 3, 32, 1, 1),
        new(7, "saturated", 70, 130, 3, 25, 1, sigma=500.0),
        new(8, "wide_batch", 64, 96, 7, 96, 2, decay=0.5),
        new(9, "two_launches", 8, 4097, 2, 1, 1, decay=0.3, store_every=241),
        new(10, "store_tail", 33, 23, 3, 5, 2, store_every=4),
    ]
    # the six cases of tests/test_gpu_cls.py with their inputs; the longer ones keep every second or
    # third step, which holds the fixture under its size and loses no step: an error stays in theta
    every = (3, 2, 1, 2, 1, 1)
    for idx, (c, se) in enumerate(zip(CLS.SAMPLER_CASES, every)):
        n, N, C, m, burnin, maxepoch, decay, sigma = c
        out.append(Case("old_" + CLS.case_name(c), n, N, C, m, burnin + maxepoch, decay, sigma, se,
                        EPS0, idx, None))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
REFUSED_N = 640          # theta_fills_lds' shape at this n: 8·n·32 bytes alone are 160 KiB


def nb(c):
    return -(-c.N // c.m)


def total(c):
    return c.epochs * nb(c)


def kept(c):
    return total(c) // c.store_every


# ---------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """(phi (n, N) column-major, labels (N,) float64), read-only."""
    c = BY_NAME[name]
    phi, y, eps = CLS.sampler_inputs((c.n, c.N, c.C), c.idx)
    assert eps == EPS0
    if c.labels is not None:
        lo, hi = c.labels
        y = lo + (np.arange(c.N) % (hi - lo + 1))
        np.random.default_rng(4100 + c.idx).shuffle(y)
        y = y.astype(np.float64)
    phi.setflags(write=False)
    y.setflags(write=False)
    return phi, y


def digest(c):
    h = hashlib.sha256(repr(tuple(c)).encode())
    for a in inputs(c.name):
        a = np.asfortranarray(a)
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    return h.hexdigest()


def select(n, size):
    """Flat column-major indices of the kept entries of a step of `size` entries."""
    if size <= KEEP:
        return np.arange(size)
    S = -(-size // KEEP)
    while math.gcd(S, n) != 1:
        S += 1
    return np.unique(np.concatenate([np.arange(0, size, S), np.arange(EDGE),
                                     np.arange(size - EDGE, size)]))


def flat_steps(store):
    """theta_store (n, C, kept) -> (kept, n·C column-major)."""
    store = np.asarray(store)
    return np.transpose(store, (2, 1, 0)).reshape(store.shape[2], -1)


# --------------------------------------------------------------------------- device layout restated
def _al16(x):
    return (x + 15) & ~15


def ntc_layout(n, C, m):
    """gpt_amd/csrc/cls.hip's ntc_layout: CC, the byte offsets, stage and bytes."""
    CC = 2 if C <= 2 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32
    L = dict(CC=CC, o_theta=0)
    o = _al16(8 * n * CC)
    L["o_idx"] = o
    o = _al16(o + 4 * m)
    L["o_yb"] = o
    o = _al16(o + 4 * m)
    L["o_P"] = o
    o = _al16(o + 8 * C * m)
    L["o_flag"] = o
    o = _al16(o + 4 * NW)
    L["o_phi"] = L["base"] = o
    staged = _al16(o + 8 * n * m)
    L["stage"] = staged <= LDS
    L["bytes"] = staged if L["stage"] else o
    return L


# ------------------------------------------------------------------ the fp64 restatement (hooked)
# name -> relative size; None: a gross defect.  tests/test_cls_step_cases.py holds run_f64 without a
# defect bit for bit to cls_ref.gpnt_sgld_class.
DEFECTS = {"P_scaled": 1e-10, "prior_scaled": 1e-9, "NB_scaled": 1e-10, "sqrt_eps_scaled": 1e-10,
           "noise_scaled": 1e-10, "short_batch_N_over_m": None, "no_max_shift": None}


def run_f64(c, defect=None, probe=None):
    """cls_ref.gpnt_sgld_class on the case with one of DEFECTS: theta_store (n, C, kept), NaN and
    inf kept as they come.  probe='first': dict(xmax, grad_rms, noise_rms, P, softmax) of step 1."""
    phi, y = inputs(c.name)
    d = DEFECTS[defect] if defect else 0.0
    n, N, C, m = c.n, c.N, c.C, c.m
    yi, _ = CLS.check_labels(y, C)
    theta = np.empty((n, C))
    for k in range(C):
        theta[:, k] = c.sigma * px.normals(n, SEED, 0, px.THETA_INIT, k)
    store = np.zeros((n, C, kept(c)), order="F")
    order = np.arange(N)
    t = 0
    with np.errstate(all="ignore"):
        for epoch in range(1, c.epochs + 1):
            order = order[px.randperm(N, SEED, epoch - 1)]
            for batch in range(1, nb(c) + 1):
                t += 1
                idx = order[m * (batch - 1): min(m * batch, N)]
                pb = phi[:, idx]
                B = len(idx)
                eps = c.eps * float(t) ** (-c.decay)
                x = theta.T @ pb
                if defect == "no_max_shift":
                    lse = np.log(np.exp(x).sum(axis=0))
                else:
                    a = x.max(axis=0)
                    lse = a + np.log(np.exp(x - a).sum(axis=0))
                P = np.exp(x - lse)
                soft = P.copy() if probe else None
                if defect == "P_scaled":
                    P = P * (1 + d)
                P[yi[idx] - 1, np.arange(B)] -= 1.0
                cN = N / B
                if defect == "NB_scaled":
                    cN *= 1 + d
                if defect == "short_batch_N_over_m":
                    cN = N / m
                gradtheta = cN * (pb @ P.T) + (theta * (1 + d) if defect == "prior_scaled" else theta)
                noise = np.empty((n, C))
                for k in range(C):
                    noise[:, k] = px.normals(n, SEED, t - 1, px.THETA_NOISE, k)
                if probe == "first":
                    return dict(xmax=float(np.abs(x).max()), grad_rms=float(np.sqrt(np.mean(gradtheta ** 2))),
                                noise_rms=float(np.sqrt(np.mean(noise ** 2))), P=P, softmax=soft)
                if defect == "noise_scaled":
                    noise = noise * (1 + d)
                sq = math.sqrt(eps)
                if defect == "sqrt_eps_scaled":
                    sq *= 1 + d
                theta = theta - (eps * gradtheta / 2 + sq * noise)
                if t % c.store_every == 0:
                    store[:, :, t // c.store_every - 1] = theta
    return store


def run_numpy(c):
    """The restatement of record: cls_ref.gpnt_sgld_class."""
    phi, y = inputs(c.name)
    return CLS.gpnt_sgld_class(phi, y, c.sigma, c.m, c.eps, c.decay, 0, c.epochs, SEED,
                               store_every=c.store_every, ncls=c.C)


def share(c):
    """(eps/2·rms grad) / (sqrt(eps)·rms noise) at step 1: the gradient's part of the move over
    the noise's."""
    p = run_f64(c, probe="first")
    return (c.eps / 2 * p["grad_rms"]) / (math.sqrt(c.eps) * p["noise_rms"])


# ------------------------------------------------------------------------------ mpmath reference
def compute(c):
    """[stored step][n·C column-major] of mpf: the case at MP_DIGITS digits (module docstring)."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _compute(c, mp)


def _compute(c, mp):
    f = lambda v: mp.mpf(float(v))                                            # noqa: E731
    phi, y = inputs(c.name)
    n, N, C, m = c.n, c.N, c.C, c.m
    yi = CLS.check_labels(y, C)[0] - 1
    col = {}                                              # columns of phi as they are first used
    th = [[f(v) for v in c.sigma * px.normals(n, SEED, 0, px.THETA_INIT, k)] for k in range(C)]
    eps_theta, decay = f(c.eps), f(c.decay)
    order = np.arange(N)
    out, t = [], 0
    for epoch in range(1, c.epochs + 1):
        order = order[px.randperm(N, SEED, epoch - 1)]
        for batch in range(1, nb(c) + 1):
            t += 1
            idx = [int(i) for i in order[m * (batch - 1): min(m * batch, N)]]
            B = len(idx)
            for i in idx:
                if i not in col:
                    col[i] = [f(v) for v in phi[:, i]]
            eps = eps_theta * mp.mpf(t) ** (-decay)
            sq = mp.sqrt(eps)
            P = [[None] * B for _ in range(C)]
            for bi, i in enumerate(idx):
                x = [mp.fdot(th[k], col[i]) for k in range(C)]
                a = max(x)
                lse = a + mp.log(mp.fsum(mp.exp(v - a) for v in x))
                for k in range(C):
                    P[k][bi] = mp.exp(x[k] - lse) - (1 if k == yi[i] else 0)
            cN = mp.mpf(N) / B
            rows = [[col[i][j] for i in idx] for j in range(n)]
            new = []
            for k in range(C):
                xi = SC._mp_normals(n, SEED, t - 1, px.THETA_NOISE, k)
                new.append([th[k][j] - (eps * (cN * mp.fdot(rows[j], P[k]) + th[k][j]) / 2 + sq * xi[j])
                            for j in range(n)])
            th = new
            if t % c.store_every == 0:
                out.append([v for colk in th for v in colk])
    return out


def pack(c, ref):
    """compute()'s result as the fixture's arrays {suffix: array}."""
    import mpmath as mp
    sel = select(c.n, c.n * c.C)
    with mp.workdps(MP_DIGITS):
        hi = np.array([[float(step[i]) for i in sel] for step in ref])
        lo = np.array([[float(step[i] - mp.mpf(float(step[i]))) for i in sel] for step in ref],
                      dtype=np.float32)
        scale = np.array([float(max(abs(v) for v in step)) for step in ref])
    return dict(hi=hi, lo=lo, scale=scale)


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(hi, lo, scale, sel, u, bar) of a case from the committed file; the digest has to be the
    one of the inputs this machine regenerates.  Shared and read-only."""
    st, c = _stored(), BY_NAME[name]
    if str(st.get(name + "_digest")) != digest(c):
        raise AssertionError("tests/golden/cls_step_mp.npz does not belong to these inputs: %s" % name)
    u = float(st[name + "_u"])
    return dict(hi=st[name + "_hi"], lo=st[name + "_lo"].astype(np.float64), scale=st[name + "_scale"],
                sel=select(c.n, c.n * c.C), u=u, bar=MARGIN * u)


def step_errors(store, ref):
    """Per stored step max|store − ref| over the kept entries over that step's max|theta|; inf for
    a step that is not finite."""
    got = flat_steps(store)[:, ref["sel"]]
    assert got.shape == ref["hi"].shape, (got.shape, ref["hi"].shape)
    err = np.abs((got - ref["hi"]) - ref["lo"]).max(axis=1) / ref["scale"]
    return np.where(np.isfinite(got).all(axis=1), err, np.inf)


def error(store, ref):
    return float(step_errors(store, ref).max())
