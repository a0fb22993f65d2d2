"""Cases, inputs, the 50-digit reference and the CPU-side measurements of the full-theta regression
sampler's step tests (tests/test_gpu_gpnt_step.py on the device, tests/test_gpnt_step_cases.py on the
CPU): GPNT_SGLD (GPT_SGLD.jl:809-847), gpnt_chain_kernel<PJ> of gpt_amd/csrc/gpnt.hip at every carry
width PJ and on each of its three routes (whole batch staged, row groups, nothing staged), and
gpnt_step_kernel of gpt_amd/csrc/feature.hip, at the sizes where either clamps an index or takes a
second trip.

A case is a Case tuple.  phi and y are built like gpnt_ref.inputs from the case's own generator;
old_A and old_B are gpnt_ref.step_problem's problems (inputs, variances, decay and seed) at a step size
of their own (OLD_EPS), so that the reference here can be set beside gpnt_ref.three_steps_mp called at
that step size.

The reference (compute) is GPT_SGLD.jl:826-843 on the exact doubles of phi, y, eps, the variances and
theta0 = sigma_theta·philox.normals, with everything else at MP_DIGITS digits: the dot products, g,
eps_t = eps·t^(-decay), its square root and the update.  The step noise is
oracle.step_cases._mp_normals: the project's 50-digit Box–Muller on the Philox integers, not the
doubles of philox.normals, so no allowance for the device's own draw is added to any bar.  Nothing is
rounded between steps.

Storage (tests/golden/gpnt_step_mp.npz, maker tests/golden/make_gpnt_step_golden.py): per case `name`
name_digest (SHA-256 of the case and its regenerated inputs), name_hi (kept steps, entries) float64 +
name_lo float32, name_scale (kept steps,) = max|theta| of the whole step, name_u, name_share,
name_share_g and name_seconds.  A step of more than KEEP entries is kept at cls_step_cases.select's
entries: every S-th, S the smallest stride coprime to n that leaves at most KEEP, and the first and
last EDGE.  The three-step cases run two epochs (four steps) on the device and hold the first three.

Error of a run: max|run − ref| over the kept entries of a stored step over that step's max|theta|,
the largest over the stored steps.  Bar per case: B = MARGIN·u, u that error of the numpy restatement
(oracle.gpt_sgld_ref.GPNT_SGLD thinned as gpnt_ref.gpnt_sgld_chains does) as the maker measured it.

Step sizes: at gpnt_ref.EPS the gradient moves theta by 1e-5 of what the noise does, and a defect in g
hides below rounding.  Each new case's eps is chosen so that at step 1 both eps/2·rms(grad) and
eps/2·rms((N/B)·g/signal_var), the data term alone, are at least SHARE_MIN of sqrt(eps)·rms(xi).
old_A and old_B take OLD_EPS by the same rule: at gpnt_ref.EPS[0] old_B's share is 0.024.

Nothing here comes from the device.  Test infrastructure: numpy / mpmath, no GPU.
"""
import collections
import functools
import hashlib
import math
import os

import numpy as np

import cls_step_cases as CS
import gpnt_ref as GR
from oracle import philox as px
from oracle import step_cases as SC

MP_DIGITS = SC.MP_DIGITS
MARGIN = SC.MARGIN       # device bar B = MARGIN·u (tests/test_gpu_step.py explains the factor)
CAP_SHORT, CAP = 1e-14, 1e-13            # on B: cases of at most SHORT_STEPS steps, every case
SHORT_STEPS = 10
OLD_BAR = 1e-9           # tests/test_gpu_gpnt.py::test_chains_match_the_oracle
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpnt_step_mp.npz")
KEEP, EDGE = CS.KEEP, CS.EDGE
select = CS.select
NT, NW = 512, 8          # kNT, kNW: threads and waves of a workgroup
LDS = 160 * 1024         # kMaxLds
LAUNCH_STEPS = 4096      # steps of one launch, within an epoch (host_util.h)
DOT_SPAN = 64 * 32       # 64·kGpntU: columns of a row that one trip of the dots loop covers
MIN_ROWS = NW // 2       # kGpntMinRows
CARRIES = (1, 2, 4, 8, 12, 16, 20)       # GpntCarries
SEED = 5
SIBLING_SEED = 2 ** 40 + 9
SHARE_MIN = 0.1
OLD_EPS = {"A": 5e-4, "B": 4e-3}       # in place of gpnt_ref.EPS[0], for shares of at least SHARE_MIN

# rows: GPTSGLD_GPNT_ROWS of the run, None = unset.  keep: the stored steps held, None = all.
Case = collections.namedtuple(
    "Case", "name n N m epochs decay store_every rows keep signal_var sigma_theta eps seed idx")


def _cases():
    out = []

    def three(name, n, m, tail, rows, sv, sth, eps):
        out.append(Case(name, n, m + tail, m, 2, 0.0, 1, rows, 3, sv, sth, eps, SEED, len(out)))
    three("pj1_full", 512, 40, 8, None, 0.05, 0.7, 1e-3)
    three("pj2_first", 513, 40, 8, None, 0.04, 1.3, 1e-3)
    three("pj2_full", 1024, 24, 8, None, 0.03, 0.8, 2e-3)
    three("pj4_first", 1025, 24, 8, None, 0.05, 1.2, 2e-3)
    three("dots_one_trip", 2048, 12, 3, None, 0.02, 0.9, 3e-3)
    three("dots_two_trips", 2049, 12, 3, None, 0.02, 1.1, 4e-3)
    three("pj8_default", 4000, 6, 3, None, 0.02, 0.6, 4e-3)
    three("pj8_full", 4096, 5, 3, 3, 0.025, 1.4, 5e-3)
    three("pj12_first", 4097, 5, 3, 3, 0.02, 0.75, 3e-3)
    three("pj12_full", 6144, 5, 3, 2, 0.015, 1.25, 4e-3)
    three("pj16_first", 6145, 5, 3, 2, 0.02, 0.85, 7e-3)
    three("pj16_full", 8192, 3, 2, 1, 0.015, 1.15, 7e-3)
    three("pj20_first", 8193, 3, 2, 1, 0.01, 0.65, 5e-3)
    three("pj20_last_fit", 10234, 2, 1, 1, 0.0018, 1.35, 1.2e-3)
    three("nostage_ragged", 70, 19, 11, 0, 0.06, 0.55, 1e-3)
    three("nostage_big", 10300, 9, 2, None, 0.01, 0.95, 4e-3)
    three("one_group_uneven", 130, 13, 4, None, 0.07, 1.05, 1e-3)
    three("wide_batch", 600, 70, 5, None, 0.04, 0.9, 1e-3)
    out.append(Case("decay_store_tail", 33, 23, 5, 2, 0.5, 4, None, None, 0.08, 1.45, 2e-3, SEED,
                    len(out)))
    # m = 1 is contractive while eps·N/(2·signal_var) is well below 1: 0.034 here
    out.append(Case("two_launches", 8, 4097, 1, 1, 0.3, 241, None, None, 0.3, 0.5, 5e-6, SEED, len(out)))
    for name in GR.STEP_CASES:
        phi, y, sv, sth, m, _, decay, seed = GR.step_problem(name)
        eps = OLD_EPS[name]
        out.append(Case("old_" + name, phi.shape[0], phi.shape[1], m, 2, decay, 1, None, 3, sv, sth,
                        eps, seed, len(out)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
OLD = tuple(c.name for c in CASES if c.name.startswith("old_"))


# name -> (rows per group, groups of a full batch, LDS bytes, PJ): what the device has to report
# (tests/test_gpnt_step_cases.py derives each from the restatement of gpnt_layout below)
ROUTES = {
    "pj1_full": (32, 2, 136000, 1),
    "pj2_first": (32, 2, 136272, 2),
    "pj2_full": (16, 2, 139776, 2),
    "pj4_first": (16, 2, 139920, 4),
    "dots_one_trip": (8, 2, 147728, 4),
    "dots_two_trips": (8, 2, 147808, 8),
    "pj8_default": (4, 2, 160160, 8),
    "pj8_full": (3, 2, 131232, 8),
    "pj12_first": (3, 2, 131272, 12),
    "pj12_full": (2, 3, 147616, 12),
    "pj16_first": (2, 3, 147648, 16),
    "pj16_full": (1, 3, 131184, 16),
    "pj20_first": (1, 3, 131208, 20),
    "pj20_last_fit": (1, 2, 163824, 20),
    "nostage_ragged": (0, 0, 992, 0),
    "nostage_big": (0, 0, 82640, 0),
    "one_group_uneven": (13, 1, 14880, 0),
    "wide_batch": (32, 3, 159840, 2),
    "decay_store_tail": (5, 1, 1752, 0),
    "two_launches": (1, 1, 208, 0),
    "old_A": (25, 1, 15120, 0),
    "old_B": (16, 2, 150032, 4),
}


def nb(c):
    return -(-c.N // c.m)


def total(c):
    """Steps the device runs."""
    return c.epochs * nb(c)


def kept(c):
    """Stored steps that are held to the reference."""
    k = total(c) // c.store_every
    return k if c.keep is None else min(k, c.keep)


def steps(c):
    """Steps the reference takes: up to the last one held."""
    return kept(c) * c.store_every


# ---------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """(phi (n, N) column-major, y (N,)), read-only."""
    c = BY_NAME[name]
    if name in OLD:
        phi, y = GR.step_problem(name[len("old_"):])[:2]
    else:
        rng = np.random.default_rng(7100 + c.idx)
        phi = np.asfortranarray(math.sqrt(2.0 / c.n) * np.cos(rng.uniform(0, 2 * np.pi, (c.n, c.N))))
        y = phi.T @ rng.standard_normal(c.n) + 0.1 * rng.standard_normal(c.N)
    assert phi.shape == (c.n, c.N) and y.shape == (c.N,)
    phi.setflags(write=False)
    y.setflags(write=False)
    return phi, y


def digest(c):
    h = hashlib.sha256(repr(tuple(c)).encode())
    for a in inputs(c.name):
        a = np.asfortranarray(a)
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    return h.hexdigest()


# --------------------------------------------------------------------------- device layout restated
def _al16(x):
    return (x + 15) & ~15


def gpnt_layout(n, N, m, rows_cap=None):
    """gpt_amd/csrc/gpnt.hip's gpnt_layout: the byte offsets, rows per group, groups and bytes;
    `fit` is the number of rows that fit beside theta before any rule is applied."""
    mb = min(m, N)
    L = dict(o_theta=0)
    o = _al16(8 * n)
    L["o_idx"] = o
    o = _al16(o + 4 * mb)
    L["o_y"] = o
    o = _al16(o + 8 * mb)
    L["o_res"] = o
    o = _al16(o + 8 * mb)
    L["o_flag"] = o
    o = _al16(o + 4 * NW)
    L["o_phi"] = L["base"] = o
    row = 8 * n
    rows = L["fit"] = (LDS - o) // row if o < LDS else 0
    if rows >= mb:
        rows = mb
    elif rows > NW:
        rows -= rows % NW
    if rows_cap is not None and rows_cap >= 0:
        rows = min(rows, rows_cap)
    elif rows < mb and rows < MIN_ROWS:
        rows = 0
    L["rows"] = rows
    L["groups"] = -(-mb // rows) if rows else 0
    L["bytes"] = o + row * rows
    return L


def gpnt_carry(n):
    """gpnt.hip's gpnt_carry: the smallest listed PJ with n <= PJ·kNT, -1 when there is none."""
    for pj in CARRIES:
        if n <= pj * NT:
            return pj
    return -1


Route = collections.namedtuple("Route", "rows groups lds_bytes pj")


def route(c, rows=-1, n=None):
    """The route launch_gpnt_chain takes for the case (rows: another GPTSGLD_GPNT_ROWS than its own)."""
    n = c.n if n is None else n
    L = gpnt_layout(n, c.N, c.m, c.rows if rows == -1 else rows)
    pj = gpnt_carry(n) if L["groups"] > 1 else 0
    assert pj >= 0, (c.name, n)
    return Route(L["rows"], L["groups"], L["bytes"], pj)


# ------------------------------------------------------- the fp64 restatement, group by group (hooked)
# name -> the case it is named for (tests/test_gpnt_step_cases.py).  Every defect is planted whole
# (size 1) and at `size` = 1e-9: g, or the factor the defect is in, moved by that part of the
# difference between the defective and the right value.
DEFECTS = {
    "short_group_last_row_dropped": "pj8_default",
    "previous_groups_residuals": "pj1_full",
    "clamped_column_leaks": "pj2_first",
    "ragged_batch_N_over_m": "nostage_ragged",
    "eps_of_t_not_t_plus_1": "decay_store_tail",
    "second_trip_column_skipped": "dots_two_trips",
    "column_65_dropped": "wide_batch",
}
SMALL = 1e-9


def run_groups(c, defect=None, size=1.0, probe=None):
    """The step as gpnt_chain_kernel<PJ> takes it on the case's route, in float64: residuals by trips
    of DOT_SPAN columns, g group by group in the PJ slots of each of the NT threads (a slot past n
    reads the clamped column n − 1 and is not written out), one group for PJ = 0.  Returns the held
    steps (n, kept); NaN and inf stay as they come.  probe='first': dict(grad_rms, data_rms,
    noise_rms) of step 1."""
    assert defect is None or defect in DEFECTS
    phi, y = inputs(c.name)
    n, N, m = c.n, c.N, c.m
    rt = route(c)
    G = rt.rows if rt.groups > 1 else max(m, 1)
    slots = np.arange(max(rt.pj, -(-n // NT)) * NT)          # thread tid, slot p: column tid + NT·p
    cols = np.minimum(slots, n - 1)
    theta = c.sigma_theta * px.normals(n, c.seed, 0, px.THETA_INIT, 0)
    store = np.zeros((n, kept(c)), order="F")
    order = np.arange(N)
    t = 0
    with np.errstate(all="ignore"):
        for epoch in range(1, c.epochs + 1):
            order = order[px.randperm(N, c.seed, epoch - 1)]
            for batch in range(1, nb(c) + 1):
                if t == steps(c):
                    return store
                t += 1
                idx = order[m * (batch - 1): min(m * batch, N)]
                B = len(idx)
                pb = phi[:, idx]
                dot = np.zeros(B)
                for j0 in range(0, n, DOT_SPAN):
                    j1 = min(n, j0 + DOT_SPAN)
                    dot += pb[j0:j1].T @ theta[j0:j1]
                res = y[idx] - dot
                res_bad = res
                if defect == "second_trip_column_skipped" and n > DOT_SPAN:
                    res_bad = res + pb[DOT_SPAN] * theta[DOT_SPAN]
                if defect == "column_65_dropped" and B > 64:
                    res_bad = res.copy()
                    res_bad[64] = 0.0
                g = np.zeros(slots.size)
                g_bad = np.zeros(slots.size)
                for i0 in range(0, B, G):
                    cnt = min(G, B - i0)
                    rows = pb[:, i0:i0 + cnt][cols]
                    g += rows @ res[i0:i0 + cnt]
                    r, use = res_bad[i0:i0 + cnt], cnt
                    if defect == "previous_groups_residuals" and i0 > 0:
                        r = res[i0 - G:i0 - G + cnt]
                    if defect == "short_group_last_row_dropped" and cnt < G and rt.groups > 1:
                        use = cnt - 1
                    g_bad += rows[:, :use] @ r[:use]
                if defect == "clamped_column_leaks" and slots.size > n:
                    g_bad[n - 1] += g_bad[n]                    # slot n holds column n − 1's sum
                g = (g + size * (g_bad - g))[:n] if defect else g[:n]
                cN = N / B
                if defect == "ragged_batch_N_over_m":
                    cN += size * (N / m - cN)
                eps = c.eps * float(t) ** (-c.decay)
                if defect == "eps_of_t_not_t_plus_1":
                    bad = float(c.eps * np.float64(t - 1) ** (-c.decay))     # inf at the first step
                    if size == 1.0:
                        eps = bad
                    elif math.isfinite(bad):
                        eps += size * (bad - eps)
                data = cN * g / c.signal_var
                grad = -theta / c.sigma_theta ** 2 + data
                noise = px.normals(n, c.seed, t - 1, px.THETA_NOISE, 0)
                if probe == "first":
                    rms = lambda v: float(np.sqrt(np.mean(v ** 2)))             # noqa: E731
                    return dict(grad_rms=rms(grad), data_rms=rms(data), noise_rms=rms(noise))
                theta = theta + (eps * grad / 2 + math.sqrt(eps) * noise)
                if t % c.store_every == 0:
                    store[:, t // c.store_every - 1] = theta
    return store


def run_numpy(c):
    """The restatement of record: oracle.gpt_sgld_ref.GPNT_SGLD, thinned by gpnt_ref.gpnt_sgld_chains;
    the held steps (n, kept)."""
    phi, y = inputs(c.name)
    store, status = GR.gpnt_sgld_chains(phi, y, [c.signal_var], [c.sigma_theta], c.m, [c.eps], c.decay,
                                        0, c.epochs, [c.seed], store_every=c.store_every)
    assert not status.any()
    return store[:, :kept(c), 0]


def shares(c):
    """(eps/2·rms grad, eps/2·rms of its data term) / (sqrt(eps)·rms noise) at step 1: the
    gradient's part of the move over the noise's."""
    p = run_groups(c, probe="first")
    f = c.eps / 2 / (math.sqrt(c.eps) * p["noise_rms"])
    return f * p["grad_rms"], f * p["data_rms"]


# ------------------------------------------------------------------------------ mpmath reference
def compute(c):
    """[held step][n] of mpf: the case at MP_DIGITS digits (module docstring)."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _compute(c, mp)


def _compute(c, mp):
    f = lambda v: mp.mpf(float(v))                                            # noqa: E731
    phi, y = inputs(c.name)
    n, N, m = c.n, c.N, c.m
    col = {}                                              # columns of phi as they are first used
    th = [f(v) for v in c.sigma_theta * px.normals(n, c.seed, 0, px.THETA_INIT, 0)]
    eps_theta, decay, sv, s2 = f(c.eps), f(c.decay), f(c.signal_var), f(c.sigma_theta) ** 2
    order = np.arange(N)
    out, t = [], 0
    for epoch in range(1, c.epochs + 1):
        order = order[px.randperm(N, c.seed, epoch - 1)]
        for batch in range(1, nb(c) + 1):
            if t == steps(c):
                return out
            t += 1
            idx = [int(i) for i in order[m * (batch - 1): min(m * batch, N)]]
            B = len(idx)
            for i in idx:
                if i not in col:
                    col[i] = [f(v) for v in phi[:, i]]
            eps = eps_theta * mp.mpf(t) ** (-decay)
            sq = mp.sqrt(eps)
            res = [f(y[i]) - mp.fdot(col[i], th) for i in idx]
            cN = mp.mpf(N) / B
            xi = SC._mp_normals(n, c.seed, t - 1, px.THETA_NOISE, 0)
            th = [th[j] + (eps * (-th[j] / s2 + cN * mp.fdot([col[i][j] for i in idx], res) / sv) / 2
                           + sq * xi[j]) for j in range(n)]
            if t % c.store_every == 0:
                out.append(th)
    return out


def pack(c, ref):
    """compute()'s result as the fixture's arrays {suffix: array}."""
    import mpmath as mp
    sel = select(c.n, c.n)
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
    """dict(hi, lo, scale, sel, u, bar, share, share_g) of a case from the committed file; the digest
    has to be the one of the inputs this machine regenerates.  Shared and read-only."""
    st, c = _stored(), BY_NAME[name]
    if str(st.get(name + "_digest")) != digest(c):
        raise AssertionError("tests/golden/gpnt_step_mp.npz does not belong to these inputs: %s" % name)
    u = float(st[name + "_u"])
    return dict(hi=st[name + "_hi"], lo=st[name + "_lo"].astype(np.float64), scale=st[name + "_scale"],
                sel=select(c.n, c.n), u=u, bar=MARGIN * u, share=float(st[name + "_share"]),
                share_g=float(st[name + "_share_g"]))


def step_errors(store, ref):
    """store (n, kept) -> per held step max|store − ref| over the kept entries over that step's
    max|theta|; inf for a step that is not finite."""
    got = np.asarray(store).T[:, ref["sel"]]
    assert got.shape == ref["hi"].shape, (got.shape, ref["hi"].shape)
    with np.errstate(all="ignore"):
        err = np.abs((got - ref["hi"]) - ref["lo"]).max(axis=1) / ref["scale"]
    return np.where(np.isfinite(got).all(axis=1), err, np.inf)


def error(store, ref):
    return float(step_errors(store, ref).max())
