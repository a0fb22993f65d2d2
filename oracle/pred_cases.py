"""Cases, inputs, mpmath references and error bounds of the prediction kernels
(gpt_amd/csrc/pred.hip; tests/test_gpu_pred.py on the device, tests/test_pred_cases.py on the CPU).

CASES lists one shape (n, D, Ntest, r, Q, S) per dispatch branch of launch_pred_mfma and per tile
edge of pred_temp_mfma_kernel, with the route the dispatch gives it (kind, template dimension, rows
per wave: the first three entries of gpt_pred_last_route).  Inputs are regenerated from the shape
and a seed, never stored:

    phi = feature(X, ls, 1, sqrt(n / Q^(1/D)), Z, b)    X, Z standard normal, b uniform in [0, 2π)
    U   = standard normal / sqrt(n)                     (no Stiefel U: n < r is allowed)
    w   = standard normal
    I   = integers in 1..r, (Q, D)                      (duplicate entries are fine for prediction)

The reference is f[s, i] = Σ_q w_q·Π_k t[k, I[q,k]], t[k, l] = Σ_j U[j, l, k]·phi[j, k, i], of those
doubles in mpmath at MP_DIGITS digits, kept as a double-double (hi float64, lo float32).  The bound
E[s, i] is derived, not measured.  With u = 2^-53 and γ_n = n·u / (1 − n·u), any order of summing
the n products of t (FMA or not, MFMA blocks or a butterfly) gives t·(1 + δ), |δ| ≤ γ_n·T̄/|t|,
T̄ = Σ_j |U|·|phi|.  A term V_q = w_q·Π_k t then carries D − 1 products of the factors, one with w
and, on its way into f, at most Q + 15 additions (Q entries and up to 16 wave partials), each
(1 + δ), |δ| ≤ u: c = D + Q + 18 covers them with room for the pair tables' association.  So

    E_i = Σ_q |V_q,i|·((1 + u)^c · Π_k (1 + γ_n·T̄_k/|t_k|) − 1)

holds for every summation order, for FMA or separate rounding, and for the pairwise association of
the D factors in the pair-table kernel.  It is evaluated in mpmath and rounded up to a double.  A
slack bound would hide errors, so every case must satisfy max E ≤ SLACK·max|f|
(tests/test_pred_cases.py); a case that does not is reseeded or shrunk.

The pairs are committed in tests/golden/pred_mp.npz (written by tests/golden/make_pred_golden.py)
under the SHA-256 of the case's inputs; a case whose digest is not in the file is recomputed with
mpmath on the spot.  Nothing here comes from the device.

Test infrastructure: pure numpy / mpmath, no GPU.
"""
import collections
import functools
import hashlib
import math
import os

import numpy as np

from . import gpt_sgld_ref as R

MP_DIGITS = 50
SLACK = 1e-11            # max E <= SLACK·max|f|: the condition on the fixture
BAR = 1e-12              # the project's prediction bar (tests/test_gpu_parity.py): |Δ| <= BAR·max|f|
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                      "pred_mp.npz")

PAIRS, ROWS_PF, ROWS, DIRECT = 0, 1, 2, 4            # the kinds of gpt_pred_last_vphase

Case = collections.namedtuple("Case", "group shape rows kind tdim npw seed")


def _c(group, shape, kind, tdim, npw=0, rows=False, seed=0):
    return Case(group, tuple(shape), rows, kind, tdim, npw, seed)


def _cases():
    out = []
    for s in ((8, 1, 70, 5, 5, 2), (8, 2, 70, 5, 5, 2), (8, 2, 70, 1, 1, 2)):
        out.append(_c("pairs, one table", s, PAIRS, 1))
    out.append(_c("pairs, eight tables", (8, 15, 70, 5, 40, 2), PAIRS, 8))    # odd last dimension
    out.append(_c("pairs, eight tables", (8, 16, 70, 3, 40, 2), PAIRS, 8))
    out.append(_c("pairs NT = 6, 7", (8, 11, 70, 2, 40, 2), PAIRS, 6))
    out.append(_c("pairs NT = 6, 7", (8, 13, 70, 4, 40, 2), PAIRS, 7))
    out.append(_c("tables over 96 KB", (8, 16, 70, 5, 40, 2), ROWS_PF, 0, 10))
    for s in ((20, 1, 70, 8, 8, 3), (20, 1, 70, 8, 3, 2),                     # fewer entries than waves
              (64, 11, 70, 12, 50, 3), (64, 13, 70, 12, 50, 3)):
        out.append(_c("run-time D", s, ROWS_PF, 0, 10))
    for D in (2, 4, 5, 6, 7, 9, 10, 12):
        out.append(_c("fixed D", (24, D, 70, 6, 30, 2), ROWS_PF, D, 10))
    out.append(_c("16 rows per wave", (64, 12, 70, 16, 50, 3), ROWS_PF, 0, 16))
    out.append(_c("16 rows per wave", (64, 16, 70, 16, 8, 2), ROWS_PF, 0, 16))   # D·r = 256
    out.append(_c("over 256 rows", (64, 14, 70, 20, 8, 2), ROWS, 0))
    out.append(_c("w loaded at park", (24, 4, 70, 6, 1100, 2), ROWS_PF, 4, 10))
    out.append(_c("w loaded at park", (24, 4, 70, 6, 1025, 2), ROWS_PF, 4, 10))
    out.append(_c("forced rows at r <= 5", (8, 2, 70, 1, 1, 2), ROWS_PF, 2, 10, rows=True))
    out.append(_c("forced rows at r <= 5", (16, 3, 70, 5, 30, 2), ROWS_PF, 3, 10, rows=True))
    for n in (1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33):
        out.append(_c("GEMM K edge", (n, 2, 20, 2, 4, 3), PAIRS, 1))
    for S in EDGE_SIZES:
        out.append(_c("GEMM column edge", (6, 2, 20, 1, 1, S), PAIRS, 1))
    for Nt in EDGE_SIZES:
        out.append(_c("GEMM row edge", (6, 2, Nt, 2, 4, 2), PAIRS, 1))
    out.append(_c("XCD numbering", (6, 3, 300, 2, 6, 2), PAIRS, 2))           # 9 workgroup tiles
    out.append(_c("XCD numbering", (6, 1, 20, 2, 2, 1), PAIRS, 1))            # 1
    return tuple(out)


EDGE_SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
CASES = _cases()
GROUPS = tuple(dict.fromkeys(c.group for c in CASES))
# the cases the direct kernels (GPTSGLD_PRED=direct) are run on
DIRECT_SHAPES = ((8, 2, 70, 1, 1, 2), (16, 3, 70, 5, 30, 2), (64, 14, 70, 20, 8, 2))
# the existing tests that hold what CASES leaves out (tests/test_pred_cases.py)
HELD_ELSEWHERE = {
    ("DD", 8): "tests/test_gpu_parity.py::test_pred_stacked_samples_mfma[150-8-130-20-200-4]",
    ("NT", 3): "tests/test_gpu_parity.py::test_pred_on_reference_fixture[5D-0.03125]",
    ("NT", 4): "tests/test_gpu_parity.py::test_pred_stacked_samples_mfma[500-8-700-5-200-40]",
    ("NT", 5): "tests/test_gpu_parity.py::test_pred_on_reference_fixture[10D-0.0258]",
}


def case_id(c):
    return "%d-%d-%d-%d-%d-%d%s" % (c.shape + ("-rows" if c.rows else "",))


def find(shape, rows=None):
    """The case of a shape (the one with rows forced or not, where given)."""
    for c in CASES:
        if c.shape == tuple(shape) and rows in (None, c.rows):
            return c
    raise KeyError(shape)


# ------------------------------------------------------------------------- the dispatch, restated
def gemm_tiles(shape):
    """Workgroup tiles of pred_temp_mfma_kernel<V2, 4, 4> for one pass over all S samples."""
    n, D, Nt, r, Q, S = shape
    return ((S * r + 127) // 128) * ((Nt + 127) // 128) * D


def expected_route(shape, rows=False):
    """(kind, tdim, npw) of launch_pred_mfma / launch_vphase_rows for a shape, from their conditions
    (pairs: r <= 5, ⌈D/2⌉ <= 8 tables of at most 96 KB; the persistent rows kernel: D·r <= 256 and
    its LDS within 160 KB, 10 rows per wave up to D·r = 160)."""
    n, D, Nt, r, Q, S = shape
    nt = (D + 1) // 2
    plds = 8 * ((D // 2) * r * r + (D & 1) * r) * 64 + 8 * 4 * 64
    if not rows and r <= 5 and nt <= 8 and plds <= 96 * 1024:
        return PAIRS, nt, 0
    pf_lds = 8 * D * r * 64 + 8 * 16 * 64 + 4 * ((Q * D + 3) & ~3) + 8 * Q
    if D * r <= 256 and pf_lds <= 160 * 1024:
        if D * r <= 160:
            return ROWS_PF, (D if D in FIXED_D else 0), 10
        return ROWS_PF, 0, 16
    return ROWS, 0, 0


FIXED_D = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12)            # pred.hip's RowsPfDs (launch_vphase_rows)


def rows_pf_grid(shape, cus):
    """The grid launch_rows_pf picks on a device of `cus` CUs before it is capped at the tile
    count: as many workgroups as their LDS lets every CU hold."""
    n, D, Nt, r, Q, S = shape
    lds = 8 * D * r * 64 + 8 * 16 * 64 + 4 * ((Q * D + 3) & ~3) + 8 * Q
    return max(1, (160 * 1024) // lds) * cus


def temp_bytes(shape):
    """One sample's temp in launch_pred_mfma (per_sample)."""
    n, D, Nt, r, Q, S = shape
    return 8 * D * r * ((Nt + 63) // 64 * 64)


def steady_shape(n, D, Nt, r, Q, cus, ratio=2.15, cap=256 << 20):
    """(n, D, Ntest, r, Q, S) with at least ratio × the persistent kernel's grid in (sample, 64-row)
    tiles, so some workgroups run two tiles and some three; Ntest is lowered (never the ratio)
    while the temp would pass `cap` bytes."""
    while True:
        nti = (Nt + 63) // 64
        S = -(-int(math.ceil(ratio * rows_pf_grid((n, D, Nt, r, Q, 1), cus))) // nti)
        shape = (n, D, Nt, r, Q, S)
        if S * temp_bytes(shape) <= cap or Nt <= 64:
            return shape
        Nt = max(64, Nt // 2)


# ---------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _inputs(shape, seed):
    n, D, Nt, r, Q, S = shape
    rng = np.random.default_rng((20261, seed) + tuple(shape))
    X = rng.standard_normal((Nt, D))
    Z = rng.standard_normal((n, D))
    b = 2 * np.pi * rng.random((n, D))
    ls = 1.0 + 0.1 * rng.random(D)
    scale = math.sqrt(n / Q ** (1.0 / D))
    phi = R.feature(X, ls, 1.0, scale, Z, b)
    U = np.asfortranarray(rng.standard_normal((n, r, D, S)) / math.sqrt(n))
    w = np.asfortranarray(rng.standard_normal((Q, S)))
    I = np.asfortranarray(rng.integers(1, r + 1, (Q, D)).astype(np.int32))
    y = rng.standard_normal(Nt)
    out = dict(X=X, Z=Z, b=b, ls=ls, scale=scale, phi=phi, U=U, w=w, I=I, y=y)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def inputs(c):
    """The inputs of a case (read-only arrays): X (Ntest, D), Z, b (n, D), ls (D), scale,
    phi (n, D, Ntest), U (n, r, D, S), w (Q, S), I (Q, D) in 1..r, y (Ntest)."""
    return _inputs(c.shape, c.seed)


def oracle_pred(c):
    """The numpy oracle's prediction of every sample, (S, Ntest)."""
    p = inputs(c)
    return np.stack([R.pred(p["w"][:, s], p["U"][..., s], p["I"], p["phi"])
                     for s in range(c.shape[5])])


def key(c):
    return "p%d_" % c.seed + "_".join(str(v) for v in c.shape)


def digest(c):
    p = inputs(c)
    h = hashlib.sha256(key(c).encode())
    for name in ("phi", "U", "w", "I"):
        a = np.asfortranarray(p[name])
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    return h.hexdigest()


# ------------------------------------------------------------------------------ mpmath reference
def compute(c):
    """(hi, lo, E) of a case by mpmath, each (S, Ntest): hi + lo = f to about 2^-77 relative (lo
    rounded to float32), E the bound of the module docstring rounded up to a double."""
    import mpmath as mp
    n, D, Nt, r, Q, S = c.shape
    p = inputs(c)
    phi, U, w, I0 = p["phi"], p["U"], p["w"], p["I"] - 1
    hi = np.empty((S, Nt)); lo = np.empty((S, Nt)); E = np.empty((S, Nt))
    with mp.workdps(MP_DIGITS):
        f = mp.mpf
        u = f(2) ** -53
        gam = n * u / (1 - n * u)
        growth = (1 + u) ** (D + Q + 18)
        used = sorted({(k, int(I0[q, k])) for q in range(Q) for k in range(D)})
        mphi = [[[f(float(phi[j, k, i])) for j in range(n)] for k in range(D)] for i in range(Nt)]
        for s in range(S):
            mU = {(k, l): [f(float(U[j, l, k, s])) for j in range(n)] for k, l in used}
            aU = {kl: [abs(v) for v in col] for kl, col in mU.items()}
            mw = [f(float(w[q, s])) for q in range(Q)]
            for i in range(Nt):
                t, rho = {}, {}
                for k, l in used:
                    col = mphi[i][k]
                    t[k, l] = mp.fdot(mU[k, l], col)
                    tbar = mp.fdot(aU[k, l], [abs(v) for v in col])
                    rho[k, l] = 1 + gam * tbar / abs(t[k, l])
                fs, es = f(0), f(0)
                for q in range(Q):
                    v, g = mw[q], growth
                    for k in range(D):
                        kl = (k, int(I0[q, k]))
                        v *= t[kl]
                        g *= rho[kl]
                    fs += v
                    es += abs(v) * (g - 1)
                hi[s, i] = float(fs)
                lo[s, i] = float(fs - f(hi[s, i]))
                e = float(es)
                E[s, i] = e if f(e) >= es else np.nextafter(e, np.inf)
    return hi, lo.astype(np.float32).astype(np.float64), E


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def _reference(shape, seed):
    c = Case("", shape, False, 0, 0, 0, seed)
    st, k = _stored(), key(c)
    if str(st.get(k + "_digest")) == digest(c):
        out = st[k + "_hi"], st[k + "_lo"].astype(np.float64), st[k + "_E"]
    else:
        out = compute(c)
    for a in out:
        a.setflags(write=False)
    return out


def reference(c):
    """(hi, lo, E) of a case, each (S, Ntest), from the committed file where the case's digest is
    there, else by mpmath.  Shared and read-only."""
    return _reference(c.shape, c.seed)


def err_abs(out, ref):
    """|out − (hi + lo)|; out − hi is exact wherever the two agree to a factor of two."""
    hi, lo = ref[0], ref[1]
    return np.abs((np.asarray(out, dtype=np.float64) - hi) - lo)
