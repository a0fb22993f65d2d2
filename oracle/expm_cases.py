"""Input matrices for the device expm unit tests (tests/test_gpu_expm.py) and their CPU-side
conditions (tests/test_oracle.py), with the branch each matrix takes in the Padé
scaling-and-squaring of ``gpt_sgld_ref.expm``: the degree, the squaring count, whether the Padé
denominator V − U is column diagonally dominant (the device's register LU without pivoting) and
whether partial pivoting permutes its rows (the device's pivoting fallback).  Everything here is
derived from the oracle's coefficient table and thresholds, never from the device.

Test infrastructure: pure numpy / scipy / mpmath, no GPU.
"""
import functools
import hashlib
import math
import os

import numpy as np
import scipy.linalg

from . import gpt_sgld_ref as R

# gpt_debug_expm's (mode, nn) table (include/gptsgld.h): every size the samplers instantiate,
# 2r for the geodesic block and r for expm(−tA), r in {1,2,3,4,5,6,8,10,12,15,16,20}
GEOD_SIZES = (12, 16, 20, 24, 30, 32, 40)
MODE_SIZES = {
    0: (6, 8, 10, 12, 15, 16, 20, 24, 30, 32, 40),
    1: (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 16, 20, 24, 30, 32, 40),
    3: (40,),
    4: GEOD_SIZES,
}
ALL_SIZES = MODE_SIZES[1]
MODE_NN = [(mode, nn) for mode in sorted(MODE_SIZES) for nn in MODE_SIZES[mode]]

# the branch thresholds of gpt_sgld_ref.expm (Julia Base 0.3 expm!); pade_parts() below is checked
# against R.expm bit for bit (tests/test_oracle.py), so a drift between the two is a test failure
DEGREE_BOUNDS = ((0.015, 3), (0.25, 5), (0.95, 7), (2.1, 9))
THETA13 = 5.4

GEODESIC_NORMS = (0.01, 0.2, 0.6, 1.5, 2.0, 4.4, 5.3, 9.0, 40.0, 1e3)
LARGE_NORMS = (1e3, 1e5)
SWAP_NORMS = (4.4, 5.3)
# a 1 × 1 skew matrix is zero and e^-1000 underflows: nn = 1 takes [[−x]] with 700 (s = 8, e^-700
# is a normal double) in place of 1e3
NN1_NORMS = GEODESIC_NORMS[:-1] + (700.0,)
DIRECT_BAR_NORM = 40.0     # up to here the device also meets 1e-12 against R.expm directly


def one_norm(X):
    return np.abs(X).sum(axis=0).max() if X.size else 0.0


def branch_of_norm(nA):
    """(Padé degree, squarings s) of a matrix of 1-norm nA."""
    for bound, deg in DEGREE_BOUNDS:
        if nA <= bound:
            return deg, 0
    s = math.log2(nA / THETA13)
    return 13, (int(math.ceil(s)) if s > 0 else 0)


def threshold_margin(nA):
    """Smallest relative distance of nA to a branch threshold (0.015, 0.25, 0.95, 2.1, 5.4·2^k)."""
    ths = [b for b, _ in DEGREE_BOUNDS] + [THETA13 * 2.0 ** k for k in range(0, 40)]
    return min(abs(nA - t) / t for t in ths)


def pade_parts(X):
    """(degree, s, V − U, V + U) as gpt_sgld_ref.expm forms them, from its _PADE table."""
    A = np.array(X, dtype=np.float64)
    Id = np.eye(A.shape[0])
    deg, s = branch_of_norm(one_norm(A))
    C = R._PADE[deg]
    if deg < 13:
        A2 = A @ A
        P = Id.copy()
        U = C[1] * P
        V = C[0] * P
        for k in range(1, (len(C) - 1) // 2 + 1):
            P = P @ A2
            U = U + C[2 * k + 1] * P
            V = V + C[2 * k] * P
        U = A @ U
    else:
        if s > 0:
            A = A / (2.0 ** s)
        A2 = A @ A
        A4 = A2 @ A2
        A6 = A2 @ A4
        U = A @ (A6 @ (C[13] * A6 + C[11] * A4 + C[9] * A2)
                 + C[7] * A6 + C[5] * A4 + C[3] * A2 + C[1] * Id)
        V = A6 @ (C[12] * A6 + C[10] * A4 + C[8] * A2) + C[6] * A6 + C[4] * A4 + C[2] * A2 + C[0] * Id
    return deg, s, V - U, V + U


def expm_from_parts(X):
    """The oracle's result rebuilt from pade_parts (equals R.expm(X) bit for bit)."""
    deg, s, M, P = pade_parts(X)
    E = np.linalg.solve(M, P)
    for _ in range(s):
        E = E @ E
    return E


def diag_dominant(M):
    """Strict column diagonal dominance, the device's test for the LU without pivoting."""
    d = np.abs(np.diag(M))
    return bool(np.all(d > np.abs(M).sum(axis=0) - d))


def pivoting_permutes(M):
    """Whether Gaussian elimination with partial pivoting swaps a row of M."""
    P = scipy.linalg.lu(M)[0]
    return not np.array_equal(P, np.eye(M.shape[0]))


def branch(X):
    """dict(norm, degree, s, dd, swaps) of the matrix X."""
    deg, s, M, _ = pade_parts(X)
    return dict(norm=one_norm(X), degree=deg, s=s, dd=diag_dominant(M), swaps=pivoting_permutes(M))


def _scaled(T, target):
    return T * (target / one_norm(T))


def _skew(rng, nn):
    B = rng.standard_normal((nn, nn))
    return (B - B.T) / 2


def geodesic_block(rng, nn, sign=-1.0):
    """[A ∓S; I A] with A skew and S symmetric PSD, r = nn/2: what geod exponentiates (sign −1)."""
    r = nn // 2
    A = _skew(rng, r)
    W = rng.standard_normal((3 * r, r))
    return np.block([[A, sign * (W.T @ W)], [np.eye(r), A]])


def _swap_matrix(nn, target, seed):
    """A matrix at 1-norm `target` (degree 13, s = 0) whose Padé denominator partial pivoting
    permutes: a shifted identity plus dense noise, the noise shrunk until the predicate holds
    (nn = 40 needs about 0.5/nn); dense random matrices at nn = 2 and 3."""
    for attempt in range(64):
        rng = np.random.default_rng([seed, nn, attempt])
        if nn <= 3:
            X = _scaled(rng.standard_normal((nn, nn)), target)
        else:
            noise = 0.05 if attempt == 0 else 0.5 / nn / attempt
            X = _scaled(np.roll(np.eye(nn), 1, 0) + noise * rng.standard_normal((nn, nn)), target)
        _, _, M, _ = pade_parts(X)
        if not diag_dominant(M) and pivoting_permutes(M):
            return X
    raise AssertionError("no row-swapping matrix found at nn = %d, norm %g" % (nn, target))


@functools.lru_cache(maxsize=None)
def cases(nn):
    """The finite input matrices of size nn: a tuple of (name, family, X).  Families:
    'geodesic' (t·[A −S; I A] at even nn, and the skew t·A that expm(−tA) receives at the r sizes
    nn <= 20; 1-norms GEODESIC_NORMS), 'large' (skew at LARGE_NORMS: s = 8 and 15 with an
    orthogonal result) and 'swap' (partial pivoting permutes V − U; SWAP_NORMS)."""
    out = []
    if nn == 1:
        for t in NN1_NORMS:
            out.append(("neg_%g" % t, "geodesic", np.array([[-t]])))
        return tuple(out)
    rng = np.random.default_rng(1000 + nn)
    for t in GEODESIC_NORMS:
        if nn % 2 == 0:
            out.append(("block_%g" % t, "geodesic", _scaled(geodesic_block(rng, nn), t)))
        if nn <= 20:
            out.append(("skew_%g" % t, "geodesic", _scaled(_skew(rng, nn), t)))
    for t in LARGE_NORMS:
        out.append(("large_%g" % t, "large", _scaled(_skew(rng, nn), t)))
    for t in SWAP_NORMS:
        out.append(("swap_%g" % t, "swap", _swap_matrix(nn, t, 7)))
    return tuple(out)


def nonfinite_cases(nn):
    """Matrices with one Inf or one NaN entry, once in column 0 and once in the last column (the
    same column at nn = 1), on a finite geodesic-family background."""
    base = cases(nn)[3][2]
    out = []
    for val, tag in ((np.inf, "inf"), (np.nan, "nan")):
        for col in sorted({0, nn - 1}):
            X = base.copy()
            X[(nn - 1) // 2, col] = val
            out.append(("%s_col%d" % (tag, col), X))
    return out


OVERFLOW_SHIFT, BOUNDED_SHIFT = 1500.0, 400.0


def overflow_cases(nn):
    """(X_overflow, X_bounded) for nn >= 2: G + μ·I with G the geodesic-family matrix of 1-norm 2
    (the block at even nn, the skew matrix at odd nn) and μ = 1500 and 400.  The geodesic family
    alone has a purely imaginary spectrum and a bounded exponential at every norm, so the growth
    comes from the shift: exp(G + μI) = e^μ·exp(G), exp(G) has entries of both signs and a largest
    one between 1/nn and e², so the largest entry of the first is above e^1500/nn > 1e600 (the
    squarings overflow to Inf and then form Inf − Inf) and that of the second is below
    e^402 < 1e175.  (A 1 × 1 exponential overflows to Inf without ever forming a NaN.)"""
    rng = np.random.default_rng(2000 + nn)
    G = _scaled(geodesic_block(rng, nn) if nn % 2 == 0 else _skew(rng, nn), 2.0)
    Id = np.eye(nn)
    return G + OVERFLOW_SHIFT * Id, G + BOUNDED_SHIFT * Id


# ------------------------------------------------------------------------------ mpmath reference
MP_DIGITS = 60
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def expm_mpf(X):
    """exp(X) by mpmath.expm at MP_DIGITS digits as an mpmath matrix; X holds doubles or mpf."""
    import mpmath
    with mpmath.workdps(MP_DIGITS):
        return mpmath.expm(mpmath.matrix(X.tolist()))


def expm_mp(X):
    """exp(X) by mpmath.expm at MP_DIGITS digits, rounded to a pair of float64 arrays (hi, lo)
    with hi + lo = exp(X) to about 1e-23 relative (lo is kept as float32 in the fixtures)."""
    import mpmath
    n = X.shape[0]
    with mpmath.workdps(MP_DIGITS):
        Emp = expm_mpf(X)
        hi = np.array([[float(Emp[i, j]) for j in range(n)] for i in range(n)])
        lo = np.array([[float(Emp[i, j] - mpmath.mpf(hi[i, j])) for j in range(n)] for i in range(n)])
    return hi, lo.astype(np.float32).astype(np.float64)


def digest(X):
    return hashlib.sha256(np.ascontiguousarray(X, dtype=np.float64).tobytes()).hexdigest()


def golden_path(nn):
    return os.path.join(GOLDEN, "expm_mp_nn%02d.npz" % nn)


@functools.lru_cache(maxsize=None)
def mp_reference(nn):
    """(hi, lo) of mpmath's exp(X) for every matrix of cases(nn), in order.  mpmath takes seconds
    per matrix from nn = 30 up, so the results are committed (tests/golden/expm_mp_nnXX.npz, written
    by tests/golden/make_expm_golden.py) under the SHA-256 of the input matrix; a matrix whose
    digest is not in the file (another random stream) is computed on the spot."""
    stored = {}
    if os.path.exists(golden_path(nn)):
        with np.load(golden_path(nn)) as f:
            for k, d in enumerate(f["digest"]):
                stored[str(d)] = (f["hi"][k], f["lo"][k].astype(np.float64))
    return tuple(stored.get(digest(X)) or expm_mp(X) for _, _, X in cases(nn))


def err_vs_mp(E, ref):
    """max|E − E_mp| / max|E_mp| over the columns E holds (all, or the first ones), E_mp = hi + lo.
    E − hi is exact in floating point wherever the two agree to a factor of two."""
    hi, lo = ref
    c = E.shape[1]
    return float(np.abs((E - hi[:, :c]) - lo[:, :c]).max() / np.abs(hi).max())
