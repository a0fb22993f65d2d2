"""Cases, inputs, the mpmath reference and the CPU-side measurements of the exact-conditional
samplers' tests (tests/test_gpu_gibbs.py on the device, tests/test_gibbs_cases.py on the CPU): the
tensor-GP Gibbs sweep and geodesic Monte Carlo of gpt_amd/csrc/tgp.hip, the MovieLens Gibbs sweeps of
gpt_amd/csrc/cf.hip and the Gaussian draw they share, held to a 50-digit reference at rounding level,
in the shape of oracle/step_cases.py and oracle/cf_cases.py (storage hi float64 + lo float32, the
margin MARGIN).

Four families, each case regenerated from (shape, seed) and identified by a SHA-256 digest:

  tgp   (n, D, N, r, q, σ, sweeps), burnin 0: W and U of every sweep.  The reference's inputs are the
        feature array b (n, D, N) and the whitened targets as gpt_sgld_ref makes them from X and y
        (the device gets X and y and maps its own features, which have their own tests); I is drawn
        on the TGP_I stream or fixed.  The sampler has no injected state: the reference draws U on
        the TGP_U_INIT streams in mpmath.
  gmc   (n, D, N, r, Q, L, epochs, σ², ε), seed 7, the problem of tests/test_gpu_parity.py's
        _gmc_problem, from R.init_state's w and U (injected: no polar-factor difference is charged):
        w, U and the acceptance probability of every epoch.
  mlg   GPT_fullw_gibbs / GPT_fixw_gibbs on a synthetic rating design (design()): rows of one side
        with 0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128 and 130 ratings (592 in all) over 140 rows of the
        other side, as it is and transposed, and 16 ratings of 3 users; w, U, V, testpred_store and
        both RMSEs of every stored sweep; U and V are drawn on the CFG_INIT streams in mpmath.
  draw  gpt_debug_gaussian_draw alone: out = L⁻ᵀz + M⁻¹x on the matrices of
        tests/test_gpu_movielens.py::test_gaussian_draw_blocked_cholesky_and_solves.

The reference (compute) is the code of this file (_run_tgp, _run_gmc, _run_mlg, _run_draw: the
formulas of gpt_sgld_ref.GPT_inf / GPT_GMC and movielens_ref.GPT_fullw_gibbs) on the exact doubles of
the inputs in mpmath at MP_DIGITS digits: normals by Box–Muller in mpmath from the Philox words,
Cholesky and both triangular solves in mpmath, the true matrix exponential with geodboth's end point
and velocity.  The same code on float64 (run_f64) carries the defect table (DEFECTS); run_numpy is
the restatement of record (R.GPT_inf, R.GPT_GMC, M.GPT_fullw_gibbs / M.GPT_fixw_gibbs, numpy.linalg
for the draw), whose error against mpmath is u.

Nothing here comes from the device.  Test infrastructure: numpy / mpmath, no GPU.
"""
import collections
import functools
import hashlib
import math
import os

import numpy as np

from . import gpt_sgld_ref as R
from . import movielens_ref as M
from . import philox as px
from . import step_cases as SC

MP_DIGITS = SC.MP_DIGITS
MARGIN = SC.MARGIN
GOLDEN = os.path.join(os.path.dirname(SC.GOLDEN), "gibbs_mp.npz")

FAMILIES = ("tgp", "gmc", "mlg", "draw")
QUANTITIES = {
    "tgp": ("W", "U"),
    "gmc": ("w", "U", "acc"),
    "mlg": ("w", "U", "V", "testpred", "train_rmse", "test_rmse"),
    "draw": ("out",),
}
SELF_RELATIVE = ("acc", "train_rmse", "test_rmse")      # every other quantity: max|Δ| / max|x|
# the caps on B = MARGIN·u (conditions of tests/test_gibbs_cases.py)
CAPS = {
    "tgp": dict(W=1e-11, U=1e-11),
    "gmc": dict(w=1e-13, U=1e-13, acc=1e-12),
    "mlg": dict.fromkeys(QUANTITIES["mlg"], 1e-13),
    "draw": dict(out=1e-13),
}
# what tests/test_gpu_tgp.py, test_gpu_parity.py and test_gpu_movielens.py ask of the same quantities
OLD_BARS = {
    "tgp": dict(W=1e-8, U=1e-8),
    "gmc": dict(w=1e-8, U=1e-8, acc=1e-7),
    "mlg": dict(w=1e-8, U=1e-8, V=1e-8, testpred=1e-8, train_rmse=1e-9, test_rmse=1e-9),
    "draw": dict(out=1e-10),
}
METROPOLIS_MARGIN = 1e-3

TGP_GEN, TGP_SIGMA_RBF = 123, 1.4332
GMC_SEED = 7
MLG_SEED, MLG_SIGNAL_VAR, MLG_SIGMA_U, MLG_SIGMA_W = 17, 0.8, 0.3, 0.9
DESIGN_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 130)
DESIGN_OTHER = 140
MLG_NTEST = 300
DRAW_STREAM = (11, 3, 7, 0)         # seed, c1, c2, c3

Tgp = collections.namedtuple("Tgp", "name family n D N r q sigma sweeps fixed_I seed")
Gmc = collections.namedtuple("Gmc", "name family n D N r Q L epochs signal_var eps")
Mlg = collections.namedtuple("Mlg", "name family design r burnin maxepoch n_samples avg fixw")
Draw = collections.namedtuple("Draw", "name family p")

# (6, 2): column 2 never names the value 2
ABSENT_I = ((1, 1), (2, 1), (1, 1), (2, 1), (2, 1), (1, 1))


def _cases():
    out = [
        Tgp("ragged_q20_N131", "tgp", 7, 3, 131, 3, 20, 0.3, 3, None, 7),
        Tgp("absent_value_N13", "tgp", 6, 2, 13, 2, 6, 0.3, 2, ABSENT_I, 7),
        # data seed 1: at seed 7 the U_k conditionals of this shape are ten times worse conditioned and
        # the restatement's own error (1.5e-12) alone puts B past the cap
        Tgp("gemv_two_chunks_N257", "tgp", 10, 4, 257, 5, 40, 0.2299, 2, None, 1),
        Tgp("n70_padded_temp", "tgp", 70, 2, 70, 2, 12, 0.25, 2, None, 7),
        Tgp("nr180_second_pass", "tgp", 36, 2, 70, 5, 30, 0.25, 2, None, 7),
        Tgp("repeated_I_row", "tgp", 5, 2, 40, 2, 6, 0.3, 2, None, 7),
        Gmc("accepting", "gmc", 8, 3, 40, 2, 5, 5, 3, 1.0, 1e-2),
        Gmc("rejecting", "gmc", 8, 3, 40, 2, 5, 5, 2, 1.0, 1e-1),
        Gmc("odd_rank_N70", "gmc", 20, 4, 70, 5, 40, 3, 2, 1.0, 1e-3),
        Gmc("signal_var_half", "gmc", 9, 2, 67, 3, 9, 2, 2, 0.5, 1e-2),
        # with these inputs the case above accepts both epochs; this one (L = 3, ε = 2.5e-2) is rejected
        Gmc("signal_var_half_rejected", "gmc", 9, 2, 67, 3, 9, 3, 1, 0.5, 2.5e-2),
        # ε = 1e-4, not 1e-2: the energy holds |mom|²/2 ≈ n·r/2 = 520, and at ε = 1e-2 (a geodesic
        # argument of 1-norm 50) the restatement's own acceptance probability is off by 9.7e-13
        Gmc("n520", "gmc", 520, 1, 20, 2, 2, 1, 1, 1.0, 1e-4),
        Gmc("rank_one", "gmc", 12, 2, 30, 1, 1, 2, 2, 1.0, 1e-2),
    ]
    for design in ("users12", "users140"):
        for r in (3, 4, 8, 10):
            out.append(Mlg("%s_r%d" % (design, r), "mlg", design, r, 0, 2, 1, False, False))
    out += [
        Mlg("users3_r4", "mlg", "users3", 4, 0, 2, 1, False, False),
        Mlg("avg_burnin1_r3", "mlg", "users12", 3, 1, 2, 1, True, False),
        Mlg("two_samples_r4", "mlg", "users140", 4, 0, 2, 2, False, False),
        Mlg("fixw_r4", "mlg", "users12", 4, 0, 2, 1, False, True),
    ]
    out += [Draw("p%d" % p, "draw", p) for p in (1, 5, 16, 17, 33, 100, 177, 225)]
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def key(c):
    return "%s_%s" % (c.family, c.name)


def case_id(c):
    return "%s-%s" % (c.family, c.name)


# ---------------------------------------------------------------------------------------- inputs
def design(which):
    """(Rating (N, 3), Rtest (MLG_NTEST, 3), n1, n2, ymean, ystd) of a synthetic rating problem.
    "users12": user i of 12 (shuffled) has DESIGN_COUNTS[i] ratings of distinct movies out of
    DESIGN_OTHER; "users140": the same with the sides exchanged; "users3": 16 distinct pairs of 3
    users and 12 movies.  Ratings 1..5, whitened; the rating rows are shuffled; the test ratings
    name every row of both sides, the ones without training ratings included."""
    rng = np.random.default_rng((5113, {"users12": 0, "users140": 0, "users3": 1}[which]))
    if which == "users3":
        n1, n2 = 3, 12
        flat = rng.permutation(n1 * n2)[:16]
        side, other = flat // n2, flat % n2
    else:
        counts = rng.permutation(DESIGN_COUNTS)
        side = np.repeat(np.arange(len(counts)), counts)
        other = np.concatenate([rng.permutation(DESIGN_OTHER)[:k] for k in counts])
        n1, n2 = len(counts), DESIGN_OTHER
    stars = rng.integers(1, 6, len(side)).astype(np.float64)
    order = rng.permutation(len(side))
    side, other, stars = side[order], other[order], stars[order]
    tside, tother = rng.integers(0, n1, MLG_NTEST), rng.integers(0, n2, MLG_NTEST)
    tside[:n1], tother[:n2] = np.arange(n1), np.arange(n2)
    tstars = rng.integers(1, 6, MLG_NTEST).astype(np.float64)
    ymean, ystd = float(stars.mean()), float(stars.std(ddof=1))
    if which == "users140":
        side, other, tside, tother, n1, n2 = other, side, tother, tside, n2, n1
    Rating = np.column_stack([side + 1.0, other + 1.0, (stars - ymean) / ystd])
    Rtest = np.column_stack([tside + 1.0, tother + 1.0, (tstars - ymean) / ystd])
    return Rating, Rtest, n1, n2, ymean, ystd


def gmc_problem(n, D, N, r, Q):
    """tests/test_gpu_parity.py's _gmc_problem."""
    rng = np.random.default_rng(3)
    phi = rng.standard_normal((n, D, N)) * 0.5
    I = R.samplenz(r, D, Q, 1)
    w, U = R.init_state(n, r, D, Q, 3)
    return phi, R.pred(w, U, I, phi) + 0.1 * rng.standard_normal(N), I


def draw_problem(p):
    """M (p × p, SPD) and x of test_gaussian_draw_blocked_cholesky_and_solves: A·Aᵀ/p + I/2 for
    A = randn(p, p + 3), with every entry of A·Aᵀ summed by math.fsum (the correctly rounded sum of the
    rounded products), so that M has the same doubles on every machine whatever its BLAS does."""
    rng = np.random.default_rng(p)
    A = rng.standard_normal((p, p + 3))
    G = np.empty((p, p))
    for i in range(p):
        for j in range(i + 1):
            G[i, j] = G[j, i] = math.fsum(A[i] * A[j])
    return np.asfortranarray(G / p + 0.5 * np.eye(p)), rng.standard_normal(p)


@functools.lru_cache(maxsize=None)
def _inputs(k):
    c = _BY_KEY[k]
    if c.family == "tgp":
        rng = np.random.default_rng((c.seed, c.N, c.D))
        X = rng.standard_normal((c.N, c.D)) * rng.uniform(0.5, 3.0, c.D) + rng.uniform(-2, 2, c.D)
        y = np.sin(X).sum(axis=1) + 0.1 * rng.standard_normal(c.N)
        Z, bb = R.seeded_feature_inputs(c.n, c.D, TGP_GEN)
        b = R.feature(R.datawhitening(X), TGP_SIGMA_RBF, 1.0, 1.0, Z, bb)
        I = (R.tgp_draw_I(c.q, c.D, c.r, TGP_GEN) if c.fixed_I is None
             else np.asfortranarray(np.array(c.fixed_I, dtype=np.int32)))
        p = dict(X=X, y=y, b=np.asfortranarray(b), yw=R.datawhitening(y), I=I)
    elif c.family == "gmc":
        phi, y, I = gmc_problem(c.n, c.D, c.N, c.r, c.Q)
        w0, U0 = R.init_state(c.n, c.r, c.D, c.Q, GMC_SEED)
        p = dict(phi=np.asfortranarray(phi), y=y, I=I, w0=w0, U0=np.asfortranarray(U0))
    elif c.family == "mlg":
        Rating, Rtest, n1, n2, ymean, ystd = design(c.design)
        w0 = np.random.default_rng((9, c.r)).standard_normal((c.r, c.r))
        p = dict(Rating=Rating, Rtest=Rtest, n1=n1, n2=n2, ymean=ymean, ystd=ystd,
                 w0=np.asfortranarray(w0))
    else:
        Mx, x = draw_problem(c.p)
        p = dict(M=Mx, x=x)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def inputs(c):
    return _inputs(key(c))


_DIGESTED = {"tgp": ("X", "y", "b", "yw", "I"), "gmc": ("phi", "y", "I", "w0", "U0"),
             "mlg": ("Rating", "Rtest", "w0"), "draw": ("M", "x")}


def digest(c):
    p = inputs(c)
    h = hashlib.sha256(repr(tuple(c)).encode())
    for name in _DIGESTED[c.family]:
        a = np.asfortranarray(p[name])
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    if c.family == "mlg":
        h.update(np.array([p["ymean"], p["ystd"]]).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------- the restatement of record
def mlg_args(c, p):
    """(positional arguments, keywords) of the case's entry, the same for oracle.movielens_ref and
    gpt_amd.movielens."""
    ud, md = np.zeros((p["n1"], 0)), np.zeros((p["n2"], 0))
    head = (p["Rating"], ud, md, p["Rtest"], MLG_SIGNAL_VAR, MLG_SIGMA_U)
    tail = (c.burnin, c.maxepoch, c.n_samples, MLG_SEED, p["ymean"], p["ystd"])
    args = head + ((p["w0"],) if c.fixw else (MLG_SIGMA_W, p["w0"])) + tail
    return args, dict(avg=c.avg)


def mlg_entry(c):
    return "GPT_fixw_gibbs" if c.fixw else "GPT_fullw_gibbs"


def standard(c, res):
    """An entry's result -> {quantity: array, the stored sweep / epoch first}."""
    if c.family == "tgp":
        W, U = res[0], res[1]
        return dict(W=np.moveaxis(W, -1, 0).copy(), U=np.moveaxis(U, -1, 0).copy())
    if c.family == "gmc":
        w, U, acc = res
        return dict(w=np.moveaxis(w, -1, 0).copy(), U=np.moveaxis(U, -1, 0).copy(),
                    acc=np.array(acc, dtype=np.float64))
    if c.family == "mlg":
        res = tuple(res)
        if c.fixw:
            res = (None,) + res
        w, U, V, tp, trm, tsm = res
        return dict(w=None if w is None else np.moveaxis(w, -1, 0).copy(), U=np.moveaxis(U, -1, 0).copy(),
                    V=np.moveaxis(V, -1, 0).copy(), testpred=np.asarray(tp).T.copy(),
                    train_rmse=np.array(trm, dtype=np.float64), test_rmse=np.array(tsm, dtype=np.float64))
    return dict(out=np.array(res, dtype=np.float64)[None, :])


def run_numpy(c):
    p = inputs(c)
    if c.family == "tgp":
        res = R.GPT_inf(p["b"], p["yw"], c.sigma, c.n, c.r, c.q, c.sweeps, 0, TGP_GEN,
                        I=None if c.fixed_I is None else p["I"])
        assert (res[2] == p["I"]).all()
    elif c.family == "gmc":
        res = R.GPT_GMC(p["phi"], p["y"], c.signal_var, p["I"], c.r, c.Q, c.eps, c.eps, 0, c.epochs, c.L,
                        GMC_SEED, w_init=p["w0"], U_init=p["U0"])
    elif c.family == "mlg":
        args, kw = mlg_args(c, p)
        res = getattr(M, mlg_entry(c))(*args, **kw)
    else:
        seed, c1, c2, c3 = DRAW_STREAM
        L = np.linalg.cholesky(p["M"])
        res = np.linalg.solve(L.T, px.normals(c.p, seed, c1, c2, c3)) + np.linalg.solve(p["M"], p["x"])
    return standard(c, res)


# ------------------------------------------ the samplers, on float64 or on mpmath numbers
class _F64Backend:
    obj = False

    def arr(self, a):
        return np.array(a, dtype=np.float64)

    def num(self, x):
        return float(x)

    def zeros(self, shape):
        return np.zeros(shape)

    def sqrt(self, x):
        return math.sqrt(x)

    def exp(self, x):
        return math.exp(x)

    def normals(self, count, seed, c1, c2, c3):
        return px.normals(count, seed, c1, c2, c3)

    def dot(self, a, b):
        return float(np.dot(a, b)) if len(a) else 0.0

    def matvec(self, A, v):
        return A @ v

    def syrk(self, A):
        return A @ A.T

    def geodboth(self, U, mom, t):
        Un, Vn, ok = R.geodboth(U, mom, t)
        assert ok
        return Un, Vn

    def clip(self, a):
        return np.clip(a, 1.0, 5.0)


class _MPBackend:
    obj = True

    def arr(self, a):
        return SC._mpa(a)

    def num(self, x):
        import mpmath as mp
        return mp.mpf(float(x))

    def zeros(self, shape):
        return SC._mpa(np.zeros(shape))

    def sqrt(self, x):
        import mpmath as mp
        return mp.sqrt(x)

    def exp(self, x):
        import mpmath as mp
        return mp.exp(x)

    def normals(self, count, seed, c1, c2, c3):
        return SC._mp_normals(count, seed, c1, c2, c3)

    def dot(self, a, b):
        import mpmath as mp
        return mp.fdot(zip(a, b)) if len(a) else mp.mpf(0)

    def matvec(self, A, v):
        out = np.empty(A.shape[0], dtype=object)
        v = list(v)
        for i in range(A.shape[0]):
            out[i] = self.dot(A[i], v)
        return out

    def syrk(self, A):
        p = A.shape[0]
        out = np.empty((p, p), dtype=object)
        rows = [list(A[i]) for i in range(p)]
        for i in range(p):
            for j in range(i + 1):
                out[i, j] = out[j, i] = self.dot(rows[i], rows[j])
        return out

    def geodboth(self, U, mom, t):
        """gpt_sgld_ref.geodboth with the true exponentials: the end point and its velocity."""
        r = U.shape[1]
        A = U.T @ mom
        T = np.empty((2 * r, 2 * r), dtype=object)
        T[:r, :r] = A
        T[:r, r:] = -(mom.T @ mom)
        T[r:, :r] = SC._mpa(np.eye(r))
        T[r:, r:] = A
        E = SC._mp_expm(T * t)
        mexp = SC._mp_expm(A * (-t))
        X = np.hstack([U, mom])
        tmpU = (X @ E[:, :r]) @ mexp
        tmpV = (X @ E[:, r:]) @ mexp
        nrm = SC._fn("sqrt")((tmpU * tmpU).sum(axis=0))
        return tmpU / nrm[None, :], tmpV

    def clip(self, a):
        return np.frompyfunc(lambda x: min(max(x, 1), 5), 1, 1)(a)


F64, MP = _F64Backend(), _MPBackend()

# The defect table of tests/test_gibbs_cases.py: small faults of a device kernel, restated in
# run_f64.  Each changes a result by less than the bars of the oracle tests (OLD_BARS) allow.
DEFECTS = {
    "prior_diag_32bit": "the prior diagonal (1/σ_w², 1/σ_u²) rounded to 32 significant bits (at float32's "
                        "24 the oracle tests' own 1e-8 fails too)",
    "pivot_recip": "the reciprocal of the fourth pivot (the last, where p < 4) of every Cholesky factor "
                   "off by 1e-10 (by 1e-12 in the draw alone, whose old bar is 1e-10)",
    "loo_f32_recip": "the leave-one-out quotient V / temp of the first core row through a float32 "
                     "reciprocal",
    "ktail_last_col": "the last column of the SYRK's K tail scaled by 1 + 1e-9",
    "z_scaled": "the normals z of the conditional draws (GMC: the momentum p) scaled by 1 + 1e-10",
    "energy_f32": "GMC's residual energy Σ res² summed in float32",
    "rhs_scaled": "the right-hand side A·y of a conditional scaled by 1 − 1e-10",
}


def _scale_last(A, f):
    A = A.copy()
    A[:, -1] = A[:, -1] * f
    return A


def _chol(be, A, defect=None, size=1e-10):
    """Lower Cholesky factor, column by column, the column scaled by the pivot's reciprocal."""
    p = A.shape[0]
    L = be.zeros((p, p))
    for j in range(p):
        d = A[j, j] - be.dot(L[j, :j], L[j, :j])
        assert d > 0
        L[j, j] = be.sqrt(d)
        inv = 1 / L[j, j]
        if defect == "pivot_recip" and j == min(3, p - 1):
            inv = inv * (1 + size)
        if j + 1 < p:
            col = A[j + 1:, j] - be.matvec(L[j + 1:, :j], L[j, :j]) if j else A[j + 1:, j]
            L[j + 1:, j] = col * inv
    return L


def _fwd(be, L, x):
    y = x.copy()
    for j in range(len(x)):
        y[j] = (x[j] - be.dot(L[j, :j], y[:j])) / L[j, j]
    return y


def _bwd(be, L, x):
    y = x.copy()
    for j in range(len(x) - 1, -1, -1):
        y[j] = (x[j] - be.dot(L[j + 1:, j], y[j + 1:])) / L[j, j]
    return y


def _gaussian(be, prec, rhs, z, defect=None, size=1e-10):
    """L⁻ᵀz + prec⁻¹rhs for prec = L·Lᵀ (z None: the mean alone)."""
    if defect == "rhs_scaled":
        rhs = rhs * (1 - 1e-10)
    L = _chol(be, prec, defect, size)
    mu = _bwd(be, L, _fwd(be, L, rhs))
    if z is None:
        return mu
    return _bwd(be, L, z * (1 + 1e-10) if defect == "z_scaled" else z) + mu


def _diag(be, p, value):
    out = be.zeros((p, p))
    for i in range(p):
        out[i, i] = value
    return out


def _round32(x):
    m, e = math.frexp(x)
    return math.ldexp(round(m * 2.0 ** 32) / 2.0 ** 32, e)


def _run_tgp(be, c, p, defect=None):
    n, D, N, r, q = c.n, c.D, c.N, c.r, c.q
    b, y, I0 = be.arr(p["b"]), be.arr(p["yw"]), np.asarray(p["I"]) - 1
    s2 = be.num(c.sigma) * be.num(c.sigma)
    su = be.sqrt(be.num(1) / r)
    prior_w, prior_u = be.num(q) / (r ** D), be.num(r)            # 1/σ_w², 1/σ_u²
    if defect == "prior_diag_32bit":
        prior_w = _round32(prior_w)
    U = be.zeros((n, r, D))
    for d in range(D):
        U[:, :, d] = be.normals(n * r, TGP_GEN, 0, px.TGP_U_INIT, d).reshape((n, r), order="F") * su
    tail = (lambda A: _scale_last(A, 1 + 1e-9)) if defect == "ktail_last_col" else (lambda A: A)
    out = dict(W=[], U=[])
    for it in range(c.sweeps):
        temp, V, _ = SC._mp_forward(b, be.zeros(q), U, I0)
        prec = be.syrk(tail(V)) / s2 + _diag(be, q, prior_w)
        W = _gaussian(be, prec, (V @ y) / s2, be.normals(q, TGP_GEN, it, px.TGP_W_NOISE, 0), defect)
        out["W"].append(W.copy())
        out["U"].append(U.copy())
        for k in range(D):
            tk = temp[k][I0[:, k], :]
            Vk = V / tk
            if defect == "loo_f32_recip":
                Vk[0] = V[0] * (1.0 / tk[0]).astype(np.float32).astype(np.float64)
            Vkk = Vk * W[:, None]
            C = be.zeros((r, N))
            for l in range(r):
                sel = I0[:, k] == l
                if sel.any():
                    C[l] = Vkk[sel].sum(axis=0)
            Ck = (C[:, None, :] * b[None, :, k, :]).reshape((r * n, N))       # row (l, j) -> l·n + j
            prec = be.syrk(tail(Ck)) / s2 + _diag(be, n * r, prior_u)
            zu = be.normals(n * r, TGP_GEN, it, px.TGP_U_NOISE, k)
            if defect == "z_scaled":
                zu = zu * (1 + 1e-10)
            x = _gaussian(be, prec, (Ck @ y) / s2 + zu, None, defect)        # prec⁻¹(rhs + z), TGP.jl:79
            U[:, :, k] = x.reshape((n, r), order="F")
            temp[k] = U[:, :, k].T @ b[:, k, :]
            V = Vk * temp[k][I0[:, k], :]
    return {k: np.array(v, dtype=object if be.obj else np.float64) for k, v in out.items()}


def _f64_cores(pb, temp, V, res, w, I0, r):
    """step_cases._mp_cores on float64."""
    n, D, B = pb.shape
    gU = np.empty((n, r, D))
    for k in range(D):
        Uphi = V / temp[k][I0[:, k], :]
        A = np.zeros((r, B))
        for l in range(r):
            idx = np.nonzero(I0[:, k] == l)[0]
            if len(idx):
                A[l] = w[idx] @ Uphi[idx, :]
        gU[:, :, k] = pb[:, k, :] @ (A * res[None, :]).T
    return V @ res, gU


def _run_gmc(be, c, p, defect=None):
    n, D, N, r, Q = c.n, c.D, c.N, c.r, c.Q
    phi, y, I0 = be.arr(p["phi"]), be.arr(p["y"]), np.asarray(p["I"]) - 1
    w, U = be.arr(p["w0"]), be.arr(p["U0"])
    sv = be.num(c.signal_var)
    sq = be.sqrt(be.num(c.eps))
    re = r + (r & 1)
    cores = SC._mp_cores if be.obj else _f64_cores

    def gradients(w, U):
        temp, V, fhat = SC._mp_forward(phi, w, U, I0)
        res = y - fhat
        cw, cU = cores(phi, temp, V, res, w, I0, r)
        return cw / sv - w, cU / sv, res

    def energy(w, res, mom, pw):
        e = (res * res).sum()
        if defect == "energy_f32":
            e = float(np.sum((res * res).astype(np.float32), dtype=np.float32))
        return -(w * w).sum() / 2 - e / (2 * sv) - (mom * mom).sum() / 2 - (pw * pw).sum() / 2

    out = dict(w=[], U=[], acc=[])
    for epoch in range(c.epochs):
        w_old = w
        pw = be.normals(Q, GMC_SEED, epoch, px.GMC_P, 0)
        if defect == "z_scaled":
            pw = pw * (1 + 1e-10)
        mom = be.zeros((n, r, D))
        for k in range(D):
            xi = be.normals(re * n, GMC_SEED, epoch, px.GMC_MOM, k).reshape((n, re))[:, :r]
            mom[:, :, k] = SC._mp_proj(U[:, :, k], xi)
        gw, gU, res = gradients(w, U)
        H_old = energy(w, res, mom, pw)
        U = U.copy()
        for _ in range(c.L):
            pw = pw + gw * (sq / 2)
            for k in range(D):
                mom[:, :, k] = SC._mp_proj(U[:, :, k], mom[:, :, k] + gU[:, :, k] * (sq / 2))
            w = w + pw * sq
            for k in range(D):
                U[:, :, k], mom[:, :, k] = be.geodboth(U[:, :, k], mom[:, :, k], sq)
            gw, gU, res = gradients(w, U)
            pw = pw + gw * (sq / 2)
            for k in range(D):
                mom[:, :, k] = SC._mp_proj(U[:, :, k], mom[:, :, k] + gU[:, :, k] * (sq / 2))
        acc = be.exp(energy(w, res, mom, pw) - H_old)
        if px.uniform(GMC_SEED, epoch, px.GMC_U, 0) > acc:
            w = w_old                                          # U keeps its proposal (the reference's aliasing)
        out["w"].append(w.copy())
        out["U"].append(U.copy())
        out["acc"].append(acc)
    return {k: np.array(v, dtype=object if be.obj else np.float64) for k, v in out.items()}


def _run_mlg(be, c, p, defect=None):
    r, n1, n2 = c.r, p["n1"], p["n2"]
    Rating, Rtest = p["Rating"], p["Rtest"]
    N, Ntest = len(Rating), len(Rtest)
    users, movies = Rating[:, 0].astype(np.int64) - 1, Rating[:, 1].astype(np.int64) - 1
    tu, tm = Rtest[:, 0].astype(np.int64) - 1, Rtest[:, 1].astype(np.int64) - 1
    y, yt = be.arr(Rating[:, 2]), be.arr(Rtest[:, 2])
    sv, su = be.num(MLG_SIGNAL_VAR), be.num(MLG_SIGMA_U)
    prior_u, prior_w = 1 / (su * su), 1 / (be.num(MLG_SIGMA_W) * be.num(MLG_SIGMA_W))
    if defect == "prior_diag_32bit":
        prior_u = _round32(prior_u)
    ystd, ymean = be.num(p["ystd"]), be.num(p["ymean"])
    w = be.arr(p["w0"])
    U = be.normals(n1 * r, MLG_SEED, 0, px.CFG_INIT, 1).reshape((n1, r), order="F") * su
    V = be.normals(n2 * r, MLG_SEED, 0, px.CFG_INIT, 2).reshape((n2, r), order="F") * su
    tail = (lambda A: _scale_last(A, 1 + 1e-9)) if defect == "ktail_last_col" else (lambda A: A)

    def conditional(X, ysel, prior, z, dfc=None):
        """X (count, p): the draw of N(prec⁻¹Xᵀy/σ², prec⁻¹), prec = XᵀX/σ² + prior·I."""
        prec = be.syrk(tail(X.T)) / sv + _diag(be, X.shape[1], prior)
        return _gaussian(be, prec, (X.T @ ysel) / sv, z, dfc)

    out = {q: [] for q in QUANTITIES["mlg"]}
    trainpred, testpred = y * 0, yt * 0
    counter = sweep = 0
    for epoch in range(1, c.burnin + c.maxepoch + 1):
        for _ in range(c.n_samples):
            row_defect = defect if defect in ("z_scaled", "rhs_scaled") else None
            for i in range(n1):
                sel = users == i
                if sel.any():
                    U[i] = conditional(V[movies[sel]] @ w.T, y[sel], prior_u,
                                       be.normals(r, MLG_SEED, sweep, px.CFG_U, i), row_defect)
            for j in range(n2):
                sel = movies == j
                if sel.any():
                    V[j] = conditional(U[users[sel]] @ w, y[sel], prior_u,
                                       be.normals(r, MLG_SEED, sweep, px.CFG_V, j), row_defect)
            if not c.fixw:
                K = (V[movies][:, :, None] * U[users][:, None, :]).reshape((N, r * r))
                w = conditional(K, y, prior_w, be.normals(r * r, MLG_SEED, sweep, px.CFG_W, 0),
                                defect).reshape((r, r), order="F")
            sweep += 1
        if epoch > c.burnin:
            if not c.avg:
                counter = 0
            trainpred = (trainpred * counter + ((U[users] @ w) * V[movies]).sum(axis=1)) / (counter + 1)
            testpred = (testpred * counter + ((U[tu] @ w) * V[tm]).sum(axis=1)) / (counter + 1)
            ft, fs = be.clip(trainpred * ystd + ymean), be.clip(testpred * ystd + ymean)
            out["train_rmse"].append(be.sqrt((((y * ystd + ymean) - ft) ** 2).sum() / N))
            out["test_rmse"].append(be.sqrt((((yt * ystd + ymean) - fs) ** 2).sum() / Ntest))
            out["w"].append(w.copy())
            out["U"].append(U.copy())
            out["V"].append(V.copy())
            out["testpred"].append(fs)
            counter += 1
    res = {k: np.array(v, dtype=object if be.obj else np.float64) for k, v in out.items()}
    if c.fixw:
        res["w"] = None
    return res


def _run_draw(be, c, p, defect=None):
    seed, c1, c2, c3 = DRAW_STREAM
    out = _gaussian(be, be.arr(p["M"]), be.arr(p["x"]), be.normals(c.p, seed, c1, c2, c3), defect, 1e-12)
    return dict(out=np.array([out], dtype=object if be.obj else np.float64))


_RUN = {"tgp": _run_tgp, "gmc": _run_gmc, "mlg": _run_mlg, "draw": _run_draw}


def run_f64(c, defect=None):
    """The sampler of this file on float64: the restatement that carries the defect table."""
    return _RUN[c.family](F64, c, inputs(c), defect)


def compute(c):
    """The case in mpmath: {quantity: object array} laid out as standard()'s."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _RUN[c.family](MP, c, inputs(c))


def pack(c, ref):
    out = {}
    for q in QUANTITIES[c.family]:
        if ref[q] is not None:
            out[q + "_hi"], out[q + "_lo"] = SC._dd(ref[q])
    return out


def as_reference(run):
    return {q: (v, np.zeros_like(v)) for q, v in run.items() if v is not None}


def rel_err(c, out, ref):
    """{quantity: worst error over the stored sweeps / epochs}: max|Δ| / max|x| of the sweep, the
    acceptance probability and the RMSEs relative to themselves.  ref is reference()'s dict, or
    another run's."""
    if not isinstance(next(v for v in ref.values() if v is not None), tuple):
        ref = as_reference(ref)
    res = {}
    for q in QUANTITIES[c.family]:
        if q not in ref or out.get(q) is None:
            continue
        hi, lo = ref[q]
        d = np.abs((out[q] - hi) - lo)
        if q in SELF_RELATIVE:
            res[q] = float((d / np.abs(hi)).max())
        else:
            res[q] = max(float(d[s].max() / np.abs(hi[s]).max()) for s in range(len(hi)))
    return res


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def _reference(k):
    c = _BY_KEY[k]
    st = _stored()
    if str(st.get(k + "_digest")) == digest(c):
        a = {s: st[k + "_" + s] for q in QUANTITIES[c.family] for s in (q + "_hi", q + "_lo")
             if k + "_" + s in st}
    else:
        a = pack(c, compute(c))
    out = {q: (a[q + "_hi"], a[q + "_lo"].astype(np.float64)) for q in QUANTITIES[c.family] if q + "_hi" in a}
    for v in out.values():
        for x in v:
            x.setflags(write=False)
    return out


def reference(c):
    """{quantity: (hi, lo)} of a case from the committed file where the case's digest is there, else
    by mpmath.  Shared and read-only."""
    return _reference(key(c))


def bars():
    """{family: {quantity: B}} as the fixture stores them (measured by the maker on the numpy
    restatement against mpmath, never on the device)."""
    st = _stored()
    return {fam: dict(zip(QUANTITIES[fam], st["bar_" + fam])) for fam in FAMILIES}


def measured_u():
    st = _stored()
    return {fam: dict(zip(QUANTITIES[fam], st["u_" + fam])) for fam in FAMILIES}


_BY_KEY = {key(_c): _c for _c in CASES}
