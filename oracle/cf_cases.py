"""Cases, inputs, the mpmath step and the CPU-side measurements of the MovieLens CF step tests
(tests/test_gpu_cf_step.py on the device, tests/test_cf_cases.py on the CPU): the epoch kernels of
gpt_amd/csrc/cf.hip (cf_epoch_kernel, cf_move_kernel, cf_eval_kernel) held to a 50-digit reference
at rounding level, in the shape of oracle/step_cases.py, whose storage (hi float64 + lo float32),
margin and caps (MARGIN, B_MAX, COND_MAX) are used as they are.

A case is a synthetic rating problem regenerated from (shape, seed) and identified by a SHA-256
digest: N = nfull·m + tail ratings (nfull + 1 steps per epoch), burnin 0, `epochs` stored epochs.
User and movie ids are drawn from fewer ids than a batch has ratings, so duplicates within a batch
are certain; the ratings are laid out through the first epoch's permutation, so a case can say what
its first epoch's batches hold (one user only, all ids distinct, a feature none / all of a batch's
ratings carry).  The last user and the last movie have no training rating (rows no batch touches);
they are in the test set.  One user and one movie have no features.  U0 / V0 are σ_u·normal
(Euclidean) or a numpy QR factor (Stiefel) and are injected on the device (U_init / V_init).
σ_u (Euclidean cases) is the largest of SIGMA_U_TOP·2⁻ᵏ at which the rms of the last epoch's test
prediction stays below PRED_MAX rating standard deviations: moves of a quarter of U, V and w per
step grow the prediction super-exponentially (a tail batch, scaled by N/B, faster still), and once
it passes the ratings' size the fixed step overshoots and the case loses its conditioning.

Step sizes (inputs, from the float64 step 1 and rounded to three digits): σ² is the free knob.
  SGD, Euclidean:   εU·rms(gradU over the batch's rows)/2 = SGD_EUCLID_SHARE·rms U, with σ² such
                    that the prior decay 1 − εU/(2σ_u²) is 1 − DECAY (a skipped row is visible);
                    εw·rms gradw/2 = SGD_EUCLID_SHARE·rms w.
  SGLD, Euclidean:  gradient move = noise move for U, V and w, the noise SGD_EUCLID_SHARE·rms U.
  Stiefel:          the case's εU; √εU·gradU/2 has rms 1 over the batch's rows (the noise's size);
                    w as above.
ytrainMean = 3 and ytrainStd = 2 / rms(last epoch's test prediction): some stored predictions are
cut off at 1, some at 5, most are not.

The reference (compute) is oracle/movielens_ref.py's formulas (100k_movielensExperiment.jl:409-551
as that file restates them) on the exact doubles of the inputs in mpmath at MP_DIGITS digits: the
per-rating sums as matrix products with the 0 / 1 / b / c incidence matrices (sums in any order), the
true matrix exponential, normals by Box–Muller in mpmath from the Philox words, permutations from
oracle.philox.  Per stored epoch it keeps w, U, V, testpred_store, train and test RMSE, every
element.  The same code on float64 (run_f64) is the carrier of the defect table (DEFECTS).

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
MARGIN, B_MAX, COND_MAX, NORM_MAX = SC.MARGIN, SC.B_MAX, SC.COND_MAX, SC.NORM_MAX
SGD_EUCLID_SHARE = SC.SGD_EUCLID_SHARE
DECAY = 0.1               # εU/(2σ_u²) of the Euclidean SGD cases
RUN_SEED = 29
SIGMA_W = 1.5
SIGMA_U_TOP, PRED_MAX = 0.1, 0.3     # the ladder of σ_u (inputs) and what stops it
A_, B_, C_ = 0.9, 0.6, 0.4
YMEAN = 3.0
RANKS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 16, 20)       # launch_util.h Ranks
GOLDEN = os.path.join(os.path.dirname(SC.GOLDEN), "cf_step_mp.npz")

FAMILIES = ("lazy_sgd", "eager_sgd", "sgld_euclid", "sgd_stiefel", "sgld_stiefel", "fixw")
QUANTITIES = ("w", "U", "V", "testpred", "train_rmse", "test_rmse", "colnorm")
STORED = ("w", "U", "V", "testpred", "rmse")

Case = collections.namedtuple(
    "Case", "name family entry r m tail n1 n2 D1 D2 langevin stiefel avg lazy epochs nfull epsU seed "
            "special ntest")


def _mk(name, family, r, m, tail, D1=3, D2=2, n1=13, n2=11, entry="fullw_sideinfo", avg=False,
        lazy=None, epochs=2, nfull=2, epsU=0.0, seed=0, special="", ntest=19):
    langevin = family in ("sgld_euclid", "sgld_stiefel") or (family == "fixw" and epsU > 0)
    stiefel = family in ("sgd_stiefel", "sgld_stiefel") or (family == "fixw" and epsU > 0)
    return Case(name, family, entry, r, m, tail, n1, n2, D1, D2, langevin, stiefel, avg, lazy, epochs,
                nfull, epsU, seed, special, ntest)


def _cases():
    out = []
    for r in RANKS:
        out.append(_mk("rank%d" % r, "lazy_sgd", r, 24, 5))
    live = dict(D1=28, D2=18, n1=31, n2=23)
    out.append(_mk("live_r20_lazy", "lazy_sgd", 20, 100, 37, **live))
    out.append(_mk("live_r20_eager", "eager_sgd", 20, 100, 37, lazy="0", **live))
    # link edges
    out.append(_mk("sort128_tail1", "lazy_sgd", 4, 128, 1, n1=37, n2=29))
    out.append(_mk("walk129_sort128", "lazy_sgd", 4, 129, 128, n1=37, n2=29))
    out.append(_mk("walk200_tail16", "lazy_sgd", 4, 200, 16, n1=37, n2=29))
    out.append(_mk("m1030_r1", "lazy_sgd", 1, 1030, 7, D1=1, D2=1, n1=37, n2=29, epochs=1))
    out.append(_mk("one_user_batch", "lazy_sgd", 4, 24, 5, special="oneuser"))
    out.append(_mk("distinct_batch", "lazy_sgd", 4, 24, 5, n1=31, n2=29, special="distinct"))
    # feature edges
    out.append(_mk("nofeat_fullw", "lazy_sgd", 3, 24, 5, D1=0, D2=0, entry="fullw"))
    out.append(_mk("D64", "lazy_sgd", 3, 24, 5, D1=64, D2=1, special="lastcol"))
    out.append(_mk("D65_csr", "eager_sgd", 3, 24, 5, D1=65, D2=2, special="lastcol"))
    out.append(_mk("feat_none_all", "lazy_sgd", 3, 24, 5, n1=17, n2=15, special="noneall"))
    out.append(_mk("lazy_avg_eval", "lazy_sgd", 3, 24, 5, avg=True, ntest=301, seed=1))
    # Langevin, Euclidean
    out.append(_mk("sgld_r5", "sgld_euclid", 5, 24, 5))
    out.append(_mk("sgld_r20", "sgld_euclid", 20, 24, 5))
    # Stiefel
    out.append(_mk("stf_sgd_r2", "sgd_stiefel", 2, 24, 5, epsU=1e-4))
    out.append(_mk("stf_sgd_r16", "sgd_stiefel", 16, 24, 5, epsU=1e-5, n1=19, n2=17))
    out.append(_mk("stf_sgld_r5", "sgld_stiefel", 5, 24, 5, epsU=1e-4, avg=True, ntest=301))
    out.append(_mk("stf_sgld_r20", "sgld_stiefel", 20, 24, 5, epsU=1e-5, n1=23, n2=21, epochs=1, nfull=1))
    # fixed w
    out.append(_mk("fixw_side_sgd", "fixw", 3, 24, 5, entry="fixw_sideinfo"))
    out.append(_mk("fixw_sgd", "fixw", 4, 24, 5, D1=0, D2=0, entry="fixw"))
    out.append(_mk("fixw_side_stf_sgld", "fixw", 3, 24, 5, entry="fixw_sideinfo", epsU=1e-4))
    out.append(_mk("fixw_stf_sgld", "fixw", 4, 24, 5, D1=0, D2=0, entry="fixw", epsU=1e-4))
    return tuple(out)


CASES = _cases()


def key(c):
    """The key of a case's inputs and reference: everything but its name, family and launch path."""
    return "%s_r%d_m%d_%d_n%d_%d_D%d_%d_%d%d%d_e%d_f%d_%g_s%d_%s_t%d" % (
        c.entry, c.r, c.m, c.tail, c.n1, c.n2, c.D1, c.D2, c.langevin, c.stiefel, c.avg, c.epochs, c.nfull,
        c.epsU, c.seed, c.special or "-", c.ntest)


def case_id(c):
    return "%s-%s" % (c.family, c.name)


def fixw(c):
    return c.entry.startswith("fixw")


def abc(c):
    return (A_, B_, C_) if c.entry.endswith("sideinfo") else (1.0, 0.0, 0.0)


def nbatch(c):
    return c.nfull + 1


def expected_mode(c):
    """gpt_cf_last_mode: 1 the Stiefel epoch launch, 2 the lazy SGD epoch launch, 0 launch pairs."""
    if c.stiefel:
        return 1
    if c.langevin or c.D1 > 64 or c.D2 > 64 or c.lazy == "0":
        return 0
    return 2


# ---------------------------------------------------------------------------------------- inputs
def _round3(x):
    return float("%.3g" % x)


def _rms(a):
    return math.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64))))


def _raw(c, sigma_u):
    r, m, n1, n2, D1, D2 = c.r, c.m, c.n1, c.n2, c.D1, c.D2
    N = c.nfull * m + c.tail
    rng = np.random.default_rng((4201, c.seed, r, m, c.tail, D1, n1))
    u = rng.integers(0, n1 - 1, N)              # in the first epoch's order; the last id has none
    v = rng.integers(0, n2 - 1, N)
    ud = (rng.random((n1, D1)) < (0.15 if D1 > 32 else 0.4)).astype(np.float64)
    md = (rng.random((n2, D2)) < 0.4).astype(np.float64)
    if c.special == "oneuser":
        u[m:2 * m] = 2
    elif c.special == "distinct":
        u[:m] = rng.permutation(n1 - 1)[:m]
        v[:m] = rng.permutation(n2 - 1)[:m]
        assert len(set(u[:m])) == m and len(set(v[:m])) == m
    elif c.special == "noneall":                 # column 0: no rating of batch 1, every one of batch 2
        hu, hv = (n1 - 1) // 2, (n2 - 1) // 2
        u[:m], u[m:2 * m] = rng.integers(0, hu, m), rng.integers(hu, n1 - 1, m)
        v[:m], v[m:2 * m] = rng.integers(0, hv, m), rng.integers(hv, n2 - 1, m)
        ud[:, 0] = np.arange(n1) >= hu
        md[:, 0] = np.arange(n2) >= hv
    elif c.special == "lastcol":
        ud[::3, D1 - 1] = 1.0
        ud[1::3, D1 - 1] = 0.0
    zu, zv = np.bincount(u).argmax(), np.bincount(v).argmax()
    ud[zu], md[zv] = 0.0, 0.0                    # a user and a movie without features, both rated
    if c.special == "noneall":                   # (column 0 stays as stated)
        ud[zu, 0], md[zv, 0] = float(zu >= hu), float(zv >= hv)
    y = rng.integers(1, 6, N).astype(np.float64)
    mu, sd = y.mean(), y.std(ddof=1)
    perm0 = px.randperm(N, RUN_SEED, 0)
    Rating = np.empty((N, 3))
    Rating[perm0] = np.column_stack([u + 1.0, v + 1.0, (y - mu) / sd])
    tu, tv = rng.integers(0, n1, c.ntest), rng.integers(0, n2, c.ntest)
    tu[0], tv[0] = n1 - 1, n2 - 1
    ty = (rng.integers(1, 6, c.ntest) - mu) / sd
    Rtest = np.column_stack([tu + 1.0, tv + 1.0, ty])
    w0 = rng.standard_normal((r, r)) / math.sqrt(r)
    if c.stiefel:
        U0 = np.linalg.qr(rng.standard_normal((n1 + D1, r)))[0]
        V0 = np.linalg.qr(rng.standard_normal((n2 + D2, r)))[0]
    else:
        U0 = sigma_u * rng.standard_normal((n1 + D1, r))
        V0 = sigma_u * rng.standard_normal((n2 + D2, r))
    return dict(Rating=Rating, Rtest=Rtest, UserData=ud, MovieData=md, w0=np.asfortranarray(w0),
                U0=np.asfortranarray(U0), V0=np.asfortranarray(V0), N=N, sigma_u=sigma_u)


@functools.lru_cache(maxsize=None)
def _inputs(k):
    c = _BY_KEY[k]
    for halvings in range(34):
        p = _raw(c, SIGMA_U_TOP / 2 ** halvings)
        p.update(_tune(c, p))
        if c.stiefel or p["pred_rms"] <= PRED_MAX:
            break
    else:
        raise AssertionError("no sigma_u keeps %s bounded" % k)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def inputs(c):
    """Rating (N, 3), Rtest (Ntest, 3), UserData (n1, D1), MovieData (n2, D2), w0, U0, V0 and the
    step sizes signal_var, epsw, epsU, ystd with the step-1 shares they were tuned to."""
    return _inputs(key(c))


def _tune(c, p):
    be = F64
    st = _State(be, c, dict(p, signal_var=1.0, epsw=0.0, epsU=0.0, ystd=1.0))
    idx = px.randperm(p["N"], RUN_SEED, 0)[:c.m]
    g = st.gradients(idx, None, False)
    rows = np.concatenate([g["gradU"][g["touchedU"]], g["gradV"][g["touchedV"]]])
    rU = _rms(rows)                                            # ∝ 1/σ²
    r0 = _rms(np.concatenate([p["U0"], p["V0"]]))
    if c.stiefel:
        epsU = c.epsU
        sv = _round3(math.sqrt(epsU) * rU / 2)
        share_U = math.sqrt(epsU) * rU / sv / 2
    elif c.langevin:
        epsU = _round3((SGD_EUCLID_SHARE * r0) ** 2)
        sv = _round3(math.sqrt(epsU) * rU / 2)
        share_U = math.sqrt(epsU) * rU / sv / 2
    else:
        sv = _round3(DECAY * 2 * p["sigma_u"] ** 2 / (SGD_EUCLID_SHARE * 2 * r0 / rU))
        epsU = _round3(SGD_EUCLID_SHARE * 2 * r0 * sv / rU)
        share_U = epsU * rU / sv / 2 / r0
    st = _State(be, c, dict(p, signal_var=sv, epsw=0.0, epsU=epsU, ystd=1.0))
    rw = _rms(st.gradients(idx, None, False)["gradw"])
    if c.langevin:
        epsw = _round3(min(1.0, (2 / rw) ** 2))
        share_w = math.sqrt(epsw) * rw / 2
    else:
        epsw = _round3(SGD_EUCLID_SHARE * 2 * _rms(p["w0"]) / rw)
        share_w = epsw * rw / 2 / _rms(p["w0"])
    if fixw(c):
        epsw, share_w = 0.0, float("nan")
    q = dict(p, signal_var=sv, epsw=epsw, epsU=epsU, ystd=1.0)
    out = run_numpy(c, q)
    U, V = out["U"][-1], out["V"][-1]
    w = p["w0"] if out["w"] is None else out["w"][-1]
    a, b, cc = abc(c)
    uidx, vidx = M.side_rows(p["UserData"], p["MovieData"])
    with np.errstate(all="ignore"):
        pred_rms = _rms(M.predict(p["Rtest"], U, V, w, uidx, vidx, a, b, cc))
    if not 0 < pred_rms < 1e30:
        pred_rms = 1e30
    ystd = _round3(2 / pred_rms)
    return dict(signal_var=sv, epsw=epsw, epsU=epsU, ystd=ystd, share_U=share_U, share_w=share_w,
                decay=1.0 - epsU / (2 * p["sigma_u"] ** 2), pred_rms=pred_rms)


def digest(c):
    p = inputs(c)
    h = hashlib.sha256(key(c).encode())
    for name in ("Rating", "Rtest", "UserData", "MovieData", "w0", "U0", "V0"):
        a = np.asfortranarray(p[name])
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    h.update(np.array([p["sigma_u"], p["signal_var"], p["epsw"], p["epsU"], p["ystd"]]).tobytes())
    return h.hexdigest()


def perturbed(c, seed=0):
    """The inputs with every rating, w0, U0 and V0 moved to a neighbouring double."""
    p = dict(inputs(c))
    rng = np.random.default_rng((977, seed))
    for name in ("Rating", "Rtest", "w0", "U0", "V0"):
        a = p[name]
        b = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
        if name in ("Rating", "Rtest"):
            b[:, :2] = a[:, :2]
        p[name] = np.asfortranarray(b)
    return p


# ------------------------------------------------------------------- the restatement of record
def entry_args(c, p):
    """(positional arguments, keywords) of the case's entry, the same for oracle.movielens_ref and
    gpt_amd.movielens."""
    a, b, cc = abc(c)
    head = (p["Rating"], p["UserData"], p["MovieData"], p["Rtest"], p["signal_var"], p["sigma_u"])
    tail = (0, c.epochs, RUN_SEED, YMEAN, p["ystd"])
    if c.entry == "fullw_sideinfo":
        args = head + (SIGMA_W, p["w0"], c.m, p["epsw"], p["epsU"], a, b, cc) + tail
    elif c.entry == "fixw_sideinfo":
        args = head + (p["w0"], c.m, p["epsU"], a, b, cc) + tail
    elif c.entry == "fullw":
        args = head + (SIGMA_W, p["w0"], c.m, p["epsw"], p["epsU"]) + tail
    else:
        args = head + (p["w0"], c.m, p["epsU"]) + tail
    return args, dict(langevin=c.langevin, stiefel=c.stiefel, avg=c.avg, U_init=p["U0"], V_init=p["V0"])


def standard(c, res):
    """An entry's result tuple -> dict(w, U, V (epoch first), testpred (T, Ntest), rmse (T, 2))."""
    res = tuple(res)
    if fixw(c):
        res = (None,) + res
    w, U, V, tp, trm, tsm = res
    return dict(w=None if w is None else np.moveaxis(w, -1, 0).copy(), U=np.moveaxis(U, -1, 0).copy(),
                V=np.moveaxis(V, -1, 0).copy(), testpred=np.asarray(tp).T.copy(),
                rmse=np.column_stack([trm, tsm]))


def run_numpy(c, p=None):
    """oracle.movielens_ref's restatement from the injected state."""
    p = inputs(c) if p is None else p
    args, kw = entry_args(c, p)
    return standard(c, getattr(M, "GPT_" + c.entry)(*args, **kw))


def expm_norms(c):
    """‖·‖₁ of every expm argument of the numpy restatement (Stiefel cases)."""
    norms = []
    orig = R.expm

    def logged(A):
        norms.append(np.abs(A).sum(axis=0).max() if A.size else 0.0)
        return orig(A)

    with SC.patched(expm=logged):
        run_numpy(c)
    return np.array(norms)


# -------------------------------------------------- the step, on float64 or on mpmath numbers
class _F64Backend:
    obj = False

    def arr(self, a):
        return np.array(a, dtype=np.float64)

    def num(self, x):
        return float(x)

    def sqrt(self, x):
        return math.sqrt(x)

    def normals(self, count, seed, c1, c2, c3):
        return px.normals(count, seed, c1, c2, c3)

    def proj(self, U, V):
        return R.proj(U, V)

    def geod(self, U, mom, t):
        out, ok = R.geod(U, mom, t)
        assert ok
        return out

    def clip(self, a):
        return np.clip(a, 1.0, 5.0)


class _MPBackend:
    obj = True

    def arr(self, a):
        return SC._mpa(a)

    def num(self, x):
        import mpmath as mp
        return mp.mpf(float(x))

    def sqrt(self, x):
        import mpmath as mp
        return mp.sqrt(x)

    def normals(self, count, seed, c1, c2, c3):
        return SC._mp_normals(count, seed, c1, c2, c3)

    def proj(self, U, V):
        return SC._mp_proj(U, V)

    def geod(self, U, mom, t):
        return SC._mp_geod(U, mom, t)

    def clip(self, a):
        return np.frompyfunc(lambda x: min(max(x, 1), 5), 1, 1)(a)


F64, MP = _F64Backend(), _MPBackend()

# The defect table of tests/test_cf_cases.py: small faults of a device kernel, restated.
DEFECTS = {
    "feature_sum_drops_last": "a feature row's sum omits the last rating that carries it",
    "duplicate_user_lost": "a duplicate user's later rating is missing from that user's row",
    "movie_side_b": "the movie side's feature gradient scaled with b instead of c",
    "tail_scale": "the tail batch scaled by N/m instead of N/B",
    "skipped_row_decay": "a row no batch of an epoch touches decayed one step too few",
    "gradw_col17": "column 17 of gradw zero at r = 20",
    "noise_epoch_base": "the second epoch's U noise drawn with the first epoch's step numbers",
    "avg_counter": "the running average dividing by counter instead of counter + 1",
}


class _State:
    def __init__(self, be, c, p):
        self.be, self.c, self.p = be, c, p
        a, b, cc = abc(c)
        n = be.num
        self.a, self.b, self.cc = n(a), n(b), n(cc)
        self.N = p["N"]
        self.u = p["Rating"][:, 0].astype(np.int64) - 1
        self.v = p["Rating"][:, 1].astype(np.int64) - 1
        self.y = be.arr(p["Rating"][:, 2])
        self.AU = self.incidence(self.u, p["UserData"], self.b)
        self.AV = self.incidence(self.v, p["MovieData"], self.cc)
        self.w, self.U, self.V = be.arr(p["w0"]), be.arr(p["U0"]), be.arr(p["V0"])
        self.sv, self.epsw, self.epsU = n(p["signal_var"]), n(p["epsw"]), n(p["epsU"])
        self.su2, self.sw2 = n(p["sigma_u"]) * n(p["sigma_u"]), n(SIGMA_W) * n(SIGMA_W)

    def incidence(self, ids, data, scale):
        """(count, rows): 1 at a rating's own row, `scale` at each of its feature rows, so that
        sumU = A·U (:476-477) and gradU = a·Aᵀ·Utemp/σ² (:484-487)."""
        n, D = data.shape
        A = np.zeros((len(ids), n + D), dtype=object if self.be.obj else np.float64)
        if self.be.obj:
            A[:] = 0
        for i, k in enumerate(ids):
            A[i, k] = 1
            for f in np.flatnonzero(data[k]):
                A[i, n + f] = scale
        return A

    def gradients(self, idx, defect, is_tail):
        c, be = self.c, self.be
        AU, AV = self.AU[idx], self.AV[idx]
        B = len(idx)
        sumU, sumV = AU @ self.U, AV @ self.V
        e = self.y[idx] - ((sumU @ self.w) * sumV).sum(axis=1) * self.a
        Ut = (sumV * e[:, None]) @ self.w.T
        Vt = (sumU * e[:, None]) @ self.w
        touchedU = np.array([any(AU[:, j] != 0) for j in range(AU.shape[1])])
        touchedV = np.array([any(AV[:, j] != 0) for j in range(AV.shape[1])])
        GU, GV = AU, AV
        if defect == "feature_sum_drops_last":
            GU = AU.copy()
            for j in range(c.n1, AU.shape[1]):
                hit = np.flatnonzero(AU[:, j] != 0)
                if len(hit):
                    GU[hit[-1], j] = 0
                    break
        elif defect == "duplicate_user_lost":
            GU = AU.copy()
            ub = self.u[idx]
            for i in range(1, B):
                if ub[i] in ub[:i]:
                    GU[i, ub[i]] = 0
                    break
        elif defect == "movie_side_b":
            GV = AV.copy()
            feat = GV[:, c.n2:]
            feat[feat != 0] = self.b
        scale = be.num(self.N) / (c.m if defect == "tail_scale" and is_tail else B)
        gradU = (GU.T @ Ut) * (self.a * scale / self.sv)
        gradV = (GV.T @ Vt) * (self.a * scale / self.sv)
        gradw = (sumU.T @ (sumV * e[:, None])) * (scale / self.sv) - self.w / self.sw2
        if defect == "gradw_col17" and c.r == 20:
            gradw[:, 16] = gradw[:, 16] * 0
        return dict(gradw=gradw, gradU=gradU, gradV=gradV, touchedU=touchedU, touchedV=touchedV)

    def predict(self, ratings, data_u, data_v):
        AU = self.incidence(ratings[:, 0].astype(np.int64) - 1, data_u, self.b)
        AV = self.incidence(ratings[:, 1].astype(np.int64) - 1, data_v, self.cc)
        return (((AU @ self.U) @ self.w) * (AV @ self.V)).sum(axis=1) * self.a


def _run(be, c, p, defect=None):
    st = _State(be, c, p)
    r, N, nb = c.r, p["N"], nbatch(c)
    re = r + (r & 1)
    sq, sqw = be.sqrt(st.epsU), be.sqrt(st.epsw)
    ystd, ymean = be.num(p["ystd"]), be.num(YMEAN)
    truth_tr = st.y * ystd + ymean
    truth_te = be.arr(p["Rtest"][:, 2]) * ystd + ymean
    trainpred, testpred = st.y * 0, truth_te * 0
    out = dict(w=[], U=[], V=[], testpred=[], rmse=[])
    counter = step = 0
    for epoch in range(c.epochs):
        perm = px.randperm(N, RUN_SEED, epoch)
        untouched = [np.ones(st.U.shape[0], bool), np.ones(st.V.shape[0], bool)]
        for bt in range(nb):
            idx = perm[c.m * bt: min(c.m * (bt + 1), N)]
            g = st.gradients(idx, defect, bt == nb - 1)
            untouched[0] &= ~g["touchedU"]
            untouched[1] &= ~g["touchedV"]
            if not fixw(c):
                st.w = st.w + g["gradw"] * (st.epsw / 2)
                if c.langevin:
                    z = be.normals(r * r, RUN_SEED, step, px.CF_W_NOISE, 0).reshape((r, r), order="F")
                    st.w = st.w + z * sqw
            new = []
            for which, (Mx, G) in enumerate(((st.U, g["gradU"]), (st.V, g["gradV"]))):
                xi = None
                if c.langevin:
                    ns = step % nb if defect == "noise_epoch_base" and which == 0 else step
                    xi = be.normals(re * Mx.shape[0], RUN_SEED, ns, px.CF_UV_NOISE, which).reshape(
                        (Mx.shape[0], re))[:, :r]
                if c.stiefel:
                    drive = G * (sq / 2)
                    Mn = be.geod(Mx, be.proj(Mx, drive + xi if c.langevin else drive), sq)
                else:
                    Mn = Mx + (G - Mx / st.su2) * (st.epsU / 2)
                    if c.langevin:
                        Mn = Mn + xi * sq
                    if defect == "skipped_row_decay" and bt == nb - 1:
                        Mn[untouched[which]] = Mx[untouched[which]]
                new.append(Mn)
            st.U, st.V = new
            step += 1
        if not c.avg:
            counter = 0
        div = max(counter, 1) if defect == "avg_counter" else counter + 1
        trainpred = (trainpred * counter + st.predict(p["Rating"], p["UserData"], p["MovieData"])) / div
        testpred = (testpred * counter + st.predict(p["Rtest"], p["UserData"], p["MovieData"])) / div
        ft, fs = be.clip(trainpred * ystd + ymean), be.clip(testpred * ystd + ymean)
        out["rmse"].append([be.sqrt(((truth_tr - ft) ** 2).sum() / N),
                            be.sqrt(((truth_te - fs) ** 2).sum() / len(fs))])
        out["w"].append(st.w.copy())
        out["U"].append(st.U.copy())
        out["V"].append(st.V.copy())
        out["testpred"].append(fs)
        counter += 1
    dt = object if be.obj else np.float64
    res = {k: np.array(v, dtype=dt) for k, v in out.items()}
    if fixw(c):
        res["w"] = None
    return res


def run_f64(c, defect=None, p=None):
    """The step of this file on float64: the numpy restatement that carries the defect table."""
    return _run(F64, c, inputs(c) if p is None else p, defect)


def compute(c):
    """The case in mpmath: dict(w, U, V, testpred, rmse) of object arrays laid out as run_numpy's."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _run(MP, c, inputs(c))


def pack(c, ref):
    out = {}
    for q in STORED:
        if ref[q] is not None:
            out[q + "_hi"], out[q + "_lo"] = SC._dd(ref[q])
    return out


def as_reference(run):
    return {q: (run[q], np.zeros_like(run[q])) for q in STORED if run[q] is not None}


def on_manifold(c):
    return bool(c.stiefel)


def rel_err(out, ref, manifold=False):
    """{quantity: worst error over the stored epochs}: w, U, V and testpred_store as max|Δ| / max|x|
    of the epoch, each RMSE relative to itself; with `manifold` also colnorm of U and V
    (oracle.step_cases.colnorm).  ref is reference()'s dict, or another run's."""
    if not isinstance(ref["U"], tuple):
        ref = as_reference(ref)
    res = {}
    for q in ("w", "U", "V", "testpred"):
        if q not in ref or out[q] is None:
            continue
        hi, lo = ref[q]
        res[q] = max(float(np.abs((out[q][s] - hi[s]) - lo[s]).max() / np.abs(hi[s]).max())
                     for s in range(len(hi)))
    hi, lo = ref["rmse"]
    err = np.abs((out["rmse"] - hi) - lo) / np.abs(hi)
    res["train_rmse"], res["test_rmse"] = float(err[:, 0].max()), float(err[:, 1].max())
    if manifold:
        res["colnorm"] = max(SC.colnorm(out["U"]), SC.colnorm(out["V"]))
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
        a = {s: st[k + "_" + s] for q in STORED for s in (q + "_hi", q + "_lo") if k + "_" + s in st}
    else:
        a = pack(c, compute(c))
    out = {q: (a[q + "_hi"], a[q + "_lo"].astype(np.float64)) for q in STORED if q + "_hi" in a}
    for v in out.values():
        for x in v:
            x.setflags(write=False)
    return out


def reference(c):
    """{quantity: (hi, lo)} of a case from the committed file where the case's digest is there, else
    by mpmath.  Shared and read-only."""
    return _reference(key(c))


def bars():
    st = _stored()
    return {fam: dict(zip(QUANTITIES, st["bar_" + fam])) for fam in FAMILIES}


def measured_u():
    st = _stored()
    return {fam: dict(zip(QUANTITIES, st["u_" + fam])) for fam in FAMILIES}


_BY_KEY = {}
for _c in CASES:
    _BY_KEY.setdefault(key(_c), _c)
