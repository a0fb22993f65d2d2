"""Cases, inputs, the mpmath step and the CPU-side measurements of the SGLD step tests
(tests/test_gpu_step.py on the device, tests/test_step_cases.py on the CPU).

A case is (family, (n, D, r, Q, m, tail), εU, seed): N = m + tail rows, burnin = 0, maxepoch = 2,
three steps (a full batch, the ragged last batch of the epoch, the first batch of the next epoch),
store_every = 1, diag on.  Inputs are regenerated from shape and seed as
tests/test_gpu_parity.py::make_problem does and identified by a SHA-256 digest; the initial state is
R.init_state's and is injected on the device (w_init / U_init), so no polar-factor difference is
charged to the step.

Step sizes (inputs): σ² is chosen per case so that the rms entry of √εU·gradU/2 at step 1 is 1,
the size of the noise entries, and εw = (2 / rms gradw)² (at most 1) so that εw·‖gradw‖/2 and
√εw·‖ξ_w‖ are equal; both are rounded to three digits, so they are the same doubles wherever the
inputs are.  SGD + Euclidean takes εU = SGD_EUCLID_SHARE·2·rms U / rms gradU (a move of a quarter of
U itself: at the whole of U three steps amplify a one-ulp change of the inputs past COND_MAX);
RMSprop tunes σ² for its own drive √mean(εU_k)·gradU_k/2; the classifier has no σ², so there
εU = (2 / rms gradU)² and εw = (2 / rms gradw)², each capped (cls_epsU_max, 1), and its shares are
recorded, not tuned.

The reference (compute) is the reference's formulas (GPT_SGLD.jl:384-437 as gpt_sgld_ref restates
them: gradients, proj, geod, and each family's own update) on the exact doubles of the inputs in
mpmath at MP_DIGITS digits: V's factors multiplied in k order, the true matrix exponential
(expm_cases.expm_mpf, no Padé form), the normals by Box–Muller in mpmath from the Philox words
(fastmath_cases._bm), the permutations from oracle.philox.  Per step it keeps w, U, ‖gradw‖ and
‖gradU_k‖ as hi (float64) + lo (float32).  tests/golden/step_mp.npz has to stay under 500 KB, which
holds about 30 000 such pairs: U is kept at all three steps where a sample has at most U_FULL
entries, else after the last step only and at every S-th entry in column-major order, S the
smallest stride coprime to n that leaves at most U_FULL of them: S < n, so every column of every
dimension (and class) is held, and every row, since S·t mod n passes every row in n consecutive
t.  The small cases keep every element.  The fourth quantity needs no stored reference: the columns
of a U on the Stiefel path have norm one, so colnorm = max |Σ_j U_jl² − 1|/2 (math.fsum) is held to
the bar measured on the restatements in the same way.

Nothing here comes from the device.  Test infrastructure: numpy / mpmath, no GPU.
"""
import collections
import contextlib
import functools
import hashlib
import math
import os

import numpy as np

from . import expm_cases as EC
from . import fastmath_cases as FC
from . import gpt_sgld_ref as R
from . import philox as px

MP_DIGITS = 50
STEPS = 3
NCLS = 3
ALPHA = 0.9              # RMSprop's moving-average factor (tests/test_gpu_parity.py)
RUN_SEED = 23
U_FULL = 640
# The classifier's εU cap on the Stiefel variants: at 1e-2 the numpy restatement's own error against
# mpmath passes B_MAX / MARGIN on the (64, 4, 5, 30) shape.
CLS_EPSU_MAX = 1e-3
SGD_EUCLID_SHARE = 0.25  # SGD + Euclidean: εU·rms gradU/2 = this × rms U
MARGIN = 8               # device bar B = MARGIN·u (tests/test_gpu_step.py explains the factor)
B_MAX = 1e-13
COND_MAX = 1e-14
NORM_MAX = 30.0
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                      "step_mp.npz")

REG = "sgld_stiefel"
REG_FAMILIES = {          # family: (langevin, stiefel)
    "sgld_stiefel": (True, True), "sgd_stiefel": (False, True),
    "sgld_euclid": (True, False), "sgd_euclid": (False, False),
}
CLS_FAMILIES = {"cls_" + k: v for k, v in REG_FAMILIES.items()}
FAMILIES = tuple(REG_FAMILIES) + ("wonly", "rmsprop") + tuple(CLS_FAMILIES)
QUANTITIES = ("w", "U", "norms", "colnorm")

Case = collections.namedtuple("Case", "family shape epsU seed note")


def _cases():
    out = []

    def reg(shape, note, epsU=1e-6, seed=0):
        out.append(Case(REG, tuple(shape), epsU, seed, note))

    # chain engine, D <= 4 build (WV = 4)
    reg((16, 3, 2, 6, 8, 3), "chain D<=4")
    reg((16, 3, 2, 6, 8, 3), "chain D<=4, large step", 1e-4)
    reg((64, 4, 5, 30, 8, 1), "chain D<=4, tail of one row")
    reg((64, 4, 5, 30, 8, 1), "chain D<=4, tail of one row, large step", 1e-4)
    reg((500, 4, 5, 200, 40, 9), "chain D<=4, J = 8, two V tasks per wave", seed=1)
    # chain engine, D >= 5 build
    reg((200, 5, 3, 70, 20, 7), "chain D>=5, half-filled block")
    reg((258, 6, 4, 130, 15, 4), "chain D>=5, two rows in the last block", seed=1)
    reg((512, 8, 5, 256, 33, 5), "chain D>=5, n and Q maxima, a 64-member run, odd m", seed=7)
    reg((300, 7, 2, 100, 16, 2), "chain D>=5, r = 2")
    # chain edges
    reg((20, 3, 1, 1, 8, 3), "rank one")
    reg((32, 1, 3, 3, 7, 2), "D = 1")
    reg((17, 3, 2, 6, 8, 3), "odd n in one block")
    # wave engine, one per instantiated rank
    reg((40, 3, 6, 30, 16, 5), "wave r = 6")
    reg((40, 3, 6, 30, 16, 5), "wave r = 6, large step", 1e-4)
    reg((96, 4, 8, 50, 12, 3), "wave r = 8")
    reg((100, 4, 10, 60, 30, 7), "wave r = 10")
    reg((200, 5, 12, 100, 32, 9), "wave r = 12, J = 4")
    reg((77, 6, 15, 90, 9, 4), "wave r = 15, odd n, butterfly phidotU")
    reg((130, 4, 16, 120, 64, 11), "wave r = 16, m = 64, one-pass 2r = 32 solve")
    reg((60, 3, 20, 30, 8, 3), "wave r = 20, n = 3r")
    reg((64, 12, 20, 60, 10, 3), "wave r = 20, D = 12")
    # grid engine only
    reg((101, 2, 3, 9, 10, 3), "odd n past one block")
    reg((40, 12, 2, 24, 15, 5), "D > 8 lane-per-q V-phase", seed=1)
    small = ((16, 3, 2, 6, 8, 3), (24, 4, 3, 10, 8, 5))
    for fam in ("sgd_stiefel", "sgld_euclid", "sgd_euclid", "wonly", "rmsprop") + tuple(CLS_FAMILIES):
        for s in small:
            out.append(Case(fam, s, RMS_EPS_SMALL if fam == "rmsprop" else 1e-6,
                            VARIANT_SEEDS.get((fam, s[0]), 0), "variant family"))
    out.append(Case("rmsprop", (64, 4, 5, 30, 8, 1), RMS_EPS_LARGE, 7, "variant family, larger shape"))
    out.append(Case("cls_sgld_stiefel", (64, 4, 5, 30, 8, 1), 1e-6, 0, "variant family, larger shape"))
    return tuple(out)


RMS_EPS_SMALL, RMS_EPS_LARGE = 1e-5, 1e-6      # as RMS_CASES of tests/test_gpu_parity.py
# Seeds other than 0 are the first that meet the conditions of tests/test_step_cases.py (status 0,
# every expm argument within NORM_MAX, the conditioning limit, and for the n = 512 case a longest
# run of I[:, k] of exactly the chain engine's 64); seed 0 of those cases does not.
VARIANT_SEEDS = {("rmsprop", 24): 7, ("sgd_euclid", 24): 1}
CASES = _cases()
WAVE_RANKS = (6, 8, 10, 12, 15, 16, 20)


def engines(c):
    """The engines that take a case, by the predicates of tests/test_gpu_parity.py and the chain
    engine's limit of 64 core entries per value of I[:, k]; the variant families have one kernel
    path each (None: the entry takes no engine)."""
    if c.family != REG:
        return ("grid",) if c.family in REG_FAMILIES else (None,)
    n, D, r, Q, m, tail = c.shape
    out = ["grid"]
    I = inputs(c)["I"]
    longest = max(np.bincount(I[:, k]).max() for k in range(D))
    if D <= 8 and r <= 5 and n <= 512 and (n <= 64 or n % 2 == 0) and Q <= 256 and longest <= 64:
        out.append("chain")
    if r in WAVE_RANKS and 3 * r <= n <= 256 and m <= 64:
        out.append("wave")
    return tuple(out)


def key(c):
    return "%s_%s_e%g_s%d" % (c.family, "_".join(str(v) for v in c.shape), c.epsU, c.seed)


def case_id(c):
    return "%s-%s-%g" % (c.family, "-".join(str(v) for v in c.shape), c.epsU)


# ---------------------------------------------------------------------------------------- inputs
def make_problem(n, D, N, r, Q, seed=0):
    """tests/test_gpu_parity.py::make_problem."""
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
    return dict(phi=phi, I=I, y=y)


def _round3(x):
    return float("%.3g" % x)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    n, D, r, Q, m, tail = c.shape
    N = m + tail
    p = make_problem(n, D, N, r, Q, seed=11 + 100 * c.seed)
    stiefel = dict(REG_FAMILIES, **CLS_FAMILIES).get(c.family, (True, True))[1]
    if c.family in CLS_FAMILIES:
        f = p["y"] - np.median(p["y"])
        p["y"] = (1 + np.clip(np.floor((f - f.min()) / (np.ptp(f) + 1e-12) * NCLS), 0, NCLS - 1)).astype(float)
        w0, U0 = R.init_state_cls(n, r, D, Q, NCLS, 7 + c.seed, stiefel)
    else:
        w0, U0 = R.init_state(n, r, D, Q, 7 + c.seed, stiefel)
    p.update(w0=w0, U0=np.asfortranarray(U0), N=N)
    p.update(_tune(c, p))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def inputs(c):
    """phi (n, D, N), y (N), I (Q, D), the initial state w0, U0, and the step sizes signal_var,
    epsw, epsU (the RMSprop ε in both for that family), with the step-1 shares they were tuned to."""
    return _inputs(c)


def _first_batch(c, p):
    idx = px.randperm(p["N"], RUN_SEED, 0)[:c.shape[4]]
    return p["phi"][:, :, idx], p["y"][idx]


def cls_epsU_max(family):
    """The classifier's first move is a geodesic step whatever the variant; from the Euclidean
    variants' unscaled randn U (column norms √n) the expm argument passes 30 beyond t = 1e-3."""
    return CLS_EPSU_MAX if CLS_FAMILIES[family][1] else 1e-6


def _tune(c, p):
    n, D, r, Q, m, tail = c.shape
    N = p["N"]
    pb, yb = _first_batch(c, p)
    if c.family in CLS_FAMILIES:
        gw, gU = _cls_gradients(pb, yb, p["w0"], p["U0"], p["I"], N)
        rw = math.sqrt(np.mean(np.square(gw)))
        rU = math.sqrt(np.mean(np.square(gU)))
        epsw = _round3(min(1.0, (2 / rw) ** 2))
        epsU = _round3(min(cls_epsU_max(c.family), (2 / rU) ** 2))
        return dict(signal_var=1.0, epsw=epsw, epsU=epsU, share_w=math.sqrt(epsw) * rw / 2,
                    share_U=math.sqrt(epsU) * rU / 2)
    g = R.gradients(pb, yb, p["w0"], p["U0"], p["I"], N, 1.0)
    rU = math.sqrt(np.mean(np.square(g["gradU"])))                 # ∝ 1/σ²
    if c.family == "rmsprop":
        eps = c.epsU
        sv = 1.0
        for _ in range(4):                                         # drive ∝ 1/σ but for λ
            sv = _round3(sv * _rms_drive(g["gradU"] / sv, eps, N, m) ** 2)
        return dict(signal_var=sv, epsw=eps, epsU=eps, share_w=float("nan"),
                    share_U=_rms_drive(g["gradU"] / sv, eps, N, m))
    tU = 1e-6 if c.family in ("sgd_euclid", "wonly") else c.epsU
    sv = _round3(math.sqrt(tU) * rU / 2)
    g = R.gradients(pb, yb, p["w0"], p["U0"], p["I"], N, sv)
    rw = math.sqrt(np.mean(np.square(g["gradw"])))
    rU = math.sqrt(np.mean(np.square(g["gradU"])))
    epsw = _round3(min(1.0, (2 / rw) ** 2))
    epsU = c.epsU
    share_U = math.sqrt(epsU) * rU / 2
    if c.family == "sgd_euclid":
        ru0 = math.sqrt(np.mean(np.square(p["U0"])))
        epsU = _round3(SGD_EUCLID_SHARE * 2 * ru0 / rU)
        share_U = epsU * rU / 2 / ru0
    return dict(signal_var=sv, epsw=epsw, epsU=epsU, share_w=math.sqrt(epsw) * rw / 2, share_U=share_U)


def _rms_drive(gradU_batchsum, eps, N, B):
    """rms of RMSprop's step-1 drive √mean(εU_k)·gradU_k/2 (gpt_sgld_ref.GPT_SGLDERM_RMSprop) from
    gradients()'s gradU = (N/B)·Ψ·res/σ²."""
    ghat = gradU_batchsum / N
    eU = eps / (np.sqrt((1 - ALPHA) * ghat ** 2) + R.RMS_LAMBDA)
    sk = np.sqrt(eU.mean(axis=(0, 1)))
    return math.sqrt(np.mean(np.square(sk[None, None, :] * (ghat * N) / 2)))


def _cls_gradients(pb, yb, w, U, I, N):
    """The classifier's step-1 gradients of every class, stacked (gpt_sgld_ref.GPTclassification)."""
    ncls = w.shape[1]
    fhat = np.stack([R.computefhat(R.computeV(R.phidotU(U[..., c], pb), I), w[:, c])
                     for c in range(ncls)], axis=1)
    lse = np.array([R.logsumexp(fhat[i, :]) for i in range(len(yb))])
    gw, gU = [], []
    for c in range(ncls):
        res = (yb == c + 1).astype(np.float64) - np.exp(fhat[:, c] - lse)
        a, b = R.gradients_res(pb, res, w[:, c], U[..., c], I, N)
        gw.append(a)
        gU.append(b)
    return np.stack(gw), np.stack(gU)


def digest(c):
    p = inputs(c)
    h = hashlib.sha256(key(c).encode())
    for name in ("phi", "y", "I", "w0", "U0"):
        a = np.asfortranarray(p[name])
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    h.update(np.array([p["signal_var"], p["epsw"], p["epsU"]]).tobytes())
    return h.hexdigest()


def u_select(c):
    """(steps, flat column-major indices) of the U entries the fixture keeps (module docstring)."""
    n, D, r, Q, m, tail = c.shape
    shape = (n, r, D) + ((NCLS,) if c.family in CLS_FAMILIES else ())
    size = int(np.prod(shape))
    if size <= U_FULL:
        return tuple(range(STEPS)), np.arange(size)
    S = -(-size // U_FULL)
    while math.gcd(S, n) != 1:
        S += 1
    return (STEPS - 1,), np.arange(0, size, S)


# --------------------------------------------------------------------- the fp64 restatements
@contextlib.contextmanager
def patched(**attrs):
    """gpt_sgld_ref with some of its functions replaced (the mutants, the expm norm log)."""
    old = {k: getattr(R, k) for k in attrs}
    for k, v in attrs.items():
        setattr(R, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(R, k, v)


def run_numpy(c, p=None):
    """Three steps of the numpy restatement: dict(w (3, Q[, C]), U (3, n, r, D[, C]) or None,
    norms (3, [C,] 1 + D), status)."""
    p = inputs(c) if p is None else p
    n, D, r, Q, m, tail = c.shape
    a = (p["phi"], p["y"])
    kw = dict(w_init=p["w0"], U_init=p["U0"], max_steps=STEPS, record=True)
    if c.family in REG_FAMILIES:
        lang, stf = REG_FAMILIES[c.family]
        ws, Us, info = R.GPTregression(*a, p["signal_var"], p["I"], r, Q, m, p["epsw"], p["epsU"], 0, 2,
                                       RUN_SEED, langevin=lang, stiefel=stf, **kw)
        norms = np.column_stack([info["gradw_norm"], np.array(info["gradU_norm"])])
    elif c.family == "wonly":
        ws, _, info = R.GPT_SGLDERMw(*a, p["signal_var"], p["I"], r, Q, m, p["epsw"], 0, 2, RUN_SEED, **kw)
        Us, norms = None, np.array(info["gradw_norm"])[:, None]
    elif c.family == "rmsprop":
        ws, Us, info = R.GPT_SGLDERM_RMSprop(*a, p["signal_var"], p["I"], r, Q, m, p["epsU"], ALPHA, 0, 2,
                                             RUN_SEED, **kw)
        norms = np.column_stack([info["gradw_norm"], np.array(info["gradU_norm"])])
    else:
        lang, stf = CLS_FAMILIES[c.family]
        ws, Us, info = R.GPTclassification(*a, p["I"], r, Q, m, p["epsw"], p["epsU"], 0, 2, RUN_SEED,
                                           langevin=lang, stiefel=stf, **kw)
        norms = np.concatenate([np.array(info["gradw_norm"])[:, :, None],
                                np.array(info["gradU_norm"])], axis=2)
    return standard(ws, Us, norms, info["status"])


def standard(ws, Us, norms, status=0):
    """Stores with the step last (as every sampler returns them) -> step first, three steps."""
    return dict(w=np.moveaxis(ws, -1, 0)[:STEPS].copy(),
                U=None if Us is None else np.moveaxis(Us, -1, 0)[:STEPS].copy(),
                norms=np.asarray(norms)[:STEPS].copy(), status=status)


def run_cpp(c):
    """The C++ restatement (oracle/cpu_lib.py) where it implements the family: SGLD + Stiefel
    regression, w and U only."""
    from . import cpu_lib
    p = inputs(c)
    n, D, r, Q, m, tail = c.shape
    ws, Us, st = cpu_lib.GPTregression_from(p["phi"], p["y"], p["signal_var"], p["I"], r, Q, m, p["epsw"],
                                            p["epsU"], 0, 2, RUN_SEED, p["w0"], p["U0"], max_steps=STEPS)
    return standard(ws, Us, np.zeros((STEPS, 1 + D)), st)


def expm_norms(c):
    """‖·‖₁ of every expm argument of the numpy restatement's three steps."""
    norms = []
    orig = R.expm

    def logged(A):
        norms.append(np.abs(A).sum(axis=0).max() if A.size else 0.0)
        return orig(A)

    with patched(expm=logged):
        run_numpy(c)
    return np.array(norms)


def perturbed(c, seed=0):
    """The inputs with every double of phi, y, w0 and U0 moved to a neighbouring double (a relative
    2^-53 to 2^-52, the sign drawn per entry)."""
    p = dict(inputs(c))
    rng = np.random.default_rng((977, seed))
    for name in ("phi", "y", "w0", "U0"):
        if name == "y" and c.family in CLS_FAMILIES:
            continue
        a = p[name]
        p[name] = np.asfortranarray(np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf)))
    return p


def on_manifold(c):
    """Whether the family's U stays on the Stiefel manifold (every move of U a geodesic step)."""
    return c.family in ("rmsprop",) or dict(REG_FAMILIES, **CLS_FAMILIES).get(c.family, (0, 0))[1]


def colnorm(U):
    """max |‖column‖² − 1| / 2 over every column of U (steps, n, r, ...): the squares summed
    exactly, so the figure resolves well below 2^-53."""
    cols = np.moveaxis(U, 1, -1).reshape(-1, U.shape[1])
    return max(abs(math.fsum(np.append(col * col, -1.0))) for col in cols) / 2


def as_reference(run):
    """A run's dict in the layout of reference(): (hi, lo = 0) per quantity, every U entry kept."""
    ref = dict(w=(run["w"], np.zeros_like(run["w"])), norms=(run["norms"], np.zeros_like(run["norms"])),
               sel=(tuple(range(STEPS)), slice(None)))
    if run["U"] is not None:
        flat = np.stack([u.ravel(order="F") for u in run["U"]])
        ref["U"] = (flat, np.zeros_like(flat))
    return ref


def rel_err(out, ref, manifold=False):
    """{quantity: worst error over the steps}: w and U as max|Δ| / max|x| of the step, ‖gradw‖
    relative to itself and every ‖gradU_k‖ to the largest of the step (and class); with `manifold`
    also colnorm(out's U).  ref is reference()'s dict, or another run's (as_reference)."""
    if not isinstance(ref["w"], tuple):
        ref = as_reference(ref)
    res = {}
    hi, lo = ref["w"]
    res["w"] = max(np.abs((out["w"][s] - hi[s]) - lo[s]).max() / np.abs(hi[s]).max() for s in range(STEPS))
    hi, lo = ref["norms"]
    err = np.abs((out["norms"] - hi) - lo)
    res["norms"] = float((err[..., :1] / np.abs(hi[..., :1])).max())
    if hi.shape[-1] > 1:
        largest = np.abs(hi[..., 1:]).max(axis=-1, keepdims=True)
        res["norms"] = max(res["norms"], float((err[..., 1:] / largest).max()))
    if out.get("U") is not None and "U" in ref:
        hi, lo = ref["U"]
        steps, idx = ref["sel"]
        res["U"] = max(np.abs((out["U"][s].ravel(order="F")[idx] - hi[i]) - lo[i]).max() / np.abs(hi[i]).max()
                       for i, s in enumerate(steps))
    if manifold:
        res["colnorm"] = colnorm(out["U"])
    return res


# ------------------------------------------------------------------------------- the mutants
def _round40(x):
    m, e = np.frexp(x)
    return np.ldexp(np.round(m * 2.0 ** 40) / 2.0 ** 40, e)


def mutant(k):
    """Context manager: gpt_sgld_ref with the k-th defect of tests/test_step_cases.py."""
    if k == 1:        # a reciprocal without its refinement in the leave-one-out division
        def computeU_phi(V, temp, I):
            out = np.empty((I.shape[0], V.shape[1], I.shape[1]))
            for d in range(I.shape[1]):
                out[:, :, d] = V * _round40(1.0 / temp[d, I[:, d] - 1, :])
            return out
        return patched(computeU_phi=computeU_phi)
    if k == 2:        # the last member of one (k, l) run left out of A
        def computeA(U_phi, w, I, r):
            Q, B, D = U_phi.shape
            A = np.zeros((r, D, B))
            for d in range(D):
                for l in np.unique(I[:, d]):
                    idx = np.nonzero(I[:, d] == l)[0]
                    if d == D - 1 and l == I[0, d] and len(idx) > 1:
                        idx = idx[:-1]
                    A[l - 1, d, :] = w[idx] @ U_phi[idx, :, d]
            return A
        return patched(computeA=computeA)
    if k == 3:        # step 2's temp of the last dimension formed with the U of step 1
        state = dict(calls=0, U=None)

        def phidotU(U, phi):
            t = np.einsum("jki,jlk->kli", phi, U)
            state["calls"] += 1
            if state["calls"] == 2:
                t[-1] = np.einsum("ji,jl->li", phi[:, -1, :], state["U"][:, :, -1])
            state["U"] = U.copy()
            return t
        return patched(phidotU=phidotU)
    if k == 4:        # −w/σ_w² left out of gradw
        orig = R.gradients

        def gradients(phi_batch, y_batch, w, U, I, N, signal_var, sigma_w=1.0):
            g = orig(phi_batch, y_batch, w, U, I, N, signal_var, sigma_w)
            g["gradw"] = g["gradw"] + w / sigma_w ** 2
            return g
        return patched(gradients=gradients)
    if k == 5:        # Uᵀmom taken as (M − Mᵀ)/2, M = UᵀG, with U's columns scaled by 1 + 1e-9
        state = {}
        oproj = R.proj

        def proj(U, V):
            state["M"] = ((1 + 1e-9) * U).T @ V
            return oproj(U, V)

        def geod(U, mom, t):
            n, r = U.shape
            A = (state["M"] - state["M"].T) / 2
            T = np.block([[A, -(mom.T @ mom)], [np.eye(r), A]])
            tmpU = (np.hstack([U, mom]) @ R.expm(t * T)[:, :r]) @ R.expm(-t * A)
            return tmpU / np.linalg.norm(tmpU, axis=0)[None, :], True
        return patched(proj=proj, geod=geod)
    if k == 6:        # the column normalisation skipped
        def geod(U, mom, t):
            n, r = U.shape
            A = U.T @ mom
            T = np.block([[A, -(mom.T @ mom)], [np.eye(r), A]])
            return (np.hstack([U, mom]) @ R.expm(t * T)[:, :r]) @ R.expm(-t * A), True
        return patched(geod=geod)
    raise KeyError(k)


MUTANTS = (1, 2, 3, 4, 5, 6)


# ------------------------------------------------------------------------------ mpmath reference
def _mpa(a):
    """An array of doubles as an object array of mpf (exact)."""
    import mpmath as mp
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for i, v in np.ndenumerate(a):
        out[i] = mp.mpf(float(v))
    return out


def _fn(name):
    import mpmath as mp
    return np.frompyfunc(getattr(mp, name), 1, 1)


def _dd(a):
    """Object array of mpf -> (hi float64, lo float32)."""
    import mpmath as mp
    a = np.asarray(a, dtype=object)
    hi = np.empty(a.shape)
    lo = np.empty(a.shape)
    for i, v in np.ndenumerate(a):
        hi[i] = float(v)
        lo[i] = float(v - mp.mpf(hi[i]))
    return hi, lo.astype(np.float32)


def _mp_normals(count, seed, c1, c2, c3):
    """philox.normals with the Box–Muller step in mpmath."""
    import mpmath as mp
    nblk = (count + 1) // 2
    x0, x1, x2, x3 = px.philox4x32(np.arange(nblk, dtype=np.uint32), c1, c2, c3, seed)
    z = []
    for a, b in zip(px._u53(x0, x1), px._u53(x2, x3)):
        z.extend(FC._bm(mp, a, b)[1:])
    return np.array(z[:count], dtype=object)


def _mp_unoise(n, r, seed, c1, c3):
    """philox.unoise_quads on the U_NOISE stream with the Box–Muller step in mpmath; only the
    blocks that hold a row below n are formed."""
    import mpmath as mp
    nq = (-(-n // 64) + 3) // 4
    x = px.philox4x32(np.arange(r * nq * 64, dtype=np.uint32), c1, px.U_NOISE, c3, seed)
    u = [px._u32(v) for v in x]
    out = np.empty((n, r), dtype=object)
    for idx in range(r * nq * 64):
        l, q, lam = idx // (nq * 64), (idx // 64) % nq, idx % 64
        for half in (0, 1):
            rows = [lam + 64 * (4 * q + 2 * half + i) for i in (0, 1)]
            if rows[0] >= n:
                continue
            z = FC._bm(mp, u[2 * half][idx], u[2 * half + 1][idx])[1:]
            for row, v in zip(rows, z):
                if row < n:
                    out[row, l] = v
    return out


def _mp_forward(pb, w, U, I0):
    """temp (list over k of (r, B)), V (Q, B) with its factors multiplied in k order, fhat (B)."""
    D = pb.shape[1]
    temp = [U[:, :, k].T @ pb[:, k, :] for k in range(D)]
    V = None
    for k in range(D):
        f = temp[k][I0[:, k], :]
        V = f if V is None else V * f
    return temp, V, V.T @ w


def _mp_cores(pb, temp, V, res, w, I0, r):
    """V·res (Q) and Ψ_k·res as (n, r, D): the gradients before their scale factors."""
    import mpmath as mp
    n, D, B = pb.shape
    gU = np.empty((n, r, D), dtype=object)
    for k in range(D):
        Uphi = V / temp[k][I0[:, k], :]
        A = np.empty((r, B), dtype=object)
        A[:] = mp.mpf(0)
        for l in range(r):
            idx = np.nonzero(I0[:, k] == l)[0]
            if len(idx):
                A[l] = w[idx] @ Uphi[idx, :]
        gU[:, :, k] = pb[:, k, :] @ (A * res[None, :]).T
    return V @ res, gU


def _mp_proj(U, V):
    return V - (U @ (U.T @ V + V.T @ U)) / 2


def _mp_expm(X):
    E = EC.expm_mpf(X)
    out = np.empty(X.shape, dtype=object)
    for i in range(X.shape[0]):
        for j in range(X.shape[1]):
            out[i, j] = E[i, j]
    return out


def _mp_geod(U, mom, t):
    import mpmath as mp
    n, r = U.shape
    A = U.T @ mom
    T = np.empty((2 * r, 2 * r), dtype=object)
    T[:r, :r] = A
    T[:r, r:] = -(mom.T @ mom)
    T[r:, :r] = _mpa(np.eye(r))
    T[r:, r:] = A
    E = _mp_expm(T * t)
    tmpU = (np.hstack([U, mom]) @ E[:, :r]) @ _mp_expm(A * (-t))
    nrm = _fn("sqrt")((tmpU * tmpU).sum(axis=0))
    return tmpU / nrm[None, :]


def _norm(a):
    import mpmath as mp
    return mp.sqrt((a * a).sum())


def compute(c):
    """The three steps in mpmath: dict(w, U, norms) of object arrays laid out as run_numpy's."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _compute(c, mp)


def _compute(c, mp):
    p = inputs(c)
    n, D, r, Q, m, tail = c.shape
    N = p["N"]
    f = mp.mpf
    cls = c.family in CLS_FAMILIES
    lang, stf = dict(REG_FAMILIES, **CLS_FAMILIES).get(c.family, (True, True))
    phi, I0 = _mpa(p["phi"]), np.asarray(p["I"]) - 1
    y = _mpa(p["y"])
    w, U = _mpa(p["w0"]), _mpa(p["U0"])
    sv, epsw, epsU = f(p["signal_var"]), f(p["epsw"]), f(p["epsU"])
    sqw, sq = mp.sqrt(epsw), mp.sqrt(epsU)
    sqrt, exp = _fn("sqrt"), _fn("exp")
    if c.family == "rmsprop":
        alpha, lam = f(ALPHA), f(R.RMS_LAMBDA)
        gwa = _mpa(np.zeros(Q))
        gUa = _mpa(np.zeros((n, r, D)))
    order = np.arange(N)
    out = dict(w=[], U=[], norms=[])
    step = 0
    for epoch in range(2):
        order = order[px.randperm(N, RUN_SEED, epoch)]
        for batch in range(2):
            if step >= STEPS:
                break
            idx = order[m * batch: min(m * (batch + 1), N)]
            B = len(idx)
            pb, yb = phi[:, :, idx], y[idx]
            NB = f(N) / B
            if cls:
                yl = np.asarray(p["y"])[idx]
                fw = [_mp_forward(pb, w[:, k], U[..., k], I0) for k in range(NCLS)]
                fh = np.stack([t[2] for t in fw], axis=1)
                prob = exp(fh)
                prob = prob / prob.sum(axis=1)[:, None]
                gws, gUs, nr = [], [], []
                for k in range(NCLS):
                    res = _mpa((yl == k + 1).astype(np.float64)) - prob[:, k]
                    a, b = _mp_cores(pb, fw[k][0], fw[k][1], res, w[:, k], I0, r)
                    gws.append(a * NB - w[:, k])
                    gUs.append(b * NB)
                    nr.append([_norm(gws[k])] + [_norm(gUs[k][:, :, d]) for d in range(D)])
                for ps in range(2):
                    for k in range(NCLS):
                        w[:, k] = w[:, k] + gws[k] * (epsw / 2)
                        if ps == 0 or lang:
                            w[:, k] = w[:, k] + _mp_normals(Q, RUN_SEED, step, px.W_NOISE, 2 * k + ps) * sqw
                    for k in range(NCLS):
                        for d in range(D):
                            G = gUs[k][:, :, d]
                            noisy = ps == 0 or lang
                            xi = _mp_unoise(n, r, RUN_SEED, step, d + D * (2 * k + ps)) if noisy else None
                            if ps == 0 or stf:
                                drive = G * (sq / 2)
                                if noisy:
                                    drive = drive + xi
                                U[:, :, d, k] = _mp_geod(U[:, :, d, k], _mp_proj(U[:, :, d, k], drive), sq)
                            else:
                                upd = (G - U[:, :, d, k] * n) * (epsU / 2)
                                if noisy:
                                    upd = upd + xi * sq
                                U[:, :, d, k] = U[:, :, d, k] + upd
                out["norms"].append(nr)
            else:
                temp, V, fhat = _mp_forward(pb, w, U, I0)
                res = yb - fhat
                if c.family == "rmsprop":
                    gw = (V @ res) / (B * sv)
                    gwa = gwa * alpha + (gw * gw) * (1 - alpha)
                    ew = (sqrt(gwa) + lam) ** -1 * epsU
                    gradw = gw * N - w
                    w = w + ew * gradw / 2 + sqrt(ew) * _mp_normals(Q, RUN_SEED, step, px.W_NOISE, 0)
                    _, gU = _mp_cores(pb, temp, V, res, w, I0, r)              # the new w
                    gU = gU / (B * sv)
                    gUa = gUa * alpha + (gU * gU) * (1 - alpha)
                    eU = (sqrt(gUa) + lam) ** -1 * epsU
                    gradU = gU * N
                    for k in range(D):
                        sk = mp.sqrt(eU[:, :, k].sum() / (n * r))
                        mom = _mp_proj(U[:, :, k], gradU[:, :, k] * (sk / 2)
                                       + _mp_unoise(n, r, RUN_SEED, step, k))
                        U[:, :, k] = _mp_geod(U[:, :, k], mom, sk)
                else:
                    core_w, core_U = _mp_cores(pb, temp, V, res, w, I0, r)
                    gradw = core_w * (NB / sv) - w
                    gradU = core_U * (NB / sv)
                    w = w + gradw * (epsw / 2)
                    if lang:
                        w = w + _mp_normals(Q, RUN_SEED, step, px.W_NOISE, 0) * sqw
                    if c.family != "wonly":
                        for k in range(D):
                            xi = _mp_unoise(n, r, RUN_SEED, step, k) if lang else None
                            if stf:
                                drive = gradU[:, :, k] * (sq / 2)
                                mom = _mp_proj(U[:, :, k], drive + xi if lang else drive)
                                U[:, :, k] = _mp_geod(U[:, :, k], mom, sq)
                            else:
                                upd = (gradU[:, :, k] - U[:, :, k] * n) * (epsU / 2)
                                U[:, :, k] = U[:, :, k] + (upd + xi * sq if lang else upd)
                nr = [_norm(gradw)]
                if c.family != "wonly":
                    nr += [_norm(gradU[:, :, k]) for k in range(D)]
                out["norms"].append(nr)
            out["w"].append(w.copy())
            out["U"].append(U.copy())
            step += 1
    return dict(w=np.array(out["w"], dtype=object), U=np.array(out["U"], dtype=object),
                norms=np.array(out["norms"], dtype=object))


def pack(c, ref):
    """compute()'s result as the fixture's arrays: {suffix: array}."""
    steps, idx = u_select(c)
    out = {}
    out["w_hi"], out["w_lo"] = _dd(ref["w"])
    out["n_hi"], out["n_lo"] = _dd(ref["norms"])
    if c.family != "wonly":
        kept = np.array([ref["U"][s].ravel(order="F")[idx] for s in steps], dtype=object)
        out["U_hi"], out["U_lo"] = _dd(kept)
    return out


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def reference(c):
    """{w: (hi, lo), norms: (hi, lo), U: (hi, lo) at u_select's entries, sel} of a case from the
    committed file where the case's digest is there, else by mpmath.  Shared and read-only."""
    st, k = _stored(), key(c)
    if str(st.get(k + "_digest")) == digest(c):
        a = {s: st[k + "_" + s] for s in ("w_hi", "w_lo", "n_hi", "n_lo", "U_hi", "U_lo")
             if k + "_" + s in st}
    else:
        a = pack(c, compute(c))
    out = dict(w=(a["w_hi"], a["w_lo"].astype(np.float64)),
               norms=(a["n_hi"], a["n_lo"].astype(np.float64)), sel=u_select(c))
    if "U_hi" in a:
        out["U"] = (a["U_hi"], a["U_lo"].astype(np.float64))
    for v in out.values():
        for x in v:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return out


def bars():
    """{family: {quantity: B}} as the fixture stores them (measured by the maker on the two fp64
    restatements against mpmath, never on the device)."""
    st = _stored()
    return {fam: dict(zip(QUANTITIES, st["bar_" + fam])) for fam in FAMILIES}


def measured_u():
    st = _stored()
    return {fam: dict(zip(QUANTITIES, st["u_" + fam])) for fam in FAMILIES}
