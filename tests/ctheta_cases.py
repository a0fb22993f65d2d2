"""Cases, inputs, 50-digit references and CPU-side measurements of the full-theta softmax tests
(tests/test_gpu_ctheta.py on the device, tests/test_ctheta_cases.py on the CPU).

A  the joint evaluator (gpt_amd/csrc/cjoint.hip) past kCjMaxBlocks = 256 tiles, where a workgroup
   walks more than one tile (WALK): value, grad theta and the hyper-gradient at hyper point 1.
B  the three samplers on theta against mpmath at MP_DIGITS digits:
     cls       GPNT_SGLDclass, three steps on N = m + tail rows (a full batch, the ragged batch, the
               next epoch's first batch), two chains of different seeds and step sizes (CLS)
     langevin  SoftmaxJoint.langevin, steps from the golden theta (LANG)
     leapfrog  SoftmaxJoint.leapfrog on a given momentum, forward and back (LEAP)
     hmc       SoftmaxJoint.hmc, transitions with their Metropolis tests (HMC)

Every reference takes the doubles the device is given (the inputs, the initial theta and the
oracle's normals and uniforms: gpnt_ref.three_steps_mp's convention) and does everything else at
MP_DIGITS digits; nothing is rounded to double between the evaluations of a trajectory
(cjoint_ref.mp_core).  The back leapfrog starts from the doubles nearest the forward reference
(its hi parts: q and -p_new), so its reference is again the true image of given doubles.

An entry is a tuple (kind, ...) of ENTRIES; key() names its arrays in tests/golden/ctheta_mp.npz.
References are stored as hi (float64) + lo (float32); a state of more than KEEP entries (KEEP_WALK
for A) is kept at every S-th entry in column-major order, S the smallest stride coprime to n that
leaves at most KEEP of them (oracle.step_cases.u_select's rule: every row and every class column is
reached).  Inputs are regenerated from their seeds and identified by a SHA-256 digest.

Error measures: theta, q, p as max|err| / max|ref| per stored step; H0, H1, value and dH as
|err| / max(|H0|, 1).  Bars: B = MARGIN·u per family (family()) and quantity, u the largest error of the
fp64 restatements (vectorised and literal for the class sampler; value_and_grad_fused and the
literal form for the joint) against the reference over the family's entries, measured by
tests/golden/make_ctheta_golden.py and stored.

Step sizes.  The rule is a step-1 share sqrt(eps)·rms(grad)/2 (the gradient's part of the move over
the noise's) of 0.5 to 2 as long as the conditioning limit COND_MAX holds (every input double moved
to a neighbour moves no stored output by more than COND_MAX·max|x|).  LANG takes
eps = round3(min(LANG_EPS_MAX, (2 / rms grad)^2)): share 1, or 0.5 to 0.7 where the cap of 1 binds.
The class sampler's gradient is mostly +theta itself (rms about 1); its two chains take
eps = CLS_EPS = 1 and 1.5 (shares 0.5 to 0.75).  Both pass the conditioning test with room (worst
move 1e-15); the shares are recorded in the fixture.  HMC keeps chmc_ref's eps = 1e-2 and L.

Nothing here comes from the device.  Test infrastructure: numpy / mpmath, no GPU.
"""
import functools
import hashlib
import math
import os

import numpy as np

import chmc_ref as H
import cjoint_ref as CR
import cls_ref as CLS
from oracle import philox as px

MP_DIGITS = CR.MP_DIGITS
MARGIN = 8               # device bar B = MARGIN·u (tests/test_gpu_step.py explains the factor)
B_MAX = 1e-13
COND_MAX = 1e-14
KEEP, KEEP_WALK = 192, 1500
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctheta_mp.npz")
POINT = H.POINT
SEED = H.SEED
NT = 512                 # kNT: threads of a workgroup, entries of theta per workgroup of chmc.hip

# ------------------------------------------------------------------------------------ A: the walk
# (n, N, D, C, form): what the issue's table says each reaches; TI and tiles are asserted from
# cjoint_ref.cjoint_layout by tests/test_ctheta_cases.py.
WALK = [
    (33, 8230, 2, 3, "ard"),        # TI 32, 258 tiles: workgroups 0 and 1 walk two, the last has 6 columns
    (33, 16485, 2, 3, "ard"),       # 516 tiles: three for workgroups 0-3, two for the rest
    (700, 2053, 1, 2, "scalar"),    # TI 8, 257 tiles, last tile 5 columns
    (330, 4100, 4, 32, "ard"),      # TI 16, 257 tiles, theta read through L2
]
WALK_TABLE = [(32, 258), (32, 516), (8, 257), (16, 257)]          # (TI, tiles) of the issue
WALK_MP = (0, 1, 2)      # mpmath (12 s, 24 s, 55 s); the last in long double (mpmath: about 160 s)
EDGE = {"e512": (64, 8), "e513": (171, 3)}                        # n, C with n·C on a workgroup edge

# ----------------------------------------------------------------------------------- B1: cls cases
# (n, m, C, tail, decay, sigma_theta)
CLS_CASES = [
    (70, 25, 3, 3, 0.1, 1.0),       # batch staged in LDS; n not a multiple of 64
    (330, 64, 2, 6, 0.0, 1.0),      # batch re-read, not staged
    (33, 7, 16, 2, 0.0, 1.0),       # n < 64, fewer batch columns than waves
    (64, 96, 2, 3, 0.0, 0.7),       # more than 64 columns in a batch
    (40, 10, 20, 1, 0.0, 1.0),      # CC = 32, a one-column batch
]
CLS_STAGE = [True, False, True, True, True]
CLS_EPS = 1.0
CLS_CHAINS = ((5, 1.0), (2 ** 40 + 9, 1.5))        # (seed, factor on CLS_EPS) of the two chains
STEPS = 3
LANG_EPS_MAX = 1.0

LANG = [("g0", 0, 3), ("g1", 0, 3), ("g3", 0, 3), ("g4", 0, 3), ("g0", 5, 3), ("w0", 0, 1)]
LEAP = ([(g, L) for g in ("g0", "g1", "g3") for L in (1, 2, 5)]
        + [("g4", 3), ("e512", 2), ("e513", 2), ("w0", 2)])
HMC_EPS = 1e-2
# (problem, L, eps, transitions, scale of theta0)
HMC = [("g0", 1, 1e-2, 3, 1.0), ("g3", 3, 1e-2, 3, 1.0), ("g4", 5, 1e-2, 3, 1.0),
       ("g%d" % H.BOTH["idx"], H.BOTH["L"], H.BOTH["eps"], H.BOTH["ntrans"], H.BOTH["scale"])]

ENTRIES = ([("walk", k) for k in range(len(WALK))] + [("cls", k) for k in range(len(CLS_CASES))]
           + [("lang",) + a for a in LANG] + [("leap",) + a for a in LEAP]
           + [("hmc",) + a for a in HMC])
FAMILIES = {"cls": ("theta",), "lang": ("theta",), "leap": ("q", "p", "H", "dH"),
            "hmc": ("theta", "value", "dH"), "wlang": ("theta",), "wleap": ("q", "p", "H", "dH")}


def family(e):
    """The family whose bars hold an entry: its kind, and for the Langevin step and the leapfrog on
    the tile walk (N = 8230) a family of their own.  There the gradient is large against theta and p,
    so the measures max|err| / max|ref| of the restatements are larger than on the golden cases,
    and the golden cases' bars should not widen with them.  The walk families' u is the fused
    form's alone: the literal form adds its 8230 terms per class one after another and reaches
    1.9e-13 on p, which would put 8·u past B_MAX; its figure is recorded (key_meas), not used."""
    return "w" + e[0] if e[0] in ("lang", "leap") and e[1][0] == "w" else e[0]


def key(e):
    return "_".join(("%g" % v).replace("-", "m") if isinstance(v, float) else str(v) for v in e)


# ---------------------------------------------------------------------------------------- inputs
class Problem:
    """X, y, Z, b, theta (n, C), h of one joint problem; read-only."""

    def __init__(self, X, y, Z, b, theta, h):
        self.X, self.y, self.Z, self.b, self.theta, self.h = X, y, Z, b, theta, np.asarray(h)
        for a in (X, y, Z, b, theta, self.h):
            a.setflags(write=False)
        self.n, self.C = theta.shape

    def args(self, theta=None):
        return self.X, self.y, self.Z, self.b, self.theta if theta is None else theta, self.h

    def joint(self, G):
        return G.SoftmaxJoint(self.X, self.y, self.Z, self.b, C=self.C)


@functools.lru_cache(maxsize=None)
def problem(name):
    """g<i>: cjoint_ref.CASES[i] from the golden file; w<k>: WALK[k]; e512 / e513: N = 40, D = 2 with
    n·C on a workgroup edge of chmc.hip.  All at hyper point POINT, theta of case_inputs' kind."""
    if name[0] == "g":
        g = H.golden_case(int(name[1:]))
        return Problem(g["X"].copy(), g["y"].copy(), g["Z"].copy(), g["b"].copy(), g["theta"].copy(),
                       g["H"][POINT].copy())
    if name[0] == "w":
        case, idx = WALK[int(name[1:])] + ("",), 100 + int(name[1:])
    else:
        n, C = EDGE[name]
        case, idx = (n, 40, 2, C, "ard", ""), 200 + n
    return Problem(*CR.case_inputs(case, idx), CR.hyper_points(case)[POINT])


@functools.lru_cache(maxsize=None)
def cls_inputs(k):
    """phi (n, N = m + tail) and labels of CLS_CASES[k] (cls_ref.sampler_inputs; with N < C the
    classes past N are absent and C is passed explicitly)."""
    n, m, C, tail, _, _ = CLS_CASES[k]
    phi, y, _ = CLS.sampler_inputs((n, m + tail, C), 10 + k)
    phi.setflags(write=False)
    y.setflags(write=False)
    return phi, y


def _round3(x):
    return float("%.3g" % x)


@functools.lru_cache(maxsize=None)
def lang_eps(name):
    """(eps, share at the first step) of a Langevin entry's problem (module docstring)."""
    P = problem(name)
    rms = math.sqrt(np.mean(np.square(CR.gradtheta_fused(*P.args()))))
    eps = _round3(min(LANG_EPS_MAX, (2 / rms) ** 2))
    return eps, math.sqrt(eps) * rms / 2


def cls_share(k, chain):
    """sqrt(eps)·rms(grad)/2 at step 1 of a chain of CLS_CASES[k]."""
    return math.sqrt(CLS_EPS * CLS_CHAINS[chain][1]) * cls_run(k, chain, grad_rms=True) / 2


def leap_momentum(name, L):
    P = problem(name)
    return H.momentum(P.n, P.C, 3, L)


def digest(e):
    h = hashlib.sha256(key(e).encode())
    arrays = []
    if e[0] == "cls":
        arrays = list(cls_inputs(e[1])) + [np.array(CLS_CASES[e[1]], dtype=np.float64),
                                           np.array([CLS_EPS] + [v for c in CLS_CHAINS for v in c],
                                                    dtype=np.float64)]
    else:
        P = problem("w%d" % e[1] if e[0] == "walk" else e[1])
        arrays = [P.X, P.y, P.Z, P.b, P.theta, P.h]
        if e[0] == "lang":
            arrays.append(np.array([lang_eps(e[1])[0]]))
        if e[0] == "leap":
            arrays.append(leap_momentum(e[1], e[2]))
    for a in arrays:
        a = np.asfortranarray(a)
        h.update(str(a.dtype).encode() + a.tobytes(order="F"))
    return h.hexdigest()


def select(n, size, keep=KEEP):
    """Flat column-major indices of the kept entries of an (n, ...) state of `size` entries."""
    if size <= keep:
        return np.arange(size)
    S = -(-size // keep)
    while math.gcd(S, n) != 1:
        S += 1
    return np.arange(0, size, S)


def flat(a):
    return np.asarray(a).ravel(order="F")


# --------------------------------------------------------------------------- device layouts restated
def ntc_layout(n, C, m):
    """gpt_amd/csrc/cls.hip's ntc_layout: dict(CC, stage, bytes)."""
    al = CR._al16
    CC = 2 if C <= 2 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32
    o = al(8 * n * CC)
    o = al(o + 4 * m)
    o = al(o + 4 * m)
    o = al(o + 8 * C * m)
    o = al(o + 4 * CR.NW)
    staged = al(o + 8 * n * m)
    stage = staged <= 160 * 1024
    return dict(CC=CC, stage=stage, bytes=staged if stage else o)


def hmc_blocks(n, C):
    """gpt_amd/csrc/chmc.hip's hmc_blocks."""
    return (n * C + NT - 1) // NT


# ------------------------------------------------------------------- the fp64 restatements (hooked)
# `mut` names one defect of tests/test_ctheta_cases.py's list; None is the restatement itself, which
# that test holds bit for bit to cls_ref.gpnt_sgld_class, chmc_ref.leapfrog and chmc_ref.hmc.
MUT_SIZE = {"softmax": 1e-9, "residual": 1e-9, "ragged": 1e-9, "plustheta": 1e-9, "sqrteps": 1e-9,
            "lasthalf": 1e-10, "gradcol": 1e-10, "kin": None, "prior": 1e-12}
CLS_MUTANTS = ("softmax", "residual", "ragged", "plustheta", "sqrteps")
HMC_MUTANTS = ("lasthalf", "gradcol", "kin", "prior")


def cls_run(k, chain, mut=None, literal=False, phi=None, grad_rms=False, size=None):
    """theta after each of STEPS steps (STEPS, n, C) of a chain of CLS_CASES[k]."""
    n, m, C, tail, decay, sigma = CLS_CASES[k]
    seed, fac = CLS_CHAINS[chain]
    eps_theta = CLS_EPS * fac
    p0, y = cls_inputs(k)
    phi = p0 if phi is None else phi
    if literal:
        st = CLS.gpnt_sgld_class_literal(phi, y, sigma, m, eps_theta, decay, 0, 2, seed, ncls=C)
        return np.moveaxis(st, -1, 0)[:STEPS].copy()
    d = (MUT_SIZE[mut] if size is None else size) if mut else 0.0
    N = m + tail
    yi = y.astype(np.int64)
    theta = np.empty((n, C))
    for c in range(C):
        theta[:, c] = sigma * px.normals(n, seed, 0, px.THETA_INIT, c)
    order = np.arange(N)
    out = []
    t = 0
    for epoch in (1, 2):
        order = order[px.randperm(N, seed, epoch - 1)]
        for batch in (1, 2):
            t += 1
            idx = order[m * (batch - 1): min(m * batch, N)]
            pb = phi[:, idx]
            B = len(idx)
            eps = eps_theta * float(t) ** (-decay)
            x = theta.T @ pb
            a = x.max(axis=0)
            lse = a + np.log(np.exp(x - a).sum(axis=0))
            P = np.exp(x - lse)
            if mut == "softmax":
                P = P * (1 + d)
            P[yi[idx] - 1, np.arange(B)] -= 1.0
            if mut == "residual":
                P[:, 0] *= 1 + d
            cN = N / B
            if mut == "ragged" and B < m:
                cN *= 1 + d
            gradtheta = cN * (pb @ P.T) + (theta * (1 + d) if mut == "plustheta" else theta)
            if grad_rms:
                return math.sqrt(np.mean(np.square(gradtheta)))
            noise = np.empty((n, C))
            for c in range(C):
                noise[:, c] = px.normals(n, seed, t - 1, px.THETA_NOISE, c)
            sq = math.sqrt(eps)
            if mut == "sqrteps" and decay != 0.0 and t > 1:
                sq *= 1 + d
            theta = theta - (eps * gradtheta / 2 + sq * noise)
            out.append(theta)
    return np.array(out[:STEPS])


def pot_fused(P, theta, mut=None):
    val, g, _ = CR.value_and_grad_fused(*P.args(theta))
    return _pot_mut(val, g, theta, mut)


def pot_literal(P, theta, mut=None):
    return _pot_mut(CR.neglogjoint_literal(*P.args(theta)), CR.gradtheta_literal(*P.args(theta)),
                    theta, mut)


def _pot_mut(val, g, theta, mut):
    if mut == "gradcol":
        g = g.copy()
        g[:, 0] *= 1 + MUT_SIZE[mut]
    if mut == "prior":
        val = val + MUT_SIZE[mut] * (np.sum(theta ** 2) / 2)
    return val, g


def _kin(p, mut):
    if mut == "kin":
        p = np.delete(p.ravel(), np.argmin(np.abs(p)))
    return np.sum(p ** 2) / 2


def leapfrog(P, theta, eps, L, p, pot=pot_fused, mut=None, U0=None, g0=None):
    """chmc_ref.leapfrog with the potential and the defects hooked: q, p_new, H0, H1, U1, g1."""
    s = math.sqrt(eps)
    if U0 is None:
        U0, g0 = pot(P, theta, mut)
    H0 = U0 + _kin(p, mut)
    p = p - 0.5 * s * g0
    q = theta + s * p
    for _ in range(L - 1):
        _, g = pot(P, q, mut)
        p = p - s * g
        q = q + s * p
    U1, g = pot(P, q, mut)
    half = 0.5 * s
    if mut == "lasthalf":
        half *= 1 + MUT_SIZE[mut]
    p = p - half * g
    H1 = U1 + _kin(p, mut)
    return q, p, H0, H1, U1, g


def hmc_run(P, theta0, eps, L, ntrans, seed=SEED, pot=pot_fused, mut=None):
    """chmc_ref.hmc on the hooked leapfrog: dict(store (ntrans, n, C), accept, H0, dH, value)."""
    theta = np.array(theta0, dtype=np.float64, copy=True)
    U, g = pot(P, theta, mut)
    out = dict(store=[], accept=[], H0=[], dH=[], value=[])
    for t in range(ntrans):
        p = H.momentum(P.n, P.C, seed, t)
        q, _, H0, H1, U1, g1 = leapfrog(P, theta, eps, L, p, pot, mut, U, g)
        acc = H.decide(px.uniform(seed, t, H.HMC_ACCEPT, 0), H0, H1)
        if acc:
            theta, U, g = q, U1, g1
        for k, v in zip(("store", "accept", "H0", "dH", "value"), (theta, int(acc), H0, H0 - H1, U)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def perturb(a, rng):
    """Every double moved to a neighbouring double, the side drawn per entry."""
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def perturbed_problem(P, seed):
    rng = np.random.default_rng((977, seed))
    return Problem(perturb(P.X, rng), P.y.copy(), perturb(P.Z, rng), perturb(P.b, rng),
                   perturb(P.theta, rng), P.h.copy())


def run_numpy(e, pot=pot_fused, mut=None, perturb_seed=None, literal=False, size=None):
    """The restatement's outputs of an entry, laid out as reference() and the device runs are:
    {name: array}, states as (steps, n·C column-major)."""
    rng = None if perturb_seed is None else np.random.default_rng((978, perturb_seed))
    if e[0] == "cls":
        phi = None if rng is None else np.asfortranarray(perturb(cls_inputs(e[1])[0], rng))
        return {"theta%d" % c: np.array([flat(s) for s in cls_run(e[1], c, mut, literal, phi, size=size)])
                for c in range(len(CLS_CHAINS))}
    P = problem("w%d" % e[1] if e[0] == "walk" else e[1])
    if perturb_seed is not None:
        P = perturbed_problem(P, perturb_seed)
    if e[0] == "lang":
        _, name, t0, nsteps = e
        eps = lang_eps(name)[0]
        gt = (lambda X, y, Z, b, th, h: pot(P, th)[1])
        th, out = P.theta, []
        for t in range(t0, t0 + nsteps):
            th = CR.langevin(*P.args(th), eps, 1, SEED, t, gradtheta=gt)
            out.append(flat(th))
        return dict(theta=np.array(out))
    if e[0] == "leap":
        _, name, L = e
        p0 = leap_momentum(name, L)
        if rng is not None:
            p0 = perturb(p0, rng)
        q, p1, H0, H1, _, _ = leapfrog(P, P.theta, HMC_EPS, L, p0, pot, mut)
        out = dict(q=flat(q)[None], p=flat(p1)[None], H=np.array([H0, H1]), dH=np.array([H0 - H1]))
        if rng is None:
            qs, ps = back_start(e)
            q, p1, H0, H1, _, _ = leapfrog(P, qs, HMC_EPS, L, ps, pot, mut)
            out.update(bq=flat(q)[None], bp=flat(p1)[None], bH=np.array([H0, H1]),
                       bdH=np.array([H0 - H1]))
        return out
    if e[0] == "hmc":
        _, name, L, eps, ntrans, scale = e
        r = hmc_run(P, scale * P.theta, eps, L, ntrans, SEED, pot, mut)
        return dict(theta=np.array([flat(s) for s in r["store"]]), value=r["value"], dH=r["dH"],
                    accept=r["accept"], H0=r["H0"])
    raise KeyError(e)


# ------------------------------------------------------------------------------ mpmath references
def _mpf(v):
    import mpmath as mp
    return mp.mpf(float(v))


def _cols(th):
    """th[j][c] -> the column-major flat list."""
    return [th[j][c] for c in range(len(th[0])) for j in range(len(th))]


def _mp_cls(k, chain):
    import mpmath as mp
    n, m, C, tail, decay, sigma = CLS_CASES[k]
    seed, fac = CLS_CHAINS[chain]
    phi, y = cls_inputs(k)
    N = m + tail
    yi = y.astype(np.int64) - 1
    col = [[_mpf(v) for v in phi[:, i]] for i in range(N)]
    th = [[_mpf(sigma * px.normals(n, seed, 0, px.THETA_INIT, c)[j]) for j in range(n)]
          for c in range(C)]                                                     # th[c][j]
    eps_theta = _mpf(CLS_EPS * fac)
    order = np.arange(N)
    out, t = [], 0
    for epoch in (1, 2):
        order = order[px.randperm(N, seed, epoch - 1)]
        for batch in (1, 2):
            t += 1
            idx = order[m * (batch - 1): min(m * batch, N)]
            B = len(idx)
            eps = eps_theta * mp.mpf(t) ** (-_mpf(decay))
            sq = mp.sqrt(eps)
            Pm = [[None] * B for _ in range(C)]
            for bi, i in enumerate(idx):
                x = [mp.fdot(th[c], col[i]) for c in range(C)]
                a = max(x)
                lse = a + mp.log(mp.fsum(mp.exp(v - a) for v in x))
                for c in range(C):
                    Pm[c][bi] = mp.exp(x[c] - lse) - (1 if c == yi[i] else 0)
            cN = mp.mpf(N) / B
            new = []
            for c in range(C):
                xi = px.normals(n, seed, t - 1, px.THETA_NOISE, c)
                row = []
                for j in range(n):
                    g = cN * mp.fdot([col[i][j] for i in idx], Pm[c]) + th[c][j]
                    row.append(th[c][j] - (eps * g / 2 + sq * _mpf(xi[j])))
                new.append(row)
            th = new
            out.append([v for row in th for v in row])
    return out[:STEPS]


def _mp_leapfrog(F, y, th, eps, L, p, U0=None, g0=None):
    """The leapfrog on mpf theta th[j][c] and momentum p[j][c]."""
    import mpmath as mp
    n, C = len(th), len(th[0])
    s = mp.sqrt(_mpf(eps))
    kin = lambda pp: mp.fsum(v * v for row in pp for v in row) / 2            # noqa: E731
    if U0 is None:
        U0, g0, _ = CR.mp_core(F, y, th, want_h=False)
    H0 = U0 + kin(p)
    p = [[p[j][c] - s * g0[j][c] / 2 for c in range(C)] for j in range(n)]
    q = [[th[j][c] + s * p[j][c] for c in range(C)] for j in range(n)]
    for _ in range(L - 1):
        _, g, _ = CR.mp_core(F, y, q, want_h=False)
        p = [[p[j][c] - s * g[j][c] for c in range(C)] for j in range(n)]
        q = [[q[j][c] + s * p[j][c] for c in range(C)] for j in range(n)]
    U1, g, _ = CR.mp_core(F, y, q, want_h=False)
    p = [[p[j][c] - s * g[j][c] / 2 for c in range(C)] for j in range(n)]
    return q, p, H0, U1 + kin(p), U1, g


def _hi(vals):
    return np.array([float(v) for v in vals])


def compute(e):
    """The entry's reference: {name: nested lists of mpf} laid out as run_numpy's result, plus plain
    arrays under 'accept', 'margin', 'H0' (hmc).  Walk entries past WALK_MP are long double."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        return _compute(e, mp)


def _compute(e, mp):
    if e[0] == "cls":
        return {"theta%d" % c: _mp_cls(e[1], c) for c in range(len(CLS_CHAINS))}
    P = problem("w%d" % e[1] if e[0] == "walk" else e[1])
    if e[0] == "walk":
        if e[1] in WALK_MP:
            val, gt, gh = CR.mp_core(CR.mp_features(P.X, P.Z, P.b, P.h), P.y, CR.mp_theta(P.theta))
            return dict(val=[val], gtheta=[_cols(gt)], gh=gh)
        val, gt, gh = CR.ld_value_grad(*P.args())
        ld = lambda v: mp.mpf(float(v)) + mp.mpf(float(v - np.longdouble(float(v))))   # noqa: E731
        return dict(val=[ld(val)], gtheta=[[ld(v) for v in flat(gt)]], gh=[ld(v) for v in gh])
    F = CR.mp_features(P.X, P.Z, P.b, P.h, want_S=False)
    if e[0] == "lang":
        _, name, t0, nsteps = e
        eps = _mpf(lang_eps(name)[0])
        sq = mp.sqrt(eps)
        th, out = CR.mp_theta(P.theta), []
        for t in range(t0, t0 + nsteps):
            _, g, _ = CR.mp_core(F, P.y, th, want_h=False)
            xi = [px.normals(P.n, SEED, t, px.THETA_NOISE, c) for c in range(P.C)]
            th = [[th[j][c] - (eps * g[j][c] / 2 + sq * _mpf(xi[c][j])) for c in range(P.C)]
                  for j in range(P.n)]
            out.append(_cols(th))
        return dict(theta=out)
    if e[0] == "leap":
        _, name, L = e
        q, p1, H0, H1, _, _ = _mp_leapfrog(F, P.y, CR.mp_theta(P.theta), HMC_EPS, L,
                                           CR.mp_theta(leap_momentum(name, L)))
        out = dict(q=[_cols(q)], p=[_cols(p1)], H=[H0, H1], dH=[H0 - H1])
        qs = _hi(_cols(q)).reshape((P.n, P.C), order="F")
        ps = -_hi(_cols(p1)).reshape((P.n, P.C), order="F")
        q, p1, H0, H1, _, _ = _mp_leapfrog(F, P.y, CR.mp_theta(qs), HMC_EPS, L, CR.mp_theta(ps))
        out.update(bq=[_cols(q)], bp=[_cols(p1)], bH=[H0, H1], bdH=[H0 - H1],
                   start=np.array([flat(qs), flat(ps)]))
        return out
    if e[0] == "hmc":
        _, name, L, eps, ntrans, scale = e
        th = CR.mp_theta(scale * P.theta)
        U, g, _ = CR.mp_core(F, P.y, th, want_h=False)
        out = dict(theta=[], value=[], dH=[], accept=[], margin=[], H0=[])
        for t in range(ntrans):
            p = CR.mp_theta(H.momentum(P.n, P.C, SEED, t))
            q, _, H0, H1, U1, g1 = _mp_leapfrog(F, P.y, th, eps, L, p, U, g)
            lu = mp.log(_mpf(px.uniform(SEED, t, H.HMC_ACCEPT, 0)))
            acc = lu < H0 - H1
            if acc:
                th, U, g = q, U1, g1
            out["theta"].append(_cols(th))
            out["value"].append(U)
            out["dH"].append(H0 - H1)
            out["accept"].append(int(acc))
            out["margin"].append(float(abs(lu - (H0 - H1))))
            out["H0"].append(float(H0))
        return out
    raise KeyError(e)


PLAIN = ("accept", "margin", "H0", "start")
STATES = ("theta", "theta0", "theta1", "q", "p", "bq", "bp", "gtheta")


def entry_select(e, name):
    """The kept flat indices of state `name` of an entry (None: not a state, kept whole)."""
    if name not in STATES:
        return None
    if e[0] == "cls":
        n, _, C = CLS_CASES[e[1]][:3]
        return select(n, n * C)
    P = problem("w%d" % e[1] if e[0] == "walk" else e[1])
    return select(P.n, P.n * P.C, KEEP_WALK if e[0] == "walk" else KEEP)


def _dd(rows):
    import mpmath as mp
    hi = np.array([[float(v) for v in r] for r in rows])
    lo = np.array([[float(v - mp.mpf(float(v))) for v in r] for r in rows], dtype=np.float32)
    return hi, lo


def pack(e, ref):
    """compute()'s result as the fixture's arrays {suffix: array}."""
    import mpmath as mp
    out = {}
    with mp.workdps(MP_DIGITS):
        for name, v in ref.items():
            if name in PLAIN:
                out[name] = np.asarray(v)
                continue
            sel = entry_select(e, name)
            rows = [[r[i] for i in sel] for r in v] if sel is not None else [v]
            hi, lo = _dd(rows)
            if sel is None:
                hi, lo = hi[0], lo[0]
            out[name + "_hi"], out[name + "_lo"] = hi, lo
    return out


def back_start(e):
    """(q, -p_new) of a leapfrog entry as the doubles nearest the forward reference: the start of
    the back leapfrog, (n, C) each.  Needs every entry of q and p, so entries past KEEP store them
    whole under 'start'."""
    r = reference(e)
    P = problem(e[1])
    return (r["start"][0].reshape((P.n, P.C), order="F"), r["start"][1].reshape((P.n, P.C), order="F"))


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def reference(e):
    """{name: (hi, lo)} and plain arrays of an entry from the committed file (the digest has to be
    this machine's), 'sel' {state: indices}.  Shared and read-only."""
    st, k = _stored(), key(e) + "_"
    if str(st.get(k + "digest")) != digest(e):
        raise AssertionError("tests/golden/ctheta_mp.npz does not belong to these inputs: %s" % key(e))
    out = {}
    for name in st:
        if not name.startswith(k) or name == k + "digest":
            continue
        s = name[len(k):]
        if s.endswith("_hi"):
            out[s[:-3]] = (st[name], st[k + s[:-3] + "_lo"].astype(np.float64))
        elif not s.endswith("_lo"):
            out[s] = st[name]
    out["sel"] = {s: entry_select(e, s) for s in out if s in STATES}
    return out


def errors(e, run, ref):
    """{quantity: worst error} of a run (run_numpy's layout) against reference()'s dict, in the
    measures of the module docstring.  Back-leapfrog outputs count under q, p, H, dH."""
    res = {}

    def put(q, v):
        res[q] = max(res.get(q, 0.0), float(v))

    def state(q, name):
        hi, lo = ref[name]
        got = run[name][:, ref["sel"][name]]
        for s in range(hi.shape[0]):
            put(q, np.abs((got[s] - hi[s]) - lo[s]).max() / np.abs(hi[s]).max())

    def scalar(q, name, scale):
        hi, lo = ref[name]
        put(q, (np.abs((run[name] - hi) - lo) / scale).max())

    if e[0] == "cls":
        for c in range(len(CLS_CHAINS)):
            state("theta", "theta%d" % c)
    elif e[0] == "lang":
        state("theta", "theta")
    elif e[0] == "leap":
        for pre in ("", "b"):
            if pre + "q" not in run:
                continue
            scale = max(abs(ref[pre + "H"][0][0]), 1.0)
            state("q", pre + "q")
            state("p", pre + "p")
            scalar("H", pre + "H", scale)
            scalar("dH", pre + "dH", scale)
    elif e[0] == "hmc":
        scale = np.maximum(np.abs(ref["H0"]), 1.0)
        state("theta", "theta")
        scalar("value", "value", scale)
        scalar("dH", "dH", scale)
    return res


def moves(e, a, b):
    """errors() of run b against run a (both run_numpy's layout, every entry): the conditioning
    test's and the mutants' 'present comparison' measure."""
    ref = {k: (v, np.zeros_like(v)) for k, v in a.items() if k not in PLAIN}
    ref["sel"] = {k: slice(None) for k in a if k in STATES}
    if "H0" in a:
        ref["H0"] = a["H0"]
    return errors(e, b, ref)


def bars():
    """{family: {quantity: B}} as the fixture stores them."""
    st = _stored()
    return {f: dict(zip(q, st["bar_" + f])) for f, q in FAMILIES.items()}


def measured_u():
    st = _stored()
    return {f: dict(zip(q, st["u_" + f])) for f, q in FAMILIES.items()}


def walk_errors(P, val, gtheta, gh, ref):
    """(value relative, hyper per component, grad theta) of an evaluation of a walk entry in
    tests/test_gpu_cjoint.py's measures against reference()'s dict."""
    ev = abs((val - ref["val"][0][0]) - ref["val"][1][0]) / abs(ref["val"][0][0])
    hi, lo = ref["gh"]
    eh = np.abs((np.asarray(gh) - hi) - lo) / np.abs(hi)
    hi, lo = ref["gtheta"]
    got = flat(gtheta)[ref["sel"]["gtheta"]]
    et = float(np.abs((got - hi[0]) - lo[0]).max() / np.abs(hi[0]).max())
    return ev, eh, et


@functools.lru_cache(maxsize=None)
def walk_yardstick(k):
    """(per hyper-gradient component, grad theta): the larger error of the literal and the fused
    fp64 restatements against the reference (cjoint_ref.yardstick's rule; n·N·D doubles of the
    literal form stay under 1 GB in every WALK case, so it is never skipped)."""
    P = problem("w%d" % k)
    ref = reference(("walk", k))
    nC = P.n * P.C
    assert 8 * P.n * P.X.size <= 1 << 30
    lit = CR.gradneglogjoint_literal(*P.args())
    fv, ft, fh = CR.value_and_grad_fused(*P.args())
    _, eh1, et1 = walk_errors(P, fv, lit[:nC], lit[nC:], ref)
    _, eh2, et2 = walk_errors(P, fv, ft, fh, ref)
    return np.maximum(eh1, eh2), max(et1, et2)
