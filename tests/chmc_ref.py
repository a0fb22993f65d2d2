"""fp64 numpy restatement of Hamiltonian Monte Carlo on theta of the full-theta softmax classifier
(DESIGN §6i): the leapfrog integrator, the transition with its Metropolis test, a literal
transcription of the reference's MALA lines, and the cases of the device tests.

U(theta) = neglogjointlkhd(theta; h), the |theta|^2/2 prior included, and its gradient come from
cjoint_ref.value_and_grad_fused; H(theta, p) = U + |p|^2/2.  ``eps`` is the reference's squared
step, the leapfrog step is s = sqrt(eps), so L = 1 is BloodTransfusionExperiment.jl:261-265.

RNG contract of 0-based transition t: the momentum of class c is normals(n, seed, t, HMC_MOM, c),
the uniform of the test is uniform(seed, t, HMC_ACCEPT, 0).  Accept iff H1 is finite and
u < exp(H0 - H1); an overflowing exponent is +inf and accepts.

The decision margin |log u - (H0 - H1)| is a condition of every parity case: a device decision
can be compared with this one only where the margin is far from 0 (MARGIN_MIN).
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import math

import numpy as np

import cjoint_ref as CR
from oracle import philox as px

HMC_MOM, HMC_ACCEPT = 26, 27
MARGIN_MIN = 1e-6
SEED = 11
POINT = 1                      # the hyper point of every case

# (CASES index, L, eps): three transitions from the golden theta
PARITY = [(0, 1, 1e-2), (3, 3, 1e-2), (4, 5, 1e-2), (5, 2, 1e-2)]
# the configurations of the issue's CPU probe: 12 transitions each
PROBE = [(i, L, 1e-2) for i in (0, 3, 4) for L in (1, 5)]
BOTH = dict(idx=4, L=8, eps=0.09, scale=1.0, ntrans=12)          # 11 accepts and 1 reject
ALL_REJECTED = dict(idx=4, L=5, eps=0.04, scale=0.1, ntrans=12)  # every transition rejected
DIVERGENT = dict(idx=0, L=32, eps=1e8, ntrans=3)                 # H1 overflows (L = 16: 1e265 still)


def potential(X, y, Z, b, theta, h):
    """U and grad U (n, C)."""
    val, g, _ = CR.value_and_grad_fused(X, y, Z, b, theta, h)
    return val, g


def momentum(n, C, seed, t):
    p = np.empty((n, C))
    for c in range(C):
        p[:, c] = px.normals(n, seed, t, HMC_MOM, c)
    return p


def leapfrog(X, y, Z, b, theta, h, eps, L, p, U0=None, g0=None):
    """L leapfrog steps from (theta, p): q, p_new, H0, H1, U(q), grad U(q)."""
    s = math.sqrt(eps)
    if U0 is None:
        U0, g0 = potential(X, y, Z, b, theta, h)
    H0 = U0 + np.sum(p ** 2) / 2
    p = p - 0.5 * s * g0
    q = theta + s * p
    for _ in range(L - 1):
        _, g = potential(X, y, Z, b, q, h)
        p = p - s * g
        q = q + s * p
    U1, g = potential(X, y, Z, b, q, h)
    p = p - 0.5 * s * g
    H1 = U1 + np.sum(p ** 2) / 2
    return q, p, H0, H1, U1, g


def decide(u, H0, H1):
    if not math.isfinite(H1):
        return False
    d = H0 - H1
    return u < (math.exp(d) if d < 700.0 else math.inf)


def margin(u, H0, H1):
    """|log u - (H0 - H1)|; inf where H1 is not finite (the decision does not hang on rounding)."""
    if not math.isfinite(H1):
        return math.inf
    return abs(math.log(u) - (H0 - H1))


def hmc(X, y, Z, b, theta, h, eps, L, ntrans, seed, t0=0):
    """ntrans transitions from the 0-based counter t0.  Returns a dict: theta (the final state),
    store (n, C, ntrans: the state after every transition), accept, H0, dH = H0 - H1, value (U of
    the kept state), margin and divergent, one entry per transition."""
    theta = np.array(theta, dtype=np.float64, copy=True)
    n, C = theta.shape
    U, g = potential(X, y, Z, b, theta, h)
    out = dict(store=np.empty((n, C, ntrans)), accept=np.zeros(ntrans, dtype=np.int32),
               H0=np.empty(ntrans), dH=np.empty(ntrans), value=np.empty(ntrans),
               margin=np.empty(ntrans),
               divergent=np.zeros(ntrans, dtype=bool))
    for i in range(ntrans):
        t = t0 + i
        p = momentum(n, C, seed, t)
        with np.errstate(all="ignore"):
            q, _, H0, H1, U1, g1 = leapfrog(X, y, Z, b, theta, h, eps, L, p, U, g)
        u = px.uniform(seed, t, HMC_ACCEPT, 0)
        acc = decide(u, H0, H1)
        out["margin"][i] = margin(u, H0, H1)
        out["divergent"][i] = not math.isfinite(H1)
        out["H0"][i] = H0
        out["dH"][i] = H0 - H1
        if acc:
            theta, U, g = q, U1, g1
        out["accept"][i] = 1 if acc else 0
        out["value"][i] = U
        out["store"][:, :, i] = theta
    out["theta"] = theta
    return out


def mala_literal(X, y, Z, b, theta, h, eps, seed, t):
    """One iteration of BloodTransfusionExperiment.jl:260-268 on vec(theta), line by line, with
    the literal value and gradient of cjoint_ref; mom and rand() from the contract's streams.
    Returns theta (n, C), theta_prop (n, C), mom_prop (n*C), accept_prob and the decision."""
    n, C = theta.shape
    nC = n * C
    vec = lambda a: a.ravel(order="F")                         # noqa: E731
    mat = lambda v: v.reshape((n, C), order="F")               # noqa: E731
    value = lambda v: CR.neglogjoint_literal(X, y, Z, b, mat(v), h)                 # noqa: E731
    grad = lambda v: CR.gradneglogjoint_literal(X, y, Z, b, mat(v), h)[:nC]         # noqa: E731
    th = vec(theta)
    gradtheta = grad(th)
    mom = vec(momentum(n, C, seed, t))
    theta_prop = th - eps * gradtheta / 2 + math.sqrt(eps) * mom
    gradtheta_prop = grad(theta_prop)
    mom_prop = mom - math.sqrt(eps) * (gradtheta + gradtheta_prop) / 2
    accept_prob = math.exp(value(th) - value(theta_prop) + np.sum(mom ** 2) / 2
                           - np.sum(mom_prop ** 2) / 2)
    acc = px.uniform(seed, t, HMC_ACCEPT, 0) < accept_prob
    if acc:
        th = theta_prop
    return mat(th), mat(theta_prop), mom_prop, accept_prob, acc


_GOLDEN = {}
_RUNS = {}


def golden_case(idx):
    if not _GOLDEN:
        _GOLDEN.update(CR.load_golden())
    return _GOLDEN[CR.case_name(CR.CASES[idx])]


def run(idx, L, eps, ntrans, scale=1.0, seed=SEED, t0=0):
    """The restatement's run of a case from the golden inputs at hyper point POINT, computed once
    and shared (treat as read-only).  Returns (g, theta0, h, result of hmc)."""
    key = (idx, L, eps, ntrans, scale, seed, t0)
    g = golden_case(idx)
    theta0 = scale * g["theta"]
    h = g["H"][POINT]
    if key not in _RUNS:
        _RUNS[key] = hmc(g["X"], g["y"], g["Z"], g["b"], theta0, h, eps, L, ntrans, seed, t0)
    return g, theta0, h, _RUNS[key]
