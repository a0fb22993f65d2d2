"""fp64 numpy / LAPACK restatements of the function draws of gpt_amd/csrc/gpdraw.hip, the cases of
tests/golden/gpdraw_mp.npz (made by tests/gen_gpdraw_golden.py with mpmath at 50 digits) and the
error yardstick of the device parity tests.

    prior      F = L Z,            L L' = K + jitter I                      (GPrand)
    posterior  fmu = Ks' alpha,    alpha = (K + signal_var I)^-1 y,
               cov = K** - V'V,    V = L_A^-1 Ks,  L_A L_A' = K + signal_var I   (GPpost)
               F = fmu 1' + L Z,   L L' = cov + d I,  d = jitter (+ signal_var when observed)
    RFF theta  theta = l 1' + sqrt(signal_var) L^-T Z,  L L' = A = phi phi' + signal_var I,
               l = A^-1 phi y,  phi = sqrt(2/n) sigma_RBF cos((Zf / ls) X' + bf)

    K_ij = sigma_RBF^2 exp(-1/2 sum_k ((x_ik - x_jk)/l_k)^2),  h = [length_scale (D entries, or
    one); sigma_RBF; signal_var].
Test infrastructure only: nothing under gpt_amd/ imports this.
"""
import math
import os
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gpdraw_mp.npz")

# (N, D, Lh, Ntest): 33, 130 and 259 cross one, two and four 64-column panels with ragged ends,
# Ntest = 200 makes the posterior covariance's own Cholesky multi-panel
CASES = [(33, 2, 4, 33), (130, 4, 3, 64), (259, 8, 10, 100), (259, 2, 4, 200)]
RFF_N = [40, 100, 300, None]          # features of the RFF posterior of each case
S = 17                                # injected normals per case: crosses the 16-column tile
JITTER = 1e-6
COV_MAX_NT = 100                      # the golden stores cov up to this Ntest
LS = [1.4, 0.9, 2.0, 1.1]

Post = namedtuple("Post", "fmu F cov")


def case_name(case):
    return "N%d_D%d_Lh%d_T%d" % tuple(case)


def case_inputs(idx):
    """Seeded inputs of case idx: X, y, Xtest (its last five rows copies of training rows, the
    strongest cancellation in cov), h, the injected normals of the three draws and the RFF
    model's feature inputs."""
    N, D, Lh, Nt = CASES[idx]
    rng = np.random.default_rng(4100 + idx)
    X = rng.standard_normal((N, D))
    y = np.sin(X @ rng.standard_normal(D)) + 0.2 * rng.standard_normal(N)
    Xtest = rng.standard_normal((Nt, D))
    Xtest[-5:] = X[:5]
    nl = Lh - 2
    h = np.array([LS[k % 4] for k in range(nl)] + [1.3, 0.05])
    out = dict(X=X, y=y, Xtest=Xtest, h=h, Zprior=rng.standard_normal((N, S)),
               Zpost=rng.standard_normal((Nt, S)))
    n = RFF_N[idx]
    if n:
        out.update(Zf=rng.standard_normal((n, D)), bf=2 * math.pi * rng.random(n),
                   Ztheta=rng.standard_normal((n, S)))
    return out


def kern(Xa, Xb, h):
    ls = np.broadcast_to(h[:-2], (Xa.shape[1],)) if h.size == 3 else h[:-2]
    d = (Xa[:, None, :] - Xb[None, :, :]) / ls
    return h[-2] ** 2 * np.exp(-0.5 * (d * d).sum(axis=2))


def prior_factor(X, h, jitter):
    return np.linalg.cholesky(kern(X, X, h) + jitter * np.eye(X.shape[0]))


def prior(X, h, jitter, Z):
    return prior_factor(X, h, jitter) @ Z


def posterior_cov(X, y, h, Xtest):
    """(fmu, cov) of the function values at Xtest."""
    L = np.linalg.cholesky(kern(X, X, h) + h[-1] * np.eye(X.shape[0]))
    Ks = kern(X, Xtest, h)
    alpha = sla.cho_solve((L, True), y)
    V = sla.solve_triangular(L, Ks, lower=True)
    return Ks.T @ alpha, kern(Xtest, Xtest, h) - V.T @ V


def posterior(X, y, h, Xtest, jitter, observed, Z):
    fmu, cov = posterior_cov(X, y, h, Xtest)
    d = jitter + (h[-1] if observed else 0.0)
    Ls = np.linalg.cholesky(cov + d * np.eye(cov.shape[0]))
    return Post(fmu, fmu[:, None] + Ls @ Z, cov)


def features(X, h, Zf, bf):
    n, D = Zf.shape
    ls = np.broadcast_to(h[:-2], (D,)) if h.size == 3 else h[:-2]
    return math.sqrt(2.0 / n) * h[-2] * np.cos((Zf / ls) @ X.T + bf[:, None])


def rff_system(X, h, Zf, bf):
    """(phi, A = phi phi' + signal_var I)."""
    phi = features(X, h, Zf, bf)
    return phi, phi @ phi.T + h[-1] * np.eye(phi.shape[0])


def theta(X, y, h, Zf, bf, Z):
    """(l, theta) of the RFF posterior."""
    phi, A = rff_system(X, h, Zf, bf)
    L = np.linalg.cholesky(A)
    l = sla.cho_solve((L, True), phi @ y)
    return l, l[:, None] + math.sqrt(h[-1]) * sla.solve_triangular(L.T, Z, lower=False)


def load_golden():
    """{case name: dict of arrays}: the inputs of case_inputs and the mpmath Fprior, fmu, Fpost
    (function values, observed = 0), cov (Ntest <= 100), l and theta."""
    z = np.load(GOLDEN)
    out = {}
    for key in z.files:
        nm, field = key.split("/")
        out.setdefault(nm, {})[field] = z[key]
    return out


def errors(g, Fprior=None, fmu=None, Fpost=None, cov=None, l=None, th=None, cols=None):
    """Errors of results against the golden g in the units of the parity rule: prior F over
    max|F|, fmu over max|fmu|, posterior F over max|F - fmu|, cov over sigma_RBF^2, theta over
    max|theta - l|.  cols: the columns of the golden's S the results hold."""
    c = slice(None) if cols is None else cols
    e = {}
    if Fprior is not None:
        e["prior"] = np.abs(Fprior - g["Fprior"][:, c]).max() / np.abs(g["Fprior"][:, c]).max()
    if fmu is not None:
        e["fmu"] = np.abs(fmu - g["fmu"]).max() / np.abs(g["fmu"]).max()
    if Fpost is not None:
        dev = np.abs(g["Fpost"][:, c] - g["fmu"][:, None]).max()
        e["post"] = np.abs(Fpost - g["Fpost"][:, c]).max() / dev
    if cov is not None and "cov" in g:
        e["cov"] = np.abs(cov - g["cov"]).max() / g["h"][-2] ** 2
    if th is not None:
        dev = np.abs(g["theta"][:, c] - g["l"][:, None]).max()
        e["theta"] = np.abs(th - g["theta"][:, c]).max() / dev
    return e


def yardstick(g):
    """The errors of the restatements above against the golden g, all S columns."""
    post = posterior(g["X"], g["y"], g["h"], g["Xtest"], JITTER, False, g["Zpost"])
    kw = dict(Fprior=prior(g["X"], g["h"], JITTER, g["Zprior"]), fmu=post.fmu, Fpost=post.F,
              cov=post.cov)
    if "Ztheta" in g:
        kw["l"], kw["th"] = theta(g["X"], g["y"], g["h"], g["Zf"], g["bf"], g["Ztheta"])
    return errors(g, **kw)
