"""Python mirror of the reference's ``GPT_SGLD`` / ``GPT_SGLD_p`` Julia module API, running on
libgptsgld.so (HIP, gfx950).

Same function names, argument meaning, return values and error behaviour as the reference:

    feature(X, length_scale, sigma_RBF, phi_scale, Z, b)      GPT_SGLD.jl:71    (Gen D)
    feature(X, n, length_scale, sigma_RBF, seed, scale)       kin40kExperiment.jl:71 (Gen C)
    feature(X, n, length_scale, seed)                         GPT_SGLD_p.jl:40  (Gen A: b=randn)
    featureNotensor(X, length_scale, sigma_RBF, Z, b)         GPT_SGLD.jl:109   (Gen D)
    featureNotensor(X, n, length_scale, sigma_RBF, seed)      PowerPlantNoTensorExperiment.jl:32
    samplenz(r, D, Q, seed)                                   GPT_SGLD_p.jl:57
    GPTregression(phi, y, signal_var, I, r, Q, m, epsw, epsU, burnin, maxepoch[, param_seed];
                  langevin, stiefel)                          GPT_SGLD.jl:345
    GPTregression_chains(phis, y, ...) / GPTregression_chains_x(X, y, length_scales, sigma_RBFs,
                  phi_scale, Z, b, ...)                       kin40kExperiment.jl:67-74 (the sweeps)
    GPT_SGLDERM(phi, y, sigma, I, r, Q, m, epsw, epsU, burnin, maxepoch)  GPT_SGLD_p.jl:146
    GPT_SGLDERMw(phi, y, signal_var, I, r, Q, m, epsw, burnin, maxepoch)  GPT_SGLD.jl:1065
    GPTclassification(phi, y, I, r, Q, m, epsw, epsU, burnin, maxepoch[, param_seed];
                      langevin, stiefel)                      GPT_SGLD.jl:452
    GPT_GMC(phi, y, signal_var, I, r, Q, epsw, epsU, burnin, maxepoch, L, param_seed)
                                                              GPT_SGLD.jl:684
    pred(w, U, I, phitest)                                    GPT_SGLD.jl:233
    RMSE(w_store, U_store, I, phitest, ytest)                 GPT_SGLD_p.jl:124
    pred_mean_x(w_store, U_store, I, Xtest, ytest, ls, σ, scale, Z, b)  fused feature + pred
    GPNT_SGLD(phi, y, signal_var, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch,
              param_seed)                                     GPT_SGLD.jl:809
    GPNT_SGLDclass(phi, y, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch, param_seed)
                                                              GPT_SGLD.jl:851
    GPNT_SGLDclass_chains, class_eval(scores, ytest, window), GPNT_pred_class, pred_class
                                                              ImageExperiment.jl:50-72
    NoTensorMarginal(X, y, Z, b), GPNT_nlogmarginal, GPNT_gradnlogmarginal, GPNT_hyperparameters,
    GPNT_hyperparameters_optim                                GPT_SGLD.jl:921-1002
    GP_nlogmarginal(X, y, signal_var, sigma_RBF2, length_scale)   GPT_SGLD.jl:905
    ExactGP(X, y): nlogmarginal, gradnlogmarginal, value_and_grad, alpha, predict
                                                              GPkit InfExact / prediction
    SoftmaxJoint(X, y, Z, b, C): neglogjointlkhd, gradneglogjointlkhd, langevin, scores, evaluate
                                                              ImageExperiment.jl:135-204
        hmc, mala, leapfrog (HMCResult)                       BloodTransfusionExperiment.jl:255-278
    GPNT_hyperparameters_ng(init_theta, init_hyperparams, neglogjointlkhd, gradneglogjointlkhd,
                            Z, b; epsilon, num_sgld_iter, num_cg_iter)   GPT_SGLD.jl:1005
    datawhitening(X), proj, geod are not on the device path (host prep / inside the kernel).

Arrays follow Julia's column-major layout: ``phi`` is (n, D, N) Fortran-ordered, ``U`` is
(n, r, D), ``I`` is (Q, D) Int32 1-based.  Like the reference, a NaN in the geodesic prints
"Get NaN when moving along Geodesic. Try smaller epsU" and returns all-zero stores
(GPT_SGLD.jl:23-26,422-424); bad dimensions raise (the reference's ``error(...)``).

RNG: Julia's MersenneTwister stream is replaced by the framework's Philox contract
(oracle/philox.py documents it); seeds play the same role (``srand(param_seed)``).
"""
import collections
import contextlib
import math
import os

import numpy as np

from . import _lib
from ._lib import (GPT_ERR_BAD_DIMS, C, GPTError, P_D, P_I32, P_U64, SGLDConfig, check, lib)


def _f64(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _hvec(h):
    """A hyper-parameter vector as contiguous doubles."""
    return _f64(np.asarray(h, dtype=np.float64).ravel())


def _ptr(a, t=P_D):
    return a.ctypes.data_as(t)


# ------------------------------------------------------------------ data preparation (host)
def datawhitening(X):
    """GPT_SGLD.jl:62-67 — per-column (x - mean)/std, n-1 denominator (host-side data prep)."""
    X = np.array(X, dtype=np.float64, copy=True)
    if X.ndim == 1:
        return (X - X.mean()) / X.std(ddof=1)
    return (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)


# ------------------------------------------------------------------ features
def feature_inputs(n, D, seed):
    """Seeded ``Z = randn(n,D)``, ``b = 2π·rand(n,D)`` (Generation-C feature wrapper)."""
    Z = np.empty((n, D), order="F")
    b = np.empty((n, D), order="F")
    check(lib().gpt_feature_inputs(n, D, int(seed) & (2 ** 64 - 1), _ptr(Z), _ptr(b)))
    return Z, b


def feature_inputs_a(n, D, seed):
    """Seeded Generation-A inputs (GPT_SGLD_p.jl:40-54): ``Z = randn(n,D)``, ``b = randn(n,D)``."""
    Z = np.empty((n, D), order="F")
    b = np.empty((n, D), order="F")
    check(lib().gpt_feature_inputs_a(n, D, int(seed) & (2 ** 64 - 1), _ptr(Z), _ptr(b)))
    return Z, b


def epoch_orders(N, seed, epochs):
    """Row order of every epoch of a chain with ``param_seed`` = seed (randperm + phi[:,:,perm],
    GPT_SGLD.jl:373-374), built on the device: (N, epochs) int32, 0-based."""
    out = np.empty((int(N), int(epochs)), dtype=np.int32, order="F")
    check(lib().gpt_epoch_orders(int(N), int(seed) & (2 ** 64 - 1), int(epochs), _ptr(out, P_I32)))
    return out


def _feature_D(X, length_scale, sigma_RBF, phi_scale, Z, b):
    X = _f64(X)
    N, D = X.shape
    Z = _f64(Z)
    n = Z.shape[0]
    if Z.shape != (n, D):
        raise ValueError("Z must be (n, D)")
    b = _f64(np.asarray(b, dtype=np.float64).reshape((n, D), order="F"))
    ls = _f64(np.atleast_1d(length_scale))
    if ls.size not in (1, D):
        raise ValueError("dimensions of X and length_scale do not match")
    phi = np.empty((n, D, N), order="F")
    check(lib().gpt_feature(_ptr(X), N, D, _ptr(ls), ls.size, float(sigma_RBF), float(phi_scale),
                            _ptr(Z), _ptr(b), n, _ptr(phi)))
    return phi


def feature(X, *args):
    """Random Fourier features of the tensor model (all reference generations, see module doc)."""
    if len(args) == 5 and np.ndim(args[3]) == 2:          # Gen D: ls, σ, phi_scale, Z, b
        return _feature_D(X, *args)
    if len(args) == 5:                                    # Gen C: n, ls, σ, seed, scale
        n, ls, sigma, seed, scale = args
        Z, b = feature_inputs(int(n), np.shape(X)[1], seed)
        return _feature_D(X, ls, sigma, scale, Z, b)
    if len(args) == 4:                                    # Gen B: n, ls, seed, scale
        n, ls, seed, scale = args
        Z, b = feature_inputs(int(n), np.shape(X)[1], seed)
        return _feature_D(X, ls, 1.0, scale, Z, b)
    if len(args) == 3:                                    # Gen A: n, ls, seed
        # GPT_SGLD_p.jl:40-54: Z = randn(n,D)/length_scale, b = randn(n,D), phi = sqrt(2/n)·
        # cos(X[i,k]·Z[j,k] + b[j,k]) — no sigma_RBF / scale; Z/ℓ is formed first as there (the
        # kernel's argument X·Z'/1 is then the same double)
        n, ls, seed = args
        if np.size(ls) != 1:
            raise TypeError("feature(X,n,length_scale,seed): length_scale is a scalar (GPT_SGLD_p.jl:40)")
        Z, b = feature_inputs_a(int(n), np.shape(X)[1], seed)
        return _feature_D(X, 1.0, 1.0, 1.0, Z / float(np.ravel(ls)[0]), b)
    raise TypeError("feature: unsupported argument list")


def featureNotensor(X, *args):
    """Full-theta RFF features (GPT_SGLD.jl:109-120); Gen C form draws Z, b from ``seed``."""
    X = _f64(X)
    N, D = X.shape
    if len(args) != 4:
        raise TypeError("featureNotensor: unsupported argument list")
    if np.ndim(args[2]) != 2:                             # Gen C: n, ls, σ, seed
        return featureNotensor_seeded(X, *args)
    ls, sigma, Z, b = args                                # Gen D: ls, σ, Z, b
    Z = _f64(Z)
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    n = Z.shape[0]
    if Z.shape != (n, D) or b.size != n:
        raise ValueError("Z must be (n, D) and b of length n")
    ls = _f64(np.atleast_1d(ls))
    phi = np.empty((n, N), order="F")
    check(lib().gpt_feature_notensor(_ptr(X), N, D, _ptr(ls), ls.size, float(sigma), _ptr(Z),
                                     _ptr(b), n, _ptr(phi)))
    return phi


def featureNotensor_seeded(X, n, length_scale, sigma_RBF, seed):
    """Generation-C ``featureNotensor(X,n,ls,σ,seed)``: Z=randn(n,D), b=2π·rand(n)."""
    X = _f64(X)
    Z, b = feature_inputs(int(n), X.shape[1], seed)
    return featureNotensor(X, length_scale, sigma_RBF, Z, b[:, 0])


# ------------------------------------------------------------------ sparse core locations
def samplenz(r, D, Q, seed=0):
    """Q distinct lattice points of [r]^D (GPT_SGLD.jl:181-190), 1-based Int32 (Q, D)."""
    I = np.empty((Q, D), dtype=np.int32, order="F")
    check(lib().gpt_samplenz(r, D, Q, int(seed) & (2 ** 64 - 1), _ptr(I, P_I32)))
    return I


# ------------------------------------------------------------------ sampler
def make_config(n, D, N, r, Q, m, epsw, epsU, signal_var, sigma_w, burnin, maxepoch, seed,
                langevin=True, stiefel=True, store_every=1, max_steps=0):
    return SGLDConfig(n=n, D=D, N=N, r=r, Q=Q, m=m, epsw=float(epsw), epsU=float(epsU),
                      signal_var=float(signal_var), sigma_w=float(sigma_w), burnin=burnin,
                      maxepoch=maxepoch, seed=int(seed) & (2 ** 64 - 1), langevin=int(bool(langevin)),
                      stiefel=int(bool(stiefel)), store_every=store_every, max_steps=max_steps)


def init_state(n, r, D, Q, seed, stiefel=True, sigma_w=1.0):
    """Initial (w, U) GPTregression draws for ``param_seed`` (GPT_SGLD.jl:357-369)."""
    cfg = make_config(n, D, 1, r, Q, 1, 0, 0, 1.0, sigma_w, 0, 1, seed, stiefel=stiefel)
    w = np.empty(Q)
    U = np.empty((n, r, D), order="F")
    check(lib().gpt_sgld_init(C.byref(cfg), _ptr(w), _ptr(U)))
    return w, U


@contextlib.contextmanager
def _engine_env(engine):
    """GPTSGLD_ENGINE for the duration of one host-API call (the library reads it at session
    creation; include/gptsgld.h gpt_sgld_session_info)."""
    if engine is None:
        yield
        return
    if engine not in ("grid", "chain", "wave", "auto"):
        raise ValueError("engine must be 'grid', 'chain', 'wave' or 'auto'")
    old = os.environ.get("GPTSGLD_ENGINE")
    os.environ["GPTSGLD_ENGINE"] = engine
    try:
        yield
    finally:
        if old is None:
            del os.environ["GPTSGLD_ENGINE"]
        else:
            os.environ["GPTSGLD_ENGINE"] = old


def _run_counts(N, m, burnin, maxepoch, store_every=1, max_steps=0):
    """(batches per epoch, steps run, samples stored) of a sampler run, as the library counts
    them (session_counts, api_session.hip)."""
    nb = -(-N // m)
    total = (burnin + maxepoch) * nb
    return nb, total if max_steps <= 0 else min(total, max_steps), (maxepoch * nb) // store_every


def _sampler_inputs(phi, y, I, Q):
    """phi (n, D, N), y (N) and I (Q, D) as the library reads them, and (n, D, N)."""
    phi = _f64(phi)
    n, D, N = phi.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise ValueError("phi and y disagree on N")
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    if I.shape != (Q, D):
        raise ValueError("I must be (Q, D)")
    return phi, y, I, (n, D, N)


def _opt_ptr(a):
    """The pointer of an optional array argument (it keeps its array alive), or None."""
    return None if a is None else _ptr(_f64(a))


def _geodesic_epilogue(code, *stores):
    """The reference's message and all-zero stores on the geodesic NaN bail-out
    (GPT_SGLD.jl:422-424); any other code through check."""
    if code == _lib.GPT_ERR_NAN_GEODESIC:
        print("Get NaN when moving along Geodesic. Try smaller epsU")
        for s in stores:
            s[:] = 0.0
    else:
        check(code)


def GPTregression(phi, y, signal_var, I, r, Q, m, epsw, epsU, burnin, maxepoch, param_seed=0,
                  langevin=True, stiefel=True, sigma_w=1.0, store_every=1, max_steps=0,
                  w_init=None, U_init=None, diag=False, engine=None):
    """Tensor-GP regression sampler (GPT_SGLD.jl:345-448).  Returns (w_store, U_store)
    [, diag]; ``diag`` = per-step [‖gradw‖, ‖gradU_1‖, …] ((1+D) × steps).
    ``engine`` ("grid" | "chain" | "wave" | None = library default) selects the step kernel."""
    phi, y, I, (n, D, N) = _sampler_inputs(phi, y, I, Q)
    cfg = make_config(n, D, N, r, Q, m, epsw, epsU, signal_var, sigma_w, burnin, maxepoch,
                      param_seed, langevin, stiefel, store_every, max_steps)
    _, total, T = _run_counts(N, m, burnin, maxepoch, store_every, max_steps)
    w_store = np.zeros((Q, T), order="F")
    U_store = np.zeros((n, r, D, T), order="F")
    dg = np.zeros((1 + D, total), order="F") if diag else None
    with _engine_env(engine):
        code = lib().gpt_sgld_regression(C.byref(cfg), _ptr(phi), _ptr(y), _ptr(I, P_I32),
                                         _opt_ptr(w_init), _opt_ptr(U_init), _ptr(w_store),
                                         _ptr(U_store), _opt_ptr(dg))
    _geodesic_epilogue(code, w_store, U_store)
    return (w_store, U_store, dg) if diag else (w_store, U_store)


def _ptr_array(xs):
    return (P_D * len(xs))(*[_ptr(x) for x in xs])


def _regression_chains(call, seeds, y, I, dims, r, Q, m, epsw, epsU, signal_var, sigma_w, burnin,
                       maxepoch, store_every, max_steps, engine):
    """What the two _chains forms share: the per-chain scalars, the seeds, the zeroed stores and
    the returned list.  ``call(cfg, nchains, seeds, ys, I, epsw, epsU, signal_var, w_stores,
    U_stores, status)`` is the library entry with the caller's own inputs bound."""
    n, D, N = dims
    nch = len(seeds)
    ew, eu, sv = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (nch,)))
                  for v in (epsw, epsU, signal_var))
    cfg = make_config(n, D, N, r, Q, m, ew[0], eu[0], sv[0], sigma_w, burnin, maxepoch, 0, True,
                      True, store_every, max_steps)
    T = _run_counts(N, m, burnin, maxepoch, store_every)[2]
    ws = [np.zeros((Q, T), order="F") for _ in range(nch)]
    Us = [np.zeros((n, r, D, T), order="F") for _ in range(nch)]
    st = np.zeros(nch, dtype=np.int32)
    sd = np.array(seeds, dtype=np.uint64)
    with _engine_env(engine):
        check(call(C.byref(cfg), nch, sd.ctypes.data_as(P_U64), _ptr_array([y] * nch),
                   _ptr(I, P_I32), _ptr(ew), _ptr(eu), _ptr(sv), _ptr_array(ws), _ptr_array(Us),
                   _ptr(st, P_I32)))
    return [(ws[c], Us[c], int(st[c])) for c in range(nch)]


def GPTregression_chains(phis, y, signal_var, I, r, Q, m, epsw, epsU, burnin, maxepoch, seeds,
                         sigma_w=1.0, store_every=1, max_steps=0, engine=None):
    """Independent GPTregression chains in one call (gpt_sgld_regression_chains): the
    ``@parallel for j=1:10`` sweep block of kin40kExperiment.jl:67-74 (``phis`` a list with one
    phi per chain, each from its own length scales / sigma_RBF) or posterior chains on one phi
    (``phis`` a single array).  ``epsw``, ``epsU``, ``signal_var``: a scalar or one value per
    chain.  Returns a list of (w_store, U_store, status) per chain; status 1 = the geodesic NaN
    bail-out (that chain's stores are zeros, GPT_SGLD.jl:422-424)."""
    seeds = [int(s) & (2 ** 64 - 1) for s in seeds]
    nch = len(seeds)
    if not isinstance(phis, (list, tuple)):
        phis = [phis] * nch
    if len(phis) != nch:
        raise ValueError("one phi per chain, or one shared phi")
    uniq = {}
    for p in phis:                                  # one host copy per distinct array
        if id(p) not in uniq:
            uniq[id(p)] = _f64(p)
    ph = [uniq[id(p)] for p in phis]
    if any(p.shape != ph[0].shape for p in ph):
        raise ValueError("every phi must have the same (n, D, N)")
    _, y, I, dims = _sampler_inputs(ph[0], y, I, Q)
    return _regression_chains(
        lambda cfg, k, sd, ys, *rest: lib().gpt_sgld_regression_chains(cfg, k, sd, _ptr_array(ph),
                                                                       ys, *rest),
        seeds, y, I, dims, r, Q, m, epsw, epsU, signal_var, sigma_w, burnin, maxepoch, store_every,
        max_steps, engine)


def GPTregression_chains_x(X, y, length_scales, sigma_RBFs, phi_scale, Z, b, signal_var, I, r, Q,
                           m, epsw, epsU, burnin, maxepoch, seeds, sigma_w=1.0, store_every=1,
                           max_steps=0, engine=None):
    """GPTregression_chains from X (gpt_sgld_regression_chains_x): the sweep block of
    kin40kExperiment.jl:67-74 with chain c's ``feature(X, length_scales[c], sigma_RBFs[c],
    phi_scale, Z, b)`` formed on the device one minibatch ahead of the steps, so no phi (n, D, N)
    is built, held or uploaded.  ``length_scales``: one row per chain ((nchains,) scalars,
    (nchains, 1) or (nchains, D)); ``sigma_RBFs``: a scalar or one per chain; the rest and the
    return value as GPTregression_chains, whose stores on those phis these equal bit for bit."""
    seeds = [int(s) & (2 ** 64 - 1) for s in seeds]
    nch = len(seeds)
    X = _f64(X)
    if X.ndim != 2:
        raise ValueError("X must be (N, D)")
    N, D = X.shape
    Z = _f64(Z)
    n = Z.shape[0]
    if Z.shape != (n, D):
        raise ValueError("Z must be (n, D)")
    b = _f64(np.asarray(b, dtype=np.float64).reshape((n, D), order="F"))
    ls = np.asarray(length_scales, dtype=np.float64)
    if ls.ndim < 2:
        ls = ls.reshape(-1, 1)
    if ls.shape[0] != nch:
        raise ValueError("length_scales needs one row per chain")
    ls = np.ascontiguousarray(ls)                   # row c = chain c: Julia (ls_len, nchains)
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_RBFs, dtype=np.float64), (nch,)))
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise ValueError("X and y disagree on N")
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    if I.shape != (Q, D):
        raise ValueError("I must be (Q, D)")
    return _regression_chains(
        lambda cfg, k, sd, ys, Ip, *rest: lib().gpt_sgld_regression_chains_x(
            cfg, k, sd, _ptr(X), ys, _ptr(ls), ls.shape[1], _ptr(sg), float(phi_scale), _ptr(Z),
            _ptr(b), Ip, *rest),
        seeds, y, I, (n, D, N), r, Q, m, epsw, epsU, signal_var, sigma_w, burnin, maxepoch,
        store_every, max_steps, engine)


def GPT_SGLDERM_RMSprop(phi, y, signal_var, I, r, Q, m, epsilon, alpha, burnin, maxepoch,
                        param_seed=0, w_init=None, U_init=None, diag=False):
    """SGLD with RMSprop step sizes (GPT_SGLD.jl:1121-1237).  Returns (w_store, U_store)
    [, diag]; on the geodesic NaN bail-out prints the reference's message and returns zeros."""
    phi, y, I, (n, D, N) = _sampler_inputs(phi, y, I, Q)
    cfg = make_config(n, D, N, r, Q, m, epsilon, epsilon, signal_var, 1.0, burnin, maxepoch,
                      param_seed, True, True, 1, 0)
    _, total, T = _run_counts(N, m, burnin, maxepoch)
    w_store = np.zeros((Q, T), order="F")
    U_store = np.zeros((n, r, D, T), order="F")
    dg = np.zeros((1 + D, total), order="F") if diag else None
    code = lib().gpt_sgld_rmsprop(C.byref(cfg), float(epsilon), float(alpha), _ptr(phi), _ptr(y),
                                  _ptr(I, P_I32), _opt_ptr(w_init), _opt_ptr(U_init),
                                  _ptr(w_store), _ptr(U_store), _opt_ptr(dg))
    _geodesic_epilogue(code, w_store, U_store)
    return (w_store, U_store, dg) if diag else (w_store, U_store)


def GPT_SGLDERMw(phi, y, signal_var, I, r, Q, m, epsw, burnin, maxepoch, param_seed=0,
                 w_init=None, U_init=None, diag=False):
    """SGLD on w with U fixed at its uniform Stiefel draw (GPT_SGLD.jl:1065-1118).  Returns
    (w_store, U) [, gradw norms per step]."""
    phi, y, I, (n, D, N) = _sampler_inputs(phi, y, I, Q)
    cfg = make_config(n, D, N, r, Q, m, epsw, 0.0, signal_var, 1.0, burnin, maxepoch,
                      param_seed, True, True, 1, 0)
    _, total, T = _run_counts(N, m, burnin, maxepoch)
    w_store = np.zeros((Q, T), order="F")
    U = np.zeros((n, r, D), order="F")
    dg = np.zeros((1 + D, total), order="F") if diag else None
    check(lib().gpt_sgld_wonly(C.byref(cfg), _ptr(phi), _ptr(y), _ptr(I, P_I32), _opt_ptr(w_init),
                               _opt_ptr(U_init), _ptr(w_store), _ptr(U), _opt_ptr(dg)))
    return (w_store, U, dg[0].copy()) if diag else (w_store, U)


def GPTclassification(phi, y, I, r, Q, m, epsw, epsU, burnin, maxepoch, param_seed=0,
                      langevin=True, stiefel=True, w_init=None, U_init=None, diag=False):
    """Softmax tensor-GP classifier (GPT_SGLD.jl:452-680), labels y in 1..C.  Returns
    (w_store (Q, C, T), U_store (n, r, D, C, T)) [, diag (1+D, steps, C)]; on the geodesic NaN
    bail-out prints the reference's message and returns zeros."""
    phi, y, I, (n, D, N) = _sampler_inputs(phi, y, I, Q)
    ncls = int(y.max() - y.min() + 1)
    cfg = make_config(n, D, N, r, Q, m, epsw, epsU, 1.0, 1.0, burnin, maxepoch, param_seed,
                      langevin, stiefel, 1, 0)
    _, total, T = _run_counts(N, m, burnin, maxepoch)
    w_store = np.zeros((Q, ncls, T), order="F")
    U_store = np.zeros((n, r, D, ncls, T), order="F")
    dg = np.zeros((1 + D, total, ncls), order="F") if diag else None
    code = lib().gpt_sgld_classification(C.byref(cfg), _ptr(phi), _ptr(y), _ptr(I, P_I32),
                                         _opt_ptr(w_init), _opt_ptr(U_init), _ptr(w_store),
                                         _ptr(U_store), _opt_ptr(dg))
    _geodesic_epilogue(code, w_store, U_store)
    return (w_store, U_store, dg) if diag else (w_store, U_store)


def GPT_GMC(phi, y, signal_var, I, r, Q, epsw, epsU, burnin, maxepoch, L, param_seed=0,
            w_init=None, U_init=None):
    """Geodesic Monte Carlo (GPT_SGLD.jl:684-805).  Returns (w_store (Q, maxepoch),
    U_store (n, r, D, maxepoch), accept_prob (burnin+maxepoch)); on the geodesic NaN bail-out
    prints the reference's message and returns zeros and NaN probabilities."""
    phi, y, I, (n, D, N) = _sampler_inputs(phi, y, I, Q)
    w_store = np.zeros((Q, maxepoch), order="F")
    U_store = np.zeros((n, r, D, maxepoch), order="F")
    acc = np.zeros(burnin + maxepoch)
    code = lib().gpt_gmc(_ptr(phi), _ptr(y), n, D, N, r, Q, _ptr(I, P_I32), float(signal_var),
                         float(epsw), float(epsU), int(burnin), int(maxepoch), int(L),
                         int(param_seed) & (2 ** 64 - 1), _opt_ptr(w_init), _opt_ptr(U_init),
                         _ptr(w_store), _ptr(U_store), _ptr(acc))
    _geodesic_epilogue(code, w_store, U_store)
    return w_store, U_store, acc


def GPT_SGLDERM(phi, y, sigma, I, r, Q, m, epsw, epsU, burnin, maxepoch, param_seed=0, **kw):
    """Generation A/B sampler (GPT_SGLD_p.jl:146-243): ``sigma`` is the noise s.d. and the
    prior s.d. of w is sqrt(n^D/Q) (:155)."""
    n, D, _ = np.shape(phi)
    return GPTregression(phi, y, float(sigma) ** 2, I, r, Q, m, epsw, epsU, burnin, maxepoch,
                         param_seed, sigma_w=math.sqrt(float(n) ** D / Q), **kw)


# ------------------------------------------------------------------ prediction
def pred(w, U, I, phitest):
    """fhat = pred(w, U, I, phitest) (GPT_SGLD.jl:233-243)."""
    phitest = _f64(phitest)
    n, D, Nt = phitest.shape
    U = _f64(U)
    r = U.shape[1]
    w = _f64(np.asarray(w, dtype=np.float64).ravel())
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    out = np.empty(Nt)
    check(lib().gpt_pred(_ptr(w), _ptr(U), _ptr(I, P_I32), _ptr(phitest), n, D, Nt, r, w.size,
                         _ptr(out)))
    return out


def pred_mean(w_store, U_store, I, phitest, ytest, scale=1.0):
    """Posterior-mean prediction over the stored samples and its RMSE·scale
    (GPT_SGLD_p.jl:124-132; kin40kExperiment.jl:80-87).  Returns (meanfhat, rmse)."""
    phitest = _f64(phitest)
    n, D, Nt = phitest.shape
    w_store = _f64(w_store)
    U_store = _f64(U_store)
    Q, S = w_store.shape
    r = U_store.shape[1]
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    yt = _f64(np.asarray(ytest, dtype=np.float64).ravel())
    mean = np.empty(Nt)
    rm = C.c_double(0.0)
    check(lib().gpt_pred_mean(_ptr(w_store), _ptr(U_store), _ptr(I, P_I32), _ptr(phitest), _ptr(yt),
                              n, D, Nt, r, Q, S, float(scale), _ptr(mean), C.byref(rm)))
    return mean, rm.value


def pred_mean_x(w_store, U_store, I, Xtest, ytest, length_scale, sigma_RBF, phi_scale, Z, b,
                scale=1.0):
    """pred_mean with the test features formed inside the prediction kernel from Xtest (no
    n·D·Ntest phitest array; same doubles as ``feature(Xtest, length_scale, sigma_RBF,
    phi_scale, Z, b)``).  Returns (meanfhat, rmse, per-sample rmse) — the last is the
    ``testRMSE`` curve of kin40kExperiment.jl:78-83 when the samples are the epoch ends."""
    X, ls, Z, b, n = _tensor_inputs(Xtest, length_scale, Z, b)
    Nt, D = X.shape
    w_store = _f64(w_store)
    U_store = _f64(U_store)
    Q, S = w_store.shape
    r = U_store.shape[1]
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    yt = _f64(np.asarray(ytest, dtype=np.float64).ravel())
    mean = np.empty(Nt)
    srm = np.empty(S)
    rm = C.c_double(0.0)
    check(lib().gpt_pred_mean_x(_ptr(w_store), _ptr(U_store), _ptr(I, P_I32), _ptr(X), _ptr(yt), Nt,
                                D, _ptr(ls), ls.size, float(sigma_RBF), float(phi_scale), _ptr(Z),
                                _ptr(b), n, r, Q, S, float(scale), _ptr(mean), C.byref(rm),
                                _ptr(srm)))
    return mean, rm.value, srm


def RMSE(w_store, U_store, I, phitest, ytest):
    """GPT_SGLD_p.jl:124-132: RMSE of the mean prediction over ALL stored samples."""
    return pred_mean(w_store, U_store, I, phitest, ytest)[1]


# ------------------------------------------------------------------ full-theta model
def GPNT_SGLD(phi, y, signal_var, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch,
              param_seed=0):
    """Full-theta RFF SGLD (GPT_SGLD.jl:809-847).  Returns theta_store (n, T); on NaN prints
    the reference's message and returns zeros(n) (:840-843)."""
    phi = _f64(phi)
    n, N = phi.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    nb = -(-N // m)
    out = np.empty((n, (maxepoch + burnin) * nb), order="F")
    code = lib().gpt_gpnt_sgld(_ptr(phi), _ptr(y), n, N, float(signal_var), float(sigma_theta), m,
                               float(eps_theta), float(decay_rate), burnin, maxepoch,
                               int(param_seed) & (2 ** 64 - 1), _ptr(out))
    if code == _lib.GPT_ERR_NAN_THETA:
        print("Get NaN in theta. Try smaller epsilon")
        return np.zeros(n)
    check(code)
    return out


def _per_chain(values, nchains, what):
    v = _f64(np.atleast_1d(values)).ravel()
    if v.size == 1 and nchains > 1:
        v = _f64(np.full(nchains, v[0]))
    if v.size != nchains:
        raise ValueError("%s must be a scalar or have one entry per chain" % what)
    return v


def _chain_seeds(seeds, store_every):
    seeds = np.ascontiguousarray([int(s) & (2 ** 64 - 1) for s in np.atleast_1d(seeds)], dtype=np.uint64)
    if seeds.size < 1:
        raise ValueError("seeds must have one entry per chain")
    if int(store_every) < 1:
        raise ValueError("store_every must be >= 1")
    return seeds


def _chains_args(y, N, signal_vars, sigma_thetas, eps_thetas, seeds, store_every):
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise ValueError("the features and y disagree on N")
    seeds = _chain_seeds(seeds, store_every)
    k = seeds.size
    return (y, _per_chain(signal_vars, k, "signal_vars"), _per_chain(sigma_thetas, k, "sigma_thetas"),
            _per_chain(eps_thetas, k, "eps_thetas"), seeds)


def _chains_out(lead, N, m, burnin, maxepoch, store_every, nchains):
    if int(m) < 1:
        raise ValueError("m must be >= 1")
    kept = (int(maxepoch) + int(burnin)) * (-(-N // int(m))) // int(store_every)
    return np.zeros((*lead, max(kept, 0), nchains), order="F"), np.zeros(nchains, dtype=np.int32)


def GPNT_SGLD_chains(phi, y, signal_vars, sigma_thetas, m, eps_thetas, decay_rate, burnin, maxepoch,
                     seeds, store_every=1):
    """Sibling GPNT_SGLD chains on one phi / y in one launch (step-size, noise and seed sweeps):
    chain k runs GPNT_SGLD with signal_vars[k], sigma_thetas[k], eps_thetas[k] and seeds[k];
    scalars broadcast to the number of seeds.  ``store_every`` keeps the 1-based steps divisible
    by it (numbatches: the epoch ends; burn-in steps count).  Returns (theta_store (n, kept,
    nchains), status (nchains)); a chain that met a NaN has a zero store and status
    GPT_ERR_NAN_THETA."""
    phi = _f64(phi)
    n, N = phi.shape
    y, sv, sth, eps, seeds = _chains_args(y, N, signal_vars, sigma_thetas, eps_thetas, seeds,
                                          store_every)
    out, status = _chains_out((n,), N, m, burnin, maxepoch, store_every, seeds.size)
    check(lib().gpt_gpnt_sgld_chains(_ptr(phi), _ptr(y), n, N, int(m), _ptr(sv), _ptr(sth),
                                     _ptr(eps), float(decay_rate), int(burnin), int(maxepoch),
                                     _ptr(seeds, P_U64), seeds.size, int(store_every), _ptr(out),
                                     _ptr(status, P_I32)))
    return out, status


def _targets(ytest, Nt):
    yt = _f64(np.asarray(ytest, dtype=np.float64).ravel())
    if yt.size != Nt:
        raise ValueError("ytest must have one target per test row")
    return yt


def _tensor_inputs(X, length_scale, Z, b):
    """X (N, D), the length scale, Z (n, D) and b (n, D) of the tensor model's features, as the
    *_x prediction entries take them; shapes are left to the entries' own checks."""
    X = _f64(X)
    _, D = X.shape
    Z = _f64(Z)
    n = Z.shape[0]
    b = _f64(np.asarray(b, dtype=np.float64).reshape((n, D), order="F"))
    return X, _f64(np.atleast_1d(length_scale)), Z, b, n


def _notensor_inputs(X, length_scale, Z, b):
    X = _f64(X)
    if X.ndim != 2:
        raise ValueError("X must be (N, D)")
    D = X.shape[1]
    Z = _f64(Z)
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    n = Z.shape[0]
    if Z.shape != (n, D) or b.size != n:
        raise ValueError("Z must be (n, D) and b of length n")
    ls = _f64(np.atleast_1d(length_scale)).ravel()
    if ls.size not in (1, D):
        raise ValueError("dimensions of X and length_scale do not match")
    return X, ls, Z, b, n


def GPNT_SGLD_chains_x(X, y, length_scale, sigma_RBF, Z, b, signal_vars, sigma_thetas, m, eps_thetas,
                       decay_rate, burnin, maxepoch, seeds, store_every=1):
    """GPNT_SGLD_chains on phi = featureNotensor(X, length_scale, sigma_RBF, Z, b) formed on the
    device: the same doubles, and no (n, N) host array."""
    X, ls, Z, b, n = _notensor_inputs(X, length_scale, Z, b)
    N, D = X.shape
    y, sv, sth, eps, seeds = _chains_args(y, N, signal_vars, sigma_thetas, eps_thetas, seeds,
                                          store_every)
    out, status = _chains_out((n,), N, m, burnin, maxepoch, store_every, seeds.size)
    check(lib().gpt_gpnt_sgld_chains_x(_ptr(X), _ptr(y), N, D, _ptr(ls), ls.size, float(sigma_RBF),
                                       _ptr(Z), _ptr(b), n, int(m), _ptr(sv), _ptr(sth), _ptr(eps),
                                       float(decay_rate), int(burnin), int(maxepoch),
                                       _ptr(seeds, P_U64), seeds.size, int(store_every), _ptr(out),
                                       _ptr(status, P_I32)))
    return out, status


def gpnt_last_route():
    """The route of the last GPNT_SGLD_chains* call on this thread (gpt_gpnt_last_route): ``rows``
    staged per group (0 = not staged), ``groups`` per full batch, ``lds_bytes`` of the launches."""
    out = np.zeros(3, dtype=np.int32)
    check(lib().gpt_gpnt_last_route(_ptr(out, P_I32), out.size))
    return dict(rows=int(out[0]), groups=int(out[1]), lds_bytes=int(out[2]))


def gpnt_last_timing():
    """Device-event ms of the last calls on this thread (gpt_gpnt_last_timing): ``sampler`` the
    launches of GPNT_SGLD_chains*, ``eval`` the scores and reduction kernels of GPNT_pred*."""
    out = np.zeros(2)
    check(lib().gpt_gpnt_last_timing(_ptr(out), out.size))
    return dict(sampler=float(out[0]), eval=float(out[1]))


class RegEval:
    """Result of GPNT_pred / GPNT_pred_x: ``sample_rmse`` (T) the test RMSE of every sample,
    ``mean_fhat`` (Ntest) the prediction averaged over the window and ``rmse`` its test RMSE,
    ``window`` the half-open 0-based sample range, and ``scores`` (Ntest, T) when asked."""
    __slots__ = ("sample_rmse", "mean_fhat", "rmse", "window", "scores")

    def __repr__(self):
        return "RegEval(T=%d, rmse=%.6g, window=%r)" % (self.sample_rmse.size, self.rmse, self.window)


def _reg_samples(theta_store, cols, n, ytest, Nt, window):
    theta = np.asarray(theta_store, dtype=np.float64)
    if theta.ndim == 1:
        theta = theta.reshape((-1, 1))
    if theta.ndim != 2:
        raise ValueError("theta_store must be (n, T): one chain's samples")
    if cols is not None:
        theta = theta[:, np.asarray(cols, dtype=np.int64)]
    theta = _f64(theta)
    if theta.shape[0] != n:
        raise ValueError("theta_store and the test features disagree on n")
    T = theta.shape[1]
    yt = _targets(ytest, Nt)
    first, last = _window(window, T)
    if not 0 <= first < last <= T:
        raise ValueError("the window must satisfy 0 <= first < last <= %d" % T)
    return theta, yt, T, first, last


def _reg_eval_call(fn, head, Nt, T, first, last, scale, want_scores):
    res = RegEval()
    res.sample_rmse = np.empty(T)
    res.mean_fhat = np.empty(Nt)
    rmse = np.empty(1)
    res.scores = np.empty((Nt, T), order="F") if want_scores else None
    check(fn(*(head + [T, first, last, float(scale), _ptr(res.sample_rmse), _ptr(res.mean_fhat),
                       _ptr(rmse), _ptr(res.scores) if want_scores else None])))
    res.rmse = float(rmse[0])
    res.window = (first, last)
    return res


def GPNT_pred(theta_store, phitest, ytest, cols=None, window=None, scale=1.0, scores=False):
    """Evaluation of GPNT_SGLD samples (PowerPlantNoTensorExperiment.jl:51-63): theta_store (n, T)
    of one chain, phitest (n, Ntest).  ``cols`` selects stored samples (0-based) on the host before
    the call; ``window`` is the half-open 0-based range over the selected samples whose averaged
    prediction is scored ((59, 100) is Julia's 60:100; default all); ``scale`` multiplies every
    RMSE (ytrainStd).  Returns a RegEval."""
    phitest = _f64(phitest)
    if phitest.ndim != 2:
        raise ValueError("phitest must be (n, Ntest)")
    n, Nt = phitest.shape
    theta, yt, T, first, last = _reg_samples(theta_store, cols, n, ytest, Nt, window)
    return _reg_eval_call(lib().gpt_gpnt_pred, [_ptr(theta), _ptr(phitest), _ptr(yt), n, Nt], Nt, T,
                          first, last, scale, bool(scores))


def GPNT_pred_x(theta_store, Xtest, ytest, length_scale, sigma_RBF, Z, b, cols=None, window=None,
                scale=1.0, scores=False):
    """GPNT_pred on phitest = featureNotensor(Xtest, length_scale, sigma_RBF, Z, b) formed on the
    device."""
    Xtest, ls, Z, b, n = _notensor_inputs(Xtest, length_scale, Z, b)
    Nt, D = Xtest.shape
    theta, yt, T, first, last = _reg_samples(theta_store, cols, n, ytest, Nt, window)
    return _reg_eval_call(lib().gpt_gpnt_pred_x,
                          [_ptr(theta), _ptr(Xtest), _ptr(yt), Nt, D, _ptr(ls), ls.size,
                           float(sigma_RBF), _ptr(Z), _ptr(b), n], Nt, T, first, last, scale,
                          bool(scores))


# ------------------------------------------------------------------ posterior predictive of the samples
class PredictiveEval:
    """Posterior predictive of stored regression samples over a window of S of them, at noise
    variance ``signal_var`` (predictive.hip).  Arrays are in the model's units:

    ``gp``          GPPrediction(ymu, ys2, fmu, fs2, lp): fmu the window's mean prediction, fs2 its
                    variance over the samples (divisor S), ymu = fmu, ys2 = fs2 + signal_var (the
                    mean and variance of the equal-weight mixture of the S Gaussians) and lp the
                    moment-matched log density of ytest, ExactGP.predict's formula
    ``lp_mix``      log((1/S) Σ_s N(ytest | f_s, signal_var)), the Monte-Carlo predictive density
    ``mnlp``, ``mnlp_mix``   −mean(lp) + log(scale), −mean(lp_mix) + log(scale): per target in the
                    units of the unstandardised targets
    ``coverage95``  the share of rows with |ytest − ymu| <= 1.959963984540054·sqrt(ys2)
    ``rmse``, ``sample_rmse``   scale·RMSE of fmu and of every stored sample, as GPNT_pred's
    ``sample_loglik``   −SSE_s/(2 signal_var) − (Ntest/2) log(2π signal_var) of every sample
    ``mean_fhat``   fmu;  ``window`` the half-open 0-based sample range."""
    __slots__ = ("gp", "lp_mix", "mnlp", "mnlp_mix", "coverage95", "rmse", "sample_rmse",
                 "sample_loglik", "window")

    @property
    def mean_fhat(self):
        return self.gp.fmu

    def __repr__(self):
        return "PredictiveEval(T=%d, rmse=%.6g, mnlp=%.6g, mnlp_mix=%.6g, coverage95=%.4g, window=%r)" % (
            self.sample_rmse.size, self.rmse, self.mnlp, self.mnlp_mix, self.coverage95, self.window)


def _predictive_call(fn, head, Nt, T, first, last, scale, signal_var, scale_in_call=True):
    """fn(*head, [scale,] first, last, ..., the eight outputs) into a PredictiveEval; ``head``
    ends where the C entry's ``scale`` (or, without one, ``first``) begins."""
    if not 0 <= first < last <= T:
        raise ValueError("the window must satisfy 0 <= first < last <= %d" % T)
    scale, nv = float(scale), float(signal_var)
    fmu, fs2, lp, lpmix = (np.empty(Nt) for _ in range(4))
    sums, covered, rmse, srm = np.empty(2), np.empty(1), np.empty(1), np.empty(T)
    check(fn(*(head + [_ptr(fmu), _ptr(fs2), _ptr(lp), _ptr(lpmix), _ptr(sums), _ptr(covered),
                       _ptr(rmse), _ptr(srm)])))
    if not scale_in_call:
        rmse *= scale
        srm *= scale
    res = PredictiveEval()
    res.gp = GPPrediction(fmu, fs2 + nv, fmu, fs2, lp)
    res.lp_mix = lpmix
    res.mnlp = -float(sums[0]) / Nt + math.log(scale)
    res.mnlp_mix = -float(sums[1]) / Nt + math.log(scale)
    res.coverage95 = float(covered[0]) / Nt
    res.rmse = float(rmse[0])
    res.sample_rmse = srm
    sse = Nt * (srm / scale) ** 2
    res.sample_loglik = -sse / (2.0 * nv) - 0.5 * Nt * math.log(2.0 * math.pi * nv)
    res.window = (first, last)
    return res


def predictive(scores, ytest, signal_var, window=None, scale=1.0):
    """The predictive of predictions ``scores`` (Ntest, T), one column per sample (what
    ``GPNT_pred(..., scores=True).scores`` or a stack of ``pred`` columns holds), against ytest.
    ``window=(a, b)`` is the half-open 0-based range of the columns that enter (Julia's a+1:b;
    default all); the per-sample figures cover all T.  Returns a PredictiveEval."""
    F = _f64(scores)
    if F.ndim == 1:
        F = F.reshape((-1, 1), order="F")
    if F.ndim != 2:
        raise ValueError("scores must be (Ntest, T)")
    Nt, T = F.shape
    yt = _targets(ytest, Nt)
    first, last = _window(window, T)
    return _predictive_call(lib().gpt_predictive,
                            [_ptr(F), _ptr(yt), Nt, T, first, last, float(signal_var)], Nt, T,
                            first, last, scale, signal_var, scale_in_call=False)


def _tensor_samples(w_store, U_store, I, cols, n, D):
    w = np.asarray(w_store, dtype=np.float64)
    U = np.asarray(U_store, dtype=np.float64)
    if w.ndim == 1:
        w = w.reshape(w.shape + (1,))
        U = U.reshape(U.shape + (1,))
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64)
        w, U = w[:, cols], U[:, :, :, cols]
    w, U = _f64(w), _f64(U)
    Q, S = w.shape
    r = U.shape[1]
    if U.shape != (n, r, D, S):
        raise ValueError("U_store must be (n, r, D, S)")
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    if I.shape != (Q, D):
        raise ValueError("I must be (Q, D)")
    return w, U, I, r, Q, S


def pred_predictive(w_store, U_store, I, phitest, ytest, signal_var, cols=None, window=None,
                    scale=1.0):
    """The predictive of GPTregression's stored samples w_store (Q, S), U_store (n, r, D, S) on
    phitest (n, D, Ntest): pred_mean's prediction, evaluated on the device where it lies.  ``cols``
    selects stored samples (0-based) on the host before the call, ``window`` a range of the
    selected ones, ``scale`` (ytrainStd) enters the scalars only.  Returns a PredictiveEval."""
    phitest = _f64(phitest)
    n, D, Nt = phitest.shape
    w, U, I, r, Q, S = _tensor_samples(w_store, U_store, I, cols, n, D)
    yt = _targets(ytest, Nt)
    first, last = _window(window, S)
    return _predictive_call(lib().gpt_pred_predictive,
                            [_ptr(w), _ptr(U), _ptr(I, P_I32), _ptr(phitest), _ptr(yt), n, D, Nt, r,
                             Q, S, float(scale), first, last, float(signal_var)], Nt, S, first, last,
                            scale, signal_var)


def pred_predictive_x(w_store, U_store, I, Xtest, ytest, length_scale, sigma_RBF, phi_scale, Z, b,
                      signal_var, cols=None, window=None, scale=1.0):
    """pred_predictive with the test features formed on the device from Xtest, as pred_mean_x
    (the same doubles as ``feature(Xtest, length_scale, sigma_RBF, phi_scale, Z, b)``)."""
    X, ls, Z, b, n = _tensor_inputs(Xtest, length_scale, Z, b)
    Nt, D = X.shape
    w, U, I, r, Q, S = _tensor_samples(w_store, U_store, I, cols, n, D)
    yt = _targets(ytest, Nt)
    first, last = _window(window, S)
    return _predictive_call(lib().gpt_pred_predictive_x,
                            [_ptr(w), _ptr(U), _ptr(I, P_I32), _ptr(X), _ptr(yt), Nt, D, _ptr(ls),
                             ls.size, float(sigma_RBF), float(phi_scale), _ptr(Z), _ptr(b), n, r, Q,
                             S, float(scale), first, last, float(signal_var)], Nt, S, first, last,
                            scale, signal_var)


def GPNT_predictive(theta_store, phitest, ytest, signal_var, cols=None, window=None, scale=1.0):
    """The predictive of GPNT_SGLD samples theta_store (n, T) on phitest (n, Ntest): GPNT_pred's
    scores, evaluated on the device where they lie.  ``cols``, ``window`` and ``scale`` as in
    GPNT_pred.  Returns a PredictiveEval."""
    phitest = _f64(phitest)
    if phitest.ndim != 2:
        raise ValueError("phitest must be (n, Ntest)")
    n, Nt = phitest.shape
    theta, yt, T, first, last = _reg_samples(theta_store, cols, n, ytest, Nt, window)
    return _predictive_call(lib().gpt_gpnt_predictive,
                            [_ptr(theta), _ptr(phitest), _ptr(yt), n, Nt, T, first, last,
                             float(scale), float(signal_var)], Nt, T, first, last, scale, signal_var)


def GPNT_predictive_x(theta_store, Xtest, ytest, length_scale, sigma_RBF, Z, b, signal_var,
                      cols=None, window=None, scale=1.0):
    """GPNT_predictive on phitest = featureNotensor(Xtest, length_scale, sigma_RBF, Z, b) formed on
    the device."""
    Xtest, ls, Z, b, n = _notensor_inputs(Xtest, length_scale, Z, b)
    Nt, D = Xtest.shape
    theta, yt, T, first, last = _reg_samples(theta_store, cols, n, ytest, Nt, window)
    return _predictive_call(lib().gpt_gpnt_predictive_x,
                            [_ptr(theta), _ptr(Xtest), _ptr(yt), Nt, D, _ptr(ls), ls.size,
                             float(sigma_RBF), _ptr(Z), _ptr(b), n, T, first, last, float(scale),
                             float(signal_var)], Nt, T, first, last, scale, signal_var)


def predictive_last_timing():
    """Device-event ms of the evaluator's kernels alone in the last *predictive* call on this
    thread (gpt_predictive_last_timing)."""
    out = np.zeros(1)
    check(lib().gpt_predictive_last_timing(_ptr(out)))
    return float(out[0])


# ------------------------------------------------------------------ chain diagnostics of a store
class ChainDiag:
    """Diagnostics of a store x[p, s, m] over a window of S samples of M chains (diag.hip), per
    parameter (or test row) p:

    ``mean``, ``sd``   the mean of the chain means and sqrt(var+), var+ = W·(S−1)/S + B/S
    ``rhat``           split R-hat: every chain's first and last ⌊S/2⌋ samples as 2M sequences
    ``acf``            (P, K+1), with ``acf=True``: the combined autocorrelation ρ̂_k of BDA3 §11.5
    ``tau``, ``ess``, ``mcse``   Geyer's initial-monotone-sequence autocorrelation time (at least
                       1/log10(M·S)), M·S/tau and sd/sqrt(ess)
    ``truncated``      1 where the K lags ran out before a pair of autocorrelations summed to <= 0:
                       ``ess`` is then an upper bound (max_lag too small, or chains that disagree)
    ``chain_mean``, ``chain_var``   (P, M): every chain's mean and variance (divisor S − 1)
    ``chain_acf``      (P, K+1, M), with ``chain_acf=True``: acov_m(k)/acov_m(0) of every chain
    ``max_rhat``, ``min_ess``   over the parameters that are not constant (NaN when all are)
    ``n_truncated``    the number of parameters with ``truncated`` set
    A constant parameter (var+ == 0) has NaN rhat, ess, mcse, tau and acf and truncated 0.
    ``window`` is the half-open 0-based sample range, ``max_lag`` the K in use."""
    __slots__ = ("mean", "sd", "rhat", "ess", "mcse", "tau", "truncated", "chain_mean", "chain_var",
                 "acf", "chain_acf", "max_rhat", "min_ess", "n_truncated", "window", "max_lag")

    def __repr__(self):
        return "ChainDiag(P=%d, window=%r, max_lag=%d, max_rhat=%.4g, min_ess=%.4g, n_truncated=%d)" % (
            len(self.mean), self.window, self.max_lag, self.max_rhat, self.min_ess, self.n_truncated)


def _diag_store(store):
    """The store as one column-major (P, T, M) array."""
    if isinstance(store, (list, tuple)):
        chains = [np.asarray(c, dtype=np.float64) for c in store]
        if not chains or any(c.ndim < 1 or c.shape != chains[0].shape for c in chains):
            raise ValueError("a list store needs M arrays (..., T) of one shape")
        T = chains[0].shape[-1]
        x = np.empty((chains[0].size // max(T, 1), T, len(chains)), order="F")
        for m, c in enumerate(chains):
            x[:, :, m] = c.reshape((-1, T), order="F")
        return x
    x = np.asarray(store, dtype=np.float64)
    if x.ndim == 2:
        x = x.reshape(x.shape + (1,))
    if x.ndim != 3:
        raise ValueError("store must be (P, T), (P, T, M) or a list of M arrays (..., T)")
    return _f64(x)


def _diag_summary(rhat, ess, truncated):
    live = ~np.isnan(rhat)
    return (float(rhat[live].max()) if live.any() else float("nan"),
            float(ess[live].min()) if live.any() else float("nan"), int(truncated.sum()))


def chain_diagnostics(store, window=None, max_lag=None, acf=False, chain_acf=False):
    """Split R-hat, ESS, MCSE and the autocorrelation of a store on the device (gpt_chain_diag).

    ``store``: (P, T) of one chain, (P, T, M), or a list of M arrays (..., T) whose leading axes
    are flattened in column-major order: ``[w for w, U, st in GPTregression_chains(...)]``,
    ``GPNT_SGLD_chains``'s (n, T, nchains) store, ``[res.theta_store]`` of an HMCResult, or stacked
    predictions (Ntest, T, M).  ``window=(a, b)`` is the half-open 0-based sample range (default
    all; b − a >= 4), ``max_lag`` the largest lag (default min(S − 1, 256)).  Returns a ChainDiag."""
    x = _diag_store(store)
    P, T, M = x.shape
    first, last = _window(window, T)
    if not 0 <= first < last <= T or last - first < 4:
        raise ValueError("the window must satisfy 0 <= first < last <= %d with last - first >= 4" % T)
    S = last - first
    max_lag = min(S - 1, 256) if max_lag is None else int(max_lag)
    K = min(max_lag, S - 1)
    rows = [np.empty(P) for _ in range(6)]
    trunc = np.empty(P, dtype=np.int32)
    cm, cv = np.empty((P, M), order="F"), np.empty((P, M), order="F")
    ac = np.empty((P, K + 1), order="F") if acf else None
    ca = np.empty((P, K + 1, M), order="F") if chain_acf else None
    check(lib().gpt_chain_diag(_ptr(x), P, T, M, first, last, max_lag, *[_ptr(r) for r in rows],
                               _ptr(trunc, P_I32), _ptr(cm), _ptr(cv), _opt_ptr(ac), _opt_ptr(ca)))
    d = ChainDiag()
    d.mean, d.sd, d.rhat, d.ess, d.mcse, d.tau = rows
    d.truncated, d.chain_mean, d.chain_var, d.acf, d.chain_acf = trunc, cm, cv, ac, ca
    d.max_rhat, d.min_ess, d.n_truncated = _diag_summary(d.rhat, d.ess, trunc)
    d.window, d.max_lag = (first, last), K
    return d


def diag_last_timing():
    """Device-event ms of the kernels alone in the last chain_diagnostics call on this thread
    (gpt_diag_last_timing)."""
    out = np.zeros(1)
    check(lib().gpt_diag_last_timing(_ptr(out)))
    return float(out[0])


def diag_tiling():
    """dict(time_chunk, lag_block, lag_group) of the autocovariance kernel (gpt_diag_tiling)."""
    out = np.zeros(3, dtype=np.int32)
    check(lib().gpt_diag_tiling(_ptr(out, P_I32), out.size))
    return dict(time_chunk=int(out[0]), lag_block=int(out[1]), lag_group=int(out[2]))


# ------------------------------------------------------------------ classification
def GPNT_SGLDclass(phi, y, sigma_theta, m, eps_theta, decay_rate, burnin, maxepoch, param_seed=0):
    """Full-theta softmax SGLD (GPT_SGLD.jl:851-901), labels y in 1..C.  Returns theta_store
    (n, C, T); on NaN prints the reference's message and returns zeros(n) (:894-897)."""
    phi = _f64(phi)
    n, N = phi.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise ValueError("phi and y disagree on N")
    ncls = int(y.max() - y.min() + 1)
    nb = -(-N // m)
    out = np.empty((n, max(ncls, 1), (maxepoch + burnin) * nb), order="F")
    code = lib().gpt_gpnt_sgld_class(_ptr(phi), _ptr(y), n, N, float(sigma_theta), int(m),
                                     float(eps_theta), float(decay_rate), int(burnin),
                                     int(maxepoch), int(param_seed) & (2 ** 64 - 1), _ptr(out))
    if code == _lib.GPT_ERR_NAN_THETA:
        print("Get NaN in theta. Try smaller epsilon")
        return np.zeros(n)
    check(code)
    return out


def GPNT_SGLDclass_chains(phi, y, sigma_theta, m, eps_thetas, decay_rate, burnin, maxepoch, seeds,
                          store_every=1, ncls=None):
    """Sibling GPNT_SGLDclass chains on one phi / y in one launch (step-size and seed sweeps):
    chain k uses eps_thetas[k] and seeds[k].  ``store_every`` keeps the 1-based steps divisible
    by it (numbatches: the epoch ends).  Returns (theta_store (n, C, kept, nchains), status
    (nchains)); a chain that met a NaN has a zero store and status GPT_ERR_NAN_THETA."""
    phi = _f64(phi)
    n, N = phi.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise ValueError("phi and y disagree on N")
    if ncls is None:
        ncls = int(y.max() - y.min() + 1)
    seeds = _chain_seeds(seeds, store_every)
    eps = _per_chain(eps_thetas, seeds.size, "eps_thetas")
    out, status = _chains_out((n, max(int(ncls), 1)), N, m, burnin, maxepoch, store_every,
                              seeds.size)
    check(lib().gpt_gpnt_sgld_class_chains(_ptr(phi), _ptr(y), n, N, int(ncls), float(sigma_theta),
                                           int(m), _ptr(eps), float(decay_rate), int(burnin),
                                           int(maxepoch), _ptr(seeds, P_U64), seeds.size,
                                           int(store_every), _ptr(out), _ptr(status, P_I32)))
    return out, status


class ClassEval:
    """Result of the evaluation functions: ``prop_missed`` and ``mean_nlp`` (one per sample),
    ``avg_prop_missed`` and ``avg_mean_nlp`` of the scores averaged over the window, ``mean_fhat``
    (Ntest, C) those averaged scores, ``prediction`` (Ntest, 1-based) and ``nlp`` (Ntest) on them,
    ``window`` the half-open 0-based sample range, and ``scores`` (Ntest, C, T) when asked."""
    __slots__ = ("prop_missed", "mean_nlp", "avg_prop_missed", "avg_mean_nlp", "mean_fhat",
                 "prediction", "nlp", "window", "scores")

    def __repr__(self):
        return "ClassEval(T=%d, avg_prop_missed=%.6g, avg_mean_nlp=%.6g, window=%r)" % (
            self.prop_missed.size, self.avg_prop_missed, self.avg_mean_nlp, self.window)


def _labels(ytest, Nt):
    yt = np.asarray(ytest).ravel()
    if yt.size != Nt:
        raise ValueError("ytest must have one label per test row")
    yi = np.ascontiguousarray(yt, dtype=np.int32)
    if not np.array_equal(yi, yt):
        raise ValueError("labels must be integers")
    return yi


def _window(window, T):
    first, last = (0, T) if window is None else (int(window[0]), int(window[1]))
    return first, last


def _class_eval_call(fn, head, Nt, ncls, T, window, want_scores):
    first, last = _window(window, T)
    res = ClassEval()
    res.prop_missed = np.empty(T)
    res.mean_nlp = np.empty(T)
    avg = np.empty(2)
    res.mean_fhat = np.empty((Nt, ncls), order="F")
    res.prediction = np.empty(Nt, dtype=np.int32)
    res.nlp = np.empty(Nt)
    res.scores = np.empty((Nt, ncls, T), order="F") if want_scores else None
    tail = [first, last, _ptr(res.prop_missed), _ptr(res.mean_nlp), _ptr(avg), _ptr(res.mean_fhat),
            _ptr(res.prediction, P_I32), _ptr(res.nlp)]
    if want_scores is not None:
        tail.append(_ptr(res.scores) if want_scores else None)
    check(fn(*(head + tail)))
    res.avg_prop_missed, res.avg_mean_nlp = float(avg[0]), float(avg[1])
    res.window = (first, last)
    return res


def class_eval(scores, ytest, window=None):
    """Miss rate and mean negative log predictive probability of class scores (Ntest, C, T)
    against labels in 1..C, per sample and on the scores averaged over ``window`` (0-based,
    half open; default all samples): ImageExperiment.jl:50-72."""
    scores = _f64(scores)
    if scores.ndim == 2:
        scores = scores.reshape(scores.shape + (1,), order="F")
    Nt, ncls, T = scores.shape
    yi = _labels(ytest, Nt)
    return _class_eval_call(lib().gpt_class_eval, [_ptr(scores), _ptr(yi, P_I32), Nt, ncls, T], Nt,
                            ncls, T, window, None)


def GPNT_pred_class(theta_store, phitest, ytest, cols=None, window=None, scores=False):
    """Evaluation of GPNT_SGLDclass samples (ImageNoTensorExperiment.jl:50-75): theta_store
    (n, C, T), phitest (n, Ntest).  ``cols`` selects stored samples (0-based; the end of 1-based
    epoch e is numbatches*e - 1) on the host before the call."""
    theta = np.asarray(theta_store, dtype=np.float64)
    if theta.ndim == 2:
        theta = theta.reshape(theta.shape + (1,))
    if cols is not None:
        theta = theta[:, :, np.asarray(cols, dtype=np.int64)]
    theta = _f64(theta)
    phitest = _f64(phitest)
    n, Nt = phitest.shape
    if theta.shape[0] != n:
        raise ValueError("theta_store and phitest disagree on n")
    _, ncls, T = theta.shape
    yi = _labels(ytest, Nt)
    return _class_eval_call(lib().gpt_gpnt_pred_class,
                            [_ptr(theta), _ptr(phitest), _ptr(yi, P_I32), n, Nt, ncls, T], Nt, ncls,
                            T, window, bool(scores))


def pred_class(w_store, U_store, I, phitest, ytest, cols=None, window=None, scores=False):
    """Evaluation of GPTclassification samples (ImageExperiment.jl:50-72): w_store (Q, C, T),
    U_store (n, r, D, C, T), phitest (n, D, Ntest) uploaded once; the scores are ``pred`` of every
    (class, sample).  ``cols`` as in GPNT_pred_class."""
    w = np.asarray(w_store, dtype=np.float64)
    U = np.asarray(U_store, dtype=np.float64)
    if w.ndim == 2:
        w = w.reshape(w.shape + (1,))
        U = U.reshape(U.shape + (1,))
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64)
        w, U = w[:, :, cols], U[:, :, :, :, cols]
    w, U = _f64(w), _f64(U)
    phitest = _f64(phitest)
    n, D, Nt = phitest.shape
    Q, ncls, T = w.shape
    r = U.shape[1]
    if U.shape != (n, r, D, ncls, T):
        raise ValueError("U_store must be (n, r, D, C, T)")
    I = np.asfortranarray(np.asarray(I, dtype=np.int32))
    if I.shape != (Q, D):
        raise ValueError("I must be (Q, D)")
    yi = _labels(ytest, Nt)
    return _class_eval_call(lib().gpt_pred_class,
                            [_ptr(w), _ptr(U), _ptr(I, P_I32), _ptr(phitest), _ptr(yi, P_I32), n, D,
                             Nt, r, Q, ncls, T], Nt, ncls, T, window, bool(scores))


# ------------------------------------------------------------------ full-theta model: hyper-parameters
GPPrediction = collections.namedtuple("GPPrediction", "ymu ys2 fmu fs2 lp")
GPPosteriorDraw = collections.namedtuple("GPPosteriorDraw", "fmu samples cov z")
RFFKernelError = collections.namedtuple("RFFKernelError", "frob norm_K max_abs")


def _bad_dims(msg):
    return GPTError(GPT_ERR_BAD_DIMS, msg)


def _gpnt_test_args(Xtest, ytest, D):
    Xtest = _f64(Xtest)
    if Xtest.ndim != 2 or Xtest.shape[1] != D or Xtest.shape[0] < 1:
        raise _bad_dims("Xtest must be (Ntest, D) with Ntest >= 1")
    yt = None
    if ytest is not None:
        yt = _f64(np.asarray(ytest, dtype=np.float64).ravel())
        if yt.size != Xtest.shape[0]:
            raise _bad_dims("ytest must have length Ntest")
    return Xtest, yt


def _gp_test_args(Xtest, ytest, D):
    """ExactGP's and SoftmaxJoint's form of the check: a badly shaped argument is a ValueError."""
    Xtest = _f64(Xtest)
    if Xtest.ndim != 2 or Xtest.shape[1] != D:
        raise ValueError("Xtest must be (Ntest, D)")
    yt = None
    if ytest is not None:
        yt = _f64(np.asarray(ytest, dtype=np.float64).ravel())
        if yt.size != Xtest.shape[0]:
            raise ValueError("ytest must have length Ntest")
    return Xtest, yt


def _predict_call(fn, head, h, Xtest, yt, chunk=()):
    """fn(*head, h, len(h), Xtest, Ntest, ytest, *chunk, fmu, fs2, lp) as a GPPrediction."""
    Nt = Xtest.shape[0]
    fmu, fs2 = np.empty(Nt), np.empty(Nt)
    lp = np.empty(Nt) if yt is not None else None
    check(fn(*head, _ptr(h), h.size, _ptr(Xtest), Nt, _ptr(yt) if yt is not None else None, *chunk,
             _ptr(fmu), _ptr(fs2), _ptr(lp) if lp is not None else None))
    return GPPrediction(fmu, fs2 + h[-1], fmu, fs2, lp)


class _Handle:
    """Owner of one library handle, ``_h``; ``_destroy`` names the entry that frees it."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown: the library may be gone already
            pass


class _Marginal(_Handle):
    """What NoTensorMarginal and ExactGP share: the evaluation at ``h`` through ``_eval_entry``
    (its third output has ``_nextra`` entries) and the prediction through ``_predict_entry``,
    whose test arguments ``_test_args`` checks."""
    _eval_entry = _predict_entry = _test_args = None

    def _eval(self, h, want_grad, want_extra=False):
        h = _hvec(h)
        val = C.c_double()
        grad = np.empty(h.size) if want_grad else None
        extra = np.empty(self._nextra) if want_extra else None
        check(getattr(lib(), self._eval_entry)(self._h, _ptr(h), h.size, 1 if want_grad else 0,
                                               C.byref(val), _ptr(grad) if want_grad else None,
                                               _ptr(extra) if want_extra else None))
        return val.value, grad, extra

    def nlogmarginal(self, h):
        return self._eval(h, False)[0]

    def gradnlogmarginal(self, h):
        return self._eval(h, True)[1]

    def value_and_grad(self, h):
        return self._eval(h, True)[:2]

    def _predict(self, h, Xtest, ytest, chunk):
        h = _hvec(h)
        Xtest, yt = self._test_args(Xtest, ytest, self.D)
        return _predict_call(getattr(lib(), self._predict_entry), [self._h], h, Xtest, yt,
                             (0 if chunk is None else int(chunk),))


class NoTensorMarginal(_Marginal):
    """Device-resident Gaussian marginal likelihood of the no-tensor RFF GP (GPT_SGLD.jl:921-962
    with featureNotensor / gradfeatureNotensor as the feature closures).

    ``X`` (N, D), ``y`` (N), ``Z`` (n, D), ``b`` (n) are uploaded once; every method takes
    ``h = [length_scale (D entries, or one: the scalar form); sigma_RBF; signal_var]``.
    n <= 1024, D <= 16.  A failed Cholesky raises ``GPTError`` (GPT_ERR_NOT_SPD), as the
    reference's ``cholfact`` throws."""
    _destroy, _eval_entry, _predict_entry = "gpt_nlml_destroy", "gpt_nlml_eval", "gpt_nlml_predict"
    _test_args = staticmethod(_gpnt_test_args)

    def __init__(self, X, y, Z, b):
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError("X must be (N, D)")
        N, D = X.shape
        Z = _f64(Z)
        n = Z.shape[0]
        y = _f64(np.asarray(y, dtype=np.float64).ravel())
        b = _f64(np.asarray(b, dtype=np.float64).ravel())
        if Z.shape != (n, D) or b.size != n or y.size != N:
            raise ValueError("Z must be (n, D), b of length n and y of length N")
        self.n, self.N, self.D = n, N, D
        self._nextra = n
        self._h = C.c_void_p()
        check(lib().gpt_nlml_create(_ptr(X), N, D, _ptr(y), _ptr(Z), _ptr(b), n, C.byref(self._h)))

    def theta_mean(self, h):
        """l = A^-1 phi y at h: the posterior mean of the full-theta weights."""
        return self._eval(h, False, True)[2]

    def features(self, sin=False):
        """phi (n, N) of the last evaluation (and S = c sin f of the last gradient one)."""
        phi = np.empty((self.n, self.N), order="F")
        S = np.empty((self.n, self.N), order="F") if sin else None
        check(lib().gpt_nlml_features(self._h, _ptr(phi), _ptr(S) if sin else None))
        return (phi, S) if sin else phi

    def predict(self, h, Xtest, ytest=None, chunk=None):
        """The closed-form predictive of the model at ``h``: GPkit's named tuple (ymu, ys2, fmu,
        fs2, lp) for ``Xtest`` (Ntest, D), as ``ExactGP.predict`` returns it; lp is None without
        ``ytest``.  With l = theta_mean(h) and A = L L': fmu = phi*'l and fs2 = signal_var
        colsum((L^-1 phi*)^2), a sum of squares.  The factor of the last evaluation is reused when
        ``h`` equals its hyper-parameters bit for bit.  ``chunk`` test rows go through the device
        at a time (None: the library's choice); the results do not depend on it."""
        return self._predict(h, Xtest, ytest, chunk)

    def draw_theta(self, h, S, seed=0, z=None, return_z=False):
        """``S`` exact draws from the posterior theta | y ~ N(l, signal_var A^-1) at ``h``:
        (n, S) = l + sqrt(signal_var) L^-T z, the layout of a GPNT_SGLD store, so it goes straight
        to GPNT_pred, GPNT_predictive and their ``_x`` forms.  ``z`` (n, S) replaces the Philox
        normals (stream 25, kind 2); column s depends on column s of the normals only."""
        h = _hvec(h)
        S = int(S)
        z = _draw_z(z, self.n, S)
        theta = np.empty((self.n, max(S, 0)), order="F")
        zout = np.empty_like(theta) if return_z else None
        check(lib().gpt_nlml_draw_theta(self._h, _ptr(h), h.size, S, int(seed) & (2 ** 64 - 1),
                                        _ptr(z) if z is not None else None, _ptr(theta),
                                        _ptr(zout) if return_z else None))
        return (theta, zout) if return_z else theta


def _draw_z(z, M, S):
    """The injected normals of a draw call as (M, S) column-major, or None."""
    if z is None:
        return None
    z = _f64(z)
    if z.ndim == 1:
        z = _f64(z.reshape((-1, 1)))
    if z.shape != (M, S):
        raise GPTError(GPT_ERR_BAD_DIMS, "z must be (%d, S = %d)" % (M, S))
    return z


def _gpnt_feature_args(X, Z, b):
    X, Z = _f64(X), _f64(Z)
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    if X.ndim != 2 or Z.ndim != 2 or Z.shape[1] != X.shape[1] or b.size != Z.shape[0]:
        raise _bad_dims("X must be (N, D), Z (n, D) and b of length n")
    return X, Z, b


def gpnt_predict_oneshot(X, y, Z, b, hyperparams, Xtest, ytest=None):
    """The one-shot host-pointer prediction the Julia shim binds (gpt_gpnt_predict)."""
    X, Z, b = _gpnt_feature_args(X, Z, b)
    N, D = X.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise _bad_dims("y must have length N")
    Xtest, yt = _gpnt_test_args(Xtest, ytest, D)
    return _predict_call(lib().gpt_gpnt_predict,
                         [_ptr(X), N, D, _ptr(y), _ptr(Z), _ptr(b), Z.shape[0]],
                         _hvec(hyperparams), Xtest, yt)


def rff_kernel_error(X, Z, b, hyperparams):
    """How far the n random features are from the kernel they approximate
    (PowerPlantDataExperiment.jl:47-97): with K the exact squared-exponential kernel matrix of
    ``X`` (N, D) at ``hyperparams`` (ExactGP's covariance, no noise term; signal_var is validated
    and unused) and K_rff = phi'phi, phi = featureNotensor(X, l, sigma_RBF, Z, b), the named tuple
    (frob = |K - K_rff|_F, the reference's FrobError; norm_K = |K|_F; max_abs = max|K - K_rff|)
    over all N^2 entries.  Neither matrix is stored.  n <= 8192, N <= 65536, D <= 16 and
    8 n N <= 2 GiB."""
    X, Z, b = _gpnt_feature_args(X, Z, b)
    N, D = X.shape
    h = _hvec(hyperparams)
    out = np.empty(3)
    check(lib().gpt_rff_kernel_error(_ptr(X), N, D, _ptr(Z), _ptr(b), Z.shape[0], _ptr(h), h.size,
                                     _ptr(out)))
    return RFFKernelError(*out.tolist())


def rff_last_timing():
    """Device-event times in ms of the last calls: rff_kernel_error's features and its tile pass,
    and the chunks of NoTensorMarginal.predict."""
    ms = np.zeros(3)
    check(lib().gpt_rff_last_timing(_ptr(ms), 3))
    return ms


def _marginal(obj, what):
    if not isinstance(obj, NoTensorMarginal):
        raise TypeError("%s must be a NoTensorMarginal (it stands for the reference's closure over "
                        "featureNotensor / gradfeatureNotensor)" % what)
    return obj


def GPNT_nlogmarginal(y, n, hyperparams, randfeature):
    """GPT_SGLD.jl:921-933 with ``randfeature`` a NoTensorMarginal (which holds y and n)."""
    return _marginal(randfeature, "randfeature").nlogmarginal(hyperparams)


def GPNT_gradnlogmarginal(y, n, hyperparams, randfeature, gradfeature):
    """GPT_SGLD.jl:939-962 with ``randfeature`` and ``gradfeature`` the same NoTensorMarginal."""
    _marginal(gradfeature, "gradfeature")
    return _marginal(randfeature, "randfeature").gradnlogmarginal(hyperparams)


def gpnt_nlogmarginal_oneshot(X, y, Z, b, hyperparams, want_grad=True):
    """The one-shot host-pointer entry the Julia shim binds (gpt_gpnt_nlogmarginal)."""
    X = _f64(X)
    N, D = X.shape
    Z = _f64(Z)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    h = _hvec(hyperparams)
    val = C.c_double()
    grad = np.empty(h.size)
    check(lib().gpt_gpnt_nlogmarginal(_ptr(X), N, D, _ptr(y), _ptr(Z), _ptr(b), Z.shape[0], _ptr(h),
                                      h.size, 1 if want_grad else 0, C.byref(val), _ptr(grad)))
    return (val.value, grad) if want_grad else val.value


# ------------------------------------------------------------------ exact GP regression
class ExactGP(_Marginal):
    """Device-resident exact GP regression: squared-exponential kernel (iso or ARD), Gaussian
    noise, zero mean — GP_nlogmarginal (GPT_SGLD.jl:905-915) and GPkit's InfExact / prediction
    with CovSEiso or CovSEard and LikGauss, the reference's quality ceiling.

    ``X`` (N, D) and ``y`` (N) are uploaded once; every method takes
    ``h = [length_scale (D entries, or one: the iso form); sigma_RBF; signal_var]``, the vector of
    NoTensorMarginal.  N <= 16384, D <= 16.  A failed Cholesky raises ``GPTError``
    (GPT_ERR_NOT_SPD) and leaves the object usable.

    ``nlogmarginal`` and ``gradnlogmarginal`` are the callables ``GPNT_hyperparameters`` and
    ``GPNT_hyperparameters_optim`` take (the counterpart of GPkit's ``optinf``):
    ``GPNT_hyperparameters(gp.nlogmarginal, gp.gradnlogmarginal, init, lbounds)``.  GPkit's
    ``dnlZ`` (with respect to log l, log sigma_RBF, log sqrt(signal_var)) is the gradient times
    ``[l..., sigma_RBF, 2 signal_var]``."""
    _destroy, _eval_entry, _predict_entry = "gpt_egp_destroy", "gpt_egp_eval", "gpt_egp_predict"
    _test_args = staticmethod(_gp_test_args)

    def __init__(self, X, y):
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError("X must be (N, D)")
        N, D = X.shape
        y = _f64(np.asarray(y, dtype=np.float64).ravel())
        if y.size != N:
            raise ValueError("y must have length N")
        self.N, self.D = N, D
        self._nextra = N
        self._h = C.c_void_p()
        check(lib().gpt_egp_create(_ptr(X), N, D, _ptr(y), C.byref(self._h)))

    def alpha(self, h):
        """(K + signal_var I)^-1 y at h."""
        return self._eval(h, False, True)[2]

    def predict(self, h, Xtest, ytest=None, chunk=None):
        """GPkit's ``prediction``: the named tuple (ymu, ys2, fmu, fs2, lp) for ``Xtest``
        (Ntest, D); lp is None without ``ytest``.  The factor of the last evaluation is reused
        when ``h`` equals its hyper-parameters bit for bit.  ``chunk`` test rows go through the
        device at a time (None: the library's choice); the results do not depend on it."""
        return self._predict(h, Xtest, ytest, chunk)

    def draw_prior(self, h, S=1, seed=0, jitter=1e-6, z=None, return_z=False):
        """GPrand (GaussianProcess.jl:66-80) at the object's X: (N, S) = R'z with R = chol(K +
        jitter I); signal_var in ``h`` is not used.  ``z`` (N, S) replaces the Philox normals
        (stream 25, kind 0).  The next ``predict`` refits."""
        h = _hvec(h)
        S = int(S)
        z = _draw_z(z, self.N, S)
        F = np.empty((self.N, max(S, 0)), order="F")
        zout = np.empty_like(F) if return_z else None
        check(lib().gpt_egp_draw_prior(self._h, _ptr(h), h.size, float(jitter), S,
                                       int(seed) & (2 ** 64 - 1),
                                       _ptr(z) if z is not None else None, _ptr(F),
                                       _ptr(zout) if return_z else None))
        return (F, zout) if return_z else F

    def _posterior(self, h, Xtest, S, seed, jitter, observed, z, want_f, want_cov, want_z):
        h = _hvec(h)
        Xtest, _ = _gp_test_args(Xtest, None, self.D)
        Nt, S = Xtest.shape[0], int(S)
        z = _draw_z(z, Nt, S) if want_f else None
        fmu = np.empty(Nt)
        F = np.empty((Nt, max(S, 0)), order="F") if want_f else None
        cov = np.empty((Nt, Nt), order="F") if want_cov else None
        zout = np.empty_like(F) if want_f and want_z else None
        check(lib().gpt_egp_draw_posterior(
            self._h, _ptr(h), h.size, _ptr(Xtest), Nt, float(jitter), 1 if observed else 0, S,
            int(seed) & (2 ** 64 - 1), _ptr(z) if z is not None else None, _ptr(fmu),
            _ptr(F) if F is not None else None, _ptr(cov) if cov is not None else None,
            _ptr(zout) if zout is not None else None))
        return GPPosteriorDraw(fmu, F, cov, zout)

    def draw_posterior(self, h, Xtest, S=1, seed=0, jitter=1e-6, observed=False, z=None,
                       return_cov=False, return_z=False):
        """GPpost then GPrand (GaussianProcess.jl:82-122): ``S`` joint draws of the posterior GP
        at ``Xtest`` (Ntest <= 8192, D).  Returns (fmu, samples (Ntest, S), cov, z): fmu is
        ``predict``'s bit for bit, samples = fmu + L z with L L' = cov + jitter I (``observed``:
        + signal_var I, draws of observations), cov the joint covariance without either (None
        unless ``return_cov``).  ``z`` (Ntest, S) replaces the Philox normals (stream 25, kind 1)."""
        return self._posterior(h, Xtest, S, seed, jitter, observed, z, True, return_cov, return_z)

    def predict_cov(self, h, Xtest):
        """The joint predictive covariance k(x,x') - k(x)'(K + signal_var I)^-1 k(x') of the
        function values at ``Xtest``, (Ntest, Ntest); its diagonal is ``predict``'s fs2."""
        return self._posterior(h, Xtest, 0, 0, 0.0, False, None, False, True, False).cov


def _gp_hyper(signal_var, sigma_RBF2, length_scale):
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64)).ravel()
    return _f64(np.concatenate([ls, [math.sqrt(sigma_RBF2), signal_var]]))


def gp_nlogmarginal_oneshot(X, y, hyperparams, want_grad=True):
    """The one-shot host-pointer entry the Julia shim binds (gpt_gp_nlogmarginal)."""
    X = _f64(X)
    N, D = X.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    h = _hvec(hyperparams)
    val = C.c_double()
    grad = np.empty(h.size)
    check(lib().gpt_gp_nlogmarginal(_ptr(X), N, D, _ptr(y), _ptr(h), h.size,
                                    1 if want_grad else 0, C.byref(val), _ptr(grad)))
    return (val.value, grad) if want_grad else val.value


def gp_predict_oneshot(X, y, hyperparams, Xtest, ytest=None):
    """The one-shot host-pointer prediction the Julia shim binds (gpt_gp_predict)."""
    X, Xtest = _f64(X), _f64(Xtest)
    N, D = X.shape
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    yt = _f64(np.asarray(ytest, dtype=np.float64).ravel()) if ytest is not None else None
    return _predict_call(lib().gpt_gp_predict, [_ptr(X), N, D, _ptr(y)], _hvec(hyperparams), Xtest,
                         yt)


def gp_posterior_draw_oneshot(X, y, hyperparams, Xtest, S=1, seed=0, jitter=1e-6, observed=False,
                              z=None, return_cov=False):
    """The one-shot host-pointer posterior draw the Julia shim binds (gpt_gp_post_rand): what
    ExactGP(X, y).draw_posterior returns, bit for bit."""
    X, Xtest = _f64(X), _f64(Xtest)
    if X.ndim != 2 or Xtest.ndim != 2 or Xtest.shape[1] != X.shape[1]:
        raise _bad_dims("X must be (N, D) and Xtest (Ntest, D)")
    N, D = X.shape
    Nt, S = Xtest.shape[0], int(S)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise _bad_dims("y must have length N")
    h = _hvec(hyperparams)
    z = _draw_z(z, Nt, S)
    fmu = np.empty(Nt)
    F = np.empty((Nt, max(S, 0)), order="F")
    cov = np.empty((Nt, Nt), order="F") if return_cov else None
    check(lib().gpt_gp_post_rand(_ptr(X), N, D, _ptr(y), _ptr(h), h.size, _ptr(Xtest), Nt,
                                 float(jitter), 1 if observed else 0, S, int(seed) & (2 ** 64 - 1),
                                 _ptr(z) if z is not None else None, _ptr(fmu), _ptr(F),
                                 _ptr(cov) if return_cov else None))
    return GPPosteriorDraw(fmu, F, cov, None)


def gpnt_draw_theta_oneshot(X, y, Z, b, hyperparams, S, seed=0, z=None):
    """The one-shot host-pointer theta draw the Julia shim binds (gpt_gpnt_draw_theta): what
    NoTensorMarginal(X, y, Z, b).draw_theta returns, bit for bit."""
    X, Z, b = _gpnt_feature_args(X, Z, b)
    N, D = X.shape
    n, S = Z.shape[0], int(S)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    if y.size != N:
        raise _bad_dims("y must have length N")
    h = _hvec(hyperparams)
    z = _draw_z(z, n, S)
    theta = np.empty((n, max(S, 0)), order="F")
    check(lib().gpt_gpnt_draw_theta(_ptr(X), N, D, _ptr(y), _ptr(Z), _ptr(b), n, _ptr(h), h.size, S,
                                    int(seed) & (2 ** 64 - 1), _ptr(z) if z is not None else None,
                                    _ptr(theta)))
    return theta


def GPrand(X, length_scale, sigma_RBF, S=1, seed=0, jitter=1e-6):
    """GPrand (GaussianProcess.jl:66-80) of the zero-mean squared-exponential GP at ``X`` (N, D):
    (N, S) draws R'z, R = chol(K + jitter I), from Philox stream 25 (gpt_gp_rand).
    ``length_scale`` is a scalar or D entries."""
    X = _f64(X)
    if X.ndim != 2:
        raise ValueError("X must be (N, D)")
    N, D = X.shape
    h = _gp_hyper(1.0, float(sigma_RBF) ** 2, length_scale)
    h[-2] = float(sigma_RBF)
    S = int(S)
    F = np.empty((N, max(S, 0)), order="F")
    check(lib().gpt_gp_rand(_ptr(X), N, D, _ptr(h), h.size, float(jitter), S,
                            int(seed) & (2 ** 64 - 1), _ptr(F)))
    return F


def createmesh(interval_start, interval_end, npts):
    """GPT_SGLD.jl:289-301: ``(x, y, grid)`` with x = y = linspace(start, end, npts) and grid
    (npts^2, 2) whose row i*npts + j is (x[i], y[j])."""
    x = np.linspace(interval_start, interval_end, int(npts))
    y = np.linspace(interval_start, interval_end, int(npts))
    grid = np.empty((int(npts) ** 2, 2), order="F")
    grid[:, 0] = np.repeat(x, int(npts))
    grid[:, 1] = np.tile(y, int(npts))
    return x, y, grid


def fhatdraw(X, n, length_scale, sigma_RBF, r, Q, seed=0):
    """GPT_SGLD.jl:304-342: a draw ``(y, w, U, I, phi)`` from the tensor model at ``X`` (N, D):
    phi = feature(X, length_scale, sigma_RBF, sqrt(n/Q^(1/D)), Z, b) with Z, b =
    feature_inputs(n, D, seed), w ~ N(0, I) and U uniform on the Stiefel manifolds (init_state),
    I = samplenz(r, D, Q, seed), y = pred(w, U, I, phi).  ``length_scale`` is a scalar or D
    entries; any other length is the reference's error."""
    X = _f64(X)
    if X.ndim != 2:
        raise ValueError("X must be (N, D)")
    D = X.shape[1]
    if np.ndim(length_scale) > 0 and np.size(length_scale) != D:
        raise ValueError("dimensions of X and length_scale do not match")
    n, r, Q = int(n), int(r), int(Q)
    phi_scale = math.sqrt(n / Q ** (1.0 / D))
    Z, b = feature_inputs(n, D, seed)
    phi = _feature_D(X, length_scale, sigma_RBF, phi_scale, Z, b)
    w, U = init_state(n, r, D, Q, seed, stiefel=True, sigma_w=1.0)
    I = samplenz(r, D, Q, seed)
    return pred(w, U, I, phi), w, U, I, phi


def GP_nlogmarginal(X, y, signal_var, sigma_RBF2, length_scale):
    """GPT_SGLD.jl:905-915: the exact GP's negative log marginal likelihood; ``sigma_RBF2`` is
    sigma_RBF squared, ``length_scale`` a scalar or D entries.  It does not print."""
    return gp_nlogmarginal_oneshot(X, y, _gp_hyper(signal_var, sigma_RBF2, length_scale),
                                   want_grad=False)


def _log_space_minimize(nlogmarginal, gradnlogmarginal, init_hyperparams, bounds, xtol, ftol):
    from scipy.optimize import minimize

    def fun(lh):
        h = np.exp(lh)
        return float(nlogmarginal(h)), np.asarray(gradnlogmarginal(h), dtype=np.float64) * h
    x0 = np.log(np.asarray(init_hyperparams, dtype=np.float64))
    # ftol is a relative decrease of the objective as in the reference's optimisers; xtol has no
    # L-BFGS-B counterpart and bounds the projected gradient instead
    res = minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=bounds,
                   options={"ftol": float(ftol), "gtol": float(xtol), "maxiter": 200})
    return np.exp(res.x), float(res.fun)


def GPNT_hyperparameters(nlogmarginal, gradnlogmarginal, init_hyperparams, lbounds, xtol=1e-4,
                         ftol=1e-3):
    """GPT_SGLD.jl:971-989: minimise ``nlogmarginal`` over positive hyper-parameters bounded below
    by ``lbounds`` (a scalar or one per entry).  Returns ``(minx, minf)``.

    The optimiser differs from the reference's: NLopt's ``:LD_MMA`` is replaced by
    ``scipy.optimize.minimize(method="L-BFGS-B")`` over log-hyper-parameters with the chain-rule
    gradient ``g·h`` (as :992-993) and the bounds taken to log space, so iterates and stopping
    point are not the reference's.  Only the objective and its gradient are parity-tested."""
    init = np.asarray(init_hyperparams, dtype=np.float64)
    lb = np.broadcast_to(np.asarray(lbounds, dtype=np.float64), init.shape)
    if (lb <= 0).any() or (init < lb).any():
        raise ValueError("lbounds must be positive and below init_hyperparams")
    return _log_space_minimize(nlogmarginal, gradnlogmarginal, init,
                               [(math.log(v), None) for v in lb], xtol, ftol)


def GPNT_hyperparameters_optim(nlogmarginal, gradnlogmarginal, init_hyperparams, xtol=1e-4,
                               ftol=1e-3):
    """GPT_SGLD.jl:991-1002: the unconstrained form over log-hyper-parameters.  Returns
    ``(minx, minf)``.  Optim.jl's ``:cg`` is replaced by L-BFGS-B without bounds (see
    GPNT_hyperparameters); only the objective and its gradient are parity-tested."""
    return _log_space_minimize(nlogmarginal, gradnlogmarginal, init_hyperparams, None, xtol, ftol)


# ------------------------------------------------------------------ softmax classifier: hyper-parameters
class HMCResult:
    """Result of ``SoftmaxJoint.hmc`` / ``mala``: ``theta_store`` (n, C, nsamples // thin), the
    layout GPNT_pred_class takes; per transition, burn-in included, ``accept`` (int32, 0 / 1),
    ``dH`` = H0 - H1 and ``value`` = U of the kept state; ``accept_rate`` their mean acceptance
    and ``ndivergent`` the transitions rejected because H1 was not finite."""
    __slots__ = ("theta_store", "accept", "dH", "value", "accept_rate", "ndivergent")

    def __repr__(self):
        return "HMCResult(T=%d, transitions=%d, accept_rate=%.3f, ndivergent=%d)" % (
            self.theta_store.shape[2], self.accept.size, self.accept_rate, self.ndivergent)


class SoftmaxJoint(_Handle):
    """Device-resident joint likelihood -log p(y, theta; h) of the full-theta softmax classifier
    and its gradient (neglogjointlkhd / gradneglogjointlkhd, ImageExperiment.jl:135-204, with
    featureNotensor / gradfeatureNotensor at ``Z``, ``b`` in place of the seed).

    ``X`` (N, D), ``y`` (N, integers 1..C), ``Z`` (n, D), ``b`` (n) are uploaded once; ``C``
    defaults to max(y) - min(y) + 1 (GPT_SGLD.jl:854) and may be passed when a class is absent.
    Every method takes ``h = [length_scale (D entries, or one: the scalar form); sigma_RBF]``.
    theta (n, C) is resident on the device: a ``theta_vec`` argument (length n*C, column-major,
    or an (n, C) array) is uploaded and becomes the resident theta, ``None`` means the resident
    one.  n <= 1024, D <= 16, C <= 32.  Nothing of size n*N*D, or n*N, is stored."""
    _destroy = "gpt_cjoint_destroy"

    def __init__(self, X, y, Z, b, C=None):
        X = _f64(X)
        if X.ndim != 2:
            raise ValueError("X must be (N, D)")
        N, D = X.shape
        Z = _f64(Z)
        n = Z.shape[0]
        y = _f64(np.asarray(y, dtype=np.float64).ravel())
        b = _f64(np.asarray(b, dtype=np.float64).ravel())
        if Z.shape != (n, D) or b.size != n or y.size != N:
            raise ValueError("Z must be (n, D), b of length n and y of length N")
        if C is None:
            C = int(y.max() - y.min() + 1)
        self.n, self.N, self.D, self.C = n, N, D, int(C)
        self._h = _lib.C.c_void_p()
        check(lib().gpt_cjoint_create(_ptr(X), N, D, _ptr(y), self.C, _ptr(Z), _ptr(b), n,
                                      _lib.C.byref(self._h)))

    def _theta_arg(self, theta):
        if theta is None:
            return None
        t = np.asarray(theta, dtype=np.float64)
        if t.size != self.n * self.C or (t.ndim == 2 and t.shape != (self.n, self.C)):
            raise ValueError("theta must have n*C entries")
        return _f64(t.reshape((self.n, self.C), order="F"))

    def _eval(self, theta, h, want_grad, want_theta_grad=True):
        h = _hvec(h)
        th = self._theta_arg(theta)
        val = _lib.C.c_double()
        nC = self.n * self.C
        grad = np.empty(nC + h.size) if want_grad else None
        gth = _ptr(grad) if want_grad and want_theta_grad else None
        gh = _ptr(grad[nC:]) if want_grad else None
        check(lib().gpt_cjoint_eval(self._h, _ptr(h), h.size, _ptr(th) if th is not None else None,
                                    1 if want_grad else 0, _lib.C.byref(val), gth, gh))
        return val.value, grad

    def neglogjointlkhd(self, theta_vec, h):
        return self._eval(theta_vec, h, False)[0]

    def gradneglogjointlkhd(self, theta_vec, h):
        """[vec(grad theta); grad length_scale; grad sigma_RBF], n*C + len(h) entries."""
        return self._eval(theta_vec, h, True)[1]

    def value_and_grad(self, theta_vec, h):
        return self._eval(theta_vec, h, True)

    def hyper_value_and_grad(self, h):
        """Value and the gradient with respect to h alone at the resident theta (the M step)."""
        val, grad = self._eval(None, h, True, want_theta_grad=False)
        return val, grad[self.n * self.C:]

    def theta(self):
        out = np.empty((self.n, self.C), order="F")
        check(lib().gpt_cjoint_get_theta(self._h, _ptr(out)))
        return out

    def set_theta(self, theta):
        check(lib().gpt_cjoint_set_theta(self._h, _ptr(self._theta_arg(theta))))

    @property
    def steps(self):
        """0-based counter of the next Langevin step."""
        t = _lib.C.c_int64()
        check(lib().gpt_cjoint_steps(self._h, _lib.C.byref(t)))
        return t.value

    def langevin(self, h, eps, nsteps, seed, t0=None):
        """``nsteps`` Langevin steps on the resident theta at ``h`` (GPT_SGLD.jl:1031-1033),
        theta <- theta - (eps/2 grad + sqrt(eps) xi), with no host round trip; the noise of
        0-based step t and class c is normals(n, seed, t, THETA_NOISE, c).  ``t0`` sets the step
        counter first (None: it continues).  A non-finite theta raises GPTError
        (GPT_ERR_NAN_THETA) and the remaining steps are not taken."""
        h = _hvec(h)
        check(lib().gpt_cjoint_langevin(self._h, _ptr(h), h.size, float(eps), int(nsteps),
                                        int(seed), -1 if t0 is None else int(t0)))

    def hmc(self, h, eps, L, nsamples, seed, burnin=0, thin=1, t0=None):
        """``burnin + nsamples`` Hamiltonian Monte Carlo transitions on the resident theta at
        ``h`` with no host round trip: ``L`` leapfrog steps of size sqrt(``eps``) (``eps`` is the
        reference's squared step) and a Metropolis test on H = U + |p|^2/2, U the joint
        likelihood with its |theta|^2/2 prior.  The momentum of 0-based transition t and class c
        is normals(n, seed, t, 26, c) and the uniform of its test uniform(seed, t, 27, 0); the
        counter is the one ``langevin`` uses (``t0`` sets it first, None continues).  Returns an
        HMCResult.  A transition whose end Hamiltonian is not finite is rejected and counted in
        ``ndivergent``; a non-finite starting theta raises GPTError (GPT_ERR_NAN_THETA)."""
        h = _hvec(h)
        burnin, nsamples, thin = int(burnin), int(nsamples), int(thin)
        ntrans = max(burnin, 0) + max(nsamples, 0)
        ncols = max(nsamples, 0) // thin if thin >= 1 else 0
        res = HMCResult()
        res.theta_store = np.empty((self.n, self.C, ncols), order="F")
        res.accept = np.empty(ntrans, dtype=np.int32)
        res.dH, res.value = np.empty(ntrans), np.empty(ntrans)
        ndiv = _lib.C.c_int64()
        check(lib().gpt_chmc_run(self._h, _ptr(h), h.size, float(eps), int(L), burnin, nsamples,
                                   thin, int(seed), -1 if t0 is None else int(t0),
                                   _ptr(res.theta_store), _ptr(res.accept, P_I32), _ptr(res.dH),
                                   _ptr(res.value), _lib.C.byref(ndiv)))
        res.ndivergent = ndiv.value
        res.accept_rate = float(res.accept.mean()) if ntrans else float("nan")
        return res

    def mala(self, h, eps, nsamples, seed, burnin=0, thin=1, t0=None):
        """``hmc`` with one leapfrog step: the full-batch MALA loop of
        BloodTransfusionExperiment.jl:255-278."""
        return self.hmc(h, eps, 1, nsamples, seed, burnin=burnin, thin=thin, t0=t0)

    def leapfrog(self, h, eps, L, p):
        """The integrator alone: ``L`` leapfrog steps of size sqrt(``eps``) from the resident theta
        (left unchanged) on the momentum ``p`` (n, C).  Returns ``(q, p_new, H0, H1)``."""
        h = _hvec(h)
        pn = np.array(self._theta_arg(p), dtype=np.float64, order="F", copy=True)
        q = np.empty((self.n, self.C), order="F")
        H = np.empty(2)
        check(lib().gpt_chmc_leapfrog(self._h, _ptr(h), h.size, float(eps), int(L), _ptr(pn),
                                        _ptr(q), _ptr(H)))
        return q, pn, float(H[0]), float(H[1])

    def _xtest(self, Xtest):
        return _gp_test_args(Xtest, None, self.D)[0]

    def scores(self, h, Xtest):
        """featureNotensor(Xtest)' theta at ``h``: (Ntest, C)."""
        h = _hvec(h)
        Xtest = self._xtest(Xtest)
        out = np.empty((Xtest.shape[0], self.C), order="F")
        check(lib().gpt_cjoint_scores(self._h, _ptr(h), h.size, _ptr(Xtest), Xtest.shape[0],
                                      _ptr(out)))
        return out

    def evaluate(self, h, Xtest, ytest):
        """The prop_missed / mean_nlp line of the reference's loop (ImageExperiment.jl:258-268) as
        a ClassEval of one sample; the scores never leave the device before they are evaluated."""
        h = _hvec(h)
        Xtest = self._xtest(Xtest)
        Nt = Xtest.shape[0]
        yi = _labels(ytest, Nt)
        res = ClassEval()
        res.prop_missed, res.mean_nlp, avg = np.empty(1), np.empty(1), np.empty(2)
        res.mean_fhat = np.empty((Nt, self.C), order="F")
        res.prediction = np.empty(Nt, dtype=np.int32)
        res.nlp = np.empty(Nt)
        res.scores = np.empty((Nt, self.C, 1), order="F")
        check(lib().gpt_cjoint_class_eval(self._h, _ptr(h), h.size, _ptr(Xtest), _ptr(yi, P_I32), Nt,
                                          _ptr(res.prop_missed), _ptr(res.mean_nlp), _ptr(avg),
                                          _ptr(res.mean_fhat), _ptr(res.prediction, P_I32),
                                          _ptr(res.nlp), _ptr(res.scores)))
        res.avg_prop_missed, res.avg_mean_nlp = float(avg[0]), float(avg[1])
        res.window = (0, 1)
        return res


def gpnt_neglogjoint_oneshot(X, y, Z, b, theta, hyperparams, C=None, want_grad=True):
    """The one-shot host-pointer entry the Julia shim binds (gpt_gpnt_neglogjoint)."""
    X = _f64(X)
    N, D = X.shape
    Z = _f64(Z)
    n = Z.shape[0]
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    if C is None:
        C = int(y.max() - y.min() + 1)
    th = _f64(np.asarray(theta, dtype=np.float64).reshape((n, C), order="F"))
    h = _hvec(hyperparams)
    val = _lib.C.c_double()
    grad = np.empty(n * C + h.size)
    check(lib().gpt_gpnt_neglogjoint(_ptr(X), N, D, _ptr(y), C, _ptr(Z), _ptr(b), n, _ptr(th),
                                     _ptr(h), h.size, 1 if want_grad else 0, _lib.C.byref(val),
                                     _ptr(grad)))
    return (val.value, grad) if want_grad else val.value


def gpnt_joint_hmc_oneshot(X, y, Z, b, theta, hyperparams, eps, L, nsamples, seed, burnin=0, thin=1,
                           t0=0, C=None):
    """The one-shot host-pointer entry the Julia shim binds (gpt_gpnt_joint_hmc): create, run,
    destroy.  Returns ``(theta (n, C) after the run, HMCResult)``."""
    X = _f64(X)
    N, D = X.shape
    Z = _f64(Z)
    n = Z.shape[0]
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    b = _f64(np.asarray(b, dtype=np.float64).ravel())
    if C is None:
        C = int(y.max() - y.min() + 1)
    th = np.array(np.asarray(theta, dtype=np.float64).reshape((n, C), order="F"), order="F", copy=True)
    h = _hvec(hyperparams)
    burnin, nsamples, thin = int(burnin), int(nsamples), int(thin)
    ntrans = max(burnin, 0) + max(nsamples, 0)
    res = HMCResult()
    res.theta_store = np.empty((n, C, max(nsamples, 0) // thin if thin >= 1 else 0), order="F")
    res.accept = np.empty(ntrans, dtype=np.int32)
    res.dH, res.value = np.empty(ntrans), np.empty(ntrans)
    ndiv = _lib.C.c_int32()
    check(lib().gpt_gpnt_joint_hmc(_ptr(X), N, D, _ptr(y), C, _ptr(Z), _ptr(b), n, _ptr(th), _ptr(h),
                                   h.size, float(eps), int(L), burnin, nsamples, thin, int(seed),
                                   int(t0), _ptr(res.theta_store), _ptr(res.accept, P_I32),
                                   _ptr(res.dH), _ptr(res.value), _lib.C.byref(ndiv)))
    res.ndivergent = ndiv.value
    res.accept_rate = float(res.accept.mean()) if ntrans else float("nan")
    return th, res


def _joint(fn, what):
    obj = getattr(fn, "__self__", None)
    if not isinstance(obj, SoftmaxJoint) or getattr(fn, "__name__", "") != what:
        raise TypeError("%s must be the %s method of a SoftmaxJoint (it stands for the reference's "
                        "closure over the training data and the features)" % (what, what))
    return obj


def GPNT_hyperparameters_ng(init_theta, init_hyperparams, neglogjointlkhd, gradneglogjointlkhd, Z=None,
                            b=None, epsilon=1e-2, num_sgld_iter=10, num_cg_iter=10, seed=0, tol=1e-7,
                            max_iter=200, trace=False, e_step="langevin", num_leapfrog=8):
    """GPT_SGLD.jl:1005-1063: stochastic EM on the non-Gaussian joint likelihood.  The two
    function arguments are the ``neglogjointlkhd`` and ``gradneglogjointlkhd`` methods of one
    SoftmaxJoint (which holds X, y, Z and b; ``Z`` and ``b`` are accepted for the reference's
    signature and not read).  Per round: ``num_sgld_iter`` Langevin steps of size ``epsilon`` on
    the resident theta (the step counter runs on from round to round, noise from ``seed``), then
    ``num_cg_iter`` iterations of conjugate gradients over the log-hyper-parameters with theta
    fixed and the chain-rule gradient ``grad .* exp(loghyper)`` (:1021).  It stops when
    ``norm(exp(old) - exp(new)) <= tol`` (:1052, 1e-7 there) or after ``max_iter`` rounds: the
    reference's loop has no cap, and a stochastic theta can keep it running for ever.

    ``e_step="hmc"`` replaces the round's Langevin steps by a Metropolis-corrected E step, as the
    reference's experiments run it (``mcmc(..., 10, burnin=9)``, ImageExperiment.jl:278-283):
    ``num_sgld_iter`` HMC transitions of ``num_leapfrog`` leapfrog steps at squared step
    ``epsilon`` (``SoftmaxJoint.hmc``), of which the last state is kept.

    Returns ``exp(loghyper)``; with ``trace=True`` also a list with, per round, the reference's
    printed ``(function_value_before, function_value_after, hyperparams)``.  theta stays resident
    (``SoftmaxJoint.theta()``).  Optim.jl's ``:cg`` is replaced by
    ``scipy.optimize.minimize(method="CG")``, so iterates are not the reference's; only the
    objective and its gradient are parity-tested."""
    from scipy.optimize import minimize

    if e_step not in ("langevin", "hmc"):
        raise ValueError('e_step must be "langevin" or "hmc"')
    joint = _joint(neglogjointlkhd, "neglogjointlkhd")
    if _joint(gradneglogjointlkhd, "gradneglogjointlkhd") is not joint:
        raise TypeError("neglogjointlkhd and gradneglogjointlkhd must belong to one SoftmaxJoint")
    joint.set_theta(init_theta)
    lh = np.log(np.asarray(init_hyperparams, dtype=np.float64).ravel())

    def fun(x):
        hx = np.exp(x)
        val, gh = joint.hyper_value_and_grad(hx)
        return val, gh * hx

    rounds = []
    t = 0
    for _ in range(int(max_iter)):
        if num_sgld_iter > 0:
            if e_step == "hmc":
                joint.hmc(np.exp(lh), epsilon, num_leapfrog, 1, seed, burnin=int(num_sgld_iter) - 1,
                          t0=t)
            else:
                joint.langevin(np.exp(lh), epsilon, num_sgld_iter, seed, t0=t)
            t += int(num_sgld_iter)
        res = minimize(fun, lh, jac=True, method="CG", options={"maxiter": int(num_cg_iter)})
        new = np.asarray(res.x, dtype=np.float64)
        if trace:
            rounds.append((joint.neglogjointlkhd(None, np.exp(lh)),
                           joint.neglogjointlkhd(None, np.exp(new)), np.exp(new)))
        absdiff = float(np.linalg.norm(np.exp(lh) - np.exp(new)))
        lh = new
        if absdiff <= tol:
            break
    return (np.exp(lh), rounds) if trace else np.exp(lh)
