"""MovieLens-100k tensor collaborative filtering (100k_movielensExperiment.jl, §8(f) item 1 /
BASELINE config 5) on libgptsgld.so.

    GPT_fullw_sideinfo        :409-551   SGD / SGLD, side information (the four SGD entries also
    GPT_fixw_sideinfo         :282-404   take U_init=, V_init=: the initial U and V in place of the
    GPT_fullw                 :160-279   Philox draw, for the tests' injected state)
    GPT_fixw                  :56-156
    GPT_fullw_gibbs           :1032-1129
    GPT_fixw_gibbs            :945-1028
    GPT_fullw_sideinfo_folds  :733-736   the folds loop as one device launch per epoch (a list of
                                         per-fold result tuples)
    fold(data, i)     the standardised u{i}.base / u{i}.test split of :566-576

Same arguments (the signatures below) and return tuple as the reference: (w_store, U_store, V_store,
testpred_store, trainRMSEvec, testRMSEvec), without w_store for the fixed-w variants.  ``data`` is the mapping written by
scripts/make_ml100k_fixture.py (ratings per fold, the processed UserData / MovieData of
:578-584).  Randomness follows the framework's Philox contract (oracle/movielens_ref.py).
"""
import ctypes as C

import numpy as np

from ._lib import P_D, check, lib
from . import _lib

__all__ = ["GPT_fullw_sideinfo", "GPT_fullw_sideinfo_folds", "GPT_fixw_sideinfo", "GPT_fullw", "GPT_fixw", "GPT_fullw_gibbs",
           "GPT_fixw_gibbs", "fold"]


def _f64(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return a.ctypes.data_as(P_D)


def _inject(U_init, V_init):
    """Hand U_init ((n1+D1) x r) and V_init ((n2+D2) x r) to the next CF SGD run of this thread
    (gpt_debug_cf_init: one shot, the run checks the dimensions); nothing when both are None."""
    if U_init is None and V_init is None:
        return
    if U_init is None or V_init is None:
        raise ValueError("U_init and V_init go together")
    U0, V0 = _f64(U_init), _f64(V_init)
    if U0.ndim != 2 or V0.ndim != 2 or U0.shape[1] != V0.shape[1]:
        raise ValueError("U_init is (n1 + D1) x r and V_init (n2 + D2) x r")
    check(lib().gpt_debug_cf_init(_ptr(U0), U0.shape[0], _ptr(V0), V0.shape[0], U0.shape[1]))


def fold(data, i):
    """(Ratingtrain, Ratingtest, UserData, MovieData, ytrainMean, ytrainStd) of fold i (1..5),
    ratings standardised with the training mean / std (:570-575)."""
    tr = np.asarray(data["u%d_base" % i], dtype=np.float64).copy()
    te = np.asarray(data["u%d_test" % i], dtype=np.float64).copy()
    mu, sd = tr[:, 2].mean(), tr[:, 2].std(ddof=1)
    tr[:, 2] = (tr[:, 2] - mu) / sd
    te[:, 2] = (te[:, 2] - mu) / sd
    return (tr, te, np.asarray(data["user_data"], dtype=np.float64),
            np.asarray(data["movie_data"], dtype=np.float64), mu, sd)


def _stores(r, rowsU, rowsV, Ntest, maxepoch, fixw=False):
    """The zeroed outputs of one fold (no w_store for the fixed-w variants)."""
    outs = [] if fixw else [np.zeros((r, r, maxepoch), order="F")]
    return outs + [np.zeros((rowsU, r, maxepoch), order="F"), np.zeros((rowsV, r, maxepoch), order="F"),
                   np.zeros((Ntest, maxepoch), order="F"), np.zeros(maxepoch), np.zeros(maxepoch)]


def _nan_or_check(code):
    if code == _lib.GPT_ERR_NAN_GEODESIC:
        print("Get NaN when moving along Geodesic. Try smaller epsU")
    else:
        check(code)


def _run(entry, Rating, UserData, MovieData, Ratingtest, w, hyper, steps, epochs, param_seed,
         ytrainMean, ytrainStd, flags, side=False, fixw=False, init=None):
    """One call of a single-fold C entry: conversions, shape check, output stores, seed mask and
    the arguments in the entries' common order -- ratings, side information (side: the arrays with
    their sizes, else n1 and n2), test ratings, hyper (floats), w and r, steps (m, then the
    floats), epochs (ints, maxepoch second), seed, ytrainMean, ytrainStd, flags (bools), outputs.
    init = (U_init, V_init): an SGD entry (the injected state; the geodesic NaN printed); None: Gibbs."""
    Rt, Rs, w0 = _f64(Rating), _f64(Ratingtest), _f64(w)
    r, N, Ntest = w0.shape[0], Rt.shape[0], Rs.shape[0]
    if Rt.shape[1] < 3 or Rs.shape[1] < 3 or w0.shape != (r, r):
        raise ValueError("Rating / Ratingtest need (user, movie, rating) columns; %s is r x r"
                         % ("w" if fixw else "w_init"))
    if side:
        Ud, Md = _f64(UserData), _f64(MovieData)
        (n1, D1), (n2, D2) = Ud.shape, Md.shape
        middle = (_ptr(Ud), n1, D1, _ptr(Md), n2, D2)
    else:
        n1, n2, D1, D2 = np.shape(UserData)[0], np.shape(MovieData)[0], 0, 0
        middle = (n1, n2)
    outs = _stores(r, n1 + D1, n2 + D2, Ntest, int(epochs[1]), fixw)
    if init is not None:
        _inject(*init)
    code = getattr(lib(), entry)(
        _ptr(Rt), N, N, *middle, _ptr(Rs), Ntest, Ntest, *map(float, hyper), _ptr(w0), r,
        *map(int, steps[:1]), *map(float, steps[1:]), *map(int, epochs),
        int(param_seed) & (2 ** 64 - 1), float(ytrainMean), float(ytrainStd),
        *(int(bool(f)) for f in flags), *map(_ptr, outs))
    (check if init is None else _nan_or_check)(code)
    return tuple(outs)


def GPT_fullw_sideinfo(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, sigma_w,
                       w_init, m, epsw, epsU, a, b, c, burnin, maxepoch, param_seed, ytrainMean,
                       ytrainStd, langevin=False, stiefel=False, avg=False, U_init=None, V_init=None):
    """U_init / V_init (tests): the initial U and V in place of the Philox draw."""
    return _run("gpt_cf_fullw_sideinfo", Rating, UserData, MovieData, Ratingtest, w_init,
                (signal_var, sigma_u, sigma_w), (m, epsw, epsU, a, b, c), (burnin, maxepoch),
                param_seed, ytrainMean, ytrainStd, (langevin, stiefel, avg), side=True,
                init=(U_init, V_init))


def GPT_fullw_gibbs(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, sigma_w, w_init,
                    burnin, maxepoch, n_samples, param_seed, ytrainMean, ytrainStd, avg=False,
                    rotated_w=False):
    return _run("gpt_cf_fullw_gibbs", Rating, UserData, MovieData, Ratingtest, w_init,
                (signal_var, sigma_u, sigma_w), (), (burnin, maxepoch, n_samples), param_seed,
                ytrainMean, ytrainStd, (avg, rotated_w))


def GPT_fixw_sideinfo(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, w, m, epsU,
                      a, b, c, burnin, maxepoch, param_seed, ytrainMean, ytrainStd,
                      langevin=False, stiefel=False, avg=False, U_init=None, V_init=None):
    """100k_movielensExperiment.jl:282-404 -> (U_store, V_store, testpred_store, trainRMSEvec,
    testRMSEvec)."""
    return _run("gpt_cf_fixw_sideinfo", Rating, UserData, MovieData, Ratingtest, w,
                (signal_var, sigma_u), (m, epsU, a, b, c), (burnin, maxepoch), param_seed, ytrainMean,
                ytrainStd, (langevin, stiefel, avg), side=True, fixw=True, init=(U_init, V_init))


def GPT_fullw(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, sigma_w, w_init, m,
              epsw, epsU, burnin, maxepoch, param_seed, ytrainMean, ytrainStd, langevin=False,
              stiefel=False, avg=False, U_init=None, V_init=None):
    """100k_movielensExperiment.jl:160-279 (no side information) -> (w_store, U_store, V_store,
    testpred_store, trainRMSEvec, testRMSEvec)."""
    return _run("gpt_cf_fullw", Rating, UserData, MovieData, Ratingtest, w_init,
                (signal_var, sigma_u, sigma_w), (m, epsw, epsU), (burnin, maxepoch), param_seed,
                ytrainMean, ytrainStd, (langevin, stiefel, avg), init=(U_init, V_init))


def GPT_fixw(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, w, m, epsU, burnin,
             maxepoch, param_seed, ytrainMean, ytrainStd, langevin=False, stiefel=False,
             avg=False, U_init=None, V_init=None):
    """100k_movielensExperiment.jl:56-156 (no side information, w fixed) -> (U_store, V_store,
    testpred_store, trainRMSEvec, testRMSEvec)."""
    return _run("gpt_cf_fixw", Rating, UserData, MovieData, Ratingtest, w, (signal_var, sigma_u),
                (m, epsU), (burnin, maxepoch), param_seed, ytrainMean, ytrainStd,
                (langevin, stiefel, avg), fixw=True, init=(U_init, V_init))


def GPT_fixw_gibbs(Rating, UserData, MovieData, Ratingtest, signal_var, sigma_u, w, burnin,
                   maxepoch, n_samples, param_seed, ytrainMean, ytrainStd, avg=False,
                   rotated_w=False):
    """100k_movielensExperiment.jl:945-1028 -> (U_store, V_store, testpred_store, trainRMSEvec,
    testRMSEvec)."""
    return _run("gpt_cf_fixw_gibbs", Rating, UserData, MovieData, Ratingtest, w,
                (signal_var, sigma_u), (), (burnin, maxepoch, n_samples), param_seed, ytrainMean,
                ytrainStd, (avg, rotated_w), fixw=True)


def last_timing():
    """Device time of the last CF SGD / SGLD call on this thread (gpt_cf_last_timing): dict with
    epoch_ms (cf_epoch_kernel launches), eval_ms (cf_eval_kernel), epochs, fold_steps and mode
    (gpt_cf_last_mode, the library's CfMode: 0 kCfStepPairs, batch-phase + move launches per step;
    1 kCfStiefelEpoch, one Stiefel epoch launch; 2 kCfLazyEpoch, one lazy SGD epoch launch)."""
    em, vm = C.c_double(), C.c_double()
    ne, fs = C.c_int64(), C.c_int64()
    check(lib().gpt_cf_last_timing(C.byref(em), C.byref(vm), C.byref(ne), C.byref(fs)))
    mode = C.c_int32()
    check(lib().gpt_cf_last_mode(C.byref(mode)))
    return dict(epoch_ms=em.value, eval_ms=vm.value, epochs=ne.value, fold_steps=fs.value,
                mode=mode.value)


def GPT_fullw_sideinfo_folds(Ratings, UserData, MovieData, Ratingtests, signal_var, sigma_u,
                             sigma_w, w_init, m, epsw, epsU, a, b, c, burnin, maxepoch, param_seed,
                             ytrainMeans, ytrainStds, langevin=False, stiefel=False, avg=False, *,
                             return_status=False):
    """The per-fold loop of 100k_movielensExperiment.jl:733-736 (GPT_fullw_sideinfo on fold i
    with its own ratings and ytrainMean[i] / ytrainStd[i], one param_seed) with the folds as
    sibling chains of one device launch per epoch.  Returns one (w_store, U_store, V_store,
    testpred_store, trainRMSEvec, testRMSEvec) tuple per fold — the same values as separate
    GPT_fullw_sideinfo calls; a fold that hit the geodesic NaN keeps zero parameter stores.
    return_status=True: (that list, the int32 status of each fold — 0 or GPT_ERR_NAN_GEODESIC)."""
    F = len(Ratings)
    if len(Ratingtests) != F or len(ytrainMeans) != F or len(ytrainStds) != F:
        raise ValueError("one test set, ytrainMean and ytrainStd per fold")
    Rts, Rss = [_f64(R) for R in Ratings], [_f64(R) for R in Ratingtests]
    Ud, Md, w0 = _f64(UserData), _f64(MovieData), _f64(w_init)
    (n1, D1), (n2, D2) = Ud.shape, Md.shape
    r = w0.shape[0]
    outs = [tuple(_stores(r, n1 + D1, n2 + D2, Rs.shape[0], maxepoch)) for Rs in Rss]
    PP = C.c_void_p * F
    ptrs = lambda arrs: PP(*[a.ctypes.data for a in arrs])
    Ns, Nts = (np.array([R.shape[0] for R in Rx], dtype=np.int64) for Rx in (Rts, Rss))
    ym, ys = (_f64(np.asarray(y, dtype=np.float64)) for y in (ytrainMeans, ytrainStds))
    st = np.zeros(F, dtype=np.int32)
    _nan_or_check(lib().gpt_cf_fullw_sideinfo_folds(
        F, ptrs(Rts), Ns.ctypes.data, ptrs(Rss), Nts.ctypes.data, _ptr(Ud), n1, D1, _ptr(Md), n2,
        D2, float(signal_var), float(sigma_u), float(sigma_w), _ptr(w0), r, int(m), float(epsw),
        float(epsU), float(a), float(b), float(c), int(burnin), int(maxepoch),
        int(param_seed) & (2 ** 64 - 1), _ptr(ym), _ptr(ys), int(bool(langevin)),
        int(bool(stiefel)), int(bool(avg)), *(ptrs([o[k] for o in outs]) for k in range(6)),
        st.ctypes.data_as(_lib.P_I32)))
    return (outs, st) if return_status else outs
