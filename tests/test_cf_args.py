"""CPU tests of the MovieLens CF boundary (gpt_cf_*, gpt_debug_cf_init): every bad argument fails
with GPT_ERR_BAD_DIMS and its own message before any device call."""
import ctypes as C

import numpy as np
import pytest

N, NT, N1, N2, D1, D2, R, E = 6, 4, 5, 4, 2, 3, 3, 2

# parameter names of each entry, in the order of include/gptsgld.h
SIDE = ["Rating", "N", "ldr", "UserData", "n1", "D1", "MovieData", "n2", "D2", "Ratingtest", "Ntest",
        "ldt"]
PLAIN = ["Rating", "N", "ldr", "n1", "n2", "Ratingtest", "Ntest", "ldt"]
RUN = ["burnin", "maxepoch", "seed", "ymean", "ystd", "langevin", "stiefel", "avg"]
GRUN = ["burnin", "maxepoch", "n_samples", "seed", "ymean", "ystd", "avg", "rotated_w"]
OUT = ["U_store", "V_store", "testpred_store", "trainRMSE", "testRMSE"]
ENTRIES = {
    "fullw_sideinfo": SIDE + ["signal_var", "sigma_u", "sigma_w", "w", "r", "m", "epsw", "epsU", "a",
                              "b", "c"] + RUN + ["w_store"] + OUT,
    "fixw_sideinfo": SIDE + ["signal_var", "sigma_u", "w", "r", "m", "epsU", "a", "b", "c"] + RUN + OUT,
    "fullw": PLAIN + ["signal_var", "sigma_u", "sigma_w", "w", "r", "m", "epsw", "epsU"] + RUN +
             ["w_store"] + OUT,
    "fixw": PLAIN + ["signal_var", "sigma_u", "w", "r", "m", "epsU"] + RUN + OUT,
    "fullw_gibbs": PLAIN + ["signal_var", "sigma_u", "sigma_w", "w", "r"] + GRUN + ["w_store"] + OUT,
    "fixw_gibbs": PLAIN + ["signal_var", "sigma_u", "w", "r"] + GRUN + OUT,
    "fullw_sideinfo_folds": ["F", "Ratings", "Ns", "Ratingtests", "Ntests", "UserData", "n1", "D1",
                             "MovieData", "n2", "D2", "signal_var", "sigma_u", "sigma_w", "w", "r",
                             "m", "epsw", "epsU", "a", "b", "c", "burnin", "maxepoch", "seed",
                             "ymeans", "ystds", "langevin", "stiefel", "avg", "w_stores", "U_stores",
                             "V_stores", "testpred_stores", "trainRMSEs", "testRMSEs", "status"],
}
NAMES = {k: "GPT_" + k for k in ENTRIES}
SGD = ["fullw_sideinfo", "fixw_sideinfo", "fullw", "fixw", "fullw_sideinfo_folds"]
GIBBS = ["fullw_gibbs", "fixw_gibbs"]
SINGLE = [e for e in ENTRIES if e != "fullw_sideinfo_folds"]
NF = 3                               # folds of the folds entry's valid call


def _ratings(rows, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.column_stack([rng.integers(1, N1 + 1, rows), rng.integers(1, N2 + 1, rows),
                                              rng.standard_normal(rows)]).astype(np.float64))


def _values():
    """A valid call's arguments by name; the arrays live as long as the dict."""
    rng = np.random.default_rng(3)
    v = dict(Rating=_ratings(N, 1), Ratingtest=_ratings(NT, 2), N=N, ldr=N, Ntest=NT, ldt=NT,
             UserData=np.asfortranarray((rng.random((N1, D1)) < 0.5).astype(np.float64)),
             MovieData=np.asfortranarray((rng.random((N2, D2)) < 0.5).astype(np.float64)),
             n1=N1, D1=D1, n2=N2, D2=D2, signal_var=0.8, sigma_u=0.1, sigma_w=1.0,
             w=np.asfortranarray(rng.standard_normal((R, R))), r=R, m=4, epsw=1e-4, epsU=1e-6,
             a=0.5, b=0.25, c=0.5, burnin=0, maxepoch=E, n_samples=1, seed=17, ymean=3.5, ystd=1.1,
             langevin=0, stiefel=0, avg=0, rotated_w=0, w_store=np.zeros(R * R * E),
             U_store=np.zeros((N1 + D1) * R * E), V_store=np.zeros((N2 + D2) * R * E),
             testpred_store=np.zeros(NT * E), trainRMSE=np.zeros(E), testRMSE=np.zeros(E), F=NF)
    # the folds entry: arrays of per-fold pointers / sizes
    v["_folds"] = dict(
        Ratings=[_ratings(N, 10 + f) for f in range(NF)],
        Ratingtests=[_ratings(NT, 20 + f) for f in range(NF)],
        w_stores=[np.zeros(R * R * E) for _ in range(NF)],
        U_stores=[np.zeros((N1 + D1) * R * E) for _ in range(NF)],
        V_stores=[np.zeros((N2 + D2) * R * E) for _ in range(NF)],
        testpred_stores=[np.zeros(NT * E) for _ in range(NF)],
        trainRMSEs=[np.zeros(E) for _ in range(NF)], testRMSEs=[np.zeros(E) for _ in range(NF)])
    v.update(Ns=np.full(NF, N, dtype=np.int64), Ntests=np.full(NF, NT, dtype=np.int64),
             ymeans=np.full(NF, 3.5), ystds=np.full(NF, 1.1), status=np.zeros(NF, dtype=np.int32))
    return v


def _arg(v, name):
    x = v[name] if name in v else v["_folds"][name]
    if x is None:
        return None
    if isinstance(x, list):            # per-fold arrays -> an array of their addresses
        v["_keep_" + name] = (C.c_void_p * len(x))(*[None if a is None else a.ctypes.data for a in x])
        return C.cast(v["_keep_" + name], C.c_void_p)
    if isinstance(x, np.ndarray):
        from gpt_amd import _lib
        if x.dtype == np.float64:
            return x.ctypes.data_as(_lib.P_D)
        return x.ctypes.data_as(_lib.P_I32) if x.dtype == np.int32 else C.c_void_p(x.ctypes.data)
    return x


def call(entry, **over):
    """gpt_cf_<entry> on the valid arguments with `over` replacing some (None: a null pointer; for
    the folds entry a per-fold list may be replaced whole or carry None entries)."""
    from gpt_amd import _lib
    v = _values()
    for k, x in over.items():
        if k in v["_folds"]:
            v["_folds"][k] = x
        else:
            v[k] = x
    return getattr(_lib.lib(), "gpt_cf_" + entry)(*[_arg(v, n) for n in ENTRIES[entry]])


def fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert str(ei.value) == "gptsgld error %d: %s" % (_lib.GPT_ERR_BAD_DIMS, text), str(ei.value)


def bad_args(entry):
    return "bad %s arguments" % NAMES[entry]


def _arrays(entry):
    """The required arrays of an entry (w_store is none of the fixw entries' parameters)."""
    pointers = {"Rating", "Ratingtest", "UserData", "MovieData", "w", "w_store"} | set(OUT)
    return [n for n in ENTRIES[entry] if n in pointers]


@pytest.mark.parametrize("entry,name", [(e, n) for e in SINGLE for n in _arrays(e)])
def test_null_array_fails_without_a_device(entry, name):
    fails(call(entry, **{name: None}), bad_args(entry))


FOLD_POINTERS = ["Ratings", "Ns", "Ratingtests", "Ntests", "ymeans", "ystds", "w_stores", "U_stores",
                 "V_stores", "testpred_stores", "trainRMSEs", "testRMSEs", "UserData", "MovieData", "w"]
FOLD_LISTS = ["Ratings", "Ratingtests", "w_stores", "U_stores", "V_stores", "testpred_stores",
              "trainRMSEs", "testRMSEs"]


@pytest.mark.parametrize("name", FOLD_POINTERS)
def test_folds_null_argument_fails_without_a_device(name):
    fails(call("fullw_sideinfo_folds", **{name: None}), bad_args("fullw_sideinfo_folds"))


@pytest.mark.parametrize("name", FOLD_LISTS)
def test_folds_null_array_of_one_fold_fails_without_a_device(name):
    arrs = _values()["_folds"][name]
    arrs[NF - 1] = None
    fails(call("fullw_sideinfo_folds", **{name: arrs}), bad_args("fullw_sideinfo_folds"))


def test_folds_status_may_be_null():
    """status is optional: with it null the call gets as far as the next refusal."""
    fails(call("fullw_sideinfo_folds", status=None, r=7),
          "GPT_fullw_sideinfo_folds: rank not instantiated (1-6,8,10,12,15,16,20) or minibatch too large")


@pytest.mark.parametrize("entry", SINGLE)
@pytest.mark.parametrize("bad", [dict(N=0), dict(N=-2), dict(Ntest=0), dict(n1=0), dict(n2=0),
                                 dict(n1=-1), dict(ldr=N - 1), dict(ldt=NT - 1), dict(burnin=-1),
                                 dict(maxepoch=-1), dict(signal_var=0.0), dict(signal_var=-0.8),
                                 dict(signal_var=float("nan")), dict(sigma_u=0.0), dict(sigma_u=-0.1),
                                 dict(sigma_u=float("nan"))],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_scalar_fails_without_a_device(entry, bad):
    fails(call(entry, **bad), bad_args(entry))


@pytest.mark.parametrize("bad", [dict(Ns=np.zeros(NF, dtype=np.int64)),
                                 dict(Ntests=np.array([NT, 0, NT], dtype=np.int64)), dict(n1=0),
                                 dict(n2=0), dict(D1=-1), dict(D2=-1), dict(m=0), dict(burnin=-1),
                                 dict(maxepoch=-1), dict(signal_var=0.0), dict(sigma_u=-0.1),
                                 dict(sigma_w=0.0), dict(sigma_w=float("nan")),
                                 dict(F=0), dict(F=-1), dict(F=65536),
                                 dict(Ns=np.array([N, N, N - 1], dtype=np.int64))],
                         ids=lambda d: "-".join("%s=%s" % (k, np.asarray(x).tolist()) for k, x in d.items()))
def test_folds_bad_scalar_fails_without_a_device(bad):
    """F outside 1..65535, a fold without ratings, unequal N across folds and the shared bounds."""
    fails(call("fullw_sideinfo_folds", **bad), bad_args("fullw_sideinfo_folds"))


@pytest.mark.parametrize("entry", ["fullw_sideinfo", "fullw", "fullw_gibbs"])
@pytest.mark.parametrize("sigma_w", [0.0, -1.0, float("nan")])
def test_bad_sigma_w_fails_without_a_device(entry, sigma_w):
    fails(call(entry, sigma_w=sigma_w), bad_args(entry))


@pytest.mark.parametrize("entry", [e for e in SGD if e != "fullw_sideinfo_folds"])
def test_bad_minibatch_fails_without_a_device(entry):
    fails(call(entry, m=0), bad_args(entry))


@pytest.mark.parametrize("entry", ["fullw_sideinfo", "fixw_sideinfo"])
@pytest.mark.parametrize("bad", [dict(D1=-1), dict(D2=-1)], ids=["D1", "D2"])
def test_negative_side_width_fails_without_a_device(entry, bad):
    fails(call(entry, **bad), bad_args(entry))


@pytest.mark.parametrize("entry", ["fullw_sideinfo", "fixw_sideinfo", "fullw_sideinfo_folds"])
def test_side_information_may_be_null_only_when_empty(entry):
    """D1 = D2 = 0 takes null UserData / MovieData: the call gets as far as the next refusal."""
    fails(call(entry, UserData=None, D1=0, MovieData=None, D2=0, r=7),
          "%s: rank not instantiated (1-6,8,10,12,15,16,20) or minibatch too large" % NAMES[entry])


@pytest.mark.parametrize("entry", GIBBS)
def test_gibbs_bad_sample_count_fails_without_a_device(entry):
    fails(call(entry, n_samples=0), bad_args(entry))


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("r", [7, 0, 21])
def test_uninstantiated_rank_fails_without_a_device(entry, r):
    tail = "" if entry in GIBBS else " or minibatch too large"
    fails(call(entry, r=r), "%s: rank not instantiated (1-6,8,10,12,15,16,20)%s" % (NAMES[entry], tail))


@pytest.mark.parametrize("entry", SGD)
def test_minibatch_past_the_lds_bound_fails_without_a_device(entry):
    """cf_lds_bytes(r = 3, m): 8·(2r² + 4mr + m) + 16m + 4·(4m + 2) + lists + 16 passes 160 KiB
    between m = 1000 and m = 2000 with or without the feature lists."""
    text = "%s: rank not instantiated (1-6,8,10,12,15,16,20) or minibatch too large" % NAMES[entry]
    fails(call(entry, m=2000), text)


def _with_id(col, row, value, test=False):
    x = _ratings(NT if test else N, 2 if test else 1)
    x[row, col] = value
    return x


@pytest.mark.parametrize("entry", SINGLE)
@pytest.mark.parametrize("col,value", [(0, 0), (0, N1 + 1), (1, 0), (1, N2 + 1)],
                         ids=["user0", "user_past", "movie0", "movie_past"])
def test_rating_ids_out_of_range_fail_without_a_device(entry, col, value):
    fails(call(entry, Rating=_with_id(col, N - 1, value)), "rating ids out of range")
    fails(call(entry, Ratingtest=_with_id(col, NT - 1, value, test=True)), "test rating ids out of range")


def test_folds_rating_ids_out_of_range_fail_without_a_device():
    """A bad id in the last fold is found before anything of the earlier folds goes to the device."""
    v = _values()["_folds"]
    v["Ratings"][NF - 1][N - 1, 0] = N1 + 1
    fails(call("fullw_sideinfo_folds", Ratings=v["Ratings"]), "rating ids out of range")
    v["Ratingtests"][NF - 1][0, 1] = 0
    fails(call("fullw_sideinfo_folds", Ratingtests=v["Ratingtests"]), "test rating ids out of range")


def _init(U0, rowsU, V0, rowsV, r):
    from gpt_amd import _lib
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.P_D)
    return _lib.lib().gpt_debug_cf_init(p(U0), rowsU, p(V0), rowsV, r)


def test_debug_cf_init_refusals_and_disarm():
    from gpt_amd import _lib
    U0, V0 = np.ones((N1 + D1) * R), np.ones((N2 + D2) * R)
    text = "gpt_debug_cf_init: U0 and V0 (rows >= 1, r >= 1), or both null"
    fails(_init(None, N1 + D1, V0, N2 + D2, R), text)
    fails(_init(U0, N1 + D1, None, N2 + D2, R), text)
    fails(_init(U0, 0, V0, N2 + D2, R), text)
    fails(_init(U0, N1 + D1, V0, 0, R), text)
    fails(_init(U0, N1 + D1, V0, N2 + D2, 0), text)
    assert _init(None, 0, None, 0, 0) == _lib.GPT_OK                  # the disarm form
    # an armed state of another shape is refused by the run that takes it ...
    assert _init(U0, N1 + D1 - 1, V0, N2 + D2, R) == _lib.GPT_OK
    fails(call("fullw_sideinfo"),
          "GPT_fullw_sideinfo: the injected U0 / V0 (gpt_debug_cf_init) are %d and %d rows of rank "
          "%d, the run has %d and %d of rank %d" % (N1 + D1 - 1, N2 + D2, R, N1 + D1, N2 + D2, R))
    # ... and is one shot, whatever refusal the run ends with: the next run meets its own only
    assert _init(U0, N1 + D1 - 1, V0, N2 + D2, R) == _lib.GPT_OK
    fails(call("fullw_sideinfo", N=0), bad_args("fullw_sideinfo"))
    fails(call("fullw_sideinfo", r=7),
          "GPT_fullw_sideinfo: rank not instantiated (1-6,8,10,12,15,16,20) or minibatch too large")
