"""CPU tests of the stored-sample evaluation boundary (the features, the predictions of stored tensor
and full-theta samples, the posterior predictive and the class evaluation): every single bad
argument of a host-array entry fails with GPT_ERR_BAD_DIMS and its own message before any device
call, the header declares the entries and the library exports them with matching signatures.

Rejections that come only after a device call, left to the GPU suites: the null arrays of gpt_pred
and gpt_pred_mean other than ytest (their uploads meet them; test_gpu_pred*.py), every null of
gpt_pred_dev (the launch meets it), the labels of gpt_class_eval_dev, which are copied back before
they are checked (test_gpu_cls.py), and a failed allocation.  S < 1 of gpt_pred_mean returns
GPT_ERR_BAD_DIMS with no message of its own, so only its code is pinned."""
import numpy as np
import pytest

try:
    from tests.test_capi import header_functions
    from tests.test_julia_shim import header_prototypes
except ImportError:            # a foreign `tests` package on the path: the modules beside this one
    from test_capi import header_functions
    from test_julia_shim import header_prototypes

# the C argument order of every entry, by the names of _problem()
OUT8 = "fmu fs2 lp lpmix sums covered rmse srm"
CLS6 = "pm nl avg ms pr nlp"
ENTRIES = {
    "gpt_feature": "X N D ls ls_len sigma phi_scale Z b n phi",
    "gpt_feature_notensor": "X N D ls ls_len sigma Z b n phi",
    "gpt_feature_dev": "X N D ls ls_len sigma phi_scale Z b n phi stream",
    "gpt_pred": "w U I phitest n D Nt r Q fhat",
    "gpt_pred_mean": "w U I phitest ytest n D Nt r Q S scale mean rmse",
    "gpt_pred_mean_x": "w U I X ytest Nt D ls ls_len sigma phi_scale Z b n r Q S scale mean rmse srm",
    "gpt_pred_dev": "w U I phitest n D Nt r Q S fhat stream",
    "gpt_gpnt_pred": "theta phitest ytest n Nt T first last scale srm mean rmse scores_out",
    "gpt_gpnt_pred_x": "theta X ytest Nt D ls ls_len sigma Z b n T first last scale srm mean rmse "
                       "scores_out",
    "gpt_predictive": "F ytest Nt T first last noise " + OUT8,
    "gpt_predictive_dev": "F ytest Nt T first last noise fmu fs2 lp lpmix sums covered stream",
    "gpt_pred_predictive": "w U I phitest ytest n D Nt r Q S scale first last noise " + OUT8,
    "gpt_pred_predictive_x": "w U I X ytest Nt D ls ls_len sigma phi_scale Z b n r Q S scale first "
                             "last noise " + OUT8,
    "gpt_gpnt_predictive": "theta phitest ytest n Nt T first last scale noise " + OUT8,
    "gpt_gpnt_predictive_x": "theta X ytest Nt D ls ls_len sigma Z b n T first last scale noise " + OUT8,
    "gpt_class_eval": "scores yl Nt C T first last " + CLS6,
    "gpt_gpnt_pred_class": "theta phitest yl n Nt C T first last " + CLS6 + " scores_out",
    "gpt_pred_class": "w U I phitest yl n D Nt r Q C T first last " + CLS6 + " scores_out",
}
DIMS = dict(N=5, Nt=5, n=4, D=2, r=2, Q=3, S=3, T=3, C=3, ls_len=2, first=0, last=3, sigma=1.1,
            phi_scale=0.9, scale=1.5, noise=0.04, stream=None)


def _problem():
    """Valid arguments at the dims above.  Only I and the labels are read before the last check;
    one array of doubles, larger than any array these dims ask for, stands for every other."""
    p = dict(DIMS)
    p["I"] = np.asfortranarray(np.array([[1, 2], [2, 1], [2, 2]], dtype=np.int32))
    p["yl"] = np.array([1, 3, 2, 2, 1], dtype=np.int32)
    p["pr"] = np.zeros(DIMS["Nt"], dtype=np.int32)
    return p


def _call(entry, p=None, **over):
    from gpt_amd import _lib
    p = dict(_problem() if p is None else p, **over)
    dummy = np.ones(256)
    args = []
    for name in ENTRIES[entry].split():
        v = p.get(name, dummy)
        if isinstance(v, np.ndarray):
            v = v.ctypes.data_as(_lib.P_I32 if v.dtype == np.int32 else _lib.P_D)
        args.append(v)
    return getattr(_lib.lib(), entry)(*args)


def _fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert text in str(ei.value), (text, str(ei.value))


def _nulls(names, text):
    return [({k: None}, text) for k in names.split()]


def _each(values, text):
    return [(v, text) for v in values]


def _window(count, text):
    return _each([dict(first=-1), {"last": DIMS[count] + 1}, dict(first=2, last=2),
                  dict(first=3, last=2)], text)


FEATURE = "bad feature arguments"
LS = "dimensions of X and length_scale do not match"
BAD_LS = _each([dict(ls_len=0), dict(ls_len=3)], LS)
# valid_pred; `ls` keeps ls_len in {1, D} where D moves under an entry that checks ℓ first
def _pred_dims(ntest_low, **ls):
    return (_each([dict(n=0), dict(D=0, **ls), ntest_low, dict(r=0), dict(Q=0)], "bad pred dims") +
            [(dict(D=17, **ls), "D > 16 unsupported"), (dict(r=7), "rank not instantiated"),
             (dict(r=21), "rank not instantiated"), (dict(Q=100000), "pred LDS too large")])


def _bad_I():
    lo, hi = _problem()["I"], _problem()["I"]
    lo[0, 0], hi[-1, -1] = 0, DIMS["r"] + 1
    return _each([dict(I=lo), dict(I=hi)], "I entries must be in 1..r")


X_LDS = [(dict(n=8192), "pred LDS too large")]       # pred_x_lds_bytes alone: n = 8192 passes valid_pred
PV = "predictive: "
PV_DIMS = lambda count: _each([dict(Nt=0), {count: 0}, {count: 2 ** 22 + 1}, dict(Nt=2 ** 38 + 1)],
                              PV + "bad dimensions")
PV_WINDOW = lambda count: _window(count, PV + "the window must satisfy 0 <= first < last <= T")
NOISE = _each([dict(noise=v) for v in (0.0, -0.5, float("nan"), float("inf"), -float("inf"))],
              PV + "noise_var must be finite and > 0")
GP = "gpt_gpnt_pred: "
GP_DIMS = _each([dict(n=0), dict(Nt=0), dict(T=0), dict(n=2 ** 24 + 1), dict(T=2 ** 22 + 1),
                 dict(Nt=2 ** 40 + 1)], GP + "bad dimensions")
GP_WINDOW = _window("T", GP + "the window must satisfy 0 <= avg_first < avg_last <= T")
NT_FEATURE = (_nulls("ls Z b", FEATURE) + _each([dict(D=0), dict(D=2 ** 20 + 1)], FEATURE) + BAD_LS)
CE = "class_eval: "
CE_NULLS = _nulls("yl pm nl avg", CE + "null argument")
CE_DIMS = _each([dict(Nt=0), dict(C=0), dict(T=0), dict(C=2 ** 20 + 1), dict(T=2 ** 24 + 1),
                 dict(Nt=2 ** 40 + 1)], CE + "bad dimensions")
CE_WINDOW = _window("T", CE + "the window must satisfy 0 <= avg_first < avg_last <= T")


def _bad_labels():
    lo, hi = _problem()["yl"], _problem()["yl"]
    lo[0], hi[-1] = 0, DIMS["C"] + 1
    return _each([dict(yl=lo), dict(yl=hi)], CE + "labels must be in 1..C")


FEATURE_DEV = "bad gpt_feature_dev arguments (ls_len must equal D)"
NTC = "gpt_gpnt_pred_class: "
BAD = {
    "gpt_feature": _nulls("X ls Z b phi", FEATURE) + _each([dict(N=0), dict(D=0), dict(n=0)], FEATURE)
                   + BAD_LS,
    "gpt_feature_dev": _nulls("X ls Z b phi", FEATURE_DEV) +
                       _each([dict(N=0), dict(D=0), dict(n=0), dict(ls_len=1), dict(ls_len=3)],
                             FEATURE_DEV),
    "gpt_pred": _pred_dims(dict(Nt=-1)) + _bad_I(),
    "gpt_pred_mean": _nulls("ytest", "ytest required") + _pred_dims(dict(Nt=-1)) + _bad_I(),
    "gpt_pred_mean_x": _nulls("w U I X ytest ls Z b", "bad pred_mean_x arguments") +
                       [(dict(S=0), "bad pred_mean_x arguments")] + BAD_LS +
                       _pred_dims(dict(Nt=-1), ls_len=1) + X_LDS + _bad_I(),
    "gpt_pred_dev": _pred_dims(dict(Nt=-1)),
    "gpt_gpnt_pred": _nulls("theta phitest ytest srm mean rmse", GP + "null argument") + GP_DIMS +
                     GP_WINDOW,
    "gpt_gpnt_pred_x": _nulls("theta X ytest srm mean rmse", GP + "null argument") + GP_DIMS +
                       GP_WINDOW + NT_FEATURE,
    "gpt_predictive": _nulls("F ytest sums covered", PV + "null argument") + PV_DIMS("T") +
                      PV_WINDOW("T") + NOISE,
    "gpt_pred_predictive": _nulls("w U I phitest ytest sums covered rmse srm", PV + "null argument") +
                           PV_DIMS("S") + PV_WINDOW("S") + NOISE + _pred_dims(dict(n=-1)) + _bad_I(),
    "gpt_pred_predictive_x": _nulls("w ytest sums covered rmse srm", PV + "null argument") +
                             _nulls("U I X ls Z b", "bad pred_mean_x arguments") + PV_DIMS("S") +
                             PV_WINDOW("S") + NOISE + BAD_LS + _pred_dims(dict(n=-1), ls_len=1) +
                             X_LDS + _bad_I(),
    "gpt_gpnt_predictive": _nulls("theta phitest ytest sums covered rmse srm", PV + "null argument") +
                           _each([dict(n=0), dict(n=2 ** 24 + 1)], PV + "bad dimensions") +
                           PV_DIMS("T") + PV_WINDOW("T") + NOISE,
    "gpt_gpnt_predictive_x": _nulls("theta X ytest sums covered rmse srm", PV + "null argument") +
                             _each([dict(n=0), dict(n=2 ** 24 + 1)], PV + "bad dimensions") +
                             PV_DIMS("T") + PV_WINDOW("T") + NOISE + NT_FEATURE,
    "gpt_class_eval": _nulls("scores", CE + "null argument") + CE_NULLS + CE_DIMS + CE_WINDOW +
                      _bad_labels(),
    "gpt_gpnt_pred_class": _nulls("theta phitest", NTC + "bad arguments") +
                           _each([dict(n=0), dict(n=2 ** 24 + 1)], NTC + "bad arguments") + CE_NULLS +
                           CE_DIMS + CE_WINDOW + _bad_labels() +
                           [(dict(T=4194240 // 3 + 1), NTC + "C*T too large")],
    "gpt_pred_class": _nulls("w U I phitest", "gpt_pred_class: null argument") +
                      _pred_dims(dict(Nt=-1)) + CE_NULLS + CE_DIMS + CE_WINDOW + _bad_labels() +
                      [(dict(C=2 ** 20, T=2 ** 10 + 1), "gpt_pred_class: C*T too large")] + _bad_I(),
}
BAD["gpt_feature_notensor"] = BAD["gpt_feature"]
BAD["gpt_predictive_dev"] = BAD["gpt_predictive"]


def _show(v):
    return "None" if v is None else "array" if isinstance(v, np.ndarray) else repr(v)


CASES = [pytest.param(e, over, text, id="%s-%d-%s" % (e[4:], k, ",".join(
    "%s=%s" % (a, _show(v)) for a, v in over.items())))
         for e in ENTRIES for k, (over, text) in enumerate(BAD[e])]


@pytest.mark.parametrize("entry,over,text", CASES)
def test_single_bad_argument_fails_without_a_device(entry, over, text):
    _fails(_call(entry, **over), text)


def test_every_entry_has_cases():
    assert set(BAD) == set(ENTRIES)
    assert all(len(BAD[e]) >= 9 for e in ENTRIES)


def test_pred_mean_without_samples_fails_without_a_device():
    from gpt_amd import _lib
    assert _call("gpt_pred_mean", S=0) == _lib.GPT_ERR_BAD_DIMS
    assert _call("gpt_pred_mean", S=-1) == _lib.GPT_ERR_BAD_DIMS


def test_python_wrappers_raise_without_a_device():
    from gpt_amd import GPT_SGLD as G
    n, D, Nt, r, Q, S = 4, 2, 5, 2, 3, 3
    I = _problem()["I"]
    w, U = np.ones((Q, S)), np.ones((n, r, D, S))
    X, Z, b = np.ones((Nt, D)), np.ones((n, D)), np.ones((n, D))
    short = np.ones(Nt - 1)
    one_per_row = "ytest must have one target per test row"
    with pytest.raises(ValueError, match=one_per_row):
        G.predictive(np.ones((Nt, S)), short, 0.04)
    with pytest.raises(ValueError, match=one_per_row):
        G.pred_predictive(w, U, I, np.ones((n, D, Nt)), short, 0.04)
    with pytest.raises(ValueError, match=one_per_row):
        G.pred_predictive_x(w, U, I, X, short, 1.0, 1.0, 1.0, Z, b, 0.04)
    with pytest.raises(ValueError, match=one_per_row):
        G.GPNT_pred(np.ones((n, S)), np.ones((n, Nt)), short)
    with pytest.raises(ValueError, match=one_per_row):
        G.GPNT_predictive_x(np.ones((n, S)), X, short, 1.0, 1.0, Z, np.ones(n), 0.04)
    with pytest.raises(ValueError, match="U_store must be"):
        G.pred_predictive_x(w, U[:, :, :1], I, X, np.ones(Nt), 1.0, 1.0, 1.0, Z, b, 0.04)
    with pytest.raises(ValueError, match="the window must satisfy 0 <= first < last <= 3"):
        G.pred_predictive(w, U, I, np.ones((n, D, Nt)), np.ones(Nt), 0.04, window=(2, 2))
    with pytest.raises(ValueError, match="cannot reshape"):       # b is (n, D) for the tensor model
        G.pred_predictive_x(w, U, I, X, np.ones(Nt), 1.0, 1.0, 1.0, Z, np.ones(n), 0.04)
    with pytest.raises(ValueError, match="cannot reshape"):
        G.pred_mean_x(w, U, I, X, np.ones(Nt), 1.0, 1.0, 1.0, Z, np.ones(n))


def test_header_declares_and_library_exports_the_entries():
    from gpt_amd import _lib
    names = header_functions()
    protos = header_prototypes()
    lib = _lib.lib()
    for s, order in ENTRIES.items():
        assert s in names, s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert len(_lib.SIGNATURES[s][1]) == len(protos[s][1]) == len(order.split()), s
