"""CPU conditions of the posterior-predictive suite (tests/test_gpu_predictive.py): the numpy
restatement of tests/predictive_ref.py against mpmath on every case, the mixture identities by
quadrature, the conditions that let the GPU test be exact (no row sits on the interval's edge,
case h really separates the one-pass variance), the meaning of fs2 on exact posterior draws, and
the argument checks of every new C entry, which need no device."""
import math

import numpy as np
import pytest

import predictive_ref as PR
import test_julia_shim as TS

ENTRIES = ["gpt_predictive_dev", "gpt_predictive", "gpt_pred_predictive", "gpt_pred_predictive_x",
           "gpt_gpnt_predictive", "gpt_gpnt_predictive_x", "gpt_predictive_last_timing"]


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_numpy_restatement_against_mpmath(name):
    """The restatement is within (S + 16)·2^-53 of mpmath relative to the column's max, except
    where a cancellation the formula itself contains (lp_mix of case f: squared residuals scaled
    by 1/(2v) = 5e5) is larger; the yardstick carries that to the device's bar."""
    pytest.importorskip("mpmath")
    F, y, (a, b), nv = PR.inputs(name)
    got, ref, ys = PR.predictive_np(F, y, a, b, nv), PR.reference(name), PR.yardstick(name)
    print(name, {q: "%.3g" % (ys[q] / PR.U) for q in PR.QUANTITIES}, "x 2^-53")
    for q in PR.QUANTITIES:
        assert ys[q] <= 64 * (b - a + 16) * PR.U, (name, q, ys[q])
    assert (got["fs2"] >= 0).all()
    assert PR.rel_err(got["sum_lp"], ref["sum_lp"]) <= 64 * (b - a + 16) * PR.U
    assert got["covered"] == ref["covered"]
    assert np.isfinite(got["lp_mix"]).all()
    if name in ("a", "g"):
        assert (got["fs2"] == 0.0).all() and all(r == 0 for r in ref["fs2"])
        assert PR.col_err(got["lp_mix"], ref["lp"]) <= (b - a + 16) * PR.U


def test_mixture_mean_and_variance_by_quadrature():
    """∫ t m(t) dt = fmu and ∫ (t − fmu)² m(t) dt = fs2 + noise_var for m = (1/S) Σ_s N(f_s, v)."""
    mp = pytest.importorskip("mpmath")
    F, y, (a, b), nv = PR.inputs("c")
    ref = PR.reference("c")
    old = mp.mp.dps
    mp.mp.dps = 30
    try:
        v = mp.mpf(float(nv))
        for i in (0, 31, 64):
            f = sorted(mp.mpf(float(x)) for x in F[i, a:b])
            dens = lambda t: mp.fsum(mp.exp(-(t - x) ** 2 / (2 * v)) for x in f) / (len(f) * mp.sqrt(2 * mp.pi * v))
            pts = [f[0] - 14 * mp.sqrt(v)] + f + [f[-1] + 14 * mp.sqrt(v)]
            fmu, fs2 = ref["fmu"][i], ref["fs2"][i]
            assert abs(mp.quad(dens, pts) - 1) < mp.mpf(10) ** -18
            assert abs(mp.quad(lambda t: t * dens(t), pts) - fmu) < mp.mpf(10) ** -18
            var = mp.quad(lambda t: (t - fmu) ** 2 * dens(t), pts)
            assert abs(var - (fs2 + v)) < mp.mpf(10) ** -18
    finally:
        mp.mp.dps = old


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_no_row_sits_on_the_interval_edge(name):
    pytest.importorskip("mpmath")
    assert PR.reference(name)["margin"] > 1e-9


def test_case_h_separates_the_one_pass_variance():
    pytest.importorskip("mpmath")
    F, y, (a, b), nv = PR.inputs("h")
    one = PR.col_err(PR.onepass_fs2_np(F, a, b), PR.reference("h")["fs2"])
    two = PR.yardstick("h")["fs2"]
    print("one-pass %.3g, two-pass %.3g" % (one, two))
    assert one > 100 * two and two > 0


def test_fs2_of_exact_posterior_draws_is_the_posterior_variance():
    theta, phitest, ytest, var = PR.posterior_draws()
    got = PR.predictive_np(np.asfortranarray(phitest.T @ theta), ytest, 0, theta.shape[1],
                           PR.DRAWS["signal_var"])
    assert (np.abs(got["fs2"] / var - 1) <= PR.draws_band()).all()


# --------------------------------------------------------------------------- argument checks
def _args(entry, **bad):
    """The arguments of an entry on a tiny valid problem, with the named ones replaced."""
    from gpt_amd import _lib
    P, PI = _lib.P_D, _lib.P_I32
    Nt, T, n, D, r, Q = 5, 3, 4, 2, 1, 2
    rng = np.random.default_rng(1)
    a = dict(F=np.asfortranarray(rng.standard_normal((Nt, T))), y=rng.standard_normal(Nt),
             theta=np.asfortranarray(rng.standard_normal((n, T))),
             phi2=np.asfortranarray(rng.standard_normal((n, Nt))),
             phi3=np.asfortranarray(rng.standard_normal((n, D, Nt))),
             X=np.asfortranarray(rng.standard_normal((Nt, D))), ls=np.ones(D),
             Z=np.asfortranarray(rng.standard_normal((n, D))), b1=np.ones(n), b2=np.ones((n, D), order="F"),
             w=np.asfortranarray(rng.standard_normal((Q, T))),
             U=np.asfortranarray(rng.standard_normal((n, r, D, T))), I=np.ones((Q, D), dtype=np.int32, order="F"),
             fmu=np.ones(Nt), fs2=np.ones(Nt), lp=np.ones(Nt), lpmix=np.ones(Nt), sums=np.ones(2),
             covered=np.ones(1), rmse=np.ones(1), srm=np.ones(T))
    v = dict(Nt=Nt, T=T, first=0, last=T, nv=0.05)
    v.update({k: x for k, x in bad.items() if k in v})

    def p(name, t=P):
        return None if bad.get(name) is None and name in bad else a[name].ctypes.data_as(t)

    outs = [p(k) for k in ("fmu", "fs2", "lp", "lpmix", "sums", "covered")]
    tail = outs + [p("rmse"), p("srm")]
    win = [v["first"], v["last"]]
    return {
        "gpt_predictive_dev": [p("F"), p("y"), v["Nt"], v["T"]] + win + [v["nv"]] + outs + [None],
        "gpt_predictive": [p("F"), p("y"), v["Nt"], v["T"]] + win + [v["nv"]] + tail,
        "gpt_pred_predictive": [p("w"), p("U"), p("I", PI), p("phi3"), p("y"), n, D, v["Nt"], r, Q,
                                v["T"], 1.0] + win + [v["nv"]] + tail,
        "gpt_pred_predictive_x": [p("w"), p("U"), p("I", PI), p("X"), p("y"), v["Nt"], D, p("ls"), D,
                                  1.0, 1.0, p("Z"), p("b2"), n, r, Q, v["T"], 1.0] + win
                                 + [v["nv"]] + tail,
        "gpt_gpnt_predictive": [p("theta"), p("phi2"), p("y"), n, v["Nt"], v["T"]] + win
                               + [1.0, v["nv"]] + tail,
        "gpt_gpnt_predictive_x": [p("theta"), p("X"), p("y"), v["Nt"], D, p("ls"), D, 1.0, p("Z"),
                                  p("b1"), n, v["T"]] + win + [1.0, v["nv"]] + tail,
    }[entry]


BAD = [dict(first=2, last=2), dict(first=-1), dict(last=4), dict(first=3, last=1), dict(nv=0.0),
       dict(nv=-0.05), dict(nv=float("nan")), dict(nv=float("inf")), dict(T=0, last=0), dict(Nt=0),
       dict(y=None), dict(sums=None), dict(covered=None)]
# the first pointer of every entry, and the required outputs of the sample routes
NULLS = {"gpt_predictive_dev": ["F"], "gpt_predictive": ["F"],
         "gpt_pred_predictive": ["w", "U", "I", "phi3", "rmse", "srm"],
         "gpt_pred_predictive_x": ["w", "U", "I", "X", "ls", "Z", "b2", "rmse", "srm"],
         "gpt_gpnt_predictive": ["theta", "phi2", "rmse", "srm"],
         "gpt_gpnt_predictive_x": ["theta", "X", "ls", "Z", "b1", "rmse", "srm"]}


def _refused(entry, bad):
    from gpt_amd import _lib
    rc = getattr(_lib.lib(), entry)(*_args(entry, **bad))
    assert rc == _lib.GPT_ERR_BAD_DIMS, (entry, bad, rc)
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS and len(str(ei.value)) > 20


@pytest.mark.parametrize("entry", ENTRIES[:-1])
@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_bad_arguments_fail_without_a_device(entry, bad):
    _refused(entry, bad)


@pytest.mark.parametrize("entry", ENTRIES[:-1])
def test_null_pointers_fail_without_a_device(entry):
    for name in NULLS[entry]:
        _refused(entry, {name: None})
    from gpt_amd import _lib
    assert _lib.lib().gpt_predictive_last_timing(None) == _lib.GPT_ERR_BAD_DIMS


def test_python_wrappers_refuse_a_bad_window_or_shape():
    from gpt_amd import GPT_SGLD as G
    F, y, _, nv = PR.inputs("b")
    with pytest.raises(ValueError):
        G.predictive(F, y, nv, window=(2, 2))
    with pytest.raises(ValueError):
        G.predictive(F, y[:-1], nv)
    with pytest.raises(G.GPTError):
        G.predictive(F, y, -1.0)
    assert "gp" in G.PredictiveEval.__slots__ and hasattr(G.PredictiveEval, "mean_fhat")


def test_header_library_and_binding_agree():
    from gpt_amd import _lib
    protos = TS.header_prototypes()
    for name in ENTRIES:
        assert name in protos and hasattr(_lib.lib(), name), name
        assert len(_lib.SIGNATURES[name][1]) == len(protos[name][1]), name
