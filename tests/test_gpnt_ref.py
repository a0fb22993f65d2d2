"""CPU tests of the full-theta regression chains' restatements (tests/gpnt_ref.py), the yardstick
the device tests of tests/test_gpu_gpnt.py rely on, the declarations of the new entry points in
the header, the ctypes table and the Julia shim, and the argument checks of the Python wrappers."""
import os
import re

import numpy as np
import pytest

import gpnt_ref as GR
from oracle import gpt_sgld_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["gpt_gpnt_sgld_chains", "gpt_gpnt_sgld_chains_x", "gpt_gpnt_pred", "gpt_gpnt_pred_x",
                "gpt_gpnt_last_route"]
JULIA_BOUND = ["gpt_gpnt_sgld_chains", "gpt_gpnt_sgld_chains_x", "gpt_gpnt_pred", "gpt_gpnt_pred_x"]


@pytest.mark.parametrize("name", ["A", "E"])
def test_thinned_chains_restatement_equals_gpnt_sgld_columns(name):
    n, N, m, burnin, maxepoch, decay = GR.CASES[name]
    phi, y = GR.inputs(name)
    nb = -(-N // m)
    total = (burnin + maxepoch) * nb
    full = [R.GPNT_SGLD(phi, y, GR.SIGNAL_VAR[k], GR.SIGMA_THETA[k], m, GR.EPS[k], decay, burnin,
                        maxepoch, GR.SEEDS[k]) for k in range(3)]
    for every in (1, nb, 4):
        store, status = GR.gpnt_sgld_chains(phi, y, GR.SIGNAL_VAR, GR.SIGMA_THETA, m, GR.EPS, decay,
                                            burnin, maxepoch, GR.SEEDS, store_every=every)
        assert not status.any() and store.shape == (n, total // every, 3)
        for k in range(3):
            assert np.array_equal(store[:, :, k], full[k][:, every - 1::every][:, :total // every])
    assert not np.array_equal(full[0], full[2])          # the shared seed is not a shared chain


def test_nan_chain_of_the_restatement_is_zero_filled():
    n, N, m, burnin, maxepoch, decay = GR.CASES["A"]
    phi, y = GR.inputs("A")
    store, status = GR.gpnt_sgld_chains(phi, y, GR.SIGNAL_VAR, GR.SIGMA_THETA, m, [1e-4, 1e300, 1e-4],
                                        decay, burnin, maxepoch, GR.SEEDS)
    assert list(status) == [0, GR.NAN_THETA, 0]
    assert not store[:, :, 1].any() and store[:, :, 0].any() and store[:, :, 2].any()


@pytest.mark.parametrize("name", GR.STEP_CASES)
def test_numpy_three_steps_against_mpmath_is_the_yardstick(name):
    """u, the numpy restatement's own error against mpmath on the three-step inputs.  The device's
    bar is min(8·u, 1e-13) of max|theta|: u must be a rounding-level figure for that to bind."""
    u = GR.yardstick(name)
    print("case %s: numpy three-step error / max|theta| = %.3g, device bar = %.3g" % (
        name, u, GR.step_bar(name)))
    assert 0.0 < u < 1e-14
    assert GR.step_bar(name) == 8.0 * u
    n, _, m = GR.CASES[name][:3]
    ref = GR.step_reference(name)
    assert len(ref) == 3 and len(ref[0]) == n
    # a defect of 1e-12 relative in one element is far outside the bar
    phi, y, sv, sth, mm, eps, decay, seed = GR.step_problem(name)
    full = R.GPNT_SGLD(phi, y, sv, sth, mm, eps, decay, 0, 2, seed)[:, :3].copy()
    full[n // 2, 2] *= 1 + 1e-12
    assert GR.max_err_mp(full, ref) > 4 * GR.step_bar(name)


def test_evaluation_in_numpy_is_within_the_bounds_of_mpmath():
    """The bounds the device is held to, met by numpy's evaluation of the same inputs."""
    theta, phitest, ytest = GR.eval_inputs()
    n, Nt, T, scale, window = (GR.EVAL[k] for k in ("n", "Ntest", "T", "scale", "window"))
    ev = GR.eval_np(theta, phitest, ytest, window, scale)
    smp, mag = GR.scores_mp(phitest, theta)
    for i in range(Nt):
        for t in range(T):
            assert GR.abs_err_mp(ev["scores"][i, t], smp[i][t]) <= (n + 2) * GR.U * mag[i, t]
    for t in range(T):
        want = GR.rmse_mp(ev["scores"][:, t], ytest, scale)
        assert GR.rel_err_mp(ev["sample_rmse"][t], want) <= (Nt + 8) * GR.U
    S = window[1] - window[0]
    mmp = GR.mean_mp(ev["scores"], *window)
    bound = (S + 1) * GR.U * np.abs(ev["scores"][:, window[0]:window[1]]).sum(axis=1) / S
    for i in range(Nt):
        assert GR.abs_err_mp(ev["mean_fhat"][i], mmp[i]) <= bound[i]
    assert GR.rel_err_mp(ev["rmse"], GR.rmse_mp(ev["mean_fhat"], ytest, scale)) <= (Nt + 8) * GR.U


def _c_prototypes():
    txt = open(os.path.join(ROOT, "include", "gptsgld.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
            for m in re.finditer(r"^\s*int\s+(gpt_\w+)\s*\(([^)]*)\)\s*;", txt, flags=re.M | re.S)}


def test_header_table_and_julia_declare_the_new_entry_points():
    from gpt_amd import _lib
    protos = _c_prototypes()
    jl = open(os.path.join(ROOT, "julia", "GPT_SGLD_HIP.jl")).read()
    for name in ENTRY_POINTS + ["gpt_gpnt_last_timing"]:
        assert name in protos, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
        assert len(_lib.SIGNATURES[name][1]) == len(protos[name]), name
    for name in JULIA_BOUND:
        m = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % name, jl)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(protos[name]), name
    for fn in ("GPNT_SGLD_chains", "GPNT_SGLD_chains_x", "GPNT_pred", "GPNT_pred_x"):
        assert re.search(r"^function %s\(" % fn, jl, flags=re.M), fn
        assert re.search(r"^export[^#]*?\b%s\b" % fn, jl, flags=re.M | re.S), fn


def test_python_wrappers_exist():
    from gpt_amd import GPT_SGLD as G
    for fn in ("GPNT_SGLD_chains", "GPNT_SGLD_chains_x", "GPNT_pred", "GPNT_pred_x", "gpnt_last_route",
               "gpnt_last_timing", "RegEval"):
        assert callable(getattr(G, fn)), fn


def test_wrappers_reject_bad_arguments_before_any_device_call():
    from gpt_amd import GPT_SGLD as G
    phi = np.zeros((5, 8), order="F")
    y = np.zeros(8)
    ok = dict(signal_vars=0.1, sigma_thetas=1.0, m=4, eps_thetas=1e-4, decay_rate=0.0, burnin=0,
              maxepoch=1, seeds=[1, 2, 3])

    def chains(**kw):
        a = dict(ok, **kw)
        return G.GPNT_SGLD_chains(a.pop("phi", phi), a.pop("y", y), a["signal_vars"], a["sigma_thetas"],
                                  a["m"], a["eps_thetas"], a["decay_rate"], a["burnin"], a["maxepoch"],
                                  a["seeds"], store_every=a.get("store_every", 1))
    for bad in (dict(eps_thetas=[1e-4, 2e-4]), dict(signal_vars=[0.1] * 4), dict(sigma_thetas=[1.0, 2.0]),
                dict(seeds=[]), dict(store_every=0), dict(store_every=-2), dict(y=np.zeros(7)),
                dict(m=0)):
        with pytest.raises(ValueError):
            chains(**bad)
    X, Z, b = np.zeros((8, 2), order="F"), np.zeros((5, 2), order="F"), np.zeros(5)
    xargs = (0.1, 1.0, 4, 1e-4, 0.0, 0, 1)
    with pytest.raises(ValueError):
        G.GPNT_SGLD_chains_x(X, y, [1.0, 2.0, 3.0], 1.0, Z, b, *xargs, [1])      # 3 length scales, D = 2
    with pytest.raises(ValueError):
        G.GPNT_SGLD_chains_x(X, y, 1.0, 1.0, Z, np.zeros(4), *xargs, [1])         # b of the wrong length
    with pytest.raises(ValueError):
        G.GPNT_SGLD_chains_x(X, np.zeros(9), 1.0, 1.0, Z, b, *xargs, [1])
    with pytest.raises(ValueError):
        G.GPNT_SGLD_chains_x(X, y, 1.0, 1.0, Z, b, 0.1, 1.0, 4, [1e-4, 1e-4], 0.0, 0, 1, [1])
    theta, phitest, yt = np.zeros((5, 4), order="F"), np.zeros((5, 6), order="F"), np.zeros(6)
    for window in ((0, 5), (-1, 2), (2, 2), (3, 1)):
        with pytest.raises(ValueError):
            G.GPNT_pred(theta, phitest, yt, window=window)
    with pytest.raises(ValueError):
        G.GPNT_pred(theta, phitest, yt, cols=[0, 1], window=(0, 3))            # outside the columns
    with pytest.raises(ValueError):
        G.GPNT_pred(theta, phitest, np.zeros(5))
    with pytest.raises(ValueError):
        G.GPNT_pred(np.zeros((4, 4)), phitest, yt)
    with pytest.raises(ValueError):
        G.GPNT_pred_x(theta, np.zeros((6, 2)), yt, 1.0, 1.0, Z, b, window=(0, 5))


def test_c_entries_refuse_bad_dimensions_without_a_device():
    """Past the wrappers: n = 30 000 needs 240 KB for theta alone, and the message says so; null
    arguments and an empty window are refused by the C entries themselves."""
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    with pytest.raises(_lib.GPTError) as e:
        G.GPNT_SGLD_chains(np.zeros((30000, 4), order="F"), np.zeros(4), 0.1, 1.0, 2, 1e-4, 0.0, 0, 1, [1])
    assert e.value.code == _lib.GPT_ERR_BAD_DIMS and "LDS" in str(e.value)
    out = np.zeros(4)
    rc = _lib.lib().gpt_gpnt_pred(None, None, None, 4, 4, 1, 0, 1, 1.0, None, None, None, None)
    assert rc == _lib.GPT_ERR_BAD_DIMS
    P = lambda a: a.ctypes.data_as(_lib.P_D)
    rc = _lib.lib().gpt_gpnt_pred(P(out), P(out), P(out), 1, 4, 1, 1, 1, 1.0, P(out), P(out), P(out), None)
    assert rc == _lib.GPT_ERR_BAD_DIMS
    route = np.zeros(5, dtype=np.int32)
    assert _lib.lib().gpt_gpnt_last_route(route.ctypes.data_as(_lib.P_I32), 5) == 0
    assert _lib.lib().gpt_gpnt_last_route(None, 3) == _lib.GPT_ERR_BAD_DIMS
