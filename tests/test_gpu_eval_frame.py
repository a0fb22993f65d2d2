"""The routes through the host frame of the stored-sample evaluation entries
(gpt_amd/csrc/eval_frame.h): every entry that takes its predictions from a shared producer returns
the bits of its siblings, and a call writes only the timing slots that are its own.

Shapes: Ntest of 1, 257 and 513 put one row past the 256-row tiles of predictive_kernel and
class_eval_kernel and one past mean_sse_kernel's 512-thread stride; T = 1, and T = 3 with the
windows (0, 3), (1, 3), (2, 3); n = 17 for the full-theta routes, the smallest instantiated rank
(r = 1, with D = 2, Q = 3, n = 4) for the tensor routes, C = 3 classes; the length scale once as a
scalar and once per dimension.

Held bitwise elsewhere and not repeated here:
  test_gpu_predictive.py::test_tensor_routes       pred_predictive = predictive of the stacked pred
      columns (rows, scalars, RMSE figures), its fmu = pred_mean's on the window's columns, `cols`
      = `window`, and pred_predictive_x = pred_predictive on feature(X)
  test_gpu_predictive.py::test_full_theta_routes   GPNT_predictive = predictive of GPNT_pred's
      scores, its figures = GPNT_pred's at one shape, and GPNT_predictive_x = GPNT_predictive on
      featureNotensor(X)
  test_gpu_gpnt.py::test_pred_x_equals_pred_on_the_device_features   GPNT_pred_x = GPNT_pred on
      featureNotensor(X), scores included
  test_gpu_gpnt.py::test_evaluation_bit_for_bit_properties           the window's place and `cols`
  test_gpu_cls.py::test_device_pointer_evaluation_equals_the_host_form   gpt_class_eval_dev =
      gpt_class_eval
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NTESTS = [1, 257, 513]
WINDOWS = [(1, (0, 1)), (3, (0, 3)), (3, (1, 3)), (3, (2, 3))]       # T, window
N_THETA, D_THETA, C = 17, 3, 3
N_T, D_T, R_T, Q_T = 4, 2, 1, 3
NV, SCALE = 0.05, 3.1


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@functools.lru_cache(maxsize=None)
def theta_inputs(Nt, per_dim):
    rng = np.random.default_rng((4100, Nt, per_dim))
    p = dict(X=rng.standard_normal((Nt, D_THETA)), Z=rng.standard_normal((N_THETA, D_THETA)),
             b=2 * np.pi * rng.random(N_THETA), y=rng.standard_normal(Nt),
             ls=1.0 + 0.1 * rng.random(D_THETA) if per_dim else np.array([1.1]),
             theta=np.asfortranarray(rng.standard_normal((N_THETA, 3))))
    p["phi"] = G().featureNotensor(p["X"], p["ls"], 0.9, p["Z"], p["b"])
    for v in p.values():
        v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def tensor_inputs(Nt, per_dim):
    rng = np.random.default_rng((4200, Nt, per_dim))
    S = C * 3
    p = dict(X=rng.standard_normal((Nt, D_T)), Z=rng.standard_normal((N_T, D_T)),
             b=2 * np.pi * rng.random((N_T, D_T)), y=rng.standard_normal(Nt),
             ls=1.0 + 0.1 * rng.random(D_T) if per_dim else np.array([1.1]),
             w=np.asfortranarray(rng.standard_normal((Q_T, S))),
             U=np.asfortranarray(rng.standard_normal((N_T, R_T, D_T, S)) / 2.0),
             I=np.ones((Q_T, D_T), dtype=np.int32, order="F"),
             labels=rng.integers(1, C + 1, Nt).astype(np.int32))
    p["phi"] = G().feature(p["X"], p["ls"], 1.0, 1.3, p["Z"], p["b"])
    for v in p.values():
        v.setflags(write=False)
    return p


def same_figures(a, b):
    return (np.array_equal(a.mean_fhat, b.mean_fhat) and a.rmse == b.rmse
            and np.array_equal(a.sample_rmse, b.sample_rmse))


@pytest.mark.parametrize("per_dim", [False, True], ids=["ls-scalar", "ls-per-dim"])
@pytest.mark.parametrize("Nt", NTESTS)
def test_full_theta_routes_share_their_scores_and_figures(Nt, per_dim):
    p = theta_inputs(Nt, per_dim)
    for T, window in WINDOWS:
        theta = np.asfortranarray(p["theta"][:, :T])
        ref = G().GPNT_pred(theta, p["phi"], p["y"], window=window, scale=SCALE, scores=True)
        assert ref.scores.shape == (Nt, T) and np.isfinite(ref.scores).all()
        one_class = G().GPNT_pred_class(theta.reshape((N_THETA, 1, T), order="F"), p["phi"],
                                        np.ones(Nt, dtype=np.int32), window=window, scores=True)
        assert np.array_equal(one_class.scores[:, 0, :], ref.scores)
        on_phi = G().GPNT_predictive(theta, p["phi"], p["y"], NV, window=window, scale=SCALE)
        assert same_figures(on_phi, ref), (T, window)
        on_x = G().GPNT_predictive_x(theta, p["X"], p["y"], p["ls"], 0.9, p["Z"], p["b"], NV,
                                     window=window, scale=SCALE)
        assert same_figures(on_x, ref), (T, window)
        ref_x = G().GPNT_pred_x(theta, p["X"], p["y"], p["ls"], 0.9, p["Z"], p["b"], window=window,
                                scale=SCALE, scores=True)
        assert same_figures(ref_x, ref) and np.array_equal(ref_x.scores, ref.scores)


@pytest.mark.parametrize("per_dim", [False, True], ids=["ls-scalar", "ls-per-dim"])
@pytest.mark.parametrize("Nt", NTESTS)
def test_tensor_routes_share_their_predictions_and_figures(Nt, per_dim):
    p = tensor_inputs(Nt, per_dim)
    feat = (p["ls"], 1.0, 1.3, p["Z"], p["b"])
    for T, (a, b) in WINDOWS:
        w, U = np.asfortranarray(p["w"][:, :T]), np.asfortranarray(p["U"][..., :T])
        mean, rmse = G().pred_mean(w[:, a:b], U[..., a:b], p["I"], p["phi"], p["y"], scale=SCALE)
        _, _, curve = G().pred_mean_x(w, U, p["I"], p["X"], p["y"], *feat, scale=SCALE)
        assert curve.shape == (T,) and np.isfinite(curve).all()
        on_phi = G().pred_predictive(w, U, p["I"], p["phi"], p["y"], NV, window=(a, b), scale=SCALE)
        on_x = G().pred_predictive_x(w, U, p["I"], p["X"], p["y"], *feat, NV, window=(a, b),
                                     scale=SCALE)
        for ev in (on_phi, on_x):
            assert np.array_equal(ev.mean_fhat, mean) and ev.rmse == rmse, (T, a, b)
            assert np.array_equal(ev.sample_rmse, curve), (T, a, b)


@pytest.mark.parametrize("Nt", NTESTS)
def test_class_scores_are_the_stacked_predictions(Nt):
    p = tensor_inputs(Nt, True)
    for T, window in WINDOWS:
        w = np.asfortranarray(p["w"][:, :C * T].reshape((Q_T, C, T), order="F"))
        U = np.asfortranarray(p["U"][..., :C * T].reshape((N_T, R_T, D_T, C, T), order="F"))
        ev = G().pred_class(w, U, p["I"], p["phi"], p["labels"], window=window, scores=True)
        assert ev.scores.shape == (Nt, C, T)
        for t in range(T):
            for c in range(C):
                col = G().pred(w[:, c, t], U[..., c, t], p["I"], p["phi"])
                assert np.array_equal(ev.scores[:, c, t], col), (T, c, t)
        again = G().class_eval(ev.scores, p["labels"], window=window)
        assert np.array_equal(again.prop_missed, ev.prop_missed)
        assert np.array_equal(again.mean_fhat, ev.mean_fhat) and np.array_equal(again.nlp, ev.nlp)


def _class_slots():
    from gpt_amd import _lib
    ms = np.zeros(3)
    _lib.check(_lib.lib().gpt_class_last_timing(ms.ctypes.data_as(_lib.P_D)))
    return ms


def test_a_call_writes_only_its_own_timing_slots():
    p, q = theta_inputs(257, True), tensor_inputs(257, True)
    theta = np.asfortranarray(np.stack([p["theta"]] * C, axis=1))            # (n, C, T)
    cls = G().GPNT_pred_class(theta, p["phi"], q["labels"], scores=True)
    G().GPNT_pred(p["theta"], p["phi"], p["y"])
    gpnt, slots = G().gpnt_last_timing(), _class_slots()
    assert gpnt["eval"] > 0.0 and slots[1] > 0.0 and slots[2] > 0.0
    G().GPNT_predictive(p["theta"], p["phi"], p["y"], NV)
    G().GPNT_predictive_x(p["theta"], p["X"], p["y"], p["ls"], 0.9, p["Z"], p["b"], NV)
    assert G().predictive_last_timing() > 0.0
    assert G().gpnt_last_timing() == gpnt
    G().class_eval(cls.scores, q["labels"])
    after = _class_slots()
    assert after[1] == slots[1] and after[0] == slots[0]
