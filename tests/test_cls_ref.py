"""CPU tests of the classification restatements (tests/cls_ref.py), the yardsticks the device
tests of tests/test_gpu_cls.py rely on, the header and the segment fixture."""
import os
import re

import numpy as np
import pytest

import cls_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scale", CR.EVAL_SCALES)
@pytest.mark.parametrize("shape", CR.EVAL_SHAPES, ids=CR.case_name)
def test_numpy_evaluation_is_within_the_bound_of_mpmath(shape, scale):
    """Row errors within E_i and mean errors within the mean bound on every evaluation case,
    planted ties, equal rows and a far-below true class included.  Measured on these cases: worst
    row error 0.42·E, worst mean error 0.003 of its bound, so the bound cannot excuse a wrong
    kernel."""
    s, y, per = CR.eval_reference(shape, scale)
    ev = CR.class_eval_np(s, y)
    worst_row = worst_mean = 0.0
    for t, (pred, nlp, E) in enumerate(per):
        got_pred, got = CR.rows_eval_np(s[:, :, t], y)
        assert np.array_equal(got_pred, pred)
        err = np.array([abs(float(g - w)) for g, w in zip(got, nlp)])
        worst_row = max(worst_row, float((err / E).max()))
        assert (err <= E).all()
        mb = CR.mean_bound(E, nlp)
        merr = abs(float(ev["mean_nlp"][t] - CR.mp_mean(nlp)))
        worst_mean = max(worst_mean, merr / mb)
        assert merr <= mb
        assert ev["prop_missed"][t] == 1 - np.sum(pred == y) / shape[0]
    print("worst row error / E = %.3f, worst mean error / bound = %.4f" % (worst_row, worst_mean))
    assert worst_row < 0.6 and worst_mean < 0.05      # the yardstick has no slack to hide behind


@pytest.mark.parametrize("scale", CR.EVAL_SCALES)
@pytest.mark.parametrize("shape", CR.EVAL_SHAPES, ids=CR.case_name)
def test_planted_rows_and_windows_of_the_evaluation_cases(shape, scale):
    """The planted rows are what they claim, and no window's mean has a near-tie: no row would be
    left out of the window checks of the device test."""
    Nt, C, T = shape
    s, y = CR.eval_scores(shape, scale)
    pred, nlp = CR.rows_eval_np(s[:, :, 0], y)
    for i in range(12):
        k = i % 4
        if k == 0:
            assert pred[i] == 1 and y[i] == 1 and s[i, 0, 0] == s[i, C - 1, 0] == s[i, :, 0].max()
        elif k == 1:
            assert pred[i] == 1 and y[i] == C                   # a tie takes the first index
        elif k == 2:
            assert pred[i] == 1 and abs(nlp[i] - np.log(C)) < 1e-12
        else:
            assert abs(nlp[i] - 1000.0) < np.log(C) + 1e-9
    sw, _ = CR.eval_scores(shape, scale, plant=T > 1)           # T = 1: the window is sample 0
    for window in CR.eval_windows(T):
        mean = CR.window_mean(sw, window)
        gap = CR.top_two_gap(mean)
        assert (gap >= 1e-9 * (1 + np.abs(mean).max())).all(), (window, gap.min())


def test_ties_take_the_first_index():
    x = np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, -1.0, 0.0]])
    y = np.array([2, 1, 3])
    pred, _ = CR.rows_eval_np(x, y)
    assert list(pred) == [2, 1, 1]
    assert list(CR.rows_eval_mp(x, y)[0]) == [2, 1, 1]
    ev = CR.class_eval_np(x.reshape(3, 3, 1), y)
    assert ev["prop_missed"][0] == 1 - 2 / 3


def test_vectorised_sampler_equals_the_literal_loops():
    """The vectorised restatement against a one-to-one transcription of GPT_SGLD.jl:877-892."""
    for idx in (0, 3):
        case = CR.SAMPLER_CASES[idx]
        n, N, C, m, burnin, maxepoch, decay, sth = case
        phi, y, eps = CR.sampler_inputs(case, idx)
        a = CR.gpnt_sgld_class(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
        b = CR.gpnt_sgld_class_literal(phi, y, sth, m, eps, decay, burnin, maxepoch, 5)
        assert a.shape == (n, C, (burnin + maxepoch) * (-(-N // m)))
        assert CR.rel(a, b) < 1e-13, CR.rel(a, b)


def test_store_every_keeps_the_divisible_steps_and_class_0_draws_gpnt_sgld_streams():
    from oracle import philox as px
    case = CR.SAMPLER_CASES[0]
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, eps = CR.sampler_inputs(case, 0)
    nb = -(-N // m)
    full = CR.gpnt_sgld_class(phi, y, sth, m, eps, decay, burnin, maxepoch, 9)
    ends = CR.gpnt_sgld_class(phi, y, sth, m, eps, decay, burnin, maxepoch, 9, store_every=nb)
    assert np.array_equal(ends, full[:, :, nb - 1::nb])
    # eps = 0: the first step leaves theta, so column 0 is GPNT_SGLD's initial draw
    first = CR.gpnt_sgld_class(phi, y, sth, m, 0.0, decay, 0, 1, 9)
    assert np.array_equal(first[:, 0, 0], sth * px.normals(n, 9, 0, px.THETA_INIT, 0))


def test_nan_returns_zeros_n():
    case = CR.SAMPLER_CASES[0]      # theta overflows at step 2 and inf - inf is a NaN at step 3
    n, N, C, m, burnin, maxepoch, decay, sth = case
    phi, y, _ = CR.sampler_inputs(case, 0)
    with np.errstate(all="ignore"):
        out = CR.gpnt_sgld_class(phi, y, sth, m, 1e300, decay, burnin, maxepoch, 1)
    assert out.shape == (n,) and not out.any()


def test_labels_outside_1_to_C_raise():
    x = np.zeros((4, 3, 2))
    for bad in ([0, 1, 2, 3], [1, 2, 3, 4], [1.5, 1, 2, 3]):
        with pytest.raises(ValueError):
            CR.class_eval_np(x, np.array(bad))
    phi = np.zeros((5, 4))
    with pytest.raises(ValueError):
        CR.gpnt_sgld_class(phi, np.array([2.0, 3.0, 2.0, 3.0]), 1.0, 2, 1e-3, 0, 0, 1, 0)   # C = 2
    with pytest.raises(ValueError):
        CR.class_eval_np(x, np.array([1, 2, 3, 1]), window=(1, 1))


NEW_ENTRY_POINTS = ["gpt_gpnt_sgld_class", "gpt_gpnt_sgld_class_chains", "gpt_class_eval",
                    "gpt_gpnt_pred_class", "gpt_pred_class"]


def test_header_declares_the_classification_entry_points():
    txt = open(os.path.join(ROOT, "include", "gptsgld.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"^\s*int\s+(gpt_\w+)\s*\(", txt, flags=re.M))
    for want in NEW_ENTRY_POINTS + ["gpt_class_eval_dev"]:
        assert want in names, want


def test_library_and_bindings_carry_the_classification_entry_points():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    for name in NEW_ENTRY_POINTS + ["gpt_class_eval_dev"]:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    for name in ("GPNT_SGLDclass", "GPNT_SGLDclass_chains", "class_eval", "GPNT_pred_class",
                 "pred_class"):
        assert callable(getattr(G, name))


def test_bad_arguments_fail_before_any_device_work():
    """Null-free Python calls that must be refused by the C entry points on a machine without a
    GPU: an empty or out-of-range window, a label outside 1..C, C > 32, a label outside 1..C of
    the sampler."""
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    s = np.zeros((6, 3, 2), order="F")
    y = np.array([1, 2, 3, 1, 2, 3])
    for window in ((1, 1), (2, 1), (0, 3), (-1, 1)):
        with pytest.raises(_lib.GPTError) as e:
            G.class_eval(s, y, window=window)
        assert e.value.code == _lib.GPT_ERR_BAD_DIMS
    for bad in ([0, 2, 3, 1, 2, 3], [1, 2, 4, 1, 2, 3]):
        with pytest.raises(_lib.GPTError) as e:
            G.class_eval(s, np.array(bad))
        assert e.value.code == _lib.GPT_ERR_BAD_DIMS
        with pytest.raises(_lib.GPTError):
            G.GPNT_pred_class(np.zeros((4, 3, 2)), np.zeros((4, 6)), np.array(bad))
    phi = np.zeros((5, 4), order="F")
    with pytest.raises(_lib.GPTError) as e:
        G.GPNT_SGLDclass(phi, np.array([2.0, 3.0, 2.0, 3.0]), 1.0, 2, 1e-3, 0, 0, 1, 0)
    assert e.value.code == _lib.GPT_ERR_BAD_DIMS
    with pytest.raises(_lib.GPTError):
        G.GPNT_SGLDclass(phi, np.array([1.0, 40.0, 2.0, 3.0]), 1.0, 2, 1e-3, 0, 0, 1, 0)   # C = 40
    with pytest.raises(_lib.GPTError):
        G.GPNT_SGLDclass_chains(phi, np.array([1.0, 2.0, 1.0, 2.5]), 1.0, 2, [1e-3], 0, 0, 1, [0])
    with pytest.raises(_lib.GPTError) as e:                      # theta alone is 480 KB of LDS
        G.GPNT_SGLDclass(np.zeros((30000, 4), order="F"), np.array([1.0, 2.0, 1.0, 2.0]), 1.0, 2,
                         1e-3, 0, 0, 1, 0)
    assert e.value.code == _lib.GPT_ERR_BAD_DIMS and "LDS" in str(e.value)
    with pytest.raises(ValueError):
        G.GPNT_SGLDclass_chains(phi, np.array([1.0, 2.0, 1.0, 2.0]), 1.0, 2, [1e-3], 0, 0, 1, [0],
                                store_every=0)
    with pytest.raises(_lib.GPTError):                           # rank 7 is not instantiated
        G.pred_class(np.zeros((4, 3, 2)), np.zeros((5, 7, 2, 3, 2)), np.ones((4, 2), dtype=np.int32),
                     np.zeros((5, 2, 6)), y)


def test_segment_fixture():
    data = np.load(CR.GOLDEN)["data"]
    assert data.shape == (2310, 20) and data.dtype == np.float64
    assert sorted(set(data[:, -1])) == [1, 2, 3, 4, 5, 6, 7]
    Xtr, ytr, Xte, yte = CR.segment_problem()
    assert Xtr.shape == (1300, 16) and Xte.shape == (1010, 16)
    assert np.abs(Xtr.mean(axis=0)).max() < 1e-12 and np.abs(Xtr.std(axis=0, ddof=1) - 1).max() < 1e-12
    assert set(ytr) == set(yte) == set(range(1, 8))
