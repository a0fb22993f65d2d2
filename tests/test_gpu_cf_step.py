"""The stored epochs of every CF SGD / SGLD launch path (gpt_amd/csrc/cf.hip: cf_epoch_kernel's lazy,
Stiefel and batch-phase forms, cf_move_kernel, cf_eval_kernel) against mpmath at rounding level.

Every case of oracle/cf_cases.py runs through its Python entry from the injected U0 / V0
(U_init / V_init), with step sizes at which a gradient error reaches the store undiminished: every
rank the kernels instantiate on the lazy path, r = 20 on the lazy, eager, Langevin and Stiefel paths,
batches of 128, 129 + 128, 200 + 16 and 1030 + 7, a one-user batch and an all-distinct batch, 0, 64
and 65 feature columns, a feature none / all of a batch's ratings carry, rows no batch touches, and
the averaged, cut-off evaluation on more test ratings than training ones.  Every element of w, U, V
and testpred_store of every stored epoch and both RMSEs are held to the 50-digit reference of
tests/golden/cf_step_mp.npz within B·max|x| (the RMSEs relative to themselves), and the columns of U
and V on the Stiefel path to norm one (colnorm); the launch mode (last_timing()["mode"]) is asserted.

B = 8·u per family and quantity, u the largest error of the fp64 numpy restatement
(oracle/movielens_ref.py from the same injected state) against mpmath over the family's cases;
tests/golden/make_cf_golden.py measures it, tests/test_cf_cases.py holds B <= 1e-13, the
conditioning limit, and shows that eight small defects fail the bars.  The margin of 8 is
tests/test_gpu_step.py's, for the same kind of reasons: the device sums in MFMA blocks of four and
wave sums, forms e·(sumV·wᵀ) where the restatement forms (e·sumV)·wᵀ, takes c^Δ by binary powering
where the restatement multiplies Δ times, and its expm solve divides by Newton-refined reciprocals.

Measured (make_cf_golden.py; worst device error / B per family as this test prints it):
    family        u: w, U, V, testpred, train RMSE, test RMSE, colnorm        device worst / B
    lazy_sgd      3.0e-15 2.6e-15 2.9e-15 4.8e-15 1.8e-16 2.6e-16 -         0.15 0.13 0.23 0.12 0.20 0.12 -
    eager_sgd     1.6e-15 1.3e-15 9.3e-16 3.5e-15 1.5e-16 1.0e-16 -         0.23 0.21 0.27 0.08 0.12 0.54 -
    sgld_euclid   3.9e-16 3.6e-16 5.0e-16 2.3e-16 7.2e-17 1.3e-16 -         0.11 0.11 0.09 0.12 0.12 0.11 -
    sgd_stiefel   4.5e-16 8.8e-16 9.2e-16 9.9e-16 1.4e-16 1.5e-16 2.1e-16   0.10 0.12 0.13 0.17 0.09 0.12 0.10
    sgld_stiefel  2.0e-16 8.9e-16 7.3e-16 4.2e-16 1.3e-16 1.6e-16 1.9e-16   0.15 0.08 0.08 0.08 0.06 0.12 0.12
    fixw          -       3.8e-16 4.8e-16 4.0e-16 1.9e-16 1.4e-16 2.4e-16   -    0.21 0.11 0.11 0.08 0.10 0.07

B = 8·u.  36 runs, 3.6 s on MI355X; the 2r × 2r expm arguments reach the Padé degrees 5, 7, 9 and 13
(largest 1-norm 25, the r = 2 Stiefel case).  The golden maker takes 25 s on eight cores.
"""
import numpy as np
import pytest

from oracle import cf_cases as CC

pytestmark = pytest.mark.gpu


def run_device(c, monkeypatch):
    """The case's Python entry from the injected state -> (oracle.cf_cases.standard's dict, mode)."""
    from gpt_amd import movielens as ML
    if c.lazy is None:
        monkeypatch.delenv("GPTSGLD_CF_LAZY", raising=False)
    else:
        monkeypatch.setenv("GPTSGLD_CF_LAZY", c.lazy)
    args, kw = CC.entry_args(c, CC.inputs(c))
    out = CC.standard(c, getattr(ML, "GPT_" + c.entry)(*args, **kw))
    return out, ML.last_timing()["mode"]


@pytest.mark.parametrize("c", CC.CASES, ids=[CC.case_id(c) for c in CC.CASES])
def test_cf_epochs_against_mpmath(c, monkeypatch):
    ref, B = CC.reference(c), CC.bars()[c.family]
    out, mode = run_device(c, monkeypatch)
    assert mode == CC.expected_mode(c)
    for q in CC.STORED:
        assert out[q] is None or np.isfinite(out[q]).all(), q
    err = CC.rel_err(out, ref, CC.on_manifold(c))
    print("%s: worst / B: %s" % (CC.case_id(c), "  ".join(
        "%s %.3f (%.2e)" % (q, err[q] / B[q], err[q]) for q in CC.QUANTITIES if q in err)))
    for q, e in err.items():
        assert e <= B[q], (q, e, B[q])


def test_injected_state_is_one_shot_and_checked():
    """gpt_debug_cf_init: a pair whose rows or rank differ from the run's is GPT_ERR_BAD_DIMS with a
    message, and the pair is gone afterwards (the next run starts from its own draw, bit for bit
    what a run without any injection returns)."""
    from gpt_amd import _lib
    from gpt_amd import movielens as ML
    c = [c for c in CC.CASES if c.name == "rank3"][0]
    args, kw = CC.entry_args(c, CC.inputs(c))
    plain = dict(kw, U_init=None, V_init=None)
    base = ML.GPT_fullw_sideinfo(*args, **plain)
    with pytest.raises(_lib.GPTError) as ei:
        ML.GPT_fullw_sideinfo(*args, **dict(kw, U_init=kw["U_init"][:-1]))
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS and "injected" in str(ei.value)
    again = ML.GPT_fullw_sideinfo(*args, **plain)
    for a, b in zip(base, again):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        ML.GPT_fullw_sideinfo(*args, **dict(kw, V_init=None))
    injected = ML.GPT_fullw_sideinfo(*args, **kw)
    assert not np.array_equal(injected[1], base[1])
