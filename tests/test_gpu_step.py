"""Three SGLD steps of every step kernel (gpt_amd/csrc/chain.hip, wave.hip, sgld.hip and the variant
families of the grid engine) against mpmath at rounding level.

Every case of oracle/step_cases.py runs on every engine that takes it, from the injected initial
state, with step sizes at which the gradient and the noise move w and U equally (so an error in one
element of gradw or gradU reaches the stored sample undiminished), over a full batch, the ragged last
batch of the epoch and the first batch of the next epoch.  Every stored element of w and U and every
gradient norm of the three steps is held to the 50-digit reference of tests/golden/step_mp.npz
within B·max|x|, and the columns of every U on the Stiefel path to norm one (colnorm, measured and
barred the same way).

B = 8·u per family and quantity, u the largest error of the fp64 restatements
(oracle/gpt_sgld_ref.py and, for SGLD + Stiefel regression, the C++ one) against mpmath over the
family's cases; tests/golden/make_step_golden.py measures it, tests/test_step_cases.py holds
B <= 1e-13 and shows that six small defects of the step arithmetic (1e-9 relative and below) fail
it.  The margin of 8: the device sums in other associations than either restatement (8-lane groups,
butterflies, MFMA blocks of 4, up to 512 terms), its divisions are Newton-refined reciprocals (1 ulp,
not correctly rounded), its normals carry up to 7·2^-52·radius (tests/test_gpu_fastmath.py), and u is
the worst of a few dozen samples of the same rounding process.

Measured (make_step_golden.py; worst device error / B per family as this test prints it):
    family            u: w, U, norms, colnorm           B = 8·u                           device worst / B
    sgld_stiefel      3.7e-16 1.1e-15 4.0e-15 7.6e-16   3.0e-15 9.2e-15 3.2e-14 6.1e-15   0.07 0.12 0.23 0.04
    sgd_stiefel       1.4e-16 3.9e-16 7.4e-16 2.2e-16   1.1e-15 3.1e-15 5.9e-15 1.7e-15   0.13 0.13 0.10 0.10
    sgld_euclid       2.0e-16 1.5e-16 7.9e-16 -         1.6e-15 1.2e-15 6.3e-15 -         0.08 0.13 0.06 -
    sgd_euclid        9.8e-17 1.4e-16 1.4e-15 -         7.8e-16 1.1e-15 1.1e-14 -         0.13 0.13 0.08 -
    wonly             2.4e-16 -       5.8e-16 -         1.9e-15 -       4.6e-15 -         0.08 -    0.12 -
    rmsprop           2.0e-16 1.6e-15 1.2e-14 3.3e-16   1.6e-15 1.3e-14 9.7e-14 2.6e-15   0.17 0.13 0.15 0.07
    cls_sgld_stiefel  1.5e-15 6.2e-16 2.9e-15 4.3e-16   1.2e-14 5.0e-15 2.3e-14 3.4e-15   0.05 0.15 0.06 0.06
    cls_sgd_stiefel   8.2e-16 6.0e-16 1.1e-15 2.2e-16   6.6e-15 4.8e-15 9.2e-15 1.8e-15   0.13 0.11 0.14 0.10
    cls_sgld_euclid   1.9e-16 4.0e-16 2.0e-15 -         1.5e-15 3.2e-15 1.6e-14 -         0.15 0.13 0.11 -
    cls_sgd_euclid    2.5e-16 3.3e-16 2.0e-15 -         2.0e-15 2.7e-15 1.6e-14 -         0.10 0.13 0.11 -

The sgld_stiefel figures are over the grid, chain and wave engines (64 runs in all, 43 cases).
The 2r × 2r expm arguments of the fixtures reach the Padé degrees 5, 7, 9 and 13 (each also in
the εU = 1e-4 cases; the largest 1-norm is 9.6, at the n = 512 case).  The golden maker takes 165 s on
eight cores (the r = 20, D = 12 case is one process for all of it; 500 s of mpmath in all).
"""
import numpy as np
import pytest

from oracle import step_cases as SC

pytestmark = pytest.mark.gpu

RUNS = [(c, e) for c in SC.CASES for e in SC.engines(c)]


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def run_device(c, engine):
    """The family's Python entry on the case, laid out as oracle.step_cases.run_numpy's result."""
    p = SC.inputs(c)
    n, D, r, Q, m, tail = c.shape
    a = (p["phi"], p["y"])
    kw = dict(w_init=p["w0"], U_init=p["U0"], diag=True)
    if c.family in SC.REG_FAMILIES:
        lang, stf = SC.REG_FAMILIES[c.family]
        ws, Us, dg = G().GPTregression(*a, p["signal_var"], p["I"], r, Q, m, p["epsw"], p["epsU"], 0, 2,
                                       SC.RUN_SEED, langevin=lang, stiefel=stf, max_steps=SC.STEPS,
                                       engine=engine, **kw)
        return SC.standard(ws, Us, dg.T)
    if c.family == "wonly":
        ws, _, gn = G().GPT_SGLDERMw(*a, p["signal_var"], p["I"], r, Q, m, p["epsw"], 0, 2, SC.RUN_SEED,
                                     **kw)
        return SC.standard(ws, None, gn[:, None])
    if c.family == "rmsprop":
        ws, Us, dg = G().GPT_SGLDERM_RMSprop(*a, p["signal_var"], p["I"], r, Q, m, p["epsU"], SC.ALPHA,
                                             0, 2, SC.RUN_SEED, **kw)
        return SC.standard(ws, Us, dg.T)
    lang, stf = SC.CLS_FAMILIES[c.family]
    ws, Us, dg = G().GPTclassification(*a, p["I"], r, Q, m, p["epsw"], p["epsU"], 0, 2, SC.RUN_SEED,
                                       langevin=lang, stiefel=stf, **kw)
    return SC.standard(ws, Us, dg.transpose(1, 2, 0))


@pytest.mark.parametrize("c,engine", RUNS, ids=["%s-%s" % (SC.case_id(c), e) for c, e in RUNS])
def test_step_against_mpmath(c, engine):
    ref, B = SC.reference(c), SC.bars()[c.family]
    out = run_device(c, engine)
    for q in ("w", "U", "norms"):
        assert out[q] is None or np.isfinite(out[q]).all(), q
    err = SC.rel_err(out, ref, SC.on_manifold(c))
    print("%s %s: worst / B: %s" % (SC.case_id(c), engine, "  ".join(
        "%s %.3f (%.2e)" % (q, err[q] / B[q], err[q]) for q in SC.QUANTITIES if q in err)))
    for q, e in err.items():
        assert e <= B[q], (q, e, B[q])
