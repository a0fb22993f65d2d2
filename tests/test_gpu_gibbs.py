"""The exact-conditional samplers against mpmath at rounding level: the tensor-GP Gibbs sweep and
geodesic Monte Carlo (gpt_amd/csrc/tgp.hip: tgp_temp/v/c/ck/vupd, syrk_mfma, the two-launch gemv,
chol_blk, trsv_blk, the gmc_* kernels), the MovieLens Gibbs sweeps (gpt_amd/csrc/cf.hip: cfg_rows,
cfg_wprec, cfg_wprec_fin, cfg_wrhs) and the Gaussian draw they share.

Every case of oracle/gibbs_cases.py runs through its entry (TGP.GPT_inf, GPT_SGLD.GPT_GMC,
movielens.GPT_fullw_gibbs / GPT_fixw_gibbs, gpt_debug_gaussian_draw) at the smallest shapes that
reach each kernel's tile and chunk edges (tests/test_gibbs_cases.py asserts them from the inputs).
Every stored element of every sweep / epoch is held to the 50-digit reference of
tests/golden/gibbs_mp.npz within B·max|x| of its sweep, the acceptance probability and the RMSEs
relative to themselves.  The tensor-GP sweep runs from X and y: the device whitens, maps its own
features (they differ from the reference's b in a third of the entries, by up to 2e-15·max|b|, which
the bar has to cover and does) and draws its own initial U; GMC starts from the injected R.init_state.

B = 8·u per family and quantity, u the largest error of the numpy restatement (R.GPT_inf, R.GPT_GMC,
M.GPT_fullw_gibbs, numpy.linalg for the draw) against mpmath over the family's cases;
tests/golden/make_gibbs_golden.py measures it, tests/test_gibbs_cases.py holds B under its caps
(1e-11 tensor-GP, 1e-13 GMC w and U, MovieLens and the draw, 1e-12 the acceptance probability) and
shows that seven defects of 1e-9 or less pass the oracle tests' 1e-8 and fail these bars.  The margin
of 8 is tests/test_gpu_step.py's, for the reasons given there: other summation orders (MFMA blocks of
four, wave sums, per-user statistics of the w precision), reciprocal-scaled pivots, and normals with
up to 7·2⁻⁵² of the radius.

Measured (make_gibbs_golden.py; worst device error / B per family as this test prints it):
    family  quantity: u / device worst over B
    tgp     W 1.0e-13 / 0.37   U 2.7e-13 / 0.09
    gmc     w 2.3e-15 / 0.21   U 7.9e-15 / 0.09   acceptance probability 6.0e-14 / 0.35
    mlg     w 4.3e-15 / 0.09   U 1.3e-15 / 0.14   V 4.5e-15 / 0.07   testpred 1.8e-15 / 0.13
            train RMSE 1.5e-16 / 0.13   test RMSE 1.9e-16 / 0.12
    draw    8.0e-16 / 0.47

B = 8·u.  33 runs, under 3 s on MI355X.  The golden maker takes 15 s on eight cores.
"""
import numpy as np
import pytest

from oracle import gibbs_cases as GC

pytestmark = pytest.mark.gpu


def run_device(c):
    """The case through its entry -> oracle.gibbs_cases.standard's dict."""
    p = GC.inputs(c)
    if c.family == "tgp":
        from gpt_amd import TGP
        res = TGP.GPT_inf(p["X"], p["y"], c.sigma, c.n, c.r, GC.TGP_SIGMA_RBF, c.q, GC.TGP_GEN, c.sweeps, 0,
                          I=None if c.fixed_I is None else p["I"])
        assert (res[2] == p["I"]).all()
    elif c.family == "gmc":
        from gpt_amd import GPT_SGLD as G
        res = G.GPT_GMC(p["phi"], p["y"], c.signal_var, p["I"], c.r, c.Q, c.eps, c.eps, 0, c.epochs, c.L,
                        GC.GMC_SEED, w_init=p["w0"], U_init=p["U0"])
    elif c.family == "mlg":
        from gpt_amd import movielens as ML
        args, kw = GC.mlg_args(c, p)
        res = getattr(ML, GC.mlg_entry(c))(*args, **kw)
    else:
        from gpt_amd import _lib
        seed, c1, c2, c3 = GC.DRAW_STREAM
        Mx, x = np.array(p["M"], order="F"), np.array(p["x"])
        res, st = np.zeros(c.p), np.zeros(1, dtype=np.int32)
        _lib.check(_lib.lib().gpt_debug_gaussian_draw(c.p, Mx.ctypes.data_as(_lib.P_D),
                                                      x.ctypes.data_as(_lib.P_D), seed, c1, c2, c3,
                                                      res.ctypes.data_as(_lib.P_D),
                                                      st.ctypes.data_as(_lib.P_I32)))
        assert st[0] == 0
    return GC.standard(c, res)


@pytest.mark.parametrize("c", GC.CASES, ids=[GC.case_id(c) for c in GC.CASES])
def test_sampler_against_mpmath(c):
    ref, B = GC.reference(c), GC.bars()[c.family]
    out = run_device(c)
    for q, v in out.items():
        assert v is None or (v.shape == ref[q][0].shape and np.isfinite(v).all()), q
    err = GC.rel_err(c, out, ref)
    assert set(err) == set(ref)
    print("%s: worst / B: %s" % (GC.case_id(c), "  ".join(
        "%s %.3f (%.2e)" % (q, err[q] / B[q], err[q]) for q in GC.QUANTITIES[c.family] if q in err)))
    for q, e in err.items():
        assert e <= B[q], (q, e, B[q])
