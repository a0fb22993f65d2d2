"""CPU conditions of the step suite (tests/test_gpu_step.py): the committed double-double references
of oracle/step_cases.py are mpmath's and belong to the inputs this machine regenerates; every
fixture is well behaved (status 0, gradient and noise move w and U equally at step 1, every expm
argument bounded and the Padé degrees 5, 7 and 9 reached, a one-ulp change of the inputs moves no
stored output by more than 1e-14·max|x|); the bars are 8× the fp64 restatements' own error against
mpmath and at most 1e-13; and six small defects of the numpy restatement fail them."""
import os

import numpy as np
import pytest

from oracle import step_cases as SC

ST = SC._stored()
MEAS = ("share_w", "share_U", "cond_w", "cond_U", "cond_norms", "numpy_w", "numpy_U", "numpy_norms",
        "numpy_colnorm", "cpp_w", "cpp_U", "cpp_colnorm", "seconds")     # tests/golden/make_step_golden.py
REG_CASES = [c for c in SC.CASES if c.family == SC.REG]


def meas(c):
    return dict(zip(MEAS, ST[SC.key(c) + "_meas"]))


@pytest.fixture(scope="module")
def numpy_runs():
    return {c: SC.run_numpy(c) for c in SC.CASES}


def test_fixture_holds_every_case():
    assert os.path.getsize(SC.GOLDEN) < 500 * 1000
    assert len({SC.key(c) for c in SC.CASES}) == len(SC.CASES)
    for c in SC.CASES:
        k = SC.key(c)
        n, D, r, Q, m, tail = c.shape
        assert str(ST[k + "_digest"]) == SC.digest(c), k
        cls = (SC.NCLS,) if c.family in SC.CLS_FAMILIES else ()
        assert ST[k + "_w_hi"].shape == (SC.STEPS, Q) + cls
        assert ST[k + "_n_hi"].shape == (SC.STEPS,) + cls + ((1,) if c.family == "wonly" else (1 + D,))
        steps, idx = SC.u_select(c)
        names = ["w", "n"]
        if c.family != "wonly":
            names.append("U")
            assert ST[k + "_U_hi"].shape == (len(steps), len(idx))
            assert steps[-1] == SC.STEPS - 1
        for s in names:
            hi, lo = ST[k + "_%s_hi" % s], ST[k + "_%s_lo" % s]
            assert hi.dtype == np.float64 and lo.dtype == np.float32 and hi.shape == lo.shape
            assert np.isfinite(hi).all() and np.isfinite(lo).all()
            assert (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)) * (1 + 1e-6)).all(), (k, s)


def test_kept_entries_reach_every_row_column_and_dimension():
    for c in SC.CASES:
        n, D, r, Q, m, tail = c.shape
        shape = (n, r, D) + ((SC.NCLS,) if c.family in SC.CLS_FAMILIES else ())
        steps, idx = SC.u_select(c)
        sub = np.unravel_index(idx, shape, order="F")
        for axis, size in enumerate(shape):
            assert len(np.unique(sub[axis])) == size, (SC.case_id(c), axis)
        if int(np.prod(shape)) <= SC.U_FULL:
            assert steps == tuple(range(SC.STEPS)) and len(idx) == int(np.prod(shape))


def test_every_engine_path_is_in_the_table():
    """Both chain builds, every rank the wave engine instantiates, and the shapes only the grid
    engine takes; every family besides SGLD + Stiefel regression on two shapes."""
    eng = {c: SC.engines(c) for c in REG_CASES}
    chain = [c for c in REG_CASES if "chain" in eng[c]]
    assert any(c.shape[1] <= 4 for c in chain) and any(c.shape[1] >= 5 for c in chain)
    assert {c.shape for c in chain} == {c.shape for c in REG_CASES if c.shape[2] <= 5} - {
        (101, 2, 3, 9, 10, 3), (40, 12, 2, 24, 15, 5)}             # odd n past one block, D > 8
    big = [c for c in chain if c.shape[0] == 512][0]               # a run of exactly the 64 maximum
    assert max(np.bincount(SC.inputs(big)["I"][:, k]).max() for k in range(8)) == 64
    assert {c.shape[2] for c in REG_CASES if "wave" in eng[c]} == set(SC.WAVE_RANKS)
    assert any(eng[c] == ("grid",) for c in REG_CASES)
    assert all("grid" in e for e in eng.values())
    for fam in SC.FAMILIES:
        assert len([c for c in SC.CASES if c.family == fam]) >= 2, fam
    for c in SC.CASES:                                 # N = m + tail, 0 < tail < m
        assert 0 < c.shape[5] < c.shape[4]


def test_status_and_gradient_share(numpy_runs):
    """Status 0 in every step, and at step 1 the gradient's part of each move is 0.5 .. 2 times the
    noise's wherever a step size or σ² is there to set it (SGD + Euclidean moves U by
    SGD_EUCLID_SHARE of itself; RMSprop's εw is not free; the classifier has no σ² and its εU is
    capped, so its shares are recorded only)."""
    for c in SC.CASES:
        assert numpy_runs[c]["status"] == 0, SC.case_id(c)
        p, m = SC.inputs(c), meas(c)
        assert m["share_U"] == pytest.approx(p["share_U"], rel=1e-9)
        if c.family in SC.CLS_FAMILIES:
            continue
        if c.family != "rmsprop":
            assert 0.5 <= p["share_w"] <= 2, SC.case_id(c)
        if c.family == "sgd_euclid":
            assert p["share_U"] == pytest.approx(SC.SGD_EUCLID_SHARE, rel=0.01)
        elif c.family != "wonly":
            assert 0.5 <= p["share_U"] <= 2, SC.case_id(c)


def _degree(norm):
    return 3 if norm <= 0.015 else 5 if norm <= 0.25 else 7 if norm <= 0.95 else 9 if norm <= 2.1 else 13


def test_expm_arguments_are_bounded_and_reach_the_pade_degrees():
    """Every expm argument's 1-norm is recorded and at most 30; the 2r × 2r arguments (every other
    call of geod) reach the Padé degrees 5, 7 and 9, the last through the εU = 1e-4 cases."""
    degrees, large_step = set(), set()
    for c in SC.CASES:
        norms = SC.expm_norms(c)
        stored = ST[SC.key(c) + "_expm_norms"]
        assert norms.shape == stored.shape and np.allclose(norms, stored, rtol=1e-9, atol=0)
        if len(norms):
            assert norms.max() <= SC.NORM_MAX, (SC.case_id(c), norms.max())
        if c.family == SC.REG:
            d = {_degree(v) for v in norms[0::2]}
            degrees |= d
            if c.epsU == 1e-4:
                large_step |= d
    print("Padé degrees of the 2r x 2r arguments: %s; at epsU = 1e-4: %s" % (sorted(degrees),
                                                                            sorted(large_step)))
    assert {5, 7, 9} <= degrees and 9 in large_step


def test_conditioning(numpy_runs):
    """The numpy restatement with every input double moved to a neighbouring double: no stored
    output moves by more than 1e-14·max|x|."""
    worst = 0.0
    for c in SC.CASES:
        for s in range(3):
            e = SC.rel_err(SC.run_numpy(c, SC.perturbed(c, s)), numpy_runs[c])
            worst = max(worst, max(e.values()))
            assert max(e.values()) <= SC.COND_MAX, (SC.case_id(c), e)
    print("worst response to a one-ulp change of the inputs: %.2e" % worst)


def test_bars(numpy_runs):
    """B = 8·u, u the fp64 restatements' largest error against mpmath per family and quantity as the
    maker measured it; B <= 1e-13; and the numpy restatement of this machine passes what the device
    is asked to pass."""
    bars, u = SC.bars(), SC.measured_u()
    for fam in SC.FAMILIES:
        cases = [c for c in SC.CASES if c.family == fam]
        for q in SC.QUANTITIES:
            if np.isnan([meas(c)["numpy_" + q] for c in cases]).all():
                assert u[fam][q] == 0 and q in ("U", "colnorm")        # no U, or U off the manifold
                continue
            vals = [meas(c)["numpy_" + q] for c in cases]
            if fam == SC.REG and q != "norms":
                vals += [meas(c)["cpp_" + q] for c in cases]
            assert u[fam][q] == max(vals) > 0
            assert bars[fam][q] == SC.MARGIN * u[fam][q] <= SC.B_MAX, (fam, q, bars[fam][q])
        print("%-18s u = %s  B = %s" % (fam, " ".join("%.2e" % u[fam][q] for q in SC.QUANTITIES),
                                       " ".join("%.2e" % bars[fam][q] for q in SC.QUANTITIES)))
    for c in SC.CASES:
        for q, e in SC.rel_err(numpy_runs[c], SC.reference(c), SC.on_manifold(c)).items():
            assert e <= bars[c.family][q], (SC.case_id(c), q, e)


def test_cpp_restatement_within_the_bars():
    bars = SC.bars()[SC.REG]
    for c in REG_CASES:
        e = SC.rel_err(SC.run_cpp(c), SC.reference(c), True)
        assert all(e[q] <= bars[q] for q in ("w", "U", "colnorm")), (SC.case_id(c), e)


@pytest.mark.parametrize("k", SC.MUTANTS)
def test_mutant_fails_the_bar(k):
    """Each defect of oracle.step_cases.mutant, run through the comparison the device gets, exceeds
    its family's B in at least one case on a quantity tests/test_gpu_step.py asserts.  Mutants 1 to 5
    do so on the SGLD + Stiefel regression cases alone.  Mutant 6 (no column normalisation) does not:
    from a U on the manifold the exact geodesic keeps the column norms, so three steps without the
    normalisation drift by rounding only (colnorm at most 0.45·B, U at most 0.22·B there).  It is
    caught where the normalisation does work: the classifier's first move is a geodesic step
    whatever the variant, and the Euclidean variants start from randn columns of norm √n."""
    bars = SC.bars()
    caught = []
    for c in SC.CASES:
        with SC.mutant(k):
            out = SC.run_numpy(c)
        e = SC.rel_err(out, SC.reference(c), SC.on_manifold(c))
        over = {q: v / bars[c.family][q] for q, v in e.items() if v > bars[c.family][q]}
        if over:
            caught.append((c, over))
    reg = [c for c, _ in caught if c.family == SC.REG]
    print("mutant %d: over B in %d of %d cases (%d of %d SGLD + Stiefel regression cases); largest "
          "excess %.3g x B" % (k, len(caught), len(SC.CASES), len(reg), len(REG_CASES),
                               max([max(o.values()) for _, o in caught], default=0.0)))
    assert caught
    assert reg or k == 6


def test_fixture_equals_mpmath():
    """The two smallest cases recomputed: bit for bit the stored hi + lo."""
    pytest.importorskip("mpmath")
    for c in sorted(REG_CASES, key=lambda c: c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3])[:2]:
        packed = SC.pack(c, SC.compute(c))
        for s, a in packed.items():
            assert np.array_equal(a, ST[SC.key(c) + "_" + s]), (SC.case_id(c), s)
