"""CPU conditions of the CF step suite (tests/test_gpu_cf_step.py): the committed double-double
references of oracle/cf_cases.py are mpmath's and belong to the inputs this machine regenerates;
every fixture is what its name says (duplicates certain, a one-user batch, an all-distinct batch, a
feature none / all of a batch carry, rows no batch touches, bit 63 of a feature mask, predictions cut
off at 1 and at 5) and well behaved (step-1 shares as stated, the lazy decay in (0, 1), every expm
argument bounded and more than one Padé degree reached, a one-ulp change of the inputs moves no
stored output by more than 1e-14·max|x|); the bars are 8× the numpy restatement's own error against
mpmath and at most 1e-13; and eight small defects of the step fail them on named cases."""
import os

import numpy as np
import pytest

from oracle import cf_cases as CC
from oracle import philox as px
from oracle import step_cases as SC

ST = CC._stored()
Q6 = CC.QUANTITIES[:-1]
MEAS = (("share_w", "share_U", "decay", "sigma_u", "pred_rms") + tuple("cond_" + q for q in Q6)
        + tuple("numpy_" + q for q in CC.QUANTITIES) + tuple("f64_" + q for q in CC.QUANTITIES)
        + ("seconds",))                                        # tests/golden/make_cf_golden.py
BY_NAME = {c.name: c for c in CC.CASES}


def meas(c):
    return dict(zip(MEAS, ST[CC.key(c) + "_meas"]))


@pytest.fixture(scope="module")
def numpy_runs():
    return {CC.key(c): CC.run_numpy(c) for c in CC.CASES}


def batches(c, epoch=0):
    """The 0-based (user, movie) ids of every batch of an epoch."""
    p = CC.inputs(c)
    ids = p["Rating"][px.randperm(p["N"], CC.RUN_SEED, epoch)][:, :2].astype(np.int64) - 1
    return [ids[c.m * b: c.m * (b + 1)] for b in range(CC.nbatch(c))]


def test_fixture_holds_every_case():
    assert os.path.getsize(CC.GOLDEN) < 500 * 1000
    assert len({c.name for c in CC.CASES}) == len(CC.CASES)
    for c in CC.CASES:
        k = CC.key(c)
        p = CC.inputs(c)
        assert str(ST[k + "_digest"]) == CC.digest(c), c.name
        shapes = dict(w=(c.r, c.r), U=(c.n1 + c.D1, c.r), V=(c.n2 + c.D2, c.r), testpred=(c.ntest,), rmse=(2,))
        for q in CC.STORED:
            if q == "w" and CC.fixw(c):
                assert k + "_w_hi" not in ST
                continue
            hi, lo = ST[k + "_%s_hi" % q], ST[k + "_%s_lo" % q]
            assert hi.shape == lo.shape == (c.epochs,) + shapes[q], (c.name, q)
            assert hi.dtype == np.float64 and lo.dtype == np.float32
            assert np.isfinite(hi).all() and np.isfinite(lo).all()
            assert (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)) * (1 + 1e-6)).all(), (c.name, q)
        assert p["N"] == c.nfull * c.m + c.tail and 0 < c.tail < c.m


def test_every_rank_and_path_is_in_the_table():
    """Every instantiated rank on the lazy path; r = 20 on the lazy, eager, Langevin and Stiefel
    paths; every launch mode; every entry point."""
    lazy = {c.r for c in CC.CASES if CC.expected_mode(c) == 2}
    assert lazy == set(CC.RANKS)
    with open(os.path.join(os.path.dirname(SC.GOLDEN), "..", "..", "gpt_amd", "csrc", "launch_util.h")) as f:
        text = f.read()
    listed = text[text.index("Ranks"):]
    listed = listed[listed.index("<") + 1:listed.index(">")]
    assert tuple(int(x) for x in listed.split(",")) == CC.RANKS
    r20 = [c for c in CC.CASES if c.r == 20]
    assert {CC.expected_mode(c) for c in r20} == {0, 1, 2}
    assert any(c.langevin and not c.stiefel for c in r20) and any(c.lazy == "0" for c in r20)
    assert {c.entry for c in CC.CASES} == {"fullw_sideinfo", "fixw_sideinfo", "fullw", "fixw"}
    for fam in CC.FAMILIES:
        assert len([c for c in CC.CASES if c.family == fam]) >= 2, fam
    assert {(c.m, c.tail) for c in CC.CASES} >= {(128, 1), (129, 128), (200, 16), (1030, 7), (100, 37)}
    assert {c.r for c in CC.CASES if c.stiefel and not c.langevin and not CC.fixw(c)} == {2, 16}
    assert {c.r for c in CC.CASES if c.stiefel and c.langevin and not CC.fixw(c)} == {5, 20}
    assert {c.r for c in CC.CASES if c.family == "sgld_euclid"} == {5, 20}
    assert any(c.avg and CC.expected_mode(c) == 2 for c in CC.CASES)
    assert any(c.avg and CC.expected_mode(c) == 1 for c in CC.CASES)
    for c in CC.CASES:
        if c.avg:
            assert c.ntest > CC.inputs(c)["N"] and c.ntest % 256 and c.epochs == 2


def test_fixtures_are_what_their_names_say():
    for c in CC.CASES:
        p = CC.inputs(c)
        users, movies = p["Rating"][:, 0].astype(int) - 1, p["Rating"][:, 1].astype(int) - 1
        # rows no batch touches, which the test set reads
        assert c.n1 - 1 not in users and c.n2 - 1 not in movies
        assert p["Rtest"][0, 0] == c.n1 and p["Rtest"][0, 1] == c.n2
        if c.D1:                                  # a rated user and a rated movie without features
            assert any(not p["UserData"][u].any() for u in set(users)) or c.special == "noneall"
        if c.D2:
            assert any(not p["MovieData"][v].any() for v in set(movies)) or c.special == "noneall"
        first = batches(c)[0]
        if c.special != "distinct":               # duplicates are certain: more ratings than ids
            assert c.m > c.n1 - 1 and c.m > c.n2 - 1
            assert len(set(first[:, 0])) < c.m and len(set(first[:, 1])) < c.m
    b = batches(BY_NAME["one_user_batch"])
    assert len(set(b[1][:, 0])) == 1 and len(set(b[0][:, 0])) > 1
    b = batches(BY_NAME["distinct_batch"])
    assert len(set(b[0][:, 0])) == 24 and len(set(b[0][:, 1])) == 24
    c = BY_NAME["feat_none_all"]
    p, b = CC.inputs(c), batches(c)
    assert not p["UserData"][b[0][:, 0], 0].any() and p["UserData"][b[1][:, 0], 0].all()
    assert not p["MovieData"][b[0][:, 1], 0].any() and p["MovieData"][b[1][:, 1], 0].all()
    for name, D in (("D64", 64), ("D65_csr", 65)):
        c = BY_NAME[name]
        p = CC.inputs(c)
        col = p["UserData"][:, D - 1]
        rated = set(p["Rating"][:, 0].astype(int) - 1)
        assert p["UserData"].shape[1] == D and any(col[u] for u in rated) and not all(col[u] for u in rated)
    assert BY_NAME["D64"].D2 == 1 and CC.expected_mode(BY_NAME["D65_csr"]) == 0
    assert BY_NAME["nofeat_fullw"].D1 == BY_NAME["nofeat_fullw"].D2 == 0
    assert BY_NAME["m1030_r1"].D1 == BY_NAME["m1030_r1"].D2 == 1
    assert CC.inputs(BY_NAME["live_r20_lazy"]) is CC.inputs(BY_NAME["live_r20_eager"])


def test_shares_decay_and_cutoffs(numpy_runs):
    """The step-1 shares the step sizes were tuned to, the lazy move's decay factor in (0, 1), and
    stored test predictions cut off at 1 and at 5 next to ones that are not (the averaged cases with
    dozens of each)."""
    for c in CC.CASES:
        p, m = CC.inputs(c), meas(c)
        assert m["share_U"] == pytest.approx(p["share_U"], rel=1e-9)
        assert p["share_U"] == pytest.approx(1.0 if c.langevin or c.stiefel else CC.SGD_EUCLID_SHARE, rel=0.01)
        if not CC.fixw(c):
            assert p["share_w"] == pytest.approx(1.0 if c.langevin else CC.SGD_EUCLID_SHARE, rel=0.01)
        if CC.expected_mode(c) == 2 or c.family == "eager_sgd":
            assert p["decay"] == pytest.approx(1 - CC.DECAY, abs=2e-3) and 0 < p["decay"] < 1
        assert p["pred_rms"] <= CC.PRED_MAX or c.stiefel
        tp = numpy_runs[CC.key(c)]["testpred"]
        lo, hi = int((tp == 1.0).sum()), int((tp == 5.0).sum())
        assert lo + hi > 0 and lo + hi < tp.size, c.name
        if c.avg:
            assert lo >= 20 and hi >= 20 and tp.size - lo - hi >= 20, (c.name, lo, hi)


def _degree(norm):
    return 3 if norm <= 0.015 else 5 if norm <= 0.25 else 7 if norm <= 0.95 else 9 if norm <= 2.1 else 13


def test_expm_arguments_are_bounded_and_reach_several_pade_degrees():
    degrees = set()
    for c in CC.CASES:
        if not c.stiefel:
            continue
        norms = CC.expm_norms(c)
        stored = ST[CC.key(c) + "_expm_norms"]
        assert norms.shape == stored.shape and np.allclose(norms, stored, rtol=1e-9, atol=0)
        assert norms.max() <= CC.NORM_MAX, (c.name, norms.max())
        d = {_degree(v) for v in norms[0::2]}                  # the 2r x 2r arguments
        assert len(d) > 1 or c.epochs == 1, (c.name, d)
        degrees |= d
    print("Padé degrees of the 2r x 2r arguments: %s" % sorted(degrees))
    assert {5, 7, 9, 13} <= degrees


def test_conditioning(numpy_runs):
    worst = 0.0
    for c in CC.CASES:
        for s in range(3):
            e = CC.rel_err(CC.run_numpy(c, CC.perturbed(c, s)), numpy_runs[CC.key(c)])
            worst = max(worst, max(e.values()))
            assert max(e.values()) <= CC.COND_MAX, (c.name, e)
    print("worst response to a one-ulp change of the inputs: %.2e" % worst)


def test_bars(numpy_runs):
    """B = 8·u, u the numpy restatement's largest error against mpmath per family and quantity as
    the maker measured it; B <= 1e-13; the numpy restatement of this machine, and the float64 run of
    the reference's own code, pass what the device is asked to pass."""
    bars, u = CC.bars(), CC.measured_u()
    for fam in CC.FAMILIES:
        cases = [c for c in CC.CASES if c.family == fam]
        for q in CC.QUANTITIES:
            vals = [meas(c)["numpy_" + q] for c in cases]
            if np.isnan(vals).all():
                assert u[fam][q] == 0 and q in ("w", "colnorm")
                continue
            assert u[fam][q] == np.nanmax(vals) > 0
            assert bars[fam][q] == CC.MARGIN * u[fam][q] <= CC.B_MAX, (fam, q, bars[fam][q])
        print("%-14s u = %s  B = %s" % (fam, " ".join("%.1e" % u[fam][q] for q in CC.QUANTITIES),
                                       " ".join("%.1e" % bars[fam][q] for q in CC.QUANTITIES)))
    for c in CC.CASES:
        for run in (numpy_runs[CC.key(c)], CC.run_f64(c)):
            for q, e in CC.rel_err(run, CC.reference(c), CC.on_manifold(c)).items():
                assert e <= bars[c.family][q], (c.name, q, e)


# defect -> the cases that have to catch it (each fails its family's bar on an asserted quantity)
CAUGHT_BY = {
    "feature_sum_drops_last": ("rank3", "live_r20_lazy", "D64", "feat_none_all"),
    "duplicate_user_lost": ("rank4", "sort128_tail1", "walk129_sort128", "one_user_batch", "m1030_r1"),
    "movie_side_b": ("rank5", "live_r20_eager", "fixw_side_sgd"),
    "tail_scale": ("rank1", "sort128_tail1", "walk200_tail16", "sgld_r5", "stf_sgd_r2"),
    "skipped_row_decay": ("rank2", "nofeat_fullw", "m1030_r1", "fixw_sgd"),
    "gradw_col17": ("rank20", "live_r20_lazy", "sgld_r20", "stf_sgld_r20"),
    "noise_epoch_base": ("sgld_r5", "sgld_r20", "stf_sgld_r5", "fixw_stf_sgld"),
    "avg_counter": ("lazy_avg_eval", "stf_sgld_r5"),
}


@pytest.mark.parametrize("defect", sorted(CC.DEFECTS))
def test_defect_fails_the_bar(defect):
    """Each defect of oracle.cf_cases.DEFECTS, run through the comparison the device gets, exceeds
    its family's B on each of the named cases."""
    assert set(CAUGHT_BY) == set(CC.DEFECTS)
    bars = CC.bars()
    for name in CAUGHT_BY[defect]:
        c = BY_NAME[name]
        e = CC.rel_err(CC.run_f64(c, defect), CC.reference(c), CC.on_manifold(c))
        over = {q: v / bars[c.family][q] for q, v in e.items() if not v <= bars[c.family][q]}
        print("%s on %s: over B by %s" % (defect, name, {q: "%.3g" % v for q, v in over.items()}))
        assert over, (defect, name, e)


def test_fixture_equals_mpmath():
    """Two small cases recomputed: bit for bit the stored hi + lo."""
    pytest.importorskip("mpmath")
    for name in ("rank1", "fixw_stf_sgld"):
        c = BY_NAME[name]
        for s, a in CC.pack(c, CC.compute(c)).items():
            assert np.array_equal(a, ST[CC.key(c) + "_" + s]), (name, s)
