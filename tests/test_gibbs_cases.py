"""CPU conditions of the exact-conditional samplers' suite (tests/test_gpu_gibbs.py): the committed
double-double references of oracle/gibbs_cases.py are mpmath's and belong to the inputs this machine
regenerates; every case is what its name says, asserted from its inputs (the tile, panel and chunk
edges of tgp.hip and cf.hip, an absent core value, a repeated row of I, accepted and rejected epochs,
the rating counts of the synthetic design); no rounding can flip a Metropolis decision; the bars are
8× the numpy restatement's own error against mpmath and under their caps; and seven defects of 1e-9
or less pass the bars of the oracle tests and fail these on named cases.

Measured here (tests/golden/make_gibbs_golden.py): u per family and quantity
    tgp    W 1.0e-13  U 2.7e-13
    gmc    w 2.3e-15  U 7.9e-15  acceptance probability 6.0e-14
    mlg    w 4.3e-15  U 1.3e-15  V 4.5e-15  testpred 1.8e-15  train RMSE 1.5e-16  test RMSE 1.9e-16
    draw   8.0e-16
and the smallest |uniform − acceptance probability| of any epoch 0.086."""
import os
import re

import numpy as np
import pytest

from oracle import gibbs_cases as GC
from oracle import gpt_sgld_ref as R
from oracle import philox as px

ST = GC._stored()
CSRC = os.path.join(os.path.dirname(GC.GOLDEN), "..", "..", "gpt_amd", "csrc")
TILE = 16                 # the fp64 MFMA tile's rows and its K pass (four K steps of four)
WAVE = 64


def constant(name, source="tgp.hip"):
    with open(os.path.join(CSRC, source)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


def cases(family):
    return [c for c in GC.CASES if c.family == family]


def hi(c, q):
    return ST[GC.key(c) + "_%s_hi" % q]


def test_fixture_holds_every_case():
    assert os.path.getsize(GC.GOLDEN) < 500 * 1000
    assert len(GC.BY_NAME) == len(GC.CASES)
    for c in GC.CASES:
        k, p = GC.key(c), GC.inputs(c)
        assert str(ST[k + "_digest"]) == GC.digest(c), c.name
        if c.family == "tgp":
            shapes = dict(W=(c.sweeps, c.q), U=(c.sweeps, c.n, c.r, c.D))
        elif c.family == "gmc":
            shapes = dict(w=(c.epochs, c.Q), U=(c.epochs, c.n, c.r, c.D), acc=(c.epochs,))
        elif c.family == "mlg":
            T = c.maxepoch
            shapes = dict(w=(T, c.r, c.r), U=(T, p["n1"], c.r), V=(T, p["n2"], c.r), testpred=(T, GC.MLG_NTEST),
                          train_rmse=(T,), test_rmse=(T,))
        else:
            shapes = dict(out=(1, c.p))
        for q in GC.QUANTITIES[c.family]:
            if q == "w" and c.family == "mlg" and c.fixw:
                assert k + "_w_hi" not in ST
                continue
            h, l = ST[k + "_%s_hi" % q], ST[k + "_%s_lo" % q]
            assert h.shape == l.shape == shapes[q], (c.name, q)
            assert h.dtype == np.float64 and l.dtype == np.float32
            assert np.isfinite(h).all() and np.isfinite(l).all()
            assert (np.abs(l) <= 0.5 * np.spacing(np.abs(h)) * (1 + 1e-6)).all(), (c.name, q)


def test_fixture_equals_mpmath():
    """One small case of each family recomputed: bit for bit the stored hi + lo."""
    pytest.importorskip("mpmath")
    for name in ("absent_value_N13", "rank_one", "users3_r4", "p17"):
        c = GC.BY_NAME[name]
        for s, a in GC.pack(c, GC.compute(c)).items():
            assert np.array_equal(a, ST[GC.key(c) + "_" + s]), (name, s)


def test_tgp_cases_reach_the_edges():
    nb, gemv_chunk = constant("kCholNB"), constant("kGemvCh")
    by = GC.BY_NAME
    for c in cases("tgp"):
        assert c.sweeps >= 2                                       # sweep 2 holds the first drawn U
        assert GC.inputs(c)["b"].shape == (c.n, c.D, c.N) and GC.inputs(c)["I"].shape == (c.q, c.D)
    c = by["ragged_q20_N131"]
    assert c.sweeps == 3 and c.q // TILE == 1 and 0 < c.q % TILE            # two row tiles, one ragged
    assert c.N // TILE == 8 and c.N % TILE == 3                             # eight K passes + a tail of 3
    assert -(-c.N // WAVE) == 3 and c.N % WAVE                              # tgp_temp: three row tiles
    assert (c.n * c.r) // nb == 1 and (c.n * c.r) % nb == 5                 # a full panel + 5 columns
    c = by["absent_value_N13"]
    I = GC.inputs(c)["I"]
    assert c.N < TILE and c.q < TILE and c.fixed_I is not None
    assert (I[:, 1] != 2).all() and set(I[:, 0]) == {1, 2}
    # the absent value's block of the precision is r·I and its right-hand side 0: U_2[:, 2] = z / r
    z = px.normals(c.n * c.r, GC.TGP_GEN, 0, px.TGP_U_NOISE, 1).reshape((c.n, c.r), order="F")
    assert np.allclose(hi(c, "U")[1][:, 1, 1], z[:, 1] / c.r, rtol=0, atol=1e-14)   # fp64 Box–Muller
    assert not np.allclose(hi(c, "U")[1][:, 0, 1], z[:, 0] / c.r, rtol=1e-3, atol=0)
    c = by["gemv_two_chunks_N257"]
    assert c.N == gemv_chunk + 1 and c.q == 40 and c.n * c.r == 50
    c = by["n70_padded_temp"]
    assert WAVE < c.n <= 2 * WAVE and (c.n * c.r) // nb == 8 and (c.n * c.r) % nb == 12
    c = by["nr180_second_pass"]
    trailing = -(-(c.n * c.r - nb) // TILE)                                 # tiles behind the first panel
    assert c.n * c.r == 180 and trailing * (trailing + 1) // 2 > WAVE
    c = by["repeated_I_row"]
    I = GC.inputs(c)["I"]
    assert c.fixed_I is None and (I == R.tgp_draw_I(c.q, c.D, c.r, GC.TGP_GEN)).all()
    assert len({tuple(row) for row in I}) < c.q
    assert sum(c.fixed_I is None for c in cases("tgp")) == 5


def test_gmc_cases_and_the_metropolis_margin():
    """The named outcomes, from the mpmath run; every |uniform − acceptance| is at least 1e-3."""
    by = GC.BY_NAME
    margin, accepted = 1.0, {}
    for c in cases("gmc"):
        p = GC.inputs(c)
        acc = hi(c, "acc")
        u = np.array([px.uniform(GC.GMC_SEED, e, px.GMC_U, 0) for e in range(c.epochs)])
        assert (np.abs(u - acc) >= GC.METROPOLIS_MARGIN).all(), (c.name, u, acc)
        margin = min(margin, float(np.abs(u - acc).min()))
        accepted[c.name] = tuple(bool(a) for a in u <= acc)
        w, U = hi(c, "w"), hi(c, "U")
        prev_w, prev_U = p["w0"], p["U0"]
        for e in range(c.epochs):                       # a rejection restores w; U keeps its proposal
            assert np.array_equal(w[e], prev_w) == (not accepted[c.name][e]), (c.name, e)
            assert np.abs(U[e] - prev_U).max() > 1e-6
            prev_w, prev_U = w[e], U[e]
        assert np.abs(np.einsum("ejak,ejbk->eabk", U, U) - np.eye(c.r)[None, :, :, None]).max() < 1e-14
    print("smallest |uniform - acceptance probability|: %.3g; accepted: %s" % (margin, accepted))
    assert accepted["accepting"] == (True, True, True)
    assert accepted["rejecting"] == (False, True)          # ε = 1e-1: the first epoch is rejected
    assert accepted["signal_var_half"] == (True, True) and by["signal_var_half"].signal_var == 0.5
    assert accepted["signal_var_half_rejected"] == (False,) and by["signal_var_half_rejected"].signal_var == 0.5
    c = by["odd_rank_N70"]
    assert c.r % 2 == 1 and c.N == WAVE + 6
    with open(os.path.join(CSRC, "gpt_internal.h")) as f:
        assert by["n520"].n > int(re.search(r"#define GPT_NT (\d+)", f.read()).group(1)) == 512
    assert by["rank_one"].r == 1 and by["rank_one"].Q == 1
    c = by["accepting"]
    from test_gpu_parity import _gmc_problem
    for a, b in zip(_gmc_problem(c.n, c.D, c.N, c.r, c.Q), (GC.inputs(c)[k] for k in ("phi", "y", "I"))):
        assert np.array_equal(a, b)


def test_rating_design():
    chunk = WAVE                                        # cfg_rows gathers a row's ratings 64 at a time
    for which, side_col in (("users12", 0), ("users140", 1)):
        Rating, Rtest, n1, n2, ymean, ystd = GC.design(which)
        assert (n1, n2) == ((12, 140) if which == "users12" else (140, 12)) and len(Rating) == 592
        side, other = Rating[:, side_col].astype(int) - 1, Rating[:, 1 - side_col].astype(int) - 1
        counts = np.bincount(side, minlength=12)
        assert tuple(sorted(counts)) == GC.DESIGN_COUNTS and tuple(counts) != GC.DESIGN_COUNTS
        assert {chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 2} <= set(counts)
        assert {k % 4 for k in counts} == {0, 1, 2, 3} and {k % chunk % 4 for k in counts if k > chunk} == {0, 1, 2, 3}
        for i in range(12):
            assert len(set(other[side == i])) == counts[i]
        assert len(set(zip(side, other))) == 592 and other.max() < GC.DESIGN_OTHER
        assert len(Rtest) == GC.MLG_NTEST > 256
        unrated = int(np.flatnonzero(counts == 0)[0])
        assert unrated in Rtest[:, side_col].astype(int) - 1
        assert set(Rtest[:, 0].astype(int)) == set(range(1, n1 + 1))
        assert abs(Rating[:, 2].mean()) < 1e-12 and Rating[:, 2].std(ddof=1) == pytest.approx(1.0)
    a, b = GC.design("users12")[0], GC.design("users140")[0]
    assert np.array_equal(a[:, [1, 0, 2]], b)                               # the same design, transposed
    Rating, Rtest, n1, n2, _, _ = GC.design("users3")
    assert (n1, n2, len(Rating)) == (3, 12, 16) and n1 < 4                  # fewer users than K slices
    assert len({(u, v) for u, v, _ in Rating}) == 16
    ml = cases("mlg")
    for design in ("users12", "users140"):
        assert {c.r for c in ml if c.design == design and not (c.avg or c.fixw or c.n_samples > 1)} >= {3, 4, 8, 10}
    assert 8 * 8 == WAVE and WAVE < 10 * 10 < 2 * WAVE
    assert [c.burnin for c in ml if c.avg] == [1]
    assert [c.n_samples for c in ml if c.n_samples != 1] == [2]
    assert [GC.mlg_entry(c) for c in ml if c.fixw] == ["GPT_fixw_gibbs"]
    for c in ml:
        assert c.maxepoch == 2 and 0.09 == pytest.approx(GC.MLG_SIGMA_U ** 2)
        tp = hi(c, "testpred")
        assert ((tp > 1) & (tp < 5)).sum() > tp.size // 2                    # the cut-off is not the test


def test_draw_cases():
    assert [c.p for c in cases("draw")] == [1, 5, 16, 17, 33, 100, 177, 225]
    for c in cases("draw"):
        p = GC.inputs(c)
        assert np.array_equal(p["M"], p["M"].T) and np.linalg.eigvalsh(p["M"]).min() > 0.4


@pytest.fixture(scope="module")
def cpu_runs():
    return {GC.key(c): (GC.run_numpy(c), GC.run_f64(c)) for c in GC.CASES}


def test_bars(cpu_runs):
    """B = 8·u, u the numpy restatement's largest error against mpmath per family and quantity as the
    maker measured it; B under its cap; the numpy restatement of this machine, and this suite's own
    float64 run, pass what the device is asked to pass."""
    bars, u = GC.bars(), GC.measured_u()
    for fam in GC.FAMILIES:
        qs = GC.QUANTITIES[fam]
        for i, q in enumerate(qs):
            vals = [ST[GC.key(c) + "_numpy"][i] for c in cases(fam)]
            assert u[fam][q] == np.nanmax(vals) > 0
            assert bars[fam][q] == GC.MARGIN * u[fam][q] <= GC.CAPS[fam][q], (fam, q, bars[fam][q])
        print("%-5s u = %s  B = %s" % (fam, " ".join("%.1e" % u[fam][q] for q in qs),
                                      " ".join("%.1e" % bars[fam][q] for q in qs)))
    assert GC.MARGIN == 8
    for c in GC.CASES:
        for run in cpu_runs[GC.key(c)]:
            err = GC.rel_err(c, run, GC.reference(c))
            assert set(err) == set(GC.reference(c))
            for q, e in err.items():
                assert e <= bars[c.family][q], (c.name, q, e)


# defect -> the cases that have to catch it: each passes OLD_BARS and fails its family's B there
CAUGHT_BY = {
    "prior_diag_32bit": ("ragged_q20_N131", "gemv_two_chunks_N257", "users12_r3", "users140_r4", "fixw_r4"),
    "pivot_recip": ("ragged_q20_N131", "absent_value_N13", "nr180_second_pass", "users12_r4",
                    "two_samples_r4", "p16", "p17", "p225"),
    "loo_f32_recip": ("gemv_two_chunks_N257",),
    "ktail_last_col": ("ragged_q20_N131", "absent_value_N13", "gemv_two_chunks_N257", "users12_r3",
                       "users12_r8", "users140_r10", "users3_r4", "fixw_r4"),
    "z_scaled": ("repeated_I_row", "accepting", "rejecting", "rank_one", "n520", "users140_r3", "fixw_r4",
                 "p1", "p33"),
    "energy_f32": ("n520",),
    "rhs_scaled": ("ragged_q20_N131", "n70_padded_temp", "users12_r4", "avg_burnin1_r3", "p5", "p17"),
}


@pytest.mark.parametrize("defect", sorted(GC.DEFECTS))
def test_defect_passes_the_old_bar_and_fails_the_new(defect):
    assert set(CAUGHT_BY) == set(GC.DEFECTS) and len(GC.DEFECTS) >= 6
    bars = GC.bars()
    for name in CAUGHT_BY[defect]:
        c = GC.BY_NAME[name]
        e = GC.rel_err(c, GC.run_f64(c, defect), GC.reference(c))
        old = GC.OLD_BARS[c.family]
        over = {q: v / bars[c.family][q] for q, v in e.items() if not v <= bars[c.family][q]}
        print("%s on %s: over B by %s; largest share of the old bar %.3g" % (
            defect, name, {q: "%.3g" % v for q, v in over.items()}, max(v / old[q] for q, v in e.items())))
        assert all(v <= old[q] for q, v in e.items()), (defect, name, e)
        assert over, (defect, name, e)
