"""CPU conditions of the full-theta softmax tests (tests/test_gpu_ctheta.py; cases, references and
measures in tests/ctheta_cases.py; fixture tests/golden/ctheta_mp.npz).  No GPU.

  fixture       it belongs to the inputs this machine regenerates (digests), stays under 500 kB,
                |lo| <= ulp(hi)/2, and the smallest entry of every sampler family recomputed with
                mpmath equals the stored hi + lo bit for bit
  tiling        the tile-walk table of part A from cjoint_ref.cjoint_layout, the LDS staging decision
                of ntc_layout for the class sampler's shapes, hmc_blocks for the leapfrog's shapes
  conditioning  every input double moved to a neighbouring double moves no stored output by more
                than COND_MAX = 1e-14 (dH in units of max(|H0|, 1))
  bars          u recomputed on this machine, B = 8·u <= 1e-13, and the restatements pass every
                stored bar (the self-check); the decision margins of the HMC references
  mutants       nine defects of the restatements pass the present comparisons (1e-9 on theta,
                1e-9·max(|H0|, 1) on H, dH and value) and exceed B

Measured by tests/golden/make_ctheta_golden.py (60 s on eight processes; 190 s of references:
12 s, 27 s and 55 s of mpmath for the walk cases n = 33, N = 8230; n = 33, N = 16485 and n = 700,
N = 2053, 2 s of long double for n = 330, N = 4100, 38 s for the 12 HMC transitions with L = 8,
19 s for the leapfrog on N = 8230, under 10 s each for the rest):
    family  quantities      u                                 B = 8·u
    cls     theta           4.7e-16                           3.7e-15
    lang    theta           1.4e-15                           1.1e-14
    leap    q p H dH        3.2e-16 5.2e-16 3.7e-16 4.8e-16   2.6e-15 4.2e-15 3.0e-15 3.9e-15
    hmc     theta value dH  5.9e-16 4.7e-16 3.4e-16           4.8e-15 3.7e-15 2.7e-15
    wlang   theta           6.0e-17                           4.8e-16
    wleap   q p H dH        9.9e-16 9.8e-15 4.7e-16 4.2e-16   7.9e-15 7.8e-14 3.8e-15 3.4e-15
Step-1 shares 0.52 to 0.73 (class sampler, eps = 1 and 1.5) and 0.54 to 1.00 (Langevin); the worst
conditioning figure is 1.4e-15 (the leapfrog on N = 8230).  Mutants, worst error / B at the stated
size: softmax 1.8e5, residual 1.3e5, ragged 2.2e5, plustheta 3.0e5, lasthalf 6.4e3, gradcol 2.8e4,
kin 2.7e5, prior 166; sqrteps at 1e-9 moves theta by more than 1e-9 in the decay case (the present
comparison catches it) and is shown at 1e-10: 3.2e4.
"""
import os

import numpy as np
import pytest

import chmc_ref as H
import cjoint_ref as CR
import cls_ref as CLS
import ctheta_cases as T

SAMPLERS = [e for e in T.ENTRIES if e[0] != "walk"]
PRESENT = 1e-9

def test_fixture_belongs_to_these_inputs_and_is_small():
    assert os.path.getsize(T.GOLDEN) < 500_000
    st = T._stored()
    for e in T.ENTRIES:
        assert str(st[T.key(e) + "_digest"]) == T.digest(e), T.key(e)
    pairs = [k for k in st if k.endswith("_hi")]
    assert len(pairs) > 100
    for k in pairs:
        hi, lo = st[k], st[k[:-3] + "_lo"].astype(np.float64)
        assert hi.dtype == np.float64 and st[k[:-3] + "_lo"].dtype == np.float32
        assert (np.abs(lo) <= np.spacing(np.abs(hi)) / 2).all(), k
    for e in SAMPLERS:                                   # the recorded step-1 shares
        share = st[T.key(e) + "_meas"][1]
        if e[0] in ("cls", "lang"):
            assert 0.5 <= share <= 2.0, (T.key(e), share)


@pytest.mark.parametrize("e", [("cls", 2), ("lang", "g3", 0, 3), ("leap", "g3", 1),
                               ("hmc", "g3", 3, 1e-2, 3, 1.0)], ids=T.key)
def test_smallest_entries_recomputed_bit_for_bit(e):
    pytest.importorskip("mpmath")
    st = T._stored()
    packed = T.pack(e, T.compute(e))
    assert packed
    for s, a in packed.items():
        assert np.array_equal(a, st[T.key(e) + "_" + s]), s


def test_tiling():
    print("\n  case (n, N, D, C)          TI  tiles  nblk  theta in LDS  tiles per workgroup   last tile")
    for k, (case, (TI, tiles)) in enumerate(zip(T.WALK, T.WALK_TABLE)):
        n, N, D, C, form = case
        L = CR.cjoint_layout(n, N, C)
        per = np.bincount(np.arange(L["ntiles"]) % L["nblk"], minlength=L["nblk"])
        last = N - (L["ntiles"] - 1) * L["TI"]
        print("  %-26s %3d  %5d  %4d  %-12s  %d x %d, %d x %d %12d columns"
              % (case[:4], L["TI"], L["ntiles"], L["nblk"], L["theta_lds"], (per == per.max()).sum(),
                 per.max(), (per == per.min()).sum(), per.min(), last))
        assert (L["TI"], L["ntiles"], L["nblk"]) == (TI, tiles, 256)
        assert per.max() >= 2 and L["bytes"] <= CR.CJ_LDS
        assert (L["ntiles"] - 1) % L["nblk"] != L["ntiles"] - 1         # the ragged tile is no first pass
        if k == 0:
            assert list(per[:3]) == [2, 2, 1] and last == 6
        if k == 1:
            assert list(per[:5]) == [3, 3, 3, 3, 2] and per[4:].max() == 2
        if k == 2:
            assert last == 5 and L["theta_lds"]
        if k == 3:
            assert not L["theta_lds"]
    # the golden cases stay on one tile per workgroup: the walk is new ground
    assert all(CR.cjoint_layout(c[0], c[1], c[3])["ntiles"] <= 256 for c in CR.CASES)
    for case, stage in zip(T.CLS_CASES, T.CLS_STAGE):
        n, m, C = case[:3]
        L = T.ntc_layout(n, C, m)
        print("  ntc_layout n = %d, C = %d, m = %d: CC %d, staged %s, %d bytes" % (n, C, m, L["CC"], L["stage"], L["bytes"]))
        assert L["stage"] == stage and L["bytes"] <= 160 * 1024
    assert T.ntc_layout(40, 20, 10)["CC"] == 32 and T.ntc_layout(33, 16, 7)["CC"] == 16
    blocks = {name: T.hmc_blocks(T.problem(name).n, T.problem(name).C) for name, _ in T.LEAP}
    print("  hmc_blocks:", blocks)
    assert blocks == dict(g0=1, g1=1, g3=2, g4=3, e512=1, e513=2, w0=1)
    assert T.problem("e512").n * T.problem("e512").C == T.NT
    assert T.problem("e513").n * T.problem("e513").C == T.NT + 1


@pytest.mark.parametrize("e", SAMPLERS, ids=T.key)
def test_conditioning(e):
    base = T.run_numpy(e)
    worst = max(max(T.moves(e, base, T.run_numpy(e, perturb_seed=s)).values()) for s in range(3))
    print("%s: a neighbouring double of every input moves the outputs by %.2e" % (T.key(e), worst))
    assert worst <= T.COND_MAX


def literal_too(e):
    return not (e[0] == "hmc" and e[4] > 3)       # tests/golden/make_ctheta_golden.py's rule


def test_bars_and_self_check():
    """u of the restatements recomputed here; B = 8·u <= 1e-13; the stored bars are 8 x the stored
    u; and the restatements pass every bar the device is asked to pass."""
    bars, stored_u = T.bars(), T.measured_u()
    u = {f: dict.fromkeys(q, 0.0) for f, q in T.FAMILIES.items()}
    for e in SAMPLERS:
        ref = T.reference(e)
        runs = [T.run_numpy(e)]
        if e[0] == "cls":
            runs.append(T.run_numpy(e, literal=True))
        elif literal_too(e):
            runs.append(T.run_numpy(e, pot=T.pot_literal))
        for run in runs:
            f = T.family(e)
            if f[0] == "w" and run is not runs[0]:
                print("  %s, literal form (not in u): %s" % (T.key(e), T.errors(e, run, ref)))
                continue
            for q, v in T.errors(e, run, ref).items():
                assert v <= bars[f][q], (T.key(e), q, v)
                u[f][q] = max(u[f][q], v)
    print()
    for f, qs in T.FAMILIES.items():
        print("  %-5s %s" % (f, "  ".join("%s: u %.2e (stored %.2e), B %.2e" % (q, u[f][q], stored_u[f][q], bars[f][q])
                                          for q in qs)))
        for q in qs:
            assert bars[f][q] == T.MARGIN * stored_u[f][q] and stored_u[f][q] > 0
            assert T.MARGIN * u[f][q] <= T.B_MAX and bars[f][q] <= T.B_MAX


def test_decision_margins_and_both_outcomes():
    """From the references alone: every Metropolis decision of the HMC entries lies at least
    MARGIN_MIN from its threshold at 50 digits, so the device test compares every one of them; the
    12-transition entry holds both outcomes."""
    for e in T.ENTRIES:
        if e[0] != "hmc":
            continue
        ref = T.reference(e)
        print("%s: accept %s, smallest margin %.3g" % (T.key(e), ref["accept"], ref["margin"].min()))
        assert ref["margin"].min() >= H.MARGIN_MIN
        assert np.array_equal(ref["accept"], T.run_numpy(e)["accept"])
    both = T.reference(("hmc",) + T.HMC[-1])["accept"]
    assert 0 < both.sum() < both.size


@pytest.mark.parametrize("name,L", T.LEAP, ids=lambda v: str(v))
def test_back_reference_returns_to_the_start(name, L):
    """The back leapfrog's reference, started from the doubles nearest (q, -p_new), is (theta, -p)
    with H0 and H1 exchanged, within the family's bars: held to its own reference, the device has
    come back."""
    e = ("leap", name, L)
    P, ref, B = T.problem(name), T.reference(e), T.bars()[T.family(e)]
    scale = max(abs(ref["bH"][0][0]), 1.0)
    err = {}
    for q, want in (("q", T.flat(P.theta)), ("p", -T.flat(T.leap_momentum(name, L)))):
        hi, lo = ref["b" + q]
        err[q] = np.abs((want[ref["sel"]["b" + q]] - hi[0]) - lo[0]).max() / np.abs(hi[0]).max()
    err["H"] = np.abs((ref["bH"][0] - ref["H"][0][::-1]) + (ref["bH"][1] - ref["H"][1][::-1])).max() / scale
    err["dH"] = np.abs((ref["bdH"][0] + ref["dH"][0]) + (ref["bdH"][1] + ref["dH"][1])).max() / scale
    print("%s: back reference against (theta, -p): %s" % (T.key(e), "  ".join("%s %.2e" % kv for kv in err.items())))
    for q, v in err.items():
        assert v <= B[q], (q, v, B[q])


def test_hooked_restatements_are_the_modules_own():
    for k in range(len(T.CLS_CASES)):
        n, m, C, tail, decay, sigma = T.CLS_CASES[k]
        phi, y = T.cls_inputs(k)
        for c, (seed, fac) in enumerate(T.CLS_CHAINS):
            want = CLS.gpnt_sgld_class(phi, y, sigma, m, T.CLS_EPS * fac, decay, 0, 2, seed, ncls=C)
            assert np.array_equal(T.cls_run(k, c), np.moveaxis(want, -1, 0)[:T.STEPS])
    P = T.problem("g0")
    p0 = T.leap_momentum("g0", 2)
    a = T.leapfrog(P, P.theta, 1e-2, 2, p0)
    b = H.leapfrog(*P.args(), 1e-2, 2, p0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    mine, theirs = T.hmc_run(P, P.theta, 1e-2, 2, 3), H.hmc(*P.args(), 1e-2, 2, 3, T.SEED)
    assert np.array_equal(np.moveaxis(mine["store"], 0, -1), theirs["store"])
    for k in ("accept", "H0", "dH", "value"):
        assert np.array_equal(mine[k], theirs[k]), k


MUTANTS = [(m, "cls") for m in T.CLS_MUTANTS] + [(m, "leap hmc") for m in T.HMC_MUTANTS]


@pytest.mark.parametrize("mut,families", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutant_passes_the_present_comparison_and_fails_the_bar(mut, families, monkeypatch):
    """The defect at its stated size (ctheta_cases.MUT_SIZE), and a tenth and a hundredth of it where
    the stated size is already caught at 1e-9: at least one entry where the present comparison
    passes and a bar B is exceeded."""
    stated = T.MUT_SIZE[mut]
    bars = T.bars()
    entries = [e for e in SAMPLERS if e[0] in families.split() and literal_too(e)]
    base = {e: T.run_numpy(e) for e in entries}
    for size in ([None] if stated is None else [stated, stated / 10, stated / 100]):
        if size is not None:
            monkeypatch.setitem(T.MUT_SIZE, mut, size)
        caught, excess = [], 0.0
        for e in entries:
            run = T.run_numpy(e, mut=mut)
            present = max(T.moves(e, base[e], run).values())
            over = max(v / bars[T.family(e)][q] for q, v in T.errors(e, run, T.reference(e)).items())
            if present <= PRESENT and over > 1.0:
                caught.append(T.key(e))
                excess = max(excess, over)
        print("mutant %-9s size %s: passes 1e-9 and exceeds B in %d of %d entries, worst error / B = %.3g"
              % (mut, size, len(caught), len(entries), excess))
        if caught:
            break
    assert caught, mut
