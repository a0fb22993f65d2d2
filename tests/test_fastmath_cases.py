"""CPU conditions of the noise-path suite (tests/test_gpu_fastmath.py): the input sets of
oracle/fastmath_cases.py reach every branch of the functions they feed, the committed double-double
references are mpmath's, and numpy's own log / sqrt / cos / sin — the formulas of philox.normals
and philox.unoise_quads — stay within the bars the device is held to, on the same inputs, so the
reference alone passes what the device is asked to pass."""
import os

import numpy as np
import pytest

from oracle import fastmath_cases as FC
from oracle import philox as P


# ------------------------------------------------------------------------------- branch coverage
def test_u53_stays_inside_the_open_interval():
    """(k + 1/2)·2^-53 is a tie from k = 2^52 up; the all-ones k used to round to 1.0."""
    lo, hi = FC.u53_extremes()
    assert lo == 2.0 ** -54
    assert hi == 1.0 - 2.0 ** -53 and hi < 1.0
    o = np.full(1, 0xFFFFFFFF, np.uint32)
    near = P._u53(o, o - np.uint32(64))[0]            # k = 2^53 − 2: the tie rounds down to even
    assert near == (2.0 ** 53 - 2) * 2.0 ** -53
    assert P._u32(np.array([0, 0xFFFFFFFF], np.uint32)).tolist() == [2.0 ** -33, 1 - 2.0 ** -33]


def test_log_inputs_reach_every_branch():
    x = FC.log_inputs()
    e, folded, f = FC.log_decomp(x)
    assert x.min() < 2.0 ** -54 and x.max() > 1.0 and 1.0 in x
    # every exponent the uniforms can take, with both sides of the mantissa fold at each
    for k in range(-54, 0):
        assert (folded & (e == k)).any() and (~folded & (e == k)).any(), k
    # the fold itself: the constant (kept), its successor (folded)
    m = np.ldexp(FC.FOLD, -3)
    assert m in x and np.nextafter(m, 1.0) in x and np.nextafter(m, 0.0) in x
    assert f.min() >= np.sqrt(0.5) - 1 - 1e-16 and f.max() <= FC.FOLD - 1
    assert (f == 0).any() and (f < 0).any() and (f > 0).any()
    for w in FC.EDGE_WORDS:
        assert FC.u32(np.array([w]))[0] in x
    assert all(v in x for v in FC.u53_extremes())
    r = FC.radius_inputs()
    assert r.max() < 1.0 and r.size >= x.size - 3
    # the smallest squared radius is far below the [2e-10, 46] the fm_sqrt_pos comment names
    assert -2.0 * np.log(r.max()) < 3e-16


def test_sqrt_and_rcp_inputs():
    x = FC.sqrt_inputs()
    assert x.min() > 0 and x.min() < 1e-16 and x.max() > 46.0
    e = np.frexp(x)[1]
    assert (e % 2 == 0).any() and (e % 2 == 1).any()
    for k in range(-26, 3):
        v = 4.0 ** k
        assert v in x and np.nextafter(v, 0) in x and np.nextafter(v, 100) in x
    assert np.isin(-2.0 * FC.reference("log")[0][FC.log_inputs() < 1], x).all()
    d = FC.rcp_inputs()
    assert d.min() >= 2 + (np.sqrt(0.5) - 1) - 1e-15 and d.max() <= 1 + FC.FOLD and 2.0 in d


def test_sincos_inputs_reach_every_branch():
    u = FC.sincos_inputs()
    q, f, n = FC.sincos_decomp(u)
    assert u.min() == 0.0 and u.max() == 1.0
    for quad in range(4):
        assert ((q == quad) & (f < 0)).any() and ((q == quad) & (f > 0)).any()
        assert ((q == quad) & (f == 0)).any()
    assert (n == 4).any() and (q[n == 4] == 0).all()          # rint(4u) = 4 is quadrant 0
    assert 1.0 - 2.0 ** -53 in u and n[u == 1.0 - 2.0 ** -53][0] == 4
    ties = np.abs(f) == 0.5
    assert sorted(u[ties].tolist()) == [0.125, 0.375, 0.625, 0.875]
    # rint rounds a tie to even: down at 0.5 and 2.5, up at 1.5 and 3.5
    assert sorted(n[ties].tolist()) == [0, 2, 2, 4]
    assert (f[ties] > 0).sum() == 2 and (f[ties] < 0).sum() == 2
    for k in range(33):
        v = k / 32.0
        assert v in u
        assert k == 0 or np.nextafter(v, 0) in u
        assert k == 32 or np.nextafter(v, 1) in u
    assert np.isin(np.arange(16) / 256.0, u).all() and 2.0 ** -54 in u
    assert np.abs(f).max() == 0.5


def test_tab_words_reach_every_table_index_and_both_ends():
    x = FC.tab_words()
    ih, il, low = FC.tab_decomp(x)
    for want in (0, 0xFFFFFF):
        seen = {(int(a), int(b)) for a, b in zip(ih[low == want], il[low == want])}
        assert len(seen) == 256
    mid = (low != 0) & (low != 0xFFFFFF)
    assert len({(int(a), int(b)) for a, b in zip(ih[mid], il[mid])}) == 256
    assert 0 in x and 0xFFFFFFFF in x


def test_stream_cases_cover_the_seed_and_counter_families():
    cs = FC.stream_cases()
    for s in FC.SEEDS:
        mine = [c for c in cs if c[0] == s]
        assert any(c[1] == 0 for c in mine)
        assert any(c[1] + c[2] == 2 ** 31 for c in mine) and any(c[1] + c[2] == 2 ** 32 for c in mine)
        assert {c[3] for c in mine} >= {0, 2 ** 32 - 1}
    assert {c[4] for c in cs} == set(FC.STREAM_IDS)
    assert sum(s >= 2 ** 32 for s in FC.SEEDS) >= 3 and FC.BIG_SEED in FC.SEEDS
    # a seed and its low word give different words (the key's second word is seed >> 32)
    c = (FC.BIG_SEED, 0, 4, 0, P.W_NOISE, 0)
    assert not np.array_equal(FC.case_words(c), FC.case_words((FC.BIG_SEED & 0xFFFFFFFF,) + c[1:]))
    w = FC.all_stream_words()
    assert w.shape == (sum(c[2] for c in cs), 4) and w.dtype == np.uint32


def test_known_answer_vectors_are_the_oracles():
    for ctr, key, want in FC.KAT:
        got = P.philox4x32(*[np.array([c], np.uint32) for c in ctr], key[0] | (key[1] << 32))
        assert tuple(int(g[0]) for g in got) == want


# ---------------------------------------------------------------------------- fixture vs mpmath
def test_fixture_holds_every_reference_set():
    st = FC._stored()
    assert os.path.getsize(FC.GOLDEN) < 1 << 20
    for key in FC.KEYS:
        assert str(st[key + "_digest"]) == FC.digest(key), key
        assert st[key + "_hi"].dtype == np.float64 and st[key + "_lo"].dtype == np.float32
        hi, lo = FC.reference(key)
        assert np.isfinite(hi).all() and np.isfinite(lo).all()
        assert (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)) * (1 + 1e-6)).all(), key


@pytest.mark.parametrize("key", FC.KEYS)
def test_fixture_equals_mpmath(key):
    pytest.importorskip("mpmath")
    hi, lo = FC._compute(key)
    shi, slo = FC.reference(key)
    assert np.array_equal(hi, shi) and np.array_equal(lo, slo)


# ------------------------------------------------------------------- numpy's formulas in the bars
def _report(name, worst, bar):
    print("numpy %s: worst %.3f (bar %g)" % (name, worst, bar))
    assert worst <= bar, (name, worst, bar)


def test_numpy_log_sqrt_rcp_within_the_bars():
    _report("log ulp", FC.err_ulp(np.log(FC.log_inputs()), FC.reference("log")).max(), FC.BAR_LOG_ULP)
    _report("sqrt ulp", FC.err_ulp(np.sqrt(FC.sqrt_inputs()), FC.reference("sqrt")).max(),
            FC.BAR_SQRT_ULP)
    _report("rcp ulp", FC.err_ulp(1.0 / FC.rcp_inputs(), FC.reference("rcp")).max(), FC.BAR_RCP_ULP)
    u = FC.radius_inputs()
    _report("radius ulp", FC.err_ulp(np.sqrt(-2.0 * np.log(u)), FC.reference("radius")).max(),
            FC.BAR_RADIUS_ULP)


def test_numpy_normals_within_the_stream_bar():
    """philox.normals and philox.unoise_quads against Box–Muller in mpmath of the same words, on
    every stream case that starts at block 0 (the two take no first block), at the device's bar
    for the polynomial forms."""
    pz, prad = FC.reference("pair_z"), FC.reference("pair_rad")
    qz, qrad = FC.reference("quad_z"), FC.reference("quad_rad")
    worst_p = worst_q = 0.0
    for case, sl in zip(FC.stream_cases(), FC.case_slices()):
        seed, c0, nb, c1, c2, c3 = case
        if c0 != 0:
            continue
        z = P.normals(2 * nb, seed, c1, c2, c3)
        ref = (pz[0][2 * sl.start:2 * sl.stop], pz[1][2 * sl.start:2 * sl.stop])
        bar = 2.0 ** -52 * np.repeat(prad[0][sl], 2)
        worst_p = max(worst_p, (FC.err_abs(z, ref) / bar).max())
        # unoise_quads with n = 256, r = 1: NQ = 1 and blocks c0 = λ < 64 give rows λ + 64·i
        nq = min(nb, 64)
        zq = P.unoise_quads(256, 1, seed, c1, c2, c3)[:, 0].reshape(4, 64)[:, :nq].T.ravel()
        a = 4 * sl.start
        ref = (qz[0][a:a + 4 * nq], qz[1][a:a + 4 * nq])
        bar = 2.0 ** -52 * np.repeat(qrad[0][2 * sl.start:2 * sl.start + 2 * nq], 2)
        worst_q = max(worst_q, (FC.err_abs(zq, ref) / bar).max())
    _report("normals, units of 2^-52·rad", worst_p, 2 + FC.T_POLY + 1)
    _report("unoise_quads, units of 2^-52·rad", worst_q, 2 + FC.T_POLY + 1)


def test_numpy_formula_within_the_stream_bar_on_every_block():
    """The formula itself on the words of every stream case, the top of the counter range included
    (philox.normals and philox.unoise_quads take no first block)."""
    w = FC.all_stream_words()
    with np.errstate(all="raise"):
        u1, u2 = P._u53(w[:, 0], w[:, 1]), P._u53(w[:, 2], w[:, 3])
        rad, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        z = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=1).ravel()
        bar = 2.0 ** -52 * np.repeat(FC.reference("pair_rad")[0], 2)
        _report("pair formula, units of 2^-52·rad", (FC.err_abs(z, FC.reference("pair_z")) / bar).max(),
                2 + FC.T_POLY + 1)
        u = FC.u32(w)
        rad, th = np.sqrt(-2.0 * np.log(u[:, 0::2])), 2.0 * np.pi * u[:, 1::2]
        z = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=2).ravel()
        bar = 2.0 ** -52 * np.repeat(FC.reference("quad_rad")[0], 2)
        _report("quad formula, units of 2^-52·rad", (FC.err_abs(z, FC.reference("quad_z")) / bar).max(),
                2 + FC.T_POLY + 1)


# |fl(2π·u) − 2πu| <= ½ulp(θ) + u·|fl(2π) − 2π| <= 2^-51 + 2.45e-16 = 6.21·2^-53 for θ < 8, and libm's
# sin / cos add half an ulp of a value below 1
NUMPY_ANGLE_ABS = 6.21 + 0.5


def test_numpy_sincos_error_is_the_angle_rounding():
    """numpy's sin / cos of fl(2π·u), the oracle's form of the angle, does NOT meet the 2·2^-53
    absolute bar fm_sincos_2pi_c is held to: the product 2π·u is rounded to a double before the
    sine sees it, which alone moves the angle by up to 6.21·2^-53 (measured here: 6.16 on the
    polynomial's inputs).  fm_sincos_2pi_c reduces 4u exactly and has no such term.  So this one
    comparison holds numpy to the bound of its own angle rounding; the normals it makes are held
    to the device's stream bar above, which they meet (3.1 of 5)."""
    u = FC.sincos_inputs()
    th = 2.0 * np.pi * u
    for name, val, key in (("sin", np.sin(th), "sin"), ("cos", np.cos(th), "cos")):
        _report(name + " abs 2^-53", FC.err_abs53(val, FC.reference(key)).max(), NUMPY_ANGLE_ABS)
    x = FC.tab_words()
    th = 2.0 * np.pi * FC.u32(x)
    for name, val, key in (("sin", np.sin(th), "tab_sin"), ("cos", np.cos(th), "tab_cos")):
        _report("tab words " + name + " abs 2^-53", FC.err_abs53(val, FC.reference(key)).max(),
                NUMPY_ANGLE_ABS)
