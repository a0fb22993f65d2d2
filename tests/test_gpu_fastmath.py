"""The device's noise path against mpmath, through gpt_debug_fastmath and gpt_debug_normals: the
Philox words, u53 / u32u, fm_log_c, fm_sqrt_pos, fm_rcp, fm_sincos_2pi_c, fm_sincos_tab2 with its
LDS table, and the six normal generators on top of them (gpt_amd/csrc/fastmath.h, gpt_common.h).

Inputs, branch coverage and the mpmath references (50 digits, committed as double-double pairs
under tests/golden/) come from oracle/fastmath_cases.py; tests/test_fastmath_cases.py checks on the
CPU that every branch is reached and that numpy's formulas meet the same bars.  Errors are in ulps
of the true value unless "absolute" (units of 2^-53) is said.  The bars are the header's claims:

  fm_log_c <= 2 ulp          fm_rcp <= 1 ulp         fm_sqrt_pos <= 1 ulp        radius <= 2 ulp
  fm_sincos_2pi_c <= 2 ulp and <= 2 absolute; exact 0, ±1 at u = k/4; within 1 ulp of √½ at odd k/8
  fm_sincos_tab2 <= 4 absolute against the truth, <= 3 absolute against the device's fm_sincos_2pi_c
  table entries <= 1 ulp, the entries that are 0 or ±1 exact
  normals: |z − z_mp| <= (2 + T + 1)·2^-52·rad_mp, T = 2 (polynomial forms), 4 (table forms)

The worst measured values are printed, and recorded in DESIGN.md §4.  No output may be NaN or Inf.
"""
import functools

import numpy as np
import pytest

from oracle import fastmath_cases as FC
from oracle import philox as P

pytestmark = pytest.mark.gpu


def fastmath(fn, x=None, xi=None, count=None):
    """(out0, out1) of gpt_debug_fastmath; the outputs start as NaN."""
    from gpt_amd import _lib
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float64)
    if xi is not None:
        xi = np.ascontiguousarray(xi, dtype=np.uint32)
    if count is None:
        count = x.size if x is not None else (xi.size // 2 if fn == FC.FN_U53 else xi.size)
    o0, o1 = np.full(count, np.nan), np.full(count, np.nan)
    _lib.check(_lib.lib().gpt_debug_fastmath(
        fn, count, x.ctypes.data_as(_lib.P_D) if x is not None else None,
        xi.ctypes.data_as(_lib.P_U32) if xi is not None else None,
        o0.ctypes.data_as(_lib.P_D), o1.ctypes.data_as(_lib.P_D)))
    return o0, o1


def normals(gen, case):
    """(z, words) of gpt_debug_normals for a stream case: z (nblocks, 2 or 4), words (nblocks, 4)."""
    from gpt_amd import _lib
    seed, c0, nb, c1, c2, c3 = case
    per = 4 if gen in (FC.GEN_QUAD4, FC.GEN_QUAD_TAB4) else 2
    z = np.full((nb, per), np.nan)
    w = np.zeros((nb, 4), dtype=np.uint32)
    _lib.check(_lib.lib().gpt_debug_normals(gen, seed, c0, nb, c1, c2, c3, z.ctypes.data_as(_lib.P_D),
                                            w.ctypes.data_as(_lib.P_U32)))
    return z, w


def report(name, worst, bar):
    print("fastmath error: %s worst %.3f (bar %g)" % (name, worst, bar))
    assert worst <= bar, (name, worst, bar)


@functools.lru_cache(maxsize=None)
def device_sincos():
    return fastmath(FC.FN_SINCOS, x=FC.sincos_inputs())


# ------------------------------------------------------------------------------ words and uniforms
@pytest.mark.parametrize("gen", [FC.GEN_PAIR, FC.GEN_HOST], ids=["device", "host"])
def test_philox_known_answers(gen):
    """The Random123 vectors of tests/test_oracle.py::test_philox_known_answers, on the device's and
    on the host C++'s philox4x32."""
    for ctr, key, want in FC.KAT:
        _, w = normals(gen, (key[0] | (key[1] << 32), ctr[0], 1, ctr[1], ctr[2], ctr[3]))
        assert tuple(int(v) for v in w[0]) == want


@pytest.mark.parametrize("gen", [FC.GEN_AT, FC.GEN_PAIR, FC.GEN_QUAD4, FC.GEN_QUAD2, FC.GEN_QUAD_TAB4,
                                 FC.GEN_QUAD_TAB2, FC.GEN_HOST])
def test_philox_words_equal_the_oracle(gen):
    """Every seed (three of them above 2^32) and counter family, bit for bit; normal_at's range
    ends at c0 = 2^31 − 1, so the cases above are refused for it."""
    from gpt_amd import _lib
    ran = 0
    for case in FC.stream_cases():
        if gen == FC.GEN_AT and case[1] + case[2] > FC.TOP31:
            z, w = np.zeros((case[2], 2)), np.zeros((case[2], 4), dtype=np.uint32)
            code = _lib.lib().gpt_debug_normals(gen, *case, z.ctypes.data_as(_lib.P_D),
                                                w.ctypes.data_as(_lib.P_U32))
            assert code == _lib.GPT_ERR_BAD_DIMS
            continue
        _, w = normals(gen, case)
        assert np.array_equal(w, FC.case_words(case)), case
        ran += 1
    assert ran >= 2 * len(FC.SEEDS) + len(FC.STREAM_IDS)


def test_u53_and_u32u_bit_for_bit():
    w = FC.all_stream_words()
    edge = np.array(FC.EDGE_WORDS, dtype=np.uint32)
    a = np.concatenate([w[:, 0], w[:, 2], np.repeat(edge, edge.size)])
    b = np.concatenate([w[:, 1], w[:, 3], np.tile(edge, edge.size)])
    got, _ = fastmath(FC.FN_U53, xi=np.stack([a, b], axis=1).ravel())
    assert np.array_equal(got, P._u53(a, b))
    assert got.min() == 2.0 ** -54 and got.max() == 1.0 - 2.0 ** -53          # never 0, never 1
    x = np.concatenate([w.ravel(), edge])
    got, _ = fastmath(FC.FN_U32, xi=x)
    assert np.array_equal(got, P._u32(x))
    # the host's u53, on the stream cases
    for case in FC.stream_cases()[:3]:
        z, wd = normals(FC.GEN_HOST, case)
        assert np.array_equal(z[:, 0], P._u53(wd[:, 0], wd[:, 1]))
        assert np.array_equal(z[:, 1], P._u53(wd[:, 2], wd[:, 3]))


# -------------------------------------------------------------------------- functions vs mpmath
def test_log_against_mpmath():
    got, _ = fastmath(FC.FN_LOG, x=FC.log_inputs())
    assert np.isfinite(got).all()
    report("fm_log_c ulp", FC.err_ulp(got, FC.reference("log")).max(), FC.BAR_LOG_ULP)


def test_rcp_against_mpmath():
    got, _ = fastmath(FC.FN_RCP, x=FC.rcp_inputs())
    assert np.isfinite(got).all()
    report("fm_rcp ulp", FC.err_ulp(got, FC.reference("rcp")).max(), FC.BAR_RCP_ULP)


def test_sqrt_against_mpmath():
    got, _ = fastmath(FC.FN_SQRT, x=FC.sqrt_inputs())
    assert np.isfinite(got).all()
    report("fm_sqrt_pos ulp", FC.err_ulp(got, FC.reference("sqrt")).max(), FC.BAR_SQRT_ULP)


def test_radius_against_mpmath():
    """fm_sqrt_pos(−2·fm_log_c(u)) as the generators form it, down to the squared radius 2.2e-16 of
    the largest u53; and the same value from the two entries one after the other."""
    u = FC.radius_inputs()
    got, _ = fastmath(FC.FN_RADIUS, x=u)
    assert np.isfinite(got).all() and (got > 0).all()
    report("radius ulp", FC.err_ulp(got, FC.reference("radius")).max(), FC.BAR_RADIUS_ULP)
    lg, _ = fastmath(FC.FN_LOG, x=u)
    two, _ = fastmath(FC.FN_SQRT, x=-2.0 * lg)
    assert np.array_equal(two, got)


def test_sincos_against_mpmath():
    u = FC.sincos_inputs()
    sn, cs = device_sincos()
    assert np.isfinite(sn).all() and np.isfinite(cs).all()
    rs, rc = FC.reference("sin"), FC.reference("cos")
    report("fm_sincos_2pi_c sin abs 2^-53", FC.err_abs53(sn, rs).max(), FC.BAR_SINCOS_ABS)
    report("fm_sincos_2pi_c cos abs 2^-53", FC.err_abs53(cs, rc).max(), FC.BAR_SINCOS_ABS)
    # at u = k/4 exactly 0 and ±1 (the sign of a zero is free)
    for k in range(5):
        i = int(np.flatnonzero(u == k / 4.0)[0])
        assert (sn[i], cs[i]) == [(0, 1), (1, 0), (0, -1), (-1, 0), (0, 1)][k], (k, sn[i], cs[i])
    # at odd k/8 both within 1 ulp of √½
    for k in (1, 3, 5, 7):
        i = int(np.flatnonzero(u == k / 8.0)[0])
        assert FC.err_ulp(sn[i:i + 1], (rs[0][i:i + 1], rs[1][i:i + 1]))[0] <= 1.0
        assert FC.err_ulp(cs[i:i + 1], (rc[0][i:i + 1], rc[1][i:i + 1]))[0] <= 1.0
        assert abs(abs(sn[i]) - np.sqrt(0.5)) <= np.spacing(0.5)
    report("fm_sincos_2pi_c sin ulp", FC.err_ulp(sn, rs).max(), FC.BAR_SINCOS_ULP)
    report("fm_sincos_2pi_c cos ulp", FC.err_ulp(cs, rc).max(), FC.BAR_SINCOS_ULP)


def test_sincos_tab2_against_mpmath_and_the_polynomial():
    x = FC.tab_words()
    sn, cs = fastmath(FC.FN_SINCOS_TAB2, xi=x)
    assert np.isfinite(sn).all() and np.isfinite(cs).all()
    report("fm_sincos_tab2 sin abs 2^-53", FC.err_abs53(sn, FC.reference("tab_sin")).max(),
           FC.BAR_TAB2_ABS)
    report("fm_sincos_tab2 cos abs 2^-53", FC.err_abs53(cs, FC.reference("tab_cos")).max(),
           FC.BAR_TAB2_ABS)
    ps, pc = fastmath(FC.FN_SINCOS, x=FC.u32(x))
    report("fm_sincos_tab2 − fm_sincos_2pi_c, sin abs 2^-53", np.abs(sn - ps).max() * 2.0 ** 53,
           FC.BAR_TAB2_VS_POLY_ABS)
    report("fm_sincos_tab2 − fm_sincos_2pi_c, cos abs 2^-53", np.abs(cs - pc).max() * 2.0 ** 53,
           FC.BAR_TAB2_VS_POLY_ABS)


def test_lds_table_entries():
    """tab[2j], tab[2j+1] = (sin, cos)(2πj/16), tab[32+2j], tab[33+2j] = (sin, cos)(2πj/256)."""
    tab, _ = fastmath(FC.FN_TABLE, count=64)
    u = FC.sincos_inputs()
    rs, rc = FC.reference("sin"), FC.reference("cos")
    worst = 0.0
    for i in range(32):
        v = (i & 15) / (16.0 if i < 16 else 256.0)
        k = int(np.flatnonzero(u == v)[0])
        for got, ref in ((tab[2 * i], rs), (tab[2 * i + 1], rc)):
            r = (ref[0][k:k + 1], ref[1][k:k + 1])
            if r[0][0] in (0.0, 1.0, -1.0):
                assert got == r[0][0], (i, got)
            worst = max(worst, FC.err_ulp(np.array([got]), r)[0])
    report("table entries ulp", worst, FC.BAR_TABLE_ULP)
    assert np.array_equal(tab[0:2], [0, 1]) and np.array_equal(tab[32:34], [0, 1])
    assert np.array_equal(np.abs(tab[8:10]), [1, 0]) and np.array_equal(np.abs(tab[16:18]), [0, 1])


# --------------------------------------------------------------------------- streams vs mpmath
GENS = {"normal_at": (FC.GEN_AT, "pair", FC.T_POLY), "normal_pair": (FC.GEN_PAIR, "pair", FC.T_POLY),
        "normal_quad4": (FC.GEN_QUAD4, "quad", FC.T_POLY), "normal_quad2": (FC.GEN_QUAD2, "quad", FC.T_POLY),
        "normal_quad_tab4": (FC.GEN_QUAD_TAB4, "quad", FC.T_TAB),
        "normal_quad_tab2": (FC.GEN_QUAD_TAB2, "quad", FC.T_TAB)}


@pytest.mark.parametrize("name", sorted(GENS))
def test_normals_against_mpmath(name):
    """Box–Muller in mpmath of the oracle's words, per the generator's contract (u53 pairs, or u32u
    words); every seed and counter family, the block at c0 = 2^32 − 1 included (2^31 − 1 for
    normal_at).  The <2> forms give the first pair of the quad."""
    gen, contract, T = GENS[name]
    zr, rr = FC.reference(contract + "_z"), FC.reference(contract + "_rad")
    nz = 2 if contract == "pair" else 4          # reference values per block
    worst, ran = 0.0, 0
    for case, sl in zip(FC.stream_cases(), FC.case_slices()):
        if gen == FC.GEN_AT and case[1] + case[2] > FC.TOP31:
            continue
        z, _ = normals(gen, case)
        assert np.isfinite(z).all(), case
        per = z.shape[1]
        hi = zr[0][nz * sl.start:nz * sl.stop].reshape(-1, nz)[:, :per]
        lo = zr[1][nz * sl.start:nz * sl.stop].reshape(-1, nz)[:, :per]
        rad = rr[0][(nz // 2) * sl.start:(nz // 2) * sl.stop].reshape(-1, nz // 2)[:, :per // 2]
        bar = 2.0 ** -52 * np.repeat(rad, 2, axis=1)
        worst = max(worst, (FC.err_abs(z, (hi, lo)) / bar).max())
        ran += 1
    assert ran >= 2 * len(FC.SEEDS) + len(FC.STREAM_IDS)
    report("%s, units of 2^-52·rad" % name, worst, 2 + T + 1)


@pytest.mark.parametrize("name", sorted(GENS))
def test_normals_element_mapping(name):
    """Which output is which element: against philox.normals (element 2·c0 the cosine, 2·c0 + 1 the
    sine) and philox.unoise_quads (rows λ + 64·(4q + i) of column l from block (l·NQ + q)·64 + λ),
    far tighter than the distance between two different normals."""
    gen, contract, T = GENS[name]
    seed, c1 = FC.BIG_SEED, 7
    if contract == "pair":
        nb = 40
        z, _ = normals(gen, (seed, 0, nb, c1, P.W_NOISE, 0))
        want = P.normals(2 * nb, seed, c1, P.W_NOISE, 0)
        assert np.abs(z.ravel() - want).max() < 1e-13
        assert np.abs(z.ravel()[1:] - want[:-1]).min() > 1e-6
    else:
        n, r, k = 300, 2, 3                       # NQ = 2: blocks (l·2 + q)·64 + λ
        nq = 2
        want = P.unoise_quads(nq * 256, r, seed, c1, P.U_NOISE, k)
        z, _ = normals(gen, (seed, 0, r * nq * 64, c1, P.U_NOISE, k))
        for l in range(r):
            for q in range(nq):
                for i in range(z.shape[1]):
                    rows = np.arange(64) + 64 * (4 * q + i)
                    got = z[(l * nq + q) * 64:(l * nq + q + 1) * 64, i]
                    assert np.abs(got - want[rows, l]).max() < 1e-13, (l, q, i)
        assert np.array_equal(P.unoise_quads(n, r, seed, c1, P.U_NOISE, k), want[:n])
    # the last block of the counter range, against the formula on the oracle's words
    top = FC.TOP31 if gen == FC.GEN_AT else FC.TOP32
    z, w = normals(gen, (seed, top - 1, 1, c1, P.U_NOISE, 1))
    x = np.stack(P.philox4x32(np.array([top - 1], dtype=np.uint32), c1, P.U_NOISE, 1, seed), axis=1)
    assert np.array_equal(w, x)
    if contract == "pair":
        u1, u2 = P._u53(x[:, 0], x[:, 1]), P._u53(x[:, 2], x[:, 3])
    else:
        u1, u2 = P._u32(x[:, 0::2]), P._u32(x[:, 1::2])
    rad, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    want = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1).ravel()[:z.shape[1]]
    assert np.abs(z.ravel() - want).max() < 1e-13


# ------------------------------------------------------------------------------- argument checks
def test_bad_arguments():
    from gpt_amd import _lib
    L = _lib.lib()
    x = np.ones(4)
    xi = np.ones(8, dtype=np.uint32)
    o = np.zeros(64)
    px, pxi, po = x.ctypes.data_as(_lib.P_D), xi.ctypes.data_as(_lib.P_U32), o.ctypes.data_as(_lib.P_D)
    bad = _lib.GPT_ERR_BAD_DIMS
    assert L.gpt_debug_fastmath(9, 4, px, pxi, po, po) == bad           # unknown fn
    assert L.gpt_debug_fastmath(-1, 4, px, pxi, po, po) == bad
    assert L.gpt_debug_fastmath(FC.FN_LOG, 0, px, pxi, po, po) == bad
    assert L.gpt_debug_fastmath(FC.FN_LOG, 4, None, pxi, po, po) == bad
    assert L.gpt_debug_fastmath(FC.FN_U32, 4, px, None, po, po) == bad
    assert L.gpt_debug_fastmath(FC.FN_SINCOS, 4, px, pxi, po, None) == bad
    assert L.gpt_debug_fastmath(FC.FN_LOG, 4, px, pxi, None, po) == bad
    assert L.gpt_debug_fastmath(FC.FN_TABLE, 32, None, None, po, None) == bad
    assert b"gpt_debug_fastmath" in L.gpt_last_error()
    z = np.zeros(16)
    w = np.zeros(16, dtype=np.uint32)
    pz, pw = z.ctypes.data_as(_lib.P_D), w.ctypes.data_as(_lib.P_U32)
    assert L.gpt_debug_normals(7, 0, 0, 4, 0, 0, 0, pz, pw) == bad       # unknown gen
    assert L.gpt_debug_normals(FC.GEN_PAIR, 0, 0, 0, 0, 0, 0, pz, pw) == bad
    assert L.gpt_debug_normals(FC.GEN_PAIR, 0, 2 ** 32 - 3, 4, 0, 0, 0, pz, pw) == bad
    assert L.gpt_debug_normals(FC.GEN_AT, 0, 2 ** 31 - 3, 4, 0, 0, 0, pz, pw) == bad
    assert L.gpt_debug_normals(FC.GEN_PAIR, 0, 0, 4, 0, 0, 0, None, pw) == bad
    assert L.gpt_debug_normals(FC.GEN_PAIR, 0, 0, 4, 0, 0, 0, pz, None) == bad
    assert b"gpt_debug_normals" in L.gpt_last_error()
    assert L.gpt_debug_normals(FC.GEN_PAIR, 0, 2 ** 32 - 4, 4, 0, 0, 0, pz, pw) == _lib.GPT_OK
