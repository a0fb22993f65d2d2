"""CPU conditions of the full-theta regression sampler's step suite (tests/test_gpu_gpnt_step.py): the
committed double-double references of tests/gpnt_step_cases.py are mpmath's and belong to the inputs
this machine regenerates; every case takes the route its name says (rows per group, groups, LDS
bytes and the carry width PJ), asserted from a restatement of gpnt_layout and gpnt_carry whose
constants are the source's; every n at which a row fits finds a carry width; the bars are
8 x the numpy restatement's own error against mpmath and under their caps; the gradient's share of
the first move is at least SHARE_MIN; and seven defects planted in a group-by-group restatement of
the kernel fail the bar on the case named for them, whole and at 1e-9 of their size, where the old
1e-9 bar passes them.

Measured here (tests/golden/make_gpnt_step_golden.py, 5 s on eight processes): u per case
    pj1_full 1.9e-16   pj2_first 2.3e-16   pj2_full 2.0e-16   pj4_first 2.5e-16
    dots_one_trip 2.1e-16   dots_two_trips 2.0e-16   pj8_default 2.0e-16   pj8_full 2.2e-16
    pj12_first 3.5e-16   pj12_full 1.8e-16   pj16_first 2.0e-16   pj16_full 2.4e-16
    pj20_first 3.2e-16   pj20_last_fit 2.7e-16   nostage_ragged 2.1e-16   nostage_big 1.7e-16
    one_group_uneven 2.1e-16   wide_batch 2.3e-16   decay_store_tail 3.0e-16
    two_launches 3.2e-15 (4097 steps)   old_A 1.4e-16   old_B 3.3e-16
so B = 8·u is 1.2e-15 to 2.8e-15 on the short cases and 2.6e-14 on the 4097-step one."""
import glob
import math
import os
import re

import numpy as np
import pytest

import gpnt_ref as GR
import gpnt_step_cases as T
from oracle import philox as px
from oracle import step_cases as SC

ST = T._stored()
CSRC = os.path.join(os.path.dirname(T.GOLDEN), "..", "..", "gpt_amd", "csrc")

ROUTES = T.ROUTES


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_fixture_holds_every_case():
    others = [p for p in glob.glob(os.path.join(os.path.dirname(T.GOLDEN), "*")) if p != T.GOLDEN]
    assert os.path.getsize(T.GOLDEN) <= max(os.path.getsize(p) for p in others)
    assert os.path.getsize(T.GOLDEN) < 1024 * 1024
    assert len(T.BY_NAME) == len(T.CASES) == len(ROUTES) == 22
    sub = 0
    for c in T.CASES:
        assert str(ST[c.name + "_digest"]) == T.digest(c), c.name
        sel = T.select(c.n, c.n)
        h, l, s = ST[c.name + "_hi"], ST[c.name + "_lo"], ST[c.name + "_scale"]
        assert h.shape == l.shape == (T.kept(c), sel.size) and s.shape == (T.kept(c),), c.name
        assert h.dtype == np.float64 and l.dtype == np.float32
        assert np.isfinite(h).all() and np.isfinite(l).all() and (s >= np.abs(h).max(axis=1)).all()
        assert (np.abs(l) <= 0.5 * np.spacing(np.abs(h)) * (1 + 1e-6)).all(), c.name
        if c.n <= T.KEEP:
            assert sel.size == c.n
        else:               # both ends whole, and no stretch of the row unseen: every thread slot's
            sub += 1        # neighbourhood, every 64-lane span and every trip of the dots loop
            assert T.KEEP // 2 < sel.size <= T.KEEP + 2 * T.EDGE
            assert np.array_equal(sel[:T.EDGE], np.arange(T.EDGE))
            assert np.array_equal(sel[-T.EDGE:], np.arange(c.n - T.EDGE, c.n))
            assert np.diff(sel).max() <= 7
            assert set(sel // T.NT) == set(range(-(-c.n // T.NT)))
    assert sub == 10


def test_fixture_equals_mpmath():
    """Five cheap cases recomputed: bit for bit the stored hi + lo and scale."""
    pytest.importorskip("mpmath")
    for name in ("nostage_ragged", "one_group_uneven", "decay_store_tail", "old_A", "pj2_first"):
        c = T.BY_NAME[name]
        for s, a in T.pack(c, T.compute(c)).items():
            assert np.array_equal(a, ST[name + "_" + s]), (name, s)


def test_old_and_new_references_meet():
    """old_A and old_B are gpnt_ref.step_problem's inputs, variances, decay and seed at OLD_EPS, the
    step size at which their shares reach SHARE_MIN, so the reference here and gpnt_ref.three_steps_mp
    called at that step size differ only by the step noise: 50-digit Box–Muller here, the doubles of
    philox.normals there.  d_t = max|difference of the two draws| at step t enters theta as
    sqrt(eps_t)·d_t, and what is there already is carried on by the step's matrix
    I − eps_t/2·(I/sigma_theta² + (N/B)·Phi_B·Phi_Bᵀ/signal_var), whose max-norm is at most
    1 + eps_t/2·(1/sigma_theta² + (N/B)·‖Phi_B·Phi_Bᵀ‖∞/signal_var), taken from the inputs."""
    mp = pytest.importorskip("mpmath")
    for name in T.OLD:
        c, ref = T.BY_NAME[name], T.reference(name)
        phi, y, sv, sth, m, eps0, decay, seed = GR.step_problem(name[len("old_"):])
        assert (c.signal_var, c.sigma_theta, c.m, c.decay, c.seed) == (sv, sth, m, decay, seed)
        assert c.eps == T.OLD_EPS[name[len("old_"):]] > eps0 == GR.EPS[0]
        old = GR.three_steps_mp(phi, y, sv, sth, m, c.eps, decay, seed)
        order = np.arange(c.N)[px.randperm(c.N, seed, 0)]
        batches = [order[:m], order[m:], order[px.randperm(c.N, seed, 1)][:m]]
        bound = 0.0
        with mp.workdps(T.MP_DIGITS):
            for s, idx in enumerate(batches):
                eps = c.eps * (s + 1) ** -c.decay
                gram = np.abs(phi[:, idx] @ phi[:, idx].T).sum(axis=1).max()
                grow = 1 + eps / 2 * (1 / sth ** 2 + c.N / len(idx) * gram / sv)
                d = SC._mp_normals(c.n, seed, s, px.THETA_NOISE, 0) - \
                    np.array([mp.mpf(float(v)) for v in px.normals(c.n, seed, s, px.THETA_NOISE, 0)], dtype=object)
                bound = (grow * bound + math.sqrt(eps) * float(max(abs(v) for v in d))) * (1 + 1e-9)
                diff = max(abs(old[s][j] - (mp.mpf(float(ref["hi"][s, k])) + mp.mpf(float(ref["lo"][s, k]))))
                           for k, j in enumerate(ref["sel"]))
                print("%s step %d: references differ by %.3g, bound %.3g (growth %.3f)" % (
                    name, s + 1, float(diff), bound, grow))
                assert 0 < diff <= bound + 2.0 ** -76 * ref["scale"][s], (name, s)


def test_restated_constants_are_the_kernels():
    """kGpntMinRows, kGpntU, the carry widths and the list of instantiations, kNT, kNW, the 160 KiB
    (kMaxLds) and the 4096-step launch limit are the sources'.  The formulas of gpnt_layout are not
    matched as text: the device test compares what gpnt_last_route() reports with the restatement's
    route for every case, on both sides of each edge."""
    src = source("gpnt.hip")
    for line in ("constexpr int kGpntMinRows = kNW / 2;",
                 "constexpr int kGpntU = 32;",
                 "using GpntCarries = IntList<%s>;" % ", ".join(map(str, T.CARRIES)),
                 "IntList<0, %s>{}" % ", ".join(map(str, T.CARRIES))):
        assert line in src, line
    assert T.DOT_SPAN == 64 * 32 and T.MIN_ROWS == T.NW // 2
    nt = int(re.search(r"#define GPT_NT (\d+)", source("gpt_internal.h")).group(1))
    assert nt == T.NT and nt // 64 == T.NW
    assert "std::min<long long>(R.nb, %d)" % T.LAUNCH_STEPS in source("host_util.h")
    assert "constexpr int kMaxLds = 160 * 1024;" in source("launch_util.h") and T.LDS == 160 * 1024
    for c in T.CASES:
        L = T.gpnt_layout(c.n, c.N, c.m, c.rows)
        offs = [L[k] for k in ("o_theta", "o_idx", "o_y", "o_res", "o_flag", "o_phi")]
        assert offs == sorted(offs) and all(o % 16 == 0 for o in offs)
        assert L["base"] <= L["bytes"] <= T.LDS, c.name


def test_every_n_at_which_a_row_fits_finds_a_carry():
    """gpnt_carry returns −1 past 20·512 columns, and with_value then has nothing to launch: no n
    at which a row fits beside theta (the bookkeeping at its smallest, m = 1) may get there."""
    last = 0
    for n in range(1, 2 * T.LDS // 8):
        L = T.gpnt_layout(n, 2, 1, 1)
        if L["fit"] >= 1:
            last = n
            assert 0 < T.gpnt_carry(n) and n <= T.gpnt_carry(n) * T.NT, n
            assert n == 1 or T.gpnt_carry(n) >= T.gpnt_carry(n - 1)
    assert 10230 <= last <= T.CARRIES[-1] * T.NT
    assert T.gpnt_carry(T.CARRIES[-1] * T.NT + 1) == -1
    for pj in T.CARRIES:
        assert T.gpnt_carry(pj * T.NT) == pj and T.gpnt_carry(pj * T.NT + 1) != pj


def test_cases_take_their_routes():
    by = T.BY_NAME
    for c in T.CASES:
        assert tuple(T.route(c)) == ROUTES[c.name], (c.name, T.route(c))
        assert T.kept(c) >= 2 and (c.signal_var != 1 and c.sigma_theta != 1)
        if c.keep == 3:      # a full batch, the ragged batch, the next epoch's first
            assert c.N > c.m and T.nb(c) == 2 and T.total(c) == 4 and c.store_every == 1
    new = [c for c in T.CASES if c.name not in T.OLD]
    assert len({c.signal_var for c in new}) >= 8 and len({c.sigma_theta for c in new}) >= 12
    # all eight instantiations
    assert {ROUTES[c.name][3] for c in T.CASES} == {0} | set(T.CARRIES)
    # PJ = 16 and 20 only where the environment asks for rows
    for c in T.CASES:
        if ROUTES[c.name][3] >= 16:
            assert c.rows is not None and T.route(c, rows=None).rows == 0, c.name

    def edge(full, first, pj_full, pj_first):
        a, b = by[full], by[first]
        assert a.n == pj_full * T.NT and b.n == a.n + 1
        assert (T.route(a).pj, T.route(b).pj) == (pj_full, pj_first)
        assert pj_first * T.NT - b.n == (pj_first - pj_full) * T.NT - 1      # slots on the clamped column
    edge("pj1_full", "pj2_first", 1, 2)
    edge("pj2_full", "pj4_first", 2, 4)
    edge("dots_one_trip", "dots_two_trips", 4, 8)
    edge("pj8_full", "pj12_first", 8, 12)
    edge("pj12_full", "pj16_first", 12, 16)
    edge("pj16_full", "pj20_first", 16, 20)
    c = by["pj1_full"]
    assert c.rows is None and (c.n, c.m) == (512, 40) and c.m - T.route(c).rows == 8
    assert by["pj2_first"].m == 40 and 2 * T.NT - by["pj2_first"].n == 511
    assert by["pj2_full"].m == by["pj4_first"].m == 24 and by["pj2_full"].rows is None
    a, b = by["dots_one_trip"], by["dots_two_trips"]
    assert a.n == T.DOT_SPAN and b.n == T.DOT_SPAN + 1 and a.m == b.m == 12 and a.rows is b.rows is None
    c = by["pj8_default"]
    r = T.route(c)
    assert (c.n, c.m, c.N - c.m, c.rows) == (4000, 6, 3, None) and r.rows == 4 < T.NW
    assert c.m - r.rows == 2 and T.gpnt_layout(c.n, c.N, c.m)["fit"] == 4 == T.MIN_ROWS
    for name, rows in (("pj8_full", 3), ("pj12_first", 3), ("pj12_full", 2), ("pj16_first", 2),
                       ("pj16_full", 1), ("pj20_first", 1), ("pj20_last_fit", 1)):
        c = by[name]
        assert c.rows == rows == T.route(c).rows == T.gpnt_layout(c.n, c.N, c.m)["fit"], name
        assert T.route(c).groups >= 2 and c.m > rows
    c = by["pj20_last_fit"]
    assert (c.m, c.N) == (2, 3) and T.LDS - T.route(c).lds_bytes < 16 + 8
    assert T.gpnt_layout(c.n + 1, c.N, c.m, 1)["fit"] == 0         # one more and no row fits
    assert tuple(T.route(c, n=c.n + 1))[:2] == (0, 0)
    c = by["nostage_ragged"]
    assert (c.n, c.m, c.N - c.m, c.rows) == (70, 19, 11, 0)
    assert all(B > 8 and B % 8 for B in (c.m, c.N - c.m))          # pv[8]: neither <= 8 nor a multiple
    c = by["nostage_big"]
    assert c.rows is None and T.gpnt_layout(c.n, c.N, c.m)["fit"] == 0 and 8 * c.n > T.LDS // 2
    assert c.m > 8 and c.m % 8 and c.N - c.m < 8
    c = by["one_group_uneven"]
    assert T.route(c).rows == c.m == 13 and c.m % T.NW and c.n % 64
    c = by["wide_batch"]
    assert c.m > 64 and c.m % 64 and c.n > T.NT and T.route(c).rows % T.NW == 0
    c = by["decay_store_tail"]
    assert (T.total(c), c.store_every, T.kept(c), T.total(c) % c.store_every) == (10, 4, 2, 2)
    assert c.decay == 0.5
    c = by["two_launches"]
    assert T.nb(c) == T.LAUNCH_STEPS + 1 == 17 * c.store_every and c.epochs == 1 and c.decay == 0.3
    assert T.kept(c) * c.store_every == T.total(c)        # the last kept step is the second launch's
    assert c.eps * c.N / (2 * c.signal_var) < 0.05        # tests/test_gpu_gpnt.py's rule for m = 1
    for name in T.OLD:
        phi, y = GR.step_problem(name[len("old_"):])[:2]
        assert np.array_equal(phi, T.inputs(name)[0]) and np.array_equal(y, T.inputs(name)[1])


@pytest.fixture(scope="module")
def numpy_runs():
    return {c.name: T.run_numpy(c) for c in T.CASES}


def test_bars_and_shares(numpy_runs):
    """B = 8·u per case, u the numpy restatement's error against mpmath as the maker measured it;
    B <= 1e-14 for cases of at most ten steps and <= 1e-13 for every case; the restatement as this
    machine computes it passes what the device is asked to pass and stays under the caps.  The
    gradient's share of the first move, and its data term's, are as stored and at least SHARE_MIN on
    every case.  The restatement is held to 8·u, not to u: on the machine that made the fixture its
    error is u itself, but its matrix products are the BLAS's, and another build may sum them in
    another order; 8·u is what any fp64 evaluation of the step is asked to meet."""
    assert T.MARGIN == 8 and (T.CAP_SHORT, T.CAP, T.SHORT_STEPS, T.SHARE_MIN) == (1e-14, 1e-13, 10, 0.1)
    for c in T.CASES:
        ref = T.reference(c.name)
        e = T.error(numpy_runs[c.name], ref)
        cap = T.CAP_SHORT if T.steps(c) <= T.SHORT_STEPS else T.CAP
        print("%-18s u %.2e (here %.2e)  B %.2e  cap %g  share %.3f (data %.3f)" % (
            c.name, ref["u"], e, ref["bar"], cap, ref["share"], ref["share_g"]))
        assert 0 < ref["u"] and ref["bar"] == T.MARGIN * ref["u"] <= cap, c.name
        assert e <= ref["bar"] and T.MARGIN * e <= cap, (c.name, e)
        s, sg = T.shares(c)
        assert abs(s - ref["share"]) <= 1e-9 * s and abs(sg - ref["share_g"]) <= 1e-9 * sg
        assert min(ref["share"], ref["share_g"]) >= T.SHARE_MIN, c.name


def test_group_restatement_without_a_defect(numpy_runs):
    """The kernel's order of work, restated: within the bar of every case, and next to the
    restatement of record."""
    for c in T.CASES:
        run = T.run_groups(c)
        assert run.shape == (c.n, T.kept(c))
        assert T.error(run, T.reference(c.name)) <= T.reference(c.name)["bar"], c.name
        assert GR.rel(run, numpy_runs[c.name]) < 1e-13


# defect -> further cases that have to catch it, beside the one it is named for
ALSO = {
    "short_group_last_row_dropped": ("pj1_full", "wide_batch", "pj16_first"),
    "previous_groups_residuals": ("pj8_default", "pj12_full", "pj20_last_fit", "old_B"),
    "clamped_column_leaks": ("pj4_first", "dots_two_trips", "pj20_first"),
    "ragged_batch_N_over_m": ("nostage_big", "one_group_uneven", "old_A"),
    "eps_of_t_not_t_plus_1": ("two_launches",),
    "second_trip_column_skipped": ("pj8_default", "nostage_big"),
    "column_65_dropped": (),
}


@pytest.mark.parametrize("defect", sorted(T.DEFECTS))
def test_planted_defect_fails_the_bar(defect, numpy_runs):
    """Whole, the defect misses the bar (and may give inf); at 1e-9 of its size it passes the old
    bar, 1e-9 of max|theta| against the restatement, and still misses the new one."""
    assert set(ALSO) == set(T.DEFECTS) and len(T.DEFECTS) == 7 and T.SMALL == 1e-9
    for name in (T.DEFECTS[defect],) + ALSO[defect]:
        c, ref = T.BY_NAME[name], T.reference(name)
        whole = T.error(T.run_groups(c, defect), ref)
        small_run = T.run_groups(c, defect, size=T.SMALL)
        old, small = GR.rel(small_run, numpy_runs[name]), T.error(small_run, ref)
        print("%s on %s: whole %.3g x B; at 1e-9 %.3g of the old bar, %.3g x B" % (
            defect, name, whole / ref["bar"], old / T.OLD_BAR, small / ref["bar"]))
        assert not whole <= ref["bar"], (defect, name, whole)
        assert whole > 1e3 * ref["bar"]
        assert old < T.OLD_BAR, (defect, name, old)
        assert small > ref["bar"], (defect, name, small, ref["bar"])
