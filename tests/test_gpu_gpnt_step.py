"""The full-theta regression sampler on the device (gpnt_chain_kernel<PJ>, gpt_amd/csrc/gpnt.hip, and
gpnt_step_kernel, gpt_amd/csrc/feature.hip) against mpmath at rounding level, at every carry width,
on every route and at the sizes where the kernels clamp an index or take a second trip.

Every case of tests/gpnt_step_cases.py runs through GPT_SGLD.GPNT_SGLD_chains (one chain, the case's
store_every and its GPTSGLD_GPNT_ROWS, unset where the case has none); the route the library reports
has to be the one tests/test_gpnt_step_cases.py derives from its restatement of gpnt_layout, and every
held step is within B·max|theta| of the 50-digit reference of tests/golden/gpnt_step_mp.npz.  The
reference draws its step noise by Box–Muller in mpmath on the Philox integers, so no allowance for
the device's normals is added.  Each case's route (rows per group, groups, LDS bytes, PJ) is
gpnt_step_cases.ROUTES' row; what it reaches:

    pj1_full          n = 512: every thread's one column live; groups of 32 and 8
    pj2_first         n = 513: 511 threads' second slot reads the clamped column
    pj2_full          n = 1024
    pj4_first         n = 1025
    dots_one_trip     n = 2048: one trip of the dots loop, every load live
    dots_two_trips    n = 2049: the second trip has one live lane
    pj8_default       n = 4000: groups of 4 and 2, then a batch of 3; default route
    pj8_full          n = 4096, rows = 3
    pj12_first        n = 4097, rows = 3
    pj12_full         n = 6144, rows = 2
    pj16_first        n = 6145, rows = 2
    pj16_full         n = 8192, rows = 1
    pj20_first        n = 8193, rows = 1
    pj20_last_fit     n = 10234, rows = 1: 16 bytes of LDS left; at 10235 no row fits
    nostage_ragged    n = 70, rows = 0: the pv[8] pass with 19 and 11 rows
    nostage_big       n = 10300: theta is half the LDS, batches of 9 and 2
    one_group_uneven  n = 130: 13 staged rows over 8 waves
    wide_batch        n = 600, batches of 70 and 5: groups of 32, 32 and 6; the
                      second 64-column pass of gpnt_step_kernel
    decay_store_tail  10 steps, decay 0.5, store_every = 4: 2 kept, the tail unsaved
    two_launches      4097 steps in the epoch: launches of 4096 and 1, decay 0.3
    old_A, old_B      gpnt_ref.step_problem's inputs, variances and seed at eps = 5e-4 and 4e-3

B = 8·u per case, u the error of the numpy restatement against the same reference
(tests/golden/make_gpnt_step_golden.py measures it; tests/test_gpnt_step_cases.py holds B <= 1e-14 up
to ten steps and <= 1e-13 always, and shows seven planted defects failing B at 1e-9 of their size).
The margin of 8 is tests/test_gpu_step.py's.  Every case's step size is large enough for the
gradient to make at least a tenth of the first move.

A run with several groups is also repeated with GPTSGLD_GPNT_ROWS=0 and has to be equal bit for bit:
route identity at every PJ.  The cases of at most ten steps with store_every = 1 also run through
GPNT_SGLD, which launches gpnt_step_kernel once per step.  That theta past 160 KiB is refused before
any launch is tests/test_gpnt_ref.py::test_c_entries_refuse_bad_dimensions_without_a_device's.

Measured (u by the maker; device error / B as this file prints it, MI355X):
    case               u         B = 8·u   chains  GPNT_SGLD
    pj1_full           1.89e-16  1.51e-15  0.089   0.089
    pj2_first          2.27e-16  1.82e-15  0.087   0.087
    pj2_full           2.02e-16  1.62e-15  0.089   0.089
    pj4_first          2.45e-16  1.96e-15  0.074   0.087
    dots_one_trip      2.07e-16  1.66e-15  0.105   0.105
    dots_two_trips     2.04e-16  1.63e-15  0.086   0.086
    pj8_default        1.95e-16  1.56e-15  0.083   0.083
    pj8_full           2.22e-16  1.77e-15  0.072   0.072
    pj12_first         3.48e-16  2.79e-15  0.050   0.050
    pj12_full          1.75e-16  1.40e-15  0.128   0.128
    pj16_first         2.01e-16  1.61e-15  0.097   0.097
    pj16_full          2.35e-16  1.88e-15  0.068   0.068
    pj20_first         3.19e-16  2.55e-15  0.049   0.042
    pj20_last_fit      2.67e-16  2.13e-15  0.076   0.056
    nostage_ragged     2.08e-16  1.67e-15  0.112   0.112
    nostage_big        1.67e-16  1.34e-15  0.121   0.121
    one_group_uneven   2.14e-16  1.71e-15  0.048   0.048
    wide_batch         2.33e-16  1.86e-15  0.092   0.092
    decay_store_tail   3.03e-16  2.42e-15  0.056   -
    two_launches       3.21e-15  2.57e-14  0.081   -
    old_A              1.44e-16  1.15e-15  0.085   0.085
    old_B              3.28e-16  2.63e-15  0.083   0.083
The two-chain run gives two_launches' figure again (0.081).  Every route printed is the table's, and every
grouped run equals its GPTSGLD_GPNT_ROWS=0 run bit for bit.  59 tests, 3 s on MI355X.
"""
import numpy as np
import pytest

import gpnt_step_cases as T

pytestmark = pytest.mark.gpu

ROWS_ENV = "GPTSGLD_GPNT_ROWS"
ROUTES = T.ROUTES
IDS = [c.name for c in T.CASES]
GROUPED = [c for c in T.CASES if ROUTES[c.name][1] > 1]
SINGLE = [c for c in T.CASES if c.store_every == 1 and T.total(c) <= T.SHORT_STEPS]


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@pytest.fixture(autouse=True)
def no_rows_cap(monkeypatch):
    monkeypatch.delenv(ROWS_ENV, raising=False)


def run_chains(c, monkeypatch, seeds=None, rows=-1):
    """(store (n, stored, chains), status) of the case; rows: another GPTSGLD_GPNT_ROWS than its own."""
    rows = c.rows if rows == -1 else rows
    if rows is None:
        monkeypatch.delenv(ROWS_ENV, raising=False)
    else:
        monkeypatch.setenv(ROWS_ENV, str(rows))
    phi, y = T.inputs(c.name)
    seeds = [c.seed] if seeds is None else list(seeds)
    return G().GPNT_SGLD_chains(phi, y, c.signal_var, c.sigma_theta, c.m, c.eps, c.decay, 0, c.epochs,
                                seeds, store_every=c.store_every)


def hold(c, store, what="chains"):
    """Shape, finiteness and every held step within B; prints device error / B."""
    ref = T.reference(c.name)
    assert store.shape == (c.n, T.total(c) // c.store_every)
    assert np.isfinite(store).all()
    err = T.step_errors(store[:, :T.kept(c)], ref)
    print("%-18s %-6s u %.2e  B %.2e  device error / B %.3f (%.2e)" % (
        c.name, what, ref["u"], ref["bar"], err.max() / ref["bar"], err.max()))
    assert (err <= ref["bar"]).all(), (c.name, err / ref["bar"])


@pytest.mark.parametrize("c", T.CASES, ids=IDS)
def test_chain_sampler_against_mpmath(c, monkeypatch):
    store, status = run_chains(c, monkeypatch)
    route = G().gpnt_last_route()
    print("%-18s route %s PJ %d" % (c.name, route, ROUTES[c.name][3]))
    assert status.shape == (1,) and status[0] == 0 and store.shape[2] == 1
    assert (route["rows"], route["groups"], route["lds_bytes"]) == ROUTES[c.name][:3]
    hold(c, store[:, :, 0])


@pytest.mark.parametrize("c", GROUPED, ids=[c.name for c in GROUPED])
def test_grouped_route_equals_the_unstaged_one(c, monkeypatch):
    """The same doubles whether g is carried in PJ registers over the groups or formed in one go
    from memory: every listed PJ against gpnt_chain_kernel<0>."""
    assert {ROUTES[c.name][3] for c in GROUPED} == set(T.CARRIES)
    base, status = run_chains(c, monkeypatch)
    assert status[0] == 0 and G().gpnt_last_route()["groups"] == ROUTES[c.name][1]
    flat, status = run_chains(c, monkeypatch, rows=0)
    route = G().gpnt_last_route()
    assert status[0] == 0 and (route["rows"], route["groups"]) == (0, 0), route
    assert base.any() and np.array_equal(flat, base)


@pytest.mark.parametrize("c", SINGLE, ids=[c.name for c in SINGLE])
def test_single_step_kernel_against_mpmath(c):
    """GPNT_SGLD itself: gpnt_step_kernel, one launch per step, 64 batch columns per pass."""
    assert "wide_batch" in [c.name for c in SINGLE]
    phi, y = T.inputs(c.name)
    hold(c, G().GPNT_SGLD(phi, y, c.signal_var, c.sigma_theta, c.m, c.eps, c.decay, 0, c.epochs, c.seed),
         "single")


def test_launch_boundary_is_per_chain(monkeypatch):
    """Two chains across the 4096-step boundary in one call: theta goes to HBM and comes back per
    chain, so each equals its own single run bit for bit, and the first is the case itself."""
    c = T.BY_NAME["two_launches"]
    seeds = (c.seed, T.SIBLING_SEED)
    store, status = run_chains(c, monkeypatch, seeds)
    assert not status.any() and store.shape == (c.n, T.kept(c), 2)
    hold(c, store[:, :, 0], "pair")
    for k, seed in enumerate(seeds):
        alone, st = run_chains(c, monkeypatch, (seed,))
        assert st[0] == 0 and np.array_equal(alone[:, :, 0], store[:, :, k]), k
    assert not np.array_equal(store[:, :, 0], store[:, :, 1])
