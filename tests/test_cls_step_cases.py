"""CPU conditions of the full-theta softmax sampler's step suite (tests/test_gpu_cls_step.py): the
committed double-double references of tests/cls_step_cases.py are mpmath's and belong to the inputs
this machine regenerates; every case is on the side of each edge of ntc_chain_kernel that its name
says, asserted from a restatement of ntc_layout and from the inputs (CC, stage, bytes against
160 KiB, steps per epoch against the 4096 of a launch, batch columns against the waves, saturated
logits, the gradient's share of the move); the bars are 8 x the numpy restatement's own error against
mpmath and under their caps; five defects of 1e-9 and below pass the old bar (1e-9 of max|theta|) and
fail these on named cases, and two gross ones fail where they must.

Measured here (tests/golden/make_cls_step_golden.py, 8 s on eight processes, 20 s on one): u per case
    cc32_min 4.6e-16   cc32_full 2.7e-16   one_class 1.6e-16   absent_classes 1.1e-16
    stage_last 1.4e-16   stage_first_off 1.4e-16   theta_fills_lds 1.6e-16   saturated 2.7e-16
    wide_batch 1.1e-16   two_launches 2.7e-15 (4097 steps)   store_tail 2.4e-16
    old_*: 3.8e-16, 3.9e-16, 1.2e-16, 2.0e-16, 7.4e-17, 1.5e-16 in cls_ref.SAMPLER_CASES' order
so B = 8·u is 5.9e-16 to 3.7e-15 on the short cases and 2.2e-14 on the 4097-step one."""
import os
import re

import numpy as np
import pytest

import cls_ref as CLS
import cls_step_cases as T
import ctheta_cases

ST = T._stored()
CSRC = os.path.join(os.path.dirname(T.GOLDEN), "..", "..", "gpt_amd", "csrc")
WAVE = 64


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def layout(c, n=None):
    return T.ntc_layout(c.n if n is None else n, c.C, c.m)


def test_fixture_holds_every_case():
    assert os.path.getsize(T.GOLDEN) < 500 * 1000
    assert len(T.BY_NAME) == len(T.CASES) == 17
    for c in T.CASES:
        assert str(ST[c.name + "_digest"]) == T.digest(c), c.name
        sel = T.select(c.n, c.n * c.C)
        h, l, s = ST[c.name + "_hi"], ST[c.name + "_lo"], ST[c.name + "_scale"]
        assert h.shape == l.shape == (T.kept(c), sel.size) and s.shape == (T.kept(c),), c.name
        assert h.dtype == np.float64 and l.dtype == np.float32
        assert np.isfinite(h).all() and np.isfinite(l).all() and (s >= np.abs(h).max(axis=1)).all()
        assert (np.abs(l) <= 0.5 * np.spacing(np.abs(h)) * (1 + 1e-6)).all(), c.name
        # whole steps but where theta fills LDS; there both ends and every row and class column
        if c.name != "theta_fills_lds":
            assert sel.size == c.n * c.C
        else:
            assert T.KEEP // 2 < sel.size <= T.KEEP + 2 * T.EDGE
            assert set(sel % c.n) == set(range(c.n)) and set(sel // c.n) == set(range(c.C))
            assert sel[0] == 0 and sel[-1] == c.n * c.C - 1


def test_fixture_equals_mpmath():
    """Three small cases recomputed: bit for bit the stored hi + lo and scale."""
    pytest.importorskip("mpmath")
    for name in ("one_class", "absent_classes", "store_tail"):
        c = T.BY_NAME[name]
        for s, a in T.pack(c, T.compute(c)).items():
            assert np.array_equal(a, ST[name + "_" + s]), (name, s)


def test_layout_restatement_is_the_kernels():
    """The formula is cls.hip's, term for term; kNW and the 160 KiB (kMaxLds) and 4096-step limits
    (the launch loop the full-theta chains share, host_util.h) are the sources'; and it agrees with
    the restatement tests/ctheta_cases.py already holds."""
    src = source("cls.hip")
    for line in ("L.CC = C <= 2 ? 2 : (C <= 4 ? 4 : (C <= 8 ? 8 : (C <= 16 ? 16 : 32)));",
                 "L.o_theta = o; o = al16(o + 8 * (size_t)n * L.CC);",
                 "L.o_idx = o;   o = al16(o + 4 * (size_t)m);",
                 "L.o_yb = o;    o = al16(o + 4 * (size_t)m);",
                 "L.o_P = o;     o = al16(o + 8 * (size_t)C * m);",
                 "L.o_flag = o;  o = al16(o + 4 * (size_t)kNW);",
                 "const size_t staged = al16(o + 8 * (size_t)n * m);",
                 "L.stage = staged <= (size_t)kMaxLds ? 1 : 0;",
                 "L.bytes = L.stage ? staged : o;"):
        assert line in src, line
    hdr = source("gpt_internal.h")
    nt = int(re.search(r"#define GPT_NT (\d+)", hdr).group(1))
    assert nt // WAVE == T.NW
    assert "std::min<long long>(R.nb, %d)" % T.LAUNCH_STEPS in source("host_util.h")
    assert "S.run(R, " in source("api_cls.hip")
    assert "constexpr int kMaxLds = 160 * 1024;" in source("launch_util.h")
    assert "L.bytes > (size_t)kMaxLds" in source("api_cls.hip") and T.LDS == 160 * 1024
    for c in T.CASES:
        L = layout(c)
        assert {k: L[k] for k in ("CC", "stage", "bytes")} == ctheta_cases.ntc_layout(c.n, c.C, c.m)
        offs = [L[k] for k in ("o_theta", "o_idx", "o_yb", "o_P", "o_flag", "o_phi")]
        assert offs == sorted(offs) and all(o % 16 == 0 for o in offs) and L["bytes"] >= L["base"]


def test_cases_reach_the_edges():
    by = T.BY_NAME
    assert {layout(c)["CC"] for c in T.CASES} == {2, 4, 8, 16, 32}
    for c in T.CASES:
        assert layout(c)["bytes"] <= T.LDS and T.kept(c) >= 2, c.name
        yi, C = CLS.check_labels(T.inputs(c.name)[1], c.C)
        assert C == c.C
    c = by["cc32_min"]
    assert c.C == 17 and layout(c)["CC"] == 32
    assert T.ntc_layout(c.n, 16, c.m)["CC"] == 16                  # 17 is the smallest C of the build
    assert c.n % WAVE and c.N % c.m == 3 and T.total(c) == 6 and layout(c)["stage"]
    assert set(T.inputs(c.name)[1]) == set(range(1, 18))
    c = by["cc32_full"]
    assert c.C == 32 == layout(c)["CC"] and c.n < WAVE and T.total(c) == 6
    assert set(T.inputs(c.name)[1]) == set(range(1, 33))            # GPNT_SGLDclass finds C = 32 itself
    c = by["one_class"]
    assert c.C == 1 and layout(c)["CC"] == 2 and set(T.inputs(c.name)[1]) == {1.0}
    p = T.run_f64(c, probe="first")
    assert not p["P"].any()                                         # P ≡ 0: prior and noise only
    c = by["absent_classes"]
    assert set(T.inputs(c.name)[1]) == {2.0, 3.0} and c.C == 5 and layout(c)["CC"] == 8
    # an absent class's column sees no −1: its gradient's data term is a sum of positive P·phi
    p = T.run_f64(c, probe="first")
    assert (p["P"][[0, 3, 4]] > 0).all() and (p["P"][[1, 2]] < 0).any()
    c, d = by["stage_last"], by["stage_first_off"]
    assert c._replace(name="", n=0, idx=0) == d._replace(name="", n=0, idx=0) and d.n == c.n + 1
    assert layout(c)["stage"] and layout(c)["bytes"] == 163664 and T.LDS - 163664 == 176
    assert not layout(d)["stage"] and T.ntc_layout(d.n, d.C, d.m)["base"] + 8 * d.n * d.m > T.LDS
    assert layout(d)["bytes"] == layout(d)["base"] == 6496
    assert c.m == WAVE and c.N % c.m == 3                           # a full batch and one of 3
    c = by["theta_fills_lds"]
    L = layout(c)
    assert 8 * c.n * L["CC"] == 161280 and L["CC"] == 32 == c.C and not L["stage"]
    assert L["bytes"] == 161600 <= T.LDS < L["bytes"] + 8 * c.n * c.m
    assert T.ntc_layout(T.REFUSED_N, c.C, c.m)["bytes"] > T.LDS == 8 * T.REFUSED_N * 32
    c = by["saturated"]
    p = T.run_f64(c, probe="first")
    print("saturated: max|x| at step 1 = %.1f" % p["xmax"])
    assert p["xmax"] > T.SATURATION > 709.79                        # exp overflows from 709.79
    P = p["softmax"]
    sat = P.max(axis=0) == 1.0                        # 0 or 1 to the last bit: the others below 2^-53
    print("saturated: %d of %d columns have P = 1 exactly, %d entries are exact zeros" % (
        sat.sum(), sat.size, (P == 0.0).sum()))
    assert sat.sum() >= 0.8 * sat.size and (np.sort(P[:, sat], axis=0)[:-1] < 2.0 ** -53).all()
    assert (P == 0.0).any()                                         # exp(x − lse) underflows
    assert layout(c)["CC"] == 4
    c = by["wide_batch"]
    assert c.m == c.N == 96 > WAVE and c.m > T.NW and c.m % T.NW == 0 and layout(c)["CC"] == 8
    assert c.decay == 0.5 and T.total(c) == 2
    c = by["two_launches"]
    assert T.nb(c) == T.LAUNCH_STEPS + 1 == 17 * c.store_every and c.epochs == 1
    assert T.kept(c) * c.store_every == T.total(c)        # the last kept step is the second launch's
    assert c.decay == 0.3
    c = by["store_tail"]
    assert T.total(c) == 10 and c.store_every == 4 and T.kept(c) == 2 and T.total(c) % c.store_every == 2
    # more batch columns than waves and fewer; a batch wider than N
    assert {c.m > T.NW for c in T.CASES} == {True, False} and any(c.m > c.N for c in T.CASES)
    # the six cases of tests/test_gpu_cls.py, with its inputs
    old = [c for c in T.CASES if c.name.startswith("old_")]
    assert len(old) == len(CLS.SAMPLER_CASES)
    for idx, (c, case) in enumerate(zip(old, CLS.SAMPLER_CASES)):
        phi, y, eps = CLS.sampler_inputs(case, idx)
        assert np.array_equal(phi, T.inputs(c.name)[0]) and np.array_equal(y, T.inputs(c.name)[1])
        assert (c.n, c.N, c.C, c.m, c.epochs, c.decay, c.sigma, c.eps) == case[:4] + (case[4] + case[5],) + case[6:] + (eps,)


def test_gradient_share():
    """Where eps is EPS_LARGE the gradient's part of the first move, eps/2·rms(grad), is within a
    factor of ten of the noise's, sqrt(eps)·rms(xi); at the sampler_inputs step size it is not,
    but for the saturated case, whose gradient is theta of size 500."""
    shares = {c.name: T.share(c) for c in T.CASES if T.total(c) <= 20}
    print("gradient share at step 1: %s" % {k: "%.3g" % v for k, v in shares.items()})
    large = [c.name for c in T.CASES if c.eps == T.EPS_LARGE]
    assert large == ["cc32_min"]
    for name in large + ["saturated"]:
        assert shares[name] >= T.SHARE_MIN, (name, shares[name])
    assert shares["cc32_full"] < T.SHARE_MIN


@pytest.fixture(scope="module")
def numpy_runs():
    return {c.name: T.run_numpy(c) for c in T.CASES}


def test_hooked_restatement_is_the_modules_own(numpy_runs):
    for c in T.CASES:
        assert numpy_runs[c.name].shape == (c.n, c.C, T.kept(c))
        if T.total(c) <= 20:
            assert np.array_equal(T.run_f64(c), numpy_runs[c.name]), c.name


def test_bars(numpy_runs):
    """B = 8·u per case, u the numpy restatement's error against mpmath as the maker measured it;
    B <= 1e-14 for cases of at most ten steps and <= 1e-13 for every case; the restatement as this
    machine computes it passes what the device is asked to pass and stays under the caps."""
    assert T.MARGIN == 8 and (T.CAP_SHORT, T.CAP, T.SHORT_STEPS) == (1e-14, 1e-13, 10)
    for c in T.CASES:
        ref = T.reference(c.name)
        e = T.error(numpy_runs[c.name], ref)
        cap = T.CAP_SHORT if T.total(c) <= T.SHORT_STEPS else T.CAP
        print("%-30s u %.2e (here %.2e)  B %.2e  cap %g" % (c.name, ref["u"], e, ref["bar"], cap))
        assert 0 < ref["u"] and ref["bar"] == T.MARGIN * ref["u"] <= cap, c.name
        assert e <= ref["bar"] and T.MARGIN * e <= cap, (c.name, e)
        assert CLS.rel(numpy_runs[c.name], numpy_runs[c.name]) == 0.0


# defect -> the cases that have to catch it
CAUGHT_BY = {
    "P_scaled": ("cc32_min", "stage_last", "old_150_203_7_50_0_2_0_1"),
    "prior_scaled": ("one_class", "saturated", "theta_fills_lds", "two_launches"),
    "NB_scaled": ("cc32_min", "stage_first_off", "old_70_130_3_25_1_2_0.1_1"),
    "sqrt_eps_scaled": ("cc32_full", "wide_batch", "store_tail", "two_launches"),
    "noise_scaled": ("one_class", "absent_classes", "old_20_10_2_50_0_2_0_1"),
}
GROSS = {"short_batch_N_over_m": "cc32_min", "no_max_shift": "saturated"}


@pytest.mark.parametrize("defect", sorted(CAUGHT_BY))
def test_small_defect_passes_the_old_bar_and_fails_the_new(defect, numpy_runs):
    assert set(CAUGHT_BY) | set(GROSS) == set(T.DEFECTS) and len(CAUGHT_BY) >= 5
    assert 0 < T.DEFECTS[defect] <= 1e-9
    for name in CAUGHT_BY[defect]:
        c, ref = T.BY_NAME[name], T.reference(name)
        run = T.run_f64(c, defect)
        old, e = CLS.rel(run, numpy_runs[name]), T.error(run, ref)
        print("%s on %s: %.3g of the old bar, %.3g x B" % (defect, name, old / T.OLD_BAR, e / ref["bar"]))
        assert old < T.OLD_BAR, (defect, name, old)
        assert e > ref["bar"], (defect, name, e, ref["bar"])


@pytest.mark.parametrize("defect", sorted(GROSS))
def test_gross_defect_fails(defect):
    name = GROSS[defect]
    assert T.DEFECTS[defect] is None
    e = T.error(T.run_f64(T.BY_NAME[name], defect), T.reference(name))
    print("%s on %s: %.3g x B" % (defect, name, e / T.reference(name)["bar"]))
    assert not e <= T.reference(name)["bar"]


def test_theta_past_lds_is_refused_before_any_device_work():
    """theta_fills_lds' shape at n = 640 needs no device to be refused: GPT_ERR_BAD_DIMS from the
    layout, like tests/test_cls_ref.py's bad arguments."""
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    c = T.BY_NAME["theta_fills_lds"]
    phi, y = T.inputs(c.name)
    phi = np.asfortranarray(np.resize(phi, (T.REFUSED_N, c.N)))
    with pytest.raises(_lib.GPTError) as e:
        G.GPNT_SGLDclass_chains(phi, y, c.sigma, c.m, [c.eps], c.decay, 0, c.epochs, [T.SEED], ncls=c.C)
    assert e.value.code == _lib.GPT_ERR_BAD_DIMS and "160 KiB" in str(e.value)
