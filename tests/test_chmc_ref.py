"""CPU tests of the HMC restatement (tests/chmc_ref.py), which the device tests of
tests/test_gpu_chmc.py are held to: the L = 1 transition against the reference's literal MALA
lines, reversibility of the integrator, the decision margins of every device case, and the
declarations of the new entry points."""
import math
import os
import re

import numpy as np
import pytest

import chmc_ref as H
import cls_ref as CLS
from oracle import philox as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("idx", [0, 3])
def test_one_leapfrog_step_is_the_literal_mala_iteration(idx):
    """BloodTransfusionExperiment.jl:261-265 line by line, with the literal (per-row loop) value
    and gradient, against the restatement at L = 1: the proposal, the end momentum, the
    acceptance probability and the decision.  Both are fp64 evaluations of the same expressions
    in another order, so they agree to rounding: 1e-12 relative (the two gradient forms agree to
    a few 1e-15 of the largest entry at these shapes, N <= 130 terms per sum)."""
    g = H.golden_case(idx)
    h, eps, t = g["H"][H.POINT], 1e-2, 4
    args = (g["X"], g["y"], g["Z"], g["b"], g["theta"], h)
    th, prop, mom_prop, accept_prob, acc = H.mala_literal(*args, eps, H.SEED, t)
    n, C = g["theta"].shape
    p = H.momentum(n, C, H.SEED, t)
    q, p1, H0, H1, _, _ = H.leapfrog(*args, eps, 1, p)
    assert CLS.rel(q, prop) < 1e-12
    assert CLS.rel(p1.ravel(order="F"), mom_prop) < 1e-12
    assert abs(math.exp(H0 - H1) - accept_prob) <= 1e-9 * accept_prob   # |H| ~ 1e2..1e3 in the exponent
    r = H.hmc(*args, eps, 1, 1, H.SEED, t0=t)
    assert bool(r["accept"][0]) == bool(acc) and r["margin"][0] >= H.MARGIN_MIN
    assert CLS.rel(r["theta"], th) < 1e-12


@pytest.mark.parametrize("idx,L", [(0, 4), (4, 4), (3, 7)])
def test_integrator_is_reversible(idx, L):
    """L steps, p -> -p, L more steps return to (theta, -p): leapfrog is time-reversible, so only
    rounding (amplified by the trajectory's sensitivity) separates the two."""
    g = H.golden_case(idx)
    h, eps = g["H"][H.POINT], 1e-2
    base = (g["X"], g["y"], g["Z"], g["b"])
    n, C = g["theta"].shape
    p0 = H.momentum(n, C, 3, 0)
    q, p1, H0, H1, _, _ = H.leapfrog(*base, g["theta"], h, eps, L, p0)
    back, p2, G0, G1, _, _ = H.leapfrog(*base, q, h, eps, L, -p1)
    assert CLS.rel(back, g["theta"]) < 1e-12 and CLS.rel(-p2, p0) < 1e-12
    assert abs(G0 - H1) <= 1e-12 * abs(H1) and abs(G1 - H0) <= 1e-12 * abs(H0)
    assert CLS.rel(q, g["theta"]) > 1e-3                                   # it moved


def test_streams_are_the_contract():
    assert (H.HMC_MOM, H.HMC_ACCEPT) == (26, 27)
    p = H.momentum(5, 2, 9, 3)
    assert np.array_equal(p[:, 1], px.normals(5, 9, 3, 26, 1))
    txt = open(os.path.join(ROOT, "gpt_amd", "csrc", "gpt_common.h")).read()
    assert re.search(r"kHmcMom\s*=\s*26\b", txt) and re.search(r"kHmcAccept\s*=\s*27\b", txt)


def test_decision_rule():
    assert H.decide(0.5, 0.0, -1e9)                   # an overflowing exponent accepts
    assert not H.decide(0.5, 0.0, math.inf) and not H.decide(0.5, 0.0, math.nan)
    assert not H.decide(0.5, 0.0, -math.inf)          # a non-finite H1 rejects, whatever its sign
    assert H.decide(0.5, 1.0, 1.5) and not H.decide(0.7, 1.0, 1.5)        # exp(-0.5) = 0.607


@pytest.mark.parametrize("cfg", H.PROBE + H.PARITY, ids=lambda c: "case%d_L%d" % c[:2])
def test_margins_of_the_parity_and_probe_configurations(cfg):
    idx, L, eps = cfg
    ntrans = 12 if cfg in H.PROBE else 3
    r = H.run(idx, L, eps, ntrans)[3]
    print("case %d L %d eps %g: accepts %d / %d, smallest margin %.3g"
          % (idx, L, eps, r["accept"].sum(), ntrans, r["margin"].min()))
    assert r["margin"].min() >= H.MARGIN_MIN and not r["divergent"].any()


def test_margins_of_the_run_with_both_outcomes():
    c = H.BOTH
    r = H.run(c["idx"], c["L"], c["eps"], c["ntrans"], c["scale"])[3]
    assert r["margin"].min() >= H.MARGIN_MIN
    assert r["accept"].sum() == 11 and r["accept"][4] == 0       # one rejection, after accepts
    assert np.array_equal(r["store"][:, :, 4], r["store"][:, :, 3])
    assert r["value"][4] == r["value"][3]


def test_margins_of_the_all_rejected_run():
    c = H.ALL_REJECTED
    _, theta0, _, r = H.run(c["idx"], c["L"], c["eps"], c["ntrans"], c["scale"])
    assert r["margin"].min() >= H.MARGIN_MIN and not r["accept"].any()
    assert -4.3 < r["dH"].min() and r["dH"].max() < -3.3
    assert np.array_equal(r["theta"], theta0)


def test_the_divergent_configuration_overflows():
    c = H.DIVERGENT
    r = H.run(c["idx"], c["L"], c["eps"], c["ntrans"])[3]
    assert r["divergent"].all() and not r["accept"].any()


NEW_ENTRY_POINTS = ["gpt_chmc_run", "gpt_chmc_leapfrog", "gpt_gpnt_joint_hmc"]


def test_header_library_and_bindings_declare_the_hmc_entry_points():
    import inspect
    txt = open(os.path.join(ROOT, "include", "gptsgld.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"^\s*int\s+(gpt_\w+)\s*\(", txt, flags=re.M))
    from gpt_amd import GPT_SGLD as G
    from gpt_amd import _lib
    for name in NEW_ENTRY_POINTS:
        assert name in names, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    for name in ("hmc", "mala", "leapfrog"):
        assert callable(getattr(G.SoftmaxJoint, name))
    assert callable(G.gpnt_joint_hmc_oneshot)
    assert set(G.HMCResult.__slots__) == {"theta_store", "accept", "dH", "value", "accept_rate",
                                          "ndivergent"}
    sig = inspect.signature(G.GPNT_hyperparameters_ng)
    assert sig.parameters["e_step"].default == "langevin"
    assert sig.parameters["num_leapfrog"].default == 8


def test_julia_ccall_of_the_oneshot_entry_matches_the_header():
    """julia/GPT_SGLD_HIP.jl binds gpt_gpnt_joint_hmc with one ccall type per C parameter
    (tests/test_julia_shim.py's parser); no Julia is needed to check that."""
    import test_julia_shim as TS
    calls = {c[0]: c for c in TS.julia_ccalls(TS.JULIA[0])}
    protos = TS.header_prototypes()
    sym = "gpt_gpnt_joint_hmc"
    assert sym in calls and sym in protos
    _, ret, types, args = calls[sym]
    cret, cparams = protos[sym]
    assert ret in TS.C2J[cret] and len(types) == len(cparams) == len(args)
    for i, (jt, ct) in enumerate(zip(types, cparams)):
        assert jt in TS.C2J[ct], "arg %d is %s, C wants %s" % (i, jt, ct)
    src = open(TS.JULIA[0]).read()
    assert "joint_hmc" in src[src.index("export"):src.index("const LIB")]
