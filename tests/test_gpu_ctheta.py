"""The full-theta softmax side on the device against 50 digits (tests/golden/ctheta_mp.npz, cases
and measures in tests/ctheta_cases.py).

A  cjoint_eval_kernel past 256 tiles, where a workgroup walks more than one tile (the `!first`
   branches, v_acc / r_acc carried across tiles, the barrier that lets the next tile reuse LDS):
       (n, N, D, C)          TI  tiles  reaches
       (33, 8230, 2, 3)      32  258    workgroups 0 and 1 walk two tiles; the 6-column last tile is a second pass
       (33, 16485, 2, 3)     32  516    three tiles for workgroups 0-3, two for the rest
       (700, 2053, 1, 2)      8  257    the TI = 8 layout, scalar length scale; last tile 5 columns
       (330, 4100, 4, 32)    16  257    theta read through L2 while walking
   value_and_grad (kCjFull), neglogjointlkhd (kCjValue) and hyper_value_and_grad at hyper point 1
   are held by tests/test_gpu_cjoint.py's parity rule: 32 x the larger error of the literal and the
   fused fp64 restatements against the reference, floor 1e-12, the value 1e-12 relative.  The
   reference is mpmath for the first three and long double for n = 330, N = 4100 (one mpmath
   evaluation of it takes about 160 s).  The literal form is in the yardstick of all four (its
   n·N·D doubles are 43 MB at most).  kCjTheta on the walk is reached by the Langevin step and the
   leapfrog on the first case (entries lang_w0 and leap_w0 of part B); kCjScores by the
   identity-theta construction at Ntest = 8230; kCjFeatures writes nothing a caller can read, so
   it only runs, between two evaluations whose bits must not change.

B  GPNT_SGLDclass (ntc_chain_kernel), SoftmaxJoint.langevin (cjoint_update_kernel), leapfrog and
   hmc (chmc.hip) against mpmath within B = 8·u per family and quantity, u the largest error of the
   fp64 restatements against the same reference (make_ctheta_golden.py measures it,
   tests/test_ctheta_cases.py holds 8·u <= 1e-13 and shows that nine defects of 1e-9 relative and
   below fail B).  The margin of 8 is tests/test_gpu_step.py's: other summation orders (wave sums,
   butterflies, per-workgroup partials in workgroup order), the library's exp and log, and device
   normals within 7·2^-52 of the radius.  No normals term is added to any bar.

Measured (u and B by make_ctheta_golden.py: 60 s on eight processes, 190 s of references in all,
the longest 55 s for n = 700, N = 2053; device worst error / B as this file prints it, MI355X):
    family  quantities     u                                    B = 8·u                              device worst / B
    cls     theta          4.7e-16                              3.7e-15                              0.22
    lang    theta          1.4e-15                              1.1e-14                              0.06
    leap    q p H dH       3.2e-16 5.2e-16 3.7e-16 4.8e-16      2.6e-15 4.2e-15 3.0e-15 3.9e-15      0.09 0.07 0.06 0.08
    hmc     theta value dH 5.9e-16 4.7e-16 3.4e-16              4.8e-15 3.7e-15 2.7e-15              0.14 0.03 0.06
    wlang   theta          6.0e-17                              4.8e-16                              0.13
    wleap   q p H dH       9.9e-16 9.8e-15 4.7e-16 4.2e-16      7.9e-15 7.8e-14 3.8e-15 3.4e-15      0.13 0.12 0.12 0.14
wlang and wleap are the Langevin step and the L = 2 leapfrog on the N = 8230 walk case, families of
their own (ctheta_cases.family).  The walk's parity: value within 6.1e-16, the hyper-gradient within
5.8e-15 and grad theta within 1.1e-15 of the reference on all four shapes, against bounds at the
1e-12 floor.
"""
import numpy as np
import pytest

import cjoint_ref as CR
import ctheta_cases as T

pytestmark = pytest.mark.gpu

FLOOR = 1e-12

def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("k", range(len(T.WALK)), ids=lambda k: CR.case_name(T.WALK[k] + ("",)))
def test_walk_parity(k):
    P, ref = T.problem("w%d" % k), T.reference(("walk", k))
    L = CR.cjoint_layout(P.n, P.X.shape[0], P.C)
    assert L["ntiles"] > L["nblk"] == CR.CJ_MAX_BLOCKS
    nC = P.n * P.C
    yh, yt = T.walk_yardstick(k)
    bh, bt = np.maximum(32 * yh, FLOOR), max(32 * yt, FLOOR)
    j = P.joint(G())
    val, grad = j.value_and_grad(T.flat(P.theta), P.h)
    ev, eh, et = T.walk_errors(P, val, grad[:nC], grad[nC:], ref)
    v2 = j.neglogjointlkhd(None, P.h)
    hv, hg = j.hyper_value_and_grad(P.h)
    ev2 = T.walk_errors(P, v2, grad[:nC], grad[nC:], ref)[0]
    ev3, eh3, _ = T.walk_errors(P, hv, grad[:nC], hg, ref)
    print("%s: value %.2e / %.2e / %.2e; hyper worst error/bound %.3f (%.2e), hyper-only %.3f; "
          "grad theta error/bound %.3f (%.2e)" % (T.key(("walk", k)), ev, ev2, ev3, (eh / bh).max(),
                                                   eh.max(), (eh3 / bh).max(), et / bt, et))
    assert max(ev, ev2, ev3) <= 1e-12, (ev, ev2, ev3)
    assert (eh <= bh).all() and (eh3 <= bh).all(), (eh, eh3, bh)
    assert et <= bt, (et, bt)
    j.close()


def test_walk_scores_with_identity_theta_are_the_features():
    """test_gpu_cjoint.py's construction at Ntest = 8230 (258 tiles of kCjScores) and n = 33: C is
    at most 32, so theta is the first 32 columns of the identity and the scores are the first 32
    features, bit for bit (the other terms of every sum are exact zeros)."""
    n, N, D, C, Nt = 33, 40, 2, 32, 8230
    rng = np.random.default_rng(n + Nt)
    X, Z, b = rng.standard_normal((N, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    Xt = rng.standard_normal((Nt, D))
    j = G().SoftmaxJoint(X, (np.arange(N) % C) + 1.0, Z, b, C=C)
    j.set_theta(np.eye(n)[:, :C])
    ls = 0.5 + rng.random(D)
    got = j.scores(np.concatenate([ls, [1.7]]), Xt)
    want = G().featureNotensor(Xt, ls, 1.7, Z, b)
    assert got.shape == (Nt, C)
    assert np.array_equal(got, want[:C].T)


def test_walk_leaves_no_stale_partials():
    """theta1, theta2, theta1 again on one handle: the first and third evaluations give equal bits,
    and so does a fresh handle (a partial of the first walk that survived into the third would
    show); a kCjFeatures launch and a value-only one in between change nothing."""
    from gpt_amd._lib import P_D, check, lib
    P = T.problem("w1")
    th1 = T.flat(P.theta)
    th2 = T.flat(np.random.default_rng(8).standard_normal(P.theta.shape))
    j = P.joint(G())
    v1, g1 = j.value_and_grad(th1, P.h)
    v2, g2 = j.value_and_grad(th2, P.h)
    ms = np.empty(1)
    check(lib().gpt_cjoint_time(j._h, P.h.ctypes.data_as(P_D), P.h.size, 4, 1, ms.ctypes.data_as(P_D)))
    assert j.neglogjointlkhd(None, P.h) == v2
    v3, g3 = j.value_and_grad(th1, P.h)
    assert v1 == v3 and np.array_equal(g1, g3)
    assert v1 != v2 and not np.array_equal(g1, g2)
    v4, g4 = P.joint(G()).value_and_grad(th1, P.h)
    assert v1 == v4 and np.array_equal(g1, g4)


# ------------------------------------------------------------------------------------------ B
WORST = {}


def hold(e, run):
    """Every quantity of the family within its bar; prints error / B."""
    for name, v in run.items():
        assert np.isfinite(v).all(), name
    fam = T.family(e)
    err, B = T.errors(e, run, T.reference(e)), T.bars()[fam]
    print("%s: worst / B: %s" % (T.key(e), "  ".join("%s %.3f (%.2e)" % (q, err[q] / B[q], err[q])
                                                     for q in T.FAMILIES[fam])))
    for q, v in err.items():
        WORST[(fam, q)] = max(WORST.get((fam, q), 0.0), v / B[q])
    print("    %s so far, worst / B: %s" % (fam, "  ".join("%s %.3f" % (q, WORST[(fam, q)])
                                                        for q in T.FAMILIES[fam] if (fam, q) in WORST)))
    for q, v in err.items():
        assert v <= B[q], (q, v, B[q])


@pytest.mark.parametrize("k", range(len(T.CLS_CASES)), ids=lambda k: "-".join("%g" % v for v in T.CLS_CASES[k]))
def test_class_sampler_against_mpmath(k):
    n, m, C, tail, decay, sigma = T.CLS_CASES[k]
    phi, y = T.cls_inputs(k)
    store, status = G().GPNT_SGLDclass_chains(phi, y, sigma, m, [T.CLS_EPS * f for _, f in T.CLS_CHAINS],
                                              decay, 0, 2, [s for s, _ in T.CLS_CHAINS], ncls=C)
    assert not status.any() and store.shape == (n, C, 4, len(T.CLS_CHAINS))
    hold(("cls", k), {"theta%d" % c: np.array([T.flat(store[:, :, s, c]) for s in range(T.STEPS)])
                      for c in range(len(T.CLS_CHAINS))})


@pytest.mark.parametrize("name,t0,nsteps", T.LANG, ids=lambda v: str(v))
def test_langevin_against_mpmath(name, t0, nsteps):
    P = T.problem(name)
    j = P.joint(G())
    j.set_theta(P.theta)
    out = []
    for s in range(nsteps):
        j.langevin(P.h, T.lang_eps(name)[0], 1, T.SEED, t0=t0 if s == 0 else None)
        out.append(T.flat(j.theta()))
    assert j.steps == t0 + nsteps
    hold(("lang", name, t0, nsteps), dict(theta=np.array(out)))


@pytest.mark.parametrize("name,L", T.LEAP, ids=lambda v: str(v))
def test_leapfrog_against_mpmath(name, L):
    """Forward from (theta, p); back from the doubles nearest the reference's (q, -p_new), which
    returns to (theta, -p) (tests/test_ctheta_cases.py holds the back reference to that)."""
    e = ("leap", name, L)
    P = T.problem(name)
    j = P.joint(G())
    j.set_theta(P.theta)
    q, p1, H0, H1 = j.leapfrog(P.h, T.HMC_EPS, L, T.leap_momentum(name, L))
    run = dict(q=T.flat(q)[None], p=T.flat(p1)[None], H=np.array([H0, H1]), dH=np.array([H0 - H1]))
    qs, ps = T.back_start(e)
    j.set_theta(qs)
    q, p1, H0, H1 = j.leapfrog(P.h, T.HMC_EPS, L, ps)
    run.update(bq=T.flat(q)[None], bp=T.flat(p1)[None], bH=np.array([H0, H1]), bdH=np.array([H0 - H1]))
    hold(e, run)


@pytest.mark.parametrize("name,L,eps,ntrans,scale", T.HMC, ids=lambda v: str(v))
def test_hmc_against_mpmath(name, L, eps, ntrans, scale):
    e = ("hmc", name, L, eps, ntrans, scale)
    P, ref = T.problem(name), T.reference(e)
    j = P.joint(G())
    j.set_theta(scale * P.theta)
    got = j.hmc(P.h, eps, L, ntrans, T.SEED, t0=0)
    sure = ref["margin"] >= T.H.MARGIN_MIN
    assert np.array_equal(got.accept[sure], ref["accept"][sure])
    # dH as the device returns it; H0 is the reference's (the device returns no H0)
    hold(e, dict(theta=np.array([T.flat(got.theta_store[:, :, s]) for s in range(ntrans)]),
                 value=got.value, dH=got.dH))
