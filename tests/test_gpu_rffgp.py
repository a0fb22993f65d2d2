"""GPU tests of the RFF GP's closed-form predictive (NoTensorMarginal.predict, gpnt_predict_oneshot)
and of the kernel approximation error (rff_kernel_error), gpt_amd/csrc/nlml.hip, against the
50-digit golden tests/golden/rffgp_mp.npz and the fp64 restatements of tests/rffgp_ref.py.

Parity rule (tests/test_gpu_nlml.py, test_gpu_exactgp.py): the device's error against the golden
is at most 32 x the larger of the two fp64 restatements' errors against the golden, with a floor
of 1e-12.  Measures: fmu over max|fmu|, fs2 over sigma_RBF^2, lp over max|lp|; frob, norm_K and
max_abs relative.
"""
import numpy as np
import pytest

import rffgp_ref as RR

pytestmark = pytest.mark.gpu

FLOOR = 1e-12
EPS = np.finfo(np.float64).eps


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


@pytest.fixture(scope="module")
def golden():
    return RR.load_golden()


def marginal(g):
    return G().NoTensorMarginal(g["X"], g["y"], g["Z"], g["b"])


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. predictive parity
@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_name)
def test_predictive_parity(golden, case):
    nm = RR.case_name(case)
    g = golden[nm]
    m = marginal(g)
    worst = dict.fromkeys(RR.PRED_QUANT, 0.0)
    for p in range(3):
        h = g["H"][p]
        res = m.predict(h, g["Xtest"], g["ytest"])
        err = RR.pred_errors(res, g, p)
        yard = RR.pred_yardstick(g, p)[0]
        for k in RR.PRED_QUANT:
            bound = max(32 * yard[k], FLOOR)
            worst[k] = max(worst[k], err[k] / bound)
            print("%s point %d %s: error %.2e, bound %.2e" % (nm, p, k, err[k], bound))
        assert res.ymu is res.fmu
        assert np.array_equal(res.ys2, res.fs2 + h[-1])
        assert (res.fs2 > 0).all()
        assert m.predict(h, g["Xtest"]).lp is None
        for k in RR.PRED_QUANT:
            assert err[k] <= max(32 * yard[k], FLOOR), (nm, p, k, err[k], yard[k])
    print("%s: worst error/bound %s" % (nm, {k: "%.3f" % v for k, v in worst.items()}))
    m.close()


# ------------------------------------------------------------------ 2. chunking and position
@pytest.mark.parametrize("nm", ["n33_N130_D2_Lh4", "n128_N259_D8_Lh10", "n65_N1030_D16_Lh18"])
def test_chunking_and_position(golden, nm):
    g = golden[nm]
    m = marginal(g)
    h = g["H"][1]
    Xt, yt = g["Xtest"], g["ytest"]
    full = m.predict(h, Xt, yt)
    for chunk in (16, 32):
        assert same(full, m.predict(h, Xt, yt, chunk=chunk)), chunk
    for i in (0, 15, 16, 76):
        one = m.predict(h, Xt[i:i + 1], yt[i:i + 1])
        assert same(one, [q[i:i + 1] for q in full]), i
    a, b = m.predict(h, Xt[:40], yt[:40]), m.predict(h, Xt[40:], yt[40:])
    assert same([np.concatenate(q) for q in zip(a, b)], full)
    nolp = m.predict(h, Xt)
    assert same(nolp[:4], full[:4])


# ------------------------------------------------------------------ 3. factor reuse
@pytest.mark.parametrize("nm", ["n33_N130_D2_Lh4", "n100_N517_D4_Lh3", "n128_N259_D8_Lh10"])
def test_factor_reuse(golden, nm):
    g = golden[nm]
    h, other = g["H"][1], g["H"][0]
    Xt, yt = g["Xtest"], g["ytest"]
    fresh = marginal(g).predict(h, Xt, yt)
    m = marginal(g)
    val, grad = m.value_and_grad(h)
    theta = m.theta_mean(h)
    phi = m.features()
    m.value_and_grad(h)
    assert same(m.predict(h, Xt, yt), fresh)                 # the gradient evaluation's factor
    assert same(m.predict(h, Xt, yt), fresh)                 # and again, the factor predict kept
    m.value_and_grad(other)
    assert same(m.predict(h, Xt, yt), fresh)                 # after another point: refit
    m.nlogmarginal(h)
    assert same(m.predict(h, Xt, yt), fresh)                 # a value-only evaluation's factor
    one = G().gpnt_predict_oneshot(g["X"], g["y"], g["Z"], g["b"], h, Xt, yt)
    assert same(one, fresh)
    # the handle's other results are what they were
    v2, g2 = m.value_and_grad(h)
    assert v2 == val and np.array_equal(g2, grad)
    assert np.array_equal(m.theta_mean(h), theta)
    assert np.array_equal(m.features(), phi)
    m.predict(other, Xt, yt)
    assert np.array_equal(m.theta_mean(h), theta)


def test_failed_cholesky_leaves_the_handle_usable(golden):
    from gpt_amd._lib import GPT_ERR_NOT_SPD, GPTError
    g = golden["n33_N130_D2_Lh4"]
    X = g["X"].copy()
    X[7, 1] = np.nan
    bad = G().NoTensorMarginal(X, g["y"], g["Z"], g["b"])
    with pytest.raises(GPTError) as ei:
        bad.predict(g["H"][0], g["Xtest"], g["ytest"])
    assert ei.value.code == GPT_ERR_NOT_SPD
    with pytest.raises(GPTError) as ei:
        bad.predict(g["H"][0], g["Xtest"])                   # no stale factor is taken
    assert ei.value.code == GPT_ERR_NOT_SPD
    m = marginal(g)
    want = m.predict(g["H"][0], g["Xtest"], g["ytest"])
    assert np.isfinite(want.lp).all()


# ------------------------------------------------------------------ 4. link to the sampling path
@pytest.mark.parametrize("nm", ["n33_N130_D2_Lh4", "n100_N517_D4_Lh3"])
def test_mean_is_gpnt_pred_of_theta_mean(golden, nm):
    g = golden[nm]
    m = marginal(g)
    h = g["H"][1]
    D = g["X"].shape[1]
    n = g["Z"].shape[0]
    l = m.theta_mean(h)
    ls = h[:D] if h.size == D + 2 else h[0]
    phitest = G().featureNotensor(g["Xtest"], ls, h[-2], g["Z"], g["b"])
    ev = G().GPNT_pred(np.asfortranarray(l[:, None]), phitest, g["ytest"])
    fmu = m.predict(h, g["Xtest"]).fmu
    tol = 2 * (n + 2) * EPS * (np.abs(phitest).T @ np.abs(l))
    diff = np.abs(np.asarray(ev.mean_fhat).ravel() - fmu)
    print("%s: worst difference/tolerance %.3f" % (nm, (diff / tol).max()))
    assert (diff <= tol).all()


# ------------------------------------------------------------------ 5. kernel-error parity
@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_name)
def test_kernel_error_parity(golden, case):
    nm = RR.case_name(case)
    g = golden[nm]
    for q, p in enumerate(RR.KERR_POINTS):
        res = G().rff_kernel_error(g["X"], g["Z"], g["b"], g["H"][p])
        err = RR.kerr_errors(res, g, q)
        bound = np.maximum(32 * RR.kerr_yardstick(g, q)[0], FLOOR)
        print("%s point %d: errors %s, worst error/bound %.3f" % (nm, p, err, (err / bound).max()))
        assert (err <= bound).all(), (nm, p, err, bound)
        assert res._fields == ("frob", "norm_K", "max_abs")


@pytest.mark.parametrize("N,n", [(1, 2), (127, 2), (128, 31), (129, 1), (129, 2), (127, 1),
                                 (63, 31), (64, 1), (65, 2)])
def test_kernel_error_edge_shapes(N, n):
    """Against the literal restatement at 1e-12 relative: N on either side of the 64-row tile edge
    and of two tiles, one row; n odd, even and one; D = 3, both hyper-parameter forms."""
    rng = np.random.default_rng(100 * N + n)
    D = 3
    X, Z, b = rng.standard_normal((N, D)), rng.standard_normal((n, D)), 2 * np.pi * rng.random(n)
    for h in (np.array([0.8, 1.1, 1.7, 0.9, 0.04]), np.array([1.2, 1.3, 0.5])):
        want = np.array(RR.kernel_error_literal(X, Z, b, h))
        got = np.array(G().rff_kernel_error(X, Z, b, h))
        err = np.abs(got - want) / np.abs(want)
        print("N = %d, n = %d, Lh = %d: %s" % (N, n, h.size, err))
        assert (err <= 1e-12).all(), (N, n, err)


# ------------------------------------------------------------------ 6. determinism
def test_determinism(golden):
    g = golden["n100_N517_D4_Lh3"]
    h = g["H"][1]
    a = G().rff_kernel_error(g["X"], g["Z"], g["b"], h)
    assert G().rff_kernel_error(g["X"], g["Z"], g["b"], h) == a
    m = marginal(g)
    p1 = m.predict(h, g["Xtest"], g["ytest"])
    G().rff_kernel_error(g["X"], g["Z"], g["b"], g["H"][0])      # other library work in between
    m.value_and_grad(g["H"][2])
    assert G().rff_kernel_error(g["X"], g["Z"], g["b"], h) == a
    assert same(m.predict(h, g["Xtest"], g["ytest"]), p1)


# ------------------------------------------------------------------ 7. rejections
def _rejected(fn, *args, **kw):
    from gpt_amd._lib import GPT_ERR_BAD_DIMS, GPTError
    with pytest.raises(GPTError) as ei:
        fn(*args, **kw)
    assert ei.value.code == GPT_ERR_BAD_DIMS
    assert len(str(ei.value)) > len("gptsgld error 2: ")


def test_rejections(golden):
    g = golden["n33_N130_D2_Lh4"]
    X, y, Z, b, Xt, yt = (g[k] for k in ("X", "y", "Z", "b", "Xtest", "ytest"))
    h = g["H"][0]
    m = marginal(g)
    kerr = G().rff_kernel_error
    _rejected(m.predict, [1.0, 1.0, 1.0, 0.9, 0.04], Xt)               # Lh = 5 with D = 2
    _rejected(kerr, X, Z, b, [1.0, 1.0, 1.0, 0.9, 0.04])
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        for k in range(h.size):
            hb = h.copy()
            hb[k] = bad
            _rejected(m.predict, hb, Xt, yt)
            _rejected(kerr, X, Z, b, hb)
            _rejected(G().gpnt_predict_oneshot, X, y, Z, b, hb, Xt, yt)
    _rejected(m.predict, h, Xt[:, :1])                                 # wrong width
    _rejected(m.predict, h, Xt[:0])                                    # Nt = 0
    _rejected(m.predict, h, Xt, yt[:5])
    _rejected(m.predict, h, Xt, chunk=-1)
    _rejected(G().gpnt_predict_oneshot, X, y, Z, b, h, Xt[:, :1])
    _rejected(G().gpnt_predict_oneshot, X, y, Z[:, :1], b, h, Xt)
    _rejected(kerr, X, Z[:, :1], b, h)
    _rejected(kerr, X, Z, b[:5], h)
    _rejected(kerr, X, np.zeros((8193, 2)), np.zeros(8193), h)         # n beyond the limit
    _rejected(kerr, np.zeros((65537, 2)), Z, b, h)                     # N beyond the limit
    _rejected(kerr, np.zeros((65536, 2)), np.zeros((4097, 2)), np.zeros(4097), h)   # phi > 2 GiB
    want = m.predict(h, Xt, yt)                                        # the handle still works
    assert RR.pred_errors(want, g, 0)["fmu"] <= 1e-9
