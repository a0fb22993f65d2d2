"""Every route of the prediction kernels (gpt_amd/csrc/pred.hip) against mpmath and across tilings.

Golden parity: every case of oracle/pred_cases.py (one per dispatch branch of launch_pred_mfma and
per tile edge of pred_temp_mfma_kernel) at every element against the 50-digit reference of
tests/golden/pred_mp.npz, within the derived bound E of that module and within the project's
prediction bar 1e-12·max|f| (tests/test_gpu_parity.py), on the route gpt_pred_last_route reports.
The direct kernels (GPTSGLD_PRED=direct) the same.  The persistent rows kernel's steady state
(workgroups that run two and three tiles) and calls split into several passes
(GPTSGLD_PRED_PASS_BYTES) bit for bit against the same samples predicted in calls of one tile per
workgroup and of one pass: an element's arithmetic does not depend on which tile, workgroup,
register buffer or pass computes it.
"""
import numpy as np
import pytest

from oracle import gpt_sgld_ref as R
from oracle import pred_cases as PC

pytestmark = pytest.mark.gpu

RMSE_BAR = 1e-10         # test RMSE, relative (tests/test_gpu_parity.py)


def G():
    from gpt_amd import GPT_SGLD
    return GPT_SGLD


def route():
    from gpt_amd.session import pred_last_route
    return pred_last_route()


def dev(a):
    """A column-major numpy array on the device (torch sees the reversed shape)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).cuda()


class Device:
    """The inputs of a shape on the device; pred(s0, S) predicts samples s0 .. s0 + S − 1."""

    def __init__(self, shape, p):
        self.shape, self.p = shape, p
        self.w, self.U, self.phi = dev(p["w"]), dev(p["U"]), dev(p["phi"])
        self.I0 = dev((p["I"] - 1).astype(np.int32))

    def pred(self, s0=0, S=None):
        import torch
        from gpt_amd.session import pred_device
        n, D, Nt, r, Q, Sall = self.shape
        S = Sall - s0 if S is None else S
        out = torch.full((S, Nt), float("nan"), dtype=torch.float64, device="cuda")
        pred_device(self.w[s0:].data_ptr(), self.U[s0:].data_ptr(), self.I0, self.phi, n, D, Nt, r,
                    Q, S, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()


def check_bars(f, ref, what):
    """|f − ref| <= E and <= 1e-12·max|f| at every element; returns the worst error / E."""
    err = PC.err_abs(f, ref)
    ratio = err / ref[2]
    bar = PC.BAR * np.abs(ref[0]).max()
    print("%s: worst error / E = %.3f, worst error / (1e-12 max|f|) = %.3f" % (
        what, ratio.max(), err.max() / bar))
    assert np.isfinite(f).all(), what
    assert (ratio <= 1.0).all(), (what, ratio.max())
    assert (err <= bar).all(), (what, err.max() / bar)
    return ratio.max()


def set_rows(monkeypatch, rows):
    if rows:
        monkeypatch.setenv("GPTSGLD_PRED_VPHASE", "rows")
    else:
        monkeypatch.delenv("GPTSGLD_PRED_VPHASE", raising=False)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ("GPTSGLD_PRED", "GPTSGLD_PRED_VPHASE", "GPTSGLD_PRED_PASS_BYTES"):
        monkeypatch.delenv(v, raising=False)


# --------------------------------------------------------------------------------- golden parity
@pytest.mark.parametrize("group", PC.GROUPS)
def test_pred_golden_parity(group, monkeypatch):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worst = 0.0
    for c in (c for c in PC.CASES if c.group == group):
        n, D, Nt, r, Q, S = c.shape
        p, ref, cid = PC.inputs(c), PC.reference(c), PC.case_id(c)
        set_rows(monkeypatch, c.rows)
        f = Device(c.shape, p).pred()
        rt = route()
        assert (rt["kind"], rt["tdim"], rt["npw"]) == (c.kind, c.tdim, c.npw), (cid, rt)
        nti = (Nt + 63) // 64
        assert (rt["tiles"], rt["passes"], rt["first"]) == (nti * S, 1, S), (cid, rt)
        grid = nti if c.kind != PC.ROWS_PF else min(nti * S, PC.rows_pf_grid(c.shape, cus))
        assert rt["grid"] == grid, (cid, rt)
        worst = max(worst, check_bars(f, ref, cid))
        if S == 1:
            f1 = G().pred(p["w"][:, 0], p["U"][..., 0], p["I"], p["phi"])
            assert route()["kind"] == c.kind
            worst = max(worst, check_bars(f1[None, :], ref, cid + " gpt_pred"))
    print("group %s: worst error / E = %.3f" % (group, worst))


@pytest.mark.parametrize("shape,rows", [((8, 15, 70, 5, 40, 2), False), ((24, 7, 70, 6, 30, 2), False),
                                        ((64, 14, 70, 20, 8, 2), False)])
def test_pred_mean_golden(shape, rows, monkeypatch):
    c = PC.find(shape, rows)
    n, D, Nt, r, Q, S = shape
    p, (hi, lo, E) = PC.inputs(c), PC.reference(c)
    set_rows(monkeypatch, rows)
    mean, rm = G().pred_mean(p["w"], p["U"].reshape((n, r, D * S), order="F"), p["I"], p["phi"],
                             p["y"], scale=1.3)
    assert route()["kind"] == c.kind
    want = hi.mean(axis=0) + lo.mean(axis=0)
    assert np.abs(mean - want).max() <= 1e-12 * np.abs(want).max()
    assert rm == pytest.approx(R.rmse(p["y"], want, 1.3), rel=RMSE_BAR)


# -------------------------------------------------------------------------------- direct kernels
@pytest.mark.parametrize("shape", PC.DIRECT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_pred_direct_kernels(shape, monkeypatch):
    """pred_kernel (gpt_pred, gpt_pred_dev) and pred_x_kernel (gpt_pred_mean_x) under
    GPTSGLD_PRED=direct, which every call reads."""
    c = PC.find(shape)
    n, D, Nt, r, Q, S = shape
    p, ref = PC.inputs(c), PC.reference(c)
    d = Device(shape, p)
    d.pred()
    assert route()["kind"] != PC.DIRECT
    monkeypatch.setenv("GPTSGLD_PRED", "direct")
    f = d.pred()
    rt = route()
    nti = (Nt + 63) // 64
    assert rt == dict(kind=PC.DIRECT, tdim=0, npw=0, grid=nti, tiles=nti * S, passes=1, first=S)
    check_bars(f, ref, "pred_kernel, gpt_pred_dev")
    for s in range(S):
        f1 = G().pred(p["w"][:, s], p["U"][..., s], p["I"], p["phi"])
        assert route()["kind"] == PC.DIRECT and route()["first"] == 1
        check_bars(f1[None, :], tuple(a[s:s + 1] for a in ref), "pred_kernel, gpt_pred %d" % s)
    mean, rm, srm = G().pred_mean_x(p["w"], p["U"].reshape((n, r, D * S), order="F"), p["I"],
                                    p["X"], p["y"], p["ls"], 1.0, p["scale"], p["Z"], p["b"],
                                    scale=1.3)
    fref = ref[0] + ref[1]
    want = fref.mean(axis=0)
    assert np.abs(mean - want).max() <= 1e-12 * np.abs(fref).max()
    assert rm == pytest.approx(R.rmse(p["y"], want, 1.3), rel=RMSE_BAR)
    swant = 1.3 * np.sqrt(((fref - p["y"]) ** 2).mean(axis=1))
    print("pred_x_kernel: worst relative RMSE error %.3g" % (np.abs(srm / swant - 1).max()))
    assert np.abs(srm - swant).max() <= RMSE_BAR * swant.max()
    monkeypatch.delenv("GPTSGLD_PRED")
    f2 = d.pred()
    assert route()["kind"] == PC.expected_route(shape)[0]
    check_bars(f2, ref, "back on the MFMA path")


# ------------------------------------------------------------ the persistent loop's steady state
def oracle_bar(f, p, what):
    """Every sample against the numpy oracle at 1e-12·max|f|."""
    worst = 0.0
    for s in range(f.shape[0]):
        want = R.pred(p["w"][:, s], p["U"][..., s], p["I"], p["phi"])
        e = np.abs(f[s] - want).max() / np.abs(want).max()
        worst = max(worst, e)
        assert e <= PC.BAR, (what, s, e)
    print("%s: worst error against the oracle / max|f| = %.3g" % (what, worst))


@pytest.mark.parametrize("base,rows,tdim", [((32, 8, 1450, 20, 40), False, 8),
                                            ((16, 3, 6400, 5, 30), True, 3),
                                            ((24, 4, 2560, 6, 1100), False, 4)])
def test_pred_rows_pf_steady_state(base, rows, tdim, monkeypatch):
    """More than two tiles per workgroup of pred_vphase_rows_pf_kernel (some run two, some three:
    both register buffers fetched, parked and refilled; at Q > 1024 w is reloaded at every park)
    equal, bit for bit, the same samples predicted with at most one tile per workgroup."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shape = PC.steady_shape(*base, cus)
    n, D, Nt, r, Q, S = shape
    assert S * PC.temp_bytes(shape) <= 256 << 20
    p = PC._inputs(shape, 0)
    set_rows(monkeypatch, rows)
    d = Device(shape, p)
    big = d.pred()
    rt = route()
    print("CUs %d, shape %s, route %s" % (cus, shape, rt))
    assert (rt["kind"], rt["tdim"], rt["npw"], rt["passes"]) == (PC.ROWS_PF, tdim, 10, 1), rt
    assert rt["grid"] == PC.rows_pf_grid(shape, cus), rt
    assert rt["tiles"] == (Nt + 63) // 64 * S and rt["tiles"] > 2 * rt["grid"], rt
    assert rt["tiles"] < 3 * rt["grid"] and rt["tiles"] >= 2.15 * rt["grid"], rt
    step = rt["grid"] // ((Nt + 63) // 64)
    assert step >= 1
    small = np.empty_like(big)
    for s0 in range(0, S, step):
        Sc = min(step, S - s0)
        small[s0:s0 + Sc] = d.pred(s0, Sc)
        rs = route()
        assert rs["kind"] == PC.ROWS_PF and rs["tiles"] <= rs["grid"], rs
    assert np.isfinite(big).all()
    diff = np.flatnonzero((big != small).any(axis=1))
    assert np.array_equal(big, small), "samples that differ: %s" % diff[:20]
    oracle_bar(big, p, "steady state %s" % (shape,))


# ---------------------------------------------------------------------------- more than one pass
def _pass_case(shape, rows, monkeypatch):
    p = PC._inputs(shape, 0)
    set_rows(monkeypatch, rows)
    d = Device(shape, p)
    one = d.pred()
    rt = route()
    assert (rt["passes"], rt["first"]) == (1, shape[5]), rt
    oracle_bar(one, p, "one pass %s" % (shape,))
    return d, one, rt


def test_pred_passes_rounded_to_whole_gemm_tiles(monkeypatch):
    """r = 20: a budget of 40 samples is rounded to the 32 that fill whole 128-column GEMM tiles:
    passes of 32, 32 and 6 samples."""
    shape = (16, 8, 70, 20, 40, 70)
    d, one, rt1 = _pass_case(shape, False, monkeypatch)
    monkeypatch.setenv("GPTSGLD_PRED_PASS_BYTES", str(40 * PC.temp_bytes(shape) + 1000))
    f = d.pred()
    rt = route()
    assert rt == dict(rt1, passes=3, first=32, tiles=2 * 6, grid=min(rt1["grid"], 2 * 6)), rt
    assert np.array_equal(f, one)


@pytest.mark.parametrize("rows", [False, True], ids=["pairs", "rows"])
def test_pred_passes_below_the_unit(rows, monkeypatch):
    """r = 5: a budget of 7 samples is below the unit of 128, so it is taken as it is: passes of
    7, 7, 7, 7 and 2 samples.  An unset, an unparsable and a non-positive budget leave the call in
    one pass; one below a sample gives passes of one sample."""
    shape = (16, 3, 70, 5, 30, 30)
    d, one, rt1 = _pass_case(shape, rows, monkeypatch)
    assert rt1["kind"] == (PC.ROWS_PF if rows else PC.PAIRS)
    per = PC.temp_bytes(shape)
    monkeypatch.setenv("GPTSGLD_PRED_PASS_BYTES", str(8 * per - 1))
    f = d.pred()
    rt = route()
    assert rt == dict(rt1, passes=5, first=7, tiles=2 * 2, grid=min(rt1["grid"], 2 * 2)), rt
    assert np.array_equal(f, one)
    for bad in ("", "abc", "7x", "0", "-%d" % per, "1e6", "99999999999999999999999999"):
        monkeypatch.setenv("GPTSGLD_PRED_PASS_BYTES", bad)
        f = d.pred()
        assert route() == rt1, (bad, route())
        assert np.array_equal(f, one), bad
    monkeypatch.setenv("GPTSGLD_PRED_PASS_BYTES", "1")
    f = d.pred()
    rt = route()
    assert rt == dict(rt1, passes=30, first=1, tiles=2, grid=min(rt1["grid"], 2)), rt
    assert np.array_equal(f, one)
    monkeypatch.setenv("GPTSGLD_PRED_PASS_BYTES", str(1 << 40))
    f = d.pred()
    assert route() == rt1 and np.array_equal(f, one)
