"""CPU conditions of the prediction suite (tests/test_gpu_pred.py): the committed double-double
references and bounds of oracle/pred_cases.py are mpmath's, the bound is tight enough to mean
something, the numpy oracle meets it on every element (so the reference alone passes what the
device is asked to pass), and the case table reaches every instantiation of the V-phase kernels
that no other test holds."""
import os
import re

import numpy as np
import pytest

from oracle import pred_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pred_source():
    return open(os.path.join(ROOT, "gpt_amd", "csrc", "pred.hip")).read()


def _int_list(src, name):
    """The values of `using <name> = IntList<...>;` in the source."""
    return tuple(int(v) for v in re.search(r"using %s = IntList<([^>]*)>" % name, src).group(1).split(","))


def test_fixture_holds_every_case():
    st = PC._stored()
    assert os.path.getsize(PC.GOLDEN) < 1 << 20
    for c in PC.CASES:
        k = PC.key(c)
        n, D, Nt, r, Q, S = c.shape
        assert str(st[k + "_digest"]) == PC.digest(c), k
        assert st[k + "_hi"].dtype == np.float64 and st[k + "_lo"].dtype == np.float32
        assert st[k + "_E"].dtype == np.float64
        hi, lo, E = PC.reference(c)
        assert hi.shape == lo.shape == E.shape == (S, Nt)
        assert np.isfinite(hi).all() and np.isfinite(lo).all() and np.isfinite(E).all()
        assert (E > 0).all()
        assert (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)) * (1 + 1e-6)).all(), k
    assert len(st) == 4 * len({PC.key(c) for c in PC.CASES})


def _one_per_group():
    """The K-edge group and the cheapest case of every other group (a few seconds of mpmath)."""
    def cost(c):
        n, D, Nt, r, Q, S = c.shape
        return Nt * S * D * (n * min(r, Q) + Q)
    out = [c for c in PC.CASES if c.group == "GEMM K edge"]
    for g in PC.GROUPS:
        if g != "GEMM K edge":
            out.append(min((c for c in PC.CASES if c.group == g), key=cost))
    return out


@pytest.mark.parametrize("c", _one_per_group(), ids=PC.case_id)
def test_fixture_equals_mpmath(c):
    pytest.importorskip("mpmath")
    hi, lo, E = PC.compute(c)
    shi, slo, sE = PC.reference(c)
    assert np.array_equal(hi, shi) and np.array_equal(lo, slo) and np.array_equal(E, sE)


def test_bound_is_tight_on_every_case():
    """max E <= 1e-11·max|f|: the bound cannot hide an error ten times the project's bar."""
    worst = 0.0
    for c in PC.CASES:
        hi, lo, E = PC.reference(c)
        ratio = E.max() / np.abs(hi).max()
        worst = max(worst, ratio)
        assert ratio <= PC.SLACK, (PC.case_id(c), ratio)
    print("worst max E / max|f|: %.3g" % worst)


def test_numpy_oracle_within_the_bound():
    worst = {}
    for c in PC.CASES:
        ref = PC.reference(c)
        ratio = PC.err_abs(PC.oracle_pred(c), ref) / ref[2]
        worst[c.group] = max(worst.get(c.group, 0.0), ratio.max())
        assert (ratio <= 1.0).all(), (PC.case_id(c), ratio.max())
    for g in PC.GROUPS:
        print("numpy oracle, %s: worst error / E = %.3f" % (g, worst[g]))


def test_table_routes_are_the_dispatchs():
    """Every case's route is what the conditions of launch_pred_mfma / launch_vphase_rows give its
    shape, and the GEMM edge cases have the tile counts their group names."""
    for c in PC.CASES:
        assert (c.kind, c.tdim, c.npw) == PC.expected_route(c.shape, c.rows), PC.case_id(c)
    src = _pred_source()
    assert _int_list(src, "RowsPfDs") == PC.FIXED_D
    assert PC.gemm_tiles((6, 3, 300, 2, 6, 2)) == 9 and PC.gemm_tiles((6, 1, 20, 2, 2, 1)) == 1
    assert any(PC.gemm_tiles(c.shape) % 8 for c in PC.CASES)
    for s in PC.DIRECT_SHAPES:
        PC.find(s)


def test_table_reaches_every_instantiation():
    """Every DD of launch_vphase_rows' switch (and the run-time form at 10 and 16 rows per wave),
    every NT of vphase_pairs' switch and the one-tile rows kernel are in the table, but for the
    ones PC.HELD_ELSEWHERE names an existing test for."""
    src = _pred_source()
    dds, nts = set(_int_list(src, "RowsPfDs")), set(_int_list(src, "PairNTs"))
    assert dds == {2, 3, 4, 5, 6, 7, 8, 9, 10, 12} and nts == set(range(1, 9))
    have_dd = {c.tdim for c in PC.CASES if c.kind == PC.ROWS_PF and c.tdim > 0}
    have_nt = {c.tdim for c in PC.CASES if c.kind == PC.PAIRS}
    parity = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    for what, have, want in (("DD", have_dd, dds), ("NT", have_nt, nts)):
        for v in sorted(want - have):
            held = PC.HELD_ELSEWHERE[what, v]
            name = re.match(r"tests/test_gpu_parity.py::(\w+)\[", held).group(1)
            assert "def %s(" % name in parity, held
        assert not {v for w, v in PC.HELD_ELSEWHERE if w == what} & have
    assert {(c.tdim, c.npw) for c in PC.CASES if c.kind == PC.ROWS_PF} >= {(0, 10), (0, 16)}
    assert any(c.kind == PC.ROWS for c in PC.CASES)
    # the shapes the held-elsewhere ids name take those routes
    assert PC.expected_route((150, 8, 130, 20, 200, 4))[:2] == (PC.ROWS_PF, 8)
    assert PC.expected_route((5, 5, 100, 2, 32, 1))[:2] == (PC.PAIRS, 3)
    assert PC.expected_route((500, 8, 700, 5, 200, 40))[:2] == (PC.PAIRS, 4)
    assert PC.expected_route((5, 10, 100, 2, 100, 1))[:2] == (PC.PAIRS, 5)
    # Q > 1024 (w loaded at park) and fewer entries than the 16 waves
    assert any(c.kind == PC.ROWS_PF and c.shape[4] > 1024 for c in PC.CASES)
    assert any(c.kind == PC.ROWS_PF and c.shape[4] < 16 for c in PC.CASES)
