"""CPU tests of the chain diagnostics' restatements (tests/diag_ref.py): the numpy restatement of
the device's order against mpmath on every case, against an independent literal restatement, the
condition on the inputs that makes the Geyer walk well defined, the planted defects the bar has to
see, and what the numbers mean on AR(1) chains of known autocorrelation time."""
import math

import numpy as np
import pytest

import diag_ref as DR

pytest.importorskip("mpmath")


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_restatement_against_mpmath(name):
    got, ref, ys = DR.restated(name), DR.reference(name), DR.yardstick(name)
    S = DR.CASES[name]["window"][1] - DR.CASES[name]["window"][0]
    for q in DR.QUANTITIES:
        assert ys[q] <= (S + 16) * DR.U, (name, q, ys[q] / DR.U)
    assert np.array_equal(got["truncated"], ref["truncated"])
    assert np.array_equal(got["stop"], ref["stop"])
    assert got["K"] == ref["K"] == min(DR.CASES[name]["max_lag"], S - 1)


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_the_geyer_walk_is_well_defined_on_the_inputs(name):
    assert DR.reference(name)["margin"] >= 1e-9


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_restatement_equals_the_literal_one(name):
    x, (a, b), max_lag = DR.inputs(name)
    # np.mean and np.var of 1e3 + 1e-2 z carry 1e3·2^-53/1e-2 = 1e-11 of their own: the literal
    # restatement takes the offset out first (x − 1e3 is exact there), as nothing else depends on it
    shift = 1e3 if DR.CASES[name]["kind"] == "offset" else 0.0
    got, lit = DR.restated(name), DR.literal_np(x - shift, a, b, max_lag)
    assert np.array_equal((x - shift) + shift, x)
    lit["mean"], lit["chain_mean"] = lit["mean"] + shift, lit["chain_mean"] + shift
    live = np.ones(x.shape[0], dtype=bool)
    if DR.CASES[name]["kind"] == "const":
        live[DR.CONST_ROW] = False                   # the literal variance of equal values is not 0
    for q in DR.QUANTITIES:
        g, w = np.asarray(got[q])[live], np.asarray(lit[q])[live]
        assert np.array_equal(np.isnan(g), np.isnan(w)), q
        assert np.nanmax(np.abs(g - w)) <= 1e-12 * max(1.0, np.nanmax(np.abs(w))), (name, q)
    assert np.array_equal(got["truncated"][live], lit["truncated"][live])


def test_the_cases_show_what_they_are_named_for():
    r = DR.restated("p65_s200_trunc")
    assert 10 <= r["truncated"].sum() < 65           # K = 32 is too few lags at phi = 0.9 for many rows
    r = DR.restated("shifted_chain")
    assert (r["rhat"] >= 1.28).all() and (r["truncated"] == 1).all()
    r = DR.restated("antithetic")
    assert np.median(r["tau"]) < 1.0
    r = DR.restated("constant_row")
    for q in ("rhat", "ess", "mcse", "tau"):
        assert np.isnan(r[q][DR.CONST_ROW]) and np.isfinite(np.delete(r[q], DR.CONST_ROW)).all()
    assert np.isnan(r["acf"][DR.CONST_ROW]).all() and r["truncated"][DR.CONST_ROW] == 0
    assert r["sd"][DR.CONST_ROW] == 0.0
    assert DR.CASES["p63_s5"]["T"] % 2 == 1


@pytest.mark.parametrize("defect", sorted(DR.DEFECTS))
def test_the_bar_sees_a_planted_defect(defect):
    name = DR.DEFECTS[defect]
    x, (a, b), max_lag = DR.inputs(name)
    bad = DR.diag_np(x, a, b, max_lag, defect=defect)
    err = DR.errors(bad, name)
    seen = [q for q in DR.QUANTITIES if err[q] > DR.bar(name, q)]
    assert seen, (defect, name)


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ess_of_ar1_is_the_textbook_one(phi):
    P, T, M = 257, 1000, 4
    x = DR.ar1(np.random.default_rng(7), P, T, M, phi)
    d = DR.diag_np(x, 0, T, T - 1)
    ratio = np.median(d["ess"] / (M * T * (1 - phi) / (1 + phi)))
    assert 0.9 <= ratio <= 1.1, ratio
    assert d["rhat"].max() < 1.06
