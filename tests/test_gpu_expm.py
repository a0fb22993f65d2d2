"""The device matrix exponential at every size and branch the samplers use, through gpt_debug_expm:

  mode 0  wv_expm<NN> (wave engine), every column      mode 3  wave_expm<40, false> (LDS GEPP)
  mode 1  wave_expm<NN> (grid, chain, TGP, MovieLens)   mode 4  wv_expm<NN> with ncols = NN/2 (geod)

The inputs and the branch each one takes (Padé degree, squarings, diagonally dominant or pivoting
solve, row swaps) come from oracle/expm_cases.py; tests/test_oracle.py checks on the CPU that every
size sees every branch.  The reference is mpmath.expm at 60 digits (committed under tests/golden/,
recomputed for a matrix whose digest is not there).  Error measure: max|E − E_mp| / max|E_mp|.

Bounds:
  err_device <= 8·err_oracle + 1e-14 on every matrix, err_oracle being the error of the CPU oracle's
      expm on the same matrix: the device runs the same algorithm with another summation order, FMA
      contraction and Newton-refined pivot reciprocals, so its error is of the oracle's order.  (The
      worst measured ratios are in DESIGN.md §4.)
  device against R.expm directly below 1e-12 for the geodesic family up to 1-norm 40 (the bar of
      test_device_expm_all_pade_degrees).
Mode 4 is held to the same bounds on columns [0, NN/2), the ones geod reads.
"""
import functools

import numpy as np
import pytest

from oracle import expm_cases as XC
from oracle import gpt_sgld_ref as R

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 1e-14
IDS = ["mode%d-nn%d" % mn for mn in XC.MODE_NN]


def device_expm(mode, nn, mats):
    """(E, bad) of gpt_debug_expm; the output buffer starts as zeros."""
    from gpt_amd import _lib
    Ah = np.ascontiguousarray(np.stack(mats), dtype=np.float64)
    E = np.zeros_like(Ah)
    bad = np.zeros(len(mats), dtype=np.int32)
    _lib.check(_lib.lib().gpt_debug_expm(nn, len(mats), mode, Ah.ctypes.data_as(_lib.P_D),
                                         E.ctypes.data_as(_lib.P_D), bad.ctypes.data_as(_lib.P_I32)))
    return E, bad


def wanted_cols(mode, nn):
    return nn // 2 if mode == 4 else nn


@functools.lru_cache(maxsize=None)
def oracle_results(nn):
    """(R.expm(X), its error against mpmath) per matrix of cases(nn): computed once per size and
    shared by the modes."""
    out = []
    for (_, _, X), ref in zip(XC.cases(nn), XC.mp_reference(nn)):
        Eo = R.expm(X)
        out.append((Eo, XC.err_vs_mp(Eo, ref)))
    return tuple(out)


@pytest.mark.parametrize("mode,nn", XC.MODE_NN, ids=IDS)
def test_device_expm_against_mpmath(mode, nn):
    """Every finite matrix of the three families (geodesic, large-norm skew, row-swapping): no NaN
    flag, the device's error against mpmath within 8× the oracle's + 1e-14, and the direct 1e-12
    bar against the oracle for the geodesic family up to norm 40.  No matrix is left out of the
    mpmath comparison at any size."""
    cs = XC.cases(nn)
    refs = XC.mp_reference(nn)
    orc = oracle_results(nn)
    E, bad = device_expm(mode, nn, [X for _, _, X in cs])
    nc = wanted_cols(mode, nn)
    worst = 0.0
    failures = []
    for k, (name, family, X) in enumerate(cs):
        Eo, err_o = orc[k]
        err_d = XC.err_vs_mp(E[k][:, :nc], refs[k])
        worst = max(worst, err_d / err_o if err_o > 0 else 0.0)
        if bad[k]:
            failures.append("%s: bad flag" % name)
        if not err_d <= FACTOR * err_o + FLOOR:
            failures.append("%s: device %.3e, oracle %.3e" % (name, err_d, err_o))
        if family == "geodesic" and XC.one_norm(X) <= XC.DIRECT_BAR_NORM * (1 + 1e-9):
            d = np.abs(E[k][:, :nc] - Eo[:, :nc]).max() / np.abs(Eo).max()
            if not d < 1e-12:
                failures.append("%s: %.3e against the oracle" % (name, d))
    print("expm error ratio: mode %d nn %d worst device/oracle %.3f" % (mode, nn, worst))
    assert not failures, failures


@pytest.mark.parametrize("mode,nn", XC.MODE_NN, ids=IDS)
def test_device_expm_nonfinite_input_gives_nan(mode, nn):
    """One Inf or one NaN entry, in column 0 or in the last column: the flag is set and the result is
    all NaN, as the oracle's is (the early return used to leave stale scratch in the result)."""
    cs = XC.nonfinite_cases(nn)
    E, bad = device_expm(mode, nn, [X for _, X in cs])
    nc = wanted_cols(mode, nn)
    for k, (name, X) in enumerate(cs):
        assert np.isnan(R.expm(X)).all()
        assert bad[k] == 1, name
        assert np.isnan(E[k][:, :nc]).all(), name


@pytest.mark.parametrize("mode,nn", [mn for mn in XC.MODE_NN if mn[1] >= 2],
                         ids=[i for i, mn in zip(IDS, XC.MODE_NN) if mn[1] >= 2])
def test_device_expm_overflow_flag(mode, nn):
    """Squarings that overflow (largest exact entry above 1e600) raise the flag; the same matrix at a
    shift that keeps the result below 1e175 does not.  Nothing in between: the edge is left alone."""
    E, bad = device_expm(mode, nn, list(XC.overflow_cases(nn)))
    assert bad[0] == 1 and bad[1] == 0
    assert np.isfinite(E[1][:, :wanted_cols(mode, nn)]).all()


@pytest.mark.parametrize("mode,nn", [(0, 5), (0, 1), (1, 7), (1, 64), (3, 12), (4, 10), (4, 15),
                                     (5, 12), (-1, 12)])
def test_device_expm_rejects_other_pairs(mode, nn):
    """A (mode, nn) pair outside the table is GPT_ERR_BAD_DIMS."""
    from gpt_amd import _lib
    A = np.zeros((1, nn, nn))
    E = np.zeros_like(A)
    bad = np.zeros(1, dtype=np.int32)
    code = _lib.lib().gpt_debug_expm(nn, 1, mode, A.ctypes.data_as(_lib.P_D),
                                     E.ctypes.data_as(_lib.P_D), bad.ctypes.data_as(_lib.P_I32))
    assert code == _lib.GPT_ERR_BAD_DIMS
