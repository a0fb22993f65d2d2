"""wave_expm's register-resident Padé polynomial against its LDS form, on the device.

At NN <= 10 (every production size there: 1, 2, 3, 4, 5, 6, 8, 10) wave_expm keeps the current power,
U and V of the degree 3..9 polynomial in registers (gpt_debug_expm mode 1); mode 5 runs the same
function with the polynomial in its LDS form, the code every larger size still takes.  The two
perform the same floating-point operations in the same order, so the results must agree bit for
bit, flags included: no tolerance.

The inputs are oracle/expm_cases.py's: cases(nn) (tests/test_oracle.py checks on the CPU that they
take every Padé degree, the squaring branch, the diagonally dominant solve and the pivoting solve),
overflow_cases(nn) and the matrices with an Inf or NaN entry.  One wave per matrix, a few dozen
matrices per size.  The accuracy of mode 1 itself is held to mpmath in tests/test_gpu_expm.py.
"""
import numpy as np
import pytest

from oracle import expm_cases as XC

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 6, 8, 10)
REG_MODE, LDS_MODE = 1, 5


def device_expm(mode, nn, mats):
    """(E, bad) of gpt_debug_expm; the output buffer starts as zeros."""
    from gpt_amd import _lib
    Ah = np.ascontiguousarray(np.stack(mats), dtype=np.float64)
    E = np.zeros_like(Ah)
    bad = np.zeros(len(mats), dtype=np.int32)
    _lib.check(_lib.lib().gpt_debug_expm(nn, len(mats), mode, Ah.ctypes.data_as(_lib.P_D),
                                         E.ctypes.data_as(_lib.P_D), bad.ctypes.data_as(_lib.P_I32)))
    return E, bad


def assert_bitwise(nn, names, mats):
    Er, br = device_expm(REG_MODE, nn, mats)
    El, bl = device_expm(LDS_MODE, nn, mats)
    for k, name in enumerate(names):
        assert br[k] == bl[k], "%s: flag %d (registers) against %d (LDS)" % (name, br[k], bl[k])
        # the bit patterns, so that NaNs compare (sign and payload included) and -0.0 != 0.0
        assert np.array_equal(Er[k].view(np.uint64), El[k].view(np.uint64)), name
    return Er, br


@pytest.mark.parametrize("nn", SIZES)
def test_register_polynomial_matches_lds_form(nn):
    """Every matrix of cases(nn): degrees 3, 5, 7, 9 on the register path, degree 13 with and
    without squarings on the shared path, both solves."""
    cs = XC.cases(nn)
    degrees = {XC.branch_of_norm(XC.one_norm(X))[0] for _, _, X in cs}
    assert degrees >= {3, 5, 7, 9, 13}
    E, bad = assert_bitwise(nn, [name for name, _, _ in cs], [X for _, _, X in cs])
    assert not bad.any() and np.isfinite(E).all()


@pytest.mark.parametrize("nn", [n for n in SIZES if n >= 2])
def test_register_polynomial_matches_lds_form_on_overflow(nn):
    """The overflowing and the bounded shift of overflow_cases(nn): equal bits (the NaN pattern of
    the overflowed result included) and equal flags."""
    E, bad = assert_bitwise(nn, ["overflow", "bounded"], list(XC.overflow_cases(nn)))
    assert bad[0] == 1 and bad[1] == 0


@pytest.mark.parametrize("nn", SIZES)
def test_register_polynomial_matches_lds_form_on_nonfinite_input(nn):
    """An Inf or NaN entry: both forms return the flag and the same NaN fill."""
    cs = XC.nonfinite_cases(nn)
    E, bad = assert_bitwise(nn, [name for name, _ in cs], [X for _, X in cs])
    assert (bad == 1).all() and np.isnan(E).all()


def test_lds_form_mode_covers_the_register_sizes_only():
    """Mode 5 exists exactly where mode 1 takes the register path; other sizes are refused."""
    from gpt_amd import _lib
    for nn in (7, 9, 12, 16, 40):
        A = np.zeros((1, nn, nn))
        E = np.zeros_like(A)
        bad = np.zeros(1, dtype=np.int32)
        code = _lib.lib().gpt_debug_expm(nn, 1, LDS_MODE, A.ctypes.data_as(_lib.P_D),
                                         E.ctypes.data_as(_lib.P_D), bad.ctypes.data_as(_lib.P_I32))
        assert code == _lib.GPT_ERR_BAD_DIMS, nn
