"""CPU tests of the C-ABI boundary: the library loads, exports every symbol include/gptsgld.h
declares, and its host-only entry points (no device work) agree with the oracle exactly."""
import os
import re

import numpy as np
import pytest

from oracle import gpt_sgld_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(ROOT, "include", "gptsgld.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|void|int64_t|char\s*\*|const char\s*\*)\s*\**\s*(gpt_\w+)\s*\(",
                       txt, flags=re.M)
    return sorted(set(names))


def test_header_declares_the_boundary():
    names = header_functions()
    for want in ["gpt_feature", "gpt_feature_notensor", "gpt_samplenz", "gpt_sgld_regression",
                 "gpt_pred", "gpt_pred_mean", "gpt_gpnt_sgld", "gpt_last_error",
                 "gpt_sgld_session_create", "gpt_sgld_session_run"]:
        assert want in names


def test_library_exports_every_header_symbol():
    from gpt_amd import _lib
    lib = _lib.lib()
    for name in header_functions():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_samplenz_host_matches_oracle():
    from gpt_amd import GPT_SGLD as G
    for (r, D, Q, s) in [(5, 8, 200, 17), (2, 5, 32, 3), (20, 8, 200, 1), (3, 3, 27, 2)]:
        assert (G.samplenz(r, D, Q, s) == R.samplenz(r, D, Q, s)).all()


def test_init_state_host_matches_oracle():
    from gpt_amd import GPT_SGLD as G
    for stf in (True, False):
        w, U = G.init_state(60, 5, 3, 40, 77, stiefel=stf)
        wo, Uo = R.init_state(60, 5, 3, 40, 77, stiefel=stf)
        assert np.abs(w - wo).max() == 0.0
        assert np.abs(U - Uo).max() < 1e-14


def test_feature_inputs_host_matches_oracle():
    from gpt_amd import GPT_SGLD as G
    Z, b = G.feature_inputs(30, 6, 17)
    Zo, bo = R.seeded_feature_inputs(30, 6, 17)
    assert np.abs(Z - Zo).max() < 1e-15 and np.abs(b - bo).max() < 1e-15


def test_feature_inputs_generation_a_host_matches_oracle():
    """Gen A (GPT_SGLD_p.jl:43-45): b = randn(n,D), not 2π·rand."""
    from gpt_amd import GPT_SGLD as G
    Z, b = G.feature_inputs_a(30, 6, 17)
    Zo, bo = R.seeded_feature_inputs_a(30, 6, 17)
    assert np.abs(Z - Zo).max() < 1e-15 and np.abs(b - bo).max() < 1e-15
    assert b.min() < 0.0                                   # normal, not uniform on [0, 2π)
    Zc, _ = G.feature_inputs(30, 6, 17)
    assert np.array_equal(Z, Zc)                           # the Z stream is shared with Gen C


BIG_SEED = (0x299f31d0 << 32) | 0xa4093822


def test_host_draws_take_the_whole_64_bit_seed():
    """gpt_samplenz, gpt_sgld_init and gpt_feature_inputs under a seed above 2^32 (the Philox key's
    second word is seed >> 32): equal to the oracle's, and not the draws of the low word alone."""
    from gpt_amd import GPT_SGLD as G
    low = BIG_SEED & 0xFFFFFFFF
    I = G.samplenz(5, 8, 200, BIG_SEED)
    assert (I == R.samplenz(5, 8, 200, BIG_SEED)).all()
    assert not (I == G.samplenz(5, 8, 200, low)).all()
    w, U = G.init_state(60, 5, 3, 40, BIG_SEED)
    wo, Uo = R.init_state(60, 5, 3, 40, BIG_SEED)
    assert np.abs(w - wo).max() == 0.0 and np.abs(U - Uo).max() < 1e-14
    wl, Ul = G.init_state(60, 5, 3, 40, low)
    assert np.abs(w - wl).max() > 1e-3 and np.abs(U - Ul).max() > 1e-3
    Z, b = G.feature_inputs(30, 6, BIG_SEED)
    Zo, bo = R.seeded_feature_inputs(30, 6, BIG_SEED)
    assert np.abs(Z - Zo).max() < 1e-15 and np.abs(b - bo).max() < 1e-15
    Zl, bl = G.feature_inputs(30, 6, low)
    assert np.abs(Z - Zl).max() > 1e-3 and np.abs(b - bl).max() > 1e-3


def test_host_philox_and_u53_equal_the_oracle():
    """The host C++ philox4x32 and u53 (gpt_debug_normals gen 6, no device work) on every seed and
    counter family of oracle/fastmath_cases.py and on the Random123 vectors."""
    from gpt_amd import _lib
    from oracle import fastmath_cases as FC
    from oracle import philox as P

    def host(case):
        seed, c0, nb, c1, c2, c3 = case
        z = np.zeros((nb, 2))
        w = np.zeros((nb, 4), dtype=np.uint32)
        _lib.check(_lib.lib().gpt_debug_normals(FC.GEN_HOST, seed, c0, nb, c1, c2, c3,
                                                z.ctypes.data_as(_lib.P_D),
                                                w.ctypes.data_as(_lib.P_U32)))
        return z, w
    for ctr, key, want in FC.KAT:
        _, w = host((key[0] | (key[1] << 32), ctr[0], 1, ctr[1], ctr[2], ctr[3]))
        assert tuple(int(v) for v in w[0]) == want
    for case in FC.stream_cases():
        z, w = host(case)
        assert np.array_equal(w, FC.case_words(case)), case
        assert np.array_equal(z[:, 0], P._u53(w[:, 0], w[:, 1]))
        assert np.array_equal(z[:, 1], P._u53(w[:, 2], w[:, 3]))


def test_bad_arguments_fail_without_device():
    from gpt_amd import GPT_SGLD as G
    from gpt_amd._lib import GPTError
    with pytest.raises(GPTError):
        G.samplenz(2, 3, 9, 0)          # Q > r^D
