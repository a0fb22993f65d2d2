"""CPU tests of the chain-diagnostics boundary (gpt_chain_diag, gpt_chain_diag_dev): every bad
argument fails with GPT_ERR_BAD_DIMS and its own message before any device call."""
import ctypes as C

import numpy as np
import pytest

P, T, M = 3, 12, 2
HOST = ["store", "P", "T", "M", "first", "last", "max_lag", "mean", "sd", "rhat", "ess", "mcse", "tau",
        "truncated", "chain_mean", "chain_var", "acf", "chain_acf"]
DEV = HOST[:4] + ["chain_stride"] + HOST[4:] + ["hip_stream"]
REQUIRED = ["store", "mean", "sd", "rhat", "ess", "mcse", "tau", "truncated"]
OPTIONAL = ["chain_mean", "chain_var", "acf", "chain_acf"]


def _values():
    v = dict(store=np.zeros(P * T * M), P=P, T=T, M=M, chain_stride=P * T, first=0, last=T, max_lag=5,
             truncated=np.zeros(P, dtype=np.int32), chain_mean=np.zeros(P * M),
             chain_var=np.zeros(P * M), acf=np.zeros(P * 6), chain_acf=np.zeros(P * 6 * M),
             hip_stream=None)
    v.update({k: np.zeros(P) for k in ("mean", "sd", "rhat", "ess", "mcse", "tau")})
    return v


def call(entry, **over):
    """gpt_chain_diag / gpt_chain_diag_dev on valid arguments with `over` replacing some (None: a
    null pointer).  The device entry gets host addresses: every refusal comes before they are used."""
    from gpt_amd import _lib
    v = _values()
    v.update(over)
    names = HOST if entry == "gpt_chain_diag" else DEV
    args = []
    for n in names:
        x = v[n]
        if isinstance(x, np.ndarray):
            if entry == "gpt_chain_diag":
                x = x.ctypes.data_as(_lib.P_I32 if x.dtype == np.int32 else _lib.P_D)
            else:
                x = C.c_void_p(x.ctypes.data)
        args.append(x)
    return getattr(_lib.lib(), entry)(*args)


def fails(rc, text):
    from gpt_amd import _lib
    assert rc == _lib.GPT_ERR_BAD_DIMS, rc
    with pytest.raises(_lib.GPTError) as ei:
        _lib.check(rc)
    assert ei.value.code == _lib.GPT_ERR_BAD_DIMS
    assert str(ei.value) == "gptsgld error %d: %s" % (_lib.GPT_ERR_BAD_DIMS, text), str(ei.value)


ENTRIES = ["gpt_chain_diag", "gpt_chain_diag_dev"]
WINDOW = "chain_diag: the window must satisfy 0 <= first < last <= T"
BAD = [
    (dict(P=0), "chain_diag: P must be >= 1"),
    (dict(P=-1), "chain_diag: P must be >= 1"),
    (dict(T=3, last=3), "chain_diag: T must be in 4..2^22"),
    (dict(T=(1 << 22) + 1), "chain_diag: T must be in 4..2^22"),
    (dict(M=0), "chain_diag: M must be in 1..1024"),
    (dict(M=1025), "chain_diag: M must be in 1..1024"),
    (dict(max_lag=0), "chain_diag: max_lag must be in 1..4096"),
    (dict(max_lag=4097), "chain_diag: max_lag must be in 1..4096"),
    (dict(first=-1), WINDOW),
    (dict(last=T + 1), WINDOW),
    (dict(first=5, last=5), WINDOW),
    (dict(first=7, last=6), WINDOW),
    (dict(first=2, last=5), "chain_diag: the window needs last - first >= 4"),
    (dict(first=T - 3), "chain_diag: the window needs last - first >= 4"),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", REQUIRED)
def test_null_required_argument_fails_without_a_device(entry, name):
    fails(call(entry, **{name: None}), "chain_diag: null argument")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("bad,text", BAD, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items())
                         if isinstance(d, dict) else None)
def test_bad_scalar_fails_without_a_device(entry, bad, text):
    fails(call(entry, **bad), text)


@pytest.mark.parametrize("entry", ENTRIES)
def test_optional_outputs_may_be_null(entry):
    """With every optional output null the call gets as far as the next refusal."""
    fails(call(entry, max_lag=0, **{n: None for n in OPTIONAL}), "chain_diag: max_lag must be in 1..4096")


def test_host_store_larger_than_one_upload_fails_without_a_device():
    fails(call("gpt_chain_diag", P=(1 << 31) // (64 * 8) + 1, T=64, M=8, last=64),
          "chain_diag: the store must hold at most 2^31 doubles (16 GiB)")


@pytest.mark.parametrize("stride", [P * T - 1, 0, -5])
def test_device_chain_stride_below_one_chain_fails_without_a_device(stride):
    fails(call("gpt_chain_diag_dev", chain_stride=stride), "chain_diag: chain_stride must be >= P*T")


def test_timing_and_tiling_entries():
    from gpt_amd import _lib
    import diag_ref as DR
    fails(_lib.lib().gpt_diag_last_timing(None), "gpt_diag_last_timing: null output")
    fails(_lib.lib().gpt_diag_tiling(None, 3), "gpt_diag_tiling: needs room for 3 values")
    out = np.full(4, -1, dtype=np.int32)
    fails(_lib.lib().gpt_diag_tiling(out.ctypes.data_as(_lib.P_I32), 2), "gpt_diag_tiling: needs room for 3 values")
    assert _lib.lib().gpt_diag_tiling(out.ctypes.data_as(_lib.P_I32), 4) == 0
    # the edges tests/diag_ref.py places its cases at are the kernel's
    assert out.tolist() == [DR.TC, DR.KB, DR.KG, 0]


def test_python_wrapper_refuses_before_the_library():
    from gpt_amd import GPT_SGLD as G
    x = np.zeros((P, T, M))
    for window in [(0, 3), (5, 5), (-1, 8), (0, T + 1)]:
        with pytest.raises(ValueError):
            G.chain_diagnostics(x, window=window)
    with pytest.raises(ValueError):
        G.chain_diagnostics(np.zeros((2, 3, 4, 5)))
    with pytest.raises(ValueError):
        G.chain_diagnostics([np.zeros((2, T)), np.zeros((3, T))])
    with pytest.raises(G.GPTError) as ei:
        G.chain_diagnostics(x, max_lag=0)
    assert ei.value.code == G.GPT_ERR_BAD_DIMS
