"""The Julia ccall of the chain diagnostics (julia/GPT_SGLD_HIP.jl) against its C prototype in
include/gptsgld.h, with tests/test_julia_shim.py's parser; that it checks its argument lengths
before the call; and that the name is exported."""
import test_julia_shim as TS

SYM, FN = "gpt_chain_diag", "chain_diagnostics"
CHECKS = ["ndims(store) in (2, 3)", "length(store) == P * T * M", "0 <= a < b <= T", "b - a >= 4",
          "1 <= lag <= 4096"]


def calls():
    return {c[0]: c for c in TS.julia_ccalls(TS.JULIA[0])}


def test_ccall_matches_the_header():
    protos = TS.header_prototypes()
    assert SYM in protos and SYM in calls()
    _, ret, types, args = calls()[SYM]
    cret, cparams = protos[SYM]
    assert ret in TS.C2J[cret]
    assert len(types) == len(cparams) == len(args) == 18
    for i, (jt, ct) in enumerate(zip(types, cparams)):
        assert jt in TS.C2J[ct], "%s arg %d is %s, C wants %s" % (SYM, i, jt, ct)


def test_lengths_are_checked_before_the_call():
    src = open(TS.JULIA[0]).read()
    body = src[src.index("function %s(" % FN):]
    body = body[:body.index("\nend\n")]
    head = body[:body.index(":" + SYM + ",")]
    for what in CHECKS:
        assert what in head, what
    # the outputs are allocated from the checked sizes, the optional ones from K = min(lag, S - 1)
    for alloc in ["zeros(P) for _ = 1:6", "zeros(Int32, P)", "zeros(P, M)", "zeros(P, K + 1)",
                  "zeros(P, K + 1, M)", "K = min(lag, S - 1)"]:
        assert alloc in head, alloc
    tail = body[body.index(":" + SYM + ","):]
    assert "ac === nothing ? C_NULL : ac" in tail and "ca === nothing ? C_NULL : ca" in tail


def test_name_is_exported():
    src = open(TS.JULIA[0]).read()
    exported = src.split("module GPT_SGLD_HIP")[1].split("const LIB")[0]
    assert FN in exported


def test_python_signatures_match_the_header():
    from gpt_amd import _lib
    protos = TS.header_prototypes()
    for k in [SYM, "gpt_chain_diag_dev", "gpt_diag_last_timing", "gpt_diag_tiling"]:
        assert len(_lib.SIGNATURES[k][1]) == len(protos[k][1]), k
