"""The Julia ccalls of the posterior predictive (julia/GPT_SGLD_HIP.jl) against their C prototypes
in include/gptsgld.h, with tests/test_julia_shim.py's parser; that each of them checks its argument
lengths before the call; and that the names are exported."""
import pytest

import test_julia_shim as TS

BOUND = {"predictive": "gpt_predictive", "pred_predictive": "gpt_pred_predictive",
         "pred_predictive_x": "gpt_pred_predictive_x", "GPNT_predictive": "gpt_gpnt_predictive",
         "GPNT_predictive_x": "gpt_gpnt_predictive_x"}
# what each function has to have compared before its ccall
CHECKS = {
    "predictive": ["length(ytest) == Nt", "0 <= a < b <= T"],
    "pred_predictive": ["size(U_store) == (n, r, D, S)", "size(I) == (Q, D)", "length(ytest) == Nt",
                        "0 <= a < b <= S"],
    "pred_predictive_x": ["size(U_store) == (n, r, D, S)", "size(I) == (Q, D)", "length(ytest) == Nt",
                          "length(bfeat) == n * D", "length(ls) == D", "0 <= a < b <= S"],
    "GPNT_predictive": ["size(phitest, 1) == n", "length(ytest) == Nt", "0 <= a < b <= T"],
    "GPNT_predictive_x": ["size(Z) == (n, D)", "length(bfeat) == n", "length(ls) == D",
                          "length(ytest) == Nt", "0 <= a < b <= T"],
}


def calls():
    return {c[0]: c for c in TS.julia_ccalls(TS.JULIA[0])}


@pytest.mark.parametrize("sym", sorted(BOUND.values()))
def test_ccall_matches_the_header(sym):
    protos = TS.header_prototypes()
    assert sym in protos and sym in calls()
    _, ret, types, args = calls()[sym]
    cret, cparams = protos[sym]
    assert ret in TS.C2J[cret]
    assert len(types) == len(cparams) == len(args)
    for i, (jt, ct) in enumerate(zip(types, cparams)):
        assert jt in TS.C2J[ct], "%s arg %d is %s, C wants %s" % (sym, i, jt, ct)


@pytest.mark.parametrize("fn", sorted(BOUND))
def test_lengths_are_checked_before_the_call(fn):
    src = open(TS.JULIA[0]).read()
    body = src[src.index("function %s(" % fn):]
    body = body[:body.index("\nend\n")]
    head = body[:body.index(":" + BOUND[fn] + ",")]
    for what in CHECKS[fn]:
        assert what in head, (fn, what)
    # the outputs are allocated from the checked sizes
    assert "PredictiveOut(Nt, " in head


def test_names_are_exported_and_outputs_sized():
    src = open(TS.JULIA[0]).read()
    exported = src.split("module GPT_SGLD_HIP")[1].split("const LIB")[0]
    for name in BOUND:
        assert name in exported, name
    assert "PredictiveOut(Nt, T) = PredictiveOut(zeros(Nt), zeros(Nt), zeros(Nt), zeros(Nt), zeros(2), zeros(1)," in src


def test_python_signatures_match_the_header():
    from gpt_amd import _lib
    protos = TS.header_prototypes()
    for k in list(BOUND.values()) + ["gpt_predictive_dev", "gpt_predictive_last_timing"]:
        assert len(_lib.SIGNATURES[k][1]) == len(protos[k][1]), k
