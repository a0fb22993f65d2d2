"""The Julia ccalls of the softmax joint likelihood (julia/GPT_SGLD_HIP.jl) against their C
prototypes in include/gptsgld.h, with tests/test_julia_shim.py's parser; and that each of them
checks its argument lengths before the call."""
import re

import pytest

import test_julia_shim as TS

SYMS = ["gpt_gpnt_neglogjoint", "gpt_gpnt_joint_langevin", "gpt_gpnt_joint_scores"]


def calls():
    return {c[0]: c for c in TS.julia_ccalls(TS.JULIA[0])}


@pytest.mark.parametrize("sym", SYMS)
def test_ccall_matches_the_header(sym):
    protos = TS.header_prototypes()
    assert sym in protos and sym in calls()
    _, ret, types, args = calls()[sym]
    cret, cparams = protos[sym]
    assert ret in TS.C2J[cret]
    assert len(types) == len(cparams) == len(args)
    for i, (jt, ct) in enumerate(zip(types, cparams)):
        assert jt in TS.C2J[ct], "%s arg %d is %s, C wants %s" % (sym, i, jt, ct)


def test_handle_entries_are_declared():
    protos = TS.header_prototypes()
    for name in ("create", "eval", "set_theta", "get_theta", "langevin", "steps", "scores",
                 "scores_dev", "class_eval", "time", "destroy"):
        assert "gpt_cjoint_" + name in protos
    assert protos["gpt_cjoint_eval"][1][0] == "gpt_cjoint*"


@pytest.mark.parametrize("fn,sym", [("gpnt_joint", SYMS[0]), ("joint_langevin", SYMS[1]),
                                    ("joint_scores", SYMS[2])])
def test_lengths_are_checked_before_the_call(fn, sym):
    src = open(TS.JULIA[0]).read()
    body = src[src.index("function %s(" % fn):]
    body = body[:body.index("\nend\n")]
    at = body.index(":" + sym)
    head = body[:at]
    if "joint_dims(" in head:
        dims = src[src.index("function joint_dims("):]
        head += dims[:dims.index("\nend\n")]
    for what in ("length(b) == n", "hyperparams) == D + 1"):
        assert what in head, (fn, what)
    assert re.search(r"n \* C|size\(theta\)", head)


def test_python_signatures_match_the_header():
    """gpt_amd/_lib.py's argtypes of the new entries: one per C parameter."""
    from gpt_amd import _lib
    protos = TS.header_prototypes()
    names = [k for k in _lib.SIGNATURES if k.startswith("gpt_cjoint_") or k in SYMS]
    assert len(names) == 14
    for k in names:
        assert len(_lib.SIGNATURES[k][1]) == len(protos[k][1]), k
