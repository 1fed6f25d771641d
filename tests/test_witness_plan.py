"""The column groups in which bj_prove brings a host witness over PCIe (csrc/witness_plan.h: host_witness_plan, called by
round 1 of csrc/prover.hip).  Host-only: the function is pure C++ and reaches this test through the host helper library
(build.build_canon_helper), so the public header does not grow by a test hook.

G is the group width as the plan loop receives it: the prover has by then widened it so that ceil(nW / G) <= 64 and, when it
absorbs, rounded it up to a multiple of 8 (the sponge's rate)."""
import ctypes as C
import json
import os

import pytest

from era_boojum_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_witness_plans.json")
NONE = 0xFFFFFFFF
_lib = None


def plan(nW, G, absorb, uniform):
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_canon_helper())
        _lib.bj_host_witness_plan.restype = C.c_size_t
        _lib.bj_host_witness_plan.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_size_t]
    count = _lib.bj_host_witness_plan(nW, G, int(absorb), int(uniform), None, 0)
    buf = (C.c_uint * (3 * count))()
    assert _lib.bj_host_witness_plan(nW, G, int(absorb), int(uniform), buf, count) == count
    return [(buf[3 * i], buf[3 * i + 1], -1 if buf[3 * i + 2] == NONE else buf[3 * i + 2]) for i in range(count)]


CASES = [(nW, G, absorb, uniform) for nW in (1, 7, 8, 9, 94, 513) for G in (8, 16) for absorb in (False, True)
         for uniform in (False, True)]


def test_recorded_plans():
    """The plans equal the ones the loop inside prove_impl produced before it became a function (recorded once from that loop,
    compiled as it stood)."""
    recorded = {(r["nW"], r["G"], r["absorb"], r["uniform"]): [tuple(g) for g in r["plan"]] for r in json.load(open(GOLDEN))}
    assert sorted(recorded) == sorted(CASES)
    for case in CASES:
        assert plan(*case) == recorded[case], case


@pytest.mark.parametrize("nW,G,absorb,uniform", CASES)
def test_plan_invariants(nW, G, absorb, uniform):
    groups = plan(nW, G, absorb, uniform)
    assert 1 <= len(groups) <= 64                      # one event per group, 64 events in the context
    pos = absorbed = 0
    for c0, c1, absorb_from in groups:                 # the groups tile [0, nW) contiguously
        assert c0 == pos and c1 > c0
        pos = c1
        if absorb_from >= 0:                           # an absorption run takes up where the previous one ended
            assert absorb and absorb_from == absorbed
            absorbed = c1
    assert pos == nW
    assert absorbed == (nW if absorb else 0)           # every column is hashed, or none is (one leaf kernel afterwards)
