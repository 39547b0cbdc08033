"""GPU: the per-lane component kernel (tlcg_componentp_64, component_lane.h)
with the lane's FPSet and FIFO kept as a verified prefix of S's dense order
(TLCG_LANE_PREFIX=1, the default: membership is `dense index < tail`, the
state to expand is byidx[head]) and as round 9 kept them (=0, the A/B define:
a 64-bit register and a ring): the golden results both ways, error reports
included, on the shapes where the form can go wrong -- S (729 components of 62
states: a partial last batch of 25 lanes, and expansions whose two successors
are both new, so the second is judged against tail + 1), X_keys3_vals57 (a
last batch of 16), R_C2_K2 and R_C3_K0 (MaxCrashTimes = 0: only the form
without the second successor runs), V_leak and V_dup (lanes stop at a level
end beside live ones) -- the prefix form beside each other define, the
outdegree kernel and user invariants.

Every golden case named here is taken by the per-lane pass (asserted through
jit_used).

The hand-off: a lane whose insert is not the next of S's order leaves for the
cascade with the levels it has counted.  No cfg of this spec is known to do
that (tests/test_lane_prefix_host.py: every component of the golden cfgs and
8192 of G9's walk S in S's order), so the path is reached through the
test-only define TLCG_LANE_PREFIX_BREAK=p, which treats the insert at queue
position p as out of order in every lane: at the first insert, at the second
successor of an expansion that inserts two (found from the host BFS), and at
S's last position.  The results stay golden, so the cascade counted only the
levels left open.  Not covered: a real cfg whose component leaves S's order,
and a wave where only some lanes leave."""
import json
import os

import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_parity import check_against_golden

pytestmark = pytest.mark.gpu

PER_LANE = {"TLCG_JIT": "1", "TLCG_COMP_WAVE": "0", "TLCG_TREE_WAVE": "0"}
PREFIX_OFF = "TLCG_LANE_PREFIX=0"
# the default build, the prefix off, and the prefix beside each other define
VARIANTS = ["", PREFIX_OFF, "TLCG_LANE_CRASH_SKIP=0", "TLCG_LANE_INV_FEAT=0", "TLCG_LANE_LEVEL_LDS=0"]
CASES = ["S", "X_keys3_vals57", "R_C2_K2", "R_C3_K0", "V_leak", "V_dup"]

HERE = os.path.dirname(os.path.abspath(__file__))
USER = json.load(open(os.path.join(HERE, "golden", "user_inv.json")))


def per_lane(monkeypatch, defines):
    for k, v in PER_LANE.items():
        monkeypatch.setenv(k, v)
    if defines:
        monkeypatch.setenv("TLCG_JIT_DEFINES", defines)
    else:
        monkeypatch.delenv("TLCG_JIT_DEFINES", raising=False)


def run_case(case, defines, monkeypatch):
    per_lane(monkeypatch, defines)
    m = model_of(GOLDEN[case]["constants"])
    want = GOLDEN[case]["result"]
    ck = tlcgpu.Checker(m)
    try:
        r = ck.run()
        check_against_golden(case, r, False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        if want["result"] == "ok":
            assert ck.expansions() == r.distinct  # every state expanded once, by one pass
            return
        # the error report: TLC's trace, the end-of-level counts, TLC's stop counters
        assert r.tlc_exact, case
        assert [a for a, _ in r.trace] == [t["action"] for t in want["trace"]]
        assert [tlcgpu.decode(m, s) for _, s in r.trace] == [t["state"] for t in want["trace"]]
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
        assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"])
    finally:
        ck.close()


def break_positions(m):
    """queue positions of component 0's FIFO BFS in the kernel's order
    (compactor successor, then BrokerCrash's): the first insert, the second
    successor of the first expansion that inserts two, S's last position"""
    q = [tlcgpu.host_init_state(m, 0)]
    seen = {q[0]}
    second = None
    head = 0
    while head < len(q):
        new = []
        for action, t in tlcgpu.host_successors(m, q[head]):
            if t not in seen:
                seen.add(t)
                q.append(t)
                new.append(len(q) - 1)
        if len(new) == 2 and second is None:
            second = new[1]
        head += 1
    assert second is not None and 1 < second < len(q) - 1
    return {"first": 1, "second_of_two": second, "last": len(q) - 1}


@pytest.mark.parametrize("defines", VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_golden_case_each_form(case, defines, monkeypatch):
    run_case(case, defines, monkeypatch)


@pytest.mark.parametrize("where", ["first", "second_of_two", "last"])
@pytest.mark.parametrize("case", ["S", "V_leak"])
def test_an_insert_out_of_order_sends_the_lane_to_the_cascade(case, where, monkeypatch):
    """TLCG_LANE_PREFIX_BREAK=p: every lane leaves at the insert at position
    p, mid-wave, with the levels it has counted; the cascade redoes the
    components and counts the rest.  (No cfg of this spec is known to leave
    S's order by itself.)"""
    p = break_positions(model_of(GOLDEN[case]["constants"]))[where]
    run_case(case, "TLCG_LANE_PREFIX_BREAK=%d" % p, monkeypatch)


@pytest.mark.parametrize("defines", ["", PREFIX_OFF])
@pytest.mark.parametrize("case", ["S", "R_C2_K2"])
def test_outdegree_kernel(case, defines, monkeypatch):
    """tlcg_componentpod_64: an expansion's new states (tail - tail0) are
    counted the same with and without the ring"""
    per_lane(monkeypatch, defines)
    ck = tlcgpu.Checker(model_of(GOLDEN[case]["constants"]), outdegree=True)
    try:
        r = ck.run()
        check_against_golden(case, r, False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        assert ck.outdegree() == GOLDEN[case]["result"]["outdegree"]
    finally:
        ck.close()


@pytest.mark.parametrize("defines", ["", PREFIX_OFF])
@pytest.mark.parametrize("case", ["U_PhaseKnown", "U_LedgerCount"])
def test_user_invariants(case, defines, monkeypatch):
    """a module with user invariants evaluates them per insert on the states
    the prefix test calls new: one fixture that holds and one that is
    violated, checked as test_gpu_user_inv.py checks the on-chip engines"""
    per_lane(monkeypatch, defines)
    g = USER[case]
    m = tlcgpu.Model(invariants=tuple(g["invariants"]), user_defs=g["user_defs"], **g["constants"])
    want = g["result"]
    ck = tlcgpu.Checker(m)
    try:
        r = ck.run()
        assert r.status == want["result"], (case, r.status)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        if want["result"] == "ok":
            assert (r.generated, r.distinct, r.depth, r.levels) == (want["generated"], want["distinct"],
                                                                     want["depth"], want["levels"])
            assert ck.expansions() == r.distinct
            return
        assert r.tlc_exact and r.depth == want["depth"]
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
        assert r.invariant == want["invariant"]
        assert [a for a, _ in r.trace] == [t["action"] for t in want["trace"]]
        assert [tlcgpu.decode(m, s) for _, s in r.trace] == [t["state"] for t in want["trace"]]
        assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"])
    finally:
        ck.close()
