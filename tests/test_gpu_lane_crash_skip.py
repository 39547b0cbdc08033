"""GPU: the per-lane component kernel (tlcg_componentp_64, component_lane.h)
with the BrokerCrash successor's code run only in the iterations where some
live lane of the wave has BrokerCrash enabled (TLCG_LANE_CRASH_SKIP=1, the
default) and in every iteration (=0, the A/B define): the golden results both
ways, error reports included, on the shapes where the two forms of the
expansion can go wrong -- S (729 components of 62 states: a partial last batch
of 25 lanes, both successors new in one expansion), X_keys3_vals57 (144
components, a last batch of 16), R_C2_K2 (BrokerCrash enabled at two values of
crashTimes), R_C3_K0 (MaxCrashTimes = 0: no iteration takes the form with the
second successor, and 63 lanes of the wave idle), V_leak and V_dup (lanes stop
at a level end while others go on, so dead and live lanes share a wave), each
of round 8's defines off beside the skip, the per-insert invariants
(TLCG_LANE_INV_FEAT=0), a 4-entry ring (lanes leave for the cascade mid-wave),
the outdegree kernel and user invariants.

Every golden case named here is taken by the per-lane pass (asserted through
jit_used).

Not covered: a wave in which some live lanes have a crash successor and
others do not.  Without a Producer every component of a cfg walks the same
code graph in the same order, so no cfg of this spec produces such a wave; it
would run the form with the second successor, which is the kernel with the
skip off."""
import json
import os

import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_parity import check_against_golden

pytestmark = pytest.mark.gpu

PER_LANE = {"TLCG_JIT": "1", "TLCG_COMP_WAVE": "0", "TLCG_TREE_WAVE": "0"}
ROUND8 = ["TLCG_LANE_OWNER_RING", "TLCG_LANE_FP_REG", "TLCG_LANE_LEVEL_LDS"]
ROUND8_OFF = ";".join(d + "=0" for d in ROUND8)
SKIP_OFF = "TLCG_LANE_CRASH_SKIP=0"
# the default build (skip on), the skip off, and the skip on beside each other define
VARIANTS = ["", SKIP_OFF] + [d + "=0" for d in ROUND8] + [ROUND8_OFF, "TLCG_LANE_INV_FEAT=0"]
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


@pytest.mark.parametrize("defines", VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_golden_case_each_form(case, defines, monkeypatch):
    run_case(case, defines, monkeypatch)


@pytest.mark.parametrize("defines", ["TLCG_LANE_R=4", "TLCG_LANE_R=4;" + SKIP_OFF])
@pytest.mark.parametrize("case", ["S", "V_leak"])
def test_short_ring_sends_lanes_to_the_cascade(case, defines, monkeypatch):
    run_case(case, defines, monkeypatch)


@pytest.mark.parametrize("defines", ["", SKIP_OFF])
@pytest.mark.parametrize("case", ["S", "R_C2_K2"])
def test_outdegree_kernel(case, defines, monkeypatch):
    """tlcg_componentpod_64: an expansion's new states (tail - tail0) are
    counted after whichever form ran"""
    per_lane(monkeypatch, defines)
    ck = tlcgpu.Checker(model_of(GOLDEN[case]["constants"]), outdegree=True)
    try:
        r = ck.run()
        check_against_golden(case, r, False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        assert ck.outdegree() == GOLDEN[case]["result"]["outdegree"]
    finally:
        ck.close()


@pytest.mark.parametrize("defines", ["", SKIP_OFF])
@pytest.mark.parametrize("case", ["U_PhaseKnown", "U_LedgerCount"])
def test_user_invariants(case, defines, monkeypatch):
    """a module with user invariants evaluates them per insert
    (check_invariants_cbt), so the form without BrokerCrash drops the second
    evaluation too: one fixture that holds and one that is violated, checked
    as test_gpu_user_inv.py checks the on-chip engines"""
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
