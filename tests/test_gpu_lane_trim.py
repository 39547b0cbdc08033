"""GPU: the per-lane component kernel (tlcg_componentp_64, component_lane.h)
with each round-8 change on (the default build), off (its A/B define) and
all off: the
golden results, error reports included, on the shapes where they can go
wrong -- S (729 components of 62 states: a partial last batch of 25 lanes,
dense indices across bit 31/32, both successors new in one expansion), V_leak
and V_dup (a stop at a level end, event keys, TLC's stop counters), R_C2_K2,
and a 4-entry ring on S and V_leak (lanes leaving for the cascade mid-wave
with the levels they already counted)."""
import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_parity import check_against_golden

pytestmark = pytest.mark.gpu

PER_LANE = {"TLCG_JIT": "1", "TLCG_COMP_WAVE": "0", "TLCG_TREE_WAVE": "0"}
DEFINES = ["TLCG_LANE_OWNER_RING", "TLCG_LANE_FP_REG", "TLCG_LANE_LEVEL_LDS"]
ALL_OFF = ";".join(d + "=0" for d in DEFINES)
VARIANTS = [""] + [d + "=0" for d in DEFINES] + [ALL_OFF]


def run_case(case, defines, monkeypatch):
    for k, v in PER_LANE.items():
        monkeypatch.setenv(k, v)
    if defines:
        monkeypatch.setenv("TLCG_JIT_DEFINES", defines)
    else:
        monkeypatch.delenv("TLCG_JIT_DEFINES", raising=False)
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
        assert r.tlc_exact, case
        assert [a for a, _ in r.trace] == [t["action"] for t in want["trace"]]
        assert [tlcgpu.decode(m, s) for _, s in r.trace] == [t["state"] for t in want["trace"]]
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
        assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"])
    finally:
        ck.close()


@pytest.mark.parametrize("defines", VARIANTS)
@pytest.mark.parametrize("case", ["S", "V_leak", "V_dup", "R_C2_K2"])
def test_golden_case_each_define(case, defines, monkeypatch):
    run_case(case, defines, monkeypatch)


@pytest.mark.parametrize("defines", ["TLCG_LANE_R=4", "TLCG_LANE_R=4;" + ALL_OFF])
@pytest.mark.parametrize("case", ["S", "V_leak"])
def test_short_ring_sends_lanes_to_the_cascade(case, defines, monkeypatch):
    run_case(case, defines, monkeypatch)


@pytest.mark.parametrize("defines", ["", ALL_OFF, "TLCG_LANE_R=4"])
@pytest.mark.parametrize("case", ["S", "R_C2_K2"])
def test_outdegree_variant(case, defines, monkeypatch):
    """tlcg_componentpod_64: the outdegree counts ride in the lane's generated
    count and the workgroup's level sums"""
    for k, v in PER_LANE.items():
        monkeypatch.setenv(k, v)
    if defines:
        monkeypatch.setenv("TLCG_JIT_DEFINES", defines)
    else:
        monkeypatch.delenv("TLCG_JIT_DEFINES", raising=False)
    ck = tlcgpu.Checker(model_of(GOLDEN[case]["constants"]), outdegree=True)
    try:
        r = ck.run()
        check_against_golden(case, r, False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        assert ck.outdegree() == GOLDEN[case]["result"]["outdegree"]
    finally:
        ck.close()
