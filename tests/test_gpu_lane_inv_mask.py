"""GPU: the per-lane component kernel (tlcg_componentp_64, component_lane.h)
with its inserts' built-in invariants read from the owner table's feature
words (TLCG_LANE_INV_FEAT=1, the default) and evaluated per insert
(TLCG_LANE_INV_FEAT=0, the A/B define): the golden results both ways, error
reports included."""
import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_parity import check_against_golden

pytestmark = pytest.mark.gpu

PER_LANE = {"TLCG_JIT": "1", "TLCG_COMP_WAVE": "0", "TLCG_TREE_WAVE": "0"}
CASES = ["S", "S_noretain", "S_consumer", "V_leak", "V_dup", "R_C2_K2", "X_keys3_vals57", "D_N0_K1"]
G9 = dict(key_space=range(1, 16), value_space=range(1, 16))


def per_lane(monkeypatch, feat):
    for k, v in PER_LANE.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TLCG_JIT_DEFINES", "TLCG_LANE_INV_FEAT=" + feat)


@pytest.mark.parametrize("feat", ["1", "0"])
@pytest.mark.parametrize("case", CASES)
def test_golden_case_lane_inv(case, feat, monkeypatch):
    per_lane(monkeypatch, feat)
    m = model_of(GOLDEN[case]["constants"])
    want = GOLDEN[case]["result"]
    ck = tlcgpu.Checker(m)
    try:
        r = ck.run()
        check_against_golden(case, r, False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        if case == "S":  # every state is still expanded, and has its invariants decided, on its own
            assert ck.expansions() == r.distinct
        if want["result"] == "ok":
            return
        # the error report: TLC's trace, the end-of-level counts, TLC's stop counters
        assert r.tlc_exact, case
        assert [a for a, _ in r.trace] == [t["action"] for t in want["trace"]]
        assert [tlcgpu.decode(m, s) for _, s in r.trace] == [t["state"] for t in want["trace"]]
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
        assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"])
    finally:
        ck.close()


@pytest.mark.parametrize("feat", ["1", "0"])
def test_g9_some_m_lane_inv(feat, monkeypatch):
    """G9_some_M holds 100 of G9's 16^6 components (initial states 123456 ..
    123555); a context runs whole rank shares, not a range of initial states,
    so G9 runs whole and must give 16^6 / 100 times the fixture's counts,
    level by level (every component has the same code graph)"""
    per_lane(monkeypatch, feat)
    want = GOLDEN["G9_some_M"]["result"]
    lo, hi = GOLDEN["G9_some_M"]["constants"]["init_range"]
    n = 16 ** 6
    ck = tlcgpu.Checker(tlcgpu.Model(**G9))
    try:
        r = ck.run(with_trace=False)
        assert r.engine == "component" and r.jit_used & 32 and not r.jit_used & 8, r.jit_used
        assert r.status == want["result"] == "ok" and r.depth == want["depth"]
        assert (r.generated * (hi - lo), r.distinct * (hi - lo)) == (n * want["generated"], n * want["distinct"])
        assert [x * (hi - lo) for x in r.levels] == [n * x for x in want["levels"]]
        assert ck.expansions() == r.distinct
    finally:
        ck.close()
