"""GPU: PROPERTY Termination (compaction.tla:303-307) checked by the HIP
liveness pass (tlcg_check_termination, csrc/liveness.hip) against the golden
liveness results of the oracles -- the C oracle's Tarjan SCC restatement,
cross-checked with the Python oracle's DFS (tests/golden/make_golden.py) --
under Spec (no fairness, compaction.tla:233) and Spec /\\ WF_vars(Next).

What is pinned: holds / fails, |G'| (the states reachable from Init through
not-P states), its initial states and edges, the states where a behavior may
stutter forever, and the depth of the shallowest one.  Which counterexample is
printed is [TLC-ext]: the test checks that the returned one is a behavior of
the spec that never reaches P and ends where the fairness allows stuttering."""
import functools
import json
import subprocess

import pytest

import tlcgpu
from conftest import GOLDEN, ORACLE, model_of
from liveness_ref import Reference, counts_of, model_graph
from test_gpu_random_cfgs import random_model
from test_gpu_tree import random_producer_model

pytestmark = pytest.mark.gpu

LIVE_CASES = sorted(k for k, v in GOLDEN.items() if "liveness" in v)
G9 = dict(key_space=range(1, 16), value_space=range(1, 16))


def is_p(m, s):
    """Termination's predicate P: the guard of Terminating (:205-214), i.e.
    Terminating is among the state's successors (it needs P and nothing else)"""
    return any(a == "Terminating" for a, _ in tlcgpu.host_successors(m, s))


def check_counterexample(m, lv):
    assert lv.kind == "stuttering" and lv.loop_to == -1
    tr = lv.trace
    assert tr and tr[0][0] == "Init"
    assert tr[0][1] in {tlcgpu.host_init_state(m, i) for i in range(tlcgpu.init_count(m))}
    for (_, s), (a, t) in zip(tr, tr[1:]):
        assert (a, t) in tlcgpu.host_successors(m, s)
    assert not any(is_p(m, s) for _, s in tr)
    if lv.fairness == "wf":  # <<Next>>_vars disabled at the end: every successor is a stutter
        last = tr[-1][1]
        assert all(t == last for _, t in tlcgpu.host_successors(m, last))


@pytest.mark.parametrize("fair", ["none", "wf"])
@pytest.mark.parametrize("case", LIVE_CASES)
def test_termination_golden(case, fair):
    want = GOLDEN[case]["liveness"][fair]
    m = model_of(GOLDEN[case]["constants"])
    lv = tlcgpu.check_termination(m, fair)
    assert lv.holds == want["holds"], (case, fair)
    assert (lv.states_notp, lv.init_notp, lv.edges_notp, lv.stuck) == \
           (want["states_notp"], want["init_notp"], want["edges_notp"], want["stuck"]), (case, fair)
    assert (lv.on_cycles == 0) == (want["cyclic_sccs"] == 0)
    if want["holds"]:
        assert lv.kind == "holds" and lv.trace == []
        return
    check_counterexample(m, lv)
    if fair == "none":
        # Spec has no fairness: the first not-P initial state in Init order, then
        # stuttering -- the same state as the host closed form
        assert len(lv.trace) == 1
        assert lv.trace[0][1] == tlcgpu.host_init_state(m, tlcgpu.load_library().tlcg_host_termination_counterexample(
            m.to_c()))
    else:
        assert len(lv.trace) == want["stuck_min_depth"]  # a shallowest stuck state


def test_termination_regrows():
    """a store / FPSet far too small for G' is grown and the BFS redone"""
    m = model_of(GOLDEN["S_consumer"]["constants"])
    want = GOLDEN["S_consumer"]["liveness"]["wf"]
    lv = tlcgpu.check_termination(m, "wf", state_capacity=100, log2_fpset_slots=8)
    assert (lv.holds, lv.states_notp, lv.edges_notp, lv.stuck) == \
           (False, want["states_notp"], want["edges_notp"], want["stuck"])
    assert len(lv.trace) == want["stuck_min_depth"]


def test_termination_wide_states():
    """a > 63-bit layout (CompactionTimesLimit = 12): two-word states through
    the wide FPSet"""
    case = "W_C12_k1"
    m = model_of(GOLDEN[case]["constants"])
    assert tlcgpu.state_words(m) == 2
    for fair in ("none", "wf"):
        want = GOLDEN[case]["liveness"][fair]
        lv = tlcgpu.check_termination(m, fair)
        assert (lv.holds, lv.states_notp, lv.edges_notp, lv.stuck) == \
               (want["holds"], want["states_notp"], want["edges_notp"], want["stuck"])


def test_termination_g9_scaled():
    """G9 (~1e9 reachable states): components are isomorphic (SURVEY App.A.1),
    so G' is 16^6 times S's per-component figures: 57 not-P states and 71 edges
    per initial message sequence; under WF_vars(Next) no stuck state and no
    cycle, so Termination holds; without fairness it fails at the first
    initial state."""
    m = tlcgpu.Model(**G9)
    s = GOLDEN["S"]["liveness"]["wf"]
    per_state, per_edge = s["states_notp"] // 729, s["edges_notp"] // 729
    assert (per_state, per_edge) == (57, 71)
    lv = tlcgpu.check_termination(m, "wf", state_capacity=16 ** 6 * per_state + 1024)
    assert lv.holds and lv.kind == "holds"
    assert (lv.states_notp, lv.init_notp, lv.edges_notp, lv.stuck, lv.on_cycles) == \
           (16 ** 6 * per_state, 16 ** 6, 16 ** 6 * per_edge, 0, 0)
    print(f"G9 Termination under WF_vars(Next): {lv.states_notp} states, {lv.edges_notp} edges, "
          f"{lv.peel_rounds} peel rounds, kernels {lv.kernel_ms:.1f} ms, call {lv.wall_ms:.1f} ms")


# ---- the model path against the plain reference (tests/liveness_ref.py) and
# against the explicit-graph instantiation of the same kernels ----

REF_CASES = ["D_N0_K1_nodeadlock", "R_C1_K2", "X_empty_spaces", "S", "S_consumer", "X_producer_sparse"]


@functools.lru_cache(maxsize=None)
def model_ref(case):
    g, _ = model_graph(model_of(GOLDEN[case]["constants"]))
    return Reference(g)


@pytest.mark.parametrize("fair", ["none", "wf"])
@pytest.mark.parametrize("case", REF_CASES)
def test_termination_matches_reference(case, fair):
    """depth (non-empty BFS levels), the Kahn rounds, what peeling leaves and
    the stuck count are the reference's on the model's graph (model_graph),
    like every other count; the same graph as CSR through
    tlcg_liveness_graph_selftest -- the kernels' other instantiation -- gives
    identical counts"""
    ref = model_ref(case)
    want = ref.counts(fair)
    lv = tlcgpu.check_termination(model_of(GOLDEN[case]["constants"]), fair)
    assert (lv.depth, lv.peel_rounds, lv.on_cycles, lv.stuck) == \
           (want["depth"], want["peel_rounds"], want["on_cycles"], want["stuck"]), (case, fair)
    assert counts_of(lv) == want, (case, fair)
    g = ref.g
    gv = tlcgpu.liveness_graph(g.row, g.col, g.is_p, g.n_init, fairness=fair)
    assert counts_of(gv) == counts_of(lv), (case, fair)
    assert len(gv.trace) == len(lv.trace)


def oracle_liveness(m, fair):
    out = subprocess.run([ORACLE] + m.oracle_args() + ["-liveness", fair], check=True, capture_output=True,
                         text=True).stdout
    return json.loads(out)


@pytest.mark.parametrize("seed", range(20))
@pytest.mark.parametrize("gen", [random_model, random_producer_model], ids=lambda f: f.__name__)
def test_termination_random_cfg_matches_oracle(gen, seed):
    """seeded random constant sets against tlc_oracle -liveness none|wf run live"""
    m = gen(seed)
    assert tlcgpu.check_model(m) is None
    for fair in ("none", "wf"):
        want = oracle_liveness(m, fair)
        assert not want["error"]
        lv = tlcgpu.check_termination(m, fair)
        assert lv.holds == want["holds"], (seed, fair)
        assert (lv.states_notp, lv.init_notp, lv.edges_notp, lv.stuck) == \
               (want["states_notp"], want["init_notp"], want["edges_notp"], want["stuck"]), (seed, fair)
        assert lv.on_cycles == 0 and want["cyclic_sccs"] == 0
        if fair == "wf":
            assert len(lv.trace) == want["stuck_min_depth"]
        if not lv.holds:
            check_counterexample(m, lv)


@pytest.mark.parametrize("case", ["W_C12_k1", "X_producer_sparse"])
def test_termination_regrows_wide_and_producer(case):
    """the grow-and-redo path on two-word states and on a Producer's fan-out:
    from a 100-state store and a 256-slot FPSet, the unforced run's result"""
    m = model_of(GOLDEN[case]["constants"])
    for fair in ("none", "wf"):
        want = GOLDEN[case]["liveness"][fair]
        full = tlcgpu.check_termination(m, fair)
        lv = tlcgpu.check_termination(m, fair, state_capacity=100, log2_fpset_slots=8)
        assert (lv.holds, lv.states_notp, lv.init_notp, lv.edges_notp, lv.stuck) == \
               (want["holds"], want["states_notp"], want["init_notp"], want["edges_notp"], want["stuck"])
        assert counts_of(lv) == counts_of(full)
        # (the path's inner states depend on which parent won; its end and length do not)
        assert len(lv.trace) == len(full.trace) and lv.trace[-1:] == full.trace[-1:]
        if not lv.holds:
            check_counterexample(m, lv)
