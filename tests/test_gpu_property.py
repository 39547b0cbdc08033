"""GPU: properties the user defines -- <>Q, []<>Q, P ~> Q -- checked by the
seeded liveness pass (tlcg_check_property, csrc/liveness.hip) against the plain
reference of tests/property_ref.py over the model's reachable graph, with P
and Q of every node taken from the Python oracle (oracle_py.inv on the
operands, tests/property_cases.py): nothing the device computes feeds the
expectation.  Every field is compared, the trace is checked by
check_counterexample and, step by step, against tlcgpu.host_successors.

The spec's graph is acyclic for every cfg, so the cycle verdict, the copy-out
of the states left after peeling and the lasso are reached through
tlcg_property_graph_selftest only: the explicit graphs of
tests/liveness_graph_cases.py with Q = their P and a seeded P."""
import functools
import random

import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from liveness_graph_cases import HAND, PARAMS, STARRED, random_graph
from liveness_ref import counts_of as lv_counts_of
from property_cases import PROPS, model_pgraph, prop_model, reachable_pairs
from property_ref import FORMS, PropertyReference, check_counterexample, counts_of, pgraph_of

pytestmark = pytest.mark.gpu

FAIR = ("none", "wf")
MODEL_CASES = ["R_C1_K2", "R_C2_K1", "D_N0_K1_nodeadlock", "S", "X_producer_sparse"]
MODEL_PROPS = ["A", "B", "C", "D", "E", "E_box"]


@functools.lru_cache(maxsize=None)
def model_ref(case, prop):
    g, index = model_pgraph(case, "E" if prop == "E_box" else prop)
    return PropertyReference(g, PROPS[prop][0]), index


def check_model_trace(case, m, ref, index, fair, pr):
    """the trace is a behavior of the spec (initial state, then successors by
    the actions named) and the counterexample the header documents"""
    words = [w for w, _ in reachable_pairs(case)]
    check_counterexample(ref, fair, pr, node_of=lambda w: index[w], word_of=lambda v: words[v])
    if not pr.trace:
        return
    inits = {tlcgpu.host_init_state(m, i) for i in range(tlcgpu.init_count(m))}
    assert pr.trace[0] == ("Init", pr.trace[0][1]) and pr.trace[0][1] in inits
    for (_, s), (a, t) in zip(pr.trace, pr.trace[1:]):
        assert (a, t) in tlcgpu.host_successors(m, s)
    last = pr.trace[-1][1]
    if pr.loop_to >= 0:
        assert (pr.back_action, pr.trace[pr.loop_to][1]) in tlcgpu.host_successors(m, last)
    elif fair == "wf":  # <<Next>>_vars disabled at the end: every successor is a stutter
        assert all(t == last for _, t in tlcgpu.host_successors(m, last))


@pytest.mark.parametrize("fair", FAIR)
@pytest.mark.parametrize("prop", MODEL_PROPS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_property_matches_reference(case, prop, fair):
    ref, index = model_ref(case, prop)
    m = prop_model(case, prop)
    pr = tlcgpu.check_property(m, "Prop", fair)
    print(f"{case} {prop} {fair}: reachable {pr.reachable}, seeds {pr.seeds}, |G'| {pr.states_notp}, edges "
          f"{pr.edges_notp}, stuck {pr.stuck}, depth {pr.depth}, {pr.kind}; kernels {pr.kernel_ms:.2f} ms, classify "
          f"{pr.classify_ms:.3f} ms, call {pr.wall_ms:.1f} ms")
    assert pr.error is None
    assert counts_of(pr) == ref.counts(fair)
    assert pr.reachable == len(reachable_pairs(case))
    check_model_trace(case, m, ref, index, fair, pr)
    if ref.seeds:
        assert not pr.holds or fair == "wf"  # every case with seeds fails without fairness


def test_issue_table_is_what_the_reference_computes():
    """the figures the issue lists (weak fairness), recomputed: a guard on the
    reference and the fixtures, not on the device"""
    table = {("R_C1_K2", "A"): (28, 3, 13, 16, 1, 3), ("R_C1_K2", "D"): (28, 1, 19, 26, 1, 6),
             ("R_C2_K1", "A"): (37, 3, 11, 11, 0, 0), ("X_producer_sparse", "A"): (3608, 270, 1002, 1362, 0, 0),
             ("X_producer_sparse", "B"): (3608, 2904, 2904, 3000, 396, 1)}
    for (case, prop), want in table.items():
        r, _ = model_ref(case, prop)
        assert (r.reachable, len(r.seeds), r.states, r.edges, len(r.stuck_wf), r.stuck_min_level) == want


@pytest.mark.parametrize("case", ["S_consumer", "R_C1_K2", "W_C12_k1"])
def test_termination_as_a_user_property_equals_the_shipped_path(case):
    """<>(Termination's conjunction), written with the helpers' MaxLedger, through
    the reach + classify + seeded pass gives what tlcg_check_termination gives"""
    m = prop_model(case, "T")
    for fair in FAIR:
        lv = tlcgpu.check_termination(model_of(GOLDEN[case]["constants"]), fair)
        pr = tlcgpu.check_property(m, "Prop", fair)
        print(f"{case} {fair}: check_termination kernels {lv.kernel_ms:.2f} ms call {lv.wall_ms:.1f} ms; as a property "
              f"kernels {pr.kernel_ms:.2f} ms classify {pr.classify_ms:.3f} ms call {pr.wall_ms:.1f} ms")
        for f in ("holds", "states_notp", "init_notp", "edges_notp", "stuck", "depth", "peel_rounds", "on_cycles"):
            assert getattr(pr, f) == getattr(lv, f), (case, fair, f)
        assert pr.kind == lv.kind and len(pr.trace) == len(lv.trace) and pr.seed_at == (0 if pr.trace else -1)


@pytest.mark.parametrize("case,prop", [("S", "A"), ("S", "B"), ("W_C12_k1", "A"), ("W_C12_k1", "B")])
def test_property_regrows(case, prop):
    """from a 100-state store and a 256-slot FPSet the reach BFS is grown and
    redone; the counts equal the unforced run's"""
    m = prop_model(case, prop)
    for fair in FAIR:
        full = tlcgpu.check_property(m, "Prop", fair)
        small = tlcgpu.check_property(m, "Prop", fair, state_capacity=100, log2_fpset_slots=8)
        assert counts_of(small) == counts_of(full), (case, prop, fair)
        assert len(small.trace) == len(full.trace) and small.trace[-1:] == full.trace[-1:] or fair == "none"
        assert full.reachable > 100 and full.seeds > 0


def test_evaluation_error_is_reported_with_its_state():
    """P fails to evaluate in the initial state (compactedTopicContext = 0 is
    outside compactedLedgers' domain): an error naming the predicate with that
    state, not a verdict"""
    m = prop_model("R_C1_K2", "ERR")
    for fair in FAIR:
        pr = tlcgpu.check_property(m, "Prop", fair)
        assert pr.kind == "error" and not pr.holds
        assert pr.error_state == 0 and pr.reachable == 28
        assert "P (the left operand) of property Prop" in pr.error
        assert pr.trace == [("Init", tlcgpu.host_init_state(m, 0))]
        assert tlcgpu.host_property_eval(m, "Prop", [pr.trace[0][1]])[0] & 4


def test_refused_property_raises():
    m = prop_model("R_C1_K2", "A")
    m.user_defs["Prop"] = "<>[](cursor # Nil)"
    with pytest.raises(ValueError, match="property Prop cannot be checked: <>\\[\\]"):
        tlcgpu.check_property(m, "Prop")


# ---- explicit graphs: the only route to cycles ----

DENSITIES = (0.0, 0.1, 1.0)


def with_classes(g, density, seed):
    """Q = the graph's P, P drawn per node at `density`"""
    rng = random.Random(f"p/{seed}/{density}")
    return pgraph_of(g, [rng.random() < density for _ in g.is_p], g.is_p)


@functools.lru_cache(maxsize=None)
def graph_ref(key, density, form):
    g = HAND[key] if isinstance(key, str) else random_graph(*key)
    return PropertyReference(with_classes(g, density, str(key)), form)


def check_graph(monkeypatch, key, fair, regrow=False):
    """(as tests/test_gpu_liveness_graph.py: parents and the order inside a
    level are decided by races, so every run's trace is checked on its own)"""
    for density in DENSITIES:
        for form in FORMS:
            ref = graph_ref(key, density, form)
            g = ref.g
            want = ref.counts(fair)
            n = len(g.is_q)
            for words in (1, 2):
                for grid in (None, "1"):
                    if grid is None:
                        monkeypatch.delenv("TLCG_LV_GRID", raising=False)
                    else:
                        monkeypatch.setenv("TLCG_LV_GRID", grid)
                    runs = [dict()]
                    if grid is None:
                        runs.append(dict(state_capacity=n + 1, log2_fpset_slots=n.bit_length()))  # fewer than 2 n slots
                    if regrow:
                        runs.append(dict(state_capacity=100, log2_fpset_slots=8))
                    for kw in runs:
                        pr = tlcgpu.property_graph(g.row, g.col, g.is_p, g.is_q, g.n_init, form, words=words,
                                                   fairness=fair, **kw)
                        assert counts_of(pr) == want, (density, form, words, grid, kw)
                        check_counterexample(ref, fair, pr, words)
            if form == "eventually" and density == DENSITIES[0]:
                # <>Q from Init with every node in P: the shipped pass on the same graph, field by field
                ones = [1] * n
                pr = tlcgpu.property_graph(g.row, g.col, ones, g.is_q, g.n_init, form, fairness=fair)
                lv = tlcgpu.liveness_graph(g.row, g.col, g.is_q, g.n_init, fairness=fair)
                assert lv_counts_of(pr) == lv_counts_of(lv)
                assert len(pr.trace) == len(lv.trace) and pr.loop_to == lv.loop_to
                assert pr.seed_at == (0 if pr.trace else -1)


@pytest.mark.parametrize("fair", FAIR)
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_graph(monkeypatch, name, fair):
    check_graph(monkeypatch, name, fair)


@pytest.mark.parametrize("fair", FAIR)
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "n%d-%s-deg%d-s%d" % p)
def test_random_graph(monkeypatch, params, fair):
    check_graph(monkeypatch, params, fair, regrow=params[0] in STARRED)


def test_generated_set_reaches_cycles_from_seeds_off_init():
    """among the graphs above: one whose cycle is reachable only from a seed
    that is not initial (so only the seeded pass finds it), and one with a seed
    on the cycle itself"""
    only_from_late_seed = seed_on_cycle = 0
    for key in sorted(HAND) + list(PARAMS):
        for density in DENSITIES:
            for form in ("infinitely_often", "leads_to"):
                if form != "leads_to" and density != DENSITIES[0]:
                    continue
                ref = graph_ref(key, density, form)
                if not ref.left or ref.stuck_wf:
                    continue
                g = ref.g
                from_init = PropertyReference(g, "eventually")
                if not from_init.left:
                    only_from_late_seed += 1
                # a seed left after peeling with a path back to itself
                for s in ref.seeds & ref.left:
                    seen, todo = set(), [s]
                    while todo:
                        v = todo.pop()
                        for k in range(g.row[v], g.row[v + 1]):
                            t = g.col[k]
                            if t != v and t in ref.left and t not in seen:
                                seen.add(t)
                                todo.append(t)
                    if s in seen:
                        seed_on_cycle += 1
                        break
    assert only_from_late_seed > 0 and seed_on_cycle > 0, (only_from_late_seed, seed_on_cycle)
