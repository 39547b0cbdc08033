"""CPU: the plain liveness reference (tests/liveness_ref.py) and the graphs the
GPU tests feed the pass (tests/liveness_graph_cases.py).  The reference is
pinned by hand-computed values on the hand-made graphs and by the oracles'
golden liveness results on small models (through model_graph); the generator
must yield every outcome often enough for the GPU comparison to mean something."""
import collections

import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from liveness_graph_cases import HAND, MAX_DEGS, PARAMS, REGIMES, SIZES, random_graph
from liveness_ref import Reference, model_graph

# name -> (states_notp, init_notp, edges_notp, stuck under WF, depth, peel_rounds, on_cycles, kind under WF)
HAND_WANT = {
    "two_cycle": (2, 1, 2, 0, 2, 0, 2, "cycle"),
    "triangle_tail": (6, 1, 7, 0, 5, 0, 6, "cycle"),
    "cycle_behind_p": (1, 1, 0, 0, 1, 1, 0, "holds"),
    "cycle_through_p": (1, 1, 0, 0, 1, 1, 0, "holds"),
    "self_loop_only": (2, 1, 1, 1, 2, 2, 0, "stuttering"),
    "double_edge_chain": (4, 1, 4, 0, 4, 4, 0, "holds"),
    "diamond": (4, 1, 4, 0, 3, 3, 0, "holds"),
    "all_init_p": (0, 0, 0, 0, 0, 0, 0, "holds"),
    "stuck_and_cycle": (4, 1, 4, 1, 4, 1, 3, "stuttering"),
    "chain300": (300, 1, 299, 0, 300, 300, 0, "holds"),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_on_hand_made_graphs(name):
    r = Reference(HAND[name])
    got = (r.states_notp, r.init_notp, r.edges_notp, r.stuck("wf"), r.depth, r.peel_rounds, r.on_cycles,
           r.kind("wf"))
    assert got == HAND_WANT[name]
    assert r.kind("none") == ("stuttering" if r.states_notp else "holds") and r.stuck("none") == r.states_notp


def test_hand_made_cases_are_the_listed_ones():
    assert sorted(HAND) == sorted(HAND_WANT)


def test_generator_covers_every_outcome():
    """over the whole parameter list each outcome under WF occurs at least 10
    times, every size, regime and degree is drawn, and the largest out-degree
    is the one asked for and belongs to a node the pass expands"""
    assert {p[0] for p in PARAMS} == set(SIZES) and {p[1] for p in PARAMS} == set(REGIMES)
    assert {p[2] for p in PARAMS} == set(MAX_DEGS)
    assert len(set(PARAMS)) == len(PARAMS)
    seen = collections.Counter()
    both = 0
    for n, regime, deg, seed in PARAMS:
        g = random_graph(n, regime, deg, seed)
        assert len(g.is_p) == n and g.row == random_graph(n, regime, deg, seed).row  # seeded
        assert max(g.row[v + 1] - g.row[v] for v in range(n)) == deg == g.row[1] - g.row[0]
        r = Reference(g)
        kind = r.kind("wf")
        seen[kind if kind != "holds" else ("holds_empty" if r.states_notp == 0 else "holds_nonempty")] += 1
        both += kind == "stuttering" and r.on_cycles > 0
        if regime == "cyclic" and n > 1:
            assert kind == "cycle"
        if regime == "dag":
            assert r.on_cycles == 0
    print(dict(seen), "stuck and cycle together:", both)
    assert set(seen) == {"holds_empty", "holds_nonempty", "stuttering", "cycle"}
    assert min(seen.values()) >= 10, seen
    assert both >= 10


@pytest.mark.parametrize("case", ["D_N0_K1_nodeadlock", "R_C1_K2", "X_empty_spaces", "X_producer_sparse"])
def test_reference_matches_the_oracles_on_models(case):
    """model_graph + the reference give the golden liveness figures of the C
    oracle's Tarjan restatement (cross-checked with the Python oracle's DFS)"""
    g, _ = model_graph(model_of(GOLDEN[case]["constants"]))
    r = Reference(g)
    for fair in ("none", "wf"):
        want = GOLDEN[case]["liveness"][fair]
        assert (r.kind(fair) == "holds", r.states_notp, r.init_notp, r.edges_notp, r.stuck(fair)) == \
               (want["holds"], want["states_notp"], want["init_notp"], want["edges_notp"], want["stuck"])
        assert (r.on_cycles == 0) == (want["cyclic_sccs"] == 0)
        shallowest = min(1, r.states_notp) if fair == "none" else r.stuck_min_depth
        assert shallowest == want["stuck_min_depth"]


def test_malformed_graphs_are_refused():
    """an edge out of the node range, a decreasing row, n_init > n, row[0] != 0:
    tlcg_liveness_graph_selftest refuses them before it touches a device"""
    for row, col, is_p, n_init in (([0, 1, 2], [1, 2], [0, 0], 1), ([0, 2, 1], [1], [0, 0], 1),
                                   ([0, 1, 2], [1, 0], [0, 0], 3), ([1, 1, 2], [1, 0], [0, 0], 1)):
        with pytest.raises(RuntimeError, match="graph:"):
            tlcgpu.liveness_graph(row, col, is_p, n_init)
