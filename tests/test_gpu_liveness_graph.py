"""GPU: the liveness pass (csrc/liveness.hip) on explicit graphs, through
tlcg_liveness_graph_selftest, against the plain reference of
tests/liveness_ref.py.  The spec's own G' is acyclic for every cfg, so only
graphs the test supplies reach the cycle verdict, the copy-out of the states
left after peeling (k_lv_zero with left = 1, k_lv_gather), the lasso extraction and loop_to /
back_action, and only they tell an exact Kahn peeling (peel_rounds,
on_cycles, in-degrees with repeated edges) from one that merely ends empty.

Every field of tlcg_liveness is compared with the reference and the trace
with check_counterexample, under both fairness settings, with one- and
two-word states (eight nodes share a wide FPSet slot's high half), with the
default grid and with TLCG_LV_GRID=1 (one block takes every grid-stride
chunk: at n = 5000 twenty of them, reusing block_claim's LDS words); the
starred sizes also from a 100-state store and a 256-slot FPSet, where the
regrown run must equal the unforced one; every graph also with an FPSet of
fewer than 2 n slots."""
import functools

import pytest

import tlcgpu
from liveness_graph_cases import HAND, PARAMS, STARRED, random_graph
from liveness_ref import Reference, check_counterexample, counts_of

pytestmark = pytest.mark.gpu

FAIR = ("none", "wf")


@functools.lru_cache(maxsize=None)
def hand_ref(name):
    return Reference(HAND[name])


@functools.lru_cache(maxsize=None)
def random_ref(params):
    return Reference(random_graph(*params))


def check_graph(monkeypatch, ref, fair, regrow=False):
    """(Two runs need not return the same trace: which parent a state of G'
    gets, and the order of a level's states, are decided by races, so the path
    to the documented end state, and which of a level's states is the
    shallowest one left, may differ.  Every run's trace is checked on its own.)"""
    g = ref.g
    want = ref.counts(fair)
    slowest = (0.0, None)
    for words in (1, 2):
        for grid in (None, "1"):
            if grid is None:
                monkeypatch.delenv("TLCG_LV_GRID", raising=False)
            else:
                monkeypatch.setenv("TLCG_LV_GRID", grid)
            lv = tlcgpu.liveness_graph(g.row, g.col, g.is_p, g.n_init, words=words, fairness=fair)
            assert counts_of(lv) == want, (words, grid)
            check_counterexample(ref, fair, lv, words)
            slowest = max(slowest, (lv.wall_ms, (words, grid, "default", round(lv.kernel_ms, 2))))
            if grid is None:
                # a table of fewer than 2 n slots: long probe paths, so that nodes sharing a
                # high half meet in the wide FPSet (same high half, another low half: go on probing)
                n = len(g.is_p)
                tight = tlcgpu.liveness_graph(g.row, g.col, g.is_p, g.n_init, words=words, fairness=fair,
                                              state_capacity=n + 1, log2_fpset_slots=n.bit_length())
                assert counts_of(tight) == want, (words, "tight")
                check_counterexample(ref, fair, tight, words)
                slowest = max(slowest, (tight.wall_ms, (words, grid, "tight", round(tight.kernel_ms, 2))))
            if regrow:
                small = tlcgpu.liveness_graph(g.row, g.col, g.is_p, g.n_init, words=words, fairness=fair,
                                              state_capacity=100, log2_fpset_slots=8)
                assert counts_of(small) == counts_of(lv), (words, grid)
                check_counterexample(ref, fair, small, words)
                slowest = max(slowest, (small.wall_ms, (words, grid, "regrow", round(small.kernel_ms, 2))))
    print(f"slowest call {slowest[0]:.1f} ms: (words, grid, table, kernel ms) = {slowest[1]}")


@pytest.mark.parametrize("fair", FAIR)
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_graph(monkeypatch, name, fair):
    check_graph(monkeypatch, hand_ref(name), fair)


@pytest.mark.parametrize("fair", FAIR)
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "n%d-%s-deg%d-s%d" % p)
def test_random_graph(monkeypatch, params, fair):
    check_graph(monkeypatch, random_ref(params), fair, regrow=params[0] in STARRED)

