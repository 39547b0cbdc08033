"""A plain reference of the seeded liveness pass (csrc/liveness.hip,
tlcg_check_property) over an explicit graph with a P and a Q byte per node,
and a checker of its counterexamples.  Pure Python, no GPU.

The graph is liveness_ref's CSR (moves, self-loops, repeated edges as there).
Only what the initial nodes reach is a state.  The seeds S are, by form,
  eventually         the initial nodes with ~Q
  infinitely_often   every reachable node with ~Q
  leads_to           every reachable node with P /\\ ~Q
and G' is what S reaches through ~Q nodes, S included.  Levels of G' count
from the seeds (a seed has level 1); everything else -- edges, stuck states,
Kahn rounds, what is left -- is liveness_ref.Reference's definition with S in
the place of the initial not-P nodes."""
from collections import namedtuple

from liveness_ref import moves, node_of_word

FORMS = ("eventually", "infinitely_often", "leads_to")

PGraph = namedtuple("PGraph", "row col is_p is_q n_init")


def pgraph_of(g, is_p, is_q):
    """a liveness_ref.Graph (its own is_p is not used) with class bytes"""
    assert len(is_p) == len(is_q) == len(g.row) - 1
    return PGraph(g.row, g.col, [int(bool(x)) for x in is_p], [int(bool(x)) for x in is_q], g.n_init)


class PropertyReference:
    """Everything tlcg_property reports, from the definitions."""

    def __init__(self, g, form):
        assert form in FORMS
        self.g, self.form = g, form
        # phase 1: BFS of the reachable nodes; reach_depth counts from 1
        self.reach_depth = {}
        self.reach_order = []
        frontier = list(range(g.n_init))
        d = 1
        for v in frontier:
            self.reach_depth[v] = 1
        while frontier:
            self.reach_order.extend(frontier)
            nxt = []
            d += 1
            for v in frontier:
                for _, t in moves(g, v):
                    if t not in self.reach_depth:
                        self.reach_depth[t] = d
                        nxt.append(t)
            frontier = nxt
        self.reachable = len(self.reach_depth)
        # seeds (reach_order is a BFS order: levels ascending)
        if form == "eventually":
            seeds = [v for v in range(g.n_init) if not g.is_q[v]]
        elif form == "infinitely_often":
            seeds = [v for v in self.reach_order if not g.is_q[v]]
        else:
            seeds = [v for v in self.reach_order if g.is_p[v] and not g.is_q[v]]
        self.seeds = set(seeds)
        self.min_seed_depth = min((self.reach_depth[v] for v in seeds), default=0)
        # G' by BFS from the seeds
        self.level = {v: 1 for v in seeds}
        self.levels = []
        frontier = list(seeds)
        while frontier:
            self.levels.append(frontier)
            nxt = []
            for v in frontier:
                for _, t in moves(g, v):
                    if not g.is_q[t] and t not in self.level:
                        self.level[t] = len(self.levels) + 1
                        nxt.append(t)
            frontier = nxt
        self.states = len(self.level)
        self.depth = len(self.levels)
        indeg = {v: 0 for v in self.level}
        self.edges = 0
        for v in self.level:
            for _, t in moves(g, v):
                if not g.is_q[t]:
                    indeg[t] += 1
                    self.edges += 1
        self.stuck_wf = sorted(v for v in self.level if not moves(g, v))
        self.peel_rounds = 0
        layer = [v for v in self.level if indeg[v] == 0]
        removed = 0
        while layer:
            self.peel_rounds += 1
            removed += len(layer)
            nxt = []
            for v in layer:
                for _, t in moves(g, v):
                    if not g.is_q[t]:
                        indeg[t] -= 1
                        if indeg[t] == 0:
                            nxt.append(t)
            layer = nxt
        self.left = {v for v in self.level if indeg[v] != 0}
        self.on_cycles = len(self.left)
        assert self.on_cycles == self.states - removed
        self.stuck_min_level = min((self.level[v] for v in self.stuck_wf), default=0)
        self.stuck_pick = min((v for v in self.stuck_wf if self.level[v] == self.stuck_min_level), default=None)

    def stuck(self, fair):
        return self.states if fair == "none" else len(self.stuck_wf)

    def kind(self, fair):
        if fair == "none":
            return "stuttering" if self.seeds else "holds"
        if self.stuck_wf:
            return "stuttering"
        return "cycle" if self.on_cycles else "holds"

    def counts(self, fair):
        """the fields of tlcg_property, in tlcgpu.Property's names"""
        return dict(holds=self.kind(fair) == "holds", kind=self.kind(fair), form=self.form, depth=self.depth,
                    states_notp=self.states, init_notp=len(self.seeds), edges_notp=self.edges, stuck=self.stuck(fair),
                    on_cycles=self.on_cycles, peel_rounds=self.peel_rounds, reachable=self.reachable,
                    seeds=len(self.seeds), error_state=-1)


def counts_of(pr):
    return dict(holds=pr.holds, kind=pr.kind, form=pr.form, depth=pr.depth, states_notp=pr.states_notp,
                init_notp=pr.init_notp, edges_notp=pr.edges_notp, stuck=pr.stuck, on_cycles=pr.on_cycles,
                peel_rounds=pr.peel_rounds, reachable=pr.reachable, seeds=pr.seeds, error_state=pr.error_state)


def check_counterexample(ref, fair, pr, words=1, node_of=None, word_of=None):
    """pr (a tlcgpu.Property) holds the counterexample the header documents for
    ref's graph.  node_of maps a trace state to its node (default: the graph
    entry's words) and word_of a node to its packed state (default: the node
    itself; the documented pick is the least packed state); actions are
    checked when they are edge ordinals."""
    g = ref.g
    kind = ref.kind(fair)
    assert pr.kind == kind and pr.fairness == fair and pr.form == ref.form
    if kind == "holds":
        assert pr.trace == [] and pr.loop_to == -1 and pr.seed_at == -1
        return
    assert pr.trace and pr.trace[0][0] == "Init"
    if node_of is None:
        def node_of(w):
            return node_of_word(w, words)
    nodes = [node_of(w) for _, w in pr.trace]
    assert nodes[0] < g.n_init
    # every step is a move of the graph, by the edge the action names
    for u, (k, _), v in zip(nodes, pr.trace[1:], nodes[1:]):
        assert u != v and v in [t for _, t in moves(g, u)], (u, v)
        if isinstance(k, int):
            assert 0 <= k < g.row[u + 1] - g.row[u] and g.col[g.row[u] + k] == v, (u, k, v)
    # the prefix is a shortest path from an initial node to a seed
    sa = pr.seed_at
    assert 0 <= sa < len(nodes)
    seed = nodes[sa]
    assert seed in ref.seeds
    assert sa + 1 == ref.reach_depth[seed]
    # from the seed on, never Q; each step one level of G' deeper at most, and
    # the path to the end (or the loop's entry) a shortest one inside G'
    assert not any(g.is_q[v] for v in nodes[sa:])
    assert all(v in ref.level for v in nodes[sa:])
    if kind == "stuttering":
        assert pr.loop_to == -1 and pr.back_action is None
        end = nodes[-1]
        if fair == "none":
            # the first seed in BFS order: a seed of the shallowest reach level, the trace ends there
            assert sa == len(nodes) - 1 and ref.reach_depth[end] == ref.min_seed_depth
        else:
            shallowest = [v for v in ref.stuck_wf if ref.level[v] == ref.stuck_min_level]
            assert end == (min(shallowest, key=word_of) if word_of else ref.stuck_pick)
        assert len(nodes) - sa == ref.level[end]
        return
    assert sa <= pr.loop_to < len(nodes)
    last, entry = nodes[-1], nodes[pr.loop_to]
    k = pr.back_action
    assert entry in [t for _, t in moves(g, last)]
    if isinstance(k, int):
        assert 0 <= k < g.row[last + 1] - g.row[last] and g.col[g.row[last] + k] == entry
    loop = nodes[pr.loop_to:]
    assert len(set(loop)) == len(loop) and len(loop) >= 2  # (a self-loop is no move)
    assert all(v in ref.left for v in loop)
    assert pr.loop_to - sa + 1 == ref.level[entry]
