"""A plain reference of the liveness pass (csrc/liveness.hip) over an explicit
graph, and a checker of its counterexamples.  Pure Python, no GPU.

The graph is CSR: node v's moves are the edges row[v] .. row[v + 1] - 1 of
col, move k being edge row[v] + k; nodes 0 .. n_init - 1 are initial; is_p[v]
says that v satisfies P.  A self-loop is a stuttering step, never a move; a
repeated edge counts every time.  G' is what the initial not-P nodes reach
through not-P nodes.  BFS depths count from 1 (an initial node has depth 1),
as the oracle's stuck_min_depth does, so a BFS path of depth d has d states."""
from collections import namedtuple

Graph = namedtuple("Graph", "row col is_p n_init")


def graph_of(adj, is_p, n_init):
    """CSR of adjacency lists (adj[v]: v's successors in move order)"""
    row, col = [0], []
    for out in adj:
        col.extend(out)
        row.append(len(col))
    assert len(is_p) == len(adj) and n_init <= len(adj)
    return Graph(row, col, [int(bool(x)) for x in is_p], n_init)


def moves(g, v):
    """(ordinal, successor) of every move of v: its edges but the self-loops"""
    return [(k, g.col[g.row[v] + k]) for k in range(g.row[v + 1] - g.row[v]) if g.col[g.row[v] + k] != v]


class Reference:
    """Everything tlcg_liveness reports, from the definitions."""

    def __init__(self, g):
        self.g = g
        # G' by BFS, with its levels
        self.level = {}
        frontier = [v for v in range(g.n_init) if not g.is_p[v]]
        self.first_init = frontier[0] if frontier else None
        self.init_notp = len(frontier)
        self.levels = []
        for v in frontier:
            self.level[v] = 1
        while frontier:
            self.levels.append(frontier)
            nxt = []
            for v in frontier:
                for _, t in moves(g, v):
                    if not g.is_p[t] and t not in self.level:
                        self.level[t] = len(self.levels) + 1
                        nxt.append(t)
            frontier = nxt
        self.states_notp = len(self.level)
        self.depth = len(self.levels)
        # every edge into G' (from G'), self-loops excluded, and the in-degrees
        indeg = {v: 0 for v in self.level}
        self.edges_notp = 0
        for v in self.level:
            for _, t in moves(g, v):
                if not g.is_p[t]:
                    indeg[t] += 1
                    self.edges_notp += 1
        # where <<Next>>_vars is disabled: no move at all (a move into P is one)
        self.stuck_wf = sorted(v for v in self.level if not moves(g, v))
        # Kahn layers
        self.peel_rounds = 0
        layer = [v for v in self.level if indeg[v] == 0]
        removed = 0
        while layer:
            self.peel_rounds += 1
            removed += len(layer)
            nxt = []
            for v in layer:
                for _, t in moves(g, v):
                    if not g.is_p[t]:
                        indeg[t] -= 1
                        if indeg[t] == 0:
                            nxt.append(t)
            layer = nxt
        self.left = {v for v in self.level if indeg[v] != 0}
        self.on_cycles = len(self.left)
        assert self.on_cycles == self.states_notp - removed
        # the shallowest stuck level and the least word in it
        self.stuck_min_depth = min((self.level[v] for v in self.stuck_wf), default=0)
        self.stuck_pick = min((v for v in self.stuck_wf if self.level[v] == self.stuck_min_depth), default=None)

    def stuck(self, fair):
        return self.states_notp if fair == "none" else len(self.stuck_wf)

    def kind(self, fair):
        if fair == "none":
            return "stuttering" if self.states_notp else "holds"
        if self.stuck_wf:
            return "stuttering"
        return "cycle" if self.on_cycles else "holds"

    def counts(self, fair):
        """the fields of tlcg_liveness, in Liveness' names"""
        return dict(holds=self.kind(fair) == "holds", kind=self.kind(fair), depth=self.depth,
                    states_notp=self.states_notp, init_notp=self.init_notp, edges_notp=self.edges_notp,
                    stuck=self.stuck(fair), on_cycles=self.on_cycles, peel_rounds=self.peel_rounds)


def counts_of(lv):
    return dict(holds=lv.holds, kind=lv.kind, depth=lv.depth, states_notp=lv.states_notp, init_notp=lv.init_notp,
                edges_notp=lv.edges_notp, stuck=lv.stuck, on_cycles=lv.on_cycles, peel_rounds=lv.peel_rounds)


def node_of_word(word, words):
    """node v's state is the word v, or the two words {v, v >> 3}"""
    v = word & 0xFFFFFFFFFFFFFFFF
    assert word >> 64 == (v >> 3 if words == 2 else 0), hex(word)
    return v


def check_counterexample(ref, fair, lv, words=1):
    """lv (a tlcgpu.Liveness of the graph entry: actions are edge ordinals) is
    the counterexample the header documents for ref's graph"""
    g = ref.g
    kind = ref.kind(fair)
    assert lv.kind == kind and lv.fairness == fair
    if kind == "holds":
        assert lv.trace == [] and lv.loop_to == -1
        return
    assert lv.trace and lv.trace[0][0] == "Init"
    nodes = [node_of_word(w, words) for _, w in lv.trace]
    assert nodes[0] < g.n_init
    assert not any(g.is_p[v] for v in nodes)
    for (_, _), u, (k, _), v in zip(lv.trace, nodes, lv.trace[1:], nodes[1:]):
        assert isinstance(k, int) and 0 <= k < g.row[u + 1] - g.row[u] and g.col[g.row[u] + k] == v, (u, k, v)
    if kind == "stuttering":
        assert lv.loop_to == -1 and lv.back_action is None
        want = ref.first_init if fair == "none" else ref.stuck_pick
        assert nodes[-1] == want and len(nodes) == ref.level[want]
        return
    assert 0 <= lv.loop_to < len(nodes)
    last, entry = nodes[-1], nodes[lv.loop_to]
    k = lv.back_action
    assert isinstance(k, int) and 0 <= k < g.row[last + 1] - g.row[last] and g.col[g.row[last] + k] == entry
    loop = nodes[lv.loop_to:]
    assert len(set(loop)) == len(loop)
    assert lv.loop_to + 1 == ref.level[entry]
    assert len(loop) >= 2  # (a self-loop is no move)


def model_graph(m):
    """The part of model m's state graph the liveness pass sees, as a Graph and
    the packed states of its nodes: the initial states in Init order, then the
    states reached through not-P states; every successor of a not-P state is an
    edge (stuttering ones are self-loops); a P state is a leaf."""
    import tlcgpu
    states = [tlcgpu.host_init_state(m, i) for i in range(tlcgpu.init_count(m))]
    n_init = len(states)
    index = {s: i for i, s in enumerate(states)}
    assert len(index) == n_init
    adj, is_p = [], []
    v = 0
    while v < len(states):
        succ = tlcgpu.host_successors(m, states[v])
        p = any(a == "Terminating" for a, _ in succ)  # P is Terminating's guard
        is_p.append(p)
        out = []
        if not p:
            for _, t in succ:
                if t not in index:
                    index[t] = len(states)
                    states.append(t)
                out.append(index[t])
        adj.append(out)
        v += 1
    return graph_of(adj, is_p, n_init), states
