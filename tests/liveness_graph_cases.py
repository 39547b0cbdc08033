"""Explicit graphs for the liveness pass (tests/test_gpu_liveness_graph.py,
tests/test_liveness_ref.py): hand-made ones, a few nodes each, and a seeded
generator in three regimes."""
import random

from liveness_ref import graph_of


def _hand():
    c = {}
    # a 2-cycle
    c["two_cycle"] = graph_of([[1], [0]], [0, 0], 1)
    # a triangle 0 -> 1 -> 2 -> 0 with a DAG tail 2 -> 3 -> {4, 5}, 4 -> 5 -> 6(P) behind it
    c["triangle_tail"] = graph_of([[1], [2], [0, 3], [4, 5], [5], [6], []], [0, 0, 0, 0, 0, 0, 1], 1)
    # a cycle 2 <-> 3 reachable only through the P node 1: holds
    c["cycle_behind_p"] = graph_of([[1], [2], [3], [2]], [0, 1, 0, 0], 1)
    # a -> b(P) -> a: no cycle in G'
    c["cycle_through_p"] = graph_of([[1], [0]], [0, 1], 1)
    # a node whose only edge is a self-loop: stuck under WF
    c["self_loop_only"] = graph_of([[1], [1]], [0, 0], 1)
    # a double edge a => b, then a chain to P: b's in-degree is 2
    c["double_edge_chain"] = graph_of([[1, 1], [2], [3], [4], []], [0, 0, 0, 0, 1], 1)
    # a diamond into P
    c["diamond"] = graph_of([[1, 2], [3], [3], [4], []], [0, 0, 0, 0, 1], 1)
    # every initial node in P
    c["all_init_p"] = graph_of([[2], [2], [0]], [1, 1, 0], 2)
    # stuck states and a cycle together: 0 -> 1 <-> 2 -> 3 (no move)
    c["stuck_and_cycle"] = graph_of([[1], [2], [1, 3], []], [0, 0, 0, 0], 1)
    # a 300-node chain into P: 300 peel rounds
    c["chain300"] = graph_of([[v + 1] for v in range(300)] + [[]], [0] * 300 + [1], 1)
    return c


HAND = _hand()

REGIMES = ("dag", "cyclic", "mixed")
SIZES = (1, 63, 64, 65, 257, 5000)
STARRED = (257, 5000)  # also run from a store / FPSet far too small
MAX_DEGS = (4, 5, 8, 9)  # one, two and three batches of 4 moves, the last one partly filled
# (n, regime, largest out-degree, seed): two seeds of every small size
PARAMS = [(n, regime, deg, seed) for n in SIZES for regime in REGIMES for deg in MAX_DEGS
          for seed in ((0, 1) if n <= 65 else (0,))]


def random_graph(n, regime, max_deg, seed):
    """A seeded graph of n nodes whose largest out-degree is max_deg (node 0's),
    with a share of self-loops and repeated edges.
      dag     edges only to higher nodes.  max_deg 4 and 8: every not-P node
              has a move and the last node is in P, so the property holds;
              5 and 9: some nodes have no move.
      cyclic  edges anywhere; every node has a move into a not-P node, so no
              state is stuck and G' has a cycle (n = 1: the node is in P).
      mixed   edges anywhere, nodes without moves; max_deg 4: every initial
              node is in P."""
    rng = random.Random(f"{n}/{regime}/{max_deg}/{seed}")
    n_init = min(n, rng.choice([1, 2, 3]))
    p_prob = {"dag": 0.15, "cyclic": 0.1, "mixed": 0.2}[regime]
    is_p = [rng.random() < p_prob for _ in range(n)]
    for v in range(n_init):
        is_p[v] = regime == "mixed" and max_deg == 4
    clean_dag = regime == "dag" and max_deg in (4, 8)
    if regime == "dag":
        is_p[n - 1] = is_p[n - 1] or clean_dag
    if regime == "cyclic":
        if n == 1:
            is_p[0] = True
        else:
            is_p[1] = False  # a not-P node beside node 0
    not_p = [v for v in range(n) if not is_p[v]]

    def target(v):
        """a successor of v other than v, or None"""
        if regime == "dag":
            if v == n - 1:
                return None
            return rng.randint(v + 1, min(n - 1, v + 8)) if rng.random() < 0.5 else rng.randint(v + 1, n - 1)
        if n == 1:
            return None
        t = rng.randrange(n - 1)
        return t + (t >= v)

    adj = []
    for v in range(n):
        lonely = regime != "cyclic" and not clean_dag and v != 0 and rng.random() < 0.1
        deg = max_deg if v == 0 else rng.randint(0 if regime == "mixed" else 1, max_deg)
        out = []
        for _ in range(deg):
            r = rng.random()
            t = None
            if r < 0.1 or lonely:
                t = v
            elif r < 0.25 and out:
                t = rng.choice(out)
            else:
                t = target(v)
            out.append(v if t is None else t)
        if regime == "cyclic" and n > 1 and not any(t != v and not is_p[t] for t in out):
            out[rng.randrange(len(out))] = rng.choice([t for t in not_p if t != v])
        if clean_dag and v < n - 1 and all(t == v for t in out):
            out[rng.randrange(len(out))] = target(v)
        adj.append(out)
    return graph_of(adj, is_p, n_init)
