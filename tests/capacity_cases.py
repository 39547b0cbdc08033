"""The cfgs that sit on the capacity and depth rungs of the on-chip engines,
as data, and the engine each must end in by the documented admission rules.

Component engine (csrc/component.h, run_component): capacity passes of 64,
128 and 255 states (32 first under TLCG_COMP_K0=32), COMP_MAXLV = 48 levels,
16-bit code records when the code fits 16 bits, the per-lane bitmap pass for
components of <= 62 states with an 8-entry FIFO ring.  Closed tree
(csrc/tree.h, run_tree): 640-slot chunks, then 2048, codes of <= 31 bits.
Producer tree: 384-slot chunks, then 1024.  Past the last rung the global
engine takes the model.

Every number here comes from the CPU (oracle/tlc_oracle.c and the host model);
tests/test_capacity_edges.py pins them, so a GPU test over these cfgs proves
that a rung was crossed from these sizes and the engine the run ended in
(expected_engine), never from what a kernel reports."""
from collections import namedtuple

import tlcgpu

# ---- closed cfgs: MessageSentLimit = 1, KeySpace = 1..8, ValueSpace = 1..7,
# RetainNullKey TRUE, no Producer: 9 x 8 = 72 isomorphic components (one full
# batch of 64 lanes and a batch of 8)

ClosedRow = namedtuple("ClosedRow", "C K size depth width code_bits key_fits edge")

CLOSED_ROWS = [
    ClosedRow(5, 0, 32, 32, 1, 18, True, "exactly 32: fills TLCG_COMP_K0=32"),
    ClosedRow(1, 5, 58, 12, 9, 13, True, "<= 62 states, queue 9 > the 8-entry lane ring"),
    ClosedRow(2, 2, 62, 14, 8, 15, True, "62 states, queue = ring"),
    ClosedRow(1, 6, 68, 13, 10, 13, True, "first past 64"),
    ClosedRow(2, 4, 112, 14, 14, 16, True, "code_bits = 16 edge, overflows the 64 code pass"),
    ClosedRow(5, 1, 130, 32, 7, 19, True, "just past 128"),
    ClosedRow(2, 5, 137, 15, 18, 16, True, "just past 128, on code records"),
    ClosedRow(3, 4, 225, 20, 26, 17, True, "largest under 255, wide queue"),
    ClosedRow(7, 1, 222, 44, 9, 21, True, "under 255, deepest under 48 levels"),
    ClosedRow(7, 0, 44, 44, 1, 20, True, "depth 44"),
    ClosedRow(8, 0, 50, 50, 1, 23, True, "tiny but depth 50: overflows on depth alone"),
    ClosedRow(8, 1, 277, 50, 10, 24, True, "past 255 and past 48 levels"),
    ClosedRow(3, 5, 280, 21, 31, 17, True, "just past 255"),
    ClosedRow(7, 2, 637, 44, 36, 22, True, "637 of 640 slots"),
    ClosedRow(13, 1, 642, 80, 15, 29, False, "just past 640"),
    ClosedRow(4, 6, 651, 28, 58, 20, True, "just past 640, shallow and wide"),
    ClosedRow(15, 1, 830, 92, 17, 31, False, "code_bits = 31 edge"),
    ClosedRow(8, 3, 1970, 50, 123, 25, False, "largest under 2048"),
    ClosedRow(7, 4, 2168, 44, 148, 23, True, "past 2048 -> global"),
    ClosedRow(15, 2, 4417, 92, 136, 32, False, "code_bits 32 -> global"),
    ClosedRow(16, 0, 98, 98, 1, 33, False, "code_bits 33 -> global, though tiny"),
]

CLOSED_KEYS, CLOSED_VALUES = tuple(range(1, 9)), tuple(range(1, 8))
CLOSED_COMPONENTS = 72

# (C, K) -> the depth at which the oracle reports the added invariant
LEAK_ROWS = {(5, 1): 12, (3, 4): 9, (7, 1): 12, (7, 2): 9, (4, 6): 9, (13, 1): 12, (8, 3): 9, (3, 5): 9}
LEAK_HOLDS = [(8, 0)]  # CompactedLedgerLeak added, and the check passes
DUP_DEPTH = 4          # DuplicateNullKeyMessage on each of LEAK_ROWS and LEAK_HOLDS

# world sizes: (KeySpace, ValueSpace) -> components = (|KeySpace| + 1) (|ValueSpace| + 1)
WORLDS = {
    64: (tuple(range(1, 8)), tuple(range(1, 8))),   # exactly one batch
    65: (tuple(range(1, 5)), tuple(range(1, 13))),  # a one-lane last batch
    1: ((), ()),
}

# each rung of the closed ladder with the (C, K) rows next to it on either side
# (the spec reaches no component of exactly 64, 128, 255, 640 or 2048 states)
CLOSED_RUNGS = {
    "32 states": ([(5, 0)], [(7, 0), (1, 5)]),
    "64 states": ([(2, 2), (1, 5)], [(1, 6)]),
    "128 states": ([(2, 4)], [(5, 1), (2, 5)]),
    "255 states": ([(3, 4), (7, 1)], [(3, 5), (8, 1)]),
    "48 levels": ([(7, 0), (7, 1)], [(8, 0), (8, 1)]),
    "640 slots": ([(7, 2)], [(13, 1), (4, 6)]),
    "2048 slots": ([(8, 3)], [(7, 4)]),
    "16 code bits": ([(2, 4), (2, 5)], [(3, 4), (3, 5)]),
    "31 code bits": ([(15, 1)], [(15, 2), (16, 0)]),
}

# ---- Producer cfgs: KeySpace = {1}, ValueSpace = {1}, RetainNullKey FALSE;
# the largest components are in the last layer (min, max over that layer)

ProducerRow = namedtuple("ProducerRow", "N C K last_min last_max edge")

PRODUCER_ROWS = [
    ProducerRow(3, 3, 1, 267, 359, "fits 384"),
    ProducerRow(3, 4, 1, 423, 599, "384 -> 1024"),
    ProducerRow(3, 3, 2, 489, 748, "384 -> 1024"),
    ProducerRow(2, 4, 2, 485, 649, "384 -> 1024"),
    ProducerRow(2, 4, 3, 766, 1083, "straddles 1024 -> global"),
    ProducerRow(3, 3, 3, 715, 1162, "straddles 1024 -> global"),
]

PRODUCER_RUNGS = {
    "384 slots": ([(3, 3, 1)], [(3, 4, 1), (3, 3, 2), (2, 4, 2)]),
    "1024 slots": ([(3, 4, 1), (3, 3, 2), (2, 4, 2)], [(2, 4, 3), (3, 3, 3)]),
}

BASE_INVARIANTS = ("TypeSafe", "CompactionHorizonCorrectness")


def closed_model(C, K, extra_invariant=None, keys=CLOSED_KEYS, values=CLOSED_VALUES):
    inv = BASE_INVARIANTS + ((extra_invariant,) if extra_invariant else ())
    return tlcgpu.Model(msg_sent_limit=1, compaction_times_limit=C, max_crash_times=K, key_space=keys,
                        value_space=values, retain_null_key=True, model_producer=False, invariants=inv)


def producer_model(N, C, K, extra_invariant=None):
    inv = BASE_INVARIANTS + ((extra_invariant,) if extra_invariant else ())
    return tlcgpu.Model(msg_sent_limit=N, compaction_times_limit=C, max_crash_times=K, key_space=(1,),
                        value_space=(1,), retain_null_key=False, model_producer=True, invariants=inv)


def closed_row(C, K):
    return next(r for r in CLOSED_ROWS if (r.C, r.K) == (C, K))


def producer_row(N, C, K):
    return next(r for r in PRODUCER_ROWS if (r.N, r.C, r.K) == (N, C, K))


def constants_of(m):
    """a model as the golden fixtures' constants (what test_gpu_parity's rules read)"""
    return dict(N=m.msg_sent_limit, C=m.compaction_times_limit, K=m.max_crash_times, ctl=m.consume_times_limit,
                consumer=bool(m.model_consumer), producer=bool(m.model_producer), retain=bool(m.retain_null_key),
                keys=list(m.key_space), values=list(m.value_space), invariants=list(m.invariants),
                deadlock=bool(m.check_deadlock))


def closure_levels(m, s0):
    """BFS levels of the states the host model reaches from s0"""
    seen, levels = {s0}, [[s0]]
    while True:
        nxt = []
        for s in levels[-1]:
            for _, t in tlcgpu.host_successors(m, s):
                if t not in seen:
                    seen.add(t)
                    nxt.append(t)
        if not nxt:
            return levels
        levels.append(nxt)


def producer_layers(m):
    """Producer modelled: the reachable states grouped by `messages` (a
    component each; the low bits of the state word: the length, then the
    messages, csrc/model.h) -> per layer (the length) the component sizes"""
    n = m.msg_sent_limit
    lb = n.bit_length()
    mb = lb + n * (len(m.key_space).bit_length() + len(m.value_space).bit_length())
    sizes = {}
    for lvl in closure_levels(m, tlcgpu.host_init_state(m, 0)):
        for s in lvl:
            key = s & ((1 << mb) - 1)
            sizes[key] = sizes.get(key, 0) + 1
    layers = [[] for _ in range(n + 1)]
    for key, k in sizes.items():
        layers[key & ((1 << lb) - 1)].append(k)
    return layers


def expected_engine(model, per_component, depth):
    """The engine a passing check of `model` ends in, by the documented
    admission rules: per_component the states of its largest component, depth
    TLC's depth of the whole search.  Nothing of the run is read."""
    from test_gpu_parity import code_bits, component_key_fits
    from test_gpu_tree import tree_applies
    c = constants_of(model)
    if model.model_producer:
        return "tree" if tree_applies(model) and per_component <= 1024 else "global"
    if per_component <= 255 and depth <= 47 and component_key_fits(c):
        return "component"
    if code_bits(c) <= 31 and per_component <= 2048 and depth <= 126:
        return "tree"
    return "global"
