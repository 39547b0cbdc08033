"""Shared fixtures of the user-defined temporal property tests
(tests/test_property_host.py, tests/test_gpu_property.py): the properties,
models that carry them, and the graph of a model's reachable states with the
Python oracle's value of P and Q on every node."""
import functools

import tlcgpu
from conftest import GOLDEN, model_of
from liveness_ref import graph_of
from property_ref import pgraph_of
from user_inv_cases import HELPERS, paired_states

# name -> (form, P text or None, Q text, the property as the user writes it)
_E_P = "\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil"
PROPS = {
    "A": ("leads_to", "compactorState = Compactor_In_PhaseTwoUpdateContext", "cursor # Nil",
          "compactorState = Compactor_In_PhaseTwoUpdateContext ~> cursor # Nil"),
    "B": ("infinitely_often", None, "compactorState = Compactor_In_PhaseOne",
          "[]<>(compactorState = Compactor_In_PhaseOne)"),
    "C": ("leads_to", "crashTimes = MaxCrashTimes /\\ crashTimes > 0", "compactorState = Compactor_In_PhaseTwoWrite",
          "(crashTimes = MaxCrashTimes /\\ crashTimes > 0) ~> compactorState = Compactor_In_PhaseTwoWrite"),
    "D": ("eventually", None, "cursor # Nil", "<>(cursor # Nil)"),
    "E": ("leads_to", _E_P, "compactionHorizon > 0", "(" + _E_P + ") ~> compactionHorizon > 0"),
    "E_box": ("leads_to", _E_P, "compactionHorizon > 0", "[]((" + _E_P + ") => <>(compactionHorizon > 0))"),
    # Termination's conjunction (the guard of Terminating) with the helpers' MaxLedger
    "T": ("eventually", None,
          "Len(messages) = MessageSentLimit /\\ compactorState = Compactor_In_PhaseTwoWrite\n"
          "   /\\ MaxLedger = CompactionTimesLimit /\\ (ModelConsumer => consumeTimes = ConsumeTimesLimit)", None),
    # an evaluation error in the initial state: compactedTopicContext = 0 is outside the ledgers' domain
    "ERR": ("leads_to", "Len(compactedLedgers[compactedTopicContext]) >= 0", "cursor # Nil",
            "Len(compactedLedgers[compactedTopicContext]) >= 0 ~> cursor # Nil"),
}
PROPS["T"] = PROPS["T"][:3] + ("<>(" + PROPS["T"][2] + ")",)


def prop_model(case, prop):
    """the golden case's model with the property as definition Prop, and its
    operands as definitions P_ / Q_ for the oracle (which evaluates state
    predicates only and never reads Prop)"""
    form, p, q, text = PROPS[prop]
    m = model_of(GOLDEN[case]["constants"])
    defs = dict(HELPERS)
    defs["P_"] = p if p is not None else "TRUE"
    defs["Q_"] = q
    defs["Prop"] = text
    m.user_defs = defs
    return m


@functools.lru_cache(maxsize=None)
def reachable_pairs(case, limit=None):
    """(packed word, oracle state) of the case's reachable states in BFS order"""
    return paired_states(model_of(GOLDEN[case]["constants"]), limit)


def oracle_classes(case, prop, limit=None):
    """bit 0 P, bit 1 Q, bit 2 evaluation error, per reachable state, by oracle_py's inv()"""
    import oracle_py
    from user_inv_cases import oracle_model
    om = oracle_model(prop_model(case, prop))
    out = []
    for _, o in reachable_pairs(case, limit):
        c = 0
        for bit, name in ((1, "P_"), (2, "Q_")):
            try:
                c |= bit if om.inv(name, o) else 0
            except oracle_py.EvalError:
                c |= 4
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def state_graph(case):
    """the case's whole reachable graph as a liveness_ref.Graph over the nodes
    of reachable_pairs (every successor an edge, stuttering ones self-loops),
    and word -> node"""
    pairs = reachable_pairs(case)
    m = model_of(GOLDEN[case]["constants"])
    index = {w: i for i, (w, _) in enumerate(pairs)}
    adj = [[index[t] for _, t in tlcgpu.host_successors(m, w)] for w, _ in pairs]
    return graph_of(adj, [0] * len(pairs), tlcgpu.init_count(m)), index


@functools.lru_cache(maxsize=None)
def model_pgraph(case, prop):
    g, index = state_graph(case)
    cls = oracle_classes(case, prop)
    assert not any(c & 4 for c in cls), "P or Q fails to evaluate on a reachable state"
    return pgraph_of(g, [c & 1 for c in cls], [c >> 1 & 1 for c in cls]), index
