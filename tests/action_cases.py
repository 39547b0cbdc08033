"""Shared fixtures of the action property tests
(tests/test_action_property_host.py, tests/test_gpu_action_property.py): the
properties [][A]_v, the models that carry them, every step of a model's
reachable graph, and the reference's verdict on each (tests/action_ref.py)."""
import functools

import tlcgpu
from action_ref import ActionRef, model_steps, summary
from conftest import GOLDEN, model_of
from user_inv_cases import HELPERS, paired_states

# name -> (A, subscript)
ACTIONS = {
    "CrashUp": ("crashTimes' >= crashTimes /\\ crashTimes' <= crashTimes + 1", "vars"),
    "HorizonUp": ("compactionHorizon' >= compactionHorizon", "vars"),
    "ContextUp": ("compactedTopicContext' >= compactedTopicContext", "compactorVars"),
    "AppendOnly": ("Len(messages') >= Len(messages) /\\ \\A i \\in 1..Len(messages) : messages'[i] = messages[i]",
                   "messages"),
    "DeleteInDelete": ("(\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil /\\ compactedLedgers'[i] = Nil)"
                       " => compactorState = Compactor_In_PhaseTwoDeleteLedger", "vars"),
    "CursorPersist": ("cursor' # cursor => compactorState' = Compactor_In_PhaseTwoDeleteLedger", "vars"),
    "SamePhaseKeeps": ("compactorState' = compactorState => UNCHANGED <<compactedLedgers, cursor>>", "vars"),
    "CrashKeepsBookie": ("crashTimes' # crashTimes => UNCHANGED bookieVars /\\ phaseOneResult' = Nil", "vars"),
    "ReadPosKept": ("phaseOneResult = Nil \\/ phaseOneResult' = Nil \\/ "
                    "phaseOneResult'.readPosition = phaseOneResult.readPosition", "vars"),
    "CursorNeverBack": ("cursor # Nil => cursor' # Nil /\\ cursor'.compactionHorizon >= cursor.compactionHorizon",
                        "cursor"),
    "LedgerGrows": ("Cardinality({i \\in 1..CompactionTimesLimit : compactedLedgers'[i] # Nil}) >= "
                    "Cardinality({i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil})", "compactedLedgers"),
    "ErrNext": ("Len(compactedLedgers'[compactedTopicContext']) >= 0", "vars"),
}
# the tuple definitions a property's text may name (the CLI takes them from the module)
TUPLE_DEFS = {"bookieVars": "<<messages, compactedLedgers, cursor>>"}

MODELS = ("R_C1_K2", "R_C2_K1", "X_producer_sparse", "WIDE1", "S")
# states, steps, then per property "violating steps @ level of the shallowest
# violating step's source" (ErrNext: erroring steps, the first at level 1);
# the other eight properties hold with no erroring step
EXPECTED = {
    "R_C1_K2": (28, 41, {"HorizonUp": (2, 5), "ContextUp": (4, 4), "ErrNext": (20, 1)}),
    "R_C2_K1": (37, 47, {"HorizonUp": (1, 5), "ContextUp": (4, 4), "LedgerGrows": (2, 9), "ErrNext": (11, 1)}),
    "X_producer_sparse": (3608, 5695, {"HorizonUp": (114, 6), "ContextUp": (384, 5), "LedgerGrows": (228, 10),
                                       "ErrNext": (1123, 1)}),
    "WIDE1": (557, 617, {"HorizonUp": (1, 5), "ContextUp": (24, 4), "LedgerGrows": (77, 9), "ErrNext": (11, 1)}),
    "S": (45198, 56133, {"HorizonUp": (729, 5), "ContextUp": (4374, 4), "LedgerGrows": (3645, 9),
                         "ErrNext": (8019, 1)}),
}


def base_model(case):
    if case == "WIDE1":  # a 69-bit state, two words, one initial state
        return tlcgpu.Model(msg_sent_limit=3, compaction_times_limit=12, max_crash_times=1, key_space=(),
                            value_space=(), retain_null_key=True, model_producer=False, model_consumer=False)
    return model_of(GOLDEN[case]["constants"])


def prop_text(prop):
    a, sub = ACTIONS[prop]
    return f"[][{a}]_{sub}"


def action_model(case, prop=None, body=None, **extra):
    """the case's model with the property (or `body`) as definition Prop"""
    m = base_model(case)
    defs = dict(HELPERS)
    defs.update(TUPLE_DEFS)
    defs.update(extra)
    defs["Prop"] = body if body is not None else prop_text(prop)
    m.user_defs = defs
    return m


@functools.lru_cache(maxsize=None)
def pairs_of(case, limit=None):
    return paired_states(base_model(case), limit)


@functools.lru_cache(maxsize=None)
def steps_of(case, limit=None):
    """every step of the case's graph (of its first `limit` states' steps), and the level of every state"""
    return model_steps(base_model(case), pairs_of(case, limit))


@functools.lru_cache(maxsize=None)
def ref_verdicts(case, prop, limit=None):
    """the reference's TRUE / FALSE / ERROR (0 / 1 / 2) on every step of steps_of(case, limit)"""
    a, sub = ACTIONS[prop]
    ref = ActionRef(base_model(case), a, sub, defs=dict(HELPERS))
    return [ref.verdict(o, u) for _, _, o, u, _, _ in steps_of(case, limit)[0]]


@functools.lru_cache(maxsize=None)
def ref_summary(case, prop):
    return summary(ref_verdicts(case, prop), steps_of(case)[0])
