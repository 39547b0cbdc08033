"""The cases of the constraint tests (a cfg's CONSTRAINT section): small
constants, a state predicate or two as the constraint, and what the case is
there to show.  The reference (constraint_ref.ConstraintRef) runs once per case
and is shared by the tests of a session."""
import functools

import tlcgpu as T
from constraint_ref import ConstraintRef
from user_inv_cases import HELPERS, paired_states

LIVE = "{i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil}"

DEFS = {
    "CrashOnce": "crashTimes <= 1",
    "HorizonOne": "compactionHorizon <= 1",
    "FirstKeyed": "messages[1].key # NullKey",
    "NoMessages": "Len(messages) = 0",
    "CrashAny": "crashTimes <= MaxCrashTimes",
    "OneMessage": "Len(messages) <= 1",
    "CursorHorizon": "compactedTopicContext >= 1 => cursor.compactionHorizon <= MessageSentLimit",
    "TwoLedgers": "Cardinality(" + LIVE + ") <= 2",
    "ContextOne": "compactedTopicContext <= 1",
    "ContextTwo": "compactedTopicContext <= 2",
    "ContextBelowTwo": "compactedTopicContext < 2",
}

SMALL = dict(msg_sent_limit=2, compaction_times_limit=3, max_crash_times=2)
LEAK = ("TypeSafe", "CompactedLedgerLeak", "CompactionHorizonCorrectness")

# name -> (Model keywords, constraints, user invariants, discards some but not all reachable states)
CASES = {
    "crash_once": (dict(SMALL), ["CrashOnce"], [], True),
    "horizon_one": (dict(SMALL), ["HorizonOne"], [], True),
    # reads `messages`; level 0 (729 states, three blocks) is filtered across blocks
    "first_keyed": (dict(msg_sent_limit=3, compaction_times_limit=2, max_crash_times=1), ["FirstKeyed"], [], True),
    "no_init": (dict(SMALL), ["NoMessages"], [], False),
    "discards_nothing": (dict(SMALL), ["CrashAny"], [], False),
    "two_constraints": (dict(SMALL), ["CrashOnce", "HorizonOne"], [], True),
    "producer_len": (dict(SMALL, model_producer=True), ["OneMessage"], [], True),
    # a 2-word state (u128 path)
    "wide": (dict(msg_sent_limit=2, compaction_times_limit=12, max_crash_times=1), ["ContextTwo"], [], True),
    # cursor = Nil where the context is already set: the constraint fails to evaluate there
    "constraint_error": (dict(SMALL), ["CursorHorizon"], [], False),
    # the third ledger exists only in states the constraint discards: still reported
    "leak_cut": (dict(SMALL, invariants=LEAK), ["TwoLedgers"], [], False),
    # the same with a user invariant, the definition being invariant and constraint
    "user_cut": (dict(SMALL, invariants=("TypeSafe", "ContextBelowTwo")), ["ContextOne"], ["ContextBelowTwo"], False),
}
DISCARDING = sorted(k for k, v in CASES.items() if v[3])
ERROR_CASES = ("constraint_error", "leak_cut", "user_cut")


def model_of(name, constrained=True):
    kw, cons, uinv, _ = CASES[name]
    kw = dict(kw)
    kw.setdefault("invariants", ("TypeSafe", "CompactionHorizonCorrectness"))
    defs = dict(HELPERS)
    defs.update({n: DEFS[n] for n in list(cons) + list(uinv)})
    return T.Model(user_defs=defs, constraints=list(cons) if constrained else None, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, constrained=True):
    """the reference run of a case (never modified by a test)"""
    return ConstraintRef(model_of(name, constrained)).run()


@functools.lru_cache(maxsize=None)
def pairs(name):
    """(packed word, oracle state) of the case's unconstrained graph"""
    return paired_states(model_of(name, constrained=False))


@functools.lru_cache(maxsize=None)
def word_of(name):
    return {o: w for w, o in pairs(name)}
