"""Shared fixtures of the per-state tests of the user invariants' generated
code (user_inv.cpp user_device_source): the predicates, their split into
models of at most 8 invariants, the small configs whose reachable states they
are evaluated on, and the recorded outcomes of the Python oracle
(tests/golden/user_eval.json, written by tests/golden/make_golden_user_eval.py
from oracle/tla_eval.py alone)."""
import functools
import hashlib
import itertools
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from user_inv_cases import CASES, HELPERS, T, paired_states  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "user_eval.json")

# bodies written so that, with CASES, the compiled programs hold every opcode
# of user_inv.h among their needed instructions (tests/test_user_codegen_host.py
# checks the union): the cursor's fields, binary and unary minus, KeySpace / ValueSpace
# iterated and tested for membership, latestForKey under a KeySpace quantifier,
# and a division and a modulus whose divisor is 0 on many states (errors)
NEW_CASES = {
    "CursorHorizonLow": "cursor # Nil => cursor.compactionHorizon < Len(messages) \\/ cursor.compactedTopicContext > 1",
    "NegHorizon": "Len(messages) - compactionHorizon > 0 \\/ -crashTimes < 0",
    "EveryKeySent": "\\A k \\in KeySpace : \\E i \\in 1..Len(messages) : messages[i].key = k",
    "SomeValueUnsent": "\\E v \\in ValueSpace : \\A i \\in 1..Len(messages) : messages[i].value # v",
    "SpaceMembership": "\\A i \\in 1..Len(messages) :\n"
                       "   messages[i].key \\in KeySpace \\/ messages[i].value \\in ValueSpace",
    "DivByContext": "Len(messages) \\div compactedTopicContext <= MessageSentLimit",
    "ModByCrash": "compactionHorizon % crashTimes = 0",
    "LatestKnown": "phaseOneResult # Nil =>\n"
                   "  \\A k \\in KeySpace : k \\in DOMAIN phaseOneResult.latestForKey =>\n"
                   "    phaseOneResult.latestForKey[k] <= phaseOneResult.readPosition",
}


def _eval_cases():
    from bench import USER_DEFS
    out = dict(CASES)
    # the six bench invariants (bench.USER_DEFS less its helper definitions)
    for name, body in USER_DEFS.items():
        if name in ("NullKey", "KeySet", "ValueSet"):
            continue
        assert out.setdefault(name, body) == body, name  # (the same text as the fixture of that name)
    assert not set(NEW_CASES) & set(out)
    out.update(NEW_CASES)
    return out


EVAL_CASES = _eval_cases()

# models of at most 8 invariants (tlcg_model.invariants).  The first group
# opens with invariants that raise an evaluation error or fail on most states,
# followed by others: the per-invariant outcomes past the first failing one
GROUPS = [
    ["ContextLedgerError", "DivByContext", "EveryKeySent", "LedgerCount", "KeysKnown", "LatestIsLast", "ArithCase",
     "CursorHorizonLow"],
    ["PhaseKnown", "ModByCrash", "LedgerSorted", "MessageRec", "HeadFirst", "NegHorizon", "SomeValueUnsent",
     "MaxLedgerBound"],
    ["ContextBound", "CursorAfterContext", "LetChoose", "NoDoubleCrashWrite", "RecordEq", "SetMapKeys",
     "SpaceMembership", "LatestKnown"],
]
assert sorted(n for g in GROUPS for n in g) == sorted(EVAL_CASES) and all(len(g) <= 8 for g in GROUPS)

# name -> (constants, the first initial states whose components are taken
# (None: all), stride over the states in BFS order); small on purpose
CONFIGS = {
    "N2C2": (dict(msg_sent_limit=2, compaction_times_limit=2), None, 1),
    # non-contiguous keys: the select chains of the generated KeySet tables
    "N2C3K2_k59": (dict(msg_sent_limit=2, max_crash_times=2, key_space=(5, 9), value_space=(7,)), None, 1),
    "N2C3_noretain": (dict(msg_sent_limit=2, retain_null_key=False, value_space=(1,)), None, 1),
    "consumer": (dict(msg_sent_limit=2, compaction_times_limit=2, key_space=(1,), value_space=(1,),
                      model_consumer=True, consume_times_limit=2), None, 1),
    "P_N3C2": (dict(model_producer=True, compaction_times_limit=2, key_space=(1,), value_space=(1,)), None, 4),
    # a two-word layout (u128 states): every 5th state of the components of the first 32 initial states
    "wide": (dict(compaction_times_limit=12, key_space=(1, 2, 3), value_space=(1, 2, 3)), 32, 5),
}
ONE_WORD_CLOSED = ["N2C2", "N2C3K2_k59", "N2C3_noretain", "consumer"]  # the on-chip engines take these
SMALLEST = ["consumer", "N2C3_noretain"]


def base_model(cfg):
    return T.Model(**CONFIGS[cfg][0])


def group_model(cfg, names):
    defs = dict(HELPERS)
    defs.update({n: EVAL_CASES[n] for n in names})
    return T.Model(invariants=tuple(names), user_defs=defs, **CONFIGS[cfg][0])


@functools.lru_cache(maxsize=None)
def config_pairs(cfg):
    """(packed word, oracle state) of the config's states, in BFS order"""
    kw, n_inits, stride = CONFIGS[cfg]
    return tuple(paired_states(T.Model(**kw), n_inits=n_inits)[::stride])


def config_words(cfg):
    return [w for w, _ in config_pairs(cfg)]


def words_hash(words, state_words):
    h = hashlib.sha256()
    for w in words:
        h.update(int(w).to_bytes(8 * state_words, "little"))
    return h.hexdigest()


RLE_DOC = ("outcomes: runs <count><T|F|E> and repeated groups of runs <count>(<runs>), a count of 1 left out; "
           "T, F, E = EV_TRUE 0, EV_FALSE 1, EV_ERROR 2")


def rle(digits):
    """a string of 0/1/2 in the fixture's stored form: runs, "0001222" ->
    "3TF3E", and a group of up to 8 runs that repeats folded, "TFFTFFTFF" ->
    "3(T2F)" (the states of the components interleave in BFS order, so most
    strings are periodic); greedy from the left, so the form is unique"""
    t = [(str(n) if n > 1 else "") + "TFE"[int(d)]
         for d, n in ((d, len(list(run))) for d, run in itertools.groupby(digits))]
    out, i = [], 0
    while i < len(t):
        p, r = 1, 1  # the period and repeat count that save the most runs
        for q in range(1, 9):
            k = 1
            while t[i + k * q:i + (k + 1) * q] == t[i:i + q]:
                k += 1
            if (k - 1) * q > (r - 1) * p:
                p, r = q, k
        if (r - 1) * len("".join(t[i:i + p])) > 4:
            out.append(f"{r}({''.join(t[i:i + p])})")
            i += p * r
        else:
            out.append(t[i])
            i += 1
    return "".join(out)


def unrle(stored):
    assert re.fullmatch(r"(\d*[TFE]|\d+\((\d*[TFE])+\))*", stored), stored[:40]

    def runs(s):
        return "".join(str("TFE".index(c)) * int(n or 1) for n, c in re.findall(r"(\d*)([TFE])", s))
    return "".join(runs(g) * int(n) if g else runs(n + c)
                   for n, g, c in re.findall(r"(\d*)(?:\(([^()]*)\)|([TFE]))", stored))


@functools.lru_cache(maxsize=None)
def golden():
    """the fixture, its outcome strings expanded to one EV_* digit per state"""
    g = json.load(open(GOLDEN))
    assert g["encoding"] == RLE_DOC
    for e in g["configs"].values():
        e["outcomes"] = {n: unrle(s) for n, s in e["outcomes"].items()}
    return g


def golden_outcomes(cfg, name):
    """the oracle's EV_* digit per state of cfg ("0" TRUE, "1" FALSE, "2" error)"""
    return golden()["configs"][cfg]["outcomes"][name]


def checked_words(cfg):
    """the config's packed states, which must be the ones the fixture was recorded on"""
    words = config_words(cfg)
    g = golden()["configs"][cfg]
    sw = T.state_words(base_model(cfg))
    assert g["states"] == len(words) and g["hash"] == words_hash(words, sw), cfg
    return words


def write_input(path, model, words):
    """the input file of tests/fuzz/user_codegen_run.cpp"""
    sw = T.state_words(model)
    text = model.user_defs_text().encode()
    head = (f"model {model.msg_sent_limit} {model.compaction_times_limit} {model.consume_times_limit} "
            f"{model.max_crash_times} {int(model.model_consumer)} {int(model.model_producer)} "
            f"{int(model.retain_null_key)} {int(model.check_deadlock)}\n"
            f"keys {len(model.key_space)} {' '.join(map(str, model.key_space))}\n"
            f"values {len(model.value_space)} {' '.join(map(str, model.value_space))}\n"
            f"invariants {len(model.invariants)} {' '.join(model.invariants)}\n"
            f"defs {len(text)}\n").encode()
    lines = [" ".join(f"{(w >> (64 * k)) & 0xFFFFFFFFFFFFFFFF:x}" for k in range(sw)) for w in words]
    with open(path, "wb") as f:
        f.write(head + text + f"\nstates {len(words)} {sw}\n".encode() + "\n".join(lines).encode() + b"\n")
