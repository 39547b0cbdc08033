"""CPU: the temporal front end (user_inv.cpp compile_property, through
tlcg_host_property_form / tlcg_host_property_eval): the form of every accepted
spelling, every refusal by its message, P and Q against the Python oracle's
inv() on the reachable states of golden cases, and the front end under
AddressSanitizer and UBSan in a stand-alone program
(tests/fuzz/property_fuzz.cpp; nothing loaded into Python is sanitized)."""
import json
import os
import shutil
import subprocess

import pytest

import tlcgpu
from property_cases import PROPS, oracle_classes, prop_model, reachable_pairs
from user_inv_cases import HELPERS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pulsar-tlaplus_amd", "csrc")


def model_with(body, **extra):
    defs = dict(HELPERS)
    defs["Done"] = "compactorState = Compactor_In_PhaseTwoWrite /\\ crashTimes = MaxCrashTimes"
    defs.update(extra)
    defs["Prop"] = body
    return tlcgpu.Model(user_defs=defs)


SPELLINGS = [
    ("<>(cursor # Nil)", "eventually"),
    ("<>Done", "eventually"),
    ("((<>(cursor # Nil)))", "eventually"),
    ("<>(/\\ cursor # Nil\n   /\\ compactionHorizon > 0)", "eventually"),
    ("[]<>(compactorState = Compactor_In_PhaseOne)", "infinitely_often"),
    ("[]<>Done", "infinitely_often"),
    ("([]<>(Done))", "infinitely_often"),
    ("cursor = Nil ~> cursor # Nil", "leads_to"),
    ("(crashTimes > 0) ~> (Done)", "leads_to"),
    ("crashTimes > 0 /\\ cursor = Nil ~> Done \\/ cursor # Nil", "leads_to"),
    ("[]((crashTimes > 0) => <>(Done))", "leads_to"),
    ("[](crashTimes > 0 => <>Done)", "leads_to"),
    ("[](crashTimes > 0 => (<>(Done)))", "leads_to"),
    ("(\\E i \\in 1..CompactionTimesLimit : compactedLedgers[i] # Nil) ~> compactionHorizon > 0", "leads_to"),
    ("CASE crashTimes = 0 -> TRUE [] OTHER -> FALSE ~> Done", None),  # (an unparenthesised CASE: refused below)
]


@pytest.mark.parametrize("body,form", [s for s in SPELLINGS if s[1]])
def test_accepted_spellings(body, form):
    assert tlcgpu.host_property_form(model_with(body), "Prop") == form


@pytest.mark.parametrize("prop", ["A", "B", "C", "D", "E", "E_box", "T"])
def test_issue_predicates_are_accepted(prop):
    assert tlcgpu.host_property_form(prop_model("S", prop), "Prop") == PROPS[prop][0]


REFUSALS = [
    # <>[]Q
    ("<>[](cursor # Nil)", ["<>[]", "line 1, col 1"]),
    ("[](crashTimes > 0 => <>[]Done)", ["<>[]"]),
    # conjunctions (and other combinations) of temporal formulas
    ("<>(cursor # Nil) /\\ <>(Done)", ["combines temporal formulas", "line 1, col 21"]),
    ("(<>Done) /\\ (<>Done)", ["combines temporal formulas"]),
    ("[]<>Done /\\ []<>(cursor # Nil)", ["combines temporal formulas"]),
    ("~<>Done", ["combines temporal formulas"]),
    ("(cursor = Nil ~> Done) /\\ (cursor # Nil ~> Done)", ["combines temporal formulas"]),
    ("cursor = Nil ~> Done ~> cursor # Nil", ["a second ~>"]),
    ("cursor = Nil ~> <>Done", ["a temporal operator (<>) inside an operand"]),
    ("<>(cursor = Nil ~> Done)", ["a temporal operator (~>) inside an operand"]),
    ("[](cursor # Nil)", ["[] applied to something other than"]),
    ("[]Done", ["[] applied to something other than"]),
    ("[](Done => Done)", ["[](P => F) where F is not <>Q"]),
    # a <> whose operand is neither parenthesised nor a bare name running to the end
    ("<>cursor # Nil", ["neither parenthesised nor a bare name", "line 1, col 3"]),
    ("<>~Done", ["neither parenthesised nor a bare name"]),
    ("<>(cursor # Nil) \\/ Done", ["neither parenthesised nor a bare name"]),
    ("[]<>Done /\\ crashTimes = 0", ["neither parenthesised nor a bare name"]),
    # a top-level => or <=> beside ~>
    ("crashTimes > 0 => cursor = Nil ~> Done", ["a top-level => beside ~>", "line 1, col 16"]),
    ("cursor = Nil ~> Done <=> Done", ["a top-level <=> beside ~>"]),
    ("cursor = Nil ~> Done => Done", ["a top-level => beside ~>"]),
    # a bulleted list containing a temporal operator
    ("/\\ <>Done\n/\\ <>(cursor # Nil)", ["a bulleted list containing a temporal operator (<>)", "line 1, col 4"]),
    ("\\/ cursor = Nil ~> Done\n\\/ Done", ["a bulleted list containing a temporal operator (~>)"]),
    # primes, ENABLED, fairness operators
    ("<>(cursor' # Nil)", ["a primed variable (')"]),
    ("cursor = Nil ~> cursor' # Nil", ["a primed variable (')"]),
    ("<>(ENABLED Done)", ["ENABLED"]),
    ("[]<>Done /\\ WF_vars(Next)", ["a fairness operator (WF_)"]),
    ("SF_vars(Next) => <>Done", ["a fairness operator (SF_)"]),
    # an unparenthesised quantifier or CASE would take the ~> into its body
    ("\\E i \\in 1..2 : compactedLedgers[i] # Nil ~> Done", ["an unparenthesised \\E left of the temporal operator"]),
    ("CASE crashTimes = 0 -> TRUE [] OTHER -> FALSE ~> Done", ["an unparenthesised CASE"]),
    # operands outside the predicate subset, or not boolean
    ("<>(compactionHorizon + 1)", ["the operand of property Prop is a integer, not a boolean"]),
    ("crashTimes ~> Done", ["the left operand of property Prop is a integer"]),
    ("<>(\\A s \\in SUBSET KeySpace : Cardinality(s) <= 2)", ["SUBSET", "line 1"]),
    ("<>NoSuchName", ["NoSuchName"]),
]
# (a numeral past 64 bits ends in a message too, though one without a line)
TOO_LONG = "<>(crashTimes = 99999999999999999999999999)"


@pytest.mark.parametrize("body,parts", REFUSALS, ids=[r[0].replace("\n", " ")[:40] for r in REFUSALS])
def test_refusals_name_definition_line_and_construct(body, parts):
    m = model_with(body)
    with pytest.raises(ValueError) as e:
        tlcgpu.host_property_form(m, "Prop")
    msg = str(e.value)
    assert msg.startswith("property Prop cannot be checked: "), msg
    assert "line " in msg, msg
    # (a definition handed over without a "@line" is placed by its line in the
    # definitions' text: "line 1" above is the body's first line)
    text = m.user_defs_text()
    first = text[:text.index("@@DEF Prop\n")].count("\n") + 2
    for p in parts:
        assert p.replace("line 1", f"line {first}") in msg, msg


def test_numeral_past_64_bits_is_refused():
    with pytest.raises(ValueError, match="property Prop cannot be checked"):
        tlcgpu.host_property_form(model_with(TOO_LONG), "Prop")


def test_lines_are_the_definitions():
    """a refusal on the third line of a definition that starts at line 40 of its
    module (the "@line" header token, as tlc-hip passes it)"""
    defs = "@@DEF Prop @40\n  (crashTimes > 0\n    /\\ cursor = Nil)\n  ~> <>(cursor # Nil)\n"
    c = tlcgpu.Model().to_c()
    c.user_defs = defs.encode()
    import ctypes as C
    form = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = tlcgpu.load_library().tlcg_host_property_form(C.byref(c), b"Prop", C.byref(form), err, len(err))
    assert rc == -1
    assert "property Prop cannot be checked" in err.value.decode() and "at line 42, col 6" in err.value.decode()


def test_state_predicate_and_missing_definition_have_their_own_codes():
    import ctypes as C
    lib = tlcgpu.load_library()
    m = model_with("cursor # Nil")
    c = m.to_c()
    form = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    assert lib.tlcg_host_property_form(C.byref(c), b"Prop", C.byref(form), err, len(err)) == -2
    assert "is a state predicate, not a temporal formula" in err.value.decode()
    assert lib.tlcg_host_property_form(C.byref(c), b"Absent", C.byref(form), err, len(err)) == -3
    assert "property Absent is not defined" in err.value.decode()
    with pytest.raises(ValueError):
        tlcgpu.host_property_form(model_with("<>Q(1)", **{"Q(x)": "crashTimes = x"}), "Q")  # takes arguments


EVAL_CASES = [("R_C1_K2", None), ("R_C2_K1", None), ("S", 3000), ("W_C12_k1", 1500)]


@pytest.mark.parametrize("prop", ["A", "B", "C", "D", "E", "E_box", "T", "ERR"])
@pytest.mark.parametrize("case,limit", EVAL_CASES, ids=[c for c, _ in EVAL_CASES])
def test_host_eval_matches_oracle(case, limit, prop):
    """bit 0 P, bit 1 Q, bit 2 error of tlcg_host_property_eval equal oracle_py's
    inv() of the operands on every reachable state (the first `limit` in BFS order)"""
    m = prop_model(case, prop)
    pairs = reachable_pairs(case, limit)
    assert tlcgpu.state_words(m) == (2 if case.startswith("W_") else 1)
    got = tlcgpu.host_property_eval(m, "Prop", [w for w, _ in pairs])
    want = oracle_classes(case, prop, limit)
    assert got == want
    if PROPS[prop][1] is None:
        assert all(c & 1 for c in got)  # the forms without a P: TRUE
    if prop == "ERR":
        assert got[0] & 4  # the initial state: compactedTopicContext = 0
    else:
        assert not any(c & 4 for c in got)
        if limit is None:  # (the whole graph: Q neither constant nor unreachable)
            assert any(c & 2 for c in got) and not all(c & 2 for c in got)


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("propfuzz") / "property_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(HERE, "fuzz", "property_fuzz.cpp"), os.path.join(CSRC, "host_model.cpp"),
           os.path.join(CSRC, "user_inv.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_front_end_under_sanitizers(fuzz_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "150", str(seed)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["unmutated_ok"] == res["spellings"] > 0  # every accepted spelling, as written
    assert res["accepted"] > res["spellings"] and res["refused"] > 0 and res["not_temporal"] > 0
    assert res["eventually"] and res["infinitely_often"] and res["leads_to"] and res["evals"] > 0
