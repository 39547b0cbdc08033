"""CPU: state constraints (a cfg's CONSTRAINT section) up to the device's edge --
the cases' power on the reference alone, the host evaluator against the
reference's on every state, the refusals of the library and of tlc-hip."""
import subprocess

import pytest

import constraint_cases as CC
import tlcgpu as T
from conftest import CLI
from constraint_ref import ConstraintRef
from test_cli import numeric_cfg
from user_inv_cases import HELPERS


# ---- the cases, on the reference alone ----

@pytest.mark.parametrize("name", CC.DISCARDING)
def test_discarding_cases_have_power(name):
    r, u = CC.reference(name), CC.reference(name, constrained=False)
    assert r["result"] == "ok" and u["result"] == "ok"
    assert r["discarded"] > 0 and r["distinct"] > 0
    assert r["distinct"] < u["distinct"]
    assert (r["generated"], r["depth"], r["levels"]) != (u["generated"], u["depth"], u["levels"])


def test_error_cases_stop_where_the_constraint_cuts():
    ce = CC.reference("constraint_error")
    assert ce["result"] == "constraint_error" and ce["name"] == "CursorHorizon" and len(ce["trace"]) > 1
    assert ConstraintRef(CC.model_of("constraint_error")).verdict(ce["trace"][-1][1])[0] == 2
    for name, inv in (("leak_cut", "CompactedLedgerLeak"), ("user_cut", "ContextBelowTwo")):
        r = CC.reference(name)
        assert (r["result"], r["name"]) == ("invariant", inv)
        ref = ConstraintRef(CC.model_of(name))
        # the violating state is one the constraint discards; every state before it is in the model
        assert ref.verdict(r["trace"][-1][1])[0] == 1
        assert all(ref.verdict(s)[0] == 0 for _, s in r["trace"][:-1])
        assert r["trace"][-1][1] not in set(r["states"])
    # one kind of error on the level the search stops on: the order of the level does not decide the verdict
    for name in CC.ERROR_CASES:
        assert len(CC.reference(name)["level_errors"]) == 1


def test_special_cases():
    assert CC.reference("no_init")["distinct"] == 0 and CC.reference("no_init")["depth"] == 0
    assert CC.reference("no_init")["generated"] == T.init_count(CC.model_of("no_init"))
    r, u = CC.reference("discards_nothing"), CC.reference("discards_nothing", constrained=False)
    assert r["discarded"] == 0 and (r["generated"], r["levels"]) == (u["generated"], u["levels"])
    assert T.state_words(CC.model_of("wide")) == 2
    assert all(T.state_words(CC.model_of(n)) == 1 for n in CC.CASES if n != "wide")


def test_compaction_shapes_occur():
    """the level shapes the pass can go wrong on, by the reference's level sizes
    (raw: the new states of a level before the constraints, kept: after)"""
    shapes = set()
    for name in CC.CASES:
        r = CC.reference(name)
        kept = r["levels"] + [0] * (len(r["raw_levels"]) - len(r["levels"]))
        for i, (raw, k) in enumerate(zip(r["raw_levels"], kept)):
            if 0 < raw < 64:
                shapes.add("below a wave")
            if raw > 2 * 256 and 0 < k < raw:
                shapes.add("several blocks")
            if raw > 0 and k == 0:
                shapes.add("all discarded")
            if raw > 0 and k == raw:
                shapes.add("none discarded")
            if i == 0 and 0 < k < raw:
                shapes.add("level 0 filtered")
    assert shapes == {"below a wave", "several blocks", "all discarded", "none discarded", "level 0 filtered"}


# ---- the host evaluator against the reference's, state by state ----

@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_host_constraint_eval_equals_reference(name):
    m = CC.model_of(name)
    ref = ConstraintRef(m)
    ps = CC.pairs(name)
    got = T.host_constraint_eval(m, [w for w, _ in ps])
    want = [ref.verdict(o)[0] for _, o in ps]
    assert got == want
    if name == "constraint_error":
        assert 2 in got
    # a model without a constraint: every state is in the model
    assert set(T.host_constraint_eval(CC.model_of(name, constrained=False), [w for w, _ in ps[:50]])) == {0}


# ---- the library's refusals ----

def small(defs, cons, **kw):
    d = dict(HELPERS)
    d.update(defs)
    return T.Model(user_defs=d, constraints=cons, msg_sent_limit=2, **kw)


OK = small({"Ok": "crashTimes <= 1"}, ["Ok"])


def test_constraints_travel_in_user_defs():
    assert T.Model().user_defs_text() is None
    assert T.Model(user_defs={"A": "TRUE"}).user_defs_text() == "@@DEF A\nTRUE\n"
    assert OK.user_defs_text().endswith("@@DEF Ok\ncrashTimes <= 1\n@@CONSTRAINT Ok\n")
    assert T.check_model(OK) is None
    assert T.STATUS[6] == "constraint_error"


@pytest.mark.parametrize("defs,cons,parts", [
    ({"Bad": "crashTimes' = 0"}, ["Bad"], ["constraint Bad", "definition Bad", "primed variables", "line 14"]),
    ({"Bad": "/\\ crashTimes <= 1\n/\\ ENABLED Next"}, ["Bad"], ["constraint Bad", "definition Bad", "'ENABLED'",
                                                                   "line 15, col 4"]),
    ({"NotBool": "crashTimes + 1"}, ["NotBool"], ["constraint NotBool", "not a boolean"]),
    ({}, ["Nope"], ["constraint Nope is not defined"]),
    ({}, ["MaxId"], ["constraint MaxId takes arguments"]),
    ({"C%d" % i: "crashTimes <= %d" % i for i in range(9)}, ["C%d" % i for i in range(9)], ["more than 8"]),
])
def test_check_model_refuses_constraints_outside_the_subset(defs, cons, parts):
    err = T.check_model(small(defs, cons))
    assert err is not None
    for p in parts:
        assert p in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(engine="component"), "the on-chip engines (component, component tree) do not take it"),
    (dict(engine="tree"), "the on-chip engines (component, component tree) do not take it"),
    (dict(world=2), "a CONSTRAINT needs one rank"),
    (dict(spill=True), "not combined with the host spill"),
    (dict(fpset_spill=True), "not combined with the host FPSet tier"),
])
def test_create_refuses_combinations(kw, msg):
    with pytest.raises(RuntimeError, match="tlcg_create") as e:
        T.Checker(OK, **kw)
    assert msg in str(e.value)


def test_property_passes_refuse_a_constrained_model():
    for call, what in ((lambda: T.check_termination(OK), "PROPERTY Termination"),
                       (lambda: T.check_property(OK, "Ok"), "a temporal PROPERTY"),
                       (lambda: T.check_action_property(OK, "Ok"), "an action PROPERTY")):
        with pytest.raises((RuntimeError, ValueError)) as e:
            call()
        assert "the model has a CONSTRAINT: " + what + " is not checked under a state constraint" in str(e.value)


# ---- tlc-hip: the cfg section, in built-in-module mode (needs no .tla) ----

DEFS_TLA = ("CrashOnce == crashTimes <= 1\n"
            "HorizonOne ==\n    /\\ compactionHorizon <= 1\n"
            "Bounded(n) == crashTimes <= n\n"
            "Primed == crashTimes' = 0\n")


def cli(tmp_path, cfg_text, args=()):
    (tmp_path / "m.cfg").write_text(cfg_text)
    (tmp_path / "defs.tla").write_text(DEFS_TLA)
    p = subprocess.run([CLI, "-config", str(tmp_path / "m.cfg"), "-defs", str(tmp_path / "defs.tla")] + list(args),
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    return p.returncode, p.stdout + p.stderr


def constrained_cfg(section, **over):
    return numeric_cfg(**over) + "\n" + section + "\n"


@pytest.mark.parametrize("section", ["CONSTRAINT CrashOnce", "CONSTRAINTS\n    CrashOnce\n    HorizonOne",
                                     "CONSTRAINT CrashOnce, HorizonOne"])
def test_cli_parses_and_resolves_constraints(tmp_path, section):
    rc, out = cli(tmp_path, constrained_cfg(section, MaxCrashTimes="2"))
    assert "is not supported by this checker" not in out
    assert "Computing initial states..." in out
    # on a CPU-only host the run stops at device selection, never on a CPU fallback
    assert ("hipSetDevice" in out and rc == 255) or "distinct states found" in out


@pytest.mark.parametrize("section,over,expect,code", [
    ("CONSTRAINT NoSuchConstraint", {}, "The constraint NoSuchConstraint specified in the configuration file is not "
                                        "defined in the specification.", 151),
    ("CONSTRAINT Bounded", {}, "constraint Bounded takes arguments", 150),
    ("CONSTRAINT Primed", {}, "constraint Primed cannot be checked: definition Primed: primed variables", 150),
    ("CONSTRAINT CrashOnce", dict(PROPERTY="Termination"), "does not check a PROPERTY under a CONSTRAINT", 151),
    ("ACTION_CONSTRAINT CrashOnce", {}, "ACTION_CONSTRAINT is not supported by this checker", 151),
    ("ACTION_CONSTRAINTS CrashOnce", {}, "ACTION_CONSTRAINTS is not supported by this checker", 151),
    ("SYMMETRY CrashOnce", {}, "SYMMETRY is not supported by this checker", 151),
])
def test_cli_refusals(tmp_path, section, over, expect, code):
    rc, out = cli(tmp_path, constrained_cfg(section, **over))
    assert expect in out, out
    assert rc == code
    assert "Computing initial states" not in out


def test_cli_refuses_several_gpus(tmp_path):
    rc, out = cli(tmp_path, constrained_cfg("CONSTRAINT CrashOnce"), ["-gpus", "2"])
    assert "a cfg with a CONSTRAINT is checked on one GPU" in out and rc == 255
