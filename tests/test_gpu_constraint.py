"""GPU: state constraints (a cfg's CONSTRAINT section) on the global engine,
against the plain-Python reference (constraint_ref.py): verdict, counts, level
sizes, the kept states, TLC-order store order and trace, fast-order trace
properties, the constraint-error status, grow-and-redo, checkpoint / recover,
unconstrained runs, and tlc-hip end to end.  Runs under an environment setting
(TLCG_JIT) happen in a fresh child process (constraint_run.py)."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import constraint_cases as CC
import oracle_py
import tlcgpu as T
from conftest import CLI, GOLDEN, model_of
from constraint_ref import ConstraintRef
from test_cli import numeric_cfg

pytestmark = pytest.mark.gpu

ALL = sorted(CC.CASES)
# (TLCG_JIT=1 also builds the layout's whole specialized module for a one-word state: one such case)
JIT_CASES = {"0": ["constraint_error", "crash_once", "user_cut", "wide"], "1": ["crash_once", "wide"]}
REDO = "engine=global,log2_fpset_slots=8"
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "constraint_run.py")


@functools.lru_cache(maxsize=None)
def child(jit):
    """every run of one environment setting, in one fresh process"""
    cases = ALL if jit is None else JIT_CASES[jit]
    specs = [f"{n}:{t}" for n in cases for t in (0, 1)]
    if jit is None:
        specs += [f"crash_once:{t}:{REDO}" for t in (0, 1)]
    env = dict(os.environ)
    env.pop("TLCG_JIT", None)
    if jit is not None:
        env["TLCG_JIT"] = jit
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.json")
        p = subprocess.run([sys.executable, RUNNER, path] + specs, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout + p.stderr
        with open(path) as f:
            return json.load(f)


def check(name, tlc, got):
    """one run against the reference"""
    want = CC.reference(name)
    word = CC.word_of(name)
    state_of = dict(CC.pairs(name))
    ref = ConstraintRef(CC.model_of(name))
    print(name, "tlc" if tlc else "fast", {k: got[k] for k in ("status", "generated", "distinct", "depth", "levels",
                                                               "discarded", "pass_ms", "levels_redone", "jit_used")})
    assert got["engine"] == "global"
    assert got["status"] == want["result"]
    assert (got["invariant"] if want["result"] != "constraint_error" else got["constraint"]) == want["name"]
    assert (got["generated"], got["distinct"], got["depth"]) == (want["generated"], want["distinct"], want["depth"])
    assert got["levels"] == want["levels"]
    kept = [word[o] for o in want["states"]]
    assert sorted(got["states"]) == sorted(kept)
    assert (got["discarded"] > 0) == (want["discarded"] > 0)
    assert not got["tlc_exact"]
    trace = [(a, s) for a, s in got["trace"]]
    if tlc:
        # the stored order of every level is the reference's queue order; the trace is its trace
        assert got["states"] == kept
        assert trace == [(a, word[o]) for a, o in want["trace"]]
        return
    assert len(trace) == len(want["trace"])
    if not trace:
        return
    m = CC.model_of(name)
    assert trace[0][0] == "Init" and trace[0][1] in {T.host_init_state(m, i) for i in range(T.init_count(m))}
    for (_, s), (a, t) in zip(trace, trace[1:]):
        assert (a, t) in T.host_successors(m, s)
    assert all(ref.verdict(state_of[s])[0] == 0 for _, s in trace[:-1])
    last = state_of[trace[-1][1]]
    if want["result"] == "constraint_error":
        assert ref.verdict(last) == (2, want["name"])
    else:
        assert want["result"] == "invariant" and ref.om.inv(want["name"], last) is False


@pytest.mark.parametrize("tlc", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_constrained_run_equals_reference(name, tlc):
    got = child(None)[f"{name}:{tlc}"]
    check(name, tlc, got)
    assert got["levels_redone"] == 0
    assert got["jit_used"] & 4  # the pass's kernel 1 is the generated device code


@pytest.mark.parametrize("tlc", [0, 1])
@pytest.mark.parametrize("jit,name", [(j, n) for j in ("0", "1") for n in JIT_CASES[j]])
def test_interpreter_and_generated_code(jit, name, tlc):
    """TLCG_JIT=0: the precompiled k_constraint_eval interprets the program; 1: hipRTC device code"""
    got = child(jit)[f"{name}:{tlc}"]
    check(name, tlc, got)
    assert bool(got["jit_used"] & 4) == (jit == "1")


def test_constraint_error_status():
    for tlc in (0, 1):
        got = child(None)[f"constraint_error:{tlc}"]
        assert got["status"] == "constraint_error" and got["constraint"] == "CursorHorizon"
        assert T.STATUS[6] == "constraint_error"
        last = dict(CC.pairs("constraint_error"))[got["trace"][-1][1]]
        assert ConstraintRef(CC.model_of("constraint_error")).verdict(last)[0] == 2


@pytest.mark.parametrize("tlc", [0, 1])
def test_grow_and_redo_gives_identical_counts(tlc):
    """a 256-slot FPSet of fixed first size: levels overflow it and are redone after a rebuild from
    the filtered store, which no longer holds the discarded states; they are found and discarded again"""
    got = child(None)[f"crash_once:{tlc}:{REDO}"]
    assert got["levels_redone"] > 0
    check("crash_once", tlc, got)


@pytest.mark.parametrize("tlc", [False, True])
def test_checkpoint_and_recover(tmp_path, tlc):
    name = "crash_once"
    m = CC.model_of(name)
    path = str(tmp_path / "c.ckpt")
    a = T.Checker(m, tlc_order=tlc)
    try:
        st = a.init()
        for _ in range(6):
            st = a.step_level()
        assert st.status == 0
        a.checkpoint(path)
        before = (st.generated, st.distinct, st.depth)
    finally:
        a.close()
    b = T.Checker(m, tlc_order=tlc)
    try:
        st = b.recover(path)
        assert (st.generated, st.distinct, st.depth) == before
        while st.status == 0:
            st = b.step_level()
        r = b.result()
        got = dict(status=r.status, invariant=r.invariant, constraint=r.constraint, generated=r.generated,
                   distinct=r.distinct, depth=r.depth, levels=r.levels, engine=r.engine, jit_used=r.jit_used,
                   levels_redone=r.levels_redone, tlc_exact=r.tlc_exact, trace=[], states=b.copy_states(0, r.distinct),
                   discarded=b.constraint_stats()[0], pass_ms=b.constraint_stats()[1])
    finally:
        b.close()
    check(name, tlc, got)
    # the checkpoint's identity holds the constraint: another one does not resume it
    for other in (CC.model_of("horizon_one"), CC.model_of(name, constrained=False)):
        c = T.Checker(other, tlc_order=tlc, engine="global")
        try:
            with pytest.raises(RuntimeError, match="other constants or options"):
                c.recover(path)
        finally:
            c.close()


def test_unconstrained_runs_are_untouched():
    want = GOLDEN["S"]["result"]
    m = model_of(GOLDEN["S"]["constants"])
    assert m.constraints is None and m.user_defs_text() is None
    for engine in ("global", "auto"):
        ck = T.Checker(m, engine=engine)
        try:
            r = ck.run()
            assert (r.status, r.generated, r.distinct, r.depth, r.levels) == (
                "ok", want["generated"], want["distinct"], want["depth"], want["levels"])
            assert (r.engine == "global") == (engine == "global")  # auto still picks the on-chip engine
            assert ck.constraint_stats() == (0, 0.0, [])
        finally:
            ck.close()


# ---- tlc-hip, built-in-module mode with the definitions added by -defs ----

DEFS_TLA = "".join(f"{k} == {v}\n" for k, v in CC.DEFS.items() if k in ("CrashOnce", "CursorHorizon", "TwoLedgers"))
SMALL_CFG = dict(MessageSentLimit="2", CompactionTimesLimit="3", MaxCrashTimes="2")


def cli(tmp_path, constraint, **over):
    (tmp_path / "m.cfg").write_text(numeric_cfg(**dict(SMALL_CFG, **over)) + "\nCONSTRAINT " + constraint + "\n")
    (tmp_path / "defs.tla").write_text(DEFS_TLA)
    p = subprocess.run([CLI, "-config", str(tmp_path / "m.cfg"), "-defs", str(tmp_path / "defs.tla")],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    return p.returncode, p.stdout


@pytest.mark.parametrize("name,constraint,over,code,message", [
    ("crash_once", "CrashOnce", {}, 0, "Model checking completed. No error has been found."),
    ("leak_cut", "TwoLedgers", dict(INVARIANTS=", ".join(CC.LEAK)), 12, "Error: Invariant CompactedLedgerLeak is violated."),
    ("constraint_error", "CursorHorizon", {}, 75, "Error: Evaluating constraint CursorHorizon failed."),
])
def test_cli_constrained_cfg(tmp_path, name, constraint, over, code, message):
    want = CC.reference(name)
    rc, out = cli(tmp_path, constraint, **over)
    print(out)
    lines = out.splitlines()
    assert rc == code
    assert message in lines
    assert any(l.startswith(f"{want['generated']} states generated, {want['distinct']} distinct states found, ")
               for l in lines)
    assert f"The depth of the complete state graph search is {want['depth']}." in lines
    if code:
        assert "Error: The behavior up to this point is:" in lines
        assert sum(l.startswith("State ") for l in lines) == len(want["trace"])
        assert lines[lines.index("Error: The behavior up to this point is:") + 1] == "State 1: <Initial predicate>"
        # (the trace ends in the reference's last state: the discarded / erroring one)
        assert all(r in lines for r in oracle_py.Model.render(want["trace"][-1][1]).splitlines())
