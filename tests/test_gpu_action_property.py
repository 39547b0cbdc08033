"""GPU: action properties [][A]_v checked on every step of the reachable graph
(tlcg_check_action_property, csrc/liveness.hip) against the test-side reference
of tests/action_ref.py (the oracle's TLA+ evaluator over two copies of the
variables): nothing the device computes feeds the expectation.  Counts, the
verdict, the reported step by the documented rule and the trace, step by step
against tlcgpu.host_successors; the device interpreter against the host's on
every step; regrowth from a store far too small; the step pass on explicit
graphs with a verdict byte per edge; and tlc-hip end to end."""
import functools
import random
import re
import subprocess

import pytest

import tlcgpu
from action_cases import ACTIONS, EXPECTED, action_model, pairs_of, ref_summary, steps_of
from action_ref import graph_ref
from conftest import CLI, GOLDEN
from liveness_graph_cases import HAND, PARAMS, STARRED, random_graph
from test_cli import numeric_cfg

pytestmark = pytest.mark.gpu

MODEL_CASES = ["R_C1_K2", "R_C2_K1", "X_producer_sparse", "WIDE1"]


def check_model_result(case, prop, m, r):
    want = ref_summary(case, prop)
    states, nsteps, _ = EXPECTED[case]
    level = steps_of(case)[1]
    print(f"{case} {prop}: reachable {r.reachable}, steps {r.steps}, violating {r.violating}, erroring {r.erroring}, "
          f"depth {r.depth}, {r.kind}; kernels {r.kernel_ms:.3f} ms, check {r.check_ms:.3f} ms, call {r.wall_ms:.1f} ms")
    assert (r.reachable, r.steps) == (states, nsteps) == (len(pairs_of(case)), want["steps"])
    assert (r.violating, r.erroring) == (want["violating"], want["erroring"])
    assert r.depth == max(level.values())
    rep = want["reported"]
    if rep is None:
        assert r.holds and r.kind == "holds" and r.trace == [] and r.step_action is None
        assert r.step_depth == 0 and r.error_state == -1 and r.error is None
        return
    assert not r.holds and r.kind == ("error" if rep["verdict"] == 2 else "violated")
    # the reported step: shallowest level, least packed source of that level's
    # flagged states, its lowest flagged move
    assert r.step_depth == rep["level"]
    assert (r.trace[-2][1], r.trace[-1][1]) == (rep["source"], rep["target"])
    assert r.trace[-1][0] == r.step_action
    # a shortest path from an initial state, stepwise in host_successors
    assert len(r.trace) == rep["level"] + 1
    inits = {tlcgpu.host_init_state(m, i) for i in range(tlcgpu.init_count(m))}
    assert r.trace[0][0] == "Init" and r.trace[0][1] in inits
    for (_, s), (a, t) in zip(r.trace, r.trace[1:]):
        assert (a, t) in tlcgpu.host_successors(m, s)
    got = tlcgpu.host_action_property_eval(m, "Prop", [(rep["source"], rep["target"])])
    assert got == [rep["verdict"]]
    if rep["verdict"] == 2:
        assert r.error_state >= 0 and "evaluating the action of property Prop failed" in r.error
    else:
        assert r.error_state == -1 and r.error is None


@pytest.mark.parametrize("grid", [None, "1"], ids=["grid-default", "grid-1"])
@pytest.mark.parametrize("prop", sorted(ACTIONS))
@pytest.mark.parametrize("case", MODEL_CASES)
def test_action_property_matches_reference(monkeypatch, case, prop, grid):
    if grid is None:
        monkeypatch.delenv("TLCG_LV_GRID", raising=False)
    else:
        monkeypatch.setenv("TLCG_LV_GRID", grid)
    m = action_model(case, prop)
    assert tlcgpu.state_words(m) == (2 if case == "WIDE1" else 1)
    check_model_result(case, prop, m, tlcgpu.check_action_property(m, "Prop"))


@pytest.mark.parametrize("prop", sorted(ACTIONS))
@pytest.mark.parametrize("case", ["X_producer_sparse", "WIDE1"])
def test_device_evaluator_step_by_step(case, prop):
    """(the host interpreter equals the reference by tests/test_action_property_host.py)"""
    m = action_model(case, prop)
    steps = [(s[0], s[1]) for s in steps_of(case)[0]]
    assert len(steps) == EXPECTED[case][1]
    assert tlcgpu.action_eval_device(m, "Prop", steps) == tlcgpu.host_action_property_eval(m, "Prop", steps)


@pytest.mark.parametrize("prop", ["HorizonUp", "CrashUp"])
def test_action_property_regrows(prop):
    """S from a 100-state store and a 256-slot FPSet: the reach BFS is grown and
    redone; the counts equal the unforced run's and the issue's table"""
    m = action_model("S", prop)
    full = tlcgpu.check_action_property(m, "Prop")
    small = tlcgpu.check_action_property(m, "Prop", state_capacity=100, log2_fpset_slots=8)
    print(f"S {prop}: kernels {full.kernel_ms:.3f} ms, check {full.check_ms:.3f} ms, call {full.wall_ms:.1f} ms")
    states, nsteps, flagged = EXPECTED["S"]
    viol, lvl = flagged.get(prop, (0, 0))
    for r in (full, small):
        assert (r.reachable, r.steps, r.violating, r.erroring) == (states, nsteps, viol, 0)
        assert (r.holds, r.step_depth, r.depth) == (viol == 0, lvl, GOLDEN["S"]["result"]["depth"])
        assert len(r.trace) == (lvl + 1 if viol else 0)
    assert small.trace == [] or (small.trace[-2][1], small.trace[-1]) == (full.trace[-2][1], full.trace[-1])


def test_refused_action_property_raises():
    m = action_model("R_C1_K2", body="[][(cursor)' # Nil]_vars")
    with pytest.raises(ValueError, match="property Prop cannot be checked: .*a prime"):
        tlcgpu.check_action_property(m, "Prop")
    with pytest.raises(ValueError, match="is not of the form"):
        tlcgpu.check_action_property(action_model("R_C1_K2", body="<>(cursor # Nil)"), "Prop")


# ---- explicit graphs: grids, level shapes and out-degrees the spec's graph does not have ----

DENSITIES = (0.0, 0.1, 1.0)


def word_of(words):
    return (lambda v: v) if words == 1 else (lambda v: v | (v >> 3) << 64)  # (ExplicitGraph::word_of)


def check_graph(monkeypatch, key, regrow=False):
    g = HAND[key] if isinstance(key, str) else random_graph(*key)
    n = len(g.row) - 1
    for density in DENSITIES:
        rng = random.Random(f"v/{key}/{density}")
        verdict = [(1 + (rng.random() < 0.3)) if rng.random() < density else 0 for _ in g.col]
        for words in (1, 2):
            want = graph_ref(g.row, g.col, verdict, g.n_init, word_of(words))
            for grid in (None, "1"):
                if grid is None:
                    monkeypatch.delenv("TLCG_LV_GRID", raising=False)
                else:
                    monkeypatch.setenv("TLCG_LV_GRID", grid)
                runs = [dict()]
                if regrow and grid is None:
                    runs.append(dict(state_capacity=100, log2_fpset_slots=8))
                for kw in runs:
                    r = tlcgpu.action_property_graph(g.row, g.col, verdict, g.n_init, words=words, **kw)
                    at = (key, density, words, grid, kw)
                    assert (r.reachable, r.depth, r.steps, r.violating, r.erroring) == \
                        (want["reachable"], want["depth"], want["steps"], want["violating"], want["erroring"]), at
                    rep = want["reported"]
                    if rep is None:
                        assert r.holds and r.kind == "holds" and r.trace == [] and r.step_depth == 0, at
                        continue
                    lv, src, dst, k, v = rep
                    assert not r.holds and r.kind == ("error" if v == 2 else "violated"), at
                    assert (r.step_depth, r.step_action) == (lv, k), at
                    assert (r.trace[-2][1], r.trace[-1]) == (src, (k, dst)), at
                    assert (r.error_state >= 0) == (v == 2), at
                    # a shortest path from an initial node along edges of the graph
                    assert len(r.trace) == lv + 1 and r.trace[0][0] == "Init", at
                    nodes = [w & 0xFFFFFFFF for _, w in r.trace]
                    assert all(w == word_of(words)(v_) for (_, w), v_ in zip(r.trace, nodes)), at
                    assert nodes[0] < g.n_init, at
                    for a, b, (e, _) in zip(nodes, nodes[1:], r.trace[1:]):
                        assert g.row[a] + e < g.row[a + 1] and g.col[g.row[a] + e] == b and a != b, at


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_graph(monkeypatch, name):
    check_graph(monkeypatch, name)


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "n%d-%s-deg%d-s%d" % p)
def test_random_graph(monkeypatch, params):
    check_graph(monkeypatch, params, regrow=params[0] in STARRED)


def test_generated_set_covers_the_shapes():
    """among the graphs above: a last partial wave, states with no move, an
    out-degree above one batch of 4, repeated edges and self-loops"""
    gs = [random_graph(*p) for p in PARAMS]
    assert any((len(g.row) - 1) % 64 for g in gs) and any(len(g.row) - 1 > 256 for g in gs)
    assert any(g.row[v] == g.row[v + 1] for g in gs for v in range(len(g.row) - 1))
    assert any(g.row[1] - g.row[0] > 4 for g in gs)
    assert any(len(set(g.col[g.row[v]:g.row[v + 1]])) < g.row[v + 1] - g.row[v] for g in gs for v in range(len(g.row) - 1))
    assert any(v in g.col[g.row[v]:g.row[v + 1]] for g in gs for v in range(len(g.row) - 1))
    # a wide node among 5000, every edge violating: each move that leaves its node is a step
    g = random_graph(5000, "cyclic", 9, 0)
    r = tlcgpu.action_property_graph(g.row, g.col, [1] * len(g.col), g.n_init)
    want = graph_ref(g.row, g.col, [1] * len(g.col), g.n_init, word_of(1))
    assert (r.steps, r.violating, r.step_depth) == (want["steps"], want["steps"], 1) and r.steps > 4


# ---- tlc-hip end to end: the built-in module with -defs ----

ADDED = ("HorizonUp == [][compactionHorizon' >= compactionHorizon]_vars\n\n"
         "CrashUp == [][crashTimes' >= crashTimes /\\ crashTimes' <= crashTimes + 1]_vars\n\n"
         "ErrNext == [][Len(compactedLedgers'[compactedTopicContext']) >= 0]_vars\n\n"
         "AlwaysBackToPhaseOne == []<>(compactorState = Compactor_In_PhaseOne)\n")


def run_builtin(tmp_path, prop, args=()):
    defs = tmp_path / "added.tla"
    defs.write_text(ADDED)
    cfg = tmp_path / "m.cfg"
    cfg.write_text(numeric_cfg(PROPERTY=prop))
    p = subprocess.run([CLI, "-config", str(cfg), "-defs", str(defs)] + list(args), capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    return p.returncode, p.stdout + p.stderr


def test_cli_reports_a_violated_action_property(tmp_path):
    rc, out = run_builtin(tmp_path, "HorizonUp", ["-json"])
    assert rc == 12, out
    assert "Error: Action property HorizonUp is violated." in out
    assert "Error: The behavior up to this point is:" in out
    assert "45198 distinct states found" in out  # (the completed search's counts)
    hz = [int(x) for x in re.findall(r"/\\ compactionHorizon = (\d+)", out)]
    states = re.findall(r"^State (\d+): <", out, re.M)
    assert len(hz) == len(states) == EXPECTED["S"][2]["HorizonUp"][1] + 1
    assert states[0] == "1" and "State 1: <Initial predicate>" in out
    assert hz[-1] < hz[-2]  # the last state is the successor: the horizon moved backwards
    assert '"violated_property": "HorizonUp"' in out


def test_cli_checks_action_and_temporal_properties_together(tmp_path):
    rc_alone, alone = run_builtin(tmp_path, "AlwaysBackToPhaseOne")
    rc, out = run_builtin(tmp_path, "CrashUp AlwaysBackToPhaseOne")
    assert rc == rc_alone, out
    assert "Action property" not in out and "cannot be checked" not in out
    # (which seed the liveness counterexample starts from is decided by the
    # reach pass's races: the report is compared but for the states' values)
    keep = lambda text: [l for l in text.splitlines()  # noqa: E731
                         if not re.search(r"\d\d:\d\d:\d\d|Finished|^/\\ |^State \d+: <", l)]
    assert keep(out) == keep(alone)
    assert "Error: Temporal properties were violated." in out and rc == 13
    # a violated action property ends the run before the temporal ones
    rc, out = run_builtin(tmp_path, "AlwaysBackToPhaseOne HorizonUp")
    assert rc == 12 and "Temporal properties were violated" not in out


def test_cli_action_evaluation_error(tmp_path):
    rc, out = run_builtin(tmp_path, "ErrNext")
    assert rc == 75, out
    assert "Error: Evaluating property ErrNext failed: evaluating the action of property ErrNext failed" in out
    assert re.findall(r"^State (\d+): <", out, re.M) == ["1", "2"]  # an initial state and its successor
