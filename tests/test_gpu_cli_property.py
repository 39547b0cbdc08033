"""GPU: tlc-hip checking properties the user defines (here added with -defs to
the built-in module, as the box has no .tla): the cfg's properties in order up
to the first one violated, the counterexample block, the property's name in
-json, and an evaluation error of P reported as an error."""
import json

import pytest

import tlcgpu
from conftest import GOLDEN
from property_cases import PROPS, prop_model
from test_cli import numeric_cfg
from test_gpu_cli import run

pytestmark = pytest.mark.gpu

ADDED = ("FairSpec == Spec /\\ WF_vars(Next)\n\n"
         "UpdateLeadsToCursor == " + PROPS["A"][3] + "\n\n"
         "AlwaysBackToPhaseOne == " + PROPS["B"][3] + "\n\n"
         "CursorEventually == " + PROPS["D"][3] + "\n\n"
         "LedgerLength == " + PROPS["ERR"][3] + "\n")


def run_with(tmp_path, props, fair, args=()):
    defs = tmp_path / "added.tla"
    defs.write_text(ADDED)
    cfg = numeric_cfg(PROPERTY=props)
    if fair:
        cfg = cfg.replace("SPECIFICATION Spec", "SPECIFICATION FairSpec")
    return run(tmp_path, cfg, ["-defs", str(defs)] + list(args))


def test_cli_properties_in_order_under_fairness(tmp_path):
    """under WF_vars(Next) on S: A and D hold, B fails at a state where
    <<Next>>_vars is disabled; the report is B's, the run stops there"""
    want = GOLDEN["S"]["result"]
    rc, lines = run_with(tmp_path, "UpdateLeadsToCursor CursorEventually AlwaysBackToPhaseOne Termination", True, ["-json"])
    assert rc == 13, lines[-20:]
    pr = tlcgpu.check_property(prop_model("S", "B"), "Prop", "wf")
    assert not pr.holds and pr.kind == "stuttering"
    i = lines.index("Error: Temporal properties were violated.")
    assert lines[i - 1].startswith("Finished checking temporal properties in ")
    assert lines[i + 2] == "Error: The following behavior constitutes a counter-example:"
    assert lines[i + 4] == "State 1: <Initial predicate>"
    assert f"State {len(pr.trace) + 1}: Stuttering" in lines
    assert f"State {len(pr.trace) + 2}: Stuttering" not in lines
    # the end state is the documented pick: the one check_property returns
    last = tlcgpu.decode(prop_model("S", "B"), pr.trace[-1][1]).split("\n")
    j = lines.index(f"State {len(pr.trace) + 1}: Stuttering")
    assert lines[j - 1 - len(last):j - 1] == last
    assert lines.count("Error: Temporal properties were violated.") == 1
    assert f"{want['generated']} states generated, {want['distinct']} distinct states found, 0 states left on queue." in lines
    res = json.loads(lines[-1])
    assert res["violated_property"] == "AlwaysBackToPhaseOne" and res["distinct"] == want["distinct"]


def test_cli_property_without_fairness_and_holding_run(tmp_path):
    """Spec has no fairness: the first seed in BFS order, then stuttering; and a
    fair run whose properties all hold completes with no error"""
    rc, lines = run_with(tmp_path, "UpdateLeadsToCursor", False, ["-json"])
    assert rc == 13
    pr = tlcgpu.check_property(prop_model("S", "A"), "Prop", "none")
    assert f"State {len(pr.trace) + 1}: Stuttering" in lines and len(pr.trace) == pr.seed_at + 1
    assert json.loads(lines[-1])["violated_property"] == "UpdateLeadsToCursor"
    rc, lines = run_with(tmp_path, "UpdateLeadsToCursor CursorEventually", True, ["-json"])
    assert rc == 0, lines[-20:]
    assert "Model checking completed. No error has been found." in lines
    assert "violated_property" not in lines[-1]
    assert any(l.startswith("Finished checking temporal properties in ") for l in lines)


def test_cli_property_evaluation_error(tmp_path):
    rc, lines = run_with(tmp_path, "LedgerLength", True)
    assert rc == 75, lines[-20:]
    assert any(l.startswith("Error: Evaluating property LedgerLength failed: evaluating P (the left operand) of property "
                            "LedgerLength failed on a reachable state") for l in lines)
    assert "Error: The behavior up to this point is:" in lines and "State 1: <Initial predicate>" in lines
    assert "Error: Temporal properties were violated." not in lines
