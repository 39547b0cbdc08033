"""CPU: tlc-hip's cfg binding of a PROPERTY the user defines (host/cfg.cpp
through the temporal front end, tlcg_host_property_form).  The built-in module
with -defs needs no .tla, so these run wherever the binary does; the run goes
on to the GPU only after the line checked here."""
import os
import subprocess

import pytest

from conftest import CLI
from test_cli import TLA, needs_ref, numeric_cfg, run_cli

ADDED = ("CursorSet == cursor # Nil\n\n"
         "UpdateLeadsToCursor == compactorState = Compactor_In_PhaseTwoUpdateContext ~> CursorSet\n\n"
         "AlwaysBackToPhaseOne == []<>(compactorState = Compactor_In_PhaseOne)\n\n"
         "BoxForm ==\n    [](  (crashTimes = MaxCrashTimes /\\ crashTimes > 0)\n      => <>(compactorState = Compactor_In_PhaseTwoWrite))\n\n"
         "EventuallyAlways == <>[]CursorSet\n\n"
         "Both ==\n    /\\ <>CursorSet\n    /\\ []<>CursorSet\n\n"
         "Mixed == crashTimes > 0 => cursor = Nil ~> CursorSet\n\n"
         "Primed == <>(cursor' # Nil)\n\n"
         "Plain == cursor # Nil\n")


def run_builtin(tmp_path, prop, args=()):
    defs = tmp_path / "added.tla"
    defs.write_text(ADDED)
    cfg = tmp_path / "m.cfg"
    cfg.write_text(numeric_cfg(PROPERTY=prop))
    p = subprocess.run([CLI, "-config", str(cfg), "-defs", str(defs)] + list(args), capture_output=True, text=True,
                       timeout=60, cwd=str(tmp_path))
    return p.returncode, p.stdout + p.stderr


@pytest.mark.parametrize("prop", ["UpdateLeadsToCursor", "AlwaysBackToPhaseOne", "BoxForm",
                                  "UpdateLeadsToCursor AlwaysBackToPhaseOne"])
def test_added_property_is_accepted(tmp_path, prop):
    rc, out = run_builtin(tmp_path, prop)
    assert "Computing initial states..." in out, out
    assert "cannot be checked" not in out and "is not one this checker implements" not in out


@pytest.mark.parametrize("prop,parts", [
    ("EventuallyAlways", ["property EventuallyAlways cannot be checked: <>[] (eventually always) at line 11, col 21"]),
    ("Both", ["property Both cannot be checked: a bulleted list containing a temporal operator (<>) at line 14, col 8"]),
    ("Mixed", ["property Mixed cannot be checked: a top-level => beside ~>", "line 17"]),
    ("Primed", ["property Primed cannot be checked: a primed variable (')", "line 19"]),
    ("UpdateLeadsToCursor EventuallyAlways", ["property EventuallyAlways cannot be checked"]),
])
def test_refused_form_exits_150_with_the_message(tmp_path, prop, parts):
    rc, out = run_builtin(tmp_path, prop)
    for p in parts:
        assert p in out, out
    assert "Computing initial states" not in out
    assert rc == 150


def test_state_predicate_keeps_the_config_error(tmp_path):
    rc, out = run_builtin(tmp_path, "Plain")
    assert "temporal property Plain is not one this checker implements" in out
    assert "Computing initial states" not in out
    assert rc == 151


@needs_ref
def test_property_added_to_the_module(tmp_path):
    """the same through a .tla: the definition's line in the message is the module's"""
    text = open(TLA).read()
    end = text.rindex("\n====") + 1
    line = text[:end].count("\n") + 1
    added = "Recovers == (crashTimes = MaxCrashTimes /\\ crashTimes > 0) ~> compactorState = Compactor_In_PhaseTwoWrite\n\n" \
            "Stays == <>[](cursor # Nil)\n\n"
    rc, out = run_cli(tmp_path, numeric_cfg(PROPERTY="Recovers"), tla_text=text[:end] + added + text[end:])
    assert "Computing initial states..." in out, out
    rc, out = run_cli(tmp_path, numeric_cfg(PROPERTY="Stays"), tla_text=text[:end] + added + text[end:])
    assert f"property Stays cannot be checked: <>[] (eventually always) at line {line + 2}, col 10" in out, out
    assert rc == 150
    # Termination as published still goes the old way, beside a user property
    rc, out = run_cli(tmp_path, numeric_cfg(PROPERTY="Termination Recovers"), tla_text=text[:end] + added + text[end:])
    assert "Computing initial states..." in out, out
