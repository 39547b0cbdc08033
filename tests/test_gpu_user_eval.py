"""GPU: the user invariants state by state on the device, against the Python
oracle's recorded outcomes (tests/golden/user_eval.json).

A whole check reports the first violating state and stops, so a generated
predicate that is wrongly TRUE, or wrong past the first violation, passes it.
tlcg_user_eval_selftest evaluates every user invariant of a model on given
states in each form the engines run: the interpreter (k_user_check's, path
"interpreter"), the generated code over the packed word (tlcg_user_check's,
"word"), the generated code over the component code (the on-chip engines'
view, "code") and the outcome tables (code_consts_user + user_eval_c,
"tables", also as TLCG_UTAB=dyn and slow build them).  Every outcome of every
predicate on every state of the small configs of tests/user_eval_cases.py,
one-word and two-word, must be the oracle's."""
import pytest

import tlcgpu
import user_eval_cases as U

pytestmark = pytest.mark.gpu

PATHS = ("interpreter", "word", "code", "tables")
# the configs every state of which has a component code (no Producer; host
# side: tests/test_user_codegen_host.py checks the same by tlcg_host_component_selfcheck)
CODED = U.ONE_WORD_CLOSED + ["wide"]


def compare(cfg, gi, path):
    names = U.GROUPS[gi]
    words = U.checked_words(cfg)
    got = tlcgpu.user_eval_states(U.group_model(cfg, names), words, path)
    assert len(got) == len(names)
    nocode = [i for i, x in enumerate(got[0]) if x == 0xFF]
    if path in ("interpreter", "word") or cfg in CODED:
        assert not nocode, (cfg, len(nocode))
    elif len(nocode) == len(words):
        pytest.skip("the hook reports no component codes for this config")
    skip = set(nocode)
    for name, g in zip(names, got):
        assert len(g) == len(words)
        assert [i for i, x in enumerate(g) if x == 0xFF] == nocode, name  # (a state has a code or not, for every invariant)
        want = U.golden_outcomes(cfg, name)
        diff = [(i, x, int(w)) for i, (x, w) in enumerate(zip(g, want)) if i not in skip and x != int(w)]
        assert not diff, (name, len(diff), diff[:5])


@pytest.mark.parametrize("gi", range(len(U.GROUPS)))
@pytest.mark.parametrize("cfg", list(U.CONFIGS))
@pytest.mark.parametrize("path", PATHS)
def test_device_outcomes_are_the_oracles(path, cfg, gi, monkeypatch):
    monkeypatch.delenv("TLCG_UTAB", raising=False)
    if cfg == "wide":
        assert tlcgpu.state_words(U.base_model(cfg)) == 2  # (the u128 instantiations of all four paths)
    compare(cfg, gi, path)


@pytest.mark.parametrize("gi", range(len(U.GROUPS)))
@pytest.mark.parametrize("cfg", list(U.CONFIGS))
@pytest.mark.parametrize("utab", ["dyn", "slow"])
def test_device_outcome_tables_built_per_component_or_left_to_the_programs(utab, cfg, gi, monkeypatch):
    """TLCG_UTAB=dyn: every table filled on the device, one evaluation per
    pattern; slow: every entry 3, so each state falls back to its program"""
    monkeypatch.setenv("TLCG_UTAB", utab)
    compare(cfg, gi, "tables")


def test_at_least_four_configs_evaluate_every_state_on_its_component_code():
    assert len(CODED) >= 4 and set(U.ONE_WORD_CLOSED) <= set(CODED)
    for cfg in CODED:
        assert tlcgpu.host_component_selfcheck(U.group_model(cfg, U.GROUPS[0]), 0, 32) > 0, cfg


@pytest.mark.parametrize("name", ["NoDoubleCrashWrite", "CursorHorizonLow", "ModByCrash"])
def test_whole_check_stops_at_the_first_state_the_fixture_fails(name):
    """ties the hook's states to production: the state a TLC-order check of
    one failing predicate reports is the first in BFS order whose recorded
    outcome is not TRUE"""
    cfg = "N2C2"
    words = U.checked_words(cfg)
    want = U.golden_outcomes(cfg, name)
    first = next(i for i, ch in enumerate(want) if ch != "0")
    m = U.group_model(cfg, [name])
    ck = tlcgpu.Checker(m, tlc_order=True, engine="global")
    r = ck.run()
    ck.close()
    assert r.status == ("invariant" if want[first] == "1" else "invariant_error") and r.invariant == name
    assert r.trace[-1][1] == words[first], (tlcgpu.decode(m, r.trace[-1][1]), tlcgpu.decode(m, words[first]))
