"""CPU: the recorded per-state outcomes of the user-invariant predicates
(tests/golden/user_eval.json) come from the Python oracle alone and say
something: the two smallest configs regenerated with the oracle are the
file's lines byte for byte, every outcome occurs, and a good part of the
predicates is FALSE or an evaluation error somewhere."""
import importlib.util
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import user_eval_cases as U  # noqa: E402
from user_inv_cases import CASES  # noqa: E402


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_user_eval",
                                                  os.path.join(HERE, "golden", "make_golden_user_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_predicates_and_groups_cover_the_fixtures_and_the_bench_invariants():
    from bench import USER_DEFS
    assert set(CASES) <= set(U.EVAL_CASES) and all(U.EVAL_CASES[n] == b for n, b in CASES.items())
    bench = [n for n in USER_DEFS if n not in ("NullKey", "KeySet", "ValueSet")]
    assert len(bench) == 6 and all(U.EVAL_CASES[n] == USER_DEFS[n] for n in bench)
    assert sorted(n for g in U.GROUPS for n in g) == sorted(U.EVAL_CASES)
    assert all(len(g) <= 8 for g in U.GROUPS)
    g = U.golden()
    assert g["predicates"] == sorted(U.EVAL_CASES) and list(g["configs"]) == list(U.CONFIGS)
    assert len(g["oracle_refused"]) * 5 <= len(U.EVAL_CASES)
    for cfg, e in g["configs"].items():
        assert sorted(e["outcomes"]) == sorted(set(U.EVAL_CASES) - set(g["oracle_refused"]))
        assert all(len(s) == e["states"] and set(s) <= set("012") for s in e["outcomes"].values())
        assert e["state_words"] == U.T.state_words(U.base_model(cfg)) == (2 if cfg == "wide" else 1)
        assert e["states"] <= 5000
    assert os.path.getsize(U.GOLDEN) < 100_000
    digits = "0001222011"
    assert U.rle(digits) == "3TF3ET2F" and U.unrle(U.rle(digits)) == digits and U.unrle("") == ""
    assert U.rle("2" + "011" * 3 + "0") == "E3(T2F)T" and U.unrle("E3(T2F)T12E") == "2" + "011" * 3 + "0" + "2" * 12
    rng = random.Random(7)
    for _ in range(200):  # the stored form expands to the string it was made from
        s = "".join(rng.choice(["0", "1", "2", "011", "0012"]) * rng.randint(1, 6) for _ in range(rng.randint(0, 12)))
        assert U.unrle(U.rle(s)) == s


def test_the_two_smallest_configs_regenerate_byte_for_byte():
    gen = _generator()
    text = open(U.GOLDEN).read()
    sizes = {c: e["states"] for c, e in U.golden()["configs"].items()}
    assert sorted(sizes, key=sizes.get)[:2] == U.SMALLEST
    for cfg in U.SMALLEST:
        block = gen.config_block(cfg, U.golden()["oracle_refused"])
        assert "\n" + block + "\n" in text.replace("}},\n", "}}\n"), cfg


def test_recorded_outcomes_include_failures_and_errors():
    g = U.golden()
    seen, failing = set(), set()
    for e in g["configs"].values():
        for name, s in e["outcomes"].items():
            seen |= set(s)
            if set(s) & set("12"):
                failing.add(name)
    assert seen == set("012")
    assert 3 * len(failing) >= len(U.EVAL_CASES), sorted(failing)
    # a group opens with an erroring and a failing invariant, followed by others that
    # take both outcomes after it: first-failing order and per-invariant outcomes differ
    first = U.GROUPS[0]
    o = g["configs"]["N2C2"]["outcomes"]
    assert "2" in o[first[0]] and len(first) > 2
    assert any(o[first[0]][i] == "2" and o[n][i] == "1" for n in first[1:] for i in range(len(o[n])))
