"""Regenerate tests/golden/user_eval.json: the outcome of every predicate of
tests/user_eval_cases.py EVAL_CASES on every state of its CONFIGS, from the
Python oracle alone (oracle/oracle_py.py with oracle/tla_eval.py).  Nothing
the product evaluates goes into the file: the product only packs the states
(their count and the hash of the packed words tie the strings to the states a
test evaluates).

    python tests/golden/make_golden_user_eval.py

Each outcome string is stored run-length encoded (user_eval_cases.rle: the
file is a fixture, not a listing of 400,000 digits), one predicate per line,
and a test regenerates a config and compares its block of lines byte for byte
(config_block)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import user_eval_cases as U  # noqa: E402
from user_inv_cases import oracle_model  # noqa: E402

import oracle_py  # noqa: E402


def oracle_refused():
    """the predicates the oracle's parser does not take (none of their strings are recorded)"""
    out = []
    for name in sorted(U.EVAL_CASES):
        try:
            oracle_model(U.group_model("N2C2", [name]))
        except Exception:  # noqa: BLE001  (outside the oracle evaluator's subset)
            out.append(name)
    return out


def config_entry(cfg, refused):
    pairs = U.config_pairs(cfg)
    sw = U.T.state_words(U.base_model(cfg))
    outcomes = {}
    for name in sorted(U.EVAL_CASES):
        if name in refused:
            continue
        om = oracle_model(U.group_model(cfg, [name]))
        digits = []
        for _, o in pairs:
            try:
                digits.append("0" if om.inv(name, o) else "1")
            except oracle_py.EvalError:
                digits.append("2")
        outcomes[name] = U.rle("".join(digits))
    constants = {k: (list(v) if isinstance(v, (tuple, list, range)) else v) for k, v in U.CONFIGS[cfg][0].items()}
    return {"constants": constants, "state_words": sw, "states": len(pairs),
            "hash": U.words_hash([w for w, _ in pairs], sw)}, outcomes


def config_block(cfg, refused):
    head, outcomes = config_entry(cfg, refused)
    rows = ",\n".join(f" {json.dumps(n)}: {json.dumps(s)}" for n, s in sorted(outcomes.items()))
    return json.dumps(cfg) + ": " + json.dumps(head, sort_keys=True)[:-1] + ', "outcomes": {\n' + rows + "\n}}"


def main():
    refused = oracle_refused()
    assert len(refused) * 5 <= len(U.EVAL_CASES), refused
    lines = [config_block(cfg, refused) for cfg in U.CONFIGS]
    text = ("{\n\"predicates\": " + json.dumps(sorted(U.EVAL_CASES)) + ",\n\"oracle_refused\": " + json.dumps(refused) +
            ",\n\"encoding\": " + json.dumps(U.RLE_DOC) + ",\n\"configs\": {\n" + ",\n".join(lines) + "\n}\n}\n")
    json.loads(text)
    with open(U.GOLDEN, "w") as f:
        f.write(text)
    print(f"{U.GOLDEN}: {len(text)} bytes, " + ", ".join(f"{c} {len(U.config_pairs(c))}" for c in U.CONFIGS))


if __name__ == "__main__":
    main()
