"""Child process of the constraint GPU tests: runs the given cases of
constraint_cases.py on the device under the environment it was started with
(TLCG_JIT, ...) and writes what the tests compare to a JSON file.

    python constraint_run.py OUT.json CASE[:tlc_order[:keyword=value,...]] ..."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pulsar-tlaplus_amd", "python"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)

import constraint_cases as CC  # noqa: E402
import tlcgpu as T  # noqa: E402


def run_case(name, tlc_order, **kw):
    m = CC.model_of(name)
    ck = T.Checker(m, tlc_order=bool(tlc_order), **kw)
    try:
        ck.run_raw()
        r = ck.result()
        discarded, pass_ms, level_ms = ck.constraint_stats()
        return dict(status=r.status, invariant=r.invariant, constraint=r.constraint, generated=r.generated,
                    distinct=r.distinct, depth=r.depth, levels=r.levels, engine=r.engine, jit_used=r.jit_used,
                    levels_redone=r.levels_redone, tlc_exact=r.tlc_exact, trace=[[a, s] for a, s in r.trace],
                    states=ck.copy_states(0, r.distinct), discarded=discarded, pass_ms=pass_ms,
                    pass_levels=len(level_ms), kernel_ms=r.kernel_ms, expand_ms=r.expand_ms)
    finally:
        ck.close()


def main(argv):
    out = {}
    for spec in argv[2:]:
        name, _, rest = spec.partition(":")
        tlc, _, kws = rest.partition(":")
        kw = {}
        for item in filter(None, kws.split(",")):
            k, _, v = item.partition("=")
            kw[k] = v if k == "engine" else int(v)
        out[spec] = run_case(name, int(tlc or 0), **kw)
    with open(argv[1], "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
