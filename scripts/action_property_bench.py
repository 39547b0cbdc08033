"""Figures of DESIGN section 7 for the action property pass
(tlcg_check_action_property): the device time of phase 1 (the reach BFS,
kernel_ms - check_ms) and of phase 2 (the step kernel, check_ms) and wall_ms
of four properties of tests/action_cases.py on S and on W_C12_k1 (one warm-up
call, then 7 repetitions; medians and phase 2's spread).  Needs an MI355X;
prints one JSON line per case.

    python scripts/action_property_bench.py"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402,F401
import tlcgpu  # noqa: E402
from action_cases import TUPLE_DEFS, prop_text  # noqa: E402
from conftest import GOLDEN, model_of  # noqa: E402
from user_inv_cases import HELPERS  # noqa: E402

for case in ("S", "W_C12_k1"):
    for prop in ("CrashUp", "HorizonUp", "AppendOnly", "LedgerGrows"):
        m = model_of(GOLDEN[case]["constants"])
        m.user_defs = dict(HELPERS, **TUPLE_DEFS, Prop=prop_text(prop))
        rs = [tlcgpu.check_action_property(m, "Prop") for _ in range(8)][1:]
        r = rs[0]
        print(json.dumps(dict(
            case=case, property=prop, words=tlcgpu.state_words(m), reachable=r.reachable, steps=r.steps,
            violating=r.violating, erroring=r.erroring, depth=r.depth, kind=r.kind, reps=len(rs),
            reach_ms_median=statistics.median(x.kernel_ms - x.check_ms for x in rs),
            check_ms_median=statistics.median(x.check_ms for x in rs), check_ms_min=min(x.check_ms for x in rs),
            check_ms_max=max(x.check_ms for x in rs), wall_ms_median=statistics.median(x.wall_ms for x in rs))),
            flush=True)
