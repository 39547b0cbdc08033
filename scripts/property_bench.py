"""Figures of DESIGN section 7 for the property pass (tlcg_check_property):
kernel_ms / classify_ms / wall_ms of properties A and B on S, of Termination's
conjunction written as a user property next to tlcg_check_termination on
S_consumer (one warm-up call, then 5 alternating repetitions; medians and
spread), and of B on G9 (one call, checked against 16^6 x S's per-component
figures).  Needs an MI355X; prints one JSON line per case.

    python scripts/property_bench.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402,F401
import tlcgpu  # noqa: E402
from conftest import GOLDEN, model_of  # noqa: E402
from property_cases import PROPS, prop_model  # noqa: E402
from user_inv_cases import HELPERS  # noqa: E402



def emit(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return sorted(xs)[len(xs) // 2]


runs = {"S_A": lambda: tlcgpu.check_property(prop_model("S", "A"), "Prop", "wf"),
        "S_B": lambda: tlcgpu.check_property(prop_model("S", "B"), "Prop", "wf"),
        "S_consumer_T_property": lambda: tlcgpu.check_property(prop_model("S_consumer", "T"), "Prop", "wf"),
        "S_consumer_check_termination": lambda: tlcgpu.check_termination(model_of(GOLDEN["S_consumer"]["constants"]), "wf")}
for f in runs.values():
    f()
acc = {k: [] for k in runs}
for rep in range(5):
    for k, f in runs.items():
        r = f()
        acc[k].append((r.kernel_ms, getattr(r, "classify_ms", 0.0), r.wall_ms, r.states_notp, r.holds))
for k, v in acc.items():
    emit(case=k, reps=len(v), kernel_ms_median=med([x[0] for x in v]), kernel_ms_min=min(x[0] for x in v),
         kernel_ms_max=max(x[0] for x in v), classify_ms_median=med([x[1] for x in v]),
         wall_ms_median=med([x[2] for x in v]), wall_ms_min=min(x[2] for x in v), wall_ms_max=max(x[2] for x in v),
         states_notp=v[0][3], holds=v[0][4])

# G9: components are isomorphic, so B's figures are 16^6 times S's per component (729 components in S)
defs = dict(HELPERS)
defs["Prop"] = PROPS["B"][3]
g9 = tlcgpu.Model(key_space=range(1, 16), value_space=range(1, 16), user_defs=defs)
r = tlcgpu.check_property(g9, "Prop", "wf", state_capacity=1_040_187_392 + 1024)
k = 16 ** 6
emit(case="G9_B", kernel_ms=r.kernel_ms, classify_ms=r.classify_ms, wall_ms=r.wall_ms, reachable=r.reachable,
     seeds=r.seeds, states_notp=r.states_notp, edges_notp=r.edges_notp, stuck=r.stuck, depth=r.depth, kind=r.kind,
     trace_len=len(r.trace), seed_at=r.seed_at)
assert (r.reachable, r.seeds, r.states_notp, r.edges_notp, r.stuck) == \
    (1_040_187_392, k * 48, k * 48, k * 36, k * 4), "G9 B differs from 16^6 x S's per-component figures"
emit(case="G9_B_checked", ok=True)
