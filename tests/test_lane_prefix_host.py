"""CPU: the per-lane kernel's prefix form (component_lane.h TLCG_LANE_PREFIX)
keeps a component only if its FIFO BFS, in the kernel's order, inserts S's
codes in dense order at every insert.  tlcg_host_lane_prefix_selfcheck counts
those components through the owner table; here the count is compared with a
walk of its own over tlcgpu.host_successors, which knows nothing of codes or
tables: component 0's walk is taken as S (per expansion, the actions and the
queue position each successor lands on -- an old position, or the queue's
length for a new state), and a component is kept when its walk has the same
shape, expansion by expansion.

On every model here the count is the number of components asked for: no
golden case leaves S's order (that path of the kernel is reached only through
the test-only TLCG_LANE_PREFIX_BREAK, tests/test_gpu_lane_prefix.py)."""
import ctypes as C
import random

import pytest

import tlcgpu
from conftest import GOLDEN, model_of

G9 = dict(key_space=range(1, 16), value_space=range(1, 16))
STUTTERS = ("Consumer", "Terminating")


def walk_shape(m, idx):
    """the FIFO BFS of the component of initial state idx, in the kernel's
    order (the compactor's successor, then BrokerCrash's; the stutters lead
    nowhere new): per expansion a tuple of (action, queue position)"""
    q = [tlcgpu.host_init_state(m, idx)]
    pos = {q[0]: 0}
    shape = []
    head = 0
    while head < len(q):
        row = []
        for action, t in tlcgpu.host_successors(m, q[head]):
            if t == q[head] and any(s in action for s in STUTTERS):
                continue
            if t not in pos:
                pos[t] = len(q)
                q.append(t)
            row.append((action, pos[t]))
        shape.append(tuple(row))
        head += 1
    return shape


def kept_by_walk(m, comps, shape0):
    return sum(1 for i in comps if walk_shape(m, i) == shape0)


def inserts_in_order(shape):
    """the walk inserts position tail at tail, by construction of walk_shape;
    what is checked is that it names every position once"""
    new, tail = [], 1
    for row in shape:
        for _, p in row:
            if p == tail:
                new.append(p)
                tail += 1
            else:
                assert p < tail
    return new == list(range(1, tail)) and tail == len(shape)


@pytest.mark.parametrize("case", ["S", "X_keys3_vals57", "R_C2_K2", "R_C3_K0"])
def test_every_component_of_a_golden_cfg_is_kept(case):
    m = model_of(GOLDEN[case]["constants"])
    n = tlcgpu.init_count(m)
    assert n == {"S": 729, "X_keys3_vals57": 144}.get(case, n)
    shape0 = walk_shape(m, 0)
    assert inserts_in_order(shape0)
    assert len(shape0) == tlcgpu.host_lane_owner_selfcheck(m)[0]  # |S|
    want = kept_by_walk(m, range(n), shape0)
    assert tlcgpu.host_lane_prefix_selfcheck(m, 0, n) == want == n
    # a range past the last component is clipped
    assert tlcgpu.host_lane_prefix_selfcheck(m, max(n - 3, 0), 10) == min(n, 3)


def test_g9_first_components_and_a_seeded_sample():
    m = tlcgpu.Model(**G9)
    n = tlcgpu.init_count(m)
    shape0 = walk_shape(m, 0)
    assert len(shape0) == 62 and inserts_in_order(shape0)
    assert tlcgpu.host_lane_prefix_selfcheck(m, 0, 4096) == 4096
    rng = random.Random(10)
    sample = sorted(rng.sample(range(4096, n), 4096))
    assert sample[-1] > n // 2  # (the sample reaches the far half of the 16.7 M components)
    assert sum(tlcgpu.host_lane_prefix_selfcheck(m, i, 1) for i in sample) == 4096
    assert kept_by_walk(m, list(range(4096)) + sample, shape0) == 8192


def test_models_the_pass_does_not_take():
    assert tlcgpu.host_lane_prefix_selfcheck(tlcgpu.Model(model_producer=True), 0, 16) == 0
    assert tlcgpu.host_lane_prefix_selfcheck(tlcgpu.Model(compaction_times_limit=12), 0, 16) == 0
    assert tlcgpu.host_lane_prefix_selfcheck(tlcgpu.Model(max_crash_times=2), 0, 16) == 0  # (> 62 codes)


@pytest.mark.parametrize("define", ["TLCG_LANE_PREFIX=0", "TLCG_LANE_PREFIX_BREAK=1", "TLCG_LANE_FP_REG=0",
                                    "TLCG_LANE_OWNER_RING=0"])
def test_g9_module_compiles_with_define(define, tmp_path, monkeypatch):
    monkeypatch.setenv("TLCG_JIT_CACHE", str(tmp_path / "jit"))
    monkeypatch.setenv("TLCG_JIT_DEFINES", define)
    m = tlcgpu.Model(**G9).to_c()
    err = C.create_string_buffer(4096)
    n = tlcgpu.load_library().tlcg_jit_selftest(C.byref(m), b"gfx950", err, 4096)
    assert n > 0, err.value.decode()[:2000]
