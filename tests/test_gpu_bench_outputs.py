"""GPU: a plain `bench.py` run (no --full) on the S cfg and what
--dump-outputs writes of its last timed check, against the golden S case."""
import json
import os
import subprocess
import sys

import pytest

import tlcgpu
from conftest import GOLDEN, ROOT, model_of

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_its_last_check(tmp_path):
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "s", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    want = GOLDEN["S"]["result"]
    # the headline only: no other engine, no CPU baseline
    assert line["full"] is False and line["engines"] == {} and "cpu_baseline" not in line
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(want["distinct"] / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # what the timed path returned
    assert np.load(out / "counts.npy").tolist() == [want["generated"], want["distinct"], want["depth"], 1]
    assert np.load(out / "levels.npy").tolist() == want["levels"]
    assert np.load(out / "level_generated.npy").sum() == want["generated"]
    comp = np.load(out / "states_sample_component.npy").astype(np.int64)
    sample = np.load(out / "states_sample.npy")
    assert sample.dtype == np.float64 and sample.shape == (len(comp), 2)
    assert sample.min() >= 0 and sample.max() < 2 ** 32 and (sample == np.floor(sample)).all()
    words = (sample[:, 0].astype(np.uint64) | (sample[:, 1].astype(np.uint64) << np.uint64(32))).tolist()
    # the sampled components (several hundred of the 729), each one's states in
    # its queue order: the initial state first, no state twice, every state
    # one that the HBM-FPSet engine reaches, and for a few components exactly
    # the host model's closure
    m = model_of(GOLDEN["S"]["constants"])
    ck = tlcgpu.Checker(m, engine="global")
    try:
        reachable = set(ck.copy_states(0, ck.run().distinct))
    finally:
        ck.close()
    assert len(reachable) == want["distinct"]
    assert len(set(words)) == len(words) and set(words) <= reachable
    comps = sorted(set(comp.tolist()))
    assert 200 < len(comps) <= want["levels"][0] and (np.diff(comp) >= 0).all()
    by_comp = {}
    for w, c in zip(words, comp.tolist()):
        by_comp.setdefault(c, []).append(w)
    for k, ci in enumerate(comps):
        mine = by_comp[ci]
        assert mine[0] == tlcgpu.host_init_state(m, ci)
        assert len(mine) == want["distinct"] // want["levels"][0]
        if k % 64 == 0:
            seen, todo = set(), [mine[0]]
            while todo:
                s = todo.pop()
                if s not in seen:
                    seen.add(s)
                    todo.extend(t for _, t in tlcgpu.host_successors(m, s))
            assert set(mine) == seen
