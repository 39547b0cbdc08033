"""bench.py --gpus N: the rank launcher (CPU; no torch, no GPU in the parent).

The driver runs `python bench.py --gpus N` for BENCH and `torch.distributed.run
--nproc-per-node N bench.py --gpus N` for SCALE; both must measure N ranks
(VERDICT r4 item 1)."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_launch_plan():
    b = load_bench()
    assert b.launch_plan(1, {}) == ("run", None)
    assert b.launch_plan(8, {}) == ("spawn", 8)
    assert b.launch_plan(4, {"WORLD_SIZE": "4"}) == ("run", None)
    plan, why = b.launch_plan(8, {"WORLD_SIZE": "1"})
    assert plan == "refuse" and "WORLD_SIZE=1" in why
    assert b.launch_plan(0, {})[0] == "refuse"


def test_plain_run_is_the_default():
    b = load_bench()
    a = b.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dumped_words_are_exact(tmp_path):
    """--dump-outputs stores a 64-bit word as two float64 columns (low, high 32 bits)"""
    import numpy as np
    b = load_bench()
    words = np.array([[0, 1], [(1 << 64) - 1, (1 << 53) + 1], [0x0123456789ABCDEF, 1 << 63]], dtype=np.uint64)
    cols = b.u64_columns(words)
    assert cols.dtype == np.float64 and cols.shape == (3, 4)
    back = cols[:, 0::2].astype(np.uint64) | (cols[:, 1::2].astype(np.uint64) << np.uint64(32))
    assert (back == words).all()
    b.write_outputs(str(tmp_path / "d"), {"states_sample": cols}, 0)
    b.write_outputs(str(tmp_path / "d"), {"states_sample": cols}, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["states_sample.npy", "states_sample.rank1.npy"]
    assert (np.load(tmp_path / "d" / "states_sample.npy") == cols).all()


CHILD = r"""
import json, os, sys
r, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert os.environ["LOCAL_RANK"] == str(r) and os.environ["MASTER_ADDR"] == "127.0.0.1"
assert int(os.environ["MASTER_PORT"]) > 0
print(json.dumps({"rank": r, "world": n}), flush=True)
if str(r) == os.environ.get("HANG_RANK"):
    import time
    time.sleep(600)
sys.exit(int(os.environ.get("FAIL_RANK_RC", "0")) if str(r) == os.environ.get("FAIL_RANK") else 0)
"""


def run_spawn(n, extra_env, grace=5.0):
    code = ("import importlib.util,sys;"
            f"s=importlib.util.spec_from_file_location('b',{os.path.join(ROOT, 'bench.py')!r});"
            "m=importlib.util.module_from_spec(s);s.loader.exec_module(m);"
            f"sys.exit(m.spawn_ranks({n},[sys.executable,'-c',{CHILD!r}],grace_s={grace}))")
    env = dict(os.environ, **extra_env)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)


def test_spawn_ranks_rank0_stdout_only():
    p = run_spawn(3, {})
    assert p.returncode == 0, p.stderr
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines == [{"rank": 0, "world": 3}]  # the other ranks' stdout went to stderr
    assert '"rank": 1' in p.stderr and '"rank": 2' in p.stderr


def test_spawn_ranks_failing_rank_sets_the_exit_code():
    p = run_spawn(2, {"FAIL_RANK": "1", "FAIL_RANK_RC": "7"})
    assert p.returncode == 7
    assert "rank 1 of 2 failed first (exit 7)" in p.stderr


def test_bench_refuses_a_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "refused" in p.stderr and "WORLD_SIZE=2" in p.stderr


def test_spawn_ranks_ends_a_rank_left_hanging():
    """rank 1 fails, rank 0 waits in a 'collective' forever: terminated after the grace"""
    import time
    t = time.time()
    p = run_spawn(2, {"FAIL_RANK": "1", "FAIL_RANK_RC": "5", "HANG_RANK": "0"}, grace=2.0)
    assert p.returncode == 5
    assert time.time() - t < 60
