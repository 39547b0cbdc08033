"""CPU: the liveness pass's host-side lasso extraction under AddressSanitizer
and UBSan (tests/fuzz/lasso_fuzz.cpp, a stand-alone program over
csrc/liveness_graph.h built with g++ -fsanitize=address,undefined).  The
program peels seeded explicit graphs itself, calls lasso_walk through
ExplicitGraph's host side on the states left and verifies every lasso; the
spec's own G' is acyclic, so nothing else reaches this code without a GPU."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pulsar-tlaplus_amd", "csrc")


@pytest.fixture(scope="module")
def lasso_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("lasso") / "lasso_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(HERE, "fuzz", "lasso_fuzz.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_lasso_walk_under_sanitizers(lasso_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([lasso_bin, "3000", str(seed)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["graphs"] == 3000 and res["cyclic"] + res["acyclic"] == 3000
    assert res["cyclic"] >= 500 and res["acyclic"] >= 500
    # states after the cycles were among those left, and walks had to pass over them
    assert res["dead_states"] >= 100 and res["dead_skipped"] >= 20
    assert res["steps"] >= 2 * res["cyclic"]
