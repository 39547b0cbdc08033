"""CPU: the user invariants' generated code, run state by state.

user_inv.cpp user_device_source lowers the compiled register program to C++
text that hipRTC compiles into every kernel a default run uses.  The text is
plain C++ over the kernels' headers, so here it is compiled for the host
(tests/fuzz/user_codegen_run.cpp, g++ -fsanitize=address,undefined, a
stand-alone program) and run on every state of the small configs of
tests/user_eval_cases.py, for every group of invariants and every TLCG_UTAB
setting: the interpreter, the generated code over the word (UVWord) and over
the component code (UVCode), and the outcome tables (code_consts_user +
user_eval_c) must agree on every state, and the interpreter must give the
Python oracle's recorded outcome (tests/golden/user_eval.json).

The runner is compiled once per (config, group, setting) -- the text differs
in each -- at -O0, about a second and a half each, several at a time; the two
large translation units (host_model.cpp, user_inv.cpp) are built once."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import user_eval_cases as U  # noqa: E402

CSRC = os.path.join(ROOT, "pulsar-tlaplus_amd", "csrc")
SRC = os.path.join(HERE, "fuzz", "user_codegen_run.cpp")
SAN = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
SETTINGS = ("unset", "0", "dyn", "slow")  # TLCG_UTAB
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")

# opcodes of user_inv.h no program can hold, with the reason
UNREACHABLE = {
    "U_BIT": "the compiler (user_inv.cpp) has no emit of it: only the interpreter and the code generator know it",
}


def header_opcodes():
    text = open(os.path.join(CSRC, "user_inv.h")).read()
    body = re.search(r"enum UOp : uint8_t \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return re.findall(r"\bU_[A-Z0-9]+\b", body)


def parse_run(text):
    lines = text.splitlines()
    head = dict(zip(lines[0].split()[1::2], map(int, lines[0].split()[2::2])))
    assert lines[0].startswith("@@RUN"), lines[0]
    n, ku = head["states"], head["n_user"]
    rows = lines[1:1 + n]
    assert len(rows) == n and all(len(r) == 4 * ku for r in rows)
    hist = {}
    for l in lines[1 + n:]:
        tag, k, op, cnt = l.split()
        assert tag == "H"
        hist.setdefault(int(k), {})[op] = int(cnt)
    # per invariant k and path a-d: one string over the states
    paths = [["".join(r[4 * k + p] for r in rows) for p in range(4)] for k in range(ku)]
    return head, paths, hist


def switch_values(text, fn):
    """{k: value} of a generated `switch (k)` function"""
    body = re.search(r"\b" + fn + r"\(int k\) \{\n  switch \(k\) \{\n(.*?)\n  \}", text, re.S).group(1)
    return {int(k): int(v) for k, v in re.findall(r"case (\d+): return (-?\d+)u?;", body)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    d = tmp_path_factory.mktemp("codegen")
    workers = max(1, min(8, os.cpu_count() or 1))
    pool = concurrent.futures.ThreadPoolExecutor(workers)

    def cc(args):
        subprocess.run(["g++"] + SAN + args, check=True, timeout=900)

    objs = [str(d / "host_model.o"), str(d / "user_inv.o")]
    list(pool.map(cc, [["-O1", "-c", os.path.join(CSRC, "host_model.cpp"), "-o", objs[0]],
                       ["-O1", "-c", os.path.join(CSRC, "user_inv.cpp"), "-o", objs[1]]]))
    base = str(d / "emit")
    cc(["-O0", SRC] + objs + ["-o", base])
    jobs, emitted = [], {}
    for cfg in U.CONFIGS:
        words = U.checked_words(cfg)
        for gi, names in enumerate(U.GROUPS):
            model = U.group_model(cfg, names)
            inp = str(d / f"{cfg}_{gi}.in")
            U.write_input(inp, model, words)
            r = subprocess.run([base, "emit", inp], capture_output=True, text=True, timeout=300, env=ENV)
            assert r.returncode == 0, r.stderr[-3000:]
            parts = re.split(r"^@@UTAB (\w+)\n", r.stdout, flags=re.M)
            texts = dict(zip(parts[1::2], parts[2::2]))
            assert tuple(texts) == SETTINGS
            for s, t in texts.items():
                gen = str(d / f"{cfg}_{gi}_{s}.inc")
                open(gen, "w").write(t)
                emitted[cfg, gi, s] = t
                jobs.append((cfg, gi, s, inp, gen, U.T.state_words(model) == 2))

    def build_and_run(job):
        cfg, gi, s, inp, gen, wide = job
        exe = gen[:-4]
        cc(["-O0", f'-DTLCG_GEN_SRC="{gen}"'] + (["-DTLCG_GEN_WIDE=1"] if wide else []) + [SRC] + objs + ["-o", exe])
        r = subprocess.run([exe, "run", inp], capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, (cfg, gi, s, r.stderr[-3000:])
        os.unlink(exe)
        return (cfg, gi, s), parse_run(r.stdout)

    out = dict(pool.map(build_and_run, jobs))
    pool.shutdown()
    return out, emitted


@pytest.mark.parametrize("cfg", list(U.CONFIGS))
def test_generated_code_agrees_with_the_interpreter_on_every_state(runs, cfg):
    """(a) = (b) = (c) = (d) for every state, invariant and TLCG_UTAB setting;
    a state without a component code has no (c) and (d)"""
    out, _ = runs
    bad = []
    for gi, names in enumerate(U.GROUPS):
        for s in SETTINGS:
            head, paths, _ = out[cfg, gi, s]
            assert head["generated"] == 1 and head["n_user"] == len(names)
            assert head["words"] == (2 if cfg == "wide" else 1)  # (wide: the u128 instantiations)
            for k, name in enumerate(names):
                a, b, c, d = paths[k]
                assert set(a) <= set("012")
                if a != b:
                    bad.append((gi, s, name, "UVWord"))
                for p, what in ((c, "UVCode"), (d, "tables")):
                    assert [i for i, ch in enumerate(p) if ch == "x"] == [i for i, ch in enumerate(c) if ch == "x"]
                    if any(x != y for x, y in zip(a, p) if y != "x"):
                        bad.append((gi, s, name, what))
    assert not bad, bad


@pytest.mark.parametrize("cfg", list(U.CONFIGS))
def test_interpreter_gives_the_oracle_outcomes(runs, cfg):
    out, _ = runs
    assert not U.golden()["oracle_refused"]
    for gi, names in enumerate(U.GROUPS):
        _, paths, _ = out[cfg, gi, "unset"]
        for k, name in enumerate(names):
            want = U.golden_outcomes(cfg, name)
            got = paths[k][0]
            diff = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
            assert len(got) == len(want) and not diff, (name, diff[:5])


def test_on_chip_configs_have_a_component_code_for_every_state(runs):
    """the four one-word configs without a Producer are the on-chip engines':
    every state has a code, so (c) and (d) ran on all of them"""
    out, _ = runs
    for cfg in U.ONE_WORD_CLOSED + ["wide"]:
        assert U.T.host_component_selfcheck(U.group_model(cfg, U.GROUPS[0]), 0, 32) > 0, cfg
        for gi in range(len(U.GROUPS)):
            for s in SETTINGS:
                head, paths, _ = out[cfg, gi, s]
                assert head["coded"] == 1 and not any("x" in p for k in paths for p in k), (cfg, gi, s)
    # (with a Producer `messages` grows, and most states have no code: those are the tree engine's)
    assert any("x" in paths[0][2] for paths in [out["P_N3C2", 0, "unset"][1]])


def test_programs_hold_every_opcode(runs):
    out, _ = runs
    ops = header_opcodes()
    assert len(ops) == 41 and ops[0] == "U_LDI" and ops[-1] == "U_RET"
    seen = set()
    for (_, _, s), (_, _, hist) in out.items():
        for h in hist.values():
            seen |= set(h)
    assert {"U_KIN:0", "U_KIN:1", "U_KAT:0", "U_KAT:1"} <= seen  # both sets
    plain = {o.partition(":")[0] for o in seen}
    assert plain <= set(ops)
    assert set(ops) - plain == set(UNREACHABLE), sorted(set(ops) - plain)
    # (the reason given for the unreachable ones: the compiler has no emit of them)
    src = open(os.path.join(CSRC, "user_inv.cpp")).read()
    for op in UNREACHABLE:
        assert not re.search(r"emit\(\s*" + op + r"\b", src), op


def test_every_kind_of_outcome_table_is_generated(runs):
    """by tlcg_user_tab_off / tlcg_user_tab_dyn of the emitted text: a
    host-made class table, a per-component table, and no table at all; and
    what each TLCG_UTAB setting changes"""
    _, emitted = runs
    kinds = set()
    for cfg in U.ONE_WORD_CLOSED:
        for gi, names in enumerate(U.GROUPS):
            t = emitted[cfg, gi, "unset"]
            off, dyn, mask = (switch_values(t, "tlcg_user_tab_" + f) for f in ("off", "dyn", "mask"))
            assert set(off) == set(dyn) == set(mask) == set(range(len(names)))
            for k in off:
                kinds.add("none" if off[k] < 0 else "dyn" if dyn[k] else "static")
                assert off[k] >= 0 or (mask[k] == 0 and not dyn[k])
                assert off[k] < 0 or 0 <= off[k] <= 62 and bin(mask[k]).count("1") <= 4
            if any(off[k] >= 0 and not dyn[k] for k in off):
                assert "kUTabStatic[" in t
            assert all(v < 0 for v in switch_values(emitted[cfg, gi, "0"], "tlcg_user_tab_off").values())
            o2, d2 = (switch_values(emitted[cfg, gi, "dyn"], "tlcg_user_tab_" + f) for f in ("off", "dyn"))
            assert o2 == off and all(d2[k] for k in o2 if o2[k] >= 0) and "kUTabStatic[" not in emitted[cfg, gi, "dyn"]
            o3, d3 = (switch_values(emitted[cfg, gi, "slow"], "tlcg_user_tab_" + f) for f in ("off", "dyn"))
            assert o3 == off and not any(d3.values()) and "kUTabStatic[" not in emitted[cfg, gi, "slow"]
    assert kinds == {"none", "dyn", "static"}
