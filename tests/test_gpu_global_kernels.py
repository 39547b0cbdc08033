"""GPU: every expand kernel of the global HBM-FPSet engine, and each
grow-and-redo path of its host level loops, against the golden fixtures.

The whole-run parity tests reach this engine with its default kernel, on
levels of one chunk per block, and with tables and stores that never
overflow.  This module selects each kernel launch_expand (csrc/tlcgpu.hip)
can route a level to -- by TLCG_FAST_ITEMS / TLCG_PROBE / TLCG_JIT, by the
model (Producer, wide state, open partition) and by the order -- and runs it

  A. at ordinary sizes, also with TLCG_GRID=1 (one block, so the grid-stride
     loop takes many chunks and the LDS stage is flushed and reset between
     them);
  B. from a 256-slot FPSet of fixed size (log2_fpset_slots=8 switches the
     proactive ensure_fpset off), so that every growth of the table comes
     from a kernel's own "probe limit reached -> OVF_FPSET" branch and the
     host loop's grow-and-redo (run_init, step_level, tlcg_expand, the
     absorb);
  C. with the first attempt of every level given room for 64 new states
     (the TLCG_STORE_ROOM test hook), so that the kernel's "stage does not
     fit -> OVF_STORE" branch and the redo behind it run.

That a path ran is proved by counting, not by the kernels' word: the final
table holds every stored state and a redo at most doubles it (B); a level's
first attempt overflows exactly when the level holds more new states than
the room (C: the blocks claim their ranges from one counter, so the last
claim ends at the level's size)."""
import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_parity import check_against_golden
from test_gpu_user_inv import GOLD as USER_GOLD, check_path, model as user_model

pytestmark = pytest.mark.gpu

ENV = ("TLCG_FAST_ITEMS", "TLCG_PROBE", "TLCG_GRID", "TLCG_JIT", "TLCG_STORE_ROOM")

# (TLCG_FAST_ITEMS, TLCG_PROBE) -> the kernel a one-word level without a
# Producer takes in fast order on one rank, precompiled (TLCG_JIT=0)
PRECOMPILED = {
    "items0": dict(TLCG_FAST_ITEMS="0"),  # the generic k_expand<u64,false,false,false>
    "items1_load": dict(TLCG_FAST_ITEMS="1", TLCG_PROBE="0"),  # k_expand_fast<1,0>
    "items1_cas": dict(TLCG_FAST_ITEMS="1", TLCG_PROBE="1"),  # k_expand_fast<1,1>
    "items2_load": dict(TLCG_FAST_ITEMS="2", TLCG_PROBE="0"),  # k_expand_fast<2,0> (the default)
    "items2_cas": dict(TLCG_FAST_ITEMS="2", TLCG_PROBE="1"),  # k_expand_fast<2,1>
    "items4_load": dict(TLCG_FAST_ITEMS="4", TLCG_PROBE="0"),  # k_expand_fast<4,0>
    "items4_cas": dict(TLCG_FAST_ITEMS="4", TLCG_PROBE="1"),  # k_expand_fast<4,1>
}
for _v in PRECOMPILED.values():
    _v["TLCG_JIT"] = "0"
# the hipRTC-specialized tlcg_expand_fast_2 / tlcg_expand_fast_2c (jit.cpp; jit_used bit 6)
JIT_LOAD = dict(TLCG_JIT="1")
JIT_CAS = dict(TLCG_JIT="1", TLCG_PROBE="1")
GRID1_FAST = dict(PRECOMPILED["items2_load"], TLCG_GRID="1")
GRID1_GENERIC = dict(PRECOMPILED["items0"], TLCG_GRID="1")
GRID1_DEFAULT = dict(TLCG_JIT="0", TLCG_GRID="1")


def variants(*names):
    return [pytest.param(PRECOMPILED[n], id=n) for n in names]


def set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def least_redos(distinct):
    """ceil(log2(distinct / 256)): a 256-slot table holds `distinct` states
    only after this many doublings, and a redo doubles it at most once"""
    k = 0
    while (256 << k) < distinct:
        k += 1
    return k


def stored(want):
    return want["distinct"] if want["result"] == "ok" else want["eol_distinct"]


def check(case, monkeypatch, env, tlc=False, redos=None, **opts):
    """One global-engine check of golden `case` under `env`, compared with the
    fixture (check_against_golden); in TLC order also TLC's stop counters
    (error cases) or its outdegree histogram (ok cases).  `redos`: a function
    of the fixture's result giving (lower bound, exact or None) for
    levels_redone.  Returns the result."""
    set_env(monkeypatch, env)  # (tlcg_create reads the variant)
    want = GOLDEN[case]["result"]
    ok = want["result"] == "ok"
    ck = tlcgpu.Checker(model_of(GOLDEN[case]["constants"]), tlc_order=tlc, engine="global", outdegree=tlc and ok,
                        **opts)
    try:
        r = ck.run()
        assert r.engine == "global"
        assert bool(r.jit_used & 64) == (env.get("TLCG_JIT") == "1" and env.get("TLCG_FAST_ITEMS", "2") == "2"
                                         and not tlc), r.jit_used
        check_against_golden(case, r, tlc)
        if tlc and ok:
            assert ck.outdegree() == want["outdegree"], case
        elif tlc:
            assert r.tlc_exact
            assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"]), case
        if redos is not None:
            least, exact = redos(want)
            print(f"{case}: levels_redone {r.levels_redone}, at least {least}, exactly {exact}")
            assert r.levels_redone >= least, (case, r.levels_redone, least)
            assert exact is None or r.levels_redone == exact, (case, r.levels_redone, exact)
        else:
            assert r.levels_redone == 0, (case, r.levels_redone)
        return r
    finally:
        ck.close()


def check_node(case, monkeypatch, env, redos=None, **opts):
    """the same on an open partition: 2 ranks on the one GPU, the whole state
    as the partition key; counts, levels, verdict and depth as
    test_run_node_pipelined_level_overflows compares them"""
    set_env(monkeypatch, env)
    want = GOLDEN[case]["result"]
    r = tlcgpu.run_node(model_of(GOLDEN[case]["constants"]), 2, partition=2, engine="global", **opts)
    assert r.engine == "global" and r.status == want["result"]
    if want["result"] == "ok":
        assert (r.generated, r.distinct, r.depth, r.levels) == (want["generated"], want["distinct"], want["depth"],
                                                                 want["levels"])
    else:
        assert (r.invariant, r.depth) == (want["invariant"], want["depth"])
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
    if redos is not None:
        least, _ = redos(want)
        print(f"{case} at 2 ranks: levels_redone {r.levels_redone}, at least {least}")
        assert r.levels_redone >= least, (case, r.levels_redone, least)
    return r


# ---- A. every variant at ordinary sizes ----

ONE_WORD = ["S", "S_consumer", "S_noretain", "X_keys3_vals57", "X_C5_K2", "R_C6_K3", "V_leak", "V_dup", "D_N0_K1"]
PRODUCER = ["P_published", "V_leak_producer", "X_producer_sparse"]
WIDE = ["W_C12_k1", "W_C12_leak"]


@pytest.mark.parametrize("env", variants("items0", "items1_load", "items1_cas", "items2_cas", "items4_load",
                                         "items4_cas"))
@pytest.mark.parametrize("case", ONE_WORD)
def test_one_word_kernel_variants(case, env, monkeypatch):
    """fast order, one rank, a one-word state without a Producer: the generic
    k_expand<u64,false,false,false> (TLCG_FAST_ITEMS=0) and the precompiled
    k_expand_fast<1,0>, <1,1>, <2,1>, <4,0>, <4,1> (items, probe; <2,0> is
    the default every other test runs)"""
    check(case, monkeypatch, env)


@pytest.mark.parametrize("case", ["S", "S_consumer", "S_noretain"])
def test_specialized_cas_first_kernel(case, monkeypatch):
    """TLCG_JIT=1 with TLCG_PROBE=1: the hipRTC tlcg_expand_fast_2c
    (expand_fast_body<2,1> with the layout a constant; jit_used bit 6, which
    check() asserts)"""
    r = check(case, monkeypatch, JIT_CAS)
    assert r.jit_used & 64


@pytest.mark.parametrize("env", [pytest.param(GRID1_FAST, id="items2_load"), pytest.param(GRID1_GENERIC, id="items0")])
@pytest.mark.parametrize("case", ONE_WORD)
def test_one_word_single_block(case, env, monkeypatch):
    """TLCG_GRID=1: one block walks the whole frontier, 512 parents a chunk in
    k_expand_fast<2,0> (its stage flushed and reset after every chunk) and
    1024 in the generic k_expand (reserve() flushes when the stage could
    fill)"""
    check(case, monkeypatch, env)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
@pytest.mark.parametrize("case", PRODUCER)
def test_producer_generic_kernel(case, tlc, monkeypatch):
    """TLCG_FAST_ITEMS=0 with a modelled Producer: the generic
    k_expand<u64,true,false,false>, and k_expand<u64,true,true,false> in TLC
    order (the default is k_expand_prod / k_expand_prod_spread)"""
    check(case, monkeypatch, PRECOMPILED["items0"], tlc=tlc)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
@pytest.mark.parametrize("case", PRODUCER)
def test_producer_single_block(case, tlc, monkeypatch):
    """TLCG_GRID=1 with the default items: one block of k_expand_prod<8,false>
    takes the frontier 512 parents at a time, and in TLC order one block of
    k_expand_prod_spread<8,true> 256 (parent, chunk) pairs at a time (every
    frontier here is below its 2^20 threshold)"""
    check(case, monkeypatch, GRID1_DEFAULT, tlc=tlc)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
@pytest.mark.parametrize("case", WIDE)
def test_wide_single_block(case, tlc, monkeypatch):
    """a two-word state, TLCG_GRID=1: one block of k_expand<u128,false,false,
    false> (fast order) or k_expand<u128,false,true,false> (TLC order), the
    only kernels a wide level has"""
    check(case, monkeypatch, GRID1_DEFAULT, tlc=tlc)


@pytest.mark.parametrize("items", ["0", "1", "4"])
@pytest.mark.parametrize("case", ["S", "V_leak"])
def test_open_partition_kernel_variants(case, items, monkeypatch):
    """2 ranks, the whole state as the partition key: TLCG_FAST_ITEMS=0 takes
    k_expand<u64,false,false,true> (and the two-step level), 1 and 4 take
    k_expand_fast_part<1> and <4>, from tlcg_expand for the first level and
    from the pipelined ctx_absorb_expand after it (<2> is the default)"""
    check_node(case, monkeypatch, dict(TLCG_JIT="0", TLCG_FAST_ITEMS=items))


# ---- B. FPSet overflow -> grow -> redo ----

def fpset_redos(want):
    return least_redos(stored(want)), None


@pytest.mark.parametrize("env", variants("items0", "items1_load", "items2_load", "items2_cas", "items4_load")
                         + [pytest.param(JIT_LOAD, id="jit")])
def test_fpset_overflow_fast_kernels(env, monkeypatch):
    """S from 256 slots, fast order: the 729 initial states overflow
    k_init_direct<u64> (run_init's loop), then the levels overflow the
    OVF_FPSET branch of the generic k_expand, of k_expand_fast<1,0>, <2,0>,
    <2,1>, <4,0> and of the hipRTC tlcg_expand_fast_2, and step_level grows
    the table and redoes the level"""
    check("S", monkeypatch, env, redos=fpset_redos, log2_fpset_slots=8)


def test_fpset_overflow_tlc_order(monkeypatch):
    """S from 256 slots in TLC order: k_expand<u64,false,true,false>'s
    overflow; every redo reallocates and resets d_dkey_slot (rebuild_fpset),
    and the outdegree histogram of the sorted levels is the fixture's"""
    check("S", monkeypatch, PRECOMPILED["items2_load"], tlc=True, redos=fpset_redos, log2_fpset_slots=8)


@pytest.mark.parametrize("case,tlc", [("W_C12", False), ("W_C12_k1", False), ("W_C12_k1", True)])
def test_fpset_overflow_wide(case, tlc, monkeypatch):
    """two-word states from 256 slots: W_C12's 729 initial states overflow
    k_init_direct<u128>; the levels overflow the wide k_expand<u128,...> in
    both orders, and the table is rebuilt by the wide k_reinsert<u128>"""
    check(case, monkeypatch, dict(TLCG_JIT="0"), tlc=tlc, redos=fpset_redos, log2_fpset_slots=8)


@pytest.mark.parametrize("case,tlc", [("V_leak", False), ("V_leak", True), ("V_dup", False), ("V_dup", True),
                                      ("W_C12_leak", True), ("W_C12_dup", True),
                                      ("V_leak_producer", False), ("V_leak_producer", True),
                                      ("V_dup_producer", False), ("V_dup_producer", True)])
def test_fpset_overflow_on_the_error_path(case, tlc, monkeypatch):
    """error cases from 256 slots: the levels up to and including the one
    that holds the error are redone (its level is the largest so far, and the
    table must hold all of it); in TLC order the trace is TLC's, state by
    state, and tlcg_tlc_stop_stats its counters.  Producer cases:
    k_expand_prod<8,false> in fast order, k_expand_prod_spread<8,true> in TLC
    order"""
    check(case, monkeypatch, dict(TLCG_JIT="0"), tlc=tlc, redos=fpset_redos, log2_fpset_slots=8)


@pytest.mark.parametrize("case", ["X_producer_sparse", "P_published"])
def test_fpset_overflow_producer_tlc_order_outdegree(case, monkeypatch):
    """k_expand_prod_spread<8,true> from 256 slots: its overflow, the redo
    with a fresh d_dkey_slot, and tlcg_outdegree over the redone levels"""
    check(case, monkeypatch, dict(TLCG_JIT="0"), tlc=True, redos=fpset_redos, log2_fpset_slots=8)


@pytest.mark.parametrize("case", ["S", "X_producer_sparse"])
def test_fpset_overflow_open_partition(case, monkeypatch):
    """2 ranks, 256 slots each.  S: each rank's about 364 initial states
    overflow k_init_part<u64>, then k_expand_fast_part<2> and k_absorb.
    X_producer_sparse: the generic k_expand<u64,true,false,true> (PART with a
    Producer).  levels_redone is the ranks' sum: the rank with the larger
    share stores at least half the states (least_redos - 1 doublings) and the
    other more than 256 (one more)"""
    check_node(case, monkeypatch, dict(TLCG_JIT="0"), redos=fpset_redos, log2_fpset_slots=8)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
@pytest.mark.parametrize("case", ["U_LedgerCount", "U_all_hold"])
def test_fpset_overflow_then_user_check(case, tlc, monkeypatch):
    """user invariants (tests/golden/user_inv.json) from 256 slots: the
    level's user_check_level runs on the redone level (k_user_check with
    TLCG_JIT=0); the assertions of test_user_invariant_check"""
    set_env(monkeypatch, dict(TLCG_JIT="0"))
    m = user_model(case)
    want = USER_GOLD[case]["result"]
    ck = tlcgpu.Checker(m, tlc_order=tlc, engine="global", log2_fpset_slots=8)
    try:
        r = ck.run()
        assert r.engine == "global"
        assert r.status == want["result"], (case, r.status)
        assert r.levels_redone >= least_redos(stored(want)), (case, r.levels_redone)
        if want["result"] == "ok":
            assert (r.generated, r.distinct, r.depth, r.levels) == (want["generated"], want["distinct"],
                                                                     want["depth"], want["levels"])
            return
        assert r.depth == want["depth"]
        assert (r.generated, r.distinct) == (want["eol_generated"], want["eol_distinct"])
        assert r.invariant == want["invariant"]
        if tlc:
            assert [a for a, _ in r.trace] == [t["action"] for t in want["trace"]]
            assert [tlcgpu.decode(m, s) for _, s in r.trace] == [t["state"] for t in want["trace"]]
            assert ck.tlc_stop_stats() == (want["generated"], want["distinct"], want["left_on_queue"])
        else:
            check_path(m, r, want)
    finally:
        ck.close()


def test_fpset_overflow_then_rerun(monkeypatch):
    """a context whose table grew checks again: identical counts and levels
    (the second run starts from the grown table)"""
    set_env(monkeypatch, dict(TLCG_JIT="0"))
    ck = tlcgpu.Checker(model_of(GOLDEN["S"]["constants"]), engine="global", log2_fpset_slots=8)
    try:
        a = ck.run()
        check_against_golden("S", a, False)
        assert a.levels_redone >= least_redos(a.distinct)
        b = ck.run()
        assert (b.status, b.generated, b.distinct, b.depth, b.levels) == (a.status, a.generated, a.distinct, a.depth,
                                                                        a.levels)
    finally:
        ck.close()


# ---- C. store overflow -> redo, through TLCG_STORE_ROOM ----

ROOM = 64


def store_redos(want):
    """a level's first attempt overflows exactly when it holds more than ROOM
    new states (level 0 is run_init's, which the hook leaves alone); an error
    run stops at some level, so there only a lower bound"""
    if want["result"] == "ok":
        n = sum(1 for x in want["levels"][1:] if x > ROOM)
        return n, n
    return 1, None


def with_room(env):
    return dict(env, TLCG_STORE_ROOM=str(ROOM))


@pytest.mark.parametrize("env", variants("items0", "items1_load", "items2_load", "items4_cas")
                         + [pytest.param(JIT_LOAD, id="jit")])
def test_store_overflow_fast_kernels(env, monkeypatch):
    """S in fast order, 64 states of room on each level's first attempt: the
    OVF_STORE branch of the generic k_expand's flush, of k_expand_fast<1,0>,
    <2,0>, <4,1> and of the hipRTC tlcg_expand_fast_2; the redo has the real
    room.  2^20 slots: no FPSet overflow mixes in"""
    check("S", monkeypatch, with_room(env), redos=store_redos, log2_fpset_slots=20)


@pytest.mark.parametrize("case", ["S", "V_leak"])
def test_store_overflow_tlc_order(case, monkeypatch):
    """TLC order: k_expand<u64,false,true,false>'s store overflow (the level
    is not sorted, step_level redoes it with d_dkey_slot reset); the outdegree
    histogram (S), the trace and TLC's stop counters (V_leak) are the
    fixture's"""
    check(case, monkeypatch, with_room(dict(TLCG_JIT="0")), tlc=True, redos=store_redos, log2_fpset_slots=20)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
@pytest.mark.parametrize("case", ["X_producer_sparse", "V_leak_producer", "W_C12_k1", "W_C12_leak"])
def test_store_overflow_producer_and_wide(case, tlc, monkeypatch):
    """the store overflow of k_expand_prod<8,false> (fast order) and
    k_expand_prod_spread<8,true> (TLC order) with a Producer, and of the wide
    k_expand<u128,false,*,false>"""
    check(case, monkeypatch, with_room(dict(TLCG_JIT="0")), tlc=tlc, redos=store_redos, log2_fpset_slots=20)


@pytest.mark.parametrize("items", ["0", "2"])
def test_store_overflow_open_partition(items, monkeypatch):
    """2 ranks, the two-step level (TLCG_PIPELINE=0: every level's expand is
    tlcg_expand's, where the hook also applies): the store overflow of
    k_expand<u64,false,false,true>'s PART flush (TLCG_FAST_ITEMS=0) and of
    k_expand_fast_part<2>, and tlcg_expand's redo.  Level 1 has 1458 states,
    so one rank finds more than 64 of them new"""
    monkeypatch.setenv("TLCG_PIPELINE", "0")
    check_node("S", monkeypatch, with_room(dict(TLCG_JIT="0", TLCG_FAST_ITEMS=items)), redos=lambda want: (1, None),
               log2_fpset_slots=20)


@pytest.mark.parametrize("tlc", [False, True], ids=["fast", "tlc_order"])
def test_fpset_and_store_overflow_together(tlc, monkeypatch):
    """S from 256 slots with 64 states of room: both flags rise in one
    attempt, and the redo grows both.  Every level above 64 new states is
    redone at least once, and the table doubles often enough"""
    def redos(want):
        return max(store_redos(want)[0], least_redos(stored(want))), None
    check("S", monkeypatch, with_room(dict(TLCG_JIT="0")), tlc=tlc, redos=redos, log2_fpset_slots=8)
