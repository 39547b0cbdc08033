"""CPU: the capacity-edge table of tests/capacity_cases.py against the host
model (tlcgpu.host_successors) and the C oracle run live, so the cfgs next to
each rung of the on-chip engines keep sitting where the table says:
each row's component size, depth and widest level, its code bits and local
key, the oracle's counts, the error variants' verdicts, and a row on either
side of every rung."""
import pytest

import tlcgpu
from capacity_cases import (CLOSED_COMPONENTS, CLOSED_ROWS, CLOSED_RUNGS, DUP_DEPTH, LEAK_HOLDS, LEAK_ROWS,
                            PRODUCER_ROWS, PRODUCER_RUNGS, WORLDS, closed_model, closed_row, closure_levels,
                            constants_of, expected_engine, producer_layers, producer_model, producer_row)
from conftest import run_oracle
from test_gpu_parity import code_bits, component_key_fits
from test_gpu_tree import tree_applies

CLOSED_IDS = [f"C{r.C}_K{r.K}" for r in CLOSED_ROWS]
PRODUCER_IDS = [f"N{r.N}_C{r.C}_K{r.K}" for r in PRODUCER_ROWS]


@pytest.mark.parametrize("row", CLOSED_ROWS, ids=CLOSED_IDS)
def test_closed_row_sits_where_the_table_says(row):
    m = closed_model(row.C, row.K)
    assert tlcgpu.check_model(m) is None
    assert tlcgpu.init_count(m) == CLOSED_COMPONENTS and tlcgpu.state_words(m) == 1
    # the first and the last component (a null key and value; the largest of each)
    for ci in (0, CLOSED_COMPONENTS - 1):
        lv = closure_levels(m, tlcgpu.host_init_state(m, ci))
        assert (sum(map(len, lv)), len(lv), max(map(len, lv))) == (row.size, row.depth, row.width), ci
    c = constants_of(m)
    assert tlcgpu.state_bits(m) <= 63
    assert code_bits(c) == row.code_bits
    assert component_key_fits(c) == row.key_fits
    want = run_oracle(m)
    assert want["result"] == "ok"
    assert (want["distinct"], want["depth"]) == (CLOSED_COMPONENTS * row.size, row.depth)
    assert want["levels"][0] == CLOSED_COMPONENTS and len(want["levels"]) == row.depth
    assert max(want["levels"]) == CLOSED_COMPONENTS * row.width  # (isomorphic components: equal levels)


@pytest.mark.parametrize("n", sorted(WORLDS))
@pytest.mark.parametrize("ck", [(7, 2), (2, 2)])
def test_world_sizes(ck, n):
    """the same component at 1, 64 and 65 components"""
    keys, values = WORLDS[n]
    m = closed_model(*ck, keys=keys, values=values)
    assert tlcgpu.check_model(m) is None
    assert tlcgpu.init_count(m) == n
    row = closed_row(*ck)
    want = run_oracle(m)
    assert (want["result"], want["distinct"], want["depth"]) == ("ok", n * row.size, row.depth)
    c = constants_of(m)
    assert component_key_fits(c) and code_bits(c) == row.code_bits
    assert expected_engine(m, row.size, row.depth) == expected_engine(closed_model(*ck), row.size, row.depth)


@pytest.mark.parametrize("ck", sorted(LEAK_ROWS) + LEAK_HOLDS)
def test_error_variants_are_violations(ck):
    """CompactedLedgerLeak at depth 9 or 12 and DuplicateNullKeyMessage at
    depth 4, in components that later outgrow their pass; on (8, 0) the leak
    invariant holds"""
    leak = run_oracle(closed_model(*ck, "CompactedLedgerLeak"))
    if ck in LEAK_HOLDS:
        assert (leak["result"], leak["depth"]) == ("ok", closed_row(*ck).depth)
    else:
        assert (leak["result"], leak["invariant"], leak["depth"]) == ("invariant", "CompactedLedgerLeak",
                                                                      LEAK_ROWS[ck])
    dup = run_oracle(closed_model(*ck, "DuplicateNullKeyMessage"))
    assert (dup["result"], dup["invariant"], dup["depth"]) == ("invariant", "DuplicateNullKeyMessage", DUP_DEPTH)
    # the error comes before the component outgrows anything: fewer states by then than the first pass holds
    assert dup["eol_distinct"] // CLOSED_COMPONENTS < 32
    # every component violates the leak invariant, and holds at most 72 states at the end of that level;
    # a component without a NullKey message holds DuplicateNullKeyMessage, so it runs out to its full size
    last = ["-init-lo", str(CLOSED_COMPONENTS - 1), "-init-hi", str(CLOSED_COMPONENTS), "-notrace"]
    if ck not in LEAK_HOLDS:
        assert leak["eol_distinct"] % CLOSED_COMPONENTS == 0 and leak["eol_distinct"] // CLOSED_COMPONENTS <= 72
        one = run_oracle(closed_model(*ck, "CompactedLedgerLeak"), last)
        assert (one["result"], one["depth"]) == ("invariant", LEAK_ROWS[ck])
        assert one["eol_distinct"] * CLOSED_COMPONENTS == leak["eol_distinct"]
    one = run_oracle(closed_model(*ck, "DuplicateNullKeyMessage"), last)
    assert (one["result"], one["distinct"], one["depth"]) == ("ok", closed_row(*ck).size, closed_row(*ck).depth)


@pytest.mark.parametrize("row", PRODUCER_ROWS, ids=PRODUCER_IDS)
def test_producer_row_sits_where_the_table_says(row):
    m = producer_model(row.N, row.C, row.K)
    assert tlcgpu.check_model(m) is None
    assert tlcgpu.init_count(m) == 1 and tlcgpu.state_words(m) == 1
    layers = producer_layers(m)
    nkv = 4  # (key, value) pairs of a message: {NullKey, 1} x {NullValue, 1}
    assert [len(x) for x in layers] == [nkv ** l for l in range(row.N + 1)]
    assert (min(layers[-1]), max(layers[-1])) == (row.last_min, row.last_max)
    assert max(max(x) for x in layers) == row.last_max  # the largest components are in the last layer
    want = run_oracle(m)
    assert want["result"] == "ok" and want["distinct"] == sum(map(sum, layers))


def test_every_rung_has_a_row_on_either_side():
    limit = {"32 states": ("size", 32), "64 states": ("size", 64), "128 states": ("size", 128),
             "255 states": ("size", 255), "48 levels": ("depth", 47), "640 slots": ("size", 640),
             "2048 slots": ("size", 2048), "16 code bits": ("code_bits", 16), "31 code bits": ("code_bits", 31)}
    assert sorted(limit) == sorted(CLOSED_RUNGS)
    for rung, (under, over) in CLOSED_RUNGS.items():
        field, bound = limit[rung]
        assert under and over
        assert all(getattr(closed_row(*ck), field) <= bound for ck in under), rung
        assert all(getattr(closed_row(*ck), field) > bound for ck in over), rung
    # the rows under 48 levels also fit 255 states, so depth alone decides; (8, 0) is over on depth alone
    assert all(closed_row(*ck).size <= 255 for ck in CLOSED_RUNGS["48 levels"][0])
    assert closed_row(8, 0).size <= 64  # (it fits the first pass's capacity)
    # the rows on the two sides of 255 states, 48 levels, 2048 slots and 31 code bits end in different engines
    for rung, (a, b) in (("255 states", ("component", "tree")), ("48 levels", ("component", "tree")),
                         ("2048 slots", ("tree", "global")), ("31 code bits", ("tree", "global"))):
        under, over = CLOSED_RUNGS[rung]
        for cks, eng in ((under, a), (over, b)):
            for ck in cks:
                r = closed_row(*ck)
                assert expected_engine(closed_model(*ck), r.size, r.depth) == eng, (rung, ck)
    bound = {"384 slots": 384, "1024 slots": 1024}
    for rung, (under, over) in PRODUCER_RUNGS.items():
        assert under and over
        assert all(producer_row(*k).last_max <= bound[rung] for k in under), rung
        assert all(producer_row(*k).last_max > bound[rung] for k in over), rung


def test_producer_expected_engines():
    """The Producer tree keeps 31-bit local keys.  (3, 4, 1) has 33 (a 41-bit
    state above 8 bits of `messages`), so the global engine takes it whatever
    its sizes; the other rows under 1024 end in the tree, those over it in the
    global engine."""
    got = {(r.N, r.C, r.K): expected_engine(producer_model(r.N, r.C, r.K), r.last_max, 0) for r in PRODUCER_ROWS}
    assert got == {(3, 3, 1): "tree", (3, 4, 1): "global", (3, 3, 2): "tree", (2, 4, 2): "tree",
                   (2, 4, 3): "global", (3, 3, 3): "global"}
    assert not tree_applies(producer_model(3, 4, 1))
    # either side of both Producer rungs still has a row the tree takes
    assert got[(3, 3, 1)] == got[(3, 3, 2)] == got[(2, 4, 2)] == "tree"
