"""CPU: the per-lane component kernel's owner table (csrc/component_code.h
lane_owner_word, host_model.cpp build_lane_phash): every entry field by field
against component 0's code set walked on its own
(tlcg_host_lane_owner_selfcheck) on the golden cfgs the pass takes and on the
seeded random cfgs, the first word of arbitrary codes against the bit layout
worked out here, refusal exactly when a field does not fit, and the kernel's
module built with each round-8 define off."""
import ctypes as C

import pytest

import tlcgpu
from conftest import GOLDEN, model_of
from test_gpu_random_cfgs import random_model

TAKEN = ["S", "V_leak", "V_dup", "S_noretain", "X_keys3_vals57", "R_C2_K2"]
DEFINES = ["TLCG_LANE_OWNER_RING", "TLCG_LANE_FP_REG", "TLCG_LANE_LEVEL_LDS", "TLCG_LANE_OWNER_RING=0;TLCG_LANE_FP_REG"]
G9 = dict(key_space=range(1, 16), value_space=range(1, 16))


def code_bits(m):
    C_, K = m.compaction_times_limit, m.max_crash_times
    return C_ + 7 + 2 * C_.bit_length() + K.bit_length()


def step_index(m, code):
    """ph | r << 3 | max ledger << 4 from the code's layout (component_code.h:
    ledgers in bits 0..C-1, R at C, H at C + 1, ph at C + 2..C + 4)"""
    C_ = m.compaction_times_limit
    led = code & ((1 << C_) - 1)
    return ((code >> (C_ + 2)) & 7) | (((code >> C_) & 1) << 3) | (led.bit_length() << 4)


@pytest.mark.parametrize("case", TAKEN)
def test_owner_table_of_golden_cfg(case):
    m = model_of(GOLDEN[case]["constants"])
    n, overflow = tlcgpu.host_lane_owner_selfcheck(m)
    assert not overflow and n > 0, (case, n, overflow)
    assert n <= 62
    # a component is its code set: |S| states each (the closed cfgs that run to the end)
    if GOLDEN[case]["result"]["result"] == "ok":
        assert GOLDEN[case]["result"]["distinct"] == n * tlcgpu.init_count(m), (case, n)


def test_s_has_62_codes():
    assert tlcgpu.host_lane_owner_selfcheck(tlcgpu.Model()) == (62, False)
    assert tlcgpu.host_lane_owner_selfcheck(tlcgpu.Model(**G9)) == (62, False)


@pytest.mark.parametrize("seed", range(40))
def test_owner_table_of_random_cfg(seed):
    m = random_model(seed)
    n, overflow = tlcgpu.host_lane_owner_selfcheck(m)
    if tlcgpu.check_model(m) is not None:
        assert n == -1
        return
    assert n >= 0, (seed, n)  # (< 0: an entry disagrees)
    in_domain = not m.model_producer and code_bits(m) <= 16
    if not in_domain:
        assert n == 0
    else:
        assert (n == 0) == overflow, (seed, n, overflow)  # refused exactly when a field does not fit


@pytest.mark.parametrize("name", ["S", "R_C2_K2", "C3_K2"])
def test_first_word_fields(name):
    """code + 1, a feature field of 9 bits with LF_ANY set, the step index and
    a clear bit 31 on codes across the whole range; 0 when code + 1 takes more
    than 16 bits (C = 3, K = 2: 16-bit codes)"""
    m = {"S": tlcgpu.Model(), "R_C2_K2": model_of(GOLDEN["R_C2_K2"]["constants"]),
         "C3_K2": tlcgpu.Model(max_crash_times=2)}[name]
    top = 1 << code_bits(m)
    for code in list(range(0, top, 37)) + list(range(top - 64, top)):
        w = tlcgpu.host_lane_owner_word(m, code)
        if code + 1 > 0xFFFF:
            assert w == 0, code
            continue
        assert w & 0xFFFF == code + 1, code
        assert (w >> 16) & 1 == 1 and w >> 31 == 0, code
        assert (w >> 25) & 63 == step_index(m, code), code
    if name == "C3_K2":
        assert top == 1 << 16 and tlcgpu.host_lane_owner_word(m, 0xFFFF) == 0


def test_refused_when_a_field_does_not_fit():
    """C = 3 with two crashes: component 0 has more than 62 codes, a dense
    index would not fit the 64-bit register; and the random draws do meet it"""
    assert tlcgpu.host_lane_owner_selfcheck(tlcgpu.Model(max_crash_times=2)) == (0, True)
    hit = [s for s in range(40) if tlcgpu.check_model(random_model(s)) is None
           and tlcgpu.host_lane_owner_selfcheck(random_model(s)) == (0, True)]
    assert hit, "no seeded cfg overflows a field"


def test_models_the_pass_does_not_take():
    assert tlcgpu.host_lane_owner_selfcheck(tlcgpu.Model(model_producer=True)) == (0, False)
    assert tlcgpu.host_lane_owner_selfcheck(tlcgpu.Model(compaction_times_limit=12)) == (0, False)


@pytest.mark.parametrize("define", DEFINES)
def test_g9_module_compiles_with_define_off(define, tmp_path, monkeypatch):
    monkeypatch.setenv("TLCG_JIT_CACHE", str(tmp_path / "jit"))
    monkeypatch.setenv("TLCG_JIT_DEFINES", define + "=0")
    m = tlcgpu.Model(**G9).to_c()
    err = C.create_string_buffer(4096)
    n = tlcgpu.load_library().tlcg_jit_selftest(C.byref(m), b"gfx950", err, 4096)
    assert n > 0, err.value.decode()[:2000]
