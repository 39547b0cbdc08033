"""CPU: the per-lane component kernel's table-borne predicates
(csrc/component_code.h lane_inv_feat / lane_inv_mask, compactor_step_entry's
stutter flag) against the evaluated invariants and stutter count, on every
component code and every class of component constants
(tlcg_host_lane_inv_selfcheck), and the kernel's module built both ways."""
import ctypes as C

import pytest

import tlcgpu
from conftest import GOLDEN, model_of

G9 = dict(key_space=range(1, 16), value_space=range(1, 16))


def golden_model(case, **over):
    c = dict(GOLDEN[case]["constants"])
    c.update(over)
    return model_of(c)


MODELS = {
    "S": lambda: tlcgpu.Model(),
    "G9": lambda: tlcgpu.Model(**G9),
    "S_leak_invariants": lambda: golden_model("S", invariants=GOLDEN["V_leak"]["constants"]["invariants"]),
    "S_dup_invariants": lambda: golden_model("S", invariants=GOLDEN["V_dup"]["constants"]["invariants"]),
    "S_noretain": lambda: tlcgpu.Model(retain_null_key=False),
    "R_C2_K2": lambda: golden_model("R_C2_K2"),
    "R_C1_K0": lambda: golden_model("R_C1_K0"),
    "S_consumer": lambda: golden_model("S", consumer=True),
    "S_nodeadlock": lambda: golden_model("S", deadlock=False),
}


def code_bits(m):
    C_, K = m.compaction_times_limit, m.max_crash_times
    return C_ + 7 + 2 * C_.bit_length() + K.bit_length()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_features_and_mask_are_the_invariants(name):
    """Contract A and the stutter flag on every (code, class) pair: len 0..N x
    the 32 flag combinations x every code below 2^code_bits"""
    m = MODELS[name]()
    n = tlcgpu.host_lane_inv_selfcheck(m)
    assert n == (m.msg_sent_limit + 1) * 32 * (1 << code_bits(m)), (name, n)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_component_selfcheck_unchanged(name):
    assert tlcgpu.host_component_selfcheck(MODELS[name](), 0, 300) > 0


def test_models_the_pass_does_not_take():
    assert tlcgpu.host_lane_inv_selfcheck(tlcgpu.Model(model_producer=True)) == 0
    assert tlcgpu.host_lane_inv_selfcheck(tlcgpu.Model(compaction_times_limit=12)) == 0


@pytest.mark.parametrize("defines", ["", "TLCG_LANE_INV_FEAT=0"])
def test_g9_module_compiles_both_ways(defines, tmp_path, monkeypatch):
    """the G9 module for gfx950 with the feature path (the default) and with
    check_invariants_cbt on each insert (the A/B define)"""
    monkeypatch.setenv("TLCG_JIT_CACHE", str(tmp_path / "jit"))
    if defines:
        monkeypatch.setenv("TLCG_JIT_DEFINES", defines)
    else:
        monkeypatch.delenv("TLCG_JIT_DEFINES", raising=False)
    m = tlcgpu.Model(**G9).to_c()
    err = C.create_string_buffer(4096)
    n = tlcgpu.load_library().tlcg_jit_selftest(C.byref(m), b"gfx950", err, 4096)
    assert n > 0, err.value.decode()[:2000]
