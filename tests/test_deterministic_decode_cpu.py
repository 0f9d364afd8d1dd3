"""Deterministic decode mode, host side: the ordered entry points are declared and bound, and a generation call's mode follows
torch's global flag unless the call overrides it."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERED = ("ug_gemv_bf16_ord", "ug_skinny_finish_ord", "ug_decode_gemv_resid_norm_ord", "ug_attn_decode_fused_ord",
           "ug_decode_sw_kblock_ord", "ug_decode_finish_resid_norm_ord")


def test_ordered_entry_points_are_declared_and_bound():
    from unigen_hip import lib
    header = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    for name in ORDERED:
        assert name in lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert lib.ABI_VERSION == 7
    if os.path.exists(lib.LIB_PATH):
        L = lib.load()
        for name in ORDERED:
            assert callable(getattr(L, name)), name


def test_ordered_entry_points_refuse_empty_arguments():
    from unigen_hip import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    L = lib.load()
    for name in ORDERED:
        args = [0.0 if t is lib.F32 else 0 for t in lib.SIGNATURES[name]]
        assert getattr(L, name)(*args) != 0, name
        assert L.ug_last_error().decode().startswith(name), name


def test_mode_follows_the_torch_flag_unless_overridden():
    from unigen_hip.qwen2 import resolve_deterministic
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert resolve_deterministic(None) is False
        assert resolve_deterministic(True) is True
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert resolve_deterministic(None) is True
        assert resolve_deterministic(False) is False
    finally:
        torch.use_deterministic_algorithms(was)


def test_decode_state_carries_the_mode():
    from unigen_hip.qwen2 import DecodeState, Qwen2Dims
    d = Qwen2Dims(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1)
    assert DecodeState(d, 2, 8, torch.device("cpu")).deterministic is False
    assert DecodeState(d, 2, 8, torch.device("cpu"), deterministic=True).deterministic is True
