"""Host side of the shared-prefix generation calls, no GPU: the argument checks of mmu_generate_batch(prefix=...) / mmu_generate(prefix=...)
raise before anything touches a device (driven with a stub engine), and the new entry point is in the header, the binding's table and
the library's exports under the unchanged ABI version."""
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ug_attn_prefill_cached"


class _Untouchable:
    """stands where device state would: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the argument checks reached the device state (.{name})")


def _model(device="cpu"):
    """a UniGen with nothing but `llm.engine` (a stub: a device and no kernels) and a prefix object bound to it"""
    from models.unigen import MmuPrefix, UniGen
    model = object.__new__(UniGen)
    engine = types.SimpleNamespace(device=torch.device(device))
    model.__dict__["llm"] = types.SimpleNamespace(engine=engine, model=_Untouchable())
    prefix = MmuPrefix(model, _Untouchable(), 20, None, None)
    return model, prefix


def _calls(model):
    return [lambda **kw: model.mmu_generate_batch(**kw), lambda **kw: model.mmu_generate(**kw)]


def test_prefix_of_another_model_or_device_is_refused():
    from unigen_hip.lib import UniGenHipError
    model, prefix = _model()
    other, other_prefix = _model()
    tails = torch.zeros((2, 5), dtype=torch.long)
    for call in _calls(model):
        with pytest.raises(UniGenHipError, match="another model"):
            call(idx=tails[:1], prefix=other_prefix)
        with pytest.raises(UniGenHipError, match="mmu_prefix returns"):
            call(idx=tails[:1], prefix=object())
    far, far_prefix = _model("cuda:0")                       # (a device only by name: nothing is allocated on it)
    for call in _calls(far):
        with pytest.raises(UniGenHipError, match="another device"):
            call(idx=tails[:1], prefix=far_prefix)


def test_rows_masks_and_pads_are_checked_before_any_launch():
    from unigen_hip.lib import UniGenHipError
    model, prefix = _model()
    with pytest.raises(UniGenHipError, match="33 rows"):
        model.mmu_generate_batch(idx=torch.zeros((33, 4), dtype=torch.long), prefix=prefix)
    with pytest.raises(UniGenHipError, match="33 rows"):
        model.mmu_generate_batch(input_embeddings=torch.zeros((33, 4, 8)), prefix=prefix)
    tails = torch.zeros((3, 4), dtype=torch.long)
    dense = torch.zeros((3, 1, 24, 24))
    for call in _calls(model):
        with pytest.raises(UniGenHipError, match="dense attention_mask"):
            call(idx=tails[:1], attention_mask=dense[:1], prefix=prefix)
        with pytest.raises(UniGenHipError, match="idx .* or input_embeddings"):
            call(prefix=prefix)
    with pytest.raises(UniGenHipError, match="one row per call"):
        model.mmu_generate(idx=tails, prefix=prefix)
    with pytest.raises(UniGenHipError, match="cached form"):
        model.mmu_generate(idx=tails[:1], prefix=prefix, use_cache=False)
    tv = torch.tensor([[0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=torch.bool)
    with pytest.raises(UniGenHipError, match="pad in every row"):
        model.mmu_generate_batch(idx=tails, prefix=prefix, tail_valid=tv)
    with pytest.raises(UniGenHipError, match=r"tail_valid must be \[3, 4\]"):
        model.mmu_generate_batch(idx=tails, prefix=prefix, tail_valid=tv[:, :3])
    with pytest.raises(UniGenHipError, match="belongs to a call with a prefix"):
        model.mmu_generate_batch(idx=tails, attention_mask=dense, tail_valid=tv)


def test_checked_call_returns_rows_length_and_validity():
    from models.unigen import check_mmu_prefix_call
    model, prefix = _model()
    tv = torch.tensor([[1, 1, 1], [0, 0, 1]])
    R, S, got = check_mmu_prefix_call("t", model.llm.engine, prefix, torch.zeros((2, 3), dtype=torch.long), None, None, tv)
    assert (R, S) == (2, 3) and got.dtype == torch.bool and got.tolist() == [[True, True, True], [False, False, True]]
    R, S, got = check_mmu_prefix_call("t", model.llm.engine, prefix, None, torch.zeros((32, 1, 8)), None, None)
    assert (R, S, got) == (32, 1, None)


def _loaded():
    from unigen_hip import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return lib


def test_entry_point_is_in_header_binding_and_exports():
    lib = _loaded()
    with open(os.path.join(ROOT, "include", "unigen_hip.h")) as f:
        header = f.read()
    proto = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing from include/unigen_hip.h"
    params = [p for p in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if p.strip()]
    assert NAME in lib.SIGNATURES and len(lib.SIGNATURES[NAME]) == len(params) == 16
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NAME + r"\b", exported), "symbol missing from the library's exports"
    assert "FINITE" in header[header.index("Prefill onto a filled cache"):proto.start()]          # the contract on staged tiles is stated


def test_abi_version_is_unchanged_and_the_entry_point_refuses_bad_sizes():
    lib = _loaded()
    assert lib.ABI_VERSION == 7
    with open(os.path.join(ROOT, "include", "unigen_hip.h")) as f:
        assert re.search(r"#define\s+UG_ABI_VERSION\s+7\b", f.read())
    L = lib.load()
    assert L.ug_abi_version() == 7
    # (q, ldq, cache_k, cache_v, key_valid, o, ldo, rows, S, P, H, HKV, head_dim, Tmax, scale, stream): refused on the host, no launch
    assert L.ug_attn_prefill_cached(0, 1536, 0, 0, 0, 0, 1536, 2, 5, 0, 12, 2, 64, 64, 0.1, 0) == -1 and b"head_dim 64" in L.ug_last_error()
    assert L.ug_attn_prefill_cached(0, 1536, 0, 0, 0, 0, 1536, 2, 5, 0, 12, 5, 128, 64, 0.1, 0) == -1 and b"multiple of HKV" in L.ug_last_error()
    assert L.ug_attn_prefill_cached(16, 1536, 16, 16, 0, 16, 1536, 2, 5, 60, 12, 2, 128, 64, 0.1, 0) == -1 and b"Tmax=64" in L.ug_last_error()
    assert L.ug_attn_prefill_cached(16, 1536, 16, 16, 0, 16, 1536, 2, 5, -1, 12, 2, 128, 64, 0.1, 0) == -1 and NAME.encode() in L.ug_last_error()
