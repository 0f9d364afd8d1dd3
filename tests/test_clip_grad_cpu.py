"""Gradient-norm clipping, the parts that need no GPU: the span grouping as a pure function, the torch fall-back of
`unigen_hip.optim.clip_grad_norm_` on CPU tensors (bit for bit torch's result and side effect), the new C ABI entry points and
the argument checks of the Python layer."""
import ctypes
import itertools

import pytest
import torch

NEW_ENTRY_POINTS = ("ug_sumsq_spans_f32", "ug_clip_finish", "ug_scale_spans_f32", "ug_adamw_flat_dev")


def test_span_grouping_merges_exact_abutment_only():
    from unigen_hip.optim import group_spans
    A, B = 0x7000_0000, 0x9000_0000                       # two storages
    # exact abutment in one storage merges (also a chain of three, also a start that is 4 mod 16)
    assert group_spans([(A, A, 16), (A, A + 64, 5)]) == [(A, 21)]
    assert group_spans([(A, A + 4, 3), (A, A + 16, 4), (A, A + 32, 1)]) == [(A + 4, 8)]
    # a 64-byte gap does not (FusedAdamW's runs would bridge it; a norm must not read the padding)
    assert group_spans([(A, A, 16), (A, A + 64 + 64, 16)]) == [(A, 16), (A + 128, 16)]
    # even a 4-byte gap does not
    assert group_spans([(A, A, 16), (A, A + 68, 16)]) == [(A, 16), (A + 68, 16)]
    # two storages never merge, even where the addresses abut
    assert group_spans([(A, A, 16), (B, A + 64, 16)]) == [(A, 16), (A + 64, 16)]
    # empty tensors vanish
    assert group_spans([(A, A, 0), (A, A, 4)]) == [(A, 4)]
    assert group_spans([]) == []


def test_span_grouping_ignores_input_order():
    from unigen_hip.optim import group_spans
    A, B = 0x7000_0000, 0x9000_0000
    triples = [(A, A, 16), (A, A + 64, 5), (A, A + 256, 7), (B, B + 4, 3), (B, B + 16, 12), (B, B + 4096, 1)]
    want = group_spans(triples)
    assert want == [(A, 21), (A + 256, 7), (B + 4, 15), (B + 4096, 1)]
    for perm in itertools.permutations(triples):
        assert group_spans(list(perm)) == want


def _cpu_params(seed, dtypes=(torch.float32, torch.float32, torch.bfloat16)):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for i, dt in enumerate(dtypes):
        p = torch.nn.Parameter(torch.zeros(7 + 5 * i, 3, dtype=dt))
        p.grad = torch.randn(7 + 5 * i, 3, generator=gen).to(dt)
        ps.append(p)
    ps.append(torch.nn.Parameter(torch.zeros(4)))         # grad None: skipped
    return ps


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
@pytest.mark.parametrize("norm_type", [2.0, 1.0, float("inf")])
def test_cpu_tensors_take_torch_bit_for_bit(max_norm, norm_type):
    from unigen_hip.optim import clip_grad_norm_
    ours, theirs = _cpu_params(3), _cpu_params(3)
    a = clip_grad_norm_(ours, max_norm, norm_type=norm_type)
    b = torch.nn.utils.clip_grad_norm_(theirs, max_norm, norm_type=norm_type)
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    for p, q in zip(ours, theirs):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad)


def test_empty_and_single_tensor_inputs():
    from unigen_hip.optim import clip_grad_norm_
    out = clip_grad_norm_([], 1.0)
    assert torch.equal(out, torch.nn.utils.clip_grad_norm_([], 1.0)) and float(out) == 0.0
    out = clip_grad_norm_([torch.nn.Parameter(torch.zeros(3))], 1.0)       # only grad=None parameters
    assert float(out) == 0.0
    p, q = _cpu_params(5)[0], _cpu_params(5)[0]                              # a bare tensor instead of a list, as torch accepts
    assert torch.equal(clip_grad_norm_(p, 0.1), torch.nn.utils.clip_grad_norm_(q, 0.1)) and torch.equal(p.grad, q.grad)


def test_error_if_nonfinite_on_the_fallback_path():
    from unigen_hip.optim import clip_grad_norm_
    ps = _cpu_params(7)
    ps[0].grad[0, 0] = float("inf")
    with pytest.raises(RuntimeError):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


def test_new_entry_points_exist_and_reject_all_zero_arguments():
    """Fails on a library without the clipping kernels: the symbols are missing from the table and from the shared object."""
    from unigen_hip import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    L.ug_last_error.restype = ctypes.c_char_p
    zero = {lib.P: None, lib.I64: 0, lib.I32: 0, lib.F32: 0.0}
    for name in NEW_ENTRY_POINTS:
        assert name in lib.SIGNATURES, name
        assert set(lib.SIGNATURES[name]) <= set(zero), name                 # only the argument kinds the table already uses
        fn = getattr(L, name)
        fn.argtypes, fn.restype = lib.SIGNATURES[name], ctypes.c_int
        rc = fn(*[zero[t] for t in lib.SIGNATURES[name]])
        msg = L.ug_last_error().decode()
        assert rc != 0 and name.replace("_dev", "") in msg, (name, rc, msg)
    assert lib.load().ug_abi_version() == lib.ABI_VERSION == 7              # additions do not bump the version
    # the device-factor form has ug_adamw_flat's signature plus one pointer
    base, dev = lib.SIGNATURES["ug_adamw_flat"], lib.SIGNATURES["ug_adamw_flat_dev"]
    assert dev == base[:13] + [lib.P] + base[13:]
    assert lib.family_of("ug_adamw_flat_dev") == lib.family_of("ug_adamw_flat") == "adamw"


def test_clip_finish_rejects_nan_thresholds_on_the_host():
    from unigen_hip import lib
    L = lib.load()
    import numpy as np
    a = np.zeros(64, dtype=np.float64)
    ptr = (a.ctypes.data + 15) & ~15
    rc = L.ug_clip_finish(ptr, 4, float("nan"), 1.0, ptr + 64, None)         # rejected before any launch: nothing is dereferenced
    assert rc == -1 and b"NaN" in L.ug_last_error()
    rc = L.ug_sumsq_spans_f32(ptr, 1, ptr + 64, 4097, 0, None)
    assert rc == -1 and b"blocks" in L.ug_last_error()


def test_bad_thresholds_raise():
    from unigen_hip.optim import FusedAdamW, clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError):
        clip_grad_norm_([p], float("nan"))
    with pytest.raises(ValueError):
        FusedAdamW([p], max_grad_norm=-1)
    with pytest.raises(ValueError):
        FusedAdamW([p], max_grad_norm=float("nan"))
    assert FusedAdamW([p]).max_grad_norm is None and FusedAdamW([p], max_grad_norm=2).max_grad_norm == 2.0
