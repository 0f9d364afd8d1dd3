"""Why the exact-integer tests exist, and that their operands meet the method's conditions -- without a GPU.

A Frobenius-norm gate cannot see a local fault: on the 4400 x 4000 x 3104 problem of `test_gemm_bf16_partial_last_round` the faults a
tile kernel actually has -- the last k index dropped in one row, one 8-wide k chunk dropped inside one 16 x 16 fragment -- move the
relative norm by a few 1e-4, under both `_rel < 4e-3` (bf16 outputs) and `_rel < 1e-5 * sqrt(K) + 1e-6` (fp32 outputs).  With
integer operands (tests/exact_products.py) the same faults, and the wider ones (rows swapped, bias shifted by a column, beta ignored,
one k-slice's partial left out of one tile), are a failed `torch.equal`.  The faults are injected into the CPU reference here; the
GPU files apply the exact comparison to the kernels.
"""
import math

import pytest
import torch

import exact_products as ep

SHAPE = (4400, 4000, 3104)
ROW, R0, C0, K0 = 1337, 2048 + 32, 512 + 48, 1000          # the faulty row; the faulty 16 x 16 block and its 8-wide k chunk
TILE = (16, 15)                                            # the 256 x 256 tile (ragged in M and N) that loses a k-slice's partial


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def _faults(a, b, ref):
    """name -> (faulty a @ b^T, block-local?)"""
    M, N, K = a.shape[0], b.shape[0], a.shape[1]
    af, bf = a.float(), b.float()
    out = {}
    row = next(r for r in range(ROW, M) if af[r, K - 1] != 0)          # (a zero there would make the dropped product invisible)
    f = ref.clone()
    f[row] -= af[row, K - 1] * bf[:, K - 1]
    out["last k index dropped in one row"] = (f, True)
    f = ref.clone()
    lost = af[R0:R0 + 16, K0:K0 + 8] @ bf[C0:C0 + 16, K0:K0 + 8].t()
    assert lost.abs().max() > 0
    f[R0:R0 + 16, C0:C0 + 16] -= lost
    out["one 8-wide k chunk dropped inside one 16x16 block"] = (f, True)
    f = ref.clone()
    f[[ROW, ROW + 1]] = ref[[ROW + 1, ROW]]
    out["two adjacent rows swapped"] = (f, False)
    f = ref.clone()
    rows, cols = slice(TILE[0] * 256, min(M, TILE[0] * 256 + 256)), slice(TILE[1] * 256, min(N, TILE[1] * 256 + 256))
    f[rows, cols] -= af[rows, K // 2:] @ bf[cols, K // 2:].t()
    out["one slice's partial left out of one tile"] = (f, False)
    return out


def test_exact_comparison_rejects_what_the_bf16_norm_gate_accepts():
    """small-sum regime, bf16 epilogue with bias"""
    a, b, bias, ref = ep.problem(*SHAPE, "small")
    want = (ref + bias.float()).to(torch.bfloat16)
    assert torch.equal(want.float(), ref + bias.float())               # the epilogue is exact in this regime
    faults = {k: ((f + bias.float()).to(torch.bfloat16), local) for k, (f, local) in _faults(a, b, ref).items()}
    faults["bias shifted by one column"] = ((ref + bias.float().roll(1)).to(torch.bfloat16), False)
    for name, (got, local) in faults.items():
        assert not torch.equal(got, want), name
        rel = _rel(got, want)
        print(f"bf16 gate 4e-3: {name}: _rel = {rel:.3g}")
        if local:
            assert rel < 4e-3, (name, rel)                             # ... which is why the norm-gated tests pass such a kernel


def test_exact_comparison_rejects_what_the_fp32_norm_gate_accepts():
    """dense regime, accumulating fp32 epilogue"""
    M, N, K = SHAPE
    a, b, _, ref = ep.problem(M, N, K, "dense")
    pre = ep.int_prefill(M, N, seed=1)
    want = pre + ref
    gate = 1e-5 * math.sqrt(K) + 1e-6
    faults = {k: (pre + f, local) for k, (f, local) in _faults(a, b, ref).items()}
    faults["beta ignored"] = (ref.clone(), False)
    for name, (got, local) in faults.items():
        assert not torch.equal(got, want), name
        rel = _rel(got, want)
        print(f"fp32 gate {gate:.3g}: {name}: _rel = {rel:.3g}")
        if local:
            assert rel < gate, (name, rel)


def test_fp32_reference_equals_float64_on_sampled_rows():
    for regime in ("small", "dense"):
        a, b, _, ref = ep.problem(777, 333, 1000, regime)
        rows = torch.tensor([0, 1, 255, 256, 500, 776])
        assert torch.equal(ref[rows].double(), a[rows].double() @ b.double().t())


def test_generators_hold_what_they_promise():
    d = ep.dense(300, 192, seed=3).float()
    assert set(d.unique().tolist()) == {-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0}
    s = ep.small_sum(300, 4096, seed=3).float()
    assert set(s.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs((s != 0).float().mean().item() - ep.small_sum_density(4096)) < 0.01
    assert (ep.small_sum(50, 192, seed=3) != 0).all()                  # K <= 1024: density 1
    bias = ep.int_bias(4000, seed=3).float()
    assert bias.abs().max().item() == ep.BIAS_RANGE and torch.equal(bias, bias.round())
    assert torch.equal(ep.dense(64, 64, seed=9), ep.dense(64, 64, seed=9))
    x = ep.dense(13, 21, seed=1)
    km, rm = ep.store(x, True), ep.store(x, False)
    assert km.shape == (21, 13) and km.stride(0) == 24 and torch.equal(km, x.t()) and rm.stride(0) == 32 and torch.equal(rm, x)
    assert (km.as_strided((21, 24), (24, 1))[:, 13:] == ep.PAD_BF16).all() and (rm.as_strided((13, 32), (32, 1))[:, 21:] == 0).all()


def test_exact_ref_refuses_operands_outside_the_regimes():
    with pytest.raises(AssertionError):
        ep.exact_ref(torch.full((4, 2 ** 20), 4.0).to(torch.bfloat16), torch.full((4, 2 ** 20), 4.0).to(torch.bfloat16))
    with pytest.raises(AssertionError):
        ep.exact_ref(torch.ones(4, 512).to(torch.bfloat16), torch.ones(4, 512).to(torch.bfloat16), small=True)
    with pytest.raises(AssertionError):
        ep.exact_ref(torch.full((4, 8), 0.5).to(torch.bfloat16), torch.ones(4, 8).to(torch.bfloat16))


@pytest.mark.parametrize("M,N,K,regime", ep.all_problems(), ids=lambda v: str(v))
def test_every_gpu_shape_meets_its_regime_conditions(M, N, K, regime):
    """problem() builds the reference through exact_ref, which asserts |sum| < 2^24 and, in the small-sum regime, |sum + bias| <= 256:
    a shape that breaks a condition fails here and not on the GPU machine."""
    a, b, bias, ref = ep.problem(M, N, K, regime)
    assert ref.shape == (M, N) and ref.abs().max().item() < ep.EXACT_LIMIT
    if regime == "small":
        assert (ref + bias.float()).abs().max().item() <= ep.BF16_EXACT_LIMIT
    else:
        assert (a != 0).all() and (b != 0).all()
