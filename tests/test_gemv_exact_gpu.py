"""The pure-product decode entry points against the integer matmul, bit for bit (tests/exact_products.py: integer-valued bf16
operands make fp32 accumulation exact in any order, so split-K atomics, LDS pre-reduction, k-block slots and ordered sums all have to
give `torch.equal` with the CPU reference at every element).

  ug_gemv_bf16 (ops.gemv_acc_, ops.skinny_linear)          dense regime into an integer-prefilled accumulator; small-sum regime
                                                           through ug_skinny_finish (bf16 + bias, bf16-rounded residual update)
  ug_decode_gemv (ops.decode_gemv_)                        dense regime, with the clears it carries
  ug_decode_sw_kblock / ug_decode_sw_resid                 at the widths they are built for (K % 1792 == 0 / K == 1536)
  ug_gemv_bf16_ord + ug_skinny_finish_ord, ug_decode_sw_kblock_ord + ug_decode_finish_resid_norm_ord (without the norm output)

Activations and weights are stored with padded leading dimensions; accumulators carry a sentinel past column N.  The launches that
fuse RMSNorm, the residual add or SwiGLU are in tests/test_decode_exact_gpu.py (inputs that make their arithmetic integer); the ones
that fuse RoPE and attention are not integer and stay with tests/test_decode_parity_gpu.py.
"""
import pytest
import torch

import exact_products as ep

pytestmark = pytest.mark.gpu


def _ops():
    from unigen_hip import ops
    return ops


def _operands(dev, R, N, K, regime):
    x, w, bias, ref = ep.problem(R, N, K, regime)
    return ep.store(x, False, dev), ep.store(w, False, dev), bias, ref


def _clears(dev, R):
    return torch.ones(16, 2048, device=dev), torch.ones(R, 1536, device=dev), torch.ones(32, device=dev)


def _assert_cleared(*ts):
    for t in ts:
        assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("R,N,K", ep.GEMV_SHAPES + ep.GEMV_TALL_SHAPES)
def test_gemv_acc_into_prefilled_accumulator(dev, R, N, K):
    """ug_gemv_bf16: the ring kernel (K >= 256) and the direct-load kernel (K = 32); twice into the same accumulator.  The shapes of
    more than 16 rows run the two-row-block instantiations: gemv_kernel<2, .> at K = 32, gemv_ring_kernel<2, 1> and -- from 3000 tiles
    on, (24, 8016, 1536) has 501 groups x 6 slabs -- gemv_ring_kernel<2, 2>.  The shapes of 16 369 and 32 753 weight rows at K < 256
    run the direct kernel's unrolls 2, 4 and 8 (tests/test_decode_plan_cpu.py says which shape selects which instantiation)."""
    ops = _ops()
    x, w, _, ref = _operands(dev, R, N, K, "dense")
    pre = ep.int_prefill(R, N, seed=N + K)
    acc = ep.out_buffer(R, N, torch.float32, dev, prefill=pre)
    for rep in (1, 2):
        ops.gemv_acc_(x, w, acc[:, :N])
        ep.assert_exact(acc, N, pre + rep * ref, f"gemv_acc_ {(R, N, K)} call {rep}")


@pytest.mark.parametrize("R,N,K", ep.GEMV_SHAPES + ep.GEMV_TALL_SHAPES)
def test_skinny_linear_bias_and_residual(dev, R, N, K):
    ops = _ops()
    x, w, bias, ref = _operands(dev, R, N, K, "small")
    y = ops.skinny_linear(x, w, bias=bias.to(dev))
    ep.assert_exact(y, N, (ref + bias.float()).to(torch.bfloat16), f"skinny_linear + bias {(R, N, K)}")
    y = ops.skinny_linear(x, w)
    ep.assert_exact(y, N, ref.to(torch.bfloat16), f"skinny_linear {(R, N, K)}")
    pre = ep.int_prefill(R, N, seed=N + K + 1)
    res = pre.clone().to(dev)
    ops.skinny_linear(x, w, resid=res)
    ep.assert_exact(res, N, pre + ref, f"skinny_linear residual {(R, N, K)}")


@pytest.mark.parametrize("R,N,K", [s for s in ep.GEMV_SHAPES + ep.GEMV_TALL_SHAPES if s[2] >= 256])
def test_decode_gemv_with_clears(dev, R, N, K):
    ops = _ops()
    x, w, _, ref = _operands(dev, R, N, K, "dense")
    pre = ep.int_prefill(R, N, seed=N + K + 2)
    acc = ep.out_buffer(R, N, torch.float32, dev, prefill=pre)
    z0, z1, ss = _clears(dev, R)
    ops.decode_gemv_(x, w, acc[:, :N], zero0=z0, zero1=z1, ss_zero=ss)
    ep.assert_exact(acc, N, pre + ref, f"decode_gemv_ {(R, N, K)}")
    _assert_cleared(z0, z1, ss)
    ops.decode_gemv_(x, w, acc[:, :N])
    ep.assert_exact(acc, N, pre + 2 * ref, f"decode_gemv_ {(R, N, K)} second call")


@pytest.mark.parametrize("R,N,K", ep.GEMV_KBLOCK_SHAPES)
def test_decode_sw_kblock_with_clears(dev, R, N, K):
    """ug_decode_sw_kblock: k-blocks of 1 792, seven partial tiles pre-reduced in LDS, one atomic per element and k-block; N ragged
    against the 32-row workgroup"""
    ops = _ops()
    x, w, _, ref = _operands(dev, R, N, K, "dense")
    pre = ep.int_prefill(R, N, seed=N + K + 3)
    acc = ep.out_buffer(R, N, torch.float32, dev, prefill=pre)
    z0, z1, ss = _clears(dev, R)
    ops.decode_sw_kblock_(x, w, acc[:, :N], zero0=z0, zero1=z1, ss_zero=ss)
    ep.assert_exact(acc, N, pre + ref, f"decode_sw_kblock_ {(R, N, K)}")
    _assert_cleared(z0, z1, ss)
    ops.decode_sw_kblock_(x, w, acc[:, :N])
    ep.assert_exact(acc, N, pre + 2 * ref, f"decode_sw_kblock_ {(R, N, K)} second call")


@pytest.mark.parametrize("R,N,K", ep.GEMV_SW_RESID_SHAPES)
def test_decode_sw_resid(dev, R, N, K):
    """ug_decode_sw_resid: h += float(bf16(x W^T)), one writer per element (small-sum regime: the bf16 rounding is exact); twice"""
    ops = _ops()
    x, w, _, ref = _operands(dev, R, N, K, "small")
    pre = ep.int_prefill(R, N, seed=N + K + 4)
    h = pre.clone().to(dev)
    for rep in (1, 2):
        ops.decode_sw_resid_(x, w, h)
        ep.assert_exact(h, N, pre + rep * ref, f"decode_sw_resid_ {(R, N, K)} call {rep}")


@pytest.mark.parametrize("R,N,K", ep.GEMV_SHAPES + ep.GEMV_ORD_TALL_SHAPES)
def test_skinny_linear_ord(dev, R, N, K):
    """ug_gemv_bf16_ord + ug_skinny_finish_ord: per-256-k-slice slots summed in slice order -- bf16 (+ bias), residual update, fp32;
    17 rows run the two-row-block form gemv_ring_kernel<2, 1, true>"""
    ops = _ops()
    x, w, bias, ref = _operands(dev, R, N, K, "small")
    y = ops.skinny_linear_ord(x, w, bias=bias.to(dev))
    ep.assert_exact(y, N, (ref + bias.float()).to(torch.bfloat16), f"skinny_linear_ord + bias {(R, N, K)}")
    pre = ep.int_prefill(R, N, seed=N + K + 5)
    res = pre.clone().to(dev)
    ops.skinny_linear_ord(x, w, resid=res)
    ep.assert_exact(res, N, pre + ref, f"skinny_linear_ord residual {(R, N, K)}")
    x, w, _, ref = _operands(dev, R, N, K, "dense")
    out = torch.full((R, N), ep.SENTINEL, device=dev)
    ops.skinny_linear_ord(x, w, out_f32=out)
    ep.assert_exact(out, N, ref, f"skinny_linear_ord fp32 {(R, N, K)}")


@pytest.mark.parametrize("R,N,K", ep.GEMV_KBLOCK_SHAPES)
def test_decode_sw_kblock_ord_slots_and_finisher(dev, R, N, K):
    """ug_decode_sw_kblock_ord: slot b holds exactly the products of k-block b (dense regime, padded slot rows left untouched);
    ug_decode_finish_resid_norm_ord without the norm output is the pure sum x += bf16(sum of the slots) (small-sum regime)."""
    ops = _ops()
    P, ld = K // 1792, ep.round_up(N, 8) + 8
    xc, wc, _, _ = ep.problem(R, N, K, "dense")
    x, w, _, _ = _operands(dev, R, N, K, "dense")
    parts = torch.full((P, R, ld), ep.SENTINEL, device=dev)
    ops.decode_sw_kblock_ord_(x, w, parts)
    for b in range(P):
        blk = slice(b * 1792, (b + 1) * 1792)
        ep.assert_exact(parts[b], N, xc[:, blk].float() @ wc[:, blk].float().t(), f"decode_sw_kblock_ord_ {(R, N, K)} slot {b}")
    x, w, _, ref = _operands(dev, R, N, K, "small")
    ops.decode_sw_kblock_ord_(x, w, parts)
    pre = ep.int_prefill(R, N, seed=N + K + 6)
    stream = pre.clone().to(dev)
    ops.decode_finish_resid_norm_ord_(parts, stream, torch.ones(N, device=dev), None, 1e-6)
    ep.assert_exact(stream, N, pre + ref, f"decode_finish_resid_norm_ord_ {(R, N, K)}")
