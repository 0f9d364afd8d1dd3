"""`attention_masked_ref` (oracle/ops_ref.py), the float64 reference of tests/test_attention_edges_gpu.py, checked without a GPU: it
is `attention_ref` where no row is empty, gives exact zeros where the contract says so, and the per-row gradient bars of the GPU test
are 4 x what the rounding-point restatement measures (one small case of the measurement recorded in docs/experiments.md)."""
import torch

from oracle.ops_ref import attention_masked_ref, attention_ref
import test_attention_edges_gpu as E


def test_masked_ref_equals_additive_ref_without_empty_rows():
    B, L, H, HKV = 2, 70, 4, 2
    gen = torch.Generator().manual_seed(1)
    allow = torch.rand(B, L, L, generator=gen) < 0.3
    allow[:, torch.arange(L), torch.arange(L)] = True
    q = torch.randn(B, H, L, E.HD, generator=gen)
    k, v = torch.randn(B, HKV, L, E.HD, generator=gen), torch.randn(B, HKV, L, E.HD, generator=gen)
    add = torch.where(allow, 0.0, float(torch.iinfo(torch.int64).min))[:, None]
    o, lse = attention_masked_ref(q, k, v, allow, E.SCALE)
    want = attention_ref(q, k, v, add, E.SCALE)
    assert ((o - want.double()).norm() / want.double().norm()).item() < 1e-6          # attention_ref works in fp32
    s = (q.double() @ k.double().repeat_interleave(H // HKV, 1).transpose(2, 3)) * E.SCALE
    assert torch.allclose(lse, torch.logsumexp(s.masked_fill(~allow[:, None], float("-inf")), -1), rtol=0, atol=1e-12)


def test_masked_ref_empty_rows_and_unseen_keys_are_exact_zeros():
    shape = (3, 129, 6, 2)
    B, L, H, HKV = shape
    for kind in ("leftpad", "holes"):
        qkv, dout, allow, _ = E.make_inputs(shape, kind)
        o, lse, dq, dk, dv, lse32 = E._reference_cpu(qkv, dout, allow, shape)
        empty, unseen, _, _ = E.row_sets(allow)
        assert empty.any() and unseen.any()
        em, un = empty[:, None, :].expand(B, H, L), unseen[:, None, :].expand(B, HKV, L)
        assert (o[em] == 0).all() and (dq[em] == 0).all() and (lse[em] == float("inf")).all()
        assert (dk[un] == 0).all() and (dv[un] == 0).all()
        for t in (o, dq, dk, dv, lse[~em]):
            assert torch.isfinite(t).all()
        assert (lse32 - lse)[~em].abs().max().item() < 2e-6


def test_gradient_row_bars_are_four_times_the_restatement_error():
    shape = (3, 200, 4, 4)                 # holds the measured worst dk (band) and dv (leftpad) rows
    worst = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
    for kind in ("band", "leftpad"):
        qkv, dout, allow, _ = E.make_inputs(shape, kind)
        ref = dict(zip(("o", "lse", "dq", "dk", "dv", "lse32"), E._reference_cpu(qkv, dout, allow, shape)))
        sets = E.row_sets(allow)
        got = dict(zip(("o", "dq", "dk", "dv"), E.backward_restatement(qkv, dout, allow, shape)))
        for name in worst:
            den, judged = E.row_denominators(ref[name], name, sets)
            worst[name] = max(worst[name], ((got[name] - ref[name]).norm(dim=-1) / den)[judged].max().item())
    assert abs(4 * worst["dk"] / E.GRAD_ROW_BAR["dk"] - 1) < 0.01 and abs(4 * worst["dv"] / E.GRAD_ROW_BAR["dv"] - 1) < 0.01, worst
    assert 4 * worst["dq"] <= E.GRAD_ROW_BAR["dq"], worst
