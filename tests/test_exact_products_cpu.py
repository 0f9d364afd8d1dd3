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
    if regime in ep.FUSED_REGIMES:
        ep.problem(M, N, K, regime)            # the generators assert their own conditions (tests/exact_products.py, fused decode launches)
        return
    a, b, bias, ref = ep.problem(M, N, K, regime)
    assert ref.shape == (M, N) and ref.abs().max().item() < ep.EXACT_LIMIT
    if regime == "small":
        assert (ref + bias.float()).abs().max().item() <= ep.BF16_EXACT_LIMIT
    else:
        assert (a != 0).all() and (b != 0).all()


# ------------------------------------------------------------------------------------------------ fused decode launches
def test_fused_generators_hold_what_they_promise():
    p = ep.problem(5, 264, ep.SW_HIDDEN, "gate_up")
    assert set(p.sign.unique().tolist()) == {-1.0, 1.0} and p.scale[:, 0].tolist() == [0.5, 1.0, 2.0, 4.0, 8.0]
    assert torch.equal((p.target * p.target).sum(-1), ep.SW_HIDDEN * p.scale[:, 0] ** 2)          # the statistics are exact in any order
    assert (ep.bf16_round(p.pend) != p.pend).any() and torch.equal(p.x_in + ep.bf16_round(p.pend), p.target)
    assert ep.bf16_round(torch.tensor([259.0])).item() == 260.0
    p = ep.problem(5, 8960, ep.SW_HIDDEN, "gate_up")                    # large enough for the tails: g <= -104 is 3.2 sigma out
    assert 0.1 < p.exact.float().mean().item() < 0.6 and (p.g <= ep.SILU_ZERO).any() and (p.g == 0).any()
    assert ((p.g > ep.SILU_ZERO) & (p.g <= -88)).any()                  # ... and the band where fp32 exp overflows and fp64 does not
    q = ep.problem(5, 100, 8992, "swiglu")
    assert (q.operand != 0).float().mean().item() > 0.7 and (q.operand == 0).float().mean().item() > 0.2
    assert q.G.max().item() == 64 and q.G.min().item() == -120 and sorted(set(q.j[:, 0].tolist())) == [-1, 0, 1, 2, 3]
    r = ep.problem(5, 333, 1568, "resid_norm")
    assert (r.operand != 0).all() and r.operand.float().abs().max().item() == 4 and torch.equal(r.parts5.sum(0), r.pend)
    x = torch.tensor([1.0, 1.5, 255.0, 0.0, -3.0e-5])
    assert torch.equal(ep.bf16_ulp(x)[:4], torch.tensor([2.0 ** -7, 2.0 ** -7, 1.0, 0.0]))


REACHED = {         # (RB, NW, KW, XCD-major grid) of gemv_ring4_kernel by the rule of launch_ring_auto, 256 CUs
    "resid_norm": {(1, 16, 256): (1, 4, 1, False), (5, 333, 1568): (1, 4, 1, False), (16, 2048, 1536): (1, 4, 1, False),
                   (13, 272, 3584): (1, 4, 1, False), (17, 333, 1568): (2, 4, 1, False), (32, 2048, 1536): (2, 4, 1, False),
                   (16, 8208, 1536): (1, 7, 2, False), (16, 16400, 1536): (1, 9, 3, False), (16, 48, 4864): (1, 8, 2, True)},
    "swiglu": {(1, 16, 512): (1, 4, 1, False), (5, 100, 8992): (1, 8, 2, True), (16, 1536, 8960): (1, 8, 2, True),
               (24, 256, 8960): (2, 4, 1, False), (16, 1552, 8960): (1, 7, 2, False), (9, 48, 18944): (1, 8, 2, True),
               (16, 16400, 1536): (1, 9, 3, False)},
}


def test_fused_shapes_reach_the_instantiations_they_are_listed_for():
    assert set(REACHED["resid_norm"]) == set(ep.RESID_NORM_SHAPES) and set(REACHED["swiglu"]) == set(ep.SWIGLU_SHAPES)
    for table in REACHED.values():
        for shape, want in table.items():
            assert ep.ring_fused_shape(*shape) == want, (shape, ep.ring_fused_shape(*shape), want)
    # the model's gate/up projection takes (9,3); its down projection (7,2) only with the XCD-major grid switched off
    assert ep.ring_fused_shape(16, 17920, 1536) == (1, 9, 3, False) and ep.ring_fused_shape(16, 1536, 8960, xcd_major=False) == (1, 7, 2, False)
    assert [ep.ring_plain_shape(*s) for s in ep.GEMV_TALL_SHAPES[1:4]] == [(2, 1), (2, 1), (2, 2)]       # (those with K >= 256)
    # single-writer splits at 256 CUs: (units per workgroup, workgroups, tiles, units of the last workgroup)
    assert ep.sw_split(8, 256, 40, 8) == (1, 8, [1], 1) and ep.sw_split(264, 256, 40, 8)[:3] == (2, 132, [2])
    assert ep.sw_split(2056, 256, 40, 8) == (9, 229, [8, 1], 4) and ep.sw_split(8960, 256, 40, 8)[:3] == (35, 256, [8, 8, 8, 8, 3])
    assert ep.sw_split(10248, 256, 40, 8)[:3] == (40, 257, [8] * 5)
    assert ep.sw_split(128, 256, 32, 16)[:2] == (1, 128) and ep.sw_split(2047, 256, 32, 16)[:3] == (8, 256, [8])
    assert ep.sw_split(4097, 256, 32, 16)[:3] == (17, 241, [16, 1]) and ep.sw_split(8192, 256, 32, 16)[:3] == (32, 256, [16, 16])
    assert ep.sw_split(8200, 256, 32, 16) == (32, 257, [16, 16], 8) and ep.sw_split(7, 256, 32, 16)[:2] == (1, 7)


def test_ring_candidates_no_shape_reaches():
    """(4,2) costs ceil(ceil(g / 8) s / 256) * 8 >= ceil(ceil(g / 4) s / 512) * 8 >= ceil(ceil(g / 4) s / 256) * 4, the cost of (4,1), and
    a tie goes to the first candidate: gemv_ring4_kernel<1, 2, ., 4> and <2, 2, ., 4> are never launched.  Enumerated as well."""
    import numpy as np
    g, s = np.meshgrid(np.arange(1, 6001, dtype=np.int64), np.arange(1, 129, dtype=np.int64), indexing="ij")
    cost = [-(-(-(-g // (nw * kw)) * s) // 256) * nw * kw for nw, kw in ep.RING_CANDS]
    assert (cost[1] >= cost[0]).all()
    best = np.argmin(np.stack(cost), axis=0)                      # (first minimum: ties go to the earlier candidate)
    assert set(np.unique(best).tolist()) == {0, 2, 3}
    for shape in [(16, 16 * 6000, 256 * 128), (32, 16 * 4097, 1536), (20, 8208, 1536)]:
        assert ep.ring_fused_shape(*shape)[1:3] != (4, 2)


def _gate_up_model(p, rstd_shift=0, round_pend=True, inner_round=True, pair_shift=0, drop=None):
    """the launch's own formula in fp32 (torch.exp for __expf), with the faults a kernel of this kind can have"""
    I = p.g.shape[1]
    x = p.x_in + (ep.bf16_round(p.pend) if round_pend else p.pend)
    rs = torch.rsqrt((x * x).sum(-1, keepdim=True) / x.shape[1] + ep.EPS).roll(rstd_shift, 0)
    opnd = ep.bf16_round(p.norm_w * (x * rs))
    gu = opnd @ p.w.float().t()
    if drop is not None:
        c0, k0 = drop
        gu[:, c0:c0 + 16] -= opnd[:, k0:k0 + 8] @ p.w.float()[c0:c0 + 16, k0:k0 + 8].t()
    g, u = ep.bf16_round(gu[:, :I]), ep.bf16_round(gu[:, I:]).roll(-pair_shift, 1)
    sil = g / (1 + torch.exp(-g))
    return ((ep.bf16_round(sil) if inner_round else sil) * u).to(torch.bfloat16)


def _swiglu_model(p, norm_cols, ss_scale=None, rstd_shift=0, pair_shift=0, drop=None):
    K = p.G.shape[1]
    ss = norm_cols * p.ss_unit * (1 if ss_scale is None else ss_scale)
    rs = torch.rsqrt(ss / norm_cols + ep.EPS).unsqueeze(1).roll(rstd_shift, 0)
    g, u = ep.bf16_round(rs * p.gu[:, :K]), ep.bf16_round(rs * p.gu[:, K:]).roll(-pair_shift, 1)
    opnd = ep.bf16_round(ep.bf16_round(g / (1 + torch.exp(-g))) * u)
    acc = opnd @ p.w.float().t()
    if drop is not None:
        c0, k0 = drop
        acc[:, c0:c0 + 16] -= opnd[:, k0:k0 + 8] @ p.w.float()[c0:c0 + 16, k0:k0 + 8].t()
    return acc


def test_fused_checks_reject_what_the_norm_gates_accept():
    """the six faults, injected into the fp32 restatement of one gate_up and one SwiGLU-prologue launch; tests/test_kernels_gpu.py gates
    the two at _rel < 6e-3 and < 1e-2"""
    p = ep.problem(5, 2056, ep.SW_HIDDEN, "gate_up")
    assert ep.gate_up_check(_gate_up_model(p), p) <= ep.GATE_UP_DIFFER_CAP
    faults = {
        "one 8-wide k chunk dropped in one 16x16 block": dict(drop=(1040, 1000)),
        "gate of unit c with the up of unit c + 1": dict(pair_shift=1),
        "another row's rstd": dict(rstd_shift=1),
        "pending term not rounded to bf16": dict(round_pend=False),
        "inner bf16(silu) rounding skipped": dict(inner_round=False),
    }
    for name, kw in faults.items():
        got = _gate_up_model(p, **kw)
        rel = _rel(got, p.act)
        print(f"gate_up, gate 6e-3: {name}: _rel = {rel:.3g} -> the norm gate {'ACCEPTS' if rel < 6e-3 else 'rejects'} it")
        with pytest.raises(AssertionError):
            ep.gate_up_check(got, p, name)
    # the stream out (x_out) of the unrounded pending term is off by c_r wherever the rounding moved
    assert not torch.equal(p.x_in + p.pend, p.target)

    q = ep.problem(5, 100, 8992, "swiglu")
    K = 8992
    for cols in ep.SWIGLU_NORM_COLS:
        assert torch.equal(_swiglu_model(q, cols), q.acc)
    faults = {
        "one 8-wide k chunk dropped in one 16x16 block": dict(drop=(48, 4000)),
        "gate of unit c with the up of unit c + 1": dict(pair_shift=1),
        "another row's rstd": dict(rstd_shift=1),
    }
    big = ep.problem(16, 1536, 8960, "swiglu")                          # the model's down projection, for the gate's verdict
    for name, kw in faults.items():
        rel = _rel(_swiglu_model(big, 1536, **kw), big.acc)
        print(f"swiglu prologue, gate 1e-2: {name}: _rel = {rel:.3g} -> the norm gate {'ACCEPTS' if rel < 1e-2 else 'rejects'} it")
        assert rel > 0 and not torch.equal(_swiglu_model(q, 1536, **kw), q.acc), name            # the exact comparison rejects it
    # (a skipped inner rounding cannot show in this regime: silu(g) is g or -0 exactly; the epilogue's cap above is its check)
    # The ragged last slab (k 1536 .. 1567 of K = 1568) re-read by its seven clamped k-steps and counted once more in the sum of squares:
    # a fault of the PRODUCER of the statistics, ug_decode_gemv_resid_norm, whose ss_out is compared bit for bit.  Handed on to the
    # prologue above it moves rstd by 32 / (2 K): 1 % at this K, but 0.18 % at K = 8992 -- under the half ulp of bf16, by the regime's design.
    r = ep.problem(5, 333, 1568, "resid_norm")
    got = r.ss + (r.xnew[:, 1536:] ** 2).sum(-1)
    print(f"resid_norm ss_out, gate 1e-5 (tests/test_kernels_gpu.py): ragged slab's clamped re-read counted twice: _rel = {_rel(got, r.ss):.3g}")
    assert not torch.equal(got, r.ss)
    assert torch.equal(_swiglu_model(q, 1536, ss_scale=1 + 32 / K), q.acc) and not torch.equal(_swiglu_model(q, 1536, ss_scale=1 + 32 / 1568), q.acc)


@pytest.mark.parametrize("R,I", [(5, 8960), (16, 2056), (12, 10248)])
def test_gate_up_cap_separates_the_launch_from_one_without_the_inner_rounding(R, I):
    """the 1 % cap is a condition: the fp32 restatement of the launch stays far under it, the same without bf16(silu) far over it"""
    p = ep.problem(R, I, ep.SW_HIDDEN, "gate_up")
    share = ep.gate_up_check(_gate_up_model(p), p)
    skipped = (_gate_up_model(p, inner_round=False).float() != p.act.float()).float().mean().item()
    print(f"gate_up {(R, I)}: fp32 restatement differs from the fp64 expectation on {share:.5%}, without the inner rounding on {skipped:.3%}")
    assert share < ep.GATE_UP_DIFFER_CAP / 10 and skipped > 5 * ep.GATE_UP_DIFFER_CAP
