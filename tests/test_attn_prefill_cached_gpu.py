"""ug_attn_prefill_cached (csrc/attention.hip) through ops.attn_prefill_cached: causal attention of S new query rows per cache row
against keys and values that live in the decode cache [rows][HKV][Tmax][128].

Reference: oracle.ops_ref.attention_ref in fp32 on the equivalent dense problem (queries = the new rows, keys = cache [0, P+S)).
Bars: the project's forward bar over the whole output (8e-3, test_kernels_gpu.py: test_attention_fwd_bwd), and per query row
max(8e-3, 1.5 x e_row), e_row = the same row's error of ops.attn_fwd on the equivalent square problem (L = P + S, same mask) against
the same reference; 1.5 is the row-to-row spread test_decode_parity_gpu.py grants between two bf16 evaluations.
The cache holds 1e4 beyond P+S and +-1e4 at every hidden key, so a kernel that reads either into a result shows it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, HD = torch.bfloat16, 128
FWD_BAR, ROW_SPREAD = 8e-3, 1.5
# (rows, S, P, Tmax, H, HKV): S below, at and over a 16-row and a 64-row block; P at 0, 1, 63 / 64 / 65; P+S ending exactly at Tmax;
# P+S past 512
SHAPES = [(1, 1, 0, 64, 2, 1), (3, 5, 63, 128, 12, 2), (2, 70, 64, 200, 6, 2), (16, 17, 65, 128, 12, 2), (2, 64, 130, 194, 12, 2),
          (1, 130, 1, 131, 12, 2), (3, 40, 507, 560, 12, 2)]
MODES = ["none", "holes"]


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


class _Case:
    """Seeded inputs of one launch, the fp32 reference, and the outputs of the new kernel and of ops.attn_fwd on the square problem."""

    def __init__(self, shape, mode, dev):
        from oracle.ops_ref import attention_ref
        from unigen_hip import ops
        rows, S, P, Tmax, H, HKV = shape
        L = P + S
        g = torch.Generator().manual_seed(sum(v * 31 ** i for i, v in enumerate(shape)) + len(mode))
        self.q = torch.randn(rows * S, H * HD, generator=g).to(BF)
        K = torch.randn(rows, HKV, Tmax, HD, generator=g).to(BF)
        V = torch.randn(rows, HKV, Tmax, HD, generator=g).to(BF)
        K[:, :, L:], V[:, :, L:] = 1e4, 1e4
        valid = torch.ones(rows, L, dtype=torch.bool)
        self.empty = None
        if mode == "holes":
            valid[:, :P] = torch.rand(rows, P, generator=g) > 0.2                       # (own keys P + s stay visible)
            r0, s0 = int(torch.randint(rows, (1,), generator=g)), int(torch.randint(S, (1,), generator=g))
            valid[r0, :P + s0 + 1] = False                                               # this query sees nothing
            self.empty = (r0, s0)
            sign = torch.where(torch.rand(rows, 1, L, 1, generator=g) < 0.5, -1e4, 1e4)
            hide = ~valid[:, None, :, None]
            K[:, :, :L] = torch.where(hide, sign, K[:, :, :L].float()).to(BF)
            V[:, :, :L] = torch.where(hide, -sign, V[:, :, :L].float()).to(BF)
        self.K, self.V, self.valid = K, V, valid
        self.kv = None
        if mode == "holes":
            self.kv = torch.ones(rows, Tmax, dtype=torch.uint8)                           # (beyond P+S: left to the causal compare)
            self.kv[:, :L] = valid.to(torch.uint8)
        # ---- fp32 reference on the dense problem
        s = torch.arange(S)
        allow = (torch.arange(L)[None, :] <= (P + s)[:, None])[None] & valid[:, None, :]          # [rows, S, L]
        self.allow = allow
        mask_add = torch.where(allow, 0.0, float("-inf"))[:, None]
        mask_add = torch.where(allow.any(-1)[:, None, :, None], mask_add, torch.zeros(()))           # (an empty row: replaced below)
        qd = self.q.view(rows, S, H, HD).permute(0, 2, 1, 3)
        ref = attention_ref(qd, K[:, :, :L], V[:, :, :L], mask_add, 1.0 / math.sqrt(HD))             # [rows, H, S, d]
        ref = torch.where(allow.any(-1)[:, None, :, None], ref, torch.zeros(()))
        self.ref = ref.permute(0, 2, 1, 3).reshape(rows * S, H * HD)
        # ---- the new kernel (the output starts as NaN: every element must be written)
        self.Kd, self.Vd, self.qd = K.to(dev), V.to(dev), self.q.to(dev)
        self.kvd = None if self.kv is None else self.kv.to(dev)
        out = torch.full((rows * S, H * HD), float("nan"), dtype=BF, device=dev)
        ops.attn_prefill_cached(self.qd, self.Kd, self.Vd, self.kvd, S, P, H, HKV, HD, Tmax, out=out)
        self.got = out.float().cpu()
        # ---- ops.attn_fwd on the square problem: rows of L positions, the new queries at [P, L), finite filler queries before
        qkv = torch.zeros(rows, L, (H + 2 * HKV) * HD)
        qkv[:, :P, :H * HD] = torch.randn(rows, P, H * HD, generator=g)
        qkv[:, P:, :H * HD] = self.q.float().view(rows, S, H * HD)
        qkv[:, :, H * HD:(H + HKV) * HD] = K[:, :, :L].float().permute(0, 2, 1, 3).reshape(rows, L, HKV * HD)
        qkv[:, :, (H + HKV) * HD:] = V[:, :, :L].float().permute(0, 2, 1, 3).reshape(rows, L, HKV * HD)
        mb = ops.mask_causal(rows, L, dev, key_valid=valid.to(dev))
        o, _ = ops.attn_fwd(qkv.view(rows * L, -1).to(BF).to(dev), mb, H, HKV, HD)
        self.square = o.view(rows, L, H * HD)[:, P:].reshape(rows * S, H * HD).float().cpu()
        torch.cuda.synchronize()


_CASES = {}


def _case(shape, mode, dev):
    if (shape, mode) not in _CASES:
        _CASES[(shape, mode)] = _Case(shape, mode, dev)
    return _CASES[(shape, mode)]


def _row_errs(got, ref):
    return (got.double() - ref.double()).norm(dim=1) / ref.double().norm(dim=1).clamp_min(1e-30)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_fp32_reference(dev, shape, mode):
    c = _case(shape, mode, dev)
    rows, S, P, Tmax, H, HKV = shape
    assert bool(torch.isfinite(c.got).all()), "an element was not written, or a masked value reached the output"
    whole = _rel(c.got, c.ref)
    live = c.allow.any(-1).reshape(-1)
    e, e_row = _row_errs(c.got, c.ref)[live], _row_errs(c.square, c.ref)[live]
    bar = torch.clamp(ROW_SPREAD * e_row, min=FWD_BAR)
    worst = lambda t: float(t.max()) if t.numel() else 0.0
    print(f"    {shape} {mode}: whole {whole:.2e} (attn_fwd on the square problem {_rel(c.square, c.ref):.2e}); worst row {worst(e):.2e} "
          f"(attn_fwd's worst row {worst(e_row):.2e})")
    assert whole < FWD_BAR, whole
    bad = (e > bar).nonzero().flatten().tolist()
    assert not bad, [(r, float(e[r]), float(e_row[r])) for r in bad[:8]]
    if c.empty is not None:
        r0, s0 = c.empty
        assert bool((c.got[r0 * S + s0] == 0).all()), "a query that sees no key must return exact zeros"


@pytest.mark.parametrize("shape", [(1, 1, 0, 64, 2, 1), (2, 130, 0, 192, 12, 2)], ids=lambda s: "x".join(map(str, s)))
def test_p0_is_a_plain_causal_prefill(dev, shape):
    """P = 0: the same problem ops.attn_fwd solves under mask_causal, within the same bars (both against fp32, and the pair) -- and
    the same bits: both shapes have L < 256, where ops.attn_fwd runs attn_fwd_kernel<4>, whose flash step attn_prefill_cached_kernel
    repeats operation for operation (only the mask bit is obtained differently), so an edit to one copy alone shows here."""
    c = _case(shape, "none", dev)
    assert _rel(c.got, c.ref) < FWD_BAR and _rel(c.square, c.ref) < FWD_BAR
    assert _rel(c.got, c.square) < FWD_BAR, _rel(c.got, c.square)
    assert torch.equal(c.got, c.square), f"{int((c.got != c.square).sum())} of {c.got.numel()} elements differ"
    e, e_row = _row_errs(c.got, c.ref), _row_errs(c.square, c.ref)
    assert bool((e <= torch.clamp(ROW_SPREAD * e_row, min=FWD_BAR)).all())


@pytest.mark.parametrize("mode", MODES)
def test_two_runs_are_bit_equal(dev, mode):
    from unigen_hip import ops
    shape = (3, 40, 507, 560, 12, 2)
    c = _case(shape, mode, dev)
    rows, S, P, Tmax, H, HKV = shape
    a = ops.attn_prefill_cached(c.qd, c.Kd, c.Vd, c.kvd, S, P, H, HKV, HD, Tmax)
    b = ops.attn_prefill_cached(c.qd, c.Kd, c.Vd, c.kvd, S, P, H, HKV, HD, Tmax)
    assert torch.equal(a, b) and torch.equal(a.float().cpu(), c.got)


def test_wrapper_refuses_without_launching(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    rows, S, P, Tmax, H, HKV = 2, 5, 60, 64, 2, 1
    K = torch.zeros(rows, HKV, Tmax, HD, dtype=BF, device=dev)
    q = torch.zeros(rows * S, H * HD, dtype=BF, device=dev)
    out = torch.full((rows * S, H * HD), 7.0, dtype=BF, device=dev)
    with pytest.raises(UniGenHipError, match="Tmax"):
        ops.attn_prefill_cached(q, K, K, None, S, P, H, HKV, HD, Tmax, out=out)              # 60 + 5 > 64
    K64 = torch.zeros(rows, HKV, Tmax, 64, dtype=BF, device=dev)
    q64 = torch.zeros(rows * S, H * 64, dtype=BF, device=dev)
    with pytest.raises(UniGenHipError):
        ops.attn_prefill_cached(q64, K64, K64, None, S, 0, H, HKV, 64, Tmax, out=out)        # head_dim 64
    K2 = torch.zeros(rows, 2, Tmax, HD, dtype=BF, device=dev)
    q3 = torch.zeros(rows * S, 3 * HD, dtype=BF, device=dev)
    with pytest.raises(UniGenHipError, match="multiple"):
        ops.attn_prefill_cached(q3, K2, K2, None, S, 0, 3, 2, HD, Tmax, out=out)             # H = 3 over HKV = 2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
