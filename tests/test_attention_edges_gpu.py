"""Training / prefill attention (csrc/attention.hip: ug_attn_fwd, ug_attn_bwd) at the edges its two tests in test_kernels_gpu.py
never reach: query rows that see no key, keys no query sees, hidden tiles in the middle and at the start of a row's range, whole
hidden query / key tiles, and every kernel the launcher can choose -- against `attention_masked_ref` (oracle/ops_ref.py) in
float64, judged per (batch, head, row) so that an error confined to the few live rows of a ragged tile is not diluted.

The contract checked here is the one written at ug_attn_fwd / ug_attn_bwd in include/unigen_hip.h:
  * a query row that sees no key: o = 0 (bit for bit), lse = +inf, dq = 0, nothing added to dk / dv;
  * a key no query sees: dk = dv = 0;
  * every element of o, lse and dq | dk | dv is written (the outputs are pre-filled with NaN here);
  * the q / dO rows of empty query rows and the k / v rows of never-seen keys may hold any FINITE values without changing a bit of
    any other row.  They may not hold NaN / Inf: the kernels multiply those rows by exact-zero probabilities in the matrix cores
    (attn_fwd_kernel stages every V row of a visible tile and contracts it with the packed probabilities of all 64 query rows),
    and 0 * NaN = NaN.  The product never puts a non-finite value there -- an empty row leaves the layer as o = 0, so the next
    layer's q / k / v of that row are finite.  (The issue's stronger form, NaN sentinels, was weighed against zeroing the staged
    rows: docs/experiments.md, "Attention edge tests".)
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(HD)
BAR = 1e-2                 # per (row, query head) relative error of a bf16 attention output against fp64: BAR of test_decode_parity_gpu.py
FWD_WHOLE, GRAD_WHOLE = 8e-3, 2e-2       # the whole-tensor bars of test_attention_fwd_bwd
# Per-row bars of dq / dk / dv: 4 x the worst per-row error (`row_denominators`) of `backward_restatement` below -- float64 arithmetic
# that keeps the kernels' rounding points: P and dS rounded to bf16 before their contractions, delta from the bf16 o, bf16 outputs --
# against the float64 reference, over every (shape, kind) of SHAPES x KINDS on these tests' own inputs (docs/experiments.md).
# Measured worst: dq 3.50e-2 at (22, 256, 12, 2) band_sink, dk 9.08e-3 at (3, 200, 4, 4) band, dv 4.31e-3 at (3, 200, 4, 4) leftpad.
GRAD_ROW_BAR = {"dq": 4 * 3.50e-2, "dk": 4 * 9.08e-3, "dv": 4 * 4.31e-3}
LSE_FACTOR = 8             # lse: absolute error <= 8 x the error of an fp32 evaluation of the same formula on the same inputs

# (B, L, H, HKV) -> the kernels ug_attn_fwd / ug_attn_bwd select (conditions as they stand in csrc/attn_plan.h;
# nW = ceil(L / 64) key tiles, nT = ceil(L / 128) 128-row query tiles, G = H / HKV):
#   32-row forward and dQ kernels:  256 <= L <= 4096 and nT * H * B >= 512; 8-wave forward: L > 4096 and nT * H * B >= 512
#   two heads per dK/dV workgroup:  G even and nW * (H / 2) * B >= 1024;  DMA dK/dV: L <= 4096
#   fused dK/dV finish:             rope / dbias given and HKV a power of two (<= 16)
SHAPES = [
    (2, 70, 2, 1),       # L < 256: 64-row fwd (attn_fwd_kernel<4>), 16-row dQ, DMA dK/dV, 2 * 1 * 2 = 4 < 1024: one head per workgroup
    (3, 129, 6, 2),      # same kernels; nW = 3 with one live key in the last tile; 3 * 3 * 3 = 27 < 1024
    (29, 129, 24, 4),    # same fwd / dQ (L < 256), but 3 * 12 * 29 = 1044 >= 1024: two heads per dK/dV workgroup at small L
    (35, 260, 12, 2),    # nT = 3: 3 * 12 * 35 = 1260 >= 512 -> 32-row fwd + dQ (first end-aligned tile: rows -124 .. 3, 4 live);
                         # nW = 5: 5 * 6 * 35 = 1050 >= 1024 -> two heads per DMA dK/dV workgroup; fused finish: the benchmark's set
    (22, 256, 12, 2),    # nT = 2: 2 * 12 * 22 = 528 >= 512 -> 32-row kernels exactly at L = 256 (no ragged tile); 4 * 6 * 22 = 528: one head
    (22, 257, 12, 2),    # nT = 3: 792 >= 512 -> 32-row kernels, first tile has ONE live row; 5 * 6 * 22 = 660 < 1024: one head
    (3, 200, 4, 4),      # G = 1: no split workspace, attn_bwd_dkv_kernel<false>; 64-row fwd, 16-row dQ
    (13, 260, 28, 4),    # G = 7 (the 7B ratio) is odd: two heads per dK/dV workgroup do not divide it -> one; 3 * 28 * 13 = 1092 >= 512: 32-row fwd + dQ
    (4, 130, 6, 3),      # HKV = 3, not a power of two: generic dkv_finish_kernel + stand-alone RoPE / column-sum passes
]
# device-fp32 reference, head by head; `leftpad` and `band_sink` only
BIG_SHAPES = [
    (1, 4096, 16, 2),    # nT = 32: 32 * 16 = 512 >= 512 -> 32-row kernels at nW = 64: bit 63 of the vis / minem words; 64 * 8 = 512: one head
    (1, 4160, 16, 2),    # L > 4096, nT = 33: 528 >= 512 -> attn_fwd_kernel<8>, 16-row dQ, non-DMA split attn_bwd_dkv_kernel<true>
]
# The comments above as data, held against csrc/attn_plan.h by tests/test_attn_plan_cpu.py (which also requires that the two lists
# together reach every kernel and finish the plan can return): forward, dQ and dK/dV kernel, query heads per dK/dV workgroup
# (0: the kernel without a split workspace does not read it), and the dK/dV finish when RoPE tables or dbias are given.  The
# workspace is there when H > HKV (ops.attn_bwd).
FWD64, FWD128, FWD32 = "attn_fwd_kernel<4>", "attn_fwd_kernel<8>", "attn_fwd32_kernel<4>"
DQ16, DQ32 = "attn_bwd_dq_kernel", "attn_bwd_dq32_kernel<4>"
DKV_DMA, DKV_SPLIT, DKV_WHOLE = "attn_bwd_dkv_dma_kernel", "attn_bwd_dkv_kernel<true>", "attn_bwd_dkv_kernel<false>"
FIN_ROPE, FIN_PLAIN = "dkv_finish_rope_kernel", "dkv_finish_kernel"
KERNELS = {
    (2, 70, 2, 1): dict(fwd=FWD64, dq=DQ16, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (3, 129, 6, 2): dict(fwd=FWD64, dq=DQ16, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (29, 129, 24, 4): dict(fwd=FWD64, dq=DQ16, dkv=DKV_DMA, heads=2, finish=FIN_ROPE),
    (35, 260, 12, 2): dict(fwd=FWD32, dq=DQ32, dkv=DKV_DMA, heads=2, finish=FIN_ROPE),
    (22, 256, 12, 2): dict(fwd=FWD32, dq=DQ32, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (22, 257, 12, 2): dict(fwd=FWD32, dq=DQ32, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (3, 200, 4, 4): dict(fwd=FWD64, dq=DQ16, dkv=DKV_WHOLE, heads=0, finish=None),
    (13, 260, 28, 4): dict(fwd=FWD32, dq=DQ32, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (4, 130, 6, 3): dict(fwd=FWD64, dq=DQ16, dkv=DKV_DMA, heads=1, finish=FIN_PLAIN),
    (1, 4096, 16, 2): dict(fwd=FWD32, dq=DQ32, dkv=DKV_DMA, heads=1, finish=FIN_ROPE),
    (1, 4160, 16, 2): dict(fwd=FWD128, dq=DQ16, dkv=DKV_SPLIT, heads=1, finish=FIN_ROPE),
}
KINDS = ["leftpad", "band_sink", "band", "holes"]
PADS = [130, 0, 1, 63, 64, 65, 2, 5, 17, 31, 3, 7]            # left-pad counts per batch row (clamped to L - 1), cycled


def _ops():
    from unigen_hip import ops
    return ops


def edge_allow(B, L, kind, gen):
    """-> (allow [B, L, L] bool, key_valid [B, L] bool or None).  Seeded by `gen`."""
    tril = torch.tril(torch.ones(L, L, dtype=torch.bool))
    r, c = torch.arange(L)[:, None], torch.arange(L)[None, :]
    allow = torch.zeros(B, L, L, dtype=torch.bool)
    key_valid = None
    if kind == "leftpad":                # what DecodeEngine.prefill builds: causal AND key_valid; every row t < npad is empty
        key_valid = torch.ones(B, L, dtype=torch.bool)
        for b in range(B):
            key_valid[b, :min(PADS[b % len(PADS)], L - 1)] = False
        allow = tril[None] & key_valid[:, None, :]
    elif kind == "band_sink":            # tile 0 visible, middle tiles hidden, the band visible again
        allow[:] = tril & ((r - c < 70) | (c < 4))
    elif kind == "band":                 # the first visible tile is not tile 0
        allow[:] = tril & (r - c < 70)
    elif kind == "holes":
        nfull = max(L // 64, 1)
        off = L - ((L + 127) // 128) * 128              # the 32-row kernels align their 128-row query tiles to the END of the sequence
        for b in range(B):
            a = torch.rand(L, L, generator=gen) < 0.3
            a[torch.arange(L), torch.arange(L)] = True
            a[torch.rand(L, generator=gen) < 0.05] = False                   # ~5 % of the rows see nothing
            qt = (b + 1) % nfull
            a[qt * 64:(qt + 1) * 64] = False                                 # one whole 64-row query tile sees nothing
            if L >= 256:
                t128 = 1 + b % ((L + 127) // 128 - 1)
                a[max(off + t128 * 128, 0):off + (t128 + 1) * 128] = False   # one whole 128-row tile (as those kernels cut them)
            a[:, torch.rand(L, generator=gen) < 0.05] = False                # ~5 % of the keys are seen by nobody
            kt = b % nfull
            a[:, kt * 64:(kt + 1) * 64] = False                              # one whole 64-key tile is seen by nobody
            allow[b] = a
    else:
        raise ValueError(kind)
    return allow, key_valid


def split_heads(x, B, L, H, HKV):
    """[B*L, (H + 2 HKV) * 128] -> q [B,H,L,d], k, v [B,HKV,L,d] (views)"""
    q = x[:, : H * HD].view(B, L, H, HD).permute(0, 2, 1, 3)
    k = x[:, H * HD:(H + HKV) * HD].view(B, L, HKV, HD).permute(0, 2, 1, 3)
    v = x[:, (H + HKV) * HD:].view(B, L, HKV, HD).permute(0, 2, 1, 3)
    return q, k, v


def make_inputs(shape, kind):
    B, L, H, HKV = shape
    gen = torch.Generator().manual_seed(1000 * B + L + 7 * H + 100003 * KINDS.index(kind))
    allow, key_valid = edge_allow(B, L, kind, gen)
    qkv = torch.randn(B * L, (H + 2 * HKV) * HD, generator=gen).to(BF)
    dout = torch.randn(B * L, H * HD, generator=gen).to(BF)
    return qkv, dout, allow, key_valid


def backward_restatement(qkv, dout, allow, shape):
    """The backward in float64 with the kernels' rounding points (the measurement behind GRAD_ROW_BAR): probabilities rounded to bf16
    for the P.V and P^T.dO contractions, delta from the bf16 o, dS rounded to bf16 before dS.K and dS^T.Q, bf16 outputs."""
    B, L, H, HKV = shape
    G = H // HKV
    rnd = lambda t: t.to(BF).double()
    q, k, v = (t.double() for t in split_heads(qkv, B, L, H, HKV))
    do = dout.view(B, L, H, HD).permute(0, 2, 1, 3).double()
    kr, vr = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    a = allow[:, None]
    live = a.any(-1, keepdim=True)
    s = torch.where(a, q @ kr.transpose(2, 3) * SCALE, torch.full((), float("-inf"), dtype=torch.float64))
    m = torch.where(live, s.amax(-1, keepdim=True), torch.zeros((), dtype=torch.float64))
    e = torch.exp(s - m)
    l = torch.where(live, e.sum(-1, keepdim=True), torch.ones((), dtype=torch.float64))
    o = rnd((rnd(e) @ vr) / l)
    P = e / l
    dS = rnd(P * (do @ vr.transpose(2, 3) - (do * o).sum(-1, keepdim=True)))
    dq = rnd(SCALE * dS @ kr)
    dk = rnd(SCALE * (dS.transpose(2, 3) @ q).view(B, HKV, G, L, HD).sum(2))
    dv = rnd((rnd(P).transpose(2, 3) @ do).view(B, HKV, G, L, HD).sum(2))
    return o, dq, dk, dv


def row_sets(allow):
    """-> empty [B,L] (query rows that see nothing), unseen [B,L] (keys nobody sees), one_key [B,L] (rows with exactly one key: dq = 0
    analytically), dk_zero [B,L] (seen keys all of whose viewers are one-key rows: dk = 0 analytically)."""
    nk = allow.sum(-1)
    empty, one_key = nk == 0, nk == 1
    unseen = ~allow.any(1)
    dk_zero = ~unseen & ~(allow & ~one_key[:, :, None]).any(1)
    return empty, unseen, one_key, dk_zero


def row_err(got, ref):
    """relative error of every row (last dimension) of got against ref, in float64"""
    g, r = got.double().cpu(), ref.double().cpu()
    return (g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _reference_cpu(qkv, dout, allow, shape):
    from oracle.ops_ref import attention_masked_ref
    B, L, H, HKV = shape
    q, k, v = (t.double().clone().requires_grad_(True) for t in split_heads(qkv, B, L, H, HKV))
    o, lse = attention_masked_ref(q, k, v, allow, SCALE)
    o.backward(dout.view(B, L, H, HD).permute(0, 2, 1, 3).double())
    with torch.no_grad():
        q32, k32, v32 = split_heads(qkv.float(), B, L, H, HKV)
        _, lse32 = attention_masked_ref(q32, k32, v32, allow, SCALE, dtype=torch.float32)
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad, lse32.double()


def _reference_device(qkv, dout, allow, shape, dev):
    """The same formula in fp32 on the device, head by head (one [L, L] score matrix at a time); lse also in fp64 (forward only), so
    that the fp32 evaluation's own error is known."""
    from oracle.ops_ref import attention_masked_ref
    B, L, H, HKV = shape
    G = H // HKV
    q, k, v = split_heads(qkv.to(dev), B, L, H, HKV)
    do = dout.to(dev).view(B, L, H, HD).permute(0, 2, 1, 3)
    al = allow.to(dev)
    o, dq = torch.empty(B, H, L, HD, device=dev), torch.empty(B, H, L, HD, device=dev)
    dk, dv = torch.zeros(B, HKV, L, HD, device=dev), torch.zeros(B, HKV, L, HD, device=dev)
    lse64, lse32 = torch.empty(B, H, L, dtype=torch.float64, device=dev), torch.empty(B, H, L, dtype=torch.float64, device=dev)
    for h in range(H):
        hk = h // G
        qh, kh, vh = (t.float().clone().requires_grad_(True) for t in (q[:, h:h + 1], k[:, hk:hk + 1], v[:, hk:hk + 1]))
        oh, lh = attention_masked_ref(qh, kh, vh, al, SCALE, dtype=torch.float32)
        oh.backward(do[:, h:h + 1].float())
        o[:, h], dq[:, h], lse32[:, h] = oh.detach()[:, 0], qh.grad[:, 0], lh.detach()[:, 0].double()
        dk[:, hk] += kh.grad[:, 0]
        dv[:, hk] += vh.grad[:, 0]
        with torch.no_grad():
            lse64[:, h] = attention_masked_ref(q[:, h:h + 1], k[:, hk:hk + 1], v[:, hk:hk + 1], al, SCALE)[1][:, 0]
        del qh, kh, vh, oh, lh
    return tuple(t.cpu().double() for t in (o, lse64, dq, dk, dv, lse32))


@functools.lru_cache(maxsize=2)
def case(shape, kind, dev_str=None):
    """inputs + reference of one (shape, kind), computed once and shared by the tests that need it (never modified)"""
    qkv, dout, allow, key_valid = make_inputs(shape, kind)
    if dev_str is None:
        ref = _reference_cpu(qkv, dout, allow, shape)
    else:
        ref = _reference_device(qkv, dout, allow, shape, torch.device(dev_str))
    names = ("o", "lse", "dq", "dk", "dv", "lse32")
    return dict(zip(names, ref), qkv=qkv, dout=dout, allow=allow, key_valid=key_valid)


def build_mask(ops, c, shape, dev):
    """the compressed mask of a case; `leftpad` goes through ops.mask_causal(key_valid=...), as DecodeEngine.prefill does, and must
    equal ops.mask_compress of the dense equivalent word for word"""
    B, L = shape[:2]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    mb = ops.mask_compress(c["allow"].to(dev), err)
    assert err.item() == 0
    if c["key_valid"] is not None:
        mc = ops.mask_causal(B, L, dev, key_valid=c["key_valid"].to(dev))
        assert torch.equal(mc.bits, mb.bits) and torch.equal(mc.tileany, mb.tileany)
        mb = mc
    return mb


def rope_tables(L, dev):
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.float32) / HD))
    ang = torch.arange(L, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)


def run_kernels(ops, qkv, dout, mb, shape, dev, fused=True):
    """forward + the backward variants, every output pre-filled with NaN -> dict of device tensors"""
    B, L, H, HKV = shape
    W = (H + 2 * HKV) * HD
    o = torch.full((B * L, H * HD), float("nan"), dtype=BF, device=dev)
    lse = torch.full((B, H, L), float("nan"), dtype=torch.float32, device=dev)
    ops.attn_fwd(qkv, mb, H, HKV, HD, out=(o, lse))
    out = {"o": o, "lse": lse}
    variants = [("det", False, False), ("split", True, False)]
    if fused:
        variants += [("det_rope", False, True), ("split_rope", True, True)]
    for name, split, fuse in variants:
        g = torch.full((B * L, W), float("nan"), dtype=BF, device=dev)
        kw = {}
        if fuse:
            out[name + "_bias"] = kw["dbias"] = torch.zeros(W, device=dev)
            kw["rope"] = rope_tables(L, dev)
        ops.attn_bwd(qkv, o, lse, dout, mb, H, HKV, HD, split_heads=split, out=g, **kw)
        assert float(ops._dkv_workspace(B * L, 2 * HKV * HD, dev).abs().max()) == 0.0, name
        out[name] = g
    return out


def check_exact(res, shape, empty, unseen):
    """finite everywhere; empty rows: o == 0 bit for bit, lse == +inf, dq == 0; unseen keys: dk == dv == 0 -- in every variant"""
    B, L, H, HKV = shape
    o = res["o"].cpu().view(B, L, H * HD)
    lse = res["lse"].cpu()
    assert torch.isfinite(o.float()).all()
    assert (o.view(torch.int16)[empty] == 0).all(), "o of a row that sees no key"
    em = empty[:, None, :].expand(B, H, L)
    assert (lse[em] == float("inf")).all() and torch.isfinite(lse[~em]).all()
    for name in ("det", "split", "det_rope", "split_rope"):
        if name not in res:
            continue
        g = res[name].cpu().float().view(B, L, -1)
        assert torch.isfinite(g).all(), name
        assert (g[:, :, : H * HD][empty] == 0).all(), f"{name}: dq of a row that sees no key"
        assert (g[:, :, H * HD:][unseen] == 0).all(), f"{name}: dk / dv of a key no query sees"
        if name + "_bias" in res:
            assert torch.isfinite(res[name + "_bias"]).all()


def row_denominators(ref, name, sets):
    """-> (denominator [B,h,L] of the per-row error of gradient `name`, judged rows [B,h,L]).  dk and dv rows are judged relative to
    their own norm.  A dq row is judged relative to max(own norm, median row norm): dq = scale * sum_k dS_k K_k with
    dS_k = P_k (dP_k - delta) cancels when a row sees few keys (exactly to zero with one key, nearly when one of two or three keys
    takes most of the probability), while the rounding of delta (from the bf16 o) and of dS to bf16 is proportional to the terms
    P_k dP_k, not to their cancelled sum -- the restatement's own error on such rows reaches 15 x their norm.  Seen keys all of whose
    viewers are one-key rows have dk = 0 analytically and are judged against the median as well."""
    empty, unseen, one_key, dk_zero = sets
    B, nh, L = ref.shape[:3]
    norms = ref.norm(dim=-1)
    ex = lambda m: m[:, None, :].expand(B, nh, L)
    if name == "dq":
        judged = ~ex(empty)
        med = norms[judged & ~ex(one_key)].median()
        return torch.maximum(norms, med), judged
    judged = ~ex(unseen)
    if name == "dk":
        med = norms[judged & ~ex(dk_zero)].median()
        return torch.where(ex(dk_zero), med, norms), judged
    return norms, judged


def grad_row_errors(g, c, shape, sets):
    """-> {dq, dk, dv: (worst per-row error, whole-tensor relative error)} of a stored dqkv against the reference"""
    B, L, H, HKV = shape
    found = {}
    for name, got in zip(("dq", "dk", "dv"), split_heads(g.cpu().float().view(B * L, -1), B, L, H, HKV)):
        ref = c[name]
        den, judged = row_denominators(ref, name, sets)
        found[name] = (((got.double() - ref).norm(dim=-1) / den)[judged].max().item(), _rel(got, ref))
    return found


def poisoned(qkv, dout, shape, empty, unseen, gen):
    """finite garbage (|x| ~ 100) in the q and dO rows of empty query rows and the k / v rows of never-seen keys"""
    B, L, H, HKV = shape
    q2, d2 = qkv.clone().view(B, L, -1), dout.clone().view(B, L, -1)
    junk = lambda n, w: (torch.randn(n, w, generator=gen) * 100).to(BF)
    q2[:, :, : H * HD][empty] = junk(int(empty.sum()), H * HD)
    d2[empty] = junk(int(empty.sum()), H * HD)
    q2[:, :, H * HD:][unseen] = junk(int(unseen.sum()), 2 * HKV * HD)
    return q2.view(B * L, -1), d2.view(B * L, -1)


def _check_case(dev, shape, kind, on_device=False):
    ops = _ops()
    B, L, H, HKV = shape
    c = case(shape, kind, str(dev) if on_device else None)
    sets = row_sets(c["allow"])
    empty, unseen, one_key, _ = sets
    if kind == "leftpad":
        assert empty.any() and unseen.any()
    mb = build_mask(ops, c, shape, dev)
    qkv, dout = c["qkv"].to(dev), c["dout"].to(dev)
    res = run_kernels(ops, qkv, dout, mb, shape, dev)
    check_exact(res, shape, empty, unseen)
    tag = f"    attention edges B={B} L={L} H={H}/{HKV} {kind}:"

    # forward: per (b, h, row) and whole tensor
    got_o = res["o"].cpu().view(B, L, H, HD).permute(0, 2, 1, 3)
    live = ~empty[:, None, :].expand(B, H, L)
    e_o = row_err(got_o, c["o"])[live].max().item()
    yard = (c["lse32"] - c["lse"])[live].abs().max().item()
    e_lse = (res["lse"].cpu().double() - c["lse"])[live].abs().max().item()
    print(f"{tag} {int(empty.sum())} empty rows, {int(unseen.sum())} unseen keys, {int(one_key.sum())} one-key rows; "
          f"o worst row {e_o:.3e} whole {_rel(got_o, c['o']):.3e}; lse abs {e_lse:.3e} (fp32 evaluation {yard:.3e})")
    assert e_o <= BAR
    assert _rel(got_o, c["o"]) < FWD_WHOLE
    assert e_lse <= LSE_FACTOR * yard, (e_lse, yard)

    # gradients: whole tensor, per row, analytically-zero rows
    for name in ("det", "split"):
        found = grad_row_errors(res[name], c, shape, sets)
        print(f"{tag} {name}: " + "; ".join(f"{k} worst row {v[0]:.3e} whole {v[1]:.3e}" for k, v in found.items()))
        for k, (worst, whole) in found.items():
            assert whole < GRAD_WHOLE, (name, k, whole)
            assert worst <= GRAD_ROW_BAR[k], (name, k, worst)

    # sentinels: finite garbage in the rows nothing may read into a result leaves every other row's bits unchanged
    q2, d2 = poisoned(c["qkv"], c["dout"], shape, empty, unseen, torch.Generator().manual_seed(L + 13 * B))
    res2 = run_kernels(ops, q2.to(dev), d2.to(dev), mb, shape, dev, fused=False)
    check_exact(res2, shape, empty, unseen)
    assert torch.equal(res2["o"], res["o"])
    assert torch.equal(res2["lse"], res["lse"])
    nq = H * HD
    assert torch.equal(res2["det"], res["det"])                             # deterministic kernels: dq | dk | dv bit for bit
    assert torch.equal(res2["split"][:, :nq], res["split"][:, :nq])         # split dK / dV carry the fp32 atomics' order
    assert _rel(res2["split"][:, nq:], res["det"][:, nq:]) < 4e-3 and _rel(res["split"][:, nq:], res["det"][:, nq:]) < 4e-3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_edges(dev, shape, kind):
    """Every kernel choice of the launcher x every mask kind against float64 on the CPU: exact zeros / +inf for empty rows and unseen
    keys, NaN-prefilled outputs, garbage sentinels, per-row forward, lse and gradient bars (module docstring)."""
    _check_case(dev, shape, kind)


@pytest.mark.parametrize("kind", ["leftpad", "band_sink"])
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_edges_long(dev, shape, kind):
    """L = 4096 (nW = 64: the 64-bit tile words full to bit 63) and L = 4160 (the kernels only L > 4096 selects), against the same
    formula in fp32 on the device, head by head (as test_gemm_bf16_long_contraction_few_tiles keeps its reference on the device)."""
    _check_case(dev, shape, kind, on_device=True)
    case.cache_clear()


def test_edge_bars_reject_subtly_wrong_references(dev):
    """The per-row bars catch a subtly wrong kernel at the benchmark's kernel set, (35, 260, 12, 2): the kernels' output holds the
    bars against the true reference and misses each of four wrong references by >= 3 x the bar in its worst row."""
    from oracle.ops_ref import attention_masked_ref
    ops = _ops()
    shape = (35, 260, 12, 2)
    B, L, H, HKV = shape
    found = {}

    def run(kind, wrong_mask=None, q_wrong=None, uniform_empty=False, n=4):
        """worst per-row errors of the kernels' o / dq / dk / dv on the first n batch rows against their true float64 reference and
        against one computed from a wrong mask, a wrong Q, or with empty rows attending uniformly"""
        qkv, dout, allow, key_valid = make_inputs(shape, kind)
        sets = tuple(t[:n] for t in row_sets(allow))
        mb = build_mask(ops, {"allow": allow, "key_valid": key_valid}, shape, dev)
        res = run_kernels(ops, qkv.to(dev), dout.to(dev), mb, shape, dev, fused=False)
        sub = (n, L, H, HKV)
        do = dout.view(B, L, H, HD).permute(0, 2, 1, 3)[:n].double()

        def reference(a, qmap):
            q, k, v = (t[:n].double().clone().requires_grad_(True) for t in split_heads(qkv, B, L, H, HKV))
            o, _ = attention_masked_ref(qmap(q), k, v, a, SCALE)
            o.backward(do)
            return {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
        true = reference(allow[:n], lambda q: q)
        a = (allow if wrong_mask is None else wrong_mask(allow.clone()))[:n]
        if uniform_empty:                                   # a finite-minimum additive mask: an all-blocked row is a uniform one
            a = a | ~a.any(-1, keepdim=True)
        wrong = reference(a, q_wrong or (lambda q: q))
        got = dict(zip(("dq", "dk", "dv"), split_heads(res["split"].cpu().float().view(B, L, -1)[:n].reshape(n * L, -1), *sub)))
        got["o"] = res["o"].cpu().view(B, L, H, HD).permute(0, 2, 1, 3)[:n]
        errs = {}
        for kk in ("o", "dq", "dk", "dv"):                  # judged on the rows and by the denominators of the TRUE reference
            if kk == "o":
                den, keep = true["o"].norm(dim=-1), ~sets[0][:, None, :].expand(n, H, L)
            else:
                den, keep = row_denominators(true[kk], kk, sets)
            errs[kk] = tuple(((got[kk].double() - r[kk]).norm(dim=-1) / den)[keep].max().item() for r in (true, wrong))
        return errs

    # band_sink: rows 200.. see keys 0..3 and row - 69 .. row; key tile 1 (keys 64..127) is hidden from them, tile 3 (192..255) visible
    def show(a):
        a[:, 200:, 64:128] = True
        return a

    def drop(a):
        a[:, 200:, 192:256] = False
        return a
    found["a hidden middle tile made visible (band_sink)"] = run("band_sink", wrong_mask=show)
    found["a visible tile dropped (band_sink)"] = run("band_sink", wrong_mask=drop)

    def first_heads_q(q):                                    # the second query head of every pair reads the first head's Q
        q2 = q.clone()
        q2[:, 1::2] = q[:, 0::2]
        return q2
    found["second head of a pair given the first head's Q (holes)"] = run("holes", q_wrong=first_heads_q)
    found["empty rows attend uniformly (leftpad)"] = run("leftpad", uniform_empty=True)
    bars = dict(GRAD_ROW_BAR, o=BAR)
    expect = {"a hidden middle tile made visible (band_sink)": ("o", "dq", "dk", "dv"),
              "a visible tile dropped (band_sink)": ("o", "dq", "dk", "dv"),
              "second head of a pair given the first head's Q (holes)": ("o", "dk", "dv"),
              "empty rows attend uniformly (leftpad)": ("dk", "dv")}
    for name, errs in found.items():
        print(f"    {name}: " + "; ".join(f"{k} true {t:.3e} wrong {w:.3e} (bar {bars[k]:.1e})" for k, (t, w) in errs.items()))
    for name, errs in found.items():
        for k, (t, w) in errs.items():
            assert t <= bars[k], (name, k, t)
        for k in expect[name]:
            assert errs[k][1] >= 3 * bars[k], (name, k, errs[k][1])
    # the empty rows themselves: the kernels write o = 0 (test_attention_edges); the uniform reference has |o| > 0 there: a miss of 100 %
    qkv, _, allow, _ = make_inputs(shape, "leftpad")
    empty = row_sets(allow)[0][:4]
    q, k, v = (t[:4] for t in split_heads(qkv, B, L, H, HKV))
    o_uni = attention_masked_ref(q, k, v, allow[:4] | ~allow[:4].any(-1, keepdim=True), SCALE)[0]
    assert empty.any() and (o_uni.norm(dim=-1)[empty[:, None, :].expand(4, H, L)] > 0).all()


@pytest.mark.parametrize("kind", ["leftpad", "holes"])
@pytest.mark.parametrize("B,L,H,HKV,split", [(35, 260, 12, 2, True), (29, 129, 24, 4, True), (4, 130, 6, 3, True), (4, 130, 6, 3, False),
                                             (35, 260, 12, 2, False)])
def test_attention_bwd_fused_rope_and_bias_sums_at_edge_masks(dev, B, L, H, HKV, split, kind):
    """The identities of test_attention_bwd_fused_rope_and_bias_sums (test_kernels_gpu.py) with empty rows and unseen keys: RoPE
    transposed and the bias sums applied where dq / dk / dv are stored == the stand-alone passes over the stored tensor.  The `plain`
    result at these shapes is pinned to the float64 reference by test_attention_edges."""
    ops = _ops()
    shape = (B, L, H, HKV)
    qkv, dout, allow, key_valid = make_inputs(shape, kind)
    c = {"allow": allow, "key_valid": key_valid}
    mb = build_mask(ops, c, shape, dev)
    qkv, dout = qkv.to(dev), dout.to(dev)
    o, lse = ops.attn_fwd(qkv, mb, H, HKV, HD)
    cos, sin = rope_tables(L, dev)
    W = (H + 2 * HKV) * HD
    plain = ops.attn_bwd(qkv, o, lse, dout, mb, H, HKV, HD, split_heads=split)
    want = plain.clone()
    ops.rope_(want, cos, sin, L, H + HKV, HD, backward=True)
    want_b = torch.zeros(W, device=dev)
    ops.colsum_(want, want_b)
    got_b = torch.full((W,), 0.25, device=dev)                                   # accumulates into what is there
    got = ops.attn_bwd(qkv, o, lse, dout, mb, H, HKV, HD, split_heads=split, rope=(cos, sin), dbias=got_b)
    nq = H * HD
    assert torch.equal(got[:, :nq], want[:, :nq])                                # dq: deterministic kernels
    if split:
        assert _rel(got[:, nq:], want[:, nq:]) < 4e-3                            # fp32 atomics order before the bf16 rounding
        ref_b = torch.zeros_like(want_b)
        ops.colsum_(got, ref_b)                                                  # the sums of what THIS run stored
    else:
        assert torch.equal(got[:, nq:], want[:, nq:])
        ref_b = want_b
    eb = (got_b - 0.25 - ref_b).abs().max().item()
    print(f"    fused RoPE / bias sums B={B} L={L} H={H}/{HKV} split={split} {kind}: bias-gradient max diff {eb:.2e} at max {ref_b.abs().max().item():.1f}")
    assert eb < 2e-4 * max(1.0, ref_b.abs().max().item())
    assert float(ops._dkv_workspace(B * L, 2 * HKV * HD, dev).abs().max()) == 0.0
