"""Decode step against references at the shapes the product reaches: past 512 cached keys, whole blank chunks, odd layer counts.

Kernel level  the fused cache attention (ug_attn_decode_fused, its ordered form fed with six slots, and the unfused ug_attn_decode on
              the bounds checks) against an fp64 restatement that keeps the kernel's documented rounding points (csrc/decode.hip,
              attn_decode_fused_kernel: q/k/v = bf16(rstd * acc + bias), RoPE with separately rounded products), at the 64-key chunk
              edges, the 512-key edge where a wave starts its second pass and a third pass at 1 500 keys; cache writes byte for byte;
              nothing at or past the write position may reach the output; the 1e-2 bar is shown to reject subtly wrong references.
Engine level  a 3-layer model at the 1.5B width (odd depth: the single-writer layer's down-projection accumulators alternate by layer)
              through every decode form for 8 steps, against oracle.qwen2_ref stepped through its concatenating cache.
Model level   t2i_generate_ar on the same model against ar_generate_ref, eager / captured / kept session."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import YARDSTICK, fp32_yardstick, llm_config_dir

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HD = 128
NORM_COLS, EPS = 1536, 1e-6
BAR = 1e-2                      # per (row, query head) relative error against fp64: the bar of test_attn_decode_matches_reference
GUARD = 4096                    # elements after the cache / output views that no launch may touch


# ====================================================================================== kernel level
def _bf(t):
    return t.to(BF).float()


def _seq(parts):
    """ascending slot order, fp32 (the ordered kernel's documented sum)"""
    acc = parts[0].clone()
    for p in range(1, parts.shape[0]):
        acc += parts[p]
    return acc


def _finish_ref(acc, ss, bias, cos, sin, rpos, Hq, Hk):
    """The new token's q [R, Hq, 128], k / v [R, Hk, 128] (bf16 values, fp32) as the kernel builds them from the raw accumulator:
    bf16(rstd * acc + bias), then rotate-half RoPE at rpos with separately rounded fp32 products (q and k only)."""
    R = acc.shape[0]
    rs = torch.rsqrt(ss[:R].double() / NORM_COLS + EPS).float()[:, None]
    x = _bf(rs * acc + bias.float())
    q, k, v = x[:, :Hq * HD].view(R, Hq, HD), x[:, Hq * HD:(Hq + Hk) * HD].view(R, Hk, HD), x[:, (Hq + Hk) * HD:].view(R, Hk, HD)
    c, s = cos[rpos], sin[rpos]

    def rot(t):
        x1, x2 = t[..., :HD // 2], t[..., HD // 2:]
        return torch.cat([_bf(x1 * c - x2 * s), _bf(x2 * c + x1 * s)], -1)
    return rot(q), rot(k), v


def _attend_ref(q, kn, vn, K, V, vis, with_new=True):
    """fp64 softmax attention of q [R, Hq, D] over the cache keys `vis` [R, T] allows (K / V [R, Hk, T, D]) + the new token"""
    R, Hq, _ = q.shape
    Hk = K.shape[1]
    scale = 1.0 / math.sqrt(HD)
    qg = q.double().view(R, Hk, Hq // Hk, HD)                   # query heads grouped by their kv head (GQA)
    Kd, Vd = K.double(), V.double()
    s = torch.einsum("rgjd,rgtd->rgjt", qg, Kd) * scale
    s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
    if with_new:
        s = torch.cat([s, torch.einsum("rgjd,rgd->rgj", qg, kn.double())[..., None] * scale], -1)
        Vd = torch.cat([Vd, vn.double()[:, :, None]], 2)
    return torch.einsum("rgjt,rgtd->rgjd", torch.softmax(s, -1), Vd).reshape(R, Hq, HD)


def _head_err(o, ref):
    """relative error of every (row, query head) of a bf16 output [R, Hq * 128] against ref [R, Hq, 128]"""
    a = o.double().cpu().view(ref.shape)
    return (a - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def _within_one_ulp(got, want):
    """bf16 tensors: |got - want| <= one bf16 ulp of the larger magnitude"""
    a, b = got.float().cpu(), want.float().cpu()
    m = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(m > 0, torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-38))) - 7), torch.zeros(()))
    return bool(((a - b).abs() <= ulp).all())


def _guarded(body, dev):
    """body (any shape) followed by GUARD elements of a fixed random pattern, in one device buffer -> (buffer, view of the body)"""
    guard = torch.randn(GUARD, generator=torch.Generator().manual_seed(7)).to(body.dtype)
    buf = torch.cat([body.reshape(-1), guard]).to(dev)
    return buf, buf[:body.numel()].view(body.shape)


HEADS = {"1p5": (12, 2), "tiny": (2, 1)}
# (pos0, Tmax - pos0, rows, heads, key_valid, needle key).  Positions: the 64-key chunk edges, 512 (a wave's second pass begins past
# it) and 1 500 (third pass); Tmax = pos0 + 1 puts the new token in the last slot.  key_valid: none, 20 % random holes, left padding of
# 64 / 448 / 512 / pos0 - 1 keys (whole chunks blank, every first-pass chunk blank, one cache key left), every cache key masked.
CASES = [
    (0, 1, 1, "tiny", "none", None), (0, 37, 16, "1p5", "none", None),
    (1, 1, 5, "1p5", "none", 0), (1, 37, 1, "tiny", "all", None),
    (63, 1, 16, "1p5", "holes", 0), (63, 37, 5, "tiny", "none", 62),
    (64, 1, 1, "1p5", "none", 63), (64, 37, 16, "1p5", "holes", None),
    (65, 1, 5, "1p5", "pad64", 64), (65, 37, 16, "tiny", "padlast", None),
    (127, 1, 16, "1p5", "pad64", 63), (127, 37, 1, "1p5", "holes", 126),
    (128, 1, 5, "tiny", "holes", 64), (128, 37, 16, "1p5", "all", 0),
    (128, 1, 1, "1p5", "padlast", 127),
    (511, 1, 16, "1p5", "pad448", 0), (511, 37, 5, "1p5", "none", 510),
    (512, 1, 1, "1p5", "pad448", 511), (512, 37, 16, "1p5", "holes", 511), (512, 1, 16, "tiny", "none", None),
    (513, 1, 16, "1p5", "pad512", 512), (513, 37, 5, "1p5", "none", 512), (513, 1, 1, "tiny", "holes", 0),
    (575, 1, 16, "1p5", "pad512", 511), (575, 37, 5, "tiny", "holes", 574), (575, 1, 1, "1p5", "padlast", None),
    (576, 1, 16, "1p5", "none", 575), (576, 37, 5, "1p5", "pad64", 64), (576, 1, 16, "1p5", "all", None),
    (1024, 1, 16, "1p5", "holes", 512), (1024, 37, 5, "tiny", "pad448", 1023), (1024, 1, 1, "1p5", "pad512", 63),
    (1024, 37, 16, "1p5", "pad64", 511),
    (1500, 1, 16, "1p5", "none", 1499), (1500, 37, 16, "1p5", "holes", 64), (1500, 1, 5, "1p5", "padlast", None),
    (1500, 37, 1, "tiny", "pad512", 1000), (1500, 1, 16, "tiny", "all", None), (1500, 1, 16, "1p5", "pad448", 0),
]


def _key_valid(mode, R, Tmax, pos0, g):
    kv = torch.ones(R, Tmax, dtype=torch.uint8)
    if mode == "holes":
        kv[:, :pos0] = (torch.rand(R, pos0, generator=g) > 0.2).to(torch.uint8)
    elif mode.startswith("pad"):
        kv[:, :pos0 - 1 if mode == "padlast" else int(mode[3:])] = 0
    elif mode == "all":
        kv[:, :pos0] = 0
    return None if mode == "none" else kv


class _Case:
    """Inputs of one attention launch (seeded) and everything the references need."""

    def __init__(self, pos0, extra, R, heads, kv_mode, needle, dev):
        self.pos0, self.Tmax, self.R, self.dev = pos0, pos0 + extra, R, dev
        self.Hq, self.Hk = HEADS[heads]
        g = torch.Generator().manual_seed(pos0 * 1000 + extra * 37 + R)
        Hq, Hk, Tmax = self.Hq, self.Hk, self.Tmax
        nqkv = (Hq + 2 * Hk) * HD
        self.parts = 0.4 * torch.randn(6, R, nqkv, generator=g)
        self.ss_part = 100 + 50 * torch.rand(6, 32, generator=g)
        self.acc, self.ss = _seq(self.parts), _seq(self.ss_part)
        self.bias = (0.1 * torch.randn(nqkv, generator=g)).to(BF)
        self.K = torch.randn(R, Hk, Tmax, HD, generator=g).to(BF)
        self.V = torch.randn(R, Hk, Tmax, HD, generator=g).to(BF)
        kv = _key_valid(kv_mode, R, Tmax, pos0, g)
        self.kv = kv
        self.vis = torch.ones(R, pos0, dtype=torch.bool) if kv is None else kv[:, :pos0].bool()
        from unigen_hip import ops
        self.cos_d, self.sin_d = ops.rope_tables(Tmax, HD, 1e6, dev)       # (the engine's table: Tmax rows)
        self.cos, self.sin = self.cos_d.cpu(), self.sin_d.cpu()
        self.q, self.kn, self.vn = _finish_ref(self.acc, self.ss, self.bias, self.cos, self.sin, min(pos0, Tmax - 1), Hq, Hk)
        self.needle = needle
        if needle is not None:
            # a key whose score beats every other visible score of each query head of its group by >= 20: k = c * sum of the unit q's
            if kv_mode == "holes":
                self.kv[:, needle] = 1
                self.vis[:, needle] = True
            rep = Hq // Hk
            qg = self.q.double().view(R, Hk, rep, HD)
            u = (qg / qg.norm(dim=-1, keepdim=True)).sum(2)                                    # [R, Hk, D]
            s_u = torch.einsum("rgjd,rgd->rgj", qg, u) / math.sqrt(HD)
            assert bool((s_u > 0).all())
            s_all = torch.einsum("rgjd,rgtd->rgjt", qg, self.K[:, :, :pos0].double()) / math.sqrt(HD)
            s_all = s_all.masked_fill(~self.vis[:, None, None, :], float("-inf"))
            s_new = torch.einsum("rgjd,rgd->rgj", qg, self.kn.double()) / math.sqrt(HD)
            top = torch.maximum(s_all.amax(-1), s_new).amax(-1)                                # [R, Hk]
            c = (top + 30) / s_u.amin(-1)
            self.Kn = self.K.clone()
            self.Kn[:, :, needle] = (c[..., None] * u).to(BF)
            self.Vn = self.V.clone()
            self.Vn[:, :, needle] = (3 * torch.randn(R, Hk, HD, generator=g)).to(BF)
            s_needle = torch.einsum("rgjd,rgd->rgj", qg, self.Kn[:, :, needle].double()) / math.sqrt(HD)
            self.needle_margin = (s_needle - torch.maximum(s_all.amax(-1), s_new)).amin(-1)   # [R, Hk]
            self.needle_vis = self.vis[:, needle]                                                 # [R]

    def ref(self, K=None, V=None, vis=None, rpos=None, with_new=True):
        K, V, vis = (self.K if K is None else K), (self.V if V is None else V), (self.vis if vis is None else vis)
        q, kn, vn = self.q, self.kn, self.vn
        if rpos is not None:
            q, kn, vn = _finish_ref(self.acc, self.ss, self.bias, self.cos, self.sin, rpos, self.Hq, self.Hk)
        return _attend_ref(q, kn, vn, K[:, :, :self.pos0], V[:, :, :self.pos0], vis, with_new)

    def _cache(self, K, V, nan_from=None):
        """device K / V caches as views into guarded buffers; slots [nan_from, Tmax) NaN"""
        kb, kc = _guarded(K, self.dev)
        vb, vc = _guarded(V, self.dev)
        if nan_from is not None:
            kc[:, :, nan_from:] = float("nan")
            vc[:, :, nan_from:] = float("nan")
        return kb, vb, kc, vc

    def run_fused(self, K=None, V=None, nan=False, ordered=False):
        """-> (output [R, Hq * 128] bf16 on the host, K / V guarded buffers before and after the launch)"""
        from unigen_hip import ops
        K, V = (self.K if K is None else K), (self.V if V is None else V)
        kb, vb, kc, vc = self._cache(K, V, self.pos0 if nan else None)
        before = (kb.clone(), vb.clone())
        ob, o = _guarded(torch.full((self.R, self.Hq * HD), float("nan"), dtype=BF), self.dev)      # (every output element must be written)
        obefore = ob.clone()
        pos = torch.tensor([self.pos0], dtype=torch.int32, device=self.dev)
        kv = None if self.kv is None else self.kv.to(self.dev)
        bias = self.bias.to(self.dev)
        if ordered:
            ops.attn_decode_fused_ord(self.parts.to(self.dev), self.ss_part.to(self.dev), EPS, NORM_COLS, bias, self.cos_d, self.sin_d, pos,
                                      kc, vc, kv, o, self.Hq, self.Hk, HD, self.Tmax)
        else:
            ops.attn_decode_fused(self.acc.to(self.dev), self.ss.to(self.dev), EPS, NORM_COLS, bias, self.cos_d, self.sin_d, pos, kc, vc, kv, o,
                                  self.Hq, self.Hk, HD, self.Tmax)
        torch.cuda.synchronize()
        assert torch.equal(ob[o.numel():].view(torch.int16), obefore[o.numel():].view(torch.int16)), "output guard written"
        return o.cpu(), before, (kb.cpu(), vb.cpu())

    def run_unfused(self, K=None, V=None, nan=False):
        """ug_attn_decode on the cache with the new token's k / v already at pos0 (the reference's rows), len = pos0 + 1"""
        from unigen_hip import ops
        K, V = (self.K if K is None else K).clone(), (self.V if V is None else V).clone()
        K[:, :, self.pos0], V[:, :, self.pos0] = self.kn.to(BF), self.vn.to(BF)
        _, _, kc, vc = self._cache(K, V, self.pos0 + 1 if nan else None)
        kv = None if self.kv is None else self.kv.to(self.dev)
        ln = torch.tensor([self.pos0 + 1], dtype=torch.int32, device=self.dev)
        o = ops.attn_decode(self.q.reshape(self.R, -1).to(BF).to(self.dev), kc, vc, kv, self.Hq, self.Hk, HD, self.Tmax, ln)
        return o.cpu()


def _case_id(c):
    return f"p{c[0]}-T{c[0] + c[1]}-R{c[2]}-{c[3]}-{c[4]}" + ("" if c[5] is None else f"-needle{c[5]}")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_fused_decode_attention_matches_fp64(dev, case):
    pos0, extra, R, heads, kv_mode, needle = case
    c = _Case(*case, dev)
    Hq, Hk, Tmax = c.Hq, c.Hk, c.Tmax
    ref = c.ref()
    o, (kb0, vb0), (kb1, vb1) = c.run_fused()
    assert torch.isfinite(o.float()).all()
    err = _head_err(o, ref)
    assert float(err.max()) <= BAR, (f"worst (row, head) {divmod(int(err.argmax()), Hq)}", float(err.max()))
    # cache: the appended row within one bf16 ulp of the reference, every other byte (other rows / kv heads / slots, the guard) unchanged
    n = R * Hk * Tmax * HD
    for buf0, buf1, want in ((kb0, kb1, c.kn), (vb0, vb1, c.vn)):
        got = buf1[:n].view(R, Hk, Tmax, HD)[:, :, pos0]
        assert _within_one_ulp(got, want.to(BF)), "appended row"
        expect = buf0.cpu().clone()
        expect[:n].view(R, Hk, Tmax, HD)[:, :, pos0] = got
        assert torch.equal(buf1.view(torch.int16), expect.view(torch.int16)), "cache bytes other than the appended row changed"
    # nothing at or past pos0 reaches the output
    o_nan, _, _ = c.run_fused(nan=True)
    assert torch.isfinite(o_nan.float()).all() and torch.equal(o_nan.view(torch.int16), o.view(torch.int16)), "NaN slots reached the output"
    if pos0 == 0 or kv_mode == "all":                 # only the new token is visible: o = bf16(v_new) exactly
        want = c.vn.repeat_interleave(Hq // Hk, 1).reshape(R, Hq * HD).to(BF)
        assert torch.equal(o, want)
    # the unfused kernel on the same bounds
    ou = c.run_unfused()
    eu = _head_err(ou, ref)
    assert float(eu.max()) <= BAR, ("unfused", float(eu.max()))
    ou_nan = c.run_unfused(nan=True)
    assert torch.isfinite(ou_nan.float()).all() and torch.equal(ou_nan.view(torch.int16), ou.view(torch.int16)), "unfused: NaN slots"
    if pos0 == 0 or kv_mode == "all":
        assert torch.equal(ou, c.vn.repeat_interleave(Hq // Hk, 1).reshape(R, Hq * HD).to(BF))
    # the needle: dominates its group's heads where visible, changes no bit where masked
    if needle is not None:
        on, _, _ = c.run_fused(K=c.Kn, V=c.Vn)
        oun = c.run_unfused(K=c.Kn, V=c.Vn)
        refn = c.ref(K=c.Kn, V=c.Vn)
        vis = c.needle_vis
        for got, base, tag in ((on, o, "fused"), (oun, ou, "unfused")):
            if bool(vis.any()):
                assert float(c.needle_margin[vis].min()) >= 20
                e = _head_err(got[vis], refn[vis])
                assert float(e.max()) <= BAR, (tag, "needle", float(e.max()))
                vrow = c.Vn[:, :, needle].float().repeat_interleave(Hq // Hk, 1)[vis].double()
                e2 = _head_err(got[vis], vrow)
                assert float(e2.max()) <= BAR, (tag, "needle does not dominate", float(e2.max()))
            if bool((~vis).any()):
                assert torch.equal(got[~vis].view(torch.int16), base[~vis].view(torch.int16)), (tag, "masked needle changed the output")
    # the ordered form fed six slots whose ascending sum is the accumulator: the default kernel's bits, on every launch
    for _ in range(3):
        oo, _, (kbo, vbo) = c.run_fused(ordered=True)
        assert torch.equal(oo.view(torch.int16), o.view(torch.int16))
        assert torch.equal(kbo.view(torch.int16), kb1.view(torch.int16)) and torch.equal(vbo.view(torch.int16), vb1.view(torch.int16))


def test_attention_bar_rejects_subtly_wrong_references(dev):
    """The 1e-2 bar catches a subtly wrong kernel: the kernel's output misses each perturbed fp64 reference by >= 3 x the bar, on a case
    where the perturbation changes the result, while it holds the bar against the true reference."""
    wide = _Case(576, 1, 16, "1p5", "none", None, dev)            # every key of chunks 0..8 visible
    one = _Case(575, 1, 5, "1p5", "padlast", None, dev)            # cache key 574 and the new token only
    found = {}
    for c in (wide, one):
        o, _, _ = c.run_fused()
        assert float(_head_err(o, c.ref()).max()) <= BAR
        vis_drop = c.vis.clone()
        if c is wide:
            vis_drop[:, 448:512] = False
            found["keys [448, 512) dropped"] = _head_err(o, c.ref(vis=vis_drop))
            found["RoPE at pos0 - 1"] = _head_err(o, c.ref(rpos=c.pos0 - 1))
        else:
            vis_drop[:, c.pos0 - 1] = False
            found["key pos0 - 1 dropped"] = _head_err(o, c.ref(vis=vis_drop))
            vis_in = c.vis.clone()
            vis_in[:, 0] = True
            found["one masked key included"] = _head_err(o, c.ref(vis=vis_in))
            found["new token omitted"] = _head_err(o, c.ref(with_new=False))
    for name, e in found.items():
        print(f"    {name}: worst (row, head) error {float(e.max()):.3e} (bar {BAR:.0e})")
        assert float(e.max()) >= 3 * BAR, (name, float(e.max()))


# ====================================================================================== engine level
TV, VOCAB = 2048, 4096
NV = VOCAB - 1 - TV                  # head rows [2048, 4095) of the tied embedding: the code-book logits of t2i_generate_ar
STEPS = 8
ENGINE_CASES = {
    # rows, prompt, left pads per row (cycled), seed.  chunk128: the cache grows 125 -> 133 keys, across the 128 edge;
    # past512: 507 -> 515, so wave 0 runs its second chunk
    "chunk128": (16, 125, (0, 1, 63, 64, 65, 100, 124), 5),
    "past512": (3, 507, (0, 64, 480), 6),
}
# name: (deterministic, decode_fused, UNIGEN_DECODE_SW, decode_step_logits exists, captured replay)
FORMS = {
    "sw": (False, True, "1", True, True),
    "splitk": (False, True, "0", False, False),
    "separate": (False, False, "1", False, False),
    "ord_sw": (True, True, "1", True, True),
    "ord_wide": (True, False, "1", True, False),
}
# Final-norm hidden state and appended K / V rows against fp32, per row: 1e-2, or ROW_YARDSTICK x the distance of the same row of the
# oracle's own bf16-autocast path where that is larger.  Measured on the oracle alone (host, these inputs): its bf16 path is 1.0 .. 1.4 %
# from fp32 on every final-norm hidden row and up to 1.4 % on the last layer's K / V rows (0.3 % at layer 0) -- bf16 rounding of this
# 3-layer network, which no bf16 evaluation can beat -- so 1e-2 alone cannot be held there.  1.5 leaves room for the row-to-row spread
# between two bf16 evaluations; a wrong kernel (a stale accumulator, a dropped key block) is far outside it.
ROW_BAR, ROW_YARDSTICK = 1e-2, 1.5


@pytest.fixture(scope="module")
def m3(dev):
    """UniGen at the 1.5B width with THREE layers (odd depth), vocab 4 096, seeded weights, and the oracle bound to the same tensors"""
    from models import UniGen
    from oracle import qwen2_ref, weights
    cfg = dict(qwen2_ref.QWEN25_1P5B, num_hidden_layers=3, vocab_size=VOCAB)
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TV, llm_model_path=llm_config_dir(cfg), codebook_size=NV,
                   num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=-1).eval()
    names = [(n, tuple(p.shape)) for n, p in model.llm.named_parameters()]
    sd = weights.synth_llm_state(names, seed=23)
    model.llm.load_state_dict(sd, strict=False)
    with torch.device("meta"):
        lm = qwen2_ref.RefCausalLM(qwen2_ref.Qwen2Cfg(**cfg))
    lm.load_state_dict(sd, strict=False, assign=True)
    lm.lm_head.weight = lm.model.embed_tokens.weight
    return model, lm


def _engine_inputs(name):
    R, P, pads, seed = ENGINE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    prompt = 0.02 * torch.randn(R, P, 1536, generator=g)
    xs = [0.02 * torch.randn(R, 1536, generator=g) for _ in range(STEPS)]
    kv = torch.ones(R, P, dtype=torch.bool)
    for r in range(R):
        kv[r, :pads[r % len(pads)]] = False
    return prompt, xs, kv


def _oracle_steps(lm, prompt, xs, kv, autocast):
    """prefill (mask convention of ar_generate_ref) + one step per input through the concatenating cache -> per step: final-norm hidden
    [R, H], head logits [R, NV] (bf16 values under autocast), and every layer's appended k / v rows [R, Hk, 128]; all fp32"""
    from oracle import qwen2_ref
    R, P, _ = prompt.shape
    caches = [dict() for _ in lm.model.layers]
    w_head = lm.model.embed_tokens.weight[TV:VOCAB - 1]
    out = []
    with torch.no_grad(), qwen2_ref.autocast_ctx(autocast):
        r = torch.arange(P)
        allow = (r[None, :] <= r[:, None])[None, None] & kv[:, None, None, :]
        mask = torch.where(allow, 0.0, float("-inf"))
        mask = torch.where(allow.any(-1, keepdim=True), mask, torch.zeros(()))
        lm.backbone(inputs_embeds=prompt, mask=mask, caches=caches)
        for i, x in enumerate(xs):
            allow = torch.ones(R, P + i + 1, dtype=torch.bool)
            allow[:, :P] = kv
            mask = torch.where(allow[:, None, None, :], 0.0, float("-inf"))
            h = lm.backbone(inputs_embeds=x[:, None], mask=mask, caches=caches, pos_offset=P + i)[:, -1]
            out.append({"h": h.float(), "logits": F.linear(h, w_head).float(),
                        "k": [c["k"][:, :, -1].float() for c in caches], "v": [c["v"][:, :, -1].float() for c in caches]})
    return out


_ORACLE = {}


def _oracle(lm, name):
    """fp32 (exact) and bf16-autocast (control) runs, once per case"""
    if name not in _ORACLE:
        prompt, xs, kv = _engine_inputs(name)
        _ORACLE[name] = (_oracle_steps(lm, prompt, xs, kv, False), _oracle_steps(lm, prompt, xs, kv, True))
    return _ORACLE[name]


def _engine_run(eng, prompt, xs, kv, det, how, dev):
    """one decode form for len(xs) steps on a fresh state: how = step (decode_step), logits (decode_step_logits), graph
    (decode_step_logits: step 1 eager, steps 2.. replayed from one captured step) -> per step dict of what the engine produced"""
    from unigen_hip.qwen2 import DecodeState
    R, P, H = prompt.shape
    w_head = eng.fp.w("embed")[TV:VOCAB - 1]
    st = DecodeState(eng.dims, R, P + len(xs), dev, key_valid=kv, deterministic=det)
    eng.prefill(st, prompt.to(dev), kv.to(dev))
    x = torch.empty(R, H, device=dev)
    lg = torch.full((R, NV), float("nan"), device=dev)
    graph, out = None, []
    for i, xi in enumerate(xs):
        x.copy_(xi)
        rec = {}
        if how == "step":
            hn = eng.decode_step(st, x)
            rec["h"] = hn.float().cpu()
            rec["logits"] = (hn.float() @ w_head.float().t()).cpu()
        elif how == "logits" or i == 0:
            eng.decode_step_logits(st, x, w_head, lg)
            rec["logits"] = lg.cpu()
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    eng.decode_step_logits(st, x, w_head, lg)
            graph.replay()
            rec["logits"] = lg.cpu()
        rec["k"] = [st.k[l][:, :, P + i].float().cpu() for l in range(eng.dims.num_hidden_layers)]
        rec["v"] = [st.v[l][:, :, P + i].float().cpu() for l in range(eng.dims.num_hidden_layers)]
        rec["pos"], rec["len"] = int(st.pos.item()), int(st.len.item())
        out.append(rec)
    eng.check_errors()
    return out


def _row_errs(got, ref):
    a, b = got.reshape(got.shape[0], -1).double(), ref.reshape(ref.shape[0], -1).double()
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_decode_forms_match_oracle(dev, m3, case, form):
    """Every decode form the engine has at these row counts, 8 steps of decode_step (and of decode_step_logits where it exists, eager and
    with steps 2.. replayed from a captured graph for the single-writer forms), against the oracle stepped through its cache."""
    model, lm = m3
    eng = model.llm.engine
    det, fused, sw_env, has_logits, has_graph = FORMS[form]
    prompt, xs, kv = _engine_inputs(case)
    R, P, _ = prompt.shape
    r32, rbf = _oracle(lm, case)
    hows = ["step"] + (["logits"] if has_logits else []) + (["graph"] if has_graph else [])
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setenv("UNIGEN_DECODE_SW", sw_env)
        mp.setattr(eng, "decode_fused", fused, raising=False)
        from unigen_hip.qwen2 import DecodeState
        probe = DecodeState(eng.dims, R, 1, dev, deterministic=det)
        assert eng.decode_sw(probe) == (form in ("sw", "ord_sw")), form          # (the ordered forms: decode_ord_sw follows decode_sw here)
        failed = []

        def rows_ok(tag, got, i, key, l=None):
            pick = (lambda r: r[key]) if l is None else (lambda r: r[key][l])
            e, e_ref = _row_errs(got, pick(r32[i])), _row_errs(pick(rbf[i]), pick(r32[i]))
            bad = (e > torch.clamp(ROW_YARDSTICK * e_ref, min=ROW_BAR)).nonzero().flatten().tolist()
            if bad:
                failed.append(f"{tag}: rows {bad} errors {[round(float(e[r]), 4) for r in bad]} vs the oracle bf16 path's "
                              f"{[round(float(e_ref[r]), 4) for r in bad]}")

        for how in hows:
            run = _engine_run(eng, prompt, xs, kv, det, how, dev)
            for i, rec in enumerate(run):
                tag = f"{case} {form} {how} step {i + 1} (cache {P + i} keys + new)"
                if rec["pos"] != P + i + 1 or rec["len"] != P + i + 2:
                    failed.append(f"{tag}: pos / len {rec['pos']} / {rec['len']}")
                try:
                    fp32_yardstick(tag, rec["logits"], rbf[i]["logits"], r32[i]["logits"], YARDSTICK)
                except AssertionError as ex:
                    failed.append(f"{tag}: logits {ex}")
                if "h" in rec:
                    rows_ok(f"{tag} final-norm hidden", rec["h"], i, "h")
                for l in range(len(rec["k"])):
                    for kv_name in ("k", "v"):
                        rows_ok(f"{tag} layer {l} appended {kv_name}", rec[kv_name][l], i, kv_name, l)
    assert not failed, f"{len(failed)} comparisons failed:\n" + "\n".join(failed[:16])


# ====================================================================================== model level
MARGIN = 0.2                     # top-2 margin of the CFG-mixed logits below which later tokens may legitimately diverge (as test_full_depth_gen_gpu)


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_t2i_generate_ar_at_odd_depth_matches_oracle(dev, m3, deterministic):
    """t2i_generate_ar greedy (single-writer layer + head launch at odd depth): every eager step's logits against ar_generate_ref, tokens where
    the oracle's margin is clear; captured and kept-session runs agree with the eager one (bit for bit in deterministic mode)."""
    from oracle import qwen2_ref
    model, lm = m3
    eng = model.llm.engine
    # text vocabulary 2 047: a 2 048-row code-book head (the default form's head GEMV takes a multiple of 4 rows, as the product's 8 192)
    tv = TV - 1
    B, P, n, scale, PAD = 2, 70, 8, 3.0, tv - 1
    g = torch.Generator().manual_seed(47)
    cond = torch.randint(0, PAD, (B, P + n + 1), generator=g)
    uncond = torch.randint(0, PAD, (B, P + n + 1), generator=g)
    cond[0, :9] = PAD
    uncond[0, :66] = PAD
    uncond[1, :40] = PAD
    am = torch.cat([cond != PAD, uncond != PAD]).long()
    am[:, P:] = 1

    def run(**kw):
        return model.t2i_generate_ar(input_ids=cond.to(dev), uncond_input_ids=uncond.to(dev), attention_mask=am.to(dev), guidance_scale=scale,
                                     temperature=1.0, text_vocab_size=tv, image_token_num_per_image=n, greedy=True,
                                     deterministic=deterministic, **kw).cpu()
    with torch.no_grad():
        ce, ue = lm.model.embed_tokens(cond[:, :P]), lm.model.embed_tokens(uncond[:, :P])
        eng._ar_session = None
        trace = []
        eager = run(use_graph=False, trace=trace)
        eng.check_errors()
        assert len(trace) == n and not eng.last_decode_graph
        captured = run(use_graph=True)
        assert eng.last_decode_graph
        kept = run(use_graph=True)
        eng._ar_session = None
        tr_bf, tr_32 = [], []
        want, margin = qwen2_ref.ar_generate_ref(lm, ce, ue, n, scale, tv, key_valid=am[:, :P], autocast=True, trace=tr_bf)
        qwen2_ref.ar_generate_ref(lm, ce, ue, n, scale, tv, key_valid=am[:, :P], autocast=False, trace=tr_32, force_tokens=want)
    if deterministic:
        assert torch.equal(eager, captured) and torch.equal(eager, kept)
    else:
        # float atomics: a run may differ from another in the last bits, so an argmax may flip at a near-tie of the run's own logits
        for other in (captured, kept):
            for b in range(B):
                for i in range(n):
                    lg = trace[i].cpu()
                    mixed = lg[B + b] + scale * (lg[b] - lg[B + b])
                    top2 = mixed.topk(2).values
                    if float(top2[0] - top2[1]) < MARGIN:
                        break
                    assert int(other[b, i]) == int(eager[b, i]), (b, i, other[b], eager[b])
    steps = 0
    for i in range(n):
        same = torch.tensor([bool(torch.equal(eager[b, :i].long(), want[b, :i].long())) for b in range(B)])
        if not bool(same.any()):
            break
        rows = torch.cat([same, same])
        fp32_yardstick(f"t2i step {i} ({int(same.sum())} of {B} images on the oracle's trajectory)", trace[i].cpu()[rows],
                       tr_bf[i]["logits"][rows], tr_32[i]["logits"][rows])
        steps += 1
        for b in range(B):
            if same[b] and margin[b, i] >= MARGIN:
                assert int(eager[b, i]) == int(want[b, i]), (i, b, eager[b], want[b], margin[b])
    assert steps >= 4, steps
