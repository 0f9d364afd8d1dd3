"""Fused gradient-norm clipping on the GPU: the sum-of-squares kernel over span tables (exact on integer data, within one fp32
ulp of an fp64 oracle on random data, the same bits on every run), the finish's coefficient arithmetic, the in-place scale by the
device scalar, torch's semantics on non-finite norms and mixed parameter sets, the deferred form inside FusedAdamW (bit-identical
to clipping in place and stepping), and ug_adamw_flat_dev with a null factor (ug_adamw_flat's bits)."""
import math

import numpy as np
import pytest
import torch

from helpers import additive, golden, llm_config_dir

pytestmark = pytest.mark.gpu

# one element; shorter than a vector; exactly one; one + tail; no full workgroup; many workgroups + 1; beyond one trip of the
# 1024-workgroup grid (2^18 float4 per trip) with an odd tail
SPANS = [1, 3, 4, 5, 255, 1024 * 4 + 1, (1 << 20) + 7]
FIVE = [1, 5, 255, 1024 * 4 + 1, (1 << 20) + 7]


def _carve(lens, dev, first_offset=1):
    """One fp32 buffer with the spans of `lens` in it, separated by gaps, starting at element offsets 1, 2, 3, 0, 1, ... mod 4
    (first_offset=1: the first span starts at an address that is 4 mod 16).  -> (buffer, [views])"""
    offs, o = [], 0
    for k, n in enumerate(lens):
        o = (o + 3) // 4 * 4 + 8 + (first_offset + k) % 4
        offs.append(o)
        o += n
    buf = torch.zeros(o + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    views = [buf[a:a + n] for a, n in zip(offs, lens)]
    assert views[0].data_ptr() % 16 == 4 * first_offset
    return buf, views


def _params_over(views):
    ps = []
    for v in views:
        p = torch.nn.Parameter(torch.zeros_like(v))
        p.grad = v
        ps.append(p)
    return ps


def _block_of(grads, max_norm, grad_scale=1.0):
    """the finish's whole result block for a list of fp32 GPU gradients (no scaling)"""
    from unigen_hip import optim
    block = torch.empty(8, dtype=torch.float32, device=grads[0].device)
    optim._norm_into(block, list(grads), [], max_norm, grad_scale)
    return block


def _f32(x):
    return np.float32(x)


def _host_coef(max_norm, norm):
    """torch's coefficient arithmetic in fp32 on the host, from the returned norm"""
    raw = _f32(max_norm) / (_f32(norm) + _f32(1e-6))
    return min(_f32(1.0), raw)


# ------------------------------------------------------------------------------------------------ the sum kernel alone
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("blocks", [1, 3, 256, 1024])
def test_sum_of_squares_is_exact_on_integers(dev, blocks, accum):
    """Integers in [-3, 3]: every square and every partial sum is an integer below 2^24 (n <= 1.8 M), so fp64 accumulation and
    the fp32-chain form alike must return the exact sum, on every grid, for every span alone and for the tables."""
    from unigen_hip import ops
    gen = torch.Generator().manual_seed(12)
    buf, views = _carve(SPANS, dev)
    for v in views:
        v.copy_(torch.randint(-3, 4, (v.numel(),), generator=gen).float())
    exact = [int((v.cpu().long() ** 2).sum()) for v in views]
    partials = torch.zeros(blocks, dtype=torch.float64, device=dev)
    tables = [[i] for i in range(len(SPANS))] + [[SPANS.index(n) for n in FIVE], list(range(len(SPANS)))[::-1]]
    for pick in tables:
        table = torch.tensor([[views[i].data_ptr(), views[i].numel()] for i in pick], dtype=torch.int64, device=dev)
        partials.fill_(-1.0)                               # every slot must be written
        ops.sumsq_spans(table, partials, blocks, accum)
        got = partials.cpu()
        assert (got >= 0).all() and float(got.sum()) == float(sum(exact[i] for i in pick)), (pick, blocks, accum)


@pytest.mark.parametrize("pick", [[i] for i in range(len(SPANS))] + [[SPANS.index(n) for n in FIVE]], ids=lambda p: "x".join(str(SPANS[i]) for i in p))
def test_exact_norm(dev, pick):
    """total_norm == float(sqrt(exact integer sum)), through the public function; a threshold far above leaves the data alone."""
    from unigen_hip.optim import clip_grad_norm_
    gen = torch.Generator().manual_seed(13)
    buf, views = _carve([SPANS[i] for i in pick], dev)
    for v in views:
        v.copy_(torch.randint(-3, 4, (v.numel(),), generator=gen).float())
    before = buf.clone()
    exact = sum(int((v.cpu().long() ** 2).sum()) for v in views)
    out = clip_grad_norm_(_params_over(views), 1e30)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.device == buf.device
    assert _f32(out.item()) == _f32(math.sqrt(exact)), (out.item(), exact)
    assert torch.equal(buf, before)
    block = _block_of(views, 1e30)
    assert block[4:6].view(torch.float64).item() == float(exact) and block[1].item() == 1.0 and block[3].item() == 0.0


# ------------------------------------------------------------------------------------------------ random data against fp64
@pytest.fixture(scope="module")
def random_spans(dev):
    """randn gradients over the seven spans (one buffer, first span 4 mod 16) and the fp64 sums of squares per span, once"""
    gen = torch.Generator().manual_seed(14)
    buf, views = _carve(SPANS, dev)
    host = [torch.randn(n, generator=gen) for n in SPANS]
    for v, h in zip(views, host):
        v.copy_(h)
    sums = [float((h.double() ** 2).sum()) for h in host]
    return buf, views, host, sums


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_random_norm_against_fp64(dev, random_spans, scale):
    """fp64 accumulation ships: total_norm within 1 fp32 ulp of the fp64 oracle's rounded value, for every span alone and for
    the five- and seven-span tables.  torch's own clip_grad_norm_ on the same data is printed beside it as a control."""
    from unigen_hip.optim import clip_grad_norm_
    _, _, host, _ = random_spans
    scaled = [(h * scale).to(torch.float32) for h in host]
    buf, views = _carve(SPANS, dev)                        # (the same layout: the first span starts 4 mod 16)
    for v, h in zip(views, scaled):
        v.copy_(h)
    sums = [float((h.double() ** 2).sum()) for h in scaled]
    tables = [[i] for i in range(len(SPANS))] + [[SPANS.index(n) for n in FIVE], list(range(len(SPANS)))]
    worst = 0.0
    for pick in tables:
        want = _f32(math.sqrt(sum(sums[i] for i in pick)))
        ps = _params_over([views[i] for i in pick])
        ours = _f32(clip_grad_norm_(ps, 1e30).item())
        theirs = _f32(torch.nn.utils.clip_grad_norm_(ps, 1e30).item())
        ulp = float(np.spacing(want))
        print(f"    scale {scale:g} spans {[SPANS[i] for i in pick]}: ours {abs(float(ours) - float(want)) / ulp:.2f} ulp, "
              f"torch {abs(float(theirs) - float(want)) / ulp:.2f} ulp off the fp64 oracle")
        worst = max(worst, abs(float(ours) - float(want)) / ulp)
        assert abs(float(ours) - float(want)) <= ulp, (scale, pick, ours, want)
    print(f"    scale {scale:g}: worst {worst:.2f} ulp")


def test_two_calls_return_the_same_bits(dev, random_spans):
    _, views, _, _ = random_spans
    a = _block_of(views, 0.37, grad_scale=0.5).clone()
    junk = torch.randn(1 << 20, device=dev).square_().sum()             # (unrelated work in between)
    b = _block_of(views, 0.37, grad_scale=0.5).clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the block is what its contract says: norm of grad_scale * g, factor = grad_scale * coefficient
    plain = _block_of(views, 0.37)
    assert torch.equal(a[4:6].view(torch.int32), plain[4:6].view(torch.int32))
    s = plain[4:6].view(torch.float64).item()
    assert _f32(a[0].item()) == _f32(math.sqrt(s) * 0.5) and _f32(plain[0].item()) == _f32(math.sqrt(s))
    assert _f32(a[1].item()) == _host_coef(0.37, a[0].item()) and _f32(a[2].item()) == _f32(0.5) * _f32(a[1].item())


# ------------------------------------------------------------------------------------------------ in-place semantics
def test_in_place_scale_is_torch_mul_by_the_device_coefficient(dev, random_spans):
    from unigen_hip.optim import clip_grad_norm_
    buf0, views0, _, sums = random_spans
    norm = math.sqrt(sum(sums))
    for max_norm in (0.25 * norm, 4.0 * norm):
        buf = buf0.clone()
        views = [buf[v.storage_offset():v.storage_offset() + v.numel()] for v in views0]
        block = _block_of(views, max_norm)
        coef = block[1].clone()
        out = clip_grad_norm_(_params_over(views), max_norm)
        assert out.item() == block[0].item()
        assert _f32(coef.item()) == _host_coef(max_norm, out.item())
        if max_norm < norm:
            assert coef.item() < 1.0
            want = torch.mul(buf0, coef)                   # fp32 multiplication is correctly rounded: torch's product is the yardstick
            for v0, v in zip(views0, views):
                o = v0.storage_offset()
                assert torch.equal(v, want[o:o + v.numel()])
            gaps = torch.ones_like(buf, dtype=torch.bool)
            for v0 in views0:
                gaps[v0.storage_offset():v0.storage_offset() + v0.numel()] = False
            assert torch.equal(buf[gaps], buf0[gaps])      # nothing outside the spans is touched
        else:
            assert coef.item() == 1.0
            assert torch.equal(buf.view(torch.int32), buf0.view(torch.int32))


def test_one_span_beyond_32_bit_byte_offsets(dev):
    """The backbone's gradient is ONE span of 1.56 G elements: byte offsets pass 2^32.  2^30 + 2^20 + 5 integers in [-3, 3]
    starting 4 mod 16: the norm is exact (the sum stays far below 2^53), and the in-place scale reaches the elements on both
    sides of the 2^32-byte line and the last one."""
    from unigen_hip.optim import clip_grad_norm_
    n = (1 << 30) + (1 << 20) + 5
    gen = torch.Generator(device=dev).manual_seed(17)
    ints = torch.randint(-3, 4, (n,), device=dev, dtype=torch.int8, generator=gen)
    exact = int(torch.sum(ints * ints, dtype=torch.int64))
    buf = torch.empty(n + 8, dtype=torch.float32, device=dev)
    view = buf[1:1 + n]
    view.copy_(ints)
    p = _params_over([view])
    assert _f32(clip_grad_norm_(p, 1e30).item()) == _f32(math.sqrt(exact))
    max_norm = 0.3 * math.sqrt(exact)
    coef = _block_of([view], max_norm)[1].clone()
    out = clip_grad_norm_(p, max_norm)
    assert _f32(out.item()) == _f32(math.sqrt(exact)) and _f32(coef.item()) == _host_coef(max_norm, out.item()) and coef.item() < 1
    for lo, hi in ((0, 1000), ((1 << 30) - 1000, (1 << 30) + 1000), (n - 1000, n)):
        assert torch.equal(view[lo:hi], torch.mul(ints[lo:hi].float(), coef)), (lo, hi)
    assert float(view.double().square_().sum()) == pytest.approx(float(exact) * float(coef.item()) ** 2, rel=1e-6)    # (nothing skipped or scaled twice)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_norms_behave_as_in_torch(dev, random_spans, bad):
    from unigen_hip.optim import clip_grad_norm_
    buf0, views0, _, _ = random_spans

    def fresh():
        buf = buf0.clone()
        views = [buf[v.storage_offset():v.storage_offset() + v.numel()] for v in views0]
        views[5][17] = bad
        return buf, _params_over(views)
    (ba, pa), (bb, pb) = fresh(), fresh()
    a = clip_grad_norm_(pa, 1.0)
    b = torch.nn.utils.clip_grad_norm_(pb, 1.0)
    assert torch.allclose(a, b, rtol=0, atol=0, equal_nan=True), (a, b)
    for p, q in zip(pa, pb):
        assert torch.allclose(p.grad, q.grad, rtol=0, atol=0, equal_nan=True)
    bc, pc = fresh()
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(pc, 1.0, error_if_nonfinite=True)
    assert torch.allclose(bc, fresh()[0], rtol=0, atol=0, equal_nan=True)      # raised before anything was scaled


def _assert_matches_torch(ours, theirs, a, b):
    """`a`, `b`: the norms returned for the parameter lists `ours`, `theirs` (same data).  Norm: 1 fp32 ulp, the random-norm
    tolerance.  Gradients: the coefficients then differ by at most 1 ulp (norm) + 1.5 ulp (torch forms reciprocal * max_norm, two
    roundings, against one division here), and each side rounds its product once: 7 * 2^-24 < 2^-21 relative."""
    print(f"    norm: ours {a.item():.9g} torch {b.item():.9g} ({abs(a.item() - b.item()) / float(np.spacing(_f32(b.item()))):.2f} ulp apart)")
    assert abs(a.item() - b.item()) <= float(np.spacing(_f32(b.item())))
    for p, q in zip(ours, theirs):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            tol = 2.0 ** -21 if p.grad.dtype == torch.float32 else 2.0 ** -8        # (bf16: one ulp of the rounded product)
            assert torch.allclose(p.grad.float(), q.grad.float(), rtol=tol, atol=0), (p.shape, p.dtype)


def test_mixed_parameter_set(dev, random_spans):
    """fp32 spans in one buffer, a bf16 parameter, a non-contiguous fp32 parameter and a parameter without a gradient."""
    from unigen_hip.optim import clip_grad_norm_
    buf0, views0, _, _ = random_spans
    gen = torch.Generator().manual_seed(15)
    extra_bf16 = torch.randn(33, 7, generator=gen).to(dev, torch.bfloat16)
    extra_nc = torch.randn(6, 5, generator=gen).to(dev)

    def build():
        buf = buf0.clone()
        ps = _params_over([buf[v.storage_offset():v.storage_offset() + v.numel()] for v in views0])
        pb = torch.nn.Parameter(torch.zeros_like(extra_bf16)); pb.grad = extra_bf16.clone()
        pn = torch.nn.Parameter(torch.zeros(6, 5, device=dev).t()); pn.grad = extra_nc.clone().t()
        assert not pn.grad.is_contiguous()
        return ps[:3] + [pb, torch.nn.Parameter(torch.zeros(3, device=dev)), pn] + ps[3:]
    oracle = math.sqrt(sum(float((g.double() ** 2).sum()) for g in [buf0[v.storage_offset():v.storage_offset() + v.numel()] for v in views0]
                           + [extra_bf16, extra_nc]))
    for max_norm in (0.5 * oracle, 2.0 * oracle):
        ours, theirs = build(), build()
        a = clip_grad_norm_(ours, max_norm)
        b = torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        # (printed only: torch returns the bf16 tensor's norm in bf16, here as there, which alone is worth a few fp32 ulps of the total)
        print(f"    fp64 oracle {oracle:.9g}")
        _assert_matches_torch(ours, theirs, a, b)
        assert ours[4].grad is None


# ------------------------------------------------------------------------------------------------ ug_adamw_flat_dev
@pytest.mark.parametrize("mb", [0, 256])
@pytest.mark.parametrize("n", [1, 7, 4096 + 3])
def test_adamw_flat_dev_with_a_null_factor_is_adamw_flat(dev, n, mb):
    from unigen_hip import ops
    gen = torch.Generator().manual_seed(n)
    p0, g = torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
    half = torch.tensor([0.5], device=dev)
    state = []
    for form in ("flat", "dev_null", "dev_half"):
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        pb = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        for step in (1, 2, 3):
            if form == "flat":
                ops.adamw_flat_(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, grad_scale=0.5, max_blocks=mb)
            elif form == "dev_null":
                ops.adamw_flat_dev_(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, grad_scale=0.5, grad_factor=None, max_blocks=mb)
            else:                                          # 1.0 * 0.5 from the device is the same factor
                ops.adamw_flat_dev_(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, grad_scale=1.0, grad_factor=half, max_blocks=mb)
        state.append((p, m, v, pb))
    for other in state[1:]:
        for a, b in zip(state[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the tiny model
def _tiny_unigen(g, dev, w_und=False):
    from models import UniGen
    from oracle import weights
    cfg, ids = g["cfg"], g["ids"]
    extra = dict(mm_input_dim=32, und_proj_depth=2) if w_und else {}
    m = UniGen(w_und_encoder=w_und, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1, **extra)
    names = [(n, tuple(p.shape)) for n, p in (m.named_parameters() if w_und else m.llm.named_parameters()) if n != "_ddp_anchor"]
    sd = weights.synth_llm_state(names, seed=g["weight_seed"])
    res = (m if w_und else m.llm).load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    return m.train()


def _backward(model, g, dev):
    mask = additive(g["mask_allow"]).to(dev)
    _, l1, l2, l3 = model(input_ids=g["input_ids"].to(dev), attention_mask=mask, labels=g["labels"].to(dev), **g["kw"])
    (l1 + 0.1 * l2 + l3).backward()
    return l1


class _TinyStep:
    """One backward of the tiny model; weights, bf16 mirror and gradients can be put back from the snapshot, so every path starts
    from the same bits (no second backward: its fp32 atomics would make two runs differ before any optimizer is involved)."""

    def __init__(self, dev):
        from unigen_hip.optim import clip_grad_norm_
        g = golden("g2_tiny_unigen.pt")
        self.model = _tiny_unigen(g, dev)
        _backward(self.model, g, dev)
        self.fp = self.model.llm.engine.fp
        self.params = [p for p in self.model.parameters() if p.grad is not None]
        self.snap = (self.fp.master.clone(), self.fp.grad.clone(), [p.detach().clone() for p in self.params], [p.grad.clone() for p in self.params])
        self.norm0 = clip_grad_norm_(self.params, 1e30).item()
        assert math.isfinite(self.norm0) and self.norm0 > 0

    def restore_grads(self, scale=1.0):
        self.fp.wait_pending_update()                       # as the engine does before it writes gradients
        self.fp.grad.copy_(self.snap[1] * scale)
        for p, g0 in zip(self.params, self.snap[3]):
            p.grad.copy_(g0 * scale)

    def run(self, path, max_norm, steps=2, overlap=False, grad_scales=None):
        """path a: clip in place, plain step; b: FusedAdamW(max_grad_norm=...); c: clip_grad_norm_(defer_to=opt), step; none: no
        clipping.  grad_scales: step k sees the snapshot gradients times grad_scales[k].  -> weights, mirror, moments, norms"""
        from unigen_hip.optim import FusedAdamW, clip_grad_norm_
        fp, params = self.fp, self.params
        with torch.no_grad():
            fp.master.copy_(self.snap[0])
            for p, w0 in zip(params, self.snap[2]):
                p.copy_(w0)
        fp.refresh_compute_copies(force=True)               # the mirror is in sync, so the update kernels write it too
        opt = FusedAdamW(params, lr=1e-3, overlap=overlap, max_grad_norm=max_norm if path == "b" else None)
        norms = []
        busy = torch.randn(512, 512, device=fp.master.device)
        for k in range(steps):
            scale = 1.0 if grad_scales is None else grad_scales[k]
            self.restore_grads(scale)
            if path == "a":
                clip_grad_norm_(params, max_norm)
            elif path == "c":
                clip_grad_norm_(params, max_norm, defer_to=opt)
            opt.step()
            if path in ("b", "c"):
                norms.append(opt.last_grad_norm.clone())
            busy = busy @ busy.t() * 1e-3                   # unrelated work on the main stream beside an overlapped update
            if path in ("b", "c") and not overlap:
                assert torch.equal(fp.grad, self.snap[1] * scale)      # the deferred forms leave the gradients alone
        opt.synchronize()
        assert opt._pending is None
        state = [fp.master.clone(), fp.bf16.clone()] + [t.clone() for r in opt._runs for t in (r.m, r.v)] + [p.detach().clone() for p in params]
        return state, [n.item() for n in norms]


@pytest.fixture(scope="module")
def tiny_step(dev):
    return _TinyStep(dev)


def test_deferred_clipping_equals_in_place_clipping(dev, tiny_step):
    """Two optimizer steps per path from the same snapshot (the second with non-zero moments).  (a) clip in place, plain step;
    (b) FusedAdamW(max_grad_norm=...) on the unscaled gradients; (c) the function form with defer_to: g * coef * 1.0 ==
    g * (1.0 * coef), so all three leave the same bits in weights, bf16 mirror and moments.  Half the measured norm: the clip is
    active.  Twice the norm: nothing clips and the bits are also those of a step without clipping."""
    t = tiny_step
    for factor in (0.5, 2.0):
        res = {path: t.run(path, factor * t.norm0) for path in ("a", "b", "c") + (("none",) if factor > 1 else ())}
        for path in ("b", "c"):
            assert res[path][1] == [t.norm0, t.norm0]
        for path in res:
            assert len(res[path][0]) == len(res["a"][0])
            for x, y in zip(res["a"][0], res[path][0]):
                assert torch.equal(x, y), (factor, path)
        if factor < 1:
            unclipped = t.run("none", 0.0)[0]
            assert not torch.equal(unclipped[0], res["a"][0][0])       # the clip was active


def test_deferred_clipping_with_overlap(dev, tiny_step):
    """(b) with overlap=True for three steps against the in-stream run: the side stream reads the factor the main stream wrote.
    Step k sees the snapshot gradients times (1, 3, 0.2)[k], so every step has its own norm and factor (clipped, clipped, not):
    a factor read from the wrong step would show.  Tolerances of test_fused_adamw_overlapped_update_is_equivalent.  Both runs
    start from one backward's gradients -- with a backward per step, two IN-STREAM runs of this configuration already differ
    by 2.2e-5 in the third loss (fp32 atomics in the backward, amplified by Adam's sign-like first steps and bf16 rounding of
    the mirror), which says nothing about the overlap."""
    t = tiny_step
    scales = (1.0, 3.0, 0.2)
    (sa, na), (sb, nb) = (t.run("b", 0.5 * t.norm0, steps=3, overlap=ov, grad_scales=scales) for ov in (False, True))
    assert na == nb and len(na) == 3
    for n, s in zip(na, scales):                           # the norm of s * g is s * norm0 up to the rounding of the scaled gradients
        assert abs(n - s * t.norm0) <= 4 * 2.0 ** -24 * s * t.norm0
    worst = max((x.float() - y.float()).abs().max().item() for x, y in zip(sa, sb))
    print(f"    overlapped against in-stream: largest difference {worst:.3e} over {len(sa)} tensors")
    moments = sa[2:2 + (len(sa) - 2 - len(t.params))]
    for i, (x, y) in enumerate(zip(sa, sb)):
        if 2 <= i < 2 + len(moments):
            assert torch.allclose(x, y, rtol=1e-4, atol=1e-7), i
        else:
            assert torch.allclose(x.float(), y.float(), rtol=1e-5, atol=1e-6), i


def test_whole_model_norm_with_ordinary_parameters(dev):
    """The tiny model with its mm_projector on the graph (ordinary parameters beside the flat buffers, as in
    tests/ddp_gpu_worker.py's bare case): clip_grad_norm_(model.parameters(), 1.0) against torch on cloned gradients."""
    from unigen_hip.optim import clip_grad_norm_
    g = golden("g2_tiny_unigen.pt")
    model = _tiny_unigen(g, dev, w_und=True)
    ids = g["input_ids"].to(dev)
    gen = torch.Generator().manual_seed(16)
    feats = torch.randn(ids.shape[0], 6, 32, generator=gen).to(dev)
    emb = model.llm.model.embed_tokens(ids)
    emb = torch.cat([emb[:, :10], model.mm_projector(feats).to(emb.dtype), emb[:, 16:]], 1)
    _, l1, l2, l3 = model(input_ids=ids, input_embeddings=emb, attention_mask=additive(g["mask_allow"]).to(dev), labels=g["labels"].to(dev), **g["kw"])
    (l1 + 0.1 * l2 + l3).backward()
    ours = list(model.parameters())
    assert any(p.grad is not None and n.startswith("mm_projector") for n, p in model.named_parameters())
    theirs = []
    for p in ours:
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = None if p.grad is None else p.grad.clone()
        theirs.append(q)
    oracle = math.sqrt(sum(float((q.grad.double() ** 2).sum()) for q in theirs if q.grad is not None))
    a = clip_grad_norm_(ours, 1.0)
    b = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    print(f"    fp64 oracle {oracle:.9g}")
    assert abs(a.item() - float(_f32(oracle))) <= float(np.spacing(_f32(oracle)))
    _assert_matches_torch(ours, theirs, a, b)
