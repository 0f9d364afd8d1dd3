"""Bit-exact tests of the fp32 (csrc/conv_f32.hip) and split-f16 (csrc/conv_split.hip) convolution / GEMM kernels and of the SigLIP
attention kernel (csrc/siglip_attn.hip) on the operands of tests/split_exact.py: in an exact regime every partial sum is an fp32
number, so the kernel has to give the float64 contraction bit for bit at every element.  Every comparison is `torch.equal` (the one
derived bound: the uniform attention regime at T != 64).  The C entry points are called with the test's own output buffer: NaN or a
sentinel everywhere, a guard region behind M * ldy and, for the linear / GEMM entries, guard columns between N and ldy, all of
which must come back untouched.  The split kernels run twice, with the measured scale bound and with a bound one binade up.

Which instantiation each case runs is written next to it in split_exact.py (CONV_CASES, GEMM_CASES, LINEAR_CASES) and checked
against the restated launcher conditions in tests/test_split_exact_cpu.py."""
import pytest
import torch

import exact_products as ep
import split_exact as sx

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from unigen_hip import ops
    return ops


def _api():
    from unigen_hip import lib
    return lib.api()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _bounds(ops, x2d, maxabs):
    """the measured bound of the live columns and a bound from the next binade up"""
    return [("measured bound", ops.amax(x2d)), ("bound one binade up", ops.amax_const(2.0 * maxabs, x2d.device))]


def _assert_rows(got, want, what):
    """[rows, cols] results, bit for bit, with the place of the first differences"""
    if not torch.equal(got, want):
        raise AssertionError(f"{what}: {ep.mismatch_report(got.double(), want.double(), tile=(128, 128))}")


def _assert_buffer(buf, expect, what):
    """a whole output buffer (result, guard columns, gaps, guard region) against its expectation"""
    got = buf.cpu()
    if not torch.equal(got, expect):
        bad = ((got != expect) | (got.isnan() != expect.isnan())).nonzero().flatten()
        touched = int((expect[bad] == sx.SENTINEL).sum())
        first = [(int(i), float(got[i]), float(expect[i])) for i in bad[:8]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} buffer elements differ, {touched} of them guard elements; "
                             f"first (offset, got, want): {first}")


# ------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("name,regime", sx.CONV_PARAMS)
def test_conv_exact(dev, name, regime):
    """ug_conv2d_f32 / ug_conv2d_split / ug_conv3x3_split with integer bias and residual: equal to the float64 convolution at every
    element under both scale bounds, the guard behind the output intact; with `stats` the epilogue's fp64 sums per (image, group)
    are the exact integers and the trailing slot is max|y|; with `gn` the hand-built exact GroupNorm runs on the load path"""
    ops, api = _ops(), _api()
    p = sx.conv_problem(name, regime)
    c = p.case
    B, Ho, Wo, Cout = p.ref.shape
    M, n = B * Ho * Wo, p.ref.numel()
    cout_pad = ops.round_up(Cout, 128) if Cout > 32 else 32
    xd, bias, res = p.x.to(dev).contiguous(), p.bias.to(dev), p.res.to(dev).contiguous()
    wp = sx.pack_weight(p.w_pack, cout_pad).to(dev)
    ref2d = p.ref.view(M, Cout)
    pad = c.k // 2 if c.pad is None else c.pad
    pt = 0 if c.asym else pad

    def check(y, what):
        _assert_rows(y[:n].view(M, Cout).cpu(), ref2d, f"{name} {regime} [{c.kernel}] {what}")
        assert bool(y[n:].isnan().all()), f"{name} {regime} {what}: the launch wrote behind M * Cout"

    if c.entry == "f32":
        y = torch.full((n + sx.GUARD,), NAN, device=dev)
        api.ug_conv2d_f32(_ptr(xd), _ptr(wp), _ptr(bias), _ptr(res), _ptr(y), B, c.H, c.W, c.Cin, Cout, cout_pad, c.k, c.stride, pt, pt,
                          Ho, Wo, int(c.ups), _st())
        check(y, "")
        return
    ws = ops.split_conv_weight(wp)
    gn = [t.to(dev).contiguous() for t in p.gn] if c.gn else [None, None, None]
    seen = p.xn if c.gn else p.x                                   # what the contraction reads: its bound is what the kernel needs
    for what, bound in _bounds(ops, seen.to(dev).view(-1, c.Cin), seen.abs().max().item()):
        assert p.cond.loose_ok
        y = torch.full((n + sx.GUARD,), NAN, device=dev)
        st = torch.zeros(B * c.stats * 2 + 1, dtype=torch.float64, device=dev) if c.stats else None
        if c.entry == "split":
            api.ug_conv2d_split(_ptr(xd), _ptr(bound), _ptr(ws), _ptr(bias), _ptr(res), _ptr(y), B, c.H, c.W, c.Cin, Cout, cout_pad, c.k,
                                c.stride, pt, pt, Ho, Wo, int(c.ups), _ptr(st), c.stats, _st())
        else:
            api.ug_conv3x3_split(_ptr(xd), _ptr(bound), _ptr(ws), _ptr(bias), _ptr(res), _ptr(y), B, c.H, c.W, c.Cin, Cout, cout_pad,
                                 _ptr(gn[0]), _ptr(gn[1]), _ptr(gn[2]), 32 if c.gn else 0, 0, _ptr(st), c.stats, _st())
        check(y, what)
        if c.stats:
            got = st[:-1].view(B, c.stats, 2).cpu()
            assert torch.equal(got, p.stats), f"{name} {what}: epilogue sums differ at (image, group, sum|sumsq) {(got != p.stats).nonzero()[:8].tolist()}"
            assert torch.equal(ops.stats_amax(st).cpu(), p.amax.view(1)), f"{name} {what}: max|y| slot"


# ------------------------------------------------------------------------------------------------ fp32 GEMM, one- and two-level batches
@pytest.mark.parametrize("name", [g.name for g in sx.GEMM_CASES])
def test_gemm_f32_exact(dev, name):
    """ug_gemm_f32 / ug_gemm_f32_nested on integer operands with a power-of-two alpha: the whole output buffer -- results, the
    columns between N and ldc, the gaps between batches, the guard behind the last row -- equals its expectation"""
    api = _api()
    p = sx.gemm_problem(name)
    g = p.case
    a, b = p.a_buf.to(dev), p.b_buf.to(dev)
    cbuf = torch.full((p.c_expect.numel(),), sx.SENTINEL, device=dev)
    if g.outer:
        api.ug_gemm_f32_nested(_ptr(a), g.lda, g.sa[0], g.sa[1], _ptr(b), g.ldb, g.sb[0], g.sb[1], g.b_nk, _ptr(cbuf), g.ldc, g.sc[0],
                               g.sc[1], g.M, g.N, g.K, g.inner, g.outer, g.alpha, _st())
    else:
        api.ug_gemm_f32(_ptr(a), g.lda, g.sa[0], _ptr(b), g.ldb, g.sb[0], g.b_nk, _ptr(cbuf), g.ldc, g.sc[0], g.M, g.N, g.K, g.inner,
                        g.alpha, _st())
    _assert_buffer(cbuf, p.c_expect, f"{name} [{g.kernel}]")


# ------------------------------------------------------------------------------------------------ linear layers
@pytest.mark.parametrize("name,regime", sx.LINEAR_PARAMS)
def test_linear_exact(dev, name, regime):
    """ug_linear_f32 / ug_linear_split with bias, a strided residual, ldx > K and ldy > N"""
    ops, api = _ops(), _api()
    p = sx.linear_problem(name, regime)
    c = p.case
    xd, bias, res = p.x_buf.to(dev), p.bias.to(dev), p.res_buf.to(dev)
    if c.entry == "f32":
        W = torch.full((c.N, c.ldw), 3.0)
        W[:, :c.K] = p.W
        W = W.to(dev)
        y = torch.full((p.y_expect.numel(),), sx.SENTINEL, device=dev)
        api.ug_linear_f32(_ptr(xd), c.ldx, _ptr(W), c.ldw, _ptr(bias), _ptr(res), c.ldres, _ptr(y), c.ldy, c.M, c.N, c.K, 0, _st())
        _assert_buffer(y, p.y_expect, f"{name} [{c.kernel}]")
        return
    ws, n_pad = ops.split_linear_weight(p.W.to(dev))
    for what, bound in _bounds(ops, xd[:, :c.K], p.x.abs().max().item()):
        assert p.cond.loose_ok
        y = torch.full((p.y_expect.numel(),), sx.SENTINEL, device=dev)
        api.ug_linear_split(_ptr(xd), c.ldx, _ptr(bound), _ptr(ws), _ptr(bias), _ptr(res), c.ldres, _ptr(y), c.ldy, c.M, c.N, c.K, n_pad, 0,
                            _st())
        _assert_buffer(y, p.y_expect, f"{name} {regime} [{c.kernel}] {what}")


# ------------------------------------------------------------------------------------------------ split weight image
def test_split_weight_image_exact(dev):
    """ug_conv_split_weights at a ragged Cin (36) and cout_pad (256) > Cout (68), two-plane weights: both planes equal the split
    restated on the CPU at every element -- so plane 0 + plane 1 gives the scaled weight back exactly and the padding rows and
    channels are exact zeros in both planes -- and the trailing record is max|w|"""
    ops = _ops()
    wi = sx.WEIGHT_IMAGE
    w = sx.two_plane((wi["Cout"], wi["Cin"], 3, 3), 5)
    wp = sx.pack_weight(w, wi["cout_pad"])
    buf = ops.split_conv_weight(wp.to(dev))
    n = 2 * wi["taps"] * 64 * wi["cout_pad"]
    assert buf.numel() == n + 8 and float(buf[n:n + 2].view(torch.float32)) == w.abs().max().item() == 4095.0
    got = sx.weight_image_logical(buf, wi["taps"], wi["Cin"], wi["cout_pad"]).cpu()
    expect, ew = sx.weight_image_expect(wp)
    assert ew == 3
    assert torch.equal(got, expect), (got != expect).nonzero()[:8].tolist()
    assert not got[:, 1, :, :, :, 4:].any() and not got[:, :, 1].any() and not got[:, :, 0, :, wi["Cout"]:].any()
    back = (got.double().sum(dim=3) * 2.0 ** -ew).permute(0, 1, 4, 2, 3).reshape(wi["taps"], 64, wi["cout_pad"])[:, :wi["Cin"]]
    assert torch.equal(back, wp.double())


# ------------------------------------------------------------------------------------------------ SigLIP attention
def _attn(dev, qkv, B, T, H, hd, scale, bound):
    D = H * hd
    out = torch.full((B * T * (D + 8) + sx.GUARD,), sx.SENTINEL, device=dev)
    _api().ug_siglip_attn_f32(_ptr(qkv), qkv.stride(0), _ptr(bound), _ptr(out), D + 8, B, T, H, hd, float(scale), _st())
    out = out.cpu()
    rows = out[:B * T * (D + 8)].view(B * T, D + 8)
    assert bool((rows[:, D:] == sx.SENTINEL).all()) and bool((out[B * T * (D + 8):] == sx.SENTINEL).all()), "the launch wrote outside its columns"
    return rows[:, :D]


@pytest.mark.parametrize("v_regime", ["int", "x2"])
@pytest.mark.parametrize("B,T,H,hd", sx.ATTN_SHAPES)
def test_siglip_attention_selects_exactly(dev, B, T, H, hd, v_regime):
    """select regime: every query puts all of its weight on one key (every other probability is an exact zero operand, l_i = 1), so
    out[b, t, h, :] == v[b, sel(t), h, :] bit for bit, for integer and for two-plane v, under both scale bounds"""
    ops = _ops()
    p = sx.attn_select_problem(B, T, H, hd, v_regime)
    D = H * hd
    qkv = p.qkv.to(dev)
    want = p.expect.reshape(B * T, D)
    for what, bound in _bounds(ops, qkv[:, :3 * D], p.qkv[:, :3 * D].abs().max().item()):
        _assert_rows(_attn(dev, qkv, B, T, H, hd, p.scale, bound), want, f"select {(B, T, H, hd)} v {v_regime} {what}")


@pytest.mark.parametrize("B,T,H,hd", sx.ATTN_SHAPES)
def test_siglip_attention_uniform(dev, B, T, H, hd):
    """uniform regime (q = 0): out = sum_t v / T, exact at T = 64; elsewhere within 2^-22 |sum v / T| of the float64 quotient (one
    rounding in o_unscale / l_i, one in the product)"""
    ops = _ops()
    p = sx.attn_uniform_problem(B, T, H, hd)
    D = H * hd
    qkv = p.qkv.to(dev)
    want = p.quotient.expand(B, T, H, hd).reshape(B * T, D)
    for what, bound in _bounds(ops, qkv[:, :3 * D], p.qkv[:, :3 * D].abs().max().item()):
        got = _attn(dev, qkv, B, T, H, hd, hd ** -0.5, bound)
        if p.exact:
            _assert_rows(got, want.float(), f"uniform {(B, T, H, hd)} {what}")
        else:
            err = (got.double() - want).abs()
            worst = (err / want.abs().clamp_min(1e-300)).max().item()
            print(f"    uniform {(B, T, H, hd)} {what}: worst relative error {worst:.3e} (bound {sx.ATTN_UNIFORM_REL:.3e})")
            assert bool((err <= sx.ATTN_UNIFORM_REL * want.abs()).all()), worst
