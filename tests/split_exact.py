"""Exact operands for the split-f16 and fp32 convolution / GEMM kernels and for the SigLIP attention kernel.

csrc/conv_split.hip rebuilds an fp32 product from two f16 planes per operand (a = a1 + a2) and three MFMAs per block
(w1 x2, w2 x1, w1 x1); csrc/conv_f32.hip runs the same contractions on the fp32 matrix cores.  Both accumulate in fp32.  If
  * every plane of both operands is representable (the split reconstructs the operand exactly),
  * every partial product is a multiple of one unit u, and
  * sum_k (|x1| + |x2|)_k (|w1| + |w2|)_k / u < 2^24,
then every partial sum in any order or grouping is an fp32 number, and the kernel has to give the float64 contraction bit for
bit at every element (`torch.equal`): one dropped cross product, one wrong plane row, one missing tap or slab is a failed
comparison, not a fifth digit.  These are conditions of the method, asserted here (`conditions`), never measurements of a kernel;
a shape that breaks one gets another seed or density, never a bound.  tests/test_split_exact_cpu.py checks every case listed
here without a GPU.

Three regimes (power-of-two scaling is exact, so the conditions are stated on the unscaled integers):

  int   both operands hold integers in {-4..-1, 1..4} (`dense` of tests/exact_products.py as fp32): the second plane of both is
        zero.  Indexing, taps, padding, tiles, epilogues -- also for the exact-fp32 kernels of conv_f32.hip.
  x2    activations need both planes: integers in {-4..-1, 1..4}, a quarter of them replaced by ODD integers with
        2048 < |n| < 4096 (12 significant bits: one more than an f16 holds), 4095 planted once.  The odd integers are chosen with
        |n| = 1 (mod 4) for n > 0 and |n| = 3 (mod 4) for n < 0, so that x2 = x - RNE_f16(x) is +1 unit on every such entry;
        weights are integers in {-2..2} with the maximum present and a positive mean (their second plane is zero), so that the
        cross term w1 x2 is POSITIVE at every output: a kernel that drops it is wrong everywhere, not at most places.
  w2    the mirror image: two-plane weights, integer activations.  Covers w2 x1.

The scale bound: the kernel uses only the binade of the bound it is given.  Every exact case runs with the measured bound and
with a bound from the next binade up (2 max|x|); the scaled operand then has one bit less headroom below, which `conditions`
checks as well (`loose_ok`): with it the two results must be equal bit for bit.
"""
import collections
import functools
import math
import types

import torch
import torch.nn.functional as F

import exact_products as ep

EXACT_LIMIT = 2 ** 24
F16_MAX = 65504.0
SENTINEL = -77.0
GUARD = 1024                    # elements kept behind every output buffer
REGIMES = ("int", "x2", "w2")
SBK, SBM, SBN = 32, 128, 128    # csrc/conv_split.hip: slab depth, pixel tile, channel tile
P_EXP = 14                      # csrc/siglip_attn.hip: probabilities are scaled by 2^14 before their split


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed) % (2 ** 31))


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the kernel's split, restated
def scale_exp(amax):
    """scale_exp of csrc/split_f16.h: the bound's binade [2^k, 2^(k+1)) maps to [2^14, 2^15)"""
    return max(-60, min(60, 14 - math.floor(math.log2(float(amax)))))


def split_planes(a, amax=None):
    """fp32 tensor -> (a1, a2, e): the two f16 planes of a * 2^e as fp32 tensors, exactly as split2_pair makes them
    (saturating, round to nearest even), e from the bound `amax` (default: max|a|)"""
    a = a.float()
    e = scale_exp(a.abs().max().item() if amax is None else amax)
    s = torch.ldexp(a, torch.tensor(e)).clamp(-F16_MAX, F16_MAX)
    a1 = s.half().float()
    a2 = (s - a1).half().float()
    return a1, a2, e


# ------------------------------------------------------------------------------------------------ operand generators
def ints(shape, seed):
    """fp32, integers in {-4..-1, 1..4}, never zero"""
    n = int(torch.tensor(shape).prod())
    return ep.dense(1, n, seed)[0].float().reshape(shape)


def small_ints(shape, seed):
    """fp32, integers in {-2..2}, the maximum present, mean +0.45: P(2) = P(1) = 0.3, P(0) = 0.1, P(-1) = P(-2) = 0.15"""
    u = torch.rand(shape, generator=_gen(seed))
    v = torch.full(shape, -2.0)
    for bound, val in ((0.15, -1.0), (0.30, 0.0), (0.40, 1.0), (0.70, 2.0)):
        v = torch.where(u >= bound, torch.tensor(val), v)
    assert v.max().item() == 2.0 and v.min().item() == -2.0
    return v


def two_plane(shape, seed, plant=True):
    """fp32: `ints`, a quarter replaced by odd integers 2048 < |n| < 4096 whose second plane is +1 (see the module docstring), and
    4095 (second plane -1: 4095 rounds up to 4096) planted once"""
    g = _gen(seed)
    base = ints(shape, seed + 1)
    big = torch.rand(shape, generator=g) < 0.25
    k = torch.randint(512, 1023, shape, generator=g).float()            # 4 k + 1 in [2049, 4089], 4 k + 3 in [2051, 4091]
    neg = torch.rand(shape, generator=g) < 0.5
    val = torch.where(neg, -(4 * k + 3), 4 * k + 1)
    out = torch.where(big, val, base)
    if plant:
        flat = out.view(-1)
        flat[int(torch.randint(0, flat.numel(), (1,), generator=g))] = 4095.0
    return out


def int_bias(n, seed):
    return ep.int_bias(n, seed).float()


def int_prefill(shape, seed):
    n = int(torch.tensor(shape).prod())
    return ep.int_prefill(1, n, seed)[0].reshape(shape)


def operands(regime, xshape, wshape, seed):
    """(x, w) of a regime; wshape is [Cout, Cin, k, k]"""
    if regime == "int":
        return ints(xshape, seed), ints(wshape, seed + 11)
    if regime == "x2":
        return two_plane(xshape, seed), small_ints(wshape, seed + 11)
    assert regime == "w2"
    return small_ints(xshape, seed), two_plane(wshape, seed + 11)


# ------------------------------------------------------------------------------------------------ references
def conv64(x, w, *, stride=1, pad=None, asym=False, ups=False, mode="zeros"):
    """float64 convolution of NHWC x [B, H, W, Cin] with w [Cout, Cin, k, k] -> NHWC; asym: the pad (0, 1, 0, 1) of the reference's
    Downsample; ups: nearest-2x upsampling first; mode="replicate": a WRONG border (for the rejection checks)"""
    k = w.shape[-1]
    xin = x.double().permute(0, 3, 1, 2)
    if ups:
        xin = xin.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    p = (0, 1, 0, 1) if asym else ((k // 2 if pad is None else pad),) * 4
    if any(p):
        xin = F.pad(xin, p, mode="constant" if mode == "zeros" else "replicate")
    return F.conv2d(xin, w.double(), stride=stride).permute(0, 2, 3, 1).contiguous()


def out_hw(c):
    He, We = (2 * c.H, 2 * c.W) if c.ups else (c.H, c.W)
    if c.asym:
        return (He + 1 - c.k) // c.stride + 1, (We + 1 - c.k) // c.stride + 1
    p = c.k // 2 if c.pad is None else c.pad
    return (He + 2 * p - c.k) // c.stride + 1, (We + 2 * p - c.k) // c.stride + 1


def conditions(x, w, conv, unit_x=1.0, unit_w=1.0, split=True):
    """The conditions of the method for activations x (NHWC) and weights w ([Cout, Cin, k, k]) under the contraction `conv(x, w)`:
    -> namespace(share_x2, share_w2, ratio, loose_ok, x2, w2).  For the split kernels (split=True) the planes are those of the
    kernel's own split at the measured bound and one binade up; for the fp32 kernels the operand itself is its only plane."""
    x, w = x.float(), w.float()
    if split:
        x1, x2, ex = split_planes(x)
        w1, w2, ew = split_planes(w)
        assert torch.equal((x1.double() + x2.double()) * 2.0 ** -ex, x.double()), "x: the two planes do not give the operand back"
        assert torch.equal((w1.double() + w2.double()) * 2.0 ** -ew, w.double()), "w: the two planes do not give the operand back"
        assert 2.0 ** 14 <= x1.abs().max().item() <= 2.0 ** 15 and 2.0 ** 14 <= w1.abs().max().item() <= 2.0 ** 15
        l1, l2, el = split_planes(x, 2.0 * x.abs().max().item())
        loose_ok = el == ex - 1 and torch.equal(l1 * 2.0, x1) and torch.equal(l2 * 2.0, x2)      # same planes, one bit down, nothing lost
        xa = (x1.abs() + x2.abs()).double() * 2.0 ** -ex
        wa = (w1.abs() + w2.abs()).double() * 2.0 ** -ew
        for plane, e, unit in ((x1, ex, unit_x), (x2, ex, unit_x), (w1, ew, unit_w), (w2, ew, unit_w)):
            v = plane.double() * 2.0 ** -e / unit
            assert torch.equal(v, v.round()), "a plane holds a value that is no multiple of the unit"
    else:
        x2, w2, loose_ok = torch.zeros_like(x), torch.zeros_like(w), True
        xa, wa = x.abs().double(), w.abs().double()
        for t, unit in ((x, unit_x), (w, unit_w)):
            assert torch.equal(t.double() / unit, (t.double() / unit).round())
    # sum |x| |w| over the contraction, bounded from above per output pixel with max_n |w[n]| (one output channel: cheap)
    bound = conv(xa, wa.amax(dim=0, keepdim=True)).max().item() / (unit_x * unit_w)
    assert bound < EXACT_LIMIT, f"sum |x| |w| reaches {bound / EXACT_LIMIT:.3f} * 2^24: a partial sum could be rounded"
    return _ns(share_x2=(x2 != 0).float().mean().item(), share_w2=(w2 != 0).float().mean().item(), ratio=bound / EXACT_LIMIT,
               loose_ok=loose_ok, x2=x2, w2=w2)


def slab_coverage(plane_nhwc_or_w, which):
    """second-plane entries per (tap, 32-channel slab): activations [.., Cin] -> [slabs] counts (every tap reads every pixel);
    weights [Cout, Cin, k, k] -> [taps, slabs] counts"""
    nz = plane_nhwc_or_w != 0
    if which == "x":
        cin = nz.shape[-1]
        return torch.stack([nz[..., s:s + SBK].sum() for s in range(0, cin, SBK)])
    cout, cin, kh, kw = nz.shape
    return torch.stack([torch.stack([nz[:, s:s + SBK, t // kw, t % kw].sum() for s in range(0, cin, SBK)]) for t in range(kh * kw)])


# ------------------------------------------------------------------------------------------------ launcher conditions, restated
def split_kernel(M, N):
    """launch_split (csrc/conv_split.hip): 64-channel workgroups unless the 128-channel tiling gives 512 workgroups"""
    return "conv_split_kernel<4>" if cdiv(M, SBM) * cdiv(N, SBN) >= 512 else "conv_split_kernel<2>"


def split_grid_x(M):
    """(real pixel tiles, launched: rounded up to 8 for the XCD banding)"""
    return cdiv(M, SBM), cdiv(cdiv(M, SBM), 8) * 8


def patch_kernel(B, H, W, Cout, gn):
    """ug_conv3x3_split: the 16-row eight-wave kernel from 256 of its workgroups on (CONV_BIG_MIN), else the 8-row kernel in its
    64-channel form"""
    big = B * cdiv(W, 16) * cdiv(H, 16) * cdiv(Cout, 128) >= 256
    g = "true" if gn else "false"
    return f"conv3x3_patch16_kernel<{g}>" if big else f"conv3x3_patch_dma_kernel<{g}, 2>"


def igemm_kernel(mode, Cout, vec4):
    """launch_conv_mode (csrc/conv_f32.hip): Cout > 32 selects BN = 128"""
    return f"conv_igemm_kernel<{128 if Cout > 32 else 32}, {'true' if vec4 else 'false'}, {mode}>"


def conv_vec4(Cin):
    """launch_conv, convolution: Cin % 4 == 0 (and a 16-byte aligned x, which every buffer here is)"""
    return Cin % 4 == 0


def gemm_vec4(K, lda, sa, sa2, b_nk, ldb, sb, sb2):
    """launch_conv, GEMM: every 4-element A fetch aligned and inside K; with B as [N][K] the same for B"""
    return lda % 4 == 0 and K % 4 == 0 and sa % 4 == 0 and sa2 % 4 == 0 and (not b_nk or (ldb % 4 == 0 and sb % 4 == 0 and sb2 % 4 == 0))


IGEMM_ALL = [f"conv_igemm_kernel<{bn}, {v}, {m}>" for bn in (128, 32) for v in ("true", "false") for m in (0, 1, 2)]
SPLIT_ALL = ["conv_split_kernel<2>", "conv_split_kernel<4>", "conv3x3_patch_dma_kernel<false, 2>", "conv3x3_patch_dma_kernel<true, 2>",
             "conv3x3_patch16_kernel<false>", "conv3x3_patch16_kernel<true>"]

# ------------------------------------------------------------------------------------------------ convolution cases
# entry: f32 = ug_conv2d_f32, split = ug_conv2d_split, patch = ug_conv3x3_split.  `kernel` states what the launcher selects for
# the shape (the CPU test recomputes it from the restated conditions above).  stats: groups of the epilogue statistics (integer
# regime only: the sums of squares of two-plane outputs pass 2^53).  pack_cin: channels the weights are packed for (conv_in).
Case = collections.namedtuple("Case", "name entry B H W Cin Cout k stride asym ups pad gn stats pack_cin regimes kernel")


def _case(name, entry, B, H, W, Cin, Cout, kernel, k=3, stride=1, asym=False, ups=False, pad=None, gn=False, stats=0, pack_cin=None,
          regimes=REGIMES):
    return Case(name, entry, B, H, W, Cin, Cout, k, stride, asym, ups, pad, gn, stats, pack_cin or Cin, tuple(regimes), kernel)


I = ("int",)
CONV_CASES = [
    # ---- exact fp32 im2col kernel (M = B Hout Wout; 198 straddles a 128-row tile, 99 and 12 stay below one)
    _case("f32_4_128", "f32", 2, 9, 11, 4, 128, "conv_igemm_kernel<128, true, 0>", regimes=I),
    _case("f32_13_13", "f32", 2, 9, 11, 13, 13, "conv_igemm_kernel<32, false, 0>", regimes=I),
    _case("f32_13_512", "f32", 1, 9, 11, 13, 512, "conv_igemm_kernel<128, false, 0>", regimes=I),
    _case("f32_siglip_patch", "f32", 2, 28, 42, 3, 128, "conv_igemm_kernel<128, false, 0>", k=14, stride=14, pad=0, regimes=I),
    _case("f32_down", "f32", 3, 16, 14, 8, 16, "conv_igemm_kernel<32, true, 0>", stride=2, asym=True, regimes=I),
    _case("f32_up", "f32", 2, 7, 9, 8, 40, "conv_igemm_kernel<128, true, 0>", ups=True, regimes=I),
    # ---- split im2col kernel.  297 = 3 x 99 pixels: tile 0 crosses from image 0 into image 1, tile 2 is ragged, 3 tiles launch as 8
    _case("split_k1_ragged", "split", 3, 9, 11, 36, 68, "conv_split_kernel<2>", k=1),
    _case("split_k3", "split", 2, 10, 13, 64, 132, "conv_split_kernel<2>"),                       # Cout = 4 x 33
    _case("split_down", "split", 3, 16, 14, 32, 64, "conv_split_kernel<2>", stride=2, asym=True),
    _case("split_up_ragged", "split", 2, 7, 9, 100, 68, "conv_split_kernel<2>", ups=True),
    _case("split_wide", "split", 1, 128, 128, 32, 512, "conv_split_kernel<4>", k=1),             # 128 x 4 = 512 workgroups
    _case("split_wide_k3", "split", 1, 128, 128, 32, 512, "conv_split_kernel<4>", regimes=I),
    _case("split_stats", "split", 2, 16, 16, 32, 192, "conv_split_kernel<2>", stats=16, regimes=I),   # Hout Wout = 256; 192 = 128 + 64
    _case("split_wide_stats", "split", 1, 128, 128, 32, 448, "conv_split_kernel<4>", k=1, stats=16, regimes=I),   # 128 x 4; last block 64 wide
    # ---- LDS-resident patch kernels: tiles of 8 (16) x 16 pixels cut on either edge, images smaller than one tile
    _case("patch_1x33", "patch", 2, 1, 33, 32, 64, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_7x16", "patch", 2, 7, 16, 96, 68, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_8x17", "patch", 2, 8, 17, 32, 192, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_9x15", "patch", 3, 9, 15, 96, 64, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_15x1", "patch", 2, 15, 1, 32, 68, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_16x9", "patch", 2, 16, 9, 96, 192, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_17x7", "patch", 2, 17, 7, 32, 64, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_33x8", "patch", 2, 33, 8, 32, 68, "conv3x3_patch_dma_kernel<false, 2>"),
    _case("patch_conv_in", "patch", 2, 9, 17, 4, 128, "conv3x3_patch_dma_kernel<false, 2>", pack_cin=32),
    _case("patch_stats", "patch", 2, 9, 17, 32, 192, "conv3x3_patch_dma_kernel<false, 2>", stats=16, regimes=I),
    _case("patch16_120", "patch", 1, 120, 120, 32, 512, "conv3x3_patch16_kernel<false>", regimes=I),        # 64 ragged tiles x 4 blocks
    _case("patch16_many", "patch", 11, 17, 33, 32, 512, "conv3x3_patch16_kernel<false>"),                   # 66 tiles x 4 blocks
    _case("patch16_stats", "patch", 11, 17, 33, 32, 448, "conv3x3_patch16_kernel<false>", stats=16, regimes=I),
    # ---- GroupNorm on the load path, exact (32 groups need Cin = 128: four channels per group)
    _case("patch_gn", "patch", 2, 9, 17, 128, 68, "conv3x3_patch_dma_kernel<true, 2>", gn=True, regimes=I),
    _case("patch16_gn", "patch", 22, 3, 33, 128, 512, "conv3x3_patch16_kernel<true>", gn=True, regimes=I),  # 66 tiles x 4 blocks
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
CONV_PARAMS = [(c.name, r) for c in CONV_CASES for r in c.regimes]


def case_kernel(c):
    """the instantiation the launcher selects for a convolution case, from the restated conditions"""
    Ho, Wo = out_hw(c)
    if c.entry == "f32":
        return igemm_kernel(0, c.Cout, conv_vec4(c.Cin))
    if c.entry == "split":
        return split_kernel(c.B * Ho * Wo, c.Cout)
    return patch_kernel(c.B, c.H, c.W, c.Cout, c.gn)


def gn_params(c, seed):
    """hand-built GroupNorm of 32 groups: integer mean and power-of-two rstd per (image, group), gamma in +-{1/2, 1, 2} and integer
    beta per channel -> (mu_rstd [B, 32, 2], gamma, beta)"""
    g = _gen(seed)
    mu = torch.randint(-3, 4, (c.B, 32), generator=g).float()
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.B, 32), generator=g)]
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.Cin,), generator=g)] * (torch.randint(0, 2, (c.Cin,), generator=g) * 2 - 1).float()
    beta = torch.randint(-4, 5, (c.Cin,), generator=g).float()
    return torch.stack([mu, rstd], dim=-1).contiguous(), gamma, beta


def gn_apply(x, mu_rstd, gamma, beta):
    """(x - mu) rstd gamma + beta in float64 for NHWC x and 32 groups"""
    B, H, W, C = x.shape
    xg = x.double().view(B, H, W, 32, C // 32)
    mu, rstd = mu_rstd[..., 0].double().view(B, 1, 1, 32, 1), mu_rstd[..., 1].double().view(B, 1, 1, 32, 1)
    return ((xg - mu) * rstd).view(B, H, W, C) * gamma.double() + beta.double()


@functools.lru_cache(maxsize=2)
def conv_problem(name, regime):
    """Everything of one convolution case and regime, built once (treat as read-only): x [B, H, W, Cin], w [Cout, Cin, k, k] (w_pack:
    padded with zero input channels to pack_cin), bias [Cout], res / ref [B, Ho, Wo, Cout] (ref = conv + bias + res, fp32, exact),
    raw (conv alone, float64), cond (see `conditions`), for gn: x is the raw tensor, xn the normalised one, gn = (mu_rstd, gamma,
    beta); for stats: stats [B, groups, 2] float64 and amax"""
    c = CONV_BY_NAME[name]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 31 + REGIMES.index(regime)
    conv = functools.partial(conv64, stride=c.stride, pad=c.pad, asym=c.asym, ups=c.ups)
    x, w = operands(regime, (c.B, c.H, c.W, c.Cin), (c.Cout, c.Cin, c.k, c.k), seed)
    p = _ns(case=c, regime=regime, x=x, w=w, conv=conv)
    xin, unit_x = x, 1.0
    if c.gn:
        mu_rstd, gamma, beta = gn_params(c, seed + 5)
        xn = gn_apply(x, mu_rstd, gamma, beta)
        assert torch.equal(xn.float().double(), xn)
        # the kernel's own arithmetic, step by step in fp32, lands on the same values
        B, H, W, C = x.shape
        step = ((x.view(B, H, W, 32, C // 32) - mu_rstd[..., 0].view(B, 1, 1, 32, 1)) * mu_rstd[..., 1].view(B, 1, 1, 32, 1)).view(B, H, W, C)
        assert torch.equal((step * gamma + beta).double(), xn)
        p.gn, p.xn, xin, unit_x = (mu_rstd, gamma, beta), xn.float(), xn.float(), 0.25
    p.cond = conditions(xin, w, conv, unit_x=unit_x, split=c.entry != "f32")
    p.raw = conv(xin, w)
    p.bias = int_bias(c.Cout, seed + 2)
    p.res = int_prefill(tuple(p.raw.shape), seed + 3)
    full = p.raw + p.bias.double() + p.res.double()
    assert full.abs().max().item() < EXACT_LIMIT * min(unit_x, 1.0) and torch.equal(full.float().double(), full)
    p.ref = full.float()
    p.w_pack = w if c.pack_cin == c.Cin else torch.cat([w, w.new_zeros(c.Cout, c.pack_cin - c.Cin, c.k, c.k)], dim=1)
    if c.stats:
        B, Ho, Wo, _ = full.shape
        yg = full.view(B, Ho * Wo, c.stats, c.Cout // c.stats)
        p.stats = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
        assert p.stats.abs().max().item() < 2.0 ** 53 and torch.equal(full, full.round())
        p.amax = full.abs().max().float()
    return p


def pack_weight(w, cout_pad):
    """[Cout, Cin, k, k] -> the packed [k k, Cin, cout_pad] fp32 image of ops.pack_conv_weight, zero past Cout"""
    cout, cin, kh, kw = w.shape
    wp = torch.zeros(kh * kw, cin, cout_pad)
    wp[:, :, :cout] = w.float().permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    return wp


def rejected_variants(p, nsub=8):
    """{what: differs?} -- references that miss one product, one tap, one slab or the zero border, on the first `nsub` output
    channels (a difference there is a difference of the whole output).  Only variants that exist for the case are listed: a
    product whose plane is zero in the regime, the border of a convolution without padding, the second slab of a one-slab layer."""
    c, conv = p.case, p.conv
    xin = p.xn if c.gn else p.x
    w = p.w[:nsub]
    base = conv(xin, w)
    out = {}
    if c.entry != "f32":
        x1, x2, ex = split_planes(xin)
        w1, w2, ew = split_planes(p.w)
        w1, w2, un = w1[:nsub], w2[:nsub], 2.0 ** -(ex + ew)
        terms = {"w1x2": conv(x2, w1) * un, "w2x1": conv(x1, w2) * un, "w1x1": conv(x1, w1) * un}
        assert torch.equal(terms["w1x2"] + terms["w2x1"] + terms["w1x1"], base), "the three products do not add up to the contraction"
        for k, t in terms.items():
            if (p.regime, k) in (("x2", "w1x2"), ("w2", "w2x1")) or k == "w1x1":
                out["without " + k] = not torch.equal(base - t, base)
                out["share " + k] = (t != 0).double().mean().item()
    mid = c.k * c.k // 2
    for tap in sorted({0, max(mid - 1, 0), mid, min(mid + 1, c.k * c.k - 1), c.k * c.k - 1}):
        wt, only = w.clone(), torch.zeros_like(w)
        wt[:, :, tap // c.k, tap % c.k] = 0
        only[:, :, tap // c.k, tap % c.k] = 1
        if conv(torch.ones_like(xin), only).any():          # (a corner tap of a one-row image reads nothing but the border)
            out[f"without tap {tap}"] = not torch.equal(conv(xin, wt), base)
    for s in range(0, c.Cin, SBK):
        ws = w.clone()
        ws[:, s:s + SBK] = 0
        out[f"without slab {s // SBK}"] = not torch.equal(conv(xin, ws), base)
    if c.asym or (c.k // 2 if c.pad is None else c.pad) > 0:
        out["replicated border"] = not torch.equal(conv(xin, w, mode="replicate"), base)
    return out


# ------------------------------------------------------------------------------------------------ strided GEMM / linear cases
# The operands live in flat buffers filled with integers everywhere (gaps between rows and batches included), the logical operands
# are strided views of them, and the expectation is a whole output BUFFER: the sentinel everywhere except the elements the launch has
# to write -- so guard columns, gaps between batches and the region behind the last row are compared along with the result.
Gemm = collections.namedtuple("Gemm", "name b_nk M N K lda ldb ldc inner outer sa sb sc alpha kernel")
# sa / sb / sc = (inner stride, outer stride); outer = 0: one-level batch through ug_gemm_f32, else ug_gemm_f32_nested


def _heads(name, b_nk, T, N, K, H, hd, Bn, alpha, kernel, a_off=0):
    """SigLIP's interleaving: rows of a fused projection [Bn T, 3 H hd]; head z is hd columns further, image o is T rows further"""
    ld = 3 * H * hd
    if b_nk:      # scores = q k^T: A = q rows, B = k rows ([N = T][K = hd]), C [Bn][H][T][T + 4]
        return Gemm(name, 1, T, N, K, ld, ld, T + 4, H, Bn, (hd, T * ld), (hd, T * ld), (T * (T + 4), H * T * (T + 4)), alpha, kernel)
    # out = P v: A = P [Bn][H][T][T], B = v rows ([K = T][N = hd]), C into the heads of [Bn T, H hd + 8]
    ldc = H * hd + 8
    return Gemm(name, 0, T, N, K, T, ld, ldc, H, Bn, (T * T, H * T * T), (hd, T * ld), (hd, T * ldc), alpha, kernel)


GEMM_CASES = [
    # [K][N] operand (ldb padded to the N tile by contract), N <= 32 and N > 32, aligned and not
    Gemm("kn_32_vec", 0, 130, 24, 40, 44, 32, 28, 3, 0, (130 * 44, 0), (40 * 32, 0), (130 * 28 + 8, 0), 0.5, "conv_igemm_kernel<32, true, 1>"),
    Gemm("kn_32_k37", 0, 130, 24, 37, 40, 32, 28, 3, 0, (130 * 40, 0), (40 * 32, 0), (130 * 28 + 8, 0), 2.0, "conv_igemm_kernel<32, false, 1>"),
    Gemm("kn_128_vec", 0, 70, 72, 40, 40, 128, 76, 2, 0, (70 * 40 + 4, 0), (40 * 128, 0), (70 * 76, 0), 0.25, "conv_igemm_kernel<128, true, 1>"),
    Gemm("kn_128_lda41", 0, 150, 72, 40, 41, 128, 76, 2, 0, (150 * 41, 0), (40 * 128, 0), (150 * 76, 0), 1.0, "conv_igemm_kernel<128, false, 1>"),
    # [N][K] operand
    Gemm("nk_32_vec", 1, 130, 24, 40, 44, 48, 28, 3, 0, (130 * 44, 0), (24 * 48, 0), (130 * 28 + 8, 0), 0.5, "conv_igemm_kernel<32, true, 2>"),
    Gemm("nk_32_stride", 1, 130, 24, 40, 40, 40, 28, 3, 0, (130 * 40 + 1, 0), (24 * 40, 0), (130 * 28 + 8, 0), 4.0, "conv_igemm_kernel<32, false, 2>"),
    Gemm("nk_128_vec", 1, 70, 72, 40, 40, 40, 76, 2, 0, (70 * 40, 0), (72 * 40, 0), (70 * 76, 0), 0.125, "conv_igemm_kernel<128, true, 2>"),
    Gemm("nk_128_ldb43", 1, 150, 72, 40, 40, 43, 76, 2, 0, (150 * 40, 0), (72 * 43, 0), (150 * 76, 0), 1.0, "conv_igemm_kernel<128, false, 2>"),
    # two-level batches with SigLIP's strides: 2 images x 3 heads, T = 65 tokens
    _heads("heads_scores_hd24", 1, 65, 65, 24, 3, 24, 2, 0.25, "conv_igemm_kernel<128, true, 2>"),
    _heads("heads_scores_hd9", 1, 65, 65, 9, 3, 9, 2, 0.5, "conv_igemm_kernel<128, false, 2>"),            # head stride 9: scalar loads
    _heads("heads_pv_hd24", 0, 65, 24, 65, 3, 24, 2, 1.0, "conv_igemm_kernel<32, false, 1>"),              # K = 65
    _heads("heads_pv_hd40", 0, 64, 40, 64, 3, 40, 2, 2.0, "conv_igemm_kernel<128, true, 1>"),
]
GEMM_BY_NAME = {g.name: g for g in GEMM_CASES}


def gemm_kernel(g):
    return igemm_kernel(2 if g.b_nk else 1, g.N, gemm_vec4(g.K, g.lda, g.sa[0], g.sa[1] if g.outer else 0, g.b_nk, g.ldb, g.sb[0],
                                                           g.sb[1] if g.outer else 0))


def _span(shape, strides):
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


@functools.lru_cache(maxsize=2)
def gemm_problem(name):
    """-> a_buf, b_buf (flat fp32, integers everywhere), c_expect (flat fp32: sentinel + the results + GUARD sentinels), ref
    [outer, inner, M, N]"""
    g = GEMM_BY_NAME[name]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 17
    outer = max(g.outer, 1)
    a_shape, a_str = (outer, g.inner, g.M, g.K), (g.sa[1], g.sa[0], g.lda, 1)
    if g.b_nk:
        b_shape, b_str = (outer, g.inner, g.N, g.K), (g.sb[1], g.sb[0], g.ldb, 1)
    else:
        b_shape, b_str = (outer, g.inner, g.K, g.N), (g.sb[1], g.sb[0], g.ldb, 1)
    c_shape, c_str = (outer, g.inner, g.M, g.N), (g.sc[1], g.sc[0], g.ldc, 1)
    # the [K][N] form fetches whole float4s of a row padded to the N tile: the buffer has to hold them
    b_pad = 0 if g.b_nk else (cdiv(g.N, 128) * 128 if g.N > 32 else 32) - g.N
    a_buf = ints((_span(a_shape, a_str) + 8,), seed)
    b_buf = ints((_span(b_shape, b_str) + b_pad + 8,), seed + 1)
    A = torch.as_strided(a_buf, a_shape, a_str).double()
    Bm = torch.as_strided(b_buf, b_shape, b_str).double()
    ref = g.alpha * (A @ (Bm.transpose(-1, -2) if g.b_nk else Bm))
    assert (A.abs() @ (Bm.abs().transpose(-1, -2) if g.b_nk else Bm.abs())).max().item() * max(g.alpha, 1.0) < EXACT_LIMIT
    assert torch.equal(ref.float().double(), ref)
    c_expect = torch.full((_span(c_shape, c_str) + GUARD,), SENTINEL)
    view = torch.as_strided(c_expect, c_shape, c_str)
    view.copy_(ref.float())
    assert torch.equal(view.double(), ref), "output views of different batches overlap"
    return _ns(case=g, a_buf=a_buf, b_buf=b_buf, c_expect=c_expect, ref=ref.float())


# ug_linear_f32 / ug_linear_split: y = x W^T + bias + residual with ldx > K, ldy > N and a strided residual
Linear = collections.namedtuple("Linear", "name entry M N K ldx ldw ldy ldres regimes kernel")
LINEAR_CASES = [
    Linear("f32_lin_k37", "f32", 130, 24, 37, 41, 39, 28, 30, I, "conv_igemm_kernel<32, false, 2>"),
    Linear("f32_lin_vec", "f32", 70, 72, 40, 44, 40, 76, 80, I, "conv_igemm_kernel<128, true, 2>"),
    Linear("split_lin_k36", "split", 130, 68, 36, 40, 0, 72, 76, REGIMES, "conv_split_kernel<2>"),
    Linear("split_lin_k1152", "split", 70, 132, 1152, 1156, 0, 136, 140, REGIMES, "conv_split_kernel<2>"),
]
LINEAR_BY_NAME = {c.name: c for c in LINEAR_CASES}
LINEAR_PARAMS = [(c.name, r) for c in LINEAR_CASES for r in c.regimes]


def linear_kernel(c):
    if c.entry == "f32":
        return igemm_kernel(2, c.N, gemm_vec4(c.K, c.ldx, 0, 0, True, c.ldw, 0, 0))
    return split_kernel(c.M, c.N)


def _mm(x, w):
    """the linear layer as the contraction `conditions` and `rejected_variants` take: x [1, M, 1, K], w [N, K, 1, 1]"""
    return conv64(x, w, pad=0)


@functools.lru_cache(maxsize=2)
def linear_problem(name, regime):
    """-> x_buf [M, ldx] (finite non-zero garbage past K), W [N, K], bias, res_buf [M, ldres], y_expect ([M, ldy] + GUARD flat:
    sentinel outside the N live columns), cond"""
    c = LINEAR_BY_NAME[name]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 13 + REGIMES.index(regime)
    x, w = operands(regime, (1, c.M, 1, c.K), (c.N, c.K, 1, 1), seed)
    cond = conditions(x, w, _mm, split=c.entry != "f32")
    raw = _mm(x, w).view(c.M, c.N)
    bias, res = int_bias(c.N, seed + 2), int_prefill((c.M, c.N), seed + 3)
    full = raw + bias.double() + res.double()
    assert full.abs().max().item() < EXACT_LIMIT
    x_buf = torch.full((c.M, c.ldx), 3.0)
    x_buf[:, :c.K] = x.view(c.M, c.K)
    res_buf = torch.full((c.M, c.ldres), 5.0)
    res_buf[:, :c.N] = res
    y_expect = torch.full((c.M * c.ldy + GUARD,), SENTINEL)
    y_expect[:c.M * c.ldy].view(c.M, c.ldy)[:, :c.N] = full.float()
    return _ns(case=c, regime=regime, x=x, w=w, conv=_mm, cond=cond, x_buf=x_buf, W=w.view(c.N, c.K).contiguous(), bias=bias, res_buf=res_buf,
               y_expect=y_expect, ref=full.float())


def linear_as_case(c):
    """a Linear as the Case `rejected_variants` reads"""
    return _case(c.name, c.entry, 1, c.M, 1, c.K, c.N, c.kernel, k=1, pad=0, regimes=c.regimes)


# ------------------------------------------------------------------------------------------------ split weight image
WEIGHT_IMAGE = dict(taps=9, Cin=36, Cout=68, cout_pad=256)          # ragged second slab (4 of 32 channels), 188 padding rows


def weight_image_expect(wp):
    """packed fp32 weights [taps, Cin, cout_pad] -> (planes [taps, kslabs, nblks, 2, 128, 32] in LOGICAL chunk order, as the
    kernel's split makes them -- zero in the padding channels --, ew)"""
    taps, cin, cpad = wp.shape
    ks = cdiv(cin, SBK)
    full = torch.zeros(taps, ks * SBK, cpad)
    full[:, :cin] = wp
    w1, w2, ew = split_planes(full, wp.abs().max().item())
    planes = torch.stack([w1, w2], dim=0).view(2, taps, ks, SBK, cpad // SBN, SBN)      # [plane, tap, slab, c, nblk, row]
    return planes.permute(1, 2, 4, 0, 5, 3).contiguous(), ew


def weight_image_logical(buf, taps, cin, cpad):
    """the fp16 tile image ug_conv_split_weights wrote (without the trailing record) -> [taps, kslabs, nblks, 2, 128, 32] fp32 in
    logical chunk order: row r stores its 8-element chunk c at position c ^ swz_q(r), swz_q(r) = ((r >> 2) & 1) << 1"""
    ks, nb = cdiv(cin, SBK), cpad // SBN
    t = buf[:taps * ks * nb * 2 * SBN * SBK].view(taps, ks, nb, 2, SBN, 4, 8).float()
    r = torch.arange(SBN, device=buf.device)
    stored = torch.arange(4, device=buf.device)[None, :] ^ (((r[:, None] >> 2) & 1) << 1)
    idx = stored[None, None, None, None, :, :, None].expand_as(t)
    return torch.gather(t, 5, idx).reshape(taps, ks, nb, 2, SBN, SBK)


# ------------------------------------------------------------------------------------------------ SigLIP attention
ATTN_SHAPES = [(2, 65, 2, 40), (1, 130, 3, 72), (1, 64, 1, 80)]          # (B, T, H, hd); 65 and 130: a ragged last tile of 64 keys
# Select regime.  With distinct +-1 key codes and q_t = G code[sel(t)], the score of key sel(t) is scale G hd and every other key's
# is at most scale G (hd - 2): the margin is 2 scale G.  The kernel (csrc/siglip_attn.hip) computes p = __expf(s - m) -- exp2 of a
# product, relative error below 2^-20 --, scales it by 2^P_EXP and rounds to f16, whose smallest subnormal is 2^-24: a value
# below 2^-25 rounds to zero in both planes.  Three things have to vanish:
#   p 2^14 < 2^-25                        every other probability is an exact zero operand          margin > 39 ln 2 = 27.04
#   (T - 1) p < 2^-25                     l_i = 1 + (sum of the others) rounds to 1                 margin > (25 + log2 T) ln 2
#   alpha 64 max|v| < 2^-25               an earlier tile's accumulator (at most 64 keys of weight <= 1), rescaled by
#                                         alpha = __expf(m_old - m_new) <= e^-margin, is below half an ulp of any non-zero result
#                                         (>= 1 unit: v is never zero)                             margin > (31 + log2 max|v|) ln 2 = 29.8
# G is the power of two that puts the margin into [32, 64).
ATTN_MARGIN_MIN = 32.0


def attn_gain(hd):
    scale = hd ** -0.5
    G = 2.0 ** math.ceil(math.log2(ATTN_MARGIN_MIN / (2.0 * scale)))
    return G, scale


@functools.lru_cache(maxsize=2)
def attn_select_problem(B, T, H, hd, v_regime):
    """-> qkv [B T, 3 H hd + 4] (q | k | v, four garbage columns behind), sel [B, H, T], expect [B, T, H, hd] = v[b, sel, h], G, scale"""
    seed = B * 7919 + T * 131 + H * 17 + hd + (0 if v_regime == "int" else 1)
    g = _gen(seed)
    G, scale = attn_gain(hd)
    margin = 2.0 * scale * G
    code = (torch.randint(0, 2, (B, H, T, hd), generator=g) * 2 - 1).float()
    flat = code.view(B * H, T, hd)
    for z in range(B * H):
        assert torch.unique(flat[z], dim=0).shape[0] == T, "key codes must be distinct (another seed)"
    sel = torch.randint(0, T, (B, H, T), generator=g)
    sel[:, :, 0], sel[:, :, 1] = T - 1, 0
    for tile in range(cdiv(T, 64)):                       # a key of every 64-key tile, the ragged one included
        sel[:, :, 2 + tile] = min(tile * 64 + 37, T - 1)
    for tile in range(cdiv(T, 64)):
        assert ((sel >= tile * 64) & (sel < tile * 64 + 64)).any(dim=-1).all()
    q = G * torch.gather(code, 2, sel[..., None].expand(B, H, T, hd))
    v = ints((B, H, T, hd), seed + 1) if v_regime == "int" else two_plane((B, H, T, hd), seed + 1)
    assert (v != 0).all()
    vmax = v.abs().max().item()
    # the conditions above, with a factor 2^-20 of slack for __expf
    p_other = math.exp(-margin) * (1 + 2.0 ** -20)
    assert margin >= ATTN_MARGIN_MIN and p_other * 2.0 ** P_EXP < 2.0 ** -25 and (T - 1) * p_other < 2.0 ** -25
    assert p_other * 64 * vmax < 2.0 ** -25
    # scores as fp64 restate the margin: the selected key wins by at least `margin`
    s = scale * (q.double() @ code.double().transpose(-1, -2))
    top = s.gather(-1, sel[..., None])
    s_other = s.scatter(-1, sel[..., None], float("-inf"))
    assert ((top - s_other.max(dim=-1, keepdim=True).values) >= margin - 1e-9).all()
    # one scale for q, k and v; every plane representable (q = +-G, k = +-1, v as in the regime)
    amax = max(G, vmax)
    for t in (q, code, v):
        t1, t2, e = split_planes(t, amax)
        assert torch.equal((t1.double() + t2.double()) * 2.0 ** -e, t.double())
    D = H * hd
    qkv = torch.full((B * T, 3 * D + 4), 9.0)
    for i, t in enumerate((q, code, v)):
        qkv[:, i * D:(i + 1) * D] = t.permute(0, 2, 1, 3).reshape(B * T, D)
    expect = torch.gather(v, 2, sel[..., None].expand(B, H, T, hd)).permute(0, 2, 1, 3).contiguous()
    return _ns(qkv=qkv, sel=sel, expect=expect, G=G, scale=scale, margin=margin, share_v2=(split_planes(v, amax)[1] != 0).float().mean().item())


@functools.lru_cache(maxsize=2)
def attn_uniform_problem(B, T, H, hd):
    """q = 0: every probability is 1 (2^14 in f16), l_i = T, out = sum_t v / T.  -> qkv, total [B, H, hd] (float64 sum of v), exact
    (T a power of two: the quotient is exact), quotient [B, 1, H, hd] float64"""
    seed = B * 7919 + T * 131 + H * 17 + hd + 5
    D = H * hd
    k, v = ints((B, H, T, hd), seed), ints((B, H, T, hd), seed + 1)
    qkv = torch.full((B * T, 3 * D + 4), 9.0)
    qkv[:, :D] = 0.0
    for i, t in ((1, k), (2, v)):
        qkv[:, i * D:(i + 1) * D] = t.permute(0, 2, 1, 3).reshape(B * T, D)
    total = v.double().sum(dim=2)
    assert v.abs().double().sum(dim=2).max().item() < EXACT_LIMIT       # the accumulator holds integers in units of 2^(e + 14)
    return _ns(qkv=qkv, total=total, quotient=(total / T).unsqueeze(1), exact=(T & (T - 1)) == 0)


ATTN_UNIFORM_REL = 2.0 ** -22          # one rounding in o_unscale / l_i, one in the product: (1 + 2^-24)^2 - 1 < 2^-22
