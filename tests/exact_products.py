"""Exact-integer operands for the bf16 contraction kernels.

If both bf16 operands of a contraction hold small integers, every product and every partial sum is an integer below 2^24, so fp32
accumulation is exact in ANY order -- MFMA, dot instructions, atomics, private partials, LDS pre-reduction.  Every kernel form then
has to reproduce the integer matmul bit for bit at every element, and one dropped product, one misplaced row or one partial that
was not summed is a failed `torch.equal` instead of a fourth digit of a Frobenius norm.

Two regimes:

  dense      values in {-4..-1, 1..4}, never zero: dropping any single product changes the sum.  |sum| <= 16 K < 2^24 for every
             K < 2^20.  For the fp32 epilogues (first write, accumulate, device-scalar alpha).
  small-sum  values in {-1, 0, +1} with density min(1, 32 / sqrt(K)): about 1024 non-zero products per output whatever K is, so every
             output plus an integer bias in [-8, 8] stays within +-256, where bf16 holds every integer: the bf16 and
             bf16-rounded-residual epilogues are exact too, and a change of 1 is visible in them.

`exact_ref` asserts these conditions; they are conditions of the method, not measurements of the kernels.  A shape that breaks one
gets another seed or density, never another bound.  tests/test_exact_products_cpu.py checks every shape listed here without a GPU.

The decode launches that fuse RMSNorm, the residual add or SwiGLU get inputs of their own ("fused decode launches" below) that make
their bf16 operand a known integer; each generator returns the inputs together with the exact expectations.
"""
import functools
import math

import torch

EXACT_LIMIT = 2 ** 24          # fp32 holds every integer below
BF16_EXACT_LIMIT = 256         # bf16 holds every integer up to

BIAS_RANGE = 8                 # integer bias in [-8, 8]
PREFILL_RANGE = 1000           # integer contents of an accumulating output / a residual stream, in [-1000, 1000]
PAD_BF16 = 3.0                 # finite non-zero garbage in the padding of a k-major operand
SENTINEL = -77.0               # what an output buffer holds past column N (exact in bf16 and fp32)

LAYOUTS = {"nt": (False, False), "dgrad": (False, True), "wgrad": (True, True)}      # (A k-major, B k-major)


# ------------------------------------------------------------------------------------------------ operand generators
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def dense(rows, K, seed):
    """bf16 [rows, K], values in {-4..-1, 1..4}"""
    v = torch.randint(0, 8, (rows, K), generator=_gen(seed), dtype=torch.int8)
    return (v - 4 + (v >= 4).to(torch.int8)).to(torch.bfloat16)


def small_sum_density(K):
    return min(1.0, 32.0 / math.sqrt(K))


def small_sum(rows, K, seed, density=None):
    """bf16 [rows, K], values in {-1, 0, +1}, non-zero with probability min(1, 32 / sqrt(K)) (of the contraction length K)"""
    d = small_sum_density(K) if density is None else density
    g = _gen(seed)
    sign = torch.randint(0, 2, (rows, K), generator=g, dtype=torch.int8) * 2 - 1
    keep = torch.rand((rows, K), generator=g) < d
    return (sign * keep.to(torch.int8)).to(torch.bfloat16)


def int_bias(N, seed):
    """bf16 [N], integers in [-8, 8]"""
    return torch.randint(-BIAS_RANGE, BIAS_RANGE + 1, (N,), generator=_gen(seed)).to(torch.bfloat16)


def int_prefill(rows, cols, seed):
    """fp32 [rows, cols], integers in [-1000, 1000]: what an accumulating output or a residual stream holds before the launch"""
    return torch.randint(-PREFILL_RANGE, PREFILL_RANGE + 1, (rows, cols), generator=_gen(seed)).float()


# ------------------------------------------------------------------------------------------------ reference
def exact_ref(a, b, bias=None, small=False):
    """fp32 a @ b^T on the CPU of integer-valued operands a [M, K], b [N, K] -- exact, which the assertions make sure of:
    every |sum| < 2^24, and in the small-sum regime (small=True) every |sum + bias| <= 256."""
    for t in (a, b):
        f = t.float()
        assert torch.equal(f, f.round()), "operands must hold integers"
    ref = a.float() @ b.float().t()
    assert ref.abs().max().item() < EXACT_LIMIT, "a sum reaches 2^24: fp32 accumulation would no longer be exact"
    assert a.float().abs().max().item() * b.float().abs().max().item() * a.shape[1] < EXACT_LIMIT, "a partial sum could reach 2^24"
    if small:
        full = ref if bias is None else ref + bias.float()
        m = full.abs().max().item()
        assert m <= BF16_EXACT_LIMIT, f"small-sum regime: |sum + bias| reaches {m} > 256, bf16 would round it (change the seed or density)"
    else:
        assert bias is None, "a bias belongs to the bf16 epilogue: small-sum regime"
    return ref


@functools.lru_cache(maxsize=3)
def problem(M, N, K, regime):
    """(a [M, K], b [N, K], bias [N] or None, ref [M, N]) of one shape and regime -- seeded by the shape, built once and shared by the
    tests that use it (treat as read-only).  A fused regime (FUSED_REGIMES) returns the namespace of its generator below."""
    seed = (M * 1000003 + N * 10007 + K * 101 + (1 if regime == "dense" else 2)) % (2 ** 31)
    if regime in FUSED_REGIMES:
        return FUSED_REGIMES[regime](M, N, K, seed + 7 * len(regime))
    if regime == "dense":
        a, b = dense(M, K, seed), dense(N, K, seed + 1)
        return a, b, None, exact_ref(a, b)
    assert regime == "small"
    a, b, bias = small_sum(M, K, seed), small_sum(N, K, seed + 1), int_bias(N, seed + 2)
    return a, b, bias, exact_ref(a, b, bias, small=True)


# ------------------------------------------------------------------------------------------------ storage
def round_up(x, m):
    return (x + m - 1) // m * m


def store(x, kmajor, device=None):
    """logical [rows, K] -> a tensor in the requested storage order with a padded leading dimension.  k-major: [K, ld] with finite
    non-zero garbage past `rows`; row-major: [rows, round_up(K, 8) + 8] with the tail past K zero (the contract of ug_gemm_bf16: the
    8-element chunk that straddles K is fetched whole).  Returns the [K, rows] / [rows, K] view of the padded buffer."""
    rows, kk = x.shape
    if kmajor:
        buf = torch.full((kk, round_up(rows, 8) + 8), PAD_BF16, dtype=torch.bfloat16)
        buf[:, :rows] = x.t()
        view = buf if device is None else buf.to(device)
        return view[:, :rows]
    buf = torch.zeros((rows, round_up(kk, 8) + 8), dtype=torch.bfloat16)
    buf[:, :kk] = x
    view = buf if device is None else buf.to(device)
    return view[:, :kk]


def out_buffer(M, N, dtype, device, prefill=None, align=8):
    """[M, ld] output with ld = round_up(N, align) + align: `prefill` (or the sentinel) in the N live columns, the sentinel past them"""
    buf = torch.full((M, round_up(N, align) + align), SENTINEL, dtype=dtype)
    if prefill is not None:
        buf[:, :N] = prefill.to(dtype)
    return buf.to(device)


def mismatch_report(got, want, tile=(256, 256), limit=8):
    """where two [M, N] tensors differ: count, row / column extent, the 256 x 256 tiles touched, the first differences"""
    bad = (got != want) | (got.isnan() != want.isnan())
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "equal"
    rows, cols = idx[:, 0], idx[:, 1]
    tiles = sorted({(int(r) // tile[0], int(c) // tile[1]) for r, c in idx[:: max(1, idx.shape[0] // 4096)].tolist()})
    first = [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in idx[:limit].tolist()]
    return (f"{idx.shape[0]} of {got.numel()} elements differ: rows {int(rows.min())}..{int(rows.max())}, columns {int(cols.min())}.."
            f"{int(cols.max())}, {tile[0]}x{tile[1]} tiles {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; "
            f"first (row, col, got, want): {first}")


def assert_exact(buf, N, want, what=""):
    """the N live columns of `buf` equal `want` bit for bit, and the columns past N still hold the sentinel"""
    got = buf[:, :N].cpu()
    want = want.to(got.dtype)
    if not torch.equal(got, want):
        raise AssertionError(f"{what}: {mismatch_report(got.float(), want.float())}")
    if buf.shape[1] > N:
        pad = buf[:, N:].cpu()
        assert torch.equal(pad, torch.full_like(pad, SENTINEL)), f"{what}: the launch wrote past column N"


# ------------------------------------------------------------------------------------------------ fused decode launches
# The decode launches that fuse RMSNorm, the residual add or SwiGLU round to bf16 right behind the norm or the activation.  An fp32
# value within a few fp32 ulps of an integer of at most 256 rounds to that integer (bf16 moves at a relative error of 2^-9; rsqrtf,
# __expf and a division leave about 2^-21), so inputs can be chosen whose bf16 OPERAND is a known integer whatever the last bits of
# those functions are; behind the operand everything is the integer contraction of the regimes above.
#
#   rstd inside (ug_decode_sw_gate_up / _head, the xn of the finishers): stream = s * c_r, s in {-1, +1}, c_r a power of two that
#       differs by row: sum of squares K c_r^2 exactly in any order, rstd = (1 - d) / c_r with d <= eps / (2 c_r^2) = 2e-6, operand
#       bf16(w (h rstd)) = s w exactly for an integer norm weight.  Another row's statistics give s w c_r / c_r' -- not even an integer.
#   rstd at the consumer (ug_decode_gemv_resid_norm): operand bf16(norm_w * xnew), no rsqrt: xnew and norm_w in {-2, -1, 1, 2}.
#   pending accumulator: integers (times c_r) up to 320, so that bf16round(pend) really rounds (259 -> 260); stream in = target -
#       bf16round(pend), computed here: the stream out is the target bit for bit, and a launch that adds the unrounded term is off by c_r.
#   SwiGLU prologue (ug_decode_gemv_swiglu): accumulator G 2^-j | U 2^-j with ss_in = norm_cols 4^-j (rstd = 2^j (1 - d), d <= 3.2e-5);
#       G in [24, 64] -- 1 + __expf(-g) is exactly 1.0f, silu(g) = g -- or in [-120, -104] -- __expf overflows, silu(g) = -0; U in
#       {-4..-1, 1..4}: operand = G U (|G U| <= 256) or 0.
#   SwiGLU epilogue (ug_decode_sw_gate_up): gate and up pre-activations are small-sum integers g, u; see gate_up_check.
ROW_SCALES = (0.5, 1.0, 2.0, 4.0, 8.0)     # c_r, cycled over the rows
PEND_RANGE = 320                           # |pending| <= 320 (times c_r): above 256 bf16 holds even integers only
EPS = 1e-6                                 # the model's rms_norm_eps
SW_HIDDEN = 1536                           # the width ug_decode_sw_gate_up / _head are built for
SWIGLU_J = (-1, 0, 1, 2, 3)                # rstd = 2^j, cycled over the rows
SILU_ONE, SILU_ZERO = 24, -104             # g >= 24: silu(g) == g in fp32 and in fp64-then-bf16; g <= -104: silu(g) rounds to 0
TINY = 2.0 ** -100                         # see gate_up_check


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def row_scales(R):
    return torch.tensor([ROW_SCALES[r % len(ROW_SCALES)] for r in range(R)]).unsqueeze(1)


def rounding_pending(R, K, seed, scale=None):
    """fp32 [R, K]: integers in [-320, 320] (times the row's scale) -- a pending accumulator whose bf16 rounding moves a tenth of it"""
    p = torch.randint(-PEND_RANGE, PEND_RANGE + 1, (R, K), generator=_gen(seed)).float()
    p = p if scale is None else p * scale
    assert (bf16_round(p) != p).float().mean().item() > 0.05, "the pending term must really be rounded"
    return p


def _ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def norm_stream(R, K, seed):
    """the residual stream of the rstd-inside launches: target = s c_r [R, K]; pend, x_in = target - bf16round(pend); norm_w [K] in
    {-1, 0, +1} at the small-sum density of K; operand = s norm_w (what the launch has to feed its MFMAs), bf16"""
    s = (torch.randint(0, 2, (R, K), generator=_gen(seed), dtype=torch.int8) * 2 - 1).float()
    c = row_scales(R)
    target = s * c
    pend = rounding_pending(R, K, seed + 1, c)
    x_in = target - bf16_round(pend)
    assert torch.equal(x_in + bf16_round(pend), target)
    norm_w = small_sum(1, K, seed + 2)[0].float()
    operand = (s * norm_w).to(torch.bfloat16)
    # the condition the regime rests on: fp32 arithmetic as the kernels do it lands on the integer operand
    rs = torch.rsqrt((target * target).sum(-1, keepdim=True) / K + EPS)
    assert torch.equal((norm_w * (target * rs)).to(torch.bfloat16), operand)
    return _ns(target=target, pend=pend, x_in=x_in, norm_w=norm_w, operand=operand, scale=c, sign=s)


def silu_expect(g, u):
    """bf16(bf16(silu(g)) * u) with silu in fp64: what Qwen2MLP.forward gives under bf16 autocast for bf16 g, u"""
    g64 = g.double()
    return (bf16_round((g64 / (1 + torch.exp(-g64))).float()) * u.float()).to(torch.bfloat16)


def gate_up_problem(R, I, K, seed):
    """ug_decode_sw_gate_up: stream as norm_stream, w [2 I, K] small-sum (gate rows first); g, u [R, I] the exact pre-activations,
    act = silu_expect(g, u), exact = where act must match bit for bit"""
    st = norm_stream(R, K, seed)
    w = small_sum(2 * I, K, seed + 3)
    gu = exact_ref(st.operand, w, small=True)
    g, u = gu[:, :I], gu[:, I:]
    st.w, st.g, st.u, st.act = w, g, u, silu_expect(g, u)
    st.exact = (g == 0) | (g >= SILU_ONE) | (g <= SILU_ZERO)
    return st


def head_problem(R, N, K, seed):
    """ug_decode_sw_head: stream as norm_stream, w [N, K] small-sum, logits [R, N] exact"""
    st = norm_stream(R, K, seed)
    st.w = small_sum(N, K, seed + 3)
    st.logits = exact_ref(st.operand, st.w)
    return st


def finish_problem(rows, cols, _k, seed):
    """ug_decode_finish_resid_norm(_ord): acc = pend, x = x_in -> x = target, xn = s norm_w; parts [3, rows, cols]: slots that sum
    to pend in ascending order exactly"""
    st = norm_stream(rows, cols, seed)
    st.parts = split_slots(st.pend, 3, seed + 4, st.scale)
    return st


def split_slots(pend, P, seed, scale=None):
    """[P, R, K]: integer slots (times the row's scale) whose ascending fp32 sum is `pend` exactly"""
    R, K = pend.shape
    parts = torch.randint(-20, 21, (P, R, K), generator=_gen(seed)).float()
    parts = parts if scale is None else parts * scale
    parts[P - 1] = pend - parts[:P - 1].sum(0)
    acc = parts[0].clone()
    for p in range(1, P):
        acc += parts[p]
    assert torch.equal(acc, pend)
    return parts


def resid_norm_problem(R, N, K, seed):
    """ug_decode_gemv_resid_norm(_ord): xnew [R, K] and norm_w [K] in {-2, -1, 1, 2}; pend integers, x_in = xnew - bf16round(pend);
    operand = norm_w xnew (never zero: dropping any product shows); w [N, K] dense; acc [R, N], ss [R] = sum xnew^2; parts5 = five
    slots that sum to pend"""
    g = _gen(seed)
    pick = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    xnew = pick[torch.randint(0, 4, (R, K), generator=g)]
    norm_w = pick[torch.randint(0, 4, (K,), generator=g)]
    pend = rounding_pending(R, K, seed + 1)
    x_in = xnew - bf16_round(pend)
    assert torch.equal(x_in + bf16_round(pend), xnew)
    operand = (norm_w * xnew).to(torch.bfloat16)
    w = dense(N, K, seed + 3)
    return _ns(xnew=xnew, norm_w=norm_w, pend=pend, x_in=x_in, operand=operand, w=w, acc=exact_ref(operand, w),
               ss=(xnew * xnew).sum(-1), parts5=split_slots(pend, 5, seed + 4))


def swiglu_problem(R, N, K, seed):
    """ug_decode_gemv_swiglu: G, U [R, K]; gu [R, 2 K] = G 2^-j | U 2^-j, ss_unit [R] = 4^-j (ss_in = norm_cols * ss_unit);
    operand = G U where G >= 24, else 0 (a quarter of it); w [N, K] small-sum; acc [R, N]"""
    g = _gen(seed)
    G = torch.randint(SILU_ONE, 65, (R, K), generator=g).float()
    neg = torch.rand((R, K), generator=g) < 0.25
    G = torch.where(neg, torch.randint(-120, SILU_ZERO + 1, (R, K), generator=g).float(), G)
    U = dense(R, K, seed + 1).float()
    j = torch.tensor([SWIGLU_J[r % len(SWIGLU_J)] for r in range(R)]).unsqueeze(1)
    down = torch.pow(2.0, -j.float())
    gu = torch.cat([G * down, U * down], dim=1)
    operand = torch.where(neg, torch.zeros_like(G), G * U).to(torch.bfloat16)
    assert operand.float().abs().max().item() <= BF16_EXACT_LIMIT and torch.equal(operand, silu_expect(G, U))
    # the kernel's fp32 arithmetic lands on the integer operand for both norm widths (rstd = 2^j up to eps)
    for cols in (1536, 3584):
        rs = torch.rsqrt((cols * down * down) / cols + EPS)
        gg, uu = bf16_round(rs * gu[:, :K]), bf16_round(rs * gu[:, K:])
        assert torch.equal(gg, G) and torch.equal(uu, U)
        assert torch.equal((bf16_round(gg / (1 + torch.exp(-gg))) * uu).to(torch.bfloat16), operand)
    w = small_sum(N, K, seed + 3)
    return _ns(G=G, U=U, j=j, gu=gu, ss_unit=(down * down)[:, 0], operand=operand, w=w, acc=exact_ref(operand, w))


FUSED_REGIMES = {"resid_norm": resid_norm_problem, "swiglu": swiglu_problem, "gate_up": gate_up_problem, "head": head_problem,
                 "finish": finish_problem}

GATE_UP_DIFFER_CAP = 0.01


def bf16_ulp(x):
    """the bf16 ulp at |x| (fp32 tensor): 2^(exponent - 7); 0 at 0"""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def gate_up_check(got, p, what=""):
    """`got` [R, I] against the expectation of a gate_up problem -> the share of elements that differ at all.
      * where g == 0, g >= 24 or g <= -104 (p.exact): bit for bit -- silu(g) is 0, g or (rounded to bf16) 0 in any arithmetic;
      * elsewhere within two bf16 ulps of the larger magnitude: bf16(silu) can move one bf16 ulp at a rounding boundary, the product
        by the integer u is exact in fp32, and two values at most 2 ulps apart round at most 2 ulps apart;
      * at most 1 % of ALL elements differ: a launch that skips the inner bf16(silu) rounding stays within one ulp everywhere, but
        differs on a large share (tests/test_exact_products_cpu.py measures both sides of this cap).
    Magnitudes below 2^-100 count as zero on both sides: for -104 < g <= -88 fp32 exp(-g) overflows (or the quotient underflows)
    and the kernel's silu is -0, where fp64 gives up to 88 e^-88 = 5e-37 -- the two arithmetics differ there by less than 1e-34."""
    got, want = got.float().cpu(), p.act.float()
    assert got.shape == want.shape and not got.isnan().any(), what
    got, want = (torch.where(t.abs() < TINY, torch.zeros_like(t), t) for t in (got, want))
    differ = got != want
    bad = differ & p.exact
    assert not bad.any(), f"{what}: exact set: {mismatch_report(torch.where(p.exact, got, want), want)}"
    over = (got - want).abs() > 2 * bf16_ulp(torch.maximum(got.abs(), want.abs()))
    assert not over.any(), f"{what}: more than two bf16 ulps: {mismatch_report(torch.where(over, got, want), want)}"
    share = differ.float().mean().item()
    assert share <= GATE_UP_DIFFER_CAP, f"{what}: {share:.4%} of the elements differ from the expectation (cap 1 %)"
    return share


# ------------------------------------------------------------------------------------------------ launch shapes, restated
# The selection rules of csrc/decode.hip (launch_ring_auto) and csrc/decode_sw.hip (units_per_wg), so that a test can say which
# instantiation a shape reaches and the CPU test can enumerate what no shape reaches.
RING_CANDS = ((4, 1), (4, 2), (7, 2), (9, 3))          # (waves, tiles per wave)


def ring_plain_shape(R, N, K):
    """gemv_ring_kernel<RB, KW>: two tiles per wave from 3000 tiles on"""
    return (1 if R <= 16 else 2, 2 if ((N + 15) // 16) * ((K + 255) // 256) >= 3000 else 1)


def ring_fused_shape(R, N, K, xcd_major=True):
    """gemv_ring4_kernel<RB, KW, ., NW>: -> (RB, NW, KW, xcd-major grid?).  cost = ceil(workgroups / 256) * NW * KW, the first
    cheapest candidate wins; more than 16 rows take four waves; 16 or more k-slabs whose workgroups fit 32 CUs per XCD go XCD-major"""
    groups, nslabs = (N + 15) // 16, (K + 255) // 256
    best, best_cost = None, None
    for nw, kw in RING_CANDS:
        if R > 16 and nw != 4:
            continue
        blocks = -(-groups // (nw * kw)) * nslabs
        cost = -(-blocks // 256) * nw * kw
        if best_cost is None or cost < best_cost:
            best, best_cost = (nw, kw), cost
    if xcd_major and R <= 16 and nslabs >= 16 and -(-groups // 16) * -(-nslabs // 8) <= 32:
        return (1, 8, 2, True)
    return (1 if R <= 16 else 2, best[0], best[1], False)


def sw_split(nunits, ncu, max_upw, units_per_tile):
    """units_per_wg -> (units per workgroup, workgroups, tiles of a full workgroup, units of the last workgroup)"""
    upw = min(max(-(-nunits // ncu), 1), max_upw)
    grid = -(-nunits // upw)
    tiles = [min(units_per_tile, upw - t) for t in range(0, upw, units_per_tile)]
    return upw, grid, tiles, nunits - (grid - 1) * upw


# ------------------------------------------------------------------------------------------------ the shapes of the GPU files
# (M, N, K, regimes): everything tests/test_gemm_exact_gpu.py and tests/test_gemv_exact_gpu.py build goes through problem(); the CPU
# test walks these lists so that a shape that breaks a regime condition fails without a GPU.
GEMM_128 = [(130, 72, 104), (257, 129, 40), (64, 336, 256)]
GEMM_128_KMAJOR_ONLY = [(130, 72, 101)]                 # K % 8 != 0: the other operand has to be k-major (dgrad, wgrad)
GEMM_ATOMIC_SPLIT = [(64, 64, 2048), (300, 200, 1000)]
GEMM_STAGGERED = [(300, 520, 136), (771, 1536, 160)]
GEMM_STAGGERED_KMAJOR_ONLY = [(300, 520, 131)]
P10_HEIGHTS = [128, 144, 160, 176, 192, 208, 224, 240, 272, 288, 304, 320]      # policy 32 + h / 16 (40 ... 52 without 48 = 256 rows)


def p10_shape(height):
    return (2 * height + 117, 512, 96)


GEMM_P10_320 = (700, 512, 96)
GEMM_P10_AUTO = (12336, 1536, 64)
GEMM_TAIL = (4100, 3900, 2600)
GEMM_PRIVATE_WGRAD = (1536, 1040, 2100)
GEMM_PRIVATE_LONG = (1300, 1290, 65528)
WGRAD_GROUP_K = 1000
WGRAD_GROUP_SHAPES = [(300, 520), (64, 64), (777, 256), (256, 40), (130, 1000)]


def wgrad_group_k(n):
    return WGRAD_GROUP_K if n != 1 else max(40, WGRAD_GROUP_K // 3 // 8 * 8)      # the second problem has a K of its own


# (R, N, K).  The last three: the direct kernel's deeper unrolls (csrc/decode_plan.h, plan_gemv: the deepest U that leaves 2048 waves) at
# the fewest weight rows that select them -- gemv_kernel<1, 8> (2048 groups x one 256-wide slice), <1, 4> (1024 groups x two 128-wide
# slices), <1, 2> (1024 x two 64-wide); (1, 64, 32) runs <1, 1>
GEMV_SHAPES = [(16, 2048, 1536), (5, 333, 256), (16, 1536, 8960), (1, 64, 32), (16, 17920, 1536), (3, 32753, 32), (5, 16369, 160),
               (2, 16369, 96)]
# more than 16 rows: gemv_kernel<2, .> (K = 32), gemv_ring_kernel<2, 1> and, from 3000 tiles on (501 groups x 6 slabs), <2, 2>; the last
# three: gemv_kernel<2, 8>, <2, 4>, <2, 2> as above
GEMV_TALL_SHAPES = [(17, 64, 32), (24, 333, 256), (32, 2048, 1536), (24, 8016, 1536), (17, 32753, 32), (18, 16369, 160), (20, 16369, 96)]
GEMV_ORD_TALL_SHAPES = [(17, 64, 32)]          # ug_gemv_bf16_ord beyond 16 rows: gemv_ring_kernel<2, 1, true>
# tests/test_decode_exact_gpu.py (R, N, K); what each reaches is asserted in tests/test_exact_products_cpu.py
RESID_NORM_SHAPES = [(1, 16, 256), (5, 333, 1568), (16, 2048, 1536), (13, 272, 3584), (17, 333, 1568), (32, 2048, 1536),
                     (16, 8208, 1536), (16, 16400, 1536), (16, 48, 4864)]
RESID_NORM_ORD_SHAPES = [(1, 16, 256), (5, 333, 1568), (16, 2048, 1536)]
SWIGLU_SHAPES = [(1, 16, 512), (5, 100, 8992), (16, 1536, 8960), (24, 256, 8960), (16, 1552, 8960), (9, 48, 18944),
                 (16, 16400, 1536)]                    # (the last: the (9,3) workgroup, which no model size gives this launch)
SWIGLU_NORM_COLS = [1536, 3584]
GATE_UP_SHAPES = [(1, 8), (3, 264), (4, 2056), (5, 8960), (12, 10248), (13, 264), (16, 2056), (16, 8)]           # (R, I)
HEAD_SHAPES = [(1, 128), (3, 2047), (4, 4097), (5, 8192), (12, 8200), (13, 2047), (16, 4097), (16, 128)]        # (R, N)
FINISH_COLS = [4, 1536, 2048, 2052, 3584, 4096]
FINISH_ROWS = [1, 5, 16]
GEMV_KBLOCK_SHAPES = [(16, 1536, 8960), (5, 100, 1792), (16, 48, 3584)]                                # K a whole number of 1792-wide k-blocks
GEMV_SW_RESID_SHAPES = [(16, 2048, 1536), (16, 17920, 1536), (5, 333, 1536), (1, 1536, 1536)]          # K = 1536 only


def all_problems():
    """every (M, N, K, regime) the GPU files ask problem() for"""
    out = []
    both = (GEMM_128 + GEMM_128_KMAJOR_ONLY + GEMM_STAGGERED + GEMM_STAGGERED_KMAJOR_ONLY + [GEMM_TAIL])
    for s in both:
        out += [s + ("small",), s + ("dense",)]
    out += [s + ("dense",) for s in GEMM_ATOMIC_SPLIT + [GEMM_PRIVATE_WGRAD]]
    out += [p10_shape(h) + ("small",) for h in P10_HEIGHTS]
    out += [GEMM_P10_320 + ("small",), GEMM_P10_AUTO + ("small",), GEMM_PRIVATE_LONG + ("small",)]
    out += [(rows, cols, wgrad_group_k(n), "dense") for n, (rows, cols) in enumerate(WGRAD_GROUP_SHAPES)]
    for s in GEMV_SHAPES + GEMV_KBLOCK_SHAPES + GEMV_SW_RESID_SHAPES + GEMV_TALL_SHAPES:
        out += [s + ("small",), s + ("dense",)]
    out += [s + ("resid_norm",) for s in RESID_NORM_SHAPES + RESID_NORM_ORD_SHAPES]
    out += [s + ("swiglu",) for s in SWIGLU_SHAPES]
    out += [(R, I, SW_HIDDEN, "gate_up") for R, I in GATE_UP_SHAPES]
    out += [(R, N, SW_HIDDEN, "head") for R, N in HEAD_SHAPES] + [(4, 7, SW_HIDDEN, "head")]
    out += [(rows, cols, cols, "finish") for cols in FINISH_COLS for rows in FINISH_ROWS]
    return list(dict.fromkeys(out))
