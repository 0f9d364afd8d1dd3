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
    tests that use it (treat as read-only)."""
    seed = (M * 1000003 + N * 10007 + K * 101 + (1 if regime == "dense" else 2)) % (2 ** 31)
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


GEMV_SHAPES = [(16, 2048, 1536), (5, 333, 256), (16, 1536, 8960), (1, 64, 32), (16, 17920, 1536)]       # (R, N, K)
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
    for s in GEMV_SHAPES + GEMV_KBLOCK_SHAPES + GEMV_SW_RESID_SHAPES:
        out += [s + ("small",), s + ("dense",)]
    return list(dict.fromkeys(out))
