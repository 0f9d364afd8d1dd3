"""Float64 restatements of the element-wise kernels (RMSNorm forward / backward, AdamW, the fp32 -> bf16 cast, the tokenizer's
GroupNorm and row softmax), the inputs their tests use, and the bars those tests judge by.  Plain torch on the CPU:
tests/test_elementwise_ref_cpu.py checks all of it without a GPU, tests/test_elementwise_gpu.py puts the kernels in the restatements'
place.  The method is that of tests/train_rows_ref.py, whose helpers are reused.

A restatement is the operation in float64 that keeps the kernel's CONTRACTUAL rounding points -- the bf16 output, and an fp32 value
that is handed to another kernel (rstd of RMSNorm, (mean, rstd) of GroupNorm) -- and nothing else of the kernel.

How an output is judged (docs/experiments.md, "Element-wise kernels: exact and per-element tests"):

  exact      RMSNorm backward on integer-valued inputs (dw at every width, dres at power-of-two widths), the cast, AdamW against
             its operation-by-operation fp32 restatement, GroupNorm of a constant group without swish: torch.equal.
  otherwise  |got - v| <= 2^-8 |v| (bf16 outputs only) + slack * a [+ floor], per element.  v: the float64 value before its last
             rounding; a: the magnitude the fp32 error of the formula scales with (stated at each restatement); slack = MARGIN x the
             worst distance, in units of a, of a plain fp32 torch evaluation of the same formula on the CPU from float64, on these
             tests' own inputs, no kernel involved.  The distances are the *_DIST constants below with the case each came from;
             test_elementwise_ref_cpu.py measures them again and requires each constant within a factor of two of what it measures.
"""
import functools
import math
import types

import numpy as np
import torch

from exact_products import SENTINEL, round_up  # noqa: F401  (re-exported for the tests)
from train_rows_ref import BF, MARGIN, _gen, excess

F32 = np.float32
U64_OVER_U32 = 2.0 ** -29       # one float64 rounding in units of one fp32 rounding
EPS = float(F32(1e-6))          # rms_norm_eps / GroupNorm eps as the kernels receive it: a C float

# ---- measured on the CPU, fp32 torch evaluation against float64, worst over every case of the family (test_constants_*) ----
RMS_RSTD_DIST = 1.25e-7         # rstd, relative: rsqrt(mean(x^2) + eps) at (9, 1536)
RMS_Y_DIST = 2.33e-7            # w * (x * rstd), relative to |v|: (9, 1536)
RMS_BWD_DRES_DIST = 1.44e-7     # dres, in units of |dres0| + r (|g| + |xhat| mean|g xhat|): (37, 1536)
RMS_BWD_DW_DIST = 1.52e-7       # dw, in units of sum_rows |dy xhat|: (5, 1536)
ADAM_P_DIST = 1.89e-7           # p, in units of |p decay| + step_size * a_m / denom: weight_decay = 0 set, n = 15367
ADAM_M_DIST = 1.50e-7           # m, in units of |m| + w1 (|gr| + |m|): p_bf16 = None set, n = 15367
ADAM_V_DIST = 1.38e-7           # v, relative (every term is positive): beta2 = 0.95 set at step 100000, n = 15367
GN_STAT_DIST = 5.92e-8          # (mean, rstd), in units of a_mean / a_rstd: the fp32 rounding of a float64 value, (3, 128 * 128, 128, 32)
GN_Y_DIST = 2.30e-7             # (x - mu) rstd gamma + beta, in units of |x - mu| a_rstd |gamma| + |beta|: (2, 300 * 300, 32, 8)
GN_SWISH_DIST = 2.81e-7         # the same through o / (1 + exp(-o)), both sides times the swish factor: (3, 128 * 128, 128, 32)
SOFTMAX_DIST = 1.84e-7          # softmax, in units of v (1 + |scale x - max|): (2, 4097) at scale 1
SOFTMAX_FLOOR = 2.0 ** -126     # the smallest normal fp32: below it an fp32 output holds no relative precision (exp(-600) is 0)

RMS_RSTD_SLACK = MARGIN * RMS_RSTD_DIST
RMS_Y_SLACK = MARGIN * RMS_Y_DIST
RMS_BWD_DRES_SLACK = MARGIN * RMS_BWD_DRES_DIST
RMS_BWD_DW_SLACK = MARGIN * RMS_BWD_DW_DIST
ADAM_P_SLACK = MARGIN * ADAM_P_DIST
ADAM_M_SLACK = MARGIN * ADAM_M_DIST
ADAM_V_SLACK = MARGIN * ADAM_V_DIST
GN_STAT_SLACK = MARGIN * GN_STAT_DIST
GN_Y_SLACK = MARGIN * GN_Y_DIST
GN_SWISH_SLACK = MARGIN * GN_SWISH_DIST
SOFTMAX_SLACK = MARGIN * SOFTMAX_DIST


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def fp32_excess(got, v, a, slack, floor=0.0):
    """the rule for an fp32 output as a ratio per element: <= 1 passes (no 2^-8 |v| term)"""
    bar = slack * a + floor
    diff = (got.double() - v).abs()
    return torch.where(diff == 0, torch.zeros_like(diff), diff / bar.clamp_min(1e-300))


def dist(got, v, a):
    """worst |got - v| in units of a (elements whose a is 0 have to be exact)"""
    diff = (got.double() - v).abs()
    assert (diff[a == 0] == 0).all()
    return (diff[a > 0] / a[a > 0]).max().item() if (a > 0).any() else 0.0


# ================================================================================================ RMSNorm forward
RMS_FWD_WIDTHS = [4, 252, 256, 260, 1536, 2048, 2052, 3584]       # the register kernel up to 2048, the two-pass kernel beyond
RMS_FWD_ROWS = [1, 5, 9]                                            # 5: a partial four-wave workgroup
RMS_PLANTS = ("zero", "small", "outlier")


def _plant(row, kind, g):
    if kind == "zero":
        row.zero_()
    elif kind == "small":
        row.copy_(torch.randn(row.shape, generator=g) * 1e-4)       # mean(x^2) ~ 1e-8: eps = 1e-6 dominates
    elif kind == "outlier":
        row[int(torch.randint(0, row.numel(), (1,), generator=g))] = 1e4
    return row


@functools.lru_cache(maxsize=None)
def rms_fwd_inputs(rows, cols):
    """-> (w fp32 [cols], list of x fp32 [rows, cols]).  From five rows on ONE x whose rows 1, 2, 3 are the planted ones (all zero;
    |x| ~ 1e-4; one 1e4 outlier); a single row cannot hold them, so rows = 1 gives four inputs: random and each planted row."""
    g = _gen(100003 * rows + cols)
    w = torch.randn(cols, generator=g) * 0.1 + 1
    if rows >= 4:
        x = torch.randn(rows, cols, generator=g) * 3
        for r, kind in enumerate(RMS_PLANTS):
            _plant(x[1 + r], kind, g)
        return w, [x]
    xs = [torch.randn(rows, cols, generator=g) * 3]
    for kind in RMS_PLANTS:
        x = torch.randn(rows, cols, generator=g) * 3
        _plant(x[0], kind, g)
        xs.append(x)
    return w, xs


def rms_fwd_restated(x, w, eps=EPS, no_eps=False, pad_to=None):
    """float64: rstd = (mean(x^2) + eps)^-1/2 (the value before its fp32 rounding), y = w x rstd (before its bf16 / fp32 rounding).
    a of rstd and of y is the value's own magnitude: every term of the sum of squares is positive, the rest are products.
    no_eps / pad_to: the wrong references of the bars-must-bite test."""
    xd = x.double()
    ms = (xd * xd).sum(-1) / (x.shape[1] if pad_to is None else round_up(x.shape[1], pad_to))
    rstd = 1.0 / torch.sqrt(ms + (0.0 if no_eps else eps))
    if no_eps:
        rstd = torch.where(ms > 0, rstd, 1.0 / torch.sqrt(ms + eps))
    return _ns(rstd=rstd, y=w.double() * (xd * rstd[:, None]))


def rms_fwd_fp32(x, w, eps=EPS):
    """the same formula in fp32 by torch on the CPU (the yardstick of the slacks, never a reference)"""
    r = torch.rsqrt((x * x).sum(-1) / x.shape[1] + eps)
    return r, w * (x * r[:, None])


def rms_rstd_excess(got, ref):
    return fp32_excess(got, ref.rstd, ref.rstd.abs(), RMS_RSTD_SLACK).max().item()


def rms_y_excess(got, ref):
    """bf16 or fp32 y by its dtype"""
    if got.dtype == BF:
        return excess(got, ref.y, ref.y.abs(), RMS_Y_SLACK).max().item()
    return fp32_excess(got, ref.y, ref.y.abs(), RMS_Y_SLACK).max().item()


# ================================================================================================ RMSNorm backward
RMS_BWD_DW_WIDTHS = [4, 252, 256, 260, 1024, 1536, 2048]
RMS_BWD_DRES_EXACT_WIDTHS = [4, 256, 1024, 2048]                    # powers of two: dot = sum / cols is exact
RMS_BWD_ROWS = [1, 5, 16, 17, 37]                                   # 17: a second workgroup holding one row
RMS_BWD_MANY_ROWS = (7700, 256)                                     # leaves the 16-row floor: 20 rows per workgroup, 385 workgroups
RMS_BWD_REAL_CASES = [(r, c) for c in (252, 260, 1536) for r in (5, 37)]


@functools.lru_cache(maxsize=4)
def rms_bwd_int_input(rows, cols):
    """x integers in [-2, 2], rstd in {1, 0.5}, w in {+-1, +-0.5}, dy (bf16) integers in [-2, 2], dres0 integers in [-8, 8], dw0
    non-zero integers in +-[1, 9]"""
    g = _gen(7 * rows + 1000003 * cols)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)          # noqa: E731
    x = ri(-2, 2, rows, cols).float()
    rstd = torch.tensor([1.0, 0.5])[ri(0, 1, rows)]
    w = torch.tensor([1.0, -1.0, 0.5, -0.5])[ri(0, 3, cols)]
    dy = ri(-2, 2, rows, cols).to(BF)
    dres0 = ri(-8, 8, rows, cols).float()
    dw0 = (ri(1, 9, cols) * (ri(0, 1, cols) * 2 - 1)).float()
    return _ns(x=x, rstd=rstd, w=w, dy=dy, dres0=dres0, dw0=dw0)


@functools.lru_cache(maxsize=None)
def rms_bwd_real_input(rows, cols):
    """the distribution of test_rmsnorm_fwd_bwd; rstd: the float64 forward's, rounded to fp32 (an INPUT of the backward); dw0 = 0"""
    g = _gen(13 * rows + 1000003 * cols)
    x = torch.randn(rows, cols, generator=g) * 3
    w = torch.randn(cols, generator=g) * 0.1 + 1
    dy = torch.randn(rows, cols, generator=g).to(BF)
    dres0 = torch.randn(rows, cols, generator=g)
    return _ns(x=x, rstd=rms_fwd_restated(x, w).rstd.float(), w=w, dy=dy, dres0=dres0, dw0=torch.zeros(cols))


def rms_bwd_restated(p, pad_to=None, skip_row_col=None, stale_quad=None):
    """float64: xhat = x rstd, g = dy w, dot = mean(g xhat), dres = dres0 + rstd (g - xhat dot), dw = dw0 + sum_rows dy xhat.
    dres_a = |dres0| + r (|g| + |xhat| mean|g xhat|), dw_a = sum_rows |dy xhat| (+ |dw0|): the magnitudes the terms cancel from.
    steps: every intermediate, for the exactness conditions of the integer inputs.
    pad_to / skip_row_col = (row, col) / stale_quad = (row, first col): the wrong references of the bars-must-bite test."""
    x, r, w, dy = p.x.double(), p.rstd.double()[:, None], p.w.double(), p.dy.double()
    cols = x.shape[1]
    xhat, g = x * r, dy * w
    gx = g * xhat
    n = cols if pad_to is None else round_up(cols, pad_to)
    dot = gx.sum(-1, keepdim=True) / n
    upd = r * (g - xhat * dot)
    dres = p.dres0.double() + upd
    dyx = dy * xhat
    dw = p.dw0.double() + dyx.sum(0)
    if skip_row_col is not None:
        dw[skip_row_col[1]] -= dyx[skip_row_col]
    if stale_quad is not None:
        dres[stale_quad[0], stale_quad[1]:stale_quad[1] + 4] = p.dres0.double()[stale_quad[0], stale_quad[1]:stale_quad[1] + 4]
    return _ns(dres=dres, dw=dw, dres_a=p.dres0.double().abs() + r * (g.abs() + xhat.abs() * gx.abs().sum(-1, keepdim=True) / cols),
               dw_a=dyx.abs().sum(0) + p.dw0.double().abs(),
               steps=dict(xhat=xhat, g=g, gx=gx, dot=dot, xhat_dot=xhat * dot, diff=g - xhat * dot, upd=upd, dres=dres, dyx=dyx, dw=dw))


def rms_bwd_fp32(p):
    """the same formulas in fp32 by torch on the CPU (the yardstick of the slacks, never a reference) -> dres, dw"""
    x, r, w, dy = p.x, p.rstd[:, None], p.w, p.dy.float()
    xhat, g = x * r, dy * w
    dot = (g * xhat).sum(-1, keepdim=True) / x.shape[1]
    return p.dres0 + r * (g - xhat * dot), p.dw0 + (dy * xhat).sum(0)


# ================================================================================================ AdamW
ADAM_SIZES = [1, 2, 3, 515, 4099, 3 * 2 * 512 * 5 + 7]
ADAM_MAX_BLOCKS = [0, 2]
_BASE = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, first_step=1, grad_scale=1.0, factor=None, bf16=True, zeros=False)
ADAM_SETS = {
    "base": dict(_BASE),
    "no_decay": dict(_BASE, wd=0.0),
    "late_steps": dict(_BASE, beta2=0.95, first_step=100000),        # both bias corrections are 1 to fp32
    "large_eps": dict(_BASE, eps=1e-3),
    "grad_scale": dict(_BASE, grad_scale=0.125),
    "device_factor": dict(_BASE, grad_scale=0.125, factor=0.37),      # ug_adamw_flat_dev: the scale is ONE fp32 product
    "no_bf16_copy": dict(_BASE, bf16=False),
    "zero_grads": dict(_BASE, zeros=True),
}


def adam_state(n, name):
    """a random non-zero state: p, m fp32 randn-like, v > 0; three gradients (with exact zeros in a third of the places if asked)"""
    hp = ADAM_SETS[name]
    g = _gen(n * 31 + sorted(ADAM_SETS).index(name))
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01 + 1e-4
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    if hp["zeros"]:
        for gr in grads:
            gr[torch.rand(n, generator=g) < 1 / 3] = 0.0
            gr[0] = 0.0
    return p, m, v, grads


def adam_consts(hp, step, f64=False):
    """the constants as adamw_flat_launch (host, double, cast to float) and adam_consts (device, fp32, contraction off) form them;
    f64: the same expressions of the SAME fp32-rounded hyper-parameters, in float64 throughout"""
    lr, b1, b2, eps, wd, gs = (F32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "grad_scale"))
    bc1 = 1.0 - math.pow(float(b1), float(step))
    bc2_sqrt = math.sqrt(1.0 - math.pow(float(b2), float(step)))
    if f64:
        lr, b1, b2, eps, wd, gs = (float(t) for t in (lr, b1, b2, eps, wd, gs))
        gsf = gs if hp["factor"] is None else gs * float(F32(hp["factor"]))
        return _ns(gs=gsf, decay=1.0 - lr * wd, w1=1.0 - b1, beta2=b2, w2=1.0 - b2, bc2_sqrt=bc2_sqrt, eps=eps, step_size=lr / bc1)
    gsf = gs if hp["factor"] is None else gs * F32(hp["factor"])
    c = _ns(gs=gsf, decay=F32(1) - lr * wd, w1=F32(1) - b1, beta2=b2, w2=F32(1) - b2, bc2_sqrt=F32(bc2_sqrt), eps=eps, step_size=lr / F32(bc1))
    assert all(isinstance(t, np.floating) and t.dtype == np.float32 for t in vars(c).values())
    return _ns(**{k: float(t) for k, t in vars(c).items()})


def ieee_sqrt(t):
    """the correctly rounded square root.  torch.sqrt of an fp32 tensor on the CPU is a vector-library routine that is an ulp off on
    about 0.7 % of these inputs; numpy's is the IEEE instruction (test_elementwise_ref_cpu.py checks it against the float64 root
    rounded once -- 53 bits are enough for that to be the correct rounding of an fp32 root)."""
    return torch.from_numpy(np.sqrt(t.numpy())) if t.dtype == torch.float32 else torch.sqrt(t)


def adam_step(p, g, m, v, c, variant=None):
    """adamw_element, one IEEE operation per line, in the dtype of the tensors (fp32: the bit-exact restatement; float64: the
    reference of the per-element rule).  -> p, m, v and the magnitudes a_p, a_m, a_v the rule scales with.
    variant: the wrong references of the bars-must-bite test."""
    gr = g * c.gs
    pk = p * c.decay
    if variant == "decay_after":
        pk = p
    mk = m + (gr - m) * c.w1
    gv = g if variant == "scale_m_only" else gr
    vk = v * c.beta2 + (c.w2 * gv) * gv
    if variant == "eps_inside":
        denom = ieee_sqrt(vk + c.eps) / c.bc2_sqrt
    else:
        denom = ieee_sqrt(vk) / c.bc2_sqrt + c.eps
    pn = pk - c.step_size * (mk / denom)
    if variant == "decay_after":
        pn = pn * c.decay
    a_m = m.abs() + (gr.abs() + m.abs()) * c.w1
    return pn, mk, vk, _ns(p=pk.abs() + c.step_size * (a_m / denom), m=a_m, v=vk.abs())


# ================================================================================================ cast
CAST_LOW_HALVES = [0x0000, 0x7fff, 0x8000, 0x8001, 0xffff]
CAST_GRID_CAP = 256 * 8 * 256 * 4                                  # elements one pass of grid_for's capped grid covers
# 1 + 2^-8 (a tie: down to even), 1 + 3 2^-8 (a tie: up to even), just below fp32 max (up to infinity), -0, the smallest subnormals
CAST_SPECIAL = [0x3f808000, 0x3f818000, 0x7f7fffff, 0x80000000, 0x00008001]
CAST_LENGTHS = [1, 2, 3, 5, 65536 * 5 + 3, 7 * 65536 * 5 + 1]


@functools.lru_cache(maxsize=1)
def cast_pattern():
    """fp32 [5 * 65536]: every upper half with each of CAST_LOW_HALVES"""
    hi = torch.arange(65536, dtype=torch.int64) << 16
    bits = torch.cat([hi | lo for lo in CAST_LOW_HALVES])
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)


def cast_input(n):
    """the special values first for the short lengths; the whole pattern (repeated) with the special values in the scalar tail beyond"""
    sp = torch.tensor([b - 2 ** 32 if b >= 2 ** 31 else b for b in CAST_SPECIAL], dtype=torch.int32).view(torch.float32)
    if n <= len(CAST_SPECIAL):
        return sp[:n].clone()
    pat = cast_pattern()
    body = n // pat.numel() * pat.numel()
    return torch.cat([pat.repeat(n // pat.numel()), sp[:n - body]])


def cast_expected(x):
    """torch's round-to-nearest-even as int16, and where the input is a NaN (there only "a NaN" is required)"""
    return x.to(BF).view(torch.int16), x.isnan()


def cast_truncated(x):
    """the wrong reference: the upper half as it stands"""
    return (x.view(torch.int32) >> 16).to(torch.int16)


def is_bf16_nan(bits):
    b = bits.to(torch.int32) & 0x7fff
    return b > 0x7f80


# ================================================================================================ GroupNorm
# (B, H, W, C, groups)
GN_CASES = [(1, 1, 1, 128, 32), (2, 7, 9, 64, 16), (3, 5, 13, 1024, 32), (2, 25, 28, 32, 8), (3, 128, 128, 128, 32), (2, 300, 300, 32, 8)]
GN_CONST = 1.5                  # the constant group: n * 1.5 and n * 2.25 are exact in float64
GN_BIG_MEAN, GN_BIG_SPREAD = 1000.0, 1e-2


def gn_chain(B, HW, C, G):
    """The longest chain of float64 additions one element's contribution passes through in ug_groupnorm_stats, from its launch
    geometry (gn_pixels_per_block): four per pixel a thread walks, the 256 / G threads of a workgroup that share a group's LDS slot,
    the workgroups of an image that share its global slot, and the division and subtraction of the finish."""
    ppb = min(max(round_up((B * HW + 2047) // 2048, 64), 64), 1024)
    pstep = 256 // (C // 4)
    return 4 * -(-ppb // pstep) + 256 // G + -(-HW // ppb) + 2


@functools.lru_cache(maxsize=2)
def gn_input(case):
    """x fp32 NHWC, gamma, beta.  Image 0, group 1 is constant; the last group of the last image has mean 1000 and spread 1e-2."""
    B, H, W, C, G = case
    g = _gen(B * 1000003 + H * W * 101 + C + G)
    x = torch.randn(B, H, W, C, generator=g) * 2 + 0.5
    cpg = C // G
    x[0, :, :, cpg:2 * cpg] = GN_CONST
    x[B - 1, :, :, C - cpg:] = GN_BIG_MEAN + GN_BIG_SPREAD * torch.randn(H, W, cpg, generator=g)
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g)


@functools.lru_cache(maxsize=2)
def gn_int_input(case):
    """integers in [-8, 8]: the float64 sums are exact in any order, so host sums and device sums are the same bits"""
    B, H, W, C, G = case
    return torch.randint(-8, 9, (B, H, W, C), generator=_gen(B + H * W + C + G)).float()


def gn_groups(x, G):
    B, H, W, C = x.shape
    return x.double().reshape(B, H * W, G, C // G)


def gn_stats_restated(x, G, eps=EPS, unbiased=False):
    """float64, two passes (no cancellation): mean, rstd [B, G] before their fp32 rounding, and the magnitudes of the rule.

    The kernels hold float64 sums s1, s2 and form var = s2 / n - mean^2.  A sum of n terms in which every term passes through at most
    k additions is off by at most k 2^-53 of the sum of the magnitudes (Higham, Accuracy and Stability, 4.2), so
        |d mean| <= k 2^-53 mean|x|,      |d var| <= k 2^-53 (mean(x^2) + 2 |mean| mean|x|),
    and d rstd / rstd = d var / (2 (var + eps)).  With the one fp32 rounding of the result as the unit:
        a_mean = |mean| + k 2^-29 mean|x|,      a_rstd = rstd (1 + k 2^-29 (mean(x^2) + 2 |mean| mean|x|) / (2 (var + eps))).
    For an ordinary group the second terms are 1e-6 of the first; for the group with mean 1000 and spread 1e-2 the cancellation
    factor is 1.5e10 and a_rstd is what the float64 sums can deliver, no more.  k = gn_chain(...)."""
    B, H, W, C = x.shape
    xg = gn_groups(x, G)
    n = xg.shape[1] * xg.shape[3]
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3)) / ((n - 1) if unbiased else n)
    rstd = 1.0 / torch.sqrt(var + eps)
    k = gn_chain(B, H * W, C, G) * U64_OVER_U32
    mabs, msq = xg.abs().mean((1, 3)), (xg * xg).mean((1, 3))
    return _ns(mean=mean, var=var, rstd=rstd, a_mean=mean.abs() + k * mabs,
               a_rstd=rstd * (1.0 + k * (msq + 2.0 * mean.abs() * mabs) / (2.0 * (var + eps))), n=n)


def gn_stats_one_pass(x, G, eps=EPS):
    """the kernels' formula by torch on the CPU (the yardstick, never a reference): float64 sums, var = s2 / n - mean^2 clamped at 0,
    results rounded to fp32 -> (mean, rstd) fp32 [B, G], and the float64 sums [B, G, 2]"""
    xg = gn_groups(x, G)
    n = xg.shape[1] * xg.shape[3]
    s1, s2 = xg.sum((1, 3)), (xg * xg).sum((1, 3))
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float(), torch.stack((s1, s2), -1)


def gn_apply_restated(x, gamma, beta, G, st, swish, wrong_cpg=False):
    """float64: v = (x - mu) rstd gamma + beta with mu = fp32(mean) -- a contractual rounding: (mean, rstd) are fp32 values handed to
    the consumer, and where the mean dwarfs the spread the rounding of mu IS the result -- and rstd unrounded.
    a = |x - mu| a_rstd |gamma| + |beta|: the issue's magnitude with rstd's own a in rstd's place (what rstd is uncertain by, y is).
    swish: v sigmoid(v), and a times the swish factor |d (v sigmoid(v)) / dv| <= sigmoid(v) (1 + |v| (1 - sigmoid(v))).
    wrong_cpg: a channel's group taken with twice the channels per group (the wrong reference)."""
    B, H, W, C = x.shape
    cpg = C // G
    idx = torch.arange(C) // (2 * cpg if wrong_cpg else cpg)
    mu = st.mean.float().double()[:, idx][:, None, None, :]
    rs, ars = st.rstd[:, idx][:, None, None, :], st.a_rstd[:, idx][:, None, None, :]
    d = x.double() - mu
    v = d * rs * gamma.double() + beta.double()
    a = d.abs() * ars * gamma.double().abs() + beta.double().abs()
    if swish:
        sig = torch.sigmoid(v)
        v, a = v * sig, a * sig * (1.0 + v.abs() * (1.0 - sig))
    return v, a


def gn_apply_fp32(x, gamma, beta, G, mean32, rstd32, swish):
    """the kernel's expression in fp32 by torch on the CPU (the yardstick)"""
    cpg = x.shape[3] // G
    idx = torch.arange(x.shape[3]) // cpg
    o = (x - mean32[:, idx][:, None, None, :]) * rstd32[:, idx][:, None, None, :] * gamma + beta
    return o / (1.0 + torch.exp(-o)) if swish else o


def gn_mean_is_clear_of_ties(st, k_rel=1e-12):
    """the condition the fp32(mean) rounding point rests on: no group's mean lies within 1e-12 (relative) of an fp32 rounding tie, so
    a float64 sum in another order rounds to the same fp32 value.  (Up to eight elements per group the float64 sum of fp32 values
    of like magnitude is exact in any order and a tie rounds the same way every time: nothing to check.)"""
    if st.n <= 8:
        return True
    m = st.mean
    lo = m.float().double()
    other = torch.nextafter(m.float(), torch.where(m > lo, torch.tensor(float("inf")), torch.tensor(float("-inf")))).double()
    tie = (lo + other) / 2
    return bool(((m == lo) | ((m - tie).abs() > k_rel * m.abs())).all())


# ================================================================================================ row softmax
# (rows, cols, ld)
SOFTMAX_CASES = [(1, 1, 1), (5, 3, 4), (5, 3, 3), (7, 63, 63), (7, 64, 64), (9, 65, 68), (3, 729, 732), (2, 4097, 4097)]
SOFTMAX_SCALES = [0.125, 1.0]
SOFTMAX_EXTREME = (7, 64, 64)                                       # scores of +-300 at scale 1


def softmax_input(case, extreme=False):
    rows, cols, ld = case
    g = _gen(rows * 10007 + cols * 3 + ld)
    if extreme:
        x = (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1).float() * 300.0
        x[:, 0], x[:, 1] = 300.0, -300.0
        return x
    return torch.randn(rows, cols, generator=g) * 3


def softmax_restated(x, scale, scale_after=False):
    """float64 softmax of scale * x (scale a power of two or 1 here: the kernel's fp32 product is exact) -> v, a = v (1 + |z - max|):
    exp turns the absolute error of its argument, one rounding of z - max, into a relative one.
    scale_after: the wrong reference, in effect THE SCALE DROPPED -- the maximum subtracted from the unscaled scores and the scale
    applied behind it, to the exponentials, where the normalisation cancels it (a scale applied to x - max instead would be the same
    softmax: a shift)."""
    z = x.double() * scale
    if scale_after:
        e = torch.exp(x.double() - x.double().max(-1, keepdim=True).values) * scale
        return e / e.sum(-1, keepdim=True), None
    d = z - z.max(-1, keepdim=True).values
    v = torch.softmax(z, -1)
    return v, v * (1.0 + d.abs())


def softmax_fp32(x, scale):
    z = x * scale
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_excess(got, v, a):
    return fp32_excess(got, v, a, SOFTMAX_SLACK, SOFTMAX_FLOOR).max().item()
