"""Float64 restatements of the plain training row kernels (RoPE, SwiGLU backward, cross entropy), the inputs their tests use, and
the bars those tests judge by.  Plain torch on the CPU: tests/test_train_rows_ref_cpu.py checks all of it without a GPU,
tests/test_train_rows_gpu.py puts the kernels in the restatements' place.

A restatement is the operation in float64 that keeps the kernel's ROUNDING POINTS -- the places where the kernel's contract says a
value is rounded to bf16 (or, for RoPE, to fp32) -- and nothing else of the kernel: no lanes, no chunks, no fast exponentials.

How an output is judged (docs/experiments.md, "Training row kernels: exact and per-element tests"):

  exact      RoPE, the KV store, the embedding and the column sums: torch.equal.
  bf16 out   |got - v| <= 2^-8 |v| + slack * a + floor, per element.  v is the restatement's float64 value BEFORE its last rounding
             (2^-8 |v| is that rounding: half a bf16 ulp at the bottom of a binade), a is the magnitude the fp32 error of the formula
             scales with (the sum of the magnitudes of the terms that cancel in v), and slack is 4 x the worst distance, in units of
             a, of an fp32 evaluation of the same formula on the CPU (torch.sigmoid / torch.exp / torch.logsumexp) from float64, on
             these tests' own inputs, no kernel involved.
  fp32 rows  lse, logp, loss_row: |got - v| <= bar * max(1, |lse|), bar = 4 x the same kind of distance (fp32 holds lse to 2^-24 of
             its magnitude, hence the unit).

The measured distances are the constants below; test_train_rows_ref_cpu.py measures them again and requires each constant to be
4 x what it measures (within a factor of two, for another CPU's vector maths), and requires every bar to reject the listed wrong
references by 2 x while accepting the restatement.
"""
import math

import torch

from exact_products import _gen, bf16_ulp, int_prefill, round_up  # noqa: F401  (re-exported for the tests)

BF = torch.bfloat16
IGNORE = -100
HALF_ULP = 2.0 ** -8            # |bf16(v) - v| <= 2^-8 |v|

# ---- measured on the CPU, fp32 evaluation against float64, over every case below (test_bars_are_four_times_the_fp32_distance) ----
CE_ROW_DIST = 1.56e-7           # lse / logp / loss_row, in units of max(1, |lse|): worst over CE_CASES (logp at R = 300, V = 16)
CE_GRAD_DIST = 2.03e-6          # (exp(x - lse) - onehot) * sc, in units of |sc| * (p + onehot): worst at V = 159867
SWIGLU_DGATE_DIST = 6.26e-7     # dsilu * sig * (1 + g * (1 - sig)), in units of |dsilu| * sig * (1 + |g| * (1 - sig)): (1031, 4096)
SWIGLU_TIE_DIST = 1.47e-7       # g * sig before its bf16 rounding, relative: (1031, 4096)
SWIGLU_FLOOR_MAG = 4.21e-37     # largest |dgate| or |dup| on which fp32 and float64 disagree by more than 2 bf16 ulps: the planted
#                                 gates -89 and -90 only (fp32 exp(-g) overflows, sigmoid = 0; float64 keeps about 1e-39), dup of (1031, 4096)
MARGIN = 4.0                    # the device's __expf, logf and reciprocal are not torch's
CE_ROW_BAR = MARGIN * CE_ROW_DIST
CE_GRAD_SLACK = MARGIN * CE_GRAD_DIST
SWIGLU_DGATE_SLACK = MARGIN * SWIGLU_DGATE_DIST
SWIGLU_TIE_DELTA = MARGIN * SWIGLU_TIE_DIST
SWIGLU_FLOOR = MARGIN * SWIGLU_FLOOR_MAG


def r16(x):
    """round to bf16, back in the dtype it came in"""
    return x.to(torch.float32).to(BF).to(x.dtype)


def excess(got, v, a, slack, floor=0.0):
    """the bf16-output rule as a ratio per element: <= 1 passes.  got: what a kernel (or its stand-in) wrote; v, a: float64"""
    bar = HALF_ULP * v.abs() + slack * a + floor
    diff = (got.double() - v).abs()
    return torch.where(diff == 0, torch.zeros_like(diff), diff / bar.clamp_min(1e-300))


# ================================================================================================ RoPE
def rope_tables(L, head_dim, seed=None, theta=1e6):
    """cos, sin fp32 [L, head_dim / 2] as ops.rope_tables builds them (oracle.ops_ref.rope_tables_ref's first half)"""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    pos = torch.arange(L, dtype=torch.float)
    freqs = (inv_freq[None, :, None] @ pos[None, None, :]).transpose(1, 2)[0]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def rope_apply(x, cos, sin, nheads, head_dim, L=None, pos=None):
    """x bf16 [tokens, width]: rotate-half on the first nheads * head_dim columns, row t at table row t % L (or every row at `pos`),
    the other columns copied.  The arithmetic of oracle.ops_ref.rope_ref, (x * cos) + (rotate_half(x) * sin): fp32 products and sum,
    each rounded on its own, then one bf16 rounding.  The backward is this function with -sin."""
    tokens, half = x.shape[0], head_dim // 2
    rows = torch.arange(tokens) % L if pos is None else torch.full((tokens,), int(pos))
    c, s = cos[rows][:, None, :].float(), sin[rows][:, None, :].float()                  # [tokens, 1, half]
    h = x[:, : nheads * head_dim].float().reshape(tokens, nheads, head_dim)
    x1, x2 = h[..., :half], h[..., half:]
    o = torch.cat(((x1 * c) + ((-x2) * s), (x2 * c) + (x1 * s)), dim=-1)
    out = x.clone()
    out[:, : nheads * head_dim] = o.reshape(tokens, nheads * head_dim).to(BF)
    return out


def rope_transpose_by_hand(y, cos, sin, nheads, head_dim, L):
    """the transposed rotation written out: dx1 = y1 c + y2 s, dx2 = y2 c - y1 s (same roundings)"""
    tokens, half = y.shape[0], head_dim // 2
    rows = torch.arange(tokens) % L
    c, s = cos[rows][:, None, :].float(), sin[rows][:, None, :].float()
    h = y[:, : nheads * head_dim].float().reshape(tokens, nheads, head_dim)
    y1, y2 = h[..., :half], h[..., half:]
    o = torch.cat((y1 * c + y2 * s, y2 * c - y1 * s), dim=-1)
    out = y.clone()
    out[:, : nheads * head_dim] = o.reshape(tokens, nheads * head_dim).to(BF)
    return out


# (B, L, rotated heads, unrotated trailing columns, head_dim)
ROPE_CASES = [(2, 45, 4, 128, 128), (1, 1, 1, 0, 128), (5, 40, 3, 64, 64), (3, 771, 16, 256, 128)]
ROPE_SLICE_CASE = (2, 45, 3, 128, 128)       # run as a column slice that starts 4 elements into rows 24 elements wider


def rope_input(case, seed=11):
    B, L, nh, tail, hd = case
    return (torch.randn(B * L, nh * hd + tail, generator=_gen(seed + B * L + nh)) * 2).to(BF)


# ================================================================================================ SwiGLU backward
SWIGLU_SHAPES = [(77, 512), (5, 8), (1031, 4096)]
# the band where 1 + exp(-g) is finite in fp32 but its reciprocal is subnormal, the band where it overflows, and the zeros
SWIGLU_GATES = [-200.0, -90.0, -89.0, -88.5, -88.0, -87.5, -87.0, 87.0, 88.0, 90.0, 200.0, 0.0, -0.0]


def swiglu_input(tokens, i, seed=2):
    """gu bf16 [tokens, 2 i] = [gate | up], dact bf16 [tokens, i]; row 0 starts with SWIGLU_GATES (as many as fit)"""
    g = _gen(seed * 1000003 + tokens * 8191 + i)
    gu = (torch.randn(tokens, 2 * i, generator=g) * 2).to(BF)
    n = min(i, len(SWIGLU_GATES))
    gu[0, :n] = torch.tensor(SWIGLU_GATES[:n]).to(BF)
    dact = torch.randn(tokens, i, generator=g).to(BF)
    return gu, dact


class SwigluBwd:
    """dgate, dup: float64 before the last rounding; dgate_a: the magnitude dgate's fp32 error scales with; dup_alt: dup with the
    saved silu output rounded the other way where g * sig lies within `tie_delta` (relative) of a bf16 rounding tie -- there an
    evaluation that knows g * sig only to fp32 accuracy may round it to either neighbour, and both are the contract's value"""

    def dgu(self):
        return torch.cat((r16(self.dgate), r16(self.dup)), dim=1).to(BF)


def swiglu_bwd_restated(gu, dact, tie_delta=SWIGLU_TIE_DELTA):
    """The autograd of the two bf16 ops of Qwen2MLP.forward, s = silu(g) and act = s * u, as swiglu_bwd_elem (csrc/common.h) states
    it: sig in float64; s = bf16(g * sig) (the saved silu output); dsilu = bf16(d * u); dup = bf16(d * s);
    dgate = bf16(dsilu * sig * (1 + g * (1 - sig)))."""
    i = gu.shape[1] // 2
    g, u, d = gu[:, :i].double(), gu[:, i:].double(), dact.double()
    sig = 1.0 / (1.0 + torch.exp(-g))
    t = g * sig
    s = r16(t)
    dsilu = r16(d * u)
    out = SwigluBwd()
    out.sig, out.s, out.dsilu = sig, s, dsilu
    out.dgate = dsilu * (sig * (1.0 + g * (1.0 - sig)))
    out.dgate_a = dsilu.abs() * (sig * (1.0 + g.abs() * (1.0 - sig)))
    out.dup = d * s
    # the neighbour of s on the other side of t (bf16 is sign-magnitude: the bit pattern +- 1 steps the magnitude)
    bits = s.to(BF).view(torch.int16)
    step = torch.where(s.abs() > t.abs(), -torch.ones_like(bits), torch.ones_like(bits))
    alt = (bits + step).view(BF).double()
    near = (s != 0) & torch.isfinite(alt) & (((t - alt).abs() - (t - s).abs()) <= 2.0 * tie_delta * t.abs())
    out.near_tie = near
    out.dup_alt = torch.where(near, d * alt, out.dup)
    return out


def swiglu_bwd_fp32(gu, dact):
    """the same formula evaluated in fp32 by torch on the CPU (the yardstick of the slack, never a reference): -> (g * sig, dgate, dup)"""
    i = gu.shape[1] // 2
    g, u, d = gu[:, :i].float(), gu[:, i:].float(), dact.float()
    sig = torch.sigmoid(g)
    t = g * sig
    s = r16(t)
    dsilu = r16(d * u)
    return t, dsilu * (sig * (1.0 + g * (1.0 - sig))), d * s


def swiglu_excess(got_dgu, ref):
    """-> (worst ratio of dgate, worst ratio of dup); <= 1 passes"""
    i = got_dgu.shape[1] // 2
    eg = excess(got_dgu[:, :i], ref.dgate, ref.dgate_a, SWIGLU_DGATE_SLACK, SWIGLU_FLOOR)
    eu = torch.minimum(excess(got_dgu[:, i:], ref.dup, ref.dup.abs(), 0.0, SWIGLU_FLOOR),
                       excess(got_dgu[:, i:], ref.dup_alt, ref.dup_alt.abs(), 0.0, SWIGLU_FLOOR))
    return eg.max().item(), eu.max().item()


# ================================================================================================ cross entropy
# (rows or None for "the planted rows + 3", V, leading dimension: round_up(V, 64), V itself where V % 8 == 0, 8 for V = 5)
CE_CASES = [(None, 5, 8), (None, 8, 64), (None, 8, 8), (None, 24, 64), (None, 24, 24), (None, 2048, 2048), (None, 2051, 2112),
            (None, 4101, 4160), (None, 159867, 159872), (300, 16, 16), (1, 2051, 2112)]
CE_DOMINANT = 40.0              # randn * 3 stays below 17 at these sizes: dominant by more than 20


def ce_planted_columns(V):
    """one column per region a kernel can skip: column 3, the last full 8-wide chunk, each column of the ragged tail (V % 8), the
    chunk lane 0 reads in its last iteration (lanes take chunks lane, lane + 256, ...)"""
    nv = V // 8
    cols = [3] if V > 3 else []
    if nv:
        cols.append((nv - 1) * 8 + 5)
    cols += list(range(nv * 8, V))
    if nv:
        cols.append(((nv - 1) // 256) * 256 * 8 + 2)
    return list(dict.fromkeys(cols))


def ce_input(R, V, seed=6):
    """logits bf16 [R, V] (row r < len(planted) carries CE_DOMINANT at planted column r), labels int64 [R]: column 0, V - 1, the first
    tail column, ignore_index, the row's own dominant column, then random with every 7th ignored"""
    cols = ce_planted_columns(V)
    R = len(cols) + 3 if R is None else R
    g = _gen(seed * 7919 + V * 31 + R)
    logits = (torch.randn(R, V, generator=g) * 3).to(BF)
    for r, c in enumerate(cols[:R]):
        logits[r, c] = CE_DOMINANT
    labels = torch.randint(0, V, (R,), generator=g)
    special = [0, V - 1, (V // 8) * 8 if V % 8 else V - 2, IGNORE, cols[4 % len(cols)] if R > 4 and 4 < len(cols) else 1 % V]
    if R == 1:
        special = [V - 1]
    for r, lab in enumerate(special[:R]):
        labels[r] = lab
    labels[5::7] = IGNORE
    return logits, labels


class Ce:
    pass


def ce_restated(logits, labels, ignore_index=IGNORE, gscale=None, row_scale=None, lse=None):
    """float64 cross entropy of bf16 logits [R, V] by row: lse, loss_row, logp, loss (mean over the valid rows, NaN with none),
    count, and the gradient (exp(x - lse) - onehot) * sc with sc = gscale / count, or row_scale[r].  A label that is neither
    ignore_index nor inside [0, V) makes an ignored row: loss_row = logp = 0, not counted, zero gradient.
    grad_a: |sc| * (p + onehot), the magnitude the gradient's fp32 error scales with.  `lse` replaces the row statistics in the
    gradient (the wrong references of the bars-must-bite test)."""
    x = logits.double()
    R, V = x.shape
    out = Ce()
    out.lse = torch.logsumexp(x, -1)
    out.valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    lab = torch.where(out.valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, lab[:, None])[:, 0]
    zero = torch.zeros((), dtype=torch.float64)
    out.logp = torch.where(out.valid, xl - out.lse, zero)
    out.loss_row = torch.where(out.valid, out.lse - xl, zero)
    out.count = int(out.valid.sum())
    out.loss = out.loss_row.sum() / out.count if out.count else torch.tensor(float("nan"), dtype=torch.float64)
    if row_scale is not None:
        sc = row_scale.double()
    else:
        sc = torch.full((R,), (1.0 if gscale is None else float(gscale)) / max(out.count, 1), dtype=torch.float64)
    sc = torch.where(out.valid, sc, zero)
    p = torch.exp(x - (out.lse if lse is None else lse.double())[:, None])
    onehot = torch.zeros_like(x)
    onehot[out.valid, lab[out.valid]] = 1.0
    out.p, out.onehot, out.sc = p, onehot, sc
    out.grad = torch.where(out.valid[:, None], (p - onehot) * sc[:, None], zero)
    out.grad_a = torch.where(out.valid[:, None], (p + onehot) * sc.abs()[:, None], zero)
    return out


def ce_fp32(logits, labels, ignore_index=IGNORE, gscale=None, row_scale=None, lse=None):
    """the same formulas in fp32 by torch on the CPU (the yardstick of the bars, never a reference): -> lse, logp, grad (the
    gradient from the fp32 `lse` handed in, as ug_ce_bwd takes it, or from this function's own)"""
    x = logits.float()
    R, V = x.shape
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    lse_own = torch.logsumexp(x, -1)
    logp = torch.where(valid, x.gather(1, lab[:, None])[:, 0] - lse_own, torch.zeros(()))
    if row_scale is not None:
        sc = row_scale.float()
    else:
        sc = torch.full((R,), 1.0 if gscale is None else float(gscale)) / torch.tensor(float(max(int(valid.sum()), 1)))
    onehot = torch.zeros_like(x)
    onehot[valid, lab[valid]] = 1.0
    lse_in = lse_own if lse is None else lse.float()
    grad = torch.where(valid[:, None], (torch.exp(x - lse_in[:, None]) - onehot) * sc[:, None], torch.zeros(()))
    return lse_own, logp, grad


def ce_row_excess(got, want, lse):
    """lse / logp / loss_row rule as a ratio per row: <= 1 passes"""
    return ((got.double() - want).abs() / (CE_ROW_BAR * lse.abs().clamp_min(1.0))).max().item()


def ce_mean_bar(ref, R):
    """|mean - float64 mean|: the rows' own bar (a mean of errors is no larger than the largest), plus the fp32 sum of R positive
    terms in ce_reduce_kernel's order -- ceil(R / 256) terms per lane in sequence, an 8-level tree over the 256 lanes, one
    division: at most ceil(R / 256) + 9 roundings, each below 2^-24 of the running sum, which never exceeds the total"""
    rows = CE_ROW_BAR * ref.lse[ref.valid].abs().clamp_min(1.0).max().item()
    return rows + (math.ceil(R / 256) + 9) * 2.0 ** -24 * abs(ref.loss.item())


def ce_grad_excess(got, ref):
    return excess(got, ref.grad, ref.grad_a, CE_GRAD_SLACK).max().item()


# ================================================================================================ integer-valued inputs (atomics kernels)
def int_bf16(rows, cols, seed, span=4):
    """bf16 [rows, cols], integers in [-span, span]: any fp32 sum of up to 2^24 / span of them is exact in any order"""
    return torch.randint(-span, span + 1, (rows, cols), generator=_gen(seed)).to(BF)


def int_f32(rows, cols, seed, span=8):
    return torch.randint(-span, span + 1, (rows, cols), generator=_gen(seed)).float()


def distinct_ints(n, seed):
    """fp32 [n]: n different integers in [-n, n) (an accumulator's contents: a column written to the wrong place shows)"""
    return (torch.randperm(2 * n, generator=_gen(seed))[:n] - n).float()


def embed_ids(tokens, V, seed, bad=False):
    """int64 [tokens]: random ids with a long run of one value (every 3rd is 7), ids 0 and V - 1; with bad: -1 and V as well"""
    ids = torch.randint(0, V, (tokens,), generator=_gen(seed))
    ids[::3] = 7
    ids[1], ids[2] = 0, V - 1
    if bad:
        ids[4], ids[tokens - 2] = -1, V
    return ids
