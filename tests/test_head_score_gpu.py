"""ug_head_score (csrc/head_score.hip) through ops.head_score and the C ABI: the head product and its softmax statistics without
a logit matrix.

Exact part: operands from exact_products.small_sum make every logit an integer within +-256, where bf16 rounding is the identity
and ties are plentiful: `best`, `best_logit` and the label's logit have to equal the integer matmul's, whatever the tile, the wave
or the lane a table entry falls into.  lse is held against fp64 with the bar the existing ug_ce_fwd earns on the same logits.
Random part: against tests/head_score_ref.py with the bar the existing gemm_nt + ce_fwd pair earns on the same inputs.

Bars (set before any run; ROW_SPREAD = 1.5 is the spread the project grants between two evaluations of one quantity):
  lse   max(1.5 x max |ug_ce_fwd's lse - fp64| over the case, 2^-22 max(1, |lse|))
  logp  max(1.5 x max |gemm_nt + ce_fwd's logp - oracle| over the case, 2^-22 max(1, |logp|)); a row is exempt only if its label's
        or maximum's logit is exactly one bf16 step from the oracle's AND the fp64 sum lies within 2^-20 sum |x_k W_ek| of that
        rounding midpoint AND the row stays within 2^-7 (|label logit| + |best logit|); at most 1 % of a case's rows.
"""
import functools

import pytest
import torch

import exact_products as ep
from head_score_ref import bf16_steps, head_score_ref

pytestmark = pytest.mark.gpu

ROW_SPREAD = 1.5
FLOOR = 2.0 ** -22
EXEMPT_SHARE = 0.01
PAD_VALUE = 1.0e4            # what the rows behind V and behind R hold: a logit of 1e4 * anything would own every statistic
RS = [1, 17, 64, 65, 130]
VS = [1, 255, 256, 257, 1000, 4099]
KS = [256, 1536]
FULL = (3, 159867, 1536)
RANDOM_CASES = [(64, 4099, 256, 0.0625), (16, 4099, 1536, 0.05), (8, 159867, 1536, 0.02)]


# ------------------------------------------------------------------------------------------------ operands, built once, read-only
def _small_rows(rows, K, seed, density=None, piece=16384):
    return torch.cat([ep.small_sum(min(piece, rows - r0), K, seed + 17 * i, density) for i, r0 in enumerate(range(0, rows, piece))])


@functools.lru_cache(maxsize=None)
def operands(K, regime, Rmax=max(RS), Vmax=max(VS)):
    """(x [Rmax, K], W [Vmax, K], logits fp32 [Rmax, Vmax] exact, labels [Rmax]); every case is a leading slice.  "low": density
    1.5 / sqrt(K) on both sides, about 2 non-zero products per logit: logits within about +-6, every column tile carries softmax mass."""
    d = None if regime == "small" else 1.5 / K ** 0.5
    seed = 9000 + K + (0 if regime == "small" else 1)
    x, W = _small_rows(Rmax, K, seed, d), _small_rows(Vmax, K, seed + 1, d)
    ref = ep.exact_ref(x, W, small=True)
    if regime == "low":
        assert ref.abs().max().item() <= 16 and ref.std().item() > 1.0
    labels = torch.randint(0, 2 ** 31, (Rmax,), generator=torch.Generator().manual_seed(seed + 2))
    return x, W, ref, labels


def padded(t, extra, dev):
    """t [n, K] on the device in a buffer with `extra` rows of PAD_VALUE behind it -> (the buffer, its first n rows)"""
    buf = torch.full((t.shape[0] + extra, t.shape[1]), PAD_VALUE, dtype=torch.bfloat16)
    buf[:t.shape[0]] = t
    buf = buf.to(dev)
    return buf, buf[:t.shape[0]]


def stats64(logits):
    """fp64 lse, first argmax and maximum of an exact logit matrix"""
    l = logits.double()
    m = l.max(dim=1).values
    return m + torch.log(torch.exp(l - m[:, None]).sum(dim=1)), (l == m[:, None]).to(torch.int8).argmax(dim=1), m


def ce_lse(logits, dev):
    """the existing ug_ce_fwd's lse of exact bf16 logits [R, V] (ld padded to a multiple of 8)"""
    from unigen_hip import ops
    R, V = logits.shape
    buf = torch.zeros((R, ep.round_up(V, 8)), dtype=torch.bfloat16)
    buf[:, :V] = logits.to(torch.bfloat16)
    _, lse, _, _ = ops.ce_fwd(buf.to(dev), V, torch.zeros((R,), dtype=torch.int64, device=dev))
    return lse.cpu().double()


def raw_call(xv, Wbuf, V, labels, n_out, ignore_index=-100):
    """ug_head_score into NaN-filled outputs of n_out >= R elements -> (logp, lse, best (-7 where unwritten), best_logit) on the CPU"""
    from unigen_hip import lib, ops
    R, K = xv.shape
    dev = xv.device
    ws = ops._head_score_workspace(ops.head_score_ws_bytes(R, V), dev)
    f = [torch.full((n_out,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    best = torch.full((n_out,), -7, dtype=torch.int64, device=dev)
    lib.check(lib.load().ug_head_score(xv.data_ptr(), xv.stride(0), R, Wbuf.data_ptr(), Wbuf.stride(0), V, K, labels.data_ptr(), ignore_index,
                                       ws.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), best.data_ptr(), f[2].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "ug_head_score")
    return f[0].cpu(), f[1].cpu(), best.cpu(), f[2].cpu()


def check_exact(dev, x, W, ref, labels, what):
    """one exact case: x [R, K], W [V, K], ref [R, V] integers, labels [R] in [0, V)"""
    R, V = ref.shape
    xbuf, xv = padded(x, 3, dev)
    Wbuf, _ = padded(W, 64, dev)
    logp, lse, best, best_logit = raw_call(xv, Wbuf, V, labels.to(dev), R + 3)
    for name, t in (("logp", logp), ("lse", lse), ("best_logit", best_logit)):
        assert not t[:R].isnan().any(), f"{what}: {name} has unwritten rows"
        assert t[R:].isnan().all(), f"{what}: {name} written past R"
    assert (best[R:] == -7).all() and (best[:R] >= 0).all(), f"{what}: best rows"
    lse64, arg64, max64 = stats64(ref)
    assert torch.equal(best[:R], arg64), f"{what}: best: {ep.mismatch_report(best[:R, None].float(), arg64[:, None].float())}"
    assert torch.equal(best_logit[:R].double(), max64), f"{what}: best_logit"
    lab = logp[:R].double() + lse[:R].double()                # = label logit + the fp32 rounding of the subtraction (< 2^-24 * 512)
    want = ref[torch.arange(R), labels].double()
    assert (lab - lab.round()).abs().max().item() < 1e-3 and torch.equal(lab.round(), want), f"{what}: label logit"
    err = (lse[:R].double() - lse64).abs()
    e_ce = (ce_lse(ref, dev) - lse64).abs().max().item()
    bar = torch.clamp(FLOOR * torch.clamp(lse64.abs(), min=1.0), min=ROW_SPREAD * e_ce)
    print(f"{what}: lse err max {err.max().item():.3e}, ug_ce_fwd {e_ce:.3e}, floor {FLOOR * max(1.0, lse64.abs().max().item()):.3e}")
    assert (err <= bar).all(), f"{what}: lse off by {err.max().item():.3e} (ug_ce_fwd: {e_ce:.3e})"


# ------------------------------------------------------------------------------------------------ exact, structural
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("regime", ["small", "low"])
def test_exact_integer_logits_every_shape(dev, regime, V, K):
    x, W, ref, labels = operands(K, regime)
    for R in RS:
        check_exact(dev, x[:R], W[:V], ref[:R, :V], labels[:R] % V, f"{regime} R={R} V={V} K={K}")


def test_exact_full_width(dev):
    R, V, K = FULL
    x, W, ref, labels = operands(K, "small", R, V)
    check_exact(dev, x, W, ref, labels % V, f"full width R={R} V={V} K={K}")


# ------------------------------------------------------------------------------------------------ random operands
@pytest.mark.parametrize("R,V,K,sw", RANDOM_CASES)
def test_random_operands_against_fp64(dev, R, V, K, sw):
    from unigen_hip import ops
    g = torch.Generator().manual_seed(R + V + K)
    x = torch.randn((R, K), generator=g).to(torch.bfloat16)
    W = (torch.randn((V, K), generator=g) * sw).to(torch.bfloat16)
    labels = torch.randint(0, V, (R,), generator=g)
    o = head_score_ref(x, W, labels)
    xd, Wd, ld = x.to(dev), W.to(dev), labels.to(dev)
    logp, lse, best, best_logit = (t.cpu() for t in ops.head_score(xd, Wd, V, ld, want=("lse", "best", "best_logit")))
    # the existing pair on the same inputs: logits_rows-style gemm_nt into a padded bf16 matrix, then ce_fwd(want_logp)
    Vp = ep.round_up(V, 8)
    logits = torch.zeros((R, Vp), dtype=torch.bfloat16, device=dev)
    ops.gemm_nt(xd, Wd, out=logits, M=R, N=V, K=K)
    pair = ops.ce_fwd(logits, V, ld, want_logp=True)[3].cpu().double()
    e_pair = (pair - o.logp).abs().max().item()
    err = (logp.double() - o.logp).abs()
    bar = torch.clamp(FLOOR * torch.clamp(o.logp.abs(), min=1.0), min=ROW_SPREAD * e_pair)
    over = err > bar
    got_label = logp.double() + lse.double()
    step_l, step_b = bf16_steps(got_label.float(), o.label_logit), bf16_steps(best_logit, o.best_logit)
    mid_l = ((o.label_raw - (bf16_near(got_label) + o.label_logit) / 2).abs() <= 2.0 ** -20 * o.label_abs) & (step_l == 1)
    mid_b = ((o.best_raw - (best_logit.double() + o.best_logit) / 2).abs() <= 2.0 ** -20 * o.best_abs) & (step_b == 1)
    near = err <= 2.0 ** -7 * (o.label_logit.abs() + o.best_logit.abs())
    exempt = over & (mid_l | mid_b) & near
    print(f"R={R} V={V} K={K}: logp err max {err.max().item():.3e}, pair {e_pair:.3e}, over {int(over.sum())}, exempt {int(exempt.sum())}, "
          f"best differs {int((best != o.best).sum())}")
    assert not (over & ~exempt).any(), f"logp off by {err[over & ~exempt].max().item():.3e} (gemm_nt + ce_fwd: {e_pair:.3e})"
    assert int(exempt.sum()) <= EXEMPT_SHARE * R, f"{int(exempt.sum())} of {R} rows exempt"
    # the fp32 accumulation is thousands of times finer than a bf16 step: the maximum moves only across a rounding midpoint
    assert ((step_b == 0) | mid_b).all(), "best_logit differs from the oracle's off a rounding midpoint"


def bf16_near(t):
    """fp64 values that are bf16 values up to an fp32 rounding -> those bf16 values, fp64"""
    return t.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ ignored labels
def test_ignored_and_out_of_range_labels(dev):
    from unigen_hip import ops
    R, V, K = 65, 1000, 256
    x, W, ref, labels = operands(K, "low")
    xd, Wd = x[:R].to(dev), W[:V].to(dev)
    real = (labels[:R] % V)
    odd = real.clone()
    odd[0::4], odd[1::4], odd[2::4] = -100, V, -1            # ignore_index, one past the end, negative; every fourth row keeps its label
    a = [t.cpu() for t in ops.head_score(xd, Wd, V, real.to(dev), want=("lse", "best", "best_logit"))]
    b = [t.cpu() for t in ops.head_score(xd, Wd, V, odd.to(dev), want=("lse", "best", "best_logit"))]
    kept = torch.arange(R) % 4 == 3
    assert torch.equal(b[0][~kept], torch.zeros(int((~kept).sum()))) and torch.equal(b[0][kept], a[0][kept])
    assert not torch.signbit(b[0][~kept]).any()
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)
    c = ops.head_score(xd, Wd, V, real.to(dev), ignore_index=int(real[5]), want=())
    assert len(c) == 1 and (c[0].cpu()[real == real[5]] == 0).all() and torch.equal(c[0].cpu()[real != real[5]], a[0][real != real[5]])


# ------------------------------------------------------------------------------------------------ row independence, reproducibility
@pytest.mark.parametrize("V,K", [(4099, 1536), (257, 256)])
def test_a_rows_bits_do_not_depend_on_the_batch(dev, V, K):
    """random operands (every bit of the fp32 accumulation is live): the 130-row call against the same rows sent 1, 17 and 64 at a
    time -- both row-tile heights of head_score_plan.h, one and several row tiles -- and against itself"""
    from unigen_hip import ops
    g = torch.Generator().manual_seed(V + K)
    x = torch.randn((130, K), generator=g).to(torch.bfloat16).to(dev)
    W = (torch.randn((V, K), generator=g) * 0.05).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, V, (130,), generator=g).to(dev)
    want = ("lse", "best", "best_logit")
    full = [t.cpu() for t in ops.head_score(x, W, V, labels, want=want)]
    again = [t.cpu() for t in ops.head_score(x, W, V, labels, want=want)]
    for u, v in zip(full, again):
        assert torch.equal(u, v)
    for n in (1, 17, 64):
        parts = [[t.cpu() for t in ops.head_score(x[r0:r0 + n], W, V, labels[r0:r0 + n], want=want)] for r0 in range(0, 130, n)]
        for i, u in enumerate(full):
            assert torch.equal(u, torch.cat([p[i] for p in parts])), (n, want[i - 1] if i else "logp")
    # other rows' CONTENT: the first 17 rows beside 113 different neighbours
    x2 = x.clone()
    x2[17:] = x2[17:] * 3 + 1
    moved = [t.cpu() for t in ops.head_score(x2, W, V, labels, want=want)]
    for u, v in zip(full, moved):
        assert torch.equal(u[:17], v[:17])
