"""tests/train_rows_ref.py without a GPU: the restatements agree with float64 autograd of the plain formulas up to their stated
rounding points, the RoPE backward restatement is the hand-written transpose bit for bit, the constants behind the bars are 4 x what
an fp32 evaluation on this CPU measures, and the bars BITE: with the restatement standing in for the kernel, every bar of
tests/test_train_rows_gpu.py rejects each listed subtly wrong reference by at least 2 x on at least one case and accepts the
restatement (docs/experiments.md, "Training row kernels: exact and per-element tests", has the table)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import train_rows_ref as tr
from oracle.ops_ref import rope_ref, rope_tables_ref

BF = torch.bfloat16
U = 2.0 ** -8                 # one bf16 rounding, relative


@functools.lru_cache(maxsize=None)
def _ce(R, V):
    logits, labels = tr.ce_input(R, V)
    return logits, labels, tr.ce_restated(logits, labels)


@functools.lru_cache(maxsize=None)
def _swiglu(tokens, i):
    gu, dact = tr.swiglu_input(tokens, i)
    return gu, dact, tr.swiglu_bwd_restated(gu, dact)


# ================================================================================================ restatements against autograd
@pytest.mark.parametrize("case", tr.ROPE_CASES + [tr.ROPE_SLICE_CASE])
def test_rope_restatement_is_rope_ref_and_its_backward_is_the_transpose(case):
    B, L, nh, tail, hd = case
    x = tr.rope_input(case)
    cos, sin = tr.rope_tables(L, hd)
    cr, sr = rope_tables_ref(L, hd, 1e6)
    assert torch.equal(cos, cr[:, : hd // 2]) and torch.equal(sin, sr[:, : hd // 2])
    fwd = tr.rope_apply(x, cos, sin, nh, hd, L=L)
    heads = x[:, : nh * hd].view(B, L, nh, hd).permute(0, 2, 1, 3)                          # [B, heads, L, d] as rope_ref takes it
    assert torch.equal(fwd[:, : nh * hd].view(B, L, nh, hd).permute(0, 2, 1, 3), rope_ref(heads, cr, sr).to(BF))
    assert torch.equal(fwd[:, nh * hd:], x[:, nh * hd:])
    # backward = the same function with -sin = the transposed rotation written out, bit for bit
    y = tr.rope_input(case, seed=12)
    bwd = tr.rope_apply(y, cos, -sin, nh, hd, L=L)
    assert torch.equal(bwd.view(torch.int16), tr.rope_transpose_by_hand(y, cos, sin, nh, hd, L).view(torch.int16))
    # ... and float64 autograd of rope_ref, up to the fp32 roundings of two products and a sum and one bf16 rounding
    xd = heads.double().clone().requires_grad_(True)
    rope_ref(xd, cr.double(), sr.double()).backward(y[:, : nh * hd].view(B, L, nh, hd).permute(0, 2, 1, 3).double())
    got = bwd[:, : nh * hd].view(B, L, nh, hd).permute(0, 2, 1, 3).double()
    mag = y[:, : nh * hd].double().abs().view(B, L, nh, hd).permute(0, 2, 1, 3)
    half = hd // 2
    terms = mag + torch.cat((mag[..., half:], mag[..., :half]), -1)                          # |y1 c| + |y2 s| <= |y1| + |y2|
    assert ((got - xd.grad).abs() <= U * xd.grad.abs() + 3 * 2.0 ** -24 * terms).all()
    # a single position for every row (ug_rope_at)
    at = tr.rope_apply(x[:7], cos, sin, nh, hd, pos=L - 1)
    assert torch.equal(at[0], tr.rope_apply(x[:1].repeat(L, 1), cos, sin, nh, hd, L=L)[L - 1])


@pytest.mark.parametrize("tokens,i", tr.SWIGLU_SHAPES)
def test_swiglu_restatement_is_autograd_of_the_two_bf16_ops(tokens, i):
    gu, dact, ref = _swiglu(tokens, i)
    g = gu[:, :i].double().clone().requires_grad_(True)
    u = gu[:, i:].double().clone().requires_grad_(True)
    (F.silu(g) * u).backward(dact.double())
    # dup = bf16(d * bf16(silu)): two roundings of a product; dgate = bf16(bf16(d u) * silu'): likewise (silu' itself is float64)
    two = 2 * U + U * U
    assert ((tr.r16(ref.dup) - u.grad).abs() <= two * u.grad.abs() + 1e-40).all()
    assert ((tr.r16(ref.dgate) - g.grad).abs() <= two * g.grad.abs() + 1e-40).all()
    assert torch.equal(ref.dgu()[:, :i].double(), tr.r16(ref.dgate)) and ref.dgu().shape == gu.shape
    # the other admissible rounding of the saved silu output is its neighbour, and only near a tie
    assert (ref.dup_alt[~ref.near_tie] == ref.dup[~ref.near_tie]).all()
    assert 0 < int(ref.near_tie.sum()) < 2e-3 * ref.near_tie.numel() or tokens * i < 1000


@pytest.mark.parametrize("R,V,ld", tr.CE_CASES)
def test_ce_restatement_is_autograd_of_cross_entropy(R, V, ld):
    logits, labels, ref = _ce(R, V)
    R = logits.shape[0]
    rs = torch.randn(R, generator=tr._gen(V + R))
    x = logits.double().clone().requires_grad_(True)
    loss = F.cross_entropy(x, labels, ignore_index=tr.IGNORE)
    (0.5 * loss).backward()
    half = tr.ce_restated(logits, labels, gscale=0.5)
    assert abs(ref.loss.item() - loss.item()) <= 1e-12 * abs(loss.item())
    assert ref.count == int((labels != tr.IGNORE).sum())
    assert (half.grad - x.grad).abs().max().item() <= 1e-12      # two float64 sums of V terms: far below every bar, far above 2^-53
    lsm = torch.log_softmax(logits.double(), -1)
    lab = labels.clamp(min=0)
    assert (ref.logp - lsm.gather(1, lab[:, None])[:, 0])[ref.valid].abs().max().item() <= 1e-12
    assert (ref.logp[~ref.valid] == 0).all() and (ref.loss_row[~ref.valid] == 0).all() and (half.grad[~ref.valid] == 0).all()
    x = logits.double().clone().requires_grad_(True)                                         # row_scale: d(sum_r rs[r] * -logp[r])
    (-(torch.log_softmax(x, -1).gather(1, lab[:, None])[:, 0] * rs.double())[ref.valid]).sum().backward()
    assert (tr.ce_restated(logits, labels, row_scale=rs).grad - x.grad).abs().max().item() <= 1e-12
    # planted rows: the dominant logit decides lse
    cols = tr.ce_planted_columns(V)
    for r, c in enumerate(cols[:R]):
        assert logits[r, c].item() == tr.CE_DOMINANT and logits[r].float().sort().values[-2].item() <= tr.CE_DOMINANT - 20


def test_ce_restatement_label_rule():
    """a label outside [0, V) is an ignored row, as ug_head_score has it: F.cross_entropy with such labels mapped to ignore_index"""
    logits, labels, _ = _ce(None, 2051)
    labels = labels.clone()
    V = logits.shape[1]
    labels[2], labels[5], labels[6], labels[7] = V, -1, V + 1000, 1 << 40
    ref = tr.ce_restated(logits, labels, gscale=0.5)
    mapped = torch.where((labels >= 0) & (labels < V), labels, torch.full_like(labels, tr.IGNORE))
    x = logits.double().clone().requires_grad_(True)
    loss = F.cross_entropy(x, mapped, ignore_index=tr.IGNORE)
    (0.5 * loss).backward()
    assert ref.count == int((mapped != tr.IGNORE).sum()) == logits.shape[0] - 5
    assert abs(ref.loss.item() - loss.item()) <= 1e-12 * loss.item() and (ref.grad - x.grad).abs().max().item() <= 1e-12
    none = tr.ce_restated(logits, torch.full_like(labels, tr.IGNORE))
    assert none.count == 0 and torch.isnan(none.loss) and (none.grad == 0).all()


def test_integer_inputs_are_exact_in_fp32():
    """the conditions of the exact tests: every partial sum an integer below 2^24"""
    assert tr.int_bf16(1000, 240, seed=1).float().abs().sum(0).max().item() + 2 * 207 < 2 ** 24
    assert (tr.int_bf16(1000, 240, seed=1).float() == tr.int_bf16(1000, 240, seed=1).float().round()).all()
    d = tr.distinct_ints(207, seed=200)
    assert d.unique().numel() == 207
    for tokens, V, H in [(97, 333, 256), (700, 333, 1536), (5, 9, 4), (97, 333, 6)]:
        ids = tr.embed_ids(tokens, V, seed=tokens + H, bad=True)
        assert int(((ids < 0) | (ids >= V)).sum()) == 2 and (ids == -1).any() and (ids == V).any()
        assert tokens * 8 + 1000 < 2 ** 24


# ================================================================================================ the bars
def _distances():
    row = grad = 0.0
    for R, V, _ in tr.CE_CASES:
        logits, labels, base = _ce(R, V)
        rs = torch.randn(logits.shape[0], generator=tr._gen(V + logits.shape[0]))
        lse32 = base.lse.float()
        scale = base.lse.abs().clamp_min(1.0)
        lse, logp, _ = tr.ce_fp32(logits, labels)
        row = max(row, ((lse.double() - base.lse).abs() / scale).max().item(), ((logp.double() - base.logp).abs() / scale).max().item())
        for kw in (dict(gscale=0.5), dict(), dict(row_scale=rs)):
            ref = tr.ce_restated(logits, labels, lse=lse32, **kw)
            _, _, g = tr.ce_fp32(logits, labels, lse=lse32, **kw)
            m = ref.grad_a > 0
            grad = max(grad, ((g.double() - ref.grad).abs()[m] / ref.grad_a[m]).max().item())
    dgate = tie = floor = 0.0
    differing = total = 0
    for tokens, i in tr.SWIGLU_SHAPES:
        gu, dact, ref = _swiglu(tokens, i)
        t32, dgate32, dup32 = tr.swiglu_bwd_fp32(gu, dact)
        t64 = gu[:, :i].double() * ref.sig
        m = ref.dgate_a > 1e-30
        dgate = max(dgate, ((dgate32.double() - ref.dgate).abs()[m] / ref.dgate_a[m]).max().item())
        m = t64.abs() > 1e-30
        tie = max(tie, ((t32.double() - t64).abs()[m] / t64.abs()[m]).max().item())
        n = min(i, len(tr.SWIGLU_GATES))
        for v32, v64 in ((dgate32, ref.dgate), (dup32, ref.dup)):
            r32, r64 = tr.r16(v32).double(), tr.r16(v64)
            big = torch.maximum(r32.abs(), r64.abs())
            bad = (r32 - r64).abs() > 2 * tr.bf16_ulp(big.float()).double()
            differing += int((r32 != r64).sum())
            total += r32.numel()
            if bad.any():
                where = bad.nonzero()
                assert ((where[:, 0] == 0) & (where[:, 1] < n)).all(), "fp32 and float64 disagree away from the planted gates"
                floor = max(floor, big[bad].max().item())
    return dict(CE_ROW_DIST=row, CE_GRAD_DIST=grad, SWIGLU_DGATE_DIST=dgate, SWIGLU_TIE_DIST=tie, SWIGLU_FLOOR_MAG=floor), differing, total


def test_bars_are_four_times_the_fp32_distance():
    """each constant of train_rows_ref.py against what an fp32 evaluation on THIS machine measures; within a factor of two, because
    another CPU's vectorised exp / sigmoid is another implementation (the constants were measured once and are not re-fitted)"""
    got, differing, total = _distances()
    print({k: f"{v:.3e}" for k, v in got.items()}, f"fp32 and float64 SwiGLU outputs differ on {differing} of {total} elements")
    for name, v in got.items():
        const = getattr(tr, name)
        assert 0.5 * v <= const <= 2.0 * v, (name, v, const)
    assert differing * 10 ** 5 < total                       # the planted extreme gates account for all of them
    assert tr.SWIGLU_FLOOR < 1e-30
    assert tr.CE_ROW_BAR == 4 * tr.CE_ROW_DIST and tr.SWIGLU_FLOOR == 4 * tr.SWIGLU_FLOOR_MAG


def _stand_in(v):
    """what a correct kernel writes: the restatement's value rounded to bf16"""
    return tr.r16(v)


def test_bars_accept_the_restatement_and_reject_subtly_wrong_references():
    """The house rule of test_edge_bars_reject_subtly_wrong_references.  Ratios are |difference| / bar: the restatement standing in
    for the kernel must stay <= 1 against the true reference on EVERY case and reach >= 2 against each wrong one on at least one."""
    worst_true = {}
    worst_wrong = {}

    def note(table, name, ratio):
        table[name] = max(table.get(name, 0.0), ratio)

    for R, V, _ in tr.CE_CASES:
        logits, labels, ref = _ce(R, V)
        R = logits.shape[0]
        nv = V // 8
        x = logits.double()
        got_lse = ref.lse.float()                                         # the stand-in kernel: float64 rounded to fp32
        note(worst_true, "lse", tr.ce_row_excess(got_lse, ref.lse, ref.lse))
        note(worst_true, "logp", tr.ce_row_excess(ref.logp.float(), ref.logp, ref.lse))
        if V % 8 and nv:
            note(worst_wrong, "lse without the ragged tail", tr.ce_row_excess(got_lse, torch.logsumexp(x[:, : nv * 8], -1), ref.lse))
        if nv:
            keep = torch.ones(V, dtype=torch.bool)
            c0 = ((nv - 1) // 256) * 256 * 8
            keep[c0:c0 + 8] = False                                       # lane 0's last chunk
            if keep.any():
                note(worst_wrong, "lse without a lane's last chunk", tr.ce_row_excess(got_lse, torch.logsumexp(x[:, keep], -1), ref.lse))
        full = tr.ce_restated(logits, labels, lse=got_lse, gscale=0.5)
        got_grad = _stand_in(full.grad)
        note(worst_true, "ce grad", tr.ce_grad_excess(got_grad, full))
        off = tr.Ce()
        off.grad_a = full.grad_a
        shifted = torch.roll(full.onehot, 1, dims=1)
        off.grad = torch.where(full.valid[:, None], (full.p - shifted) * full.sc[:, None], torch.zeros((), dtype=torch.float64))
        if V > 1:
            note(worst_wrong, "one-hot one column off", tr.ce_grad_excess(got_grad, off))
        if full.count not in (0, R):
            byr = tr.Ce()
            byr.grad, byr.grad_a = full.grad * full.count / R, full.grad_a
            note(worst_wrong, "gradient divided by R", tr.ce_grad_excess(got_grad, byr))

    for tokens, i in tr.SWIGLU_SHAPES:
        gu, dact, ref = _swiglu(tokens, i)
        got = ref.dgu()
        eg, eu = tr.swiglu_excess(got, ref)
        note(worst_true, "swiglu dgate", eg)
        note(worst_true, "swiglu dup", eu)
        wrong = tr.swiglu_bwd_restated(gu, dact)
        wrong.dgate = ref.dsilu * ref.sig                                   # no g (1 - sig) term
        note(worst_wrong, "dgate without g (1 - sig)", tr.swiglu_excess(got, wrong)[0])
        wrong = tr.swiglu_bwd_restated(gu, dact)
        c = 8 * ((i // 8) // 2)                                           # one 8-wide chunk per row holds dup where dgate belongs and back
        wrong.dgate, wrong.dup, wrong.dup_alt = ref.dgate.clone(), ref.dup.clone(), ref.dup_alt.clone()
        wrong.dgate[:, c:c + 8], wrong.dup[:, c:c + 8], wrong.dup_alt[:, c:c + 8] = ref.dup[:, c:c + 8], ref.dgate[:, c:c + 8], ref.dgate[:, c:c + 8]
        note(worst_wrong, "dgate | dup swapped on one chunk", min(tr.swiglu_excess(got, wrong)))

    print("restatement against the true reference (<= 1):", {k: round(v, 3) for k, v in worst_true.items()})
    print("restatement against the wrong references (>= 2):", {k: f"{v:.3g}" for k, v in worst_wrong.items()})
    assert all(v <= 1.0 for v in worst_true.values()), worst_true
    assert len(worst_wrong) == 6 and all(v >= 2.0 for v in worst_wrong.values()), worst_wrong
