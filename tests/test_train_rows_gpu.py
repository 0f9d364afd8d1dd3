"""The plain training row kernels that other tests lean on as their reference -- ug_rope, ug_rope_at, ug_kv_store, ug_swiglu_fwd / _bwd,
ug_ce_fwd / _bwd, ug_colsum_bf16, ug_embed_fwd / _bwd -- each against a float64 restatement of its own (tests/train_rows_ref.py),
through unigen_hip.ops, at the smallest shapes that reach every branch: grid caps and grid-stride loops, ragged tails, padded and
offset leading dimensions, one chunk per lane and one more, the loss reduction's loop.

What is exact is tested exactly: RoPE forward and backward (the backward is the forward with the sine negated, bit for bit), the KV
store, the embedding gather, and -- with integer-valued inputs, whose fp32 sums are exact in any order the atomics land in -- the
embedding scatter and the column sums.  SwiGLU backward and the cross-entropy gradient are judged PER ELEMENT, lse / logp / loss_row
per row, by bars that were measured on the CPU with no kernel involved (docs/experiments.md, "Training row kernels: exact and
per-element tests"; the constants and the rule are in train_rows_ref.py):

  bf16 element   |got - v| <= 2^-8 |v| + slack * a [+ floor]       v: float64 before its last rounding, a: the terms' magnitudes
      CE gradient  slack = 4 x 2.03e-6        SwiGLU dgate  slack = 4 x 6.26e-7, floor = 4 x 4.21e-37 = 1.7e-36
      SwiGLU dup   no slack: d * s is exact in fp32; where g * sig is within 4 x 1.47e-7 of a bf16 tie either rounding of s passes
  fp32 row       |got - v| <= 4 x 1.56e-7 x max(1, |lse|)

tests/test_train_rows_ref_cpu.py shows without a GPU that these bars reject an lse without the ragged tail or without a lane's last
chunk, a one-hot one column off, a gradient divided by R, a dgate without g (1 - sig) and swapped dgate | dup chunks, each by 2 x.

Outputs the caller allocates are pre-filled (NaN, or a bit pattern compared as int16) wherever "everything is written" or "nothing
else is touched" is the contract; ops.swiglu_* / ops.ce_fwd / ops.embed_fwd allocate their own outputs."""
import functools
import math

import pytest
import torch

import train_rows_ref as tr
from oracle.ops_ref import swiglu_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HD = 128


def _ops():
    from unigen_hip import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().clone()


def _pattern(n, dev, seed):
    """bf16 [n] of pseudo-random bit patterns (NaNs among them: compared as int16 only)"""
    return torch.randint(-32768, 32768, (n,), generator=tr._gen(seed), dtype=torch.int16).view(BF).to(dev)


# ================================================================================================ RoPE
def _rope_case(dev, case, sliced):
    """-> x (CPU bf16 [tokens, width]), make(): a fresh device view to run on and the buffer that contains it, tables on both sides"""
    ops = _ops()
    B, L, nh, tail, hd = case
    x = tr.rope_input(case)
    cos, sin = tr.rope_tables(L, hd)
    dcos, dsin = ops.rope_tables(L, hd, 1e6, dev)
    assert torch.equal(dcos.cpu(), cos) and torch.equal(dsin.cpu(), sin) and cos.shape == (L, hd // 2)
    wide0 = _pattern(x.shape[0] * (x.shape[1] + 24), dev, 5).view(x.shape[0], x.shape[1] + 24) if sliced else None

    def make():
        if not sliced:
            buf = x.clone().to(dev)
            return buf, buf
        wide = wide0.clone()
        view = wide[:, 4:4 + x.shape[1]]                  # 8 bytes into a row 48 bytes wider: the entry point asks for 8-byte alignment only
        view.copy_(x)
        assert view.stride(0) == x.shape[1] + 24 and view.data_ptr() % 16 == 8
        return view, wide

    def expect(want):
        if not sliced:
            return want
        wide = wide0.cpu().clone()
        wide[:, 4:4 + x.shape[1]] = want
        return wide
    return x, make, expect, (cos, sin), (dcos, dsin)


@pytest.mark.parametrize("case,sliced", [(c, False) for c in tr.ROPE_CASES] + [(tr.ROPE_SLICE_CASE, True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("slice" if v else "whole"))
def test_rope_forward_and_backward_exact(dev, case, sliced):
    """(3, 771, 16 heads): 3 * 771 * 16 * 16 = 592 128 work items, past the cap of 2048 * 256 = 524 288 -- some lanes loop twice;
    head_dim 64: two work items per table row of 32; the slice: everything outside it, and the unrotated columns, bit-unchanged"""
    ops = _ops()
    B, L, nh, tail, hd = case
    x, make, expect, (cos, sin), (dcos, dsin) = _rope_case(dev, case, sliced)
    view, buf = make()
    ops.rope_(view, dcos, dsin, L, nh, hd)
    fwd = _bits(buf)
    assert torch.equal(fwd, _bits(expect(tr.rope_apply(x, cos, sin, nh, hd, L=L)))), "forward != restatement"
    view, buf = make()
    ops.rope_(view, dcos, dsin, L, nh, hd, backward=True)
    bwd = _bits(buf)
    assert torch.equal(bwd, _bits(expect(tr.rope_apply(x, cos, -sin, nh, hd, L=L)))), "backward != restatement with -sin"
    view, buf = make()
    ops.rope_(view, dcos, (-dsin).contiguous(), L, nh, hd)
    assert torch.equal(bwd, _bits(buf)), "backward kernel != forward kernel on the negated sine table"
    if case != (1, 1, 1, 0, 128):                      # position 0 is the identity: cos = 1, sin = 0
        assert not torch.equal(fwd, bwd)


@pytest.mark.parametrize("R", [1, 5, 32])
def test_rope_at_exact_and_clamps_the_position(dev, R):
    """14 heads rotated (12 q + 2 k), a v block of 256 columns behind them, a table of 96 positions; a position at or past the table's
    length is clamped to its last row (include/unigen_hip.h)"""
    ops = _ops()
    nh, T = 14, 96
    x = (torch.randn(R, nh * HD + 256, generator=tr._gen(40 + R)) * 2).to(BF)
    cos, sin = tr.rope_tables(T, HD)
    dcos, dsin = cos.to(dev), sin.to(dev)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    for pos in (0, 1, 63, 64, 95, 96, 5000):
        pos_dev.fill_(pos)
        got = ops.rope_at_(x.clone().to(dev), dcos, dsin, nh, HD, pos_dev)
        want = tr.rope_apply(x, cos, sin, nh, HD, pos=min(pos, T - 1))
        assert torch.equal(_bits(got), _bits(want)), f"pos {pos}"
        assert torch.equal(got[:, nh * HD:].cpu(), x[:, nh * HD:])


# ================================================================================================ KV store
# (rows, L, H, HKV, Tmax, first position, position on the device?, extra columns of ldq)
KV_CASES = [(3, 1, 2, 1, 64, 17, True, 0),          # one token per row at a device position
            (2, 5, 4, 2, 64, 61, False, 0),         # positions 61 .. 65 against Tmax = 64: 64 and 65 are dropped
            (2, 3, 4, 4, 32, 0, False, 64),         # HKV = 4, ldq wider than the fused row
            (1, 2, 3, 1, 8, 8, True, 0),            # everything at or past Tmax: nothing is written
            (16, 771, 4, 4, 800, 29, False, 0)]     # 16 * 771 * 4 * 16 = 789 504 chunks, past the cap of 2048 * 256; 29 + 771 = 800: the last row fits exactly


@pytest.mark.parametrize("case", KV_CASES, ids=lambda c: "x".join(map(str, map(int, c))))
def test_kv_store_writes_exactly_the_addressed_rows(dev, case):
    ops = _ops()
    R, L, H, HKV, Tmax, pos0, on_dev, extra = case
    ldq = (H + 2 * HKV) * HD + extra
    qkv = torch.randn(R * L, ldq, generator=tr._gen(70 + R * L)).to(BF)
    n = R * HKV * Tmax * HD
    flat = [_pattern(n + 4096, dev, 90 + i) for i in range(2)]                 # the caches and 8 KB behind each
    before = [_bits(f) for f in flat]
    ck, cv = (f[:n].view(R, HKV, Tmax, HD) for f in flat)
    pos_dev = torch.tensor([pos0], dtype=torch.int32, device=dev) if on_dev else None
    ops.kv_store(qkv.to(dev), ck, cv, R, L, H, HKV, HD, Tmax, pos_dev=pos_dev, pos_host=0 if on_dev else pos0)
    T = min(L, max(0, Tmax - pos0))
    src = qkv.view(R, L, ldq)[:, :T]
    for f, b, col in ((flat[0], before[0], H * HD), (flat[1], before[1], (H + HKV) * HD)):
        want = b.clone()
        rows = src[..., col:col + HKV * HD].reshape(R, T, HKV, HD).permute(0, 2, 1, 3)
        want[:n].view(R, HKV, Tmax, HD)[:, :, pos0:pos0 + T] = rows.contiguous().view(torch.int16)
        assert torch.equal(_bits(f), want)
        assert T == 0 or not torch.equal(want, b)


# ================================================================================================ SwiGLU
@pytest.mark.parametrize("tokens,i", tr.SWIGLU_SHAPES)
def test_swiglu_forward_and_backward_per_element(dev, tokens, i):
    """(1031, 4096): 527 872 work items, past the grid cap; (5, 8): one 16-byte chunk per token.  Row 0 starts with the gates where
    1 + exp(-g) overflows fp32, where it is finite but its reciprocal is subnormal, and the zeros (train_rows_ref.SWIGLU_GATES).
    At -88.5, -88 and -87.5 both kernels used to write 0 for values of about 1e-36 (v_rcp_f32 flushes a subnormal result; the
    forward rule missed by up to 1.7e-36): csrc/common.h now takes the reciprocal of d / 4 (docs/experiments.md)."""
    ops = _ops()
    gu, dact = tr.swiglu_input(tokens, i)
    act = ops.swiglu_fwd(gu.to(dev)).float().cpu()
    ref = swiglu_ref(gu).float()                      # bf16 ops on the CPU == the reference's autocast arithmetic
    assert torch.isfinite(act).all()
    # the rule of test_swiglu_fwd_bwd: silu(g) may round to the neighbouring bf16, then the product rounds once more
    worst = ((act - ref).abs() - (2.0 ** -6 * ref.abs() + 1e-37)).max().item()
    print(f"swiglu fwd ({tokens}, {i}): worst excess over the per-element rule {worst:.3e}; planted gates got {act[0, :13].tolist()}"
          f" want {ref[0, :13].tolist()}")
    assert ((act - ref).abs() <= 2.0 ** -6 * ref.abs() + 1e-37).all()
    dgu = ops.swiglu_bwd(gu.to(dev), dact.to(dev)).float().cpu()
    want = tr.swiglu_bwd_restated(gu, dact)
    eg, eu = tr.swiglu_excess(dgu, want)
    n = min(i, len(tr.SWIGLU_GATES))
    print(f"swiglu bwd ({tokens}, {i}): dgate {eg:.3f} dup {eu:.3f} of the bar; planted gates: dgate got {dgu[0, :n].tolist()} want "
          f"{want.dgate[0, :n].tolist()}; dup got {dgu[0, i:i + n].tolist()} want {want.dup[0, :n].tolist()}")
    assert torch.isfinite(dgu).all()
    assert eg <= 1.0 and eu <= 1.0


# ================================================================================================ cross entropy
def _ce_buf(logits, ld, dev):
    R, V = logits.shape
    buf = torch.full((R, ld), 7.0, dtype=BF, device=dev)
    buf[:, :V] = logits.to(dev)
    return buf


@functools.lru_cache(maxsize=None)
def _ce_case(R, V):
    logits, labels = tr.ce_input(R, V)
    return logits, labels, tr.ce_restated(logits, labels)


def _check_ce_forward(dev, logits, labels, ld, ref, what):
    ops = _ops()
    R, V = logits.shape
    lc, lse, loss_row, logp = ops.ce_fwd(_ce_buf(logits, ld, dev), V, labels.to(dev), want_logp=True)
    lc, lse, loss_row, logp = (t.cpu() for t in (lc, lse, loss_row, logp))
    e = [tr.ce_row_excess(g, w, ref.lse) for g, w in ((lse, ref.lse), (loss_row, ref.loss_row), (logp, ref.logp))]
    print(f"ce fwd {what}: lse {e[0]:.3f} loss_row {e[1]:.3f} logp {e[2]:.3f} of the bar; count {lc[1].item()} want {ref.count}; "
          f"loss {lc[0].item()!r} want {ref.loss.item()!r} bar {tr.ce_mean_bar(ref, R) if ref.count else 0:.2e}")
    assert max(e) <= 1.0
    assert (loss_row[~ref.valid] == 0).all() and (logp[~ref.valid] == 0).all()
    assert lc[1].item() == ref.count
    if ref.count:
        assert abs(lc[0].item() - ref.loss.item()) <= tr.ce_mean_bar(ref, R)
    else:
        assert math.isnan(lc[0].item())


def _check_ce_backward(dev, logits, labels, ld, what):
    """ug_ce_bwd on its own: lse (float64, rounded to fp32) and the count are handed in, so the gradient's reference is exact in them"""
    ops = _ops()
    R, V = logits.shape
    base = tr.ce_restated(logits, labels)
    lse32 = base.lse.float()
    lc = torch.tensor([0.0, float(base.count)], device=dev)
    rs = torch.randn(R, generator=tr._gen(V + R))
    for name, kw in (("gscale", dict(gscale=0.5)), ("plain mean", dict()), ("row_scale", dict(row_scale=rs))):
        ref = tr.ce_restated(logits, labels, lse=lse32, **kw)
        buf = _ce_buf(logits, ld, dev)
        ops.ce_bwd_(buf, V, labels.to(dev), lse32.to(dev), None if name == "row_scale" else lc,
                    gscale=torch.tensor([0.5], device=dev) if name == "gscale" else None,
                    row_scale=rs.to(dev) if name == "row_scale" else None)
        got = buf.float().cpu()
        e = tr.ce_grad_excess(got[:, :V], ref)
        print(f"ce bwd {what} {name}: {e:.3f} of the bar")
        assert torch.isfinite(got).all()
        assert e <= 1.0, name
        assert (got[:, V:] == 0).all() and (got[~ref.valid] == 0).all(), name
        if base.count:
            assert (got[ref.valid][:, :V] != 0).any()


@pytest.mark.parametrize("R,V,ld", tr.CE_CASES)
def test_ce_forward_per_row_and_backward_per_element(dev, R, V, ld):
    """V = 5: no vector chunk; 24: three active lanes; 2048: one chunk per lane; 2051, 4101: a ragged tail; 159 867: the shipped
    vocabulary, 78 or 79 chunks per lane; (300, 16): the loss reduction's loop over R > 256.  Rows carry a logit dominant by more than
    20 in each region a kernel could skip, so skipping it misses lse by about 20 (train_rows_ref.ce_planted_columns)."""
    logits, labels, ref = _ce_case(R, V)
    _check_ce_forward(dev, logits, labels, ld, ref, f"({logits.shape[0]}, {V}, ld {ld})")
    _check_ce_backward(dev, logits, labels, ld, f"({logits.shape[0]}, {V}, ld {ld})")


def test_ce_all_rows_ignored(dev):
    """loss = 0 / 0 = NaN like F.cross_entropy, count 0, the gradient exactly zero (and finite) in every form"""
    logits, _, _ = _ce_case(None, 2051)
    labels = torch.full((logits.shape[0],), tr.IGNORE)
    assert math.isnan(torch.nn.functional.cross_entropy(logits.float(), labels, ignore_index=tr.IGNORE).item())
    _check_ce_forward(dev, logits, labels, 2112, tr.ce_restated(logits, labels), "all ignored")
    _check_ce_backward(dev, logits, labels, 2112, "all ignored")
    ops = _ops()                                       # and chained as the product chains it: the forward's own NaN / 0 block
    buf = _ce_buf(logits, 2112, dev)
    lc, lse, _, _ = ops.ce_fwd(buf, 2051, labels.to(dev))
    ops.ce_bwd_(buf, 2051, labels.to(dev), lse, lc, torch.tensor([0.5], device=dev))
    assert (buf == 0).all()


def test_ce_label_out_of_range_is_an_ignored_row(dev):
    """A label that is neither ignore_index nor inside [0, V) (include/unigen_hip.h): loss_row = logp = 0, not counted -- the mean is
    over the valid rows -- and a zero gradient row in the mean form and the row_scale form."""
    logits, labels, _ = _ce_case(None, 2051)
    labels = labels.clone()
    R, V = logits.shape
    labels[2], labels[5], labels[6], labels[7] = V, -1, V + 1000, 1 << 40
    ref = tr.ce_restated(logits, labels)
    assert ref.count == R - 5 and int((labels == tr.IGNORE).sum()) == 1
    _check_ce_forward(dev, logits, labels, 2112, ref, "out-of-range labels")
    _check_ce_backward(dev, logits, labels, 2112, "out-of-range labels")


# ================================================================================================ column sums, embedding (integers: exact)
@pytest.mark.parametrize("R", [1, 3, 255, 256, 257, 1000])
def test_colsum_exact_on_integers(dev, R):
    """256 rows per block: R = 255 / 256 / 257 and 1000 (four row blocks, their partial sums meet in atomics); 64 columns per block:
    C = 63 / 64 / 65 and 200.  x is a column slice of a wider buffer; out accumulates, and its columns past C are not touched."""
    ops = _ops()
    for C in (1, 63, 64, 65, 200):
        wide = tr.int_bf16(R, C + 40, seed=R * 1000 + C).to(dev)
        x = wide[:, 8:8 + C]
        out0 = tr.distinct_ints(C + 7, seed=C)
        out = out0.clone().to(dev)
        ops.colsum_(x, out, R, C)
        want = out0.clone()
        want[:C] += x.float().cpu().sum(0)
        assert want.abs().max().item() < 2 ** 24
        assert torch.equal(out.cpu(), want), (R, C)


EMBED_CASES = [(97, 333, 256), (700, 333, 1536), (5, 9, 4)]        # 700 * 1536 = 1 075 200 work items (backward), past the cap


@pytest.mark.parametrize("tokens,V,H", EMBED_CASES + [(97, 333, 6)])
def test_embed_bwd_exact_on_integers(dev, tokens, V, H):
    """dW += index_add of integer rows: exact whatever order the atomics land in, so two runs are bit-equal too; ids -1 and V add
    nothing; H = 6: the backward does not need H % 4 == 0"""
    ops = _ops()
    ids = tr.embed_ids(tokens, V, seed=tokens + H, bad=True)
    dout = tr.int_f32(tokens, H, seed=H)
    dW0 = tr.int_prefill(V, H, seed=V + H)
    good = (ids >= 0) & (ids < V)
    assert int((~good).sum()) == 2 and int((ids == 7).sum()) >= tokens // 3 and (ids == 0).any() and (ids == V - 1).any()
    want = dW0.clone().index_add_(0, ids[good], dout[good])
    outs = []
    for _ in range(2):
        dW = dW0.clone().to(dev)
        ops.embed_bwd(ids.to(dev), dout.to(dev), dW)
        outs.append(dW.cpu())
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)


@pytest.mark.parametrize("tokens,V,H", EMBED_CASES)
def test_embed_fwd_exact_and_error_flag(dev, tokens, V, H):
    """out = W[ids] bit for bit; the error flag is raised by an id below 0 and by one at or past V, each on its own, and stays clear
    otherwise; a bad id reads row 0"""
    ops = _ops()
    W = torch.randn(V, H, generator=tr._gen(V * H))
    ids = tr.embed_ids(tokens, V, seed=tokens)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.embed_fwd(ids.to(dev), W.to(dev), err)
    assert torch.equal(out.cpu(), W[ids]) and err.item() == 0
    for bad in (-1, V, -(1 << 40), 1 << 40):
        b = ids.clone()
        b[tokens - 2] = bad
        err.zero_()
        out = ops.embed_fwd(b.to(dev), W.to(dev), err)
        b[tokens - 2] = 0
        assert err.item() == 1, bad
        assert torch.equal(out.cpu(), W[b]), bad
