"""The element-wise kernels every training step and every forward pass goes through -- ug_rmsnorm_fwd / _bwd, ug_adamw_flat / _dev,
ug_cast_f32_bf16, the tokenizer's ug_groupnorm_swish / _stats / _finalize and ug_softmax_rows_f32 -- each against a float64
restatement of its own (tests/elementwise_ref.py), through unigen_hip.ops, at the smallest shapes that reach every branch.

What is exact is tested exactly: the RMSNorm backward on integer-valued inputs (dw at every width in whatever order the atomics land,
dres and its bf16 copy at power-of-two widths), the cast against torch's round-to-nearest-even over every upper half of an fp32,
AdamW against its operation-by-operation fp32 restatement (p, m, v and the bf16 copy, three steps from a non-zero state), GroupNorm
of a constant group, groupnorm_finalize against groupnorm_stats on integer-valued tensors, the zero pad columns of the softmax.
Everything else is judged PER ELEMENT,

    |got - v| <= 2^-8 |v| (bf16 outputs only) + slack * a,

by bars that were measured on the CPU with no kernel involved (the constants, the magnitudes a and the rule are in elementwise_ref.py;
docs/experiments.md, "Element-wise kernels: exact and per-element tests").  tests/test_elementwise_ref_cpu.py shows without a GPU
that these bars reject a wrong reference of each kind by 2 x.

Outputs are pre-filled (NaN, or a sentinel) wherever "everything is written" or "nothing else is touched" is the contract.  Every
test prints the worst ratio it reached against its bar before it asserts (`EXCESS ...` lines under pytest -s)."""
import pytest
import torch

import elementwise_ref as ew

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def _ops():
    from unigen_hip import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu().clone()


def _report(what, case, **ratios):
    print("EXCESS", what, case, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


# ================================================================================================ RMSNorm forward
@pytest.mark.parametrize("cols", ew.RMS_FWD_WIDTHS)
@pytest.mark.parametrize("rows", ew.RMS_FWD_ROWS)
def test_rmsnorm_forward_per_element(dev, rows, cols):
    """rstd per row, y per element (bf16: the register kernel up to 2048 columns, the two-pass kernel beyond; fp32: the two-pass
    kernel at every width); an all-zero row gives y == 0 and rstd = eps^-1/2, a row of 1e-4 shows eps, a row with one 1e4 outlier;
    want_rstd=False (the inference launch) and out= give the same bits, and rows past the end of `out` stay NaN"""
    ops = _ops()
    w, xs = ew.rms_fwd_inputs(rows, cols)
    wd = w.to(dev)
    for k, x in enumerate(xs):
        xd = x.to(dev)
        ref = ew.rms_fwd_restated(x, w)
        y, rstd = ops.rmsnorm_fwd(xd, wd, ew.EPS)
        y32, rstd32 = ops.rmsnorm_fwd(xd, wd, ew.EPS, out_f32=True)
        assert y.dtype == BF and y32.dtype == torch.float32 and rstd.shape == (rows,)
        e = dict(rstd=ew.rms_rstd_excess(rstd.cpu(), ref), y=ew.rms_y_excess(y.cpu(), ref),
                 rstd_f32=ew.rms_rstd_excess(rstd32.cpu(), ref), y_f32=ew.rms_y_excess(y32.cpu(), ref))
        _report("rmsnorm_fwd", (rows, cols, k), **e)
        assert max(e.values()) <= 1, e
        zero = (x == 0).all(-1)
        assert (y.cpu()[zero] == 0).all() and (y32.cpu()[zero] == 0).all()
        # the launch without rstd, and into a caller's buffer with spare rows
        y_no, none = ops.rmsnorm_fwd(xd, wd, ew.EPS, want_rstd=False)
        assert none is None and torch.equal(_bits(y_no), _bits(y))
        for f32, want in ((False, y), (True, y32)):
            buf = torch.full((rows + 2, cols), NAN, dtype=want.dtype, device=dev)
            got, r2 = ops.rmsnorm_fwd(xd, wd, ew.EPS, out_f32=f32, out=buf[:rows])
            assert got.data_ptr() == buf.data_ptr() and torch.equal(_bits(buf[:rows]), _bits(want)) and buf[rows:].isnan().all()
            assert torch.equal(_bits(r2), _bits(rstd32 if f32 else rstd))


# ================================================================================================ RMSNorm backward
def _rms_bwd(ops, dev, p, want_bf16):
    """-> dres, dw (a 16-byte aligned slice of a sentinel buffer), the buffer, the NaN-prefilled bf16 copy (or None)"""
    rows, cols = p.x.shape
    dres = p.dres0.clone().to(dev)
    buf = torch.full((cols + 8,), ew.SENTINEL, device=dev)
    dw = buf[4:4 + cols]
    dw.copy_(p.dw0)
    assert dw.data_ptr() % 16 == 0
    d16 = torch.full((rows, cols), NAN, dtype=BF, device=dev) if want_bf16 else None
    # (ops.rmsnorm_bwd allocates its bf16 copy itself: the entry point directly, so that the copy can be pre-filled)
    dy, x, rstd, w = p.dy.to(dev), p.x.to(dev), p.rstd.to(dev), p.w.to(dev)
    ops._l.api().ug_rmsnorm_bwd(ops._p(dy), ops._p(x), ops._p(rstd), ops._p(w), ops._p(dres), ops._p(dw), ops._p(d16), rows, cols,
                                ops._stream())
    torch.cuda.synchronize()
    return dres, dw, buf, d16


def _sentinels_intact(buf, cols):
    b = buf.cpu()
    return bool((b[:4] == ew.SENTINEL).all() and (b[4 + cols:] == ew.SENTINEL).all())


@pytest.mark.parametrize("rows,cols", [(r, c) for c in ew.RMS_BWD_DW_WIDTHS for r in ew.RMS_BWD_ROWS] + [ew.RMS_BWD_MANY_ROWS])
def test_rmsnorm_backward_exact_on_integer_inputs(dev, rows, cols):
    """dw (its non-zero initial value included) bit for bit at every width, dres and its bf16 copy bit for bit at the power-of-two
    widths; 17 rows: a second workgroup holding one row; (7700, 256): 20 rows per workgroup, 385 workgroups' atomics"""
    ops = _ops()
    p = ew.rms_bwd_int_input(rows, cols)
    ref = ew.rms_bwd_restated(p)
    dres, dw, buf, d16 = _rms_bwd(ops, dev, p, True)
    assert torch.equal(dw.cpu(), ref.dw.float()), f"dw: {int((dw.cpu() != ref.dw.float()).sum())} of {cols} columns differ"
    assert _sentinels_intact(buf, cols), "written outside dw"
    assert not d16.isnan().any(), "an element of the bf16 copy was not written"
    assert torch.equal(_bits(d16), _bits(dres.to(BF)))
    if cols in ew.RMS_BWD_DRES_EXACT_WIDTHS or (rows, cols) == ew.RMS_BWD_MANY_ROWS:
        want = ref.dres.float()
        assert torch.equal(dres.cpu(), want), f"dres: {int((dres.cpu() != want).sum())} of {want.numel()} elements differ"
        assert torch.equal(_bits(d16), _bits(want.to(BF)))
    dres2, dw2, buf2, none = _rms_bwd(ops, dev, p, False)
    assert none is None and torch.equal(_bits(dres2), _bits(dres)) and torch.equal(_bits(dw2), _bits(dw)) and _sentinels_intact(buf2, cols)
    # and through ops.rmsnorm_bwd, as the model calls it
    dres3, dw3 = p.dres0.clone().to(dev), p.dw0.clone().to(dev)
    d16_3 = ops.rmsnorm_bwd(p.dy.to(dev), p.x.to(dev), p.rstd.to(dev), p.w.to(dev), dres3, dw3, want_bf16=True)
    assert torch.equal(_bits(dres3), _bits(dres)) and torch.equal(_bits(dw3), _bits(dw)) and torch.equal(_bits(d16_3), _bits(d16))


@pytest.mark.parametrize("rows,cols", ew.RMS_BWD_REAL_CASES)
def test_rmsnorm_backward_per_element_on_real_inputs(dev, rows, cols):
    ops = _ops()
    p = ew.rms_bwd_real_input(rows, cols)
    ref = ew.rms_bwd_restated(p)
    dres, dw, buf, d16 = _rms_bwd(ops, dev, p, True)
    e = dict(dres=ew.fp32_excess(dres.cpu(), ref.dres, ref.dres_a, ew.RMS_BWD_DRES_SLACK).max().item(),
             dw=ew.fp32_excess(dw.cpu(), ref.dw, ref.dw_a, ew.RMS_BWD_DW_SLACK).max().item(),
             dres_bf16=ew.excess(d16.cpu(), ref.dres, ref.dres_a, ew.RMS_BWD_DRES_SLACK).max().item())
    _report("rmsnorm_bwd", (rows, cols), **e)
    assert max(e.values()) <= 1, e
    assert _sentinels_intact(buf, cols) and torch.equal(_bits(d16), _bits(dres.to(BF)))


# ================================================================================================ AdamW
def _ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place (same-sign finite values)"""
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("name", list(ew.ADAM_SETS))
def test_adamw_bit_for_bit_against_the_fp32_restatement(dev, name):
    """p, m, v and the bf16 copy over three successive steps from a random non-zero state equal the update restated operation by
    operation in fp32 on the CPU (every operation of adamw_element is one IEEE operation, contraction off), at sizes with 0, 1, 2 and
    many trips of the pipelined loop and a scalar tail, on the default grid and on two workgroups; and each step is within the
    per-element rule of a float64 evaluation from the same state with the same fp32-rounded hyper-parameters"""
    ops = _ops()
    hp = ew.ADAM_SETS[name]
    fac = None if hp["factor"] is None else torch.tensor([hp["factor"]], dtype=torch.float32, device=dev)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for n in ew.ADAM_SIZES:
        p0, m0, v0, grads = ew.adam_state(n, name)
        for mb in ew.ADAM_MAX_BLOCKS:
            p, m, v = p0.clone(), m0.clone(), v0.clone()
            pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
            pb = torch.full((n,), NAN, dtype=BF, device=dev) if hp["bf16"] else None
            for s, g in enumerate(grads):
                step = hp["first_step"] + s
                args = (pd, g.to(dev), md, vd, pb, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], step)
                if fac is None:
                    ops.adamw_flat_(*args, grad_scale=hp["grad_scale"], max_blocks=mb)
                else:
                    ops.adamw_flat_dev_(*args, grad_scale=hp["grad_scale"], grad_factor=fac, max_blocks=mb)
                p64, m64, v64, a = ew.adam_step(p.double(), g.double(), m.double(), v.double(), ew.adam_consts(hp, step, f64=True))
                p, m, v, _ = ew.adam_step(p, g, m, v, ew.adam_consts(hp, step))
                got = (pd.cpu(), md.cpu(), vd.cpu())
                for key, gt, v64_, a_, sl in zip("pmv", got, (p64, m64, v64), (a.p, a.m, a.v), (ew.ADAM_P_SLACK, ew.ADAM_M_SLACK, ew.ADAM_V_SLACK)):
                    worst[key] = max(worst[key], ew.fp32_excess(gt, v64_, a_, sl).max().item())
                ul = [_ulps(gt, w_) for gt, w_ in zip(got, (p, m, v))]
                if any(ul):
                    print(f"ADAMW {name} n={n} max_blocks={mb} step={step}: p/m/v differ from the fp32 restatement by up to {ul} ulps in "
                          f"{[int((gt != w_).sum()) for gt, w_ in zip(got, (p, m, v))]} elements")
                for what, gt, w_ in zip("pmv", got, (p, m, v)):
                    assert torch.equal(gt, w_), (what, name, n, mb, step)
                if pb is not None:
                    assert torch.equal(_bits(pb), _bits(p.to(BF))), ("bf16 copy", name, n, mb, step)
    _report("adamw", name, **worst)
    assert max(worst.values()) <= 1, worst


# ================================================================================================ cast
@pytest.mark.parametrize("n", ew.CAST_LENGTHS)
def test_cast_is_round_to_nearest_even_on_every_upper_half(dev, n):
    """all 65536 upper halves times the lower halves 0x0000, 0x7fff, 0x8000, 0x8001, 0xffff (ties to even, the round-up to infinity
    below fp32 max, signed zeros, subnormals; a NaN has to stay a NaN), the scalar tail, a length past the capped grid; the output
    is a slice of a sentinel buffer"""
    ops = _ops()
    x = ew.cast_input(n)
    want, nan = ew.cast_expected(x)
    buf = torch.full((n + 12,), 0x5a5a, dtype=torch.int16, device=dev)
    out = buf.view(BF)[4:4 + n]
    assert out.data_ptr() % 8 == 0
    ops.cast_bf16(x.to(dev), out=out)
    b = buf.cpu()
    assert (b[:4] == 0x5a5a).all() and (b[4 + n:] == 0x5a5a).all(), "written outside the output"
    got = b[4:4 + n]
    bad = (got != want) & ~nan
    assert not bad.any(), (f"{int(bad.sum())} of {n} differ; first: " +
                           str([(hex(int(x.view(torch.int32)[i]) & 0xffffffff), hex(int(got[i]) & 0xffff), hex(int(want[i]) & 0xffff))
                                for i in bad.nonzero()[:8, 0].tolist()]))
    assert ew.is_bf16_nan(got[nan]).all(), "a NaN came out as a number"


# ================================================================================================ GroupNorm
@pytest.mark.parametrize("case", ew.GN_CASES, ids=str)
def test_groupnorm_stats_and_output_per_element(dev, case):
    """(mean, rstd) per (image, group) and y per element, swish on and off: C = 1024 (one pixel per thread pass) down to 32, 8 to 32
    groups, HW = 1, HW that is no multiple of the pixels per workgroup, 128 pixels per workgroup, the capped grid of the apply
    kernel; a constant group (y == beta bit for bit) and a group whose mean of 1000 dwarfs its spread of 1e-2"""
    ops = _ops()
    B, H, W, C, G = case
    x, ga, be = ew.gn_input(case)
    st = ew.gn_stats_restated(x, G)
    xd, gd, bd = x.to(dev), ga.to(dev), be.to(dev)
    mr = ops.groupnorm_stats(xd, groups=G, eps=ew.EPS).cpu()
    assert mr.shape == (B, G, 2)
    e = dict(mean=ew.fp32_excess(mr[..., 0], st.mean, st.a_mean, ew.GN_STAT_SLACK).max().item(),
             rstd=ew.fp32_excess(mr[..., 1], st.rstd, st.a_rstd, ew.GN_STAT_SLACK).max().item())
    e["rstd_big_mean_rel"] = abs(mr[B - 1, G - 1, 1].item() / st.rstd[B - 1, G - 1].item() - 1) / ew.GN_STAT_SLACK   # (recorded only)
    assert mr[0, 1, 0].item() == ew.GN_CONST, "the constant group's mean is exact"
    cpg = C // G
    for sw, sl in ((False, ew.GN_Y_SLACK), (True, ew.GN_SWISH_SLACK)):
        y = ops.groupnorm_swish(xd, gd, bd, groups=G, eps=ew.EPS, swish=sw).cpu()
        v, a = ew.gn_apply_restated(x, ga, be, G, st, sw)
        e["y_swish" if sw else "y"] = ew.fp32_excess(y, v, a, sl).max().item()
        if not sw:
            assert torch.equal(y[0, :, :, cpg:2 * cpg], be[cpg:2 * cpg].expand(H, W, cpg)), "constant group: y == beta bit for bit"
    big = e.pop("rstd_big_mean_rel")
    _report("groupnorm", case, **e, rstd_big_mean_in_slacks=big)
    assert max(e.values()) <= 1, e


@pytest.mark.parametrize("case", ew.GN_CASES, ids=str)
def test_groupnorm_finalize_on_host_sums_is_groupnorm_stats(dev, case):
    """integer-valued x: the float64 sums are exact in any order, so sums built on the host are the sums the statistics kernel
    gathers, and the finish has to give the same (mean, rstd) bits from either; both are within the rule of float64"""
    ops = _ops()
    B, H, W, C, G = case
    x = ew.gn_int_input(case)
    _, _, sums = ew.gn_stats_one_pass(x, G)
    stats = torch.cat((sums.reshape(-1), torch.zeros(1, dtype=torch.float64))).to(dev)       # (the trailing max|y| slot of gn_stats_slots)
    a = ops.groupnorm_stats(x.to(dev), groups=G, eps=ew.EPS)
    b = ops.groupnorm_finalize(stats, B, H * W, C, groups=G, eps=ew.EPS)
    assert torch.equal(_bits(a), _bits(b))
    st = ew.gn_stats_restated(x, G)
    e = dict(mean=ew.fp32_excess(a.cpu()[..., 0], st.mean, st.a_mean, ew.GN_STAT_SLACK).max().item(),
             rstd=ew.fp32_excess(a.cpu()[..., 1], st.rstd, st.a_rstd, ew.GN_STAT_SLACK).max().item())
    _report("groupnorm_int", case, **e)
    assert max(e.values()) <= 1, e


# ================================================================================================ row softmax
def _softmax_case(dev, case, scale, extreme=False):
    ops = _ops()
    rows, cols, ld = case
    x = ew.softmax_input(case, extreme)
    flat = torch.full((rows * ld + 8,), ew.SENTINEL, device=dev)
    view = flat[:rows * ld].view(rows, ld)
    view[:, :cols] = x.to(dev)
    ops.softmax_rows_(view, scale, cols=cols)
    out = flat.cpu()
    got = out[:rows * ld].view(rows, ld)
    v, a = ew.softmax_restated(x, scale)
    e = ew.softmax_excess(got[:, :cols], v, a)
    pad = min(ld, ew.round_up(cols, 4))
    assert (got[:, cols:pad] == 0).all(), "pad columns up to the next multiple of four read as zero"
    assert (got[:, pad:] == ew.SENTINEL).all() and (out[rows * ld:] == ew.SENTINEL).all(), "written past the padded row"
    return e


@pytest.mark.parametrize("scale", ew.SOFTMAX_SCALES)
@pytest.mark.parametrize("case", ew.SOFTMAX_CASES, ids=str)
def test_softmax_rows_per_element(dev, case, scale):
    """one column; three columns with and without a pad column; 63 / 64 / 65 columns around one per lane; 729 of 732; 4097 columns"""
    e = _softmax_case(dev, case, scale)
    _report("softmax", (case, scale), softmax=e)
    assert e <= 1


def test_softmax_rows_extreme_scores(dev):
    """scores of +-300 at scale 1: exp(-600) underflows, nothing overflows, no NaN"""
    e = _softmax_case(dev, ew.SOFTMAX_EXTREME, 1.0, extreme=True)
    _report("softmax", "extreme", softmax=e)
    assert e <= 1
