"""The row / element-wise entry points the product calls (modules.py, qwen2.py, dpo.py, siglip_encoder.py) that no kernel test called
directly: one test per entry point, through unigen_hip.ops, against float64 on the CPU, at each kernel's own branch points (one
wave per row, rows per block, grid caps and grid-stride loops, vector tails, padded leading dimensions).

Tolerances: the project's existing bars for the same kind of op (1e-6 for an fp32 normalisation forward, 1e-5 for its gradients,
exact equality for data movement); one bf16 ulp for a bf16 result of an fp32 computation (one rounding of a value known to fp32
accuracy); for fp32 transcendentals 8 x the error of torch's own fp32 CPU evaluation against fp64 on the same inputs, computed
and printed here (the hardware tanhf is not torch's, and 1 + tanh(u) cancels for negative u: no fixed relative bar is right).
Outputs are pre-filled with NaN wherever "every element is written" or "the padding is zeroed" is part of the contract."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def _ops():
    from unigen_hip import ops
    return ops


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _within_one_ulp(got, want, extra=None):
    """bf16 tensors: |got - want| <= one bf16 ulp of the larger magnitude (as test_decode_parity_gpu.py) [+ extra, elementwise]"""
    a, b = got.float().cpu(), want.float().cpu()
    m = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(m > 0, torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-38))) - 7), torch.zeros(()))
    return bool(((a - b).abs() <= (ulp if extra is None else ulp + extra)).all())


def _round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------ LayerNorm (one wave per row; backward: 32 rows per block, LDS partials)
@pytest.mark.parametrize("rows", [1, 33, 130])
@pytest.mark.parametrize("cols", [1, 72, 1152, 8192])
def test_layernorm_f32_fwd_bwd(dev, rows, cols):
    ops = _ops()
    gen = torch.Generator().manual_seed(rows * 10007 + cols)
    x = torch.randn(rows, cols, generator=gen) * 2 + 0.5
    gamma, beta = torch.randn(cols, generator=gen) * 0.2 + 1, torch.randn(cols, generator=gen) * 0.1
    dy, dres = torch.randn(rows, cols, generator=gen), torch.randn(rows, cols, generator=gen)
    xd, gd, bd = (t.double().clone().requires_grad_(True) for t in (x, gamma, beta))
    ref = F.layer_norm(xd, (cols,), gd, bd, 1e-6)
    ref.backward(dy.double())
    y = ops.layernorm_f32(x.to(dev), gamma.to(dev), beta.to(dev), 1e-6)
    if cols > 1:
        assert _rel(y, ref.detach()) < 1e-6
    else:                                                    # one column: (x - mean) = 0, y = beta exactly
        assert torch.equal(y.cpu(), beta.expand(rows, 1))
    dg0, db0 = torch.randn(cols, generator=gen), torch.randn(cols, generator=gen)      # accumulate into what is there
    for with_res in (False, True):
        dg, db = dg0.clone().to(dev), db0.clone().to(dev)
        dx = ops.layernorm_bwd_f32(dy.to(dev), x.to(dev), gamma.to(dev), 1e-6, dg, db, dres_in=dres.to(dev) if with_res else None)
        want = xd.grad + (dres.double() if with_res else 0)
        if cols > 1:
            assert _rel(dx, want) < 1e-5, (with_res, _rel(dx, want))
            assert _rel(dg, dg0.double() + gd.grad) < 1e-5
        else:
            assert (dx.cpu().double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
            assert _rel(dg, dg0) < 1e-5                      # xhat = 0: nothing is added
        assert _rel(db, db0.double() + bd.grad) < 1e-5


def test_layernorm_bwd_refuses_more_columns_than_its_lds_holds(dev):
    ops = _ops()
    from unigen_hip.lib import UniGenHipError
    z = torch.zeros(2, 8193, device=dev)
    g = torch.zeros(8193, device=dev)
    with pytest.raises(UniGenHipError):
        ops.layernorm_bwd_f32(z, z, g, 1e-6, g.clone(), g.clone())


# ------------------------------------------------------------------ gelu_pytorch_tanh, fp32
GELU_SPECIALS = [0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0, 30.0, -30.0]


@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 3])      # the last: past the grid cap (8192 blocks of 256), grid-stride loop
def test_gelu_tanh_f32_fwd_bwd(dev, n):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * 2
    ns = min(n, len(GELU_SPECIALS))
    x[-ns:] = torch.tensor(GELU_SPECIALS[:ns])                       # in the tail, where the grid-stride loop ends
    dy = torch.randn(n, generator=gen)
    xd = x.double().clone().requires_grad_(True)
    ref = F.gelu(xd, approximate="tanh")
    ref.backward(dy.double())
    x32 = x.clone().requires_grad_(True)
    t32 = F.gelu(x32, approximate="tanh")
    t32.backward(dy)
    got = ops.gelu_tanh_f32(x.to(dev)).cpu()
    dgot = ops.gelu_tanh_f32(x.to(dev), dy.to(dev)).cpu()
    assert torch.isfinite(got).all() and torch.isfinite(dgot).all()
    for what, g, r, t in (("fwd", got, ref.detach(), t32.detach()), ("bwd", dgot, xd.grad, x32.grad)):
        err = (g.double() - r).abs().max().item()
        yard = (t.double() - r).abs().max().item()
        print(f"    gelu_tanh_f32 n={n} {what}: max abs error {err:.3e} (torch fp32 on the CPU {yard:.3e})")
        assert err <= 8 * yard, (what, err, yard)


# ------------------------------------------------------------------ softmax backward rows (one wave per row, padded leading dimension)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 729])
def test_softmax_bwd_rows(dev, rows, cols):
    ops = _ops()
    gen = torch.Generator().manual_seed(rows * 1009 + cols)
    for ld in (_round_up(cols, 4), cols + 7):
        s = torch.randn(rows, cols, generator=gen).double().requires_grad_(True)
        P = torch.softmax(0.3 * s, -1)
        dP = torch.randn(rows, cols, generator=gen)
        P.backward(dP.double())
        Pb = torch.full((rows, ld), NAN)
        dPb = torch.full((rows, ld), NAN)
        Pb[:, :cols], dPb[:, :cols] = P.detach().float(), dP
        out = ops.softmax_bwd_rows_(Pb.to(dev), dPb.to(dev), 0.3, cols).cpu()
        assert (out[:, cols:] == 0).all()                                          # the padding of dP: NaN on entry, 0 on exit
        # fp32 arithmetic on fp32-rounded probabilities: the project's 1e-5 bar for fp32 gradients, per row (absolute for the
        # single column, whose gradient is zero up to the rounding of P * dP)
        err = (out[:, :cols].double() - s.grad).norm(dim=-1)
        ref = s.grad.norm(dim=-1)
        assert (err <= 1e-5 * torch.maximum(ref, 0.3 * dP.double().norm(dim=-1) / max(cols, 1) ** 0.5)).all(), (ld, err, ref)


# ------------------------------------------------------------------ column sums, fp32 (64 rows per block, 256 columns per block)
@pytest.mark.parametrize("rows", [1, 64, 65, 1000])
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1152])
def test_colsum_f32(dev, rows, cols):
    ops = _ops()
    gen = torch.Generator().manual_seed(rows * 4099 + cols)
    ld = cols + 5
    buf = torch.full((rows, ld), NAN)
    x = torch.randn(rows, cols, generator=gen)
    buf[:, :cols] = x
    out0 = torch.randn(cols, generator=gen)
    out = ops.colsum_f32_(buf.to(dev)[:, :cols], out0.clone().to(dev))
    want = out0.double() + x.double().sum(0)
    # an fp32 sum of `rows` terms: relative to the sum of magnitudes (the sum itself may cancel)
    mag = out0.double().abs() + x.double().abs().sum(0)
    assert ((out.cpu().double() - want).abs() <= 1e-6 * mag).all()


# ------------------------------------------------------------------ transpose (32 x 32 tiles, batched, zero tail)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (729, 72), (72, 729)])
def test_transpose_f32(dev, rows, cols, batch):
    ops = _ops()
    gen = torch.Generator().manual_seed(rows * 733 + cols + batch)
    ld_in, pad_to = cols + 3, 8
    stride_in = rows * ld_in + 11
    buf = torch.full((batch * stride_in,), NAN)
    x = torch.randn(batch, rows, cols, generator=gen)
    for z in range(batch):
        buf[z * stride_in: z * stride_in + rows * ld_in].view(rows, ld_in)[:, :cols] = x[z]
    ld_out = _round_up(rows, pad_to)
    out = torch.full((batch, cols, ld_out), NAN, device=dev)
    got = ops.transpose_f32(buf.to(dev), rows, cols, batch=batch, ld_in=ld_in, stride_in=stride_in, pad_to=pad_to, out=out).cpu()
    assert torch.equal(got[:, :, :rows], x.transpose(1, 2))
    assert (got[:, :, rows:] == 0).all()                                           # the zero tail up to pad_to
    if batch == 1:                                                                  # the plain 2-D form, default padding to 4
        got2 = ops.transpose_f32(x[0].contiguous().to(dev)).cpu()
        assert got2.shape == (1, cols, _round_up(rows, 4))
        assert torch.equal(got2[0, :, :rows], x[0].t()) and (got2[0, :, rows:] == 0).all()


# ------------------------------------------------------------------ GELU (erf), bf16
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (2048 * 256 + 5)])      # the last: past the grid cap of 2048 blocks
def test_gelu_bf16_fwd_bwd(dev, n):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=gen) * 2).to(BF)
    x[-8:] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0, 30.0, -30.0]).to(BF)
    dy = torch.randn(n, generator=gen).to(BF)
    xd = x.double().clone().requires_grad_(True)
    ref = F.gelu(xd)
    ref.backward(dy.double())
    got = ops.gelu(x.to(dev))
    dgot = ops.gelu(x.to(dev), dy.to(dev))
    # one bf16 rounding of a value known to fp32 accuracy: within one bf16 ulp of the rounded fp64 result.  In the negative tail the
    # fp32 value itself is only known absolutely: 0.5 (1 + erf) is formed at magnitude 1, so x * cdf carries up to |x| * 2^-23
    # (erff's own last bits included) whatever is left after the cancellation -- at x = -5 that is 4 % of the result
    assert _within_one_ulp(got, ref.detach().to(BF), extra=x.float().abs() * 2.0 ** -23)
    assert _within_one_ulp(dgot, xd.grad.to(BF), extra=dy.float().abs() * 2.0 ** -22)


# ------------------------------------------------------------------ row gather / scatter (bf16, 16-byte chunks)
@pytest.mark.parametrize("C", [8, 1536])
def test_gather_and_scatter_rows(dev, C):
    ops = _ops()
    gen = torch.Generator().manual_seed(C)
    R, n = 301, 777
    wide = torch.randn(R, C + 24, generator=gen).to(BF)
    src = wide[:, 16:16 + C]                                                       # a column view of a wider buffer
    idx = torch.randint(0, R, (n,), generator=gen)
    idx[::7] = 5                                                                   # repeated indices
    got = ops.gather_rows(wide.to(dev)[:, 16:16 + C], idx.to(dev))
    assert torch.equal(got.cpu(), src[idx])
    perm = torch.randperm(R, generator=gen)
    out_wide = torch.full((R + 3, C + 8), 7.0, dtype=BF, device=dev)
    out = out_wide[:, 8:8 + C] if C > 8 else out_wide[:, :C]
    ops.scatter_rows_(wide.to(dev)[:, 16:16 + C], perm.to(dev), out)
    want = torch.full((R + 3, C + 8), 7.0, dtype=BF)
    (want[:, 8:8 + C] if C > 8 else want[:, :C])[perm] = src
    assert torch.equal(out_wide.cpu(), want)                                       # the listed rows, and nothing else


# ------------------------------------------------------------------ fp32 -> bf16 cast (four elements per lane + a tail)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 4099, 2 ** 21 + 3])
def test_cast_bf16(dev, n):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * 3
    special = torch.tensor([1.00390625, 1.01171875, -1.00390625, 1.0039063692092896, 1.0039061307907104,   # ties to even, just off a tie
                            float("inf"), -float("inf"), NAN, 1e-40, -1e-40, 3.3895313892515355e38, 0.0, -0.0, 65280.0, 9.18e-41])
    k = min(n, special.numel())
    x[-k:] = special[:k]                                                           # in the tail
    out = torch.full((n,), NAN, dtype=BF, device=dev)
    got = ops.cast_bf16(x.to(dev), out).cpu()
    want = x.to(BF)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
