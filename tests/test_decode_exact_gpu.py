"""The decode launches that fuse RMSNorm, the residual add or SwiGLU against exact expectations (tests/exact_products.py, "fused decode
launches": inputs whose bf16 operand is a known integer whatever the last bits of rsqrtf / __expf are, so everything behind the operand
is the integer contraction and has to come out bit for bit).

  ug_decode_gemv_resid_norm (+ _ord)   acc, x_out and ss_out bit for bit; the ordered twin slab by slab
  ug_decode_gemv_swiglu                acc bit for bit, both norm widths
  ug_decode_sw_gate_up                 x_out bit for bit; act bit for bit where silu is exact, within 2 bf16 ulps elsewhere, at most
                                       1 % of the elements differing at all (ep.gate_up_check)
  ug_decode_sw_head                    logits and x_out bit for bit
  ug_decode_finish_resid_norm (+ _ord) x, xn, the zeroed accumulator, the advance

Weights, pending accumulators and outputs have padded leading dimensions (K + 8, H + 8, N + 8) with a sentinel in the padding of
everything a launch writes; accumulating outputs start from integers.  Which kernel instantiation a shape reaches follows the rules of
csrc/decode.hip (launch_ring_auto) and csrc/decode_sw.hip (units_per_wg), restated in ep.ring_fused_shape / ep.sw_split and asserted
per shape in tests/test_exact_products_cpu.py:
  split-K prologues  cost(NW, KW) = ceil(ceil(groups / (NW KW)) * slabs / 256) * NW * KW over (4,1) (4,2) (7,2) (9,3), first cheapest;
                     more than 16 rows: four waves, two row blocks; >= 16 slabs and ceil(groups / 16) * ceil(slabs / 8) <= 32: XCD-major (8,2)
  single writer      units per workgroup = min(ceil(units / CUs), cap), cap 40 (gate_up, 8 units per tile) or 32 (head, 16 per tile)
"""
import pytest
import torch

import exact_products as ep

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
S = ep.SENTINEL


def _ops():
    from unigen_hip import ops
    return ops


def _padded(t, dev, pad=8):
    """[..., K] -> the [..., K] view of a device buffer with leading dimension K + pad (sentinel in the padding), and the buffer"""
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), S, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    buf = buf.to(dev)
    return buf[..., :t.shape[-1]], buf


def _guarded(n, dev):
    """n ones between two 4-float sentinel guards: a clear has to zero exactly the n"""
    buf = torch.full((n + 8,), S, device=dev)
    buf[4:4 + n] = 1.0
    return buf, buf[4:4 + n]


def _clears(dev, R):
    return [_guarded(n, dev) for n in (16 * 2048, R * 1536, 32)]


def _assert_cleared(clears):
    for buf, view in clears:
        assert float(view.abs().max()) == 0.0, "a clear left something behind"
        assert bool((buf[:4] == S).all()) and bool((buf[-4:] == S).all()), "a clear went past its range"


def _equal(got, want, what):
    got, want = got.cpu(), want.to(got.dtype).cpu()
    if not torch.equal(got, want):
        g2, w2 = got.float().reshape(-1, got.shape[-1]), want.float().reshape(-1, want.shape[-1])
        raise AssertionError(f"{what}: {ep.mismatch_report(g2, w2)}")


# ------------------------------------------------------------------------------------------------ 1. ug_decode_gemv_resid_norm
@pytest.mark.parametrize("R,N,K", ep.RESID_NORM_SHAPES)
def test_resid_norm_prologue(dev, R, N, K):
    """operand = bf16(norm_w * (x_in + bf16round(pending))): integers in +-4, never zero, against a dense weight; x_out and the row
    sums of squares (fp32 atomics of integers) bit for bit.  First launch with the clears, second without into the same accumulator.
    (1,16,256) one group, one slab; (5,333,1568) ragged N and a ragged last slab (the clamped re-read must not count in ss_out);
    (17,.) (32,.) two row blocks; (16,8208,1536) the (7,2) workgroup; (16,16400,1536) (9,3); (16,48,4864) 19 slabs: XCD-major (8,2)."""
    ops = _ops()
    p = ep.problem(R, N, K, "resid_norm")
    w, x_in, nw = ep.store(p.w, False, dev), p.x_in.to(dev), p.norm_w.to(dev)
    pend, pend_buf = _padded(p.pend, dev)
    pre, ss_pre = ep.int_prefill(R, N, seed=N + K), ep.int_prefill(1, 32, seed=R + K)[0]
    acc, ss = ep.out_buffer(R, N, F32, dev, prefill=pre), ss_pre.clone().to(dev)
    for rep, clears in ((1, _clears(dev, R)), (2, None)):
        x_out = torch.full((R + 1, K), S, device=dev)
        kw = dict(zero0=clears[0][1], zero1=clears[1][1], ss_zero=clears[2][1]) if clears else {}
        ops.decode_gemv_resid_norm_(x_in, pend, nw, x_out, ss, w, acc[:, :N], **kw)
        what = f"decode_gemv_resid_norm_ {(R, N, K)} call {rep}"
        ep.assert_exact(acc, N, pre + rep * p.acc, what)
        _equal(x_out[:R], p.xnew, what + " x_out")
        assert bool((x_out[R] == S).all()), what + ": wrote past the last row of x_out"
        want_ss = ss_pre.clone()
        want_ss[:R] += rep * p.ss
        _equal(ss.unsqueeze(0), want_ss.unsqueeze(0), what + " ss_out")
        if clears:
            _assert_cleared(clears)
    _equal(pend_buf, _padded(p.pend, "cpu")[1], "the pending accumulator is an input")


@pytest.mark.parametrize("npend", [0, 5])
@pytest.mark.parametrize("R,N,K", ep.RESID_NORM_ORD_SHAPES)
def test_resid_norm_prologue_ordered(dev, R, N, K, npend):
    """ug_decode_gemv_resid_norm_ord: slab s's slot holds exactly the products of k-slice s and its row sums of squares; the slot sums are
    the reference; padded slot rows and statistics past R stay untouched.  npend 5: the pending term is five slots summed in order."""
    ops = _ops()
    p = ep.problem(R, N, K, "resid_norm")
    w, nw = ep.store(p.w, False, dev), p.norm_w.to(dev)
    nslab, ld = (K + 255) // 256, ep.round_up(N, 8) + 8
    part, ss_part = torch.full((nslab, R, ld), S, device=dev), torch.full((nslab, 32), S, device=dev)
    x_out = torch.full((R, K), S, device=dev)
    if npend:
        parts, _ = _padded(p.parts5, dev)
        ops.decode_gemv_resid_norm_ord_(p.x_in.to(dev), parts, nw, x_out, ss_part, w, part)
    else:
        ops.decode_gemv_resid_norm_ord_(p.xnew.to(dev), None, nw, x_out, ss_part, w, part)
    what = f"decode_gemv_resid_norm_ord_ {(R, N, K)} npend {npend}"
    a, b = p.operand.float(), p.w.float()
    for s in range(nslab):
        sl = slice(s * 256, min(K, (s + 1) * 256))
        ep.assert_exact(part[s], N, a[:, sl] @ b[:, sl].t(), f"{what} slab {s}")
        want_ss = torch.full((32,), S)
        want_ss[:R] = (p.xnew[:, sl] ** 2).sum(-1)
        _equal(ss_part[s:s + 1], want_ss.unsqueeze(0), f"{what} ss slab {s}")
    _equal(part[:, :, :N].sum(0), p.acc, what + " slot sums")
    _equal(x_out, p.xnew, what + " x_out")


# ------------------------------------------------------------------------------------------------ 2. ug_decode_gemv_swiglu
@pytest.mark.parametrize("R,N,K", ep.SWIGLU_SHAPES)
def test_swiglu_prologue(dev, R, N, K):
    """operand = bf16(bf16(silu(g)) * u), g, u = bf16(rstd * gate|up accumulator) = G U or 0 exactly (rstd = 2^j by row, from ss_in =
    norm_cols 4^-j) against a {-1, 0, +1} weight: acc bit for bit at both norm widths, with and without the clears.
    (5,100,8992) ragged last slab; (16,1536,8960) XCD-major (8,2); (24,.) two row blocks; (16,1552,8960) just past the XCD-major limit:
    (7,2); (9,48,18944) 74 slabs; (16,16400,1536) the (9,3) workgroup."""
    ops = _ops()
    p = ep.problem(R, N, K, "swiglu")
    w = ep.store(p.w, False, dev)
    gu, gu_buf = _padded(p.gu, dev)
    pre = ep.int_prefill(R, N, seed=N + K + 1)
    acc, rep = ep.out_buffer(R, N, F32, dev, prefill=pre), 0
    for norm_cols in ep.SWIGLU_NORM_COLS:
        ss_in = torch.full((32,), S)
        ss_in[:R] = norm_cols * p.ss_unit
        ss_in = ss_in.to(dev)
        for clears in (_clears(dev, R), None):
            rep += 1
            kw = dict(zero0=clears[0][1], zero1=clears[1][1], ss_zero=clears[2][1]) if clears else {}
            ops.decode_gemv_swiglu_(gu, ss_in, ep.EPS, norm_cols, w, acc[:, :N], **kw)
            ep.assert_exact(acc, N, pre + rep * p.acc, f"decode_gemv_swiglu_ {(R, N, K)} norm_cols {norm_cols} call {rep}")
            if clears:
                _assert_cleared(clears)
    _equal(gu_buf, _padded(p.gu, "cpu")[1], "the gate|up accumulator is an input")


# ------------------------------------------------------------------------------------------------ 3. ug_decode_sw_gate_up
def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("R,I", ep.GATE_UP_SHAPES)
def test_sw_gate_up(dev, R, I):
    """RMSNorm with the statistics inside (per-row scale c_r: another row's rstd is no integer operand), SwiGLU in the epilogue.
    With 256 CUs: I = 8 one unit per workgroup and exactly the eight workgroups x_out needs; 264 two units; 2056 tiles 8 + 1 and a
    ragged last workgroup; 8960 the model's 35 = 8 8 8 8 3; 10248 the cap of 40 units and more workgroups than CUs.  R walks the
    edges of the 4-row register groups."""
    ops = _ops()
    p = ep.problem(R, I, ep.SW_HIDDEN, "gate_up")
    upw, grid, tiles, last = ep.sw_split(I, _ncu(dev), 40, 8)
    what = f"decode_sw_gate_up_ {(R, I)} (units/workgroup {upw}, workgroups {grid}, tiles {tiles}, last workgroup {last} units)"
    w, nw, target = ep.store(p.w, False, dev), p.norm_w.to(dev), p.target.to(dev)

    def run(*a, **kw):
        act = torch.full((R, I + 8), S, dtype=BF, device=dev)
        ops.decode_sw_gate_up_(*a, act[:, :I], **kw)
        assert bool((act[:, I:] == S).all()), what + ": wrote past column I"
        return act[:, :I]

    act = run(target, nw, ep.EPS, w)
    share = ep.gate_up_check(act, p, what)
    print(f"{what}: {share:.5%} of the elements differ from the fp64 expectation")
    assert torch.equal(run(target, nw, ep.EPS, w), act), what + ": two launches differ"
    pend, pend_buf = _padded(p.pend, dev)
    x_in = p.x_in.to(dev)
    assert torch.equal(run(x_in, nw, ep.EPS, w, pend=pend), act), what + ": with the pending accumulator"
    if grid >= 8:
        x_out = torch.full((R + 1, ep.SW_HIDDEN), S, device=dev)
        assert torch.equal(run(x_in, nw, ep.EPS, w, pend=pend, x_out=x_out), act), what + ": with pending and x_out"
        _equal(x_out[:R], p.target, what + " x_out")
        assert bool((x_out[R] == S).all()), what + ": wrote past the last row of x_out"
    _equal(pend_buf, _padded(p.pend, "cpu")[1], what + ": the pending accumulator is left as it is")


# ------------------------------------------------------------------------------------------------ 4. ug_decode_sw_head
@pytest.mark.parametrize("R,N", ep.HEAD_SHAPES)
def test_sw_head(dev, R, N):
    """fp32 logits of the integer contraction.  With 256 CUs: N = 128 one row per workgroup (half the CUs idle); 2047 the code-book
    slice of the tests' models; 4097 tiles 16 + 1; 8192 the model's 32 per workgroup; 8200 the cap of 32 and more workgroups than CUs."""
    ops = _ops()
    p = ep.problem(R, N, ep.SW_HIDDEN, "head")
    upw, grid, tiles, last = ep.sw_split(N, _ncu(dev), 32, 16)
    what = f"decode_sw_head_ {(R, N)} (rows/workgroup {upw}, workgroups {grid}, tiles {tiles}, last workgroup {last} rows)"
    w, nw, target = ep.store(p.w, False, dev), p.norm_w.to(dev), p.target.to(dev)

    def run(*a, **kw):
        logits = torch.full((R, N + 8), S, device=dev)
        ops.decode_sw_head_(*a, logits[:, :N], **kw)
        ep.assert_exact(logits, N, p.logits, what)

    run(target, nw, ep.EPS, w)
    pend, pend_buf = _padded(p.pend, dev)
    x_in = p.x_in.to(dev)
    pos, ln = torch.tensor([7], dtype=torch.int32, device=dev), torch.tensor([8], dtype=torch.int32, device=dev)
    run(x_in, nw, ep.EPS, w, pend=pend, advance=(pos, ln))
    assert int(pos.item()) == 8 and int(ln.item()) == 9, what + ": advance increments once"
    assert grid >= 8
    x_out = torch.full((R + 1, ep.SW_HIDDEN), S, device=dev)
    run(x_in, nw, ep.EPS, w, pend=pend, x_out=x_out)
    _equal(x_out[:R], p.target, what + " x_out")
    assert bool((x_out[R] == S).all()), what + ": wrote past the last row of x_out"
    assert int(pos.item()) == 8 and int(ln.item()) == 9
    _equal(pend_buf, _padded(p.pend, "cpu")[1], what + ": the pending accumulator is left as it is")


def test_sw_head_fewer_than_eight_workgroups(dev):
    """N = 7: seven workgroups cannot write x_out (refused); without x_out the launch is exact"""
    ops = _ops()
    from unigen_hip.lib import UniGenHipError
    R, N = 4, 7
    p = ep.problem(R, N, ep.SW_HIDDEN, "head")
    w, nw = ep.store(p.w, False, dev), p.norm_w.to(dev)
    pend, _ = _padded(p.pend, dev)
    logits = torch.full((R, N + 8), S, device=dev)
    with pytest.raises(UniGenHipError):
        ops.decode_sw_head_(p.x_in.to(dev), nw, ep.EPS, w, logits[:, :N], pend=pend, x_out=torch.empty(R, ep.SW_HIDDEN, device=dev))
    assert bool((logits == S).all())
    ops.decode_sw_head_(p.x_in.to(dev), nw, ep.EPS, w, logits[:, :N], pend=pend)
    ep.assert_exact(logits, N, p.logits, "decode_sw_head_ (4, 7) with the pending accumulator")
    logits.fill_(S)
    ops.decode_sw_head_(p.target.to(dev), nw, ep.EPS, w, logits[:, :N])
    ep.assert_exact(logits, N, p.logits, "decode_sw_head_ (4, 7)")


# ------------------------------------------------------------------------------------------------ 5. finishers
@pytest.mark.parametrize("cols", ep.FINISH_COLS)
def test_finishers(dev, cols):
    """ug_decode_finish_resid_norm / _ord: x += bf16round(acc | slot sum) is the target bit for bit, xn = s w bit for bit, the
    accumulator is zeroed (default form) / the slots are left (ordered form), the advance increments once.  cols <= 2048 run the
    8-vector instantiation, above it the 16-vector one: 4, 2048 | 2052, 4096 are their edges."""
    ops = _ops()
    for rows in ep.FINISH_ROWS:
        p = ep.problem(rows, cols, cols, "finish")
        what = f"finish_resid_norm {(rows, cols)}"
        w = p.norm_w.to(dev)
        acc, acc_buf = _padded(p.pend, dev)
        x, xn = p.x_in.clone().to(dev), torch.full((rows + 1, cols), S, dtype=BF, device=dev)
        pos, ln = torch.tensor([7], dtype=torch.int32, device=dev), torch.tensor([8], dtype=torch.int32, device=dev)
        ops.decode_finish_resid_norm_(acc, x, w, xn, ep.EPS, advance=(pos, ln))
        _equal(x, p.target, what + " x")
        _equal(xn[:rows], p.operand, what + " xn")
        assert bool((xn[rows] == S).all()), what + ": wrote past the last row of xn"
        assert float(acc.abs().max()) == 0.0 and bool((acc_buf[:, cols:] == S).all()), what + ": the accumulator is zeroed, its padding kept"
        assert int(pos.item()) == 8 and int(ln.item()) == 9
        parts, parts_buf = _padded(p.parts, dev)
        x, xn = p.x_in.clone().to(dev), torch.full((rows + 1, cols), S, dtype=BF, device=dev)
        ops.decode_finish_resid_norm_ord_(parts, x, w, xn, ep.EPS, advance=(pos, ln))
        _equal(x, p.target, what + " ordered x")
        _equal(xn[:rows], p.operand, what + " ordered xn")
        assert bool((xn[rows] == S).all()), what + ": ordered form wrote past the last row of xn"
        _equal(parts_buf, _padded(p.parts, "cpu")[1], what + ": the slots are inputs")
        assert int(pos.item()) == 9 and int(ln.item()) == 10
        x = p.x_in.clone().to(dev)
        ops.decode_finish_resid_norm_ord_(parts, x, w, None, ep.EPS)
        _equal(x, p.target, what + " ordered x without the norm output")


def test_finishers_refuse_more_than_4096_columns(dev):
    ops = _ops()
    from unigen_hip.lib import UniGenHipError
    cols = 4100
    acc, x, w = torch.zeros(1, cols, device=dev), torch.zeros(1, cols, device=dev), torch.ones(cols, device=dev)
    xn = torch.zeros(1, cols, dtype=BF, device=dev)
    with pytest.raises(UniGenHipError):
        ops.decode_finish_resid_norm_(acc, x, w, xn, ep.EPS)
    with pytest.raises(UniGenHipError):
        ops.decode_finish_resid_norm_ord_(acc.unsqueeze(0), x, w, xn, ep.EPS)
