"""ug_attn_decode_seq (csrc/decode.hip, attn_decode_seq_kernel): decode attention over S consecutive positions of ONE sequence, the
attention launch of a speculative verify step.  Against the fp64 restatement of test_decode_parity_gpu.py (_finish_ref / _attend_ref,
that file's BAR per (row, head)) with the causal staircase added -- row s sees the cache keys [0, p) that key_valid allows and the new
keys of rows 0 .. s -- and against S successive one-row ug_attn_decode_fused launches at p, p + 1, ...: the cache they leave is the cache
this launch leaves, byte for byte.  Also: the prefix property, stale cache contents, the end of the cache, the empty cache."""
import pytest
import torch

from test_decode_parity_gpu import BAR, BF, EPS, HD, NORM_COLS, _attend_ref, _finish_ref, _guarded, _head_err

pytestmark = pytest.mark.gpu

POS = (0, 63, 64, 511, 512, 700)          # the 64-key chunk edges, one pass of the four waves (256), several passes
ROWS = (1, 2, 8)
HEADS = ((12, 2), (4, 4))


class _Case:
    def __init__(self, p, S, heads, holes, dev, Tmax=None):
        from unigen_hip import ops
        self.p, self.S, (self.Hq, self.Hk), self.dev = p, S, heads, dev
        self.Tmax = Tmax = p + S + 5 if Tmax is None else Tmax
        Hq, Hk = heads
        g = torch.Generator().manual_seed(p * 100 + S * 10 + Hq + int(holes))
        nqkv = (Hq + 2 * Hk) * HD
        self.acc = 0.4 * torch.randn(S, nqkv, generator=g)
        self.ss = 100 + 50 * torch.rand(32, generator=g)
        self.bias = (0.1 * torch.randn(nqkv, generator=g)).to(BF)
        self.K = torch.randn(1, Hk, Tmax, HD, generator=g).to(BF)
        self.V = torch.randn(1, Hk, Tmax, HD, generator=g).to(BF)
        self.kv = None
        if holes:
            self.kv = torch.ones(1, Tmax, dtype=torch.uint8)
            self.kv[:, :p] = (torch.rand(1, p, generator=g) > 0.2).to(torch.uint8)        # holes in the prompt part only
        self.len = min(p, Tmax)
        self.vis = torch.ones(1, self.len, dtype=torch.bool) if self.kv is None else self.kv[:, :self.len].bool()
        self.cos_d, self.sin_d = ops.rope_tables(Tmax, HD, 1e6, dev)                       # max_pos = Tmax rows
        self.cos, self.sin = self.cos_d.cpu(), self.sin_d.cpu()
        # every row's q / k / v as the kernels build them (bf16 values): row s at table row min(p + s, max_pos - 1)
        rows = [_finish_ref(self.acc[s:s + 1], self.ss[s:s + 1], self.bias, self.cos, self.sin, min(p + s, Tmax - 1), Hq, Hk) for s in range(S)]
        self.q, self.kn, self.vn = (torch.cat([r[i] for r in rows]) for i in range(3))   # [S, heads, 128]

    def ref(self):
        """fp64 output [S, Hq, 128]: row s over the visible cache keys, the new keys 0 .. s - 1 (all visible) and its own"""
        out = []
        for s in range(self.S):
            K = torch.cat([self.K[:, :, :self.len].float(), self.kn[:s].transpose(0, 1)[None]], 2)
            V = torch.cat([self.V[:, :, :self.len].float(), self.vn[:s].transpose(0, 1)[None]], 2)
            vis = torch.cat([self.vis, torch.ones(1, s, dtype=torch.bool)], 1)
            out.append(_attend_ref(self.q[s:s + 1], self.kn[s:s + 1], self.vn[s:s + 1], K, V, vis))
        return torch.cat(out)

    def caches(self, nan_from=None):
        kb, kc = _guarded(self.K, self.dev)
        vb, vc = _guarded(self.V, self.dev)
        if nan_from is not None:
            kc[:, :, nan_from:] = float("nan")
            vc[:, :, nan_from:] = float("nan")
        return kb, vb, kc, vc

    def run_seq(self, rows=None, acc=None, nan_from=None):
        """one ug_attn_decode_seq launch on the first `rows` rows -> (o [rows, Hq * 128] on the host, the guarded K / V buffers after)"""
        from unigen_hip import ops
        rows = self.S if rows is None else rows
        acc = (self.acc if acc is None else acc)[:rows].contiguous().to(self.dev)
        kb, vb, kc, vc = self.caches(nan_from)
        ob, o = _guarded(torch.full((rows, self.Hq * HD), float("nan"), dtype=BF), self.dev)   # (every output element must be written)
        obefore = ob.clone()
        pos = torch.tensor([self.p], dtype=torch.int32, device=self.dev)
        kv = None if self.kv is None else self.kv.to(self.dev)
        ops.attn_decode_seq(acc, self.ss.to(self.dev), EPS, NORM_COLS, self.bias.to(self.dev), self.cos_d, self.sin_d, pos, kc, vc, kv, o,
                            self.Hq, self.Hk, HD, self.Tmax)
        torch.cuda.synchronize()
        assert torch.equal(ob[o.numel():].view(torch.int16), obefore[o.numel():].view(torch.int16)), "output guard written"
        return o.cpu(), (kb.cpu(), vb.cpu())

    def run_fused_steps(self):
        """S successive one-row ug_attn_decode_fused launches at p, p + 1, ... on one cache -> (o [S, Hq * 128], the buffers after)"""
        from unigen_hip import ops
        kb, vb, kc, vc = self.caches()
        o = torch.full((self.S, self.Hq * HD), float("nan"), dtype=BF, device=self.dev)
        kv = None if self.kv is None else self.kv.to(self.dev)
        bias = self.bias.to(self.dev)
        for s in range(self.S):
            pos = torch.tensor([self.p + s], dtype=torch.int32, device=self.dev)
            ss = torch.cat([self.ss[s:s + 1], self.ss[:31]]).to(self.dev)
            ops.attn_decode_fused(self.acc[s:s + 1].contiguous().to(self.dev), ss, EPS, NORM_COLS, bias, self.cos_d, self.sin_d, pos, kc, vc, kv,
                                  o[s:s + 1], self.Hq, self.Hk, HD, self.Tmax)
        torch.cuda.synchronize()
        return o.cpu(), (kb.cpu(), vb.cpu())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("holes", [False, True], ids=["nomask", "holes"])
@pytest.mark.parametrize("heads", HEADS, ids=["12x2", "4x4"])
@pytest.mark.parametrize("S", ROWS)
@pytest.mark.parametrize("p", POS)
def test_seq_attention_matches_fp64_and_successive_fused_launches(dev, p, S, heads, holes):
    c = _Case(p, S, heads, holes, dev)
    Hq, Hk, Tmax = c.Hq, c.Hk, c.Tmax
    ref = c.ref()
    o, (kb1, vb1) = c.run_seq()
    assert torch.isfinite(o.float()).all()
    err = _head_err(o, ref)
    assert float(err.max()) <= BAR, (f"worst (row, head) {divmod(int(err.argmax()), Hq)}", float(err.max()))
    # S one-row launches of the fused kernel: the same cache byte for byte (appended rows, everything else, the guard); o within the bar
    of, (kbf, vbf) = c.run_fused_steps()
    assert _same_bits(kb1, kbf) and _same_bits(vb1, vbf), "the cache differs from the one S successive fused launches leave"
    assert float(_head_err(of, ref).max()) <= BAR
    n = Hk * Tmax * HD
    for buf1, base, new in ((kb1, c.K, c.kn), (vb1, c.V, c.vn)):
        got = buf1[:n].view(1, Hk, Tmax, HD)
        assert _same_bits(buf1[n:], c.caches()[0].cpu()[n:]), "guard region written"
        assert _same_bits(got[0, :, :p], base[0, :, :p]) and _same_bits(got[0, :, p + S:], base[0, :, p + S:]), "cache bytes outside [p, p + S) changed"
        assert float((got[0, :, p:p + S].float() - new.transpose(0, 1)).abs().max()) <= 2.0 ** -6 * float(new.abs().max()), "appended rows"
    # stale cache: NaN at and past p before the launch reaches no output
    o_nan, _ = c.run_seq(nan_from=p)
    assert torch.isfinite(o_nan.float()).all() and _same_bits(o_nan, o), "cache contents at or past p reached the output"
    # the prefix property, also under huge and NaN accumulators in the rows behind the prefix
    for s in sorted({0, S // 2, S - 2} & set(range(S - 1))):
        head, _ = c.run_seq(rows=s + 1)
        assert _same_bits(head, o[:s + 1]), ("prefix", s)
        for bad in (float("nan"), 3e37):
            acc = c.acc.clone()
            acc[s + 1:] = bad
            poisoned, _ = c.run_seq(acc=acc)
            assert _same_bits(poisoned[:s + 1], o[:s + 1]), ("prefix under poisoned rows", s, bad)
    if p == 0:                                          # empty cache: row 0 sees its own key alone
        want = c.vn[0].repeat_interleave(Hq // Hk, 0).reshape(Hq * HD).to(BF)
        assert torch.equal(o[0], want)


@pytest.mark.parametrize("p,S,short", [(63, 2, 1), (63, 8, 3), (700, 8, 8), (512, 8, 1), (5, 1, 1)])
def test_rows_at_or_past_the_cache_end_write_nothing(dev, p, S, short):
    """Tmax = p + S - short: the last `short` rows sit at or past Tmax (short == S: p == Tmax, the cache is full).  They still attend
    -- to the cache and to the step's earlier rows, from the accumulator -- but append nothing; RoPE clamps to the table's last row."""
    c = _Case(p, S, (12, 2), False, dev, Tmax=p + S - short)
    Tmax, Hk = c.Tmax, c.Hk
    o, (kb1, vb1) = c.run_seq()
    assert float(_head_err(o, c.ref()).max()) <= BAR
    kb0, vb0, _, _ = c.caches()
    n = Hk * Tmax * HD
    for buf0, buf1, new in ((kb0.cpu(), kb1, c.kn), (vb0.cpu(), vb1, c.vn)):
        got = buf1[:n].view(1, Hk, Tmax, HD)[0, :, p:]
        expect = buf0.clone()
        expect[:n].view(1, Hk, Tmax, HD)[0, :, p:] = got                        # (Tmax - p rows, S - short of them)
        assert got.shape[1] == S - short
        assert _same_bits(buf1, expect), "a row at or past Tmax wrote to the cache or the guard"
        if S > short:
            assert float((got.float() - new[:S - short].transpose(0, 1)).abs().max()) <= 2.0 ** -6 * float(new.abs().max())


def test_argument_checks(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    c = _Case(8, 2, (4, 4), False, dev)
    _, _, kc, vc = c.caches()
    pos = torch.tensor([8], dtype=torch.int32, device=dev)

    def launch(acc, k=kc, v=vc):
        o = torch.empty((acc.shape[0], 4 * HD), dtype=BF, device=dev)
        ops.attn_decode_seq(acc.to(dev), c.ss.to(dev), EPS, NORM_COLS, c.bias.to(dev), c.cos_d, c.sin_d, pos, k, v, None, o, 4, 4, HD, c.Tmax)
    with pytest.raises(UniGenHipError, match="rows"):
        launch(torch.zeros(9, c.acc.shape[1]))                                  # more than UG_SPEC_MAX_ROWS positions
    with pytest.raises(UniGenHipError, match="ONE sequence"):
        launch(c.acc, k=kc.repeat(2, 1, 1, 1), v=vc.repeat(2, 1, 1, 1))
