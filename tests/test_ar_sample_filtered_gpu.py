"""ug_ar_sample_filtered (csrc/sampler.hip: ar_sample_filtered_kernel) through ops.ar_sample_filtered_: the kept set and the draw
of every step against the float64 restatement in truncation_ref.py.

Inputs are flat on purpose (0.5 * randn, guidance scale 2, temperature 0.8): truncation then changes most draws, so the unfiltered
sampler fails this test.  Scale 2 is a power of two, so the mixed logit is exact in fp32 and the test reproduces it bit for bit.
Acceptance per draw, no excluded rows (D = 1e-5, truncation_ref.D): the threshold the kernel reports lies in the float64 bracket,
the reported count is the size of {v >= tau}, the token is in that set and is a legitimate inverse-CDF draw over it."""
import pytest
import torch

import truncation_ref as ref

pytestmark = pytest.mark.gpu

SETTINGS = [(50, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (200, 0.8, 0.02), (1, 1.0, 0.0), (0, 0.5, 0.0), (1000, 0.95, 0.0)]
SCALE, TEMP = 2.0, 0.8


@pytest.mark.parametrize("V", [8192, 5000])
@pytest.mark.parametrize("case", range(len(SETTINGS)))
def test_ar_sample_filtered_kernel_matches_restatement(dev, V, case):
    from unigen_hip import ops
    top_k, top_p, min_p = SETTINGS[case]
    bsz, H, n, P, off = 6, 256, 10, 40, 100
    g = torch.Generator().manual_seed(100 + case)
    acc = 0.5 * torch.randn(2 * bsz, V, generator=g)
    emb = torch.randn(off + V, H, generator=g)
    u = torch.rand(n, bsz, generator=g)
    u[0, 0] = 0.0
    u[1, 0] = 1.0 - 2.0 ** -24
    v32 = ref.mixed_logits(acc, bsz, SCALE, TEMP)
    v = v32.double()
    brackets = [ref.tau_bracket(v[b], top_k, top_p, min_p) for b in range(bsz)]
    emb_d, u_d = emb.to(dev), u.to(dev)
    for step in range(n):
        pos = torch.tensor([P + step], dtype=torch.int32).to(dev)
        res = []
        for _ in range(2):
            tok = torch.zeros(bsz, 1, dtype=torch.long, device=dev)
            out = torch.zeros(bsz, n, dtype=torch.int32, device=dev)
            x = torch.zeros(2 * bsz, H, device=dev)
            stats = torch.full((bsz, 2), -1.0, device=dev)
            acc_d = acc.clone().to(dev)
            ops.ar_sample_filtered_(acc_d, bsz, V, SCALE, TEMP, False, u_d, pos, P, n, emb_d, off, tok, out, x,
                                    top_k=top_k, top_p=top_p, min_p=min_p, stats=stats)
            res.append((tok.cpu(), x.cpu(), stats.cpu(), out.cpu(), float(acc_d.abs().max())))
        (tok, x, stats, out, acc_max), again = res
        assert torch.equal(tok, again[0]) and torch.equal(x, again[1]) and torch.equal(stats, again[2])      # bit-reproducible
        got = tok[:, 0]
        for b in range(bsz):
            t, cnt, lo_hi = float(stats[b, 0]), int(stats[b, 1]), brackets[b]
            print(f"case {case} V {V} step {step} row {b}: tau {t!r} in [{lo_hi[0]!r}, {lo_hi[1]!r}], kept {cnt}, token {int(got[b])}, u {float(u[step, b])!r}")
            assert lo_hi[0] <= t <= lo_hi[1], (case, V, step, b, t, lo_hi)
            assert cnt == int((v[b] >= t).sum()) and cnt >= 1, (case, V, step, b, cnt)
            assert 0 <= int(got[b]) < V and bool(v[b][got[b]] >= t), (case, V, step, b)
            assert ref.draw_ok(v[b], t, int(got[b]), u[step, b].double()), (case, V, step, b, int(got[b]))
        assert torch.equal(out[:, step].long(), got) and int(out.abs().sum()) == int(got.sum())       # written at this step only
        assert torch.equal(x[:bsz], emb[got + off]) and torch.equal(x[bsz:], emb[got + off])
        assert acc_max == 0.0


def test_ar_sample_filtered_rejects_bad_filters(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    bsz, V, H, n, P = 2, 64, 256, 4, 8
    acc = torch.zeros(2 * bsz, V, device=dev)
    emb = torch.zeros(V, H, device=dev)
    u = torch.zeros(n, bsz, device=dev)
    pos = torch.tensor([P], dtype=torch.int32, device=dev)
    tok = torch.zeros(bsz, 1, dtype=torch.long, device=dev)
    out = torch.zeros(bsz, n, dtype=torch.int32, device=dev)
    x = torch.zeros(2 * bsz, H, device=dev)
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": -0.1}, {"min_p": 1.5}, {"top_k": -1}):
        with pytest.raises(UniGenHipError):
            ops.ar_sample_filtered_(acc, bsz, V, 1.0, 1.0, False, u, pos, P, n, emb, 0, tok, out, x, **kw)
