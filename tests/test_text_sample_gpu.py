"""ug_text_sample (csrc/text_sampler.hip: histogram, selection, locate) through ops.text_sample_: the kept set and the draw of every
step against the float64 restatements (truncation_ref.py for the kept set, text_pick_ref.sorted_draw_ok for the draw in
value-descending order), plus the CPU test that pins those helpers against truncation_ref on rows with heavy ties.

Tolerance d = truncation_ref.D = 1e-5.  The kernel's running mass of a key is a serial sum of at most 64 bin masses in key order,
under a 6-level wave scan, under a 4-level scan of the 16 wave totals: at most 64 + 6 + 4 = 74 roundings; a bin mass itself is
float(count) * expf(v - max) (one rounding each for the product and the difference's exponent argument -- |v - max| < 8 here, so the
difference is off by at most 2^-22 -- and ~1 ulp of expf).  Worst case (74 + 3) * 2^-24 + 2^-22 = 4.8e-6, below D / 2."""
import pytest
import torch

import truncation_ref as ref
from text_pick_ref import sorted_draw_ok, sorted_draw_terms

SETTINGS = [(50, 1.0), (0, 0.9), (200, 0.8), (1, 1.0), (0, 0.5), (1000, 0.95)]
TEMP = 0.8


def _v32(logits):
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(TEMP, dtype=torch.float32)
    return logits.float().to(torch.bfloat16).float() * inv_t


@pytest.mark.gpu
@pytest.mark.parametrize("V", [159867, 5000])
@pytest.mark.parametrize("case", range(len(SETTINGS)))
def test_text_sample_kernel_matches_restatement(dev, V, case):
    from unigen_hip import ops
    top_k, top_p = SETTINGS[case]
    R, H, n = 6, 64, 5
    ld = ops.round_up(V, 8)
    g = torch.Generator().manual_seed(200 + case)
    logits = torch.full((R, ld), 1e30)
    logits[:, :V] = 0.5 * torch.randn(R, V, generator=g)
    emb = torch.randn(V, H, generator=g)
    u = torch.rand(n, R, generator=g)
    u[0, 0] = 0.0
    u[1, 0] = 1.0 - 2.0 ** -24
    u[2, 1] = 0.0
    u[3, 2] = 1.0 - 2.0 ** -24
    v = _v32(logits[:, :V]).double()
    brackets = [ref.tau_bracket(v[b], top_k, top_p) for b in range(R)]
    emb_d, u_d = emb.to(dev), u.to(dev)
    runs = []
    for _ in range(2):
        ws = ops.text_sample_workspace(R, dev)
        state = ops.text_state(R, dev)
        tok = torch.zeros(R, dtype=torch.long, device=dev)
        out = torch.full((R, n), -1, dtype=torch.int32, device=dev)
        x = torch.zeros(R, H, device=dev)
        steps = []
        for step in range(n):
            clear = step == n - 1
            lg = logits.to(dev)
            stats = torch.full((R, 2), -1.0, device=dev)
            ops.text_sample_(lg, V, state, n, emb_d, tok, out, x, u_d, ws, temperature=TEMP, top_k=top_k, top_p=top_p, clear=clear, stats=stats)
            assert int(ws.abs().max()) == 0                               # the workspace is all zero after every step
            assert torch.equal(lg[:, V:].cpu(), logits[:, V:])
            assert torch.equal(lg[:, :V].cpu(), torch.zeros(R, V) if clear else logits[:, :V])
            steps.append((tok.cpu().clone(), x.cpu().clone(), stats.cpu()))
        runs.append((steps, out.cpu(), state.cpu()))
    (steps, out, state), again = runs
    assert torch.equal(out, again[1]) and torch.equal(state, again[2])
    assert state[:4].tolist() == [n, R, 0, 0]
    for step in range(n):
        tok, x, stats = steps[step]
        assert all(torch.equal(a, b) for a, b in zip(steps[step], again[0][step]))                # bit-reproducible
        for b in range(R):
            t, cnt, lo_hi, got = float(stats[b, 0]), int(stats[b, 1]), brackets[b], int(tok[b])
            above, j, e, T = sorted_draw_terms(v[b], t, got)
            print(f"case {case} V {V} step {step} row {b}: tau {t!r} in [{lo_hi[0]!r}, {lo_hi[1]!r}], kept {cnt}, token {got}, u {float(u[step, b])!r}, "
                  f"u*T {float(u[step, b]) * T!r} in [{above + j * e!r}, {above + (j + 1) * e!r})")
            assert lo_hi[0] <= t <= lo_hi[1], (case, V, step, b, t, lo_hi)
            assert cnt == int((v[b] >= t).sum()) and cnt >= 1, (case, V, step, b, cnt)
            assert 0 <= got < V and bool(v[b][got] >= t), (case, V, step, b)
            assert sorted_draw_ok(v[b], t, got, u[step, b].double()), (case, V, step, b, got)
        assert torch.equal(out[:, step].long(), tok)
        assert torch.equal(x, emb[tok])


@pytest.mark.gpu
def test_text_sample_applies_the_stop_rule_and_top_k_one_is_greedy(dev):
    from unigen_hip import ops
    R, V, H, n = 4, 3000, 64, 3
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(R, ops.round_up(V, 8), generator=g)
    want = torch.tensor([5, 77, 77, V - 1])
    logits[torch.arange(R), want] = 9.0                               # a unique maximum per row: top_k = 1 keeps it alone
    logits, want = logits.to(dev), want.to(dev)
    emb = torch.randn(V, H, generator=g).to(dev)
    stop = want[1:2].clone()                                          # rows 1 and 2 pick the stop id
    ws, state = ops.text_sample_workspace(R, dev), ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, n), dtype=torch.int32, device=dev)
    lengths = torch.full((R,), n, dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    u = torch.rand(n, R, generator=g).to(dev)
    for _ in range(2):
        ops.text_sample_(logits, V, state, n, emb, tok, out, x, u, ws, temperature=0.7, top_k=1, stop_ids=stop, pad_id=5, lengths=lengths)
    hit = want == stop
    assert torch.equal(out[:, 0].long(), want)
    assert torch.equal(out[:, 1].long(), torch.where(hit, torch.full_like(want, 5), want))
    assert torch.equal(lengths.long(), torch.where(hit, torch.ones_like(want), torch.full_like(want, n)))
    assert state[:3].tolist() == [2, R - int(hit.sum()), 0] and state[4:4 + R].tolist() == hit.int().tolist()


@pytest.mark.gpu
def test_text_sample_rejects_bad_filters(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    R, V, H, n = 2, 64, 64, 4
    logits = torch.zeros(R, V, device=dev)
    emb = torch.zeros(V, H, device=dev)
    ws, state = ops.text_sample_workspace(R, dev), ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, n), dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    u = torch.zeros(n, R, device=dev)
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"top_k": -1}, {"temperature": 0.0}, {"temperature": -1.0}):
        with pytest.raises(UniGenHipError):
            ops.text_sample_(logits, V, state, n, emb, tok, out, x, u, ws, **kw)
    with pytest.raises(UniGenHipError):
        ops.text_sample_workspace(33, dev)
    assert int(state[0]) == 0 and int(ws.abs().max()) == 0           # a refused call launches nothing


def test_sorted_draw_and_stop_rule_helpers_on_heavy_ties():
    """CPU: the yardsticks themselves.  (1) On a row sorted by value descending the sorted order IS the index order, so the new check
    must agree with truncation_ref.draw_ok for every token and uniform tried.  (2) On quantised rows (long runs of equal values) the
    token an exact float64 inverse CDF over the explicitly sorted kept entries draws passes, its neighbours in that order fail once u
    is moved to the middle of the drawn token's interval, and a dropped token never passes.  (3) StopRule against emit_until_stop."""
    from models.unigen import emit_until_stop
    g = torch.Generator().manual_seed(11)
    V = 600
    rows = 0.5 * torch.randn(4, V, generator=g, dtype=torch.float64) * 1.25
    rows[1:] = (rows[1:] * 8).round() / 8
    for top_k, top_p in [(0, 1.0), (50, 1.0), (0, 0.9), (200, 0.8), (1, 1.0)]:
        for b in range(4):
            v = rows[b]
            t = ref.tau(v, top_k, top_p)
            order = sorted(range(V), key=lambda i: (-float(v[i]), i))
            kept = [i for i in order if float(v[i]) >= t]
            ex = torch.exp(v - v.max())
            cum = torch.cumsum(ex[kept], 0)
            T = float(cum[-1])
            assert abs(T - sorted_draw_terms(v, t, kept[0])[3]) <= 1e-12 * T
            for u in (0.0, 0.13, 0.5, 0.77, 1.0 - 2.0 ** -24):
                pos = int((cum > u * T).nonzero()[0])
                assert sorted_draw_ok(v, t, kept[pos], u, d=1e-12), (top_k, top_p, b, u)
                mid = (float(cum[pos]) - 0.5 * float(ex[kept[pos]])) / T
                assert sorted_draw_ok(v, t, kept[pos], mid, d=1e-12)
                for other in (pos - 1, pos + 1):
                    if 0 <= other < len(kept):
                        assert not sorted_draw_ok(v, t, kept[other], mid, d=1e-12), (top_k, top_p, b, u, other)
            if len(kept) < V:
                assert not sorted_draw_ok(v, t, order[len(kept)], 0.5)
            # sorted by value, descending: both checks describe the same order
            vs = v[order]
            for u in (0.0, 0.3, 0.9):
                for tokn in (0, 1, len(kept) // 2, len(kept) - 1, min(V - 1, len(kept))):
                    assert sorted_draw_ok(vs, t, tokn, u) == ref.draw_ok(vs, t, tokn, torch.tensor(u, dtype=torch.float64)), (top_k, top_p, b, u, tokn)
    # the stop rule
    from text_pick_ref import StopRule
    R, n = 4, 7
    picks = torch.randint(0, 6, (n, R), generator=g)
    for stops, pad, with_len in [((2, 4), 1, True), ((3,), None, True), ((), None, False)]:
        out = torch.zeros((R, n), dtype=torch.long)
        lengths = torch.full((R,), n, dtype=torch.long)
        stop = torch.tensor(stops) if stops else None
        emit = emit_until_stop(out, stop, pad, lengths=lengths if with_len else None)
        rule = StopRule(R, n, stops, pad if stops else None)
        for i in range(n):
            fed, all_done = emit(i, picks[i][:, None].clone())
            assert fed[:, 0].tolist() == rule.emit(picks[i].tolist())
            assert bool(all_done) == (rule.remaining == 0 and bool(stops))
        assert out.tolist() == rule.out
        if with_len:
            assert lengths.tolist() == rule.lengths
