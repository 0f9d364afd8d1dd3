"""ug_text_pick (csrc/text_sampler.hip: text_pick_kernel) through ops.text_pick_: exact.  The greedy token over the whole vocabulary
(bf16-rounded values, lowest index on ties, padding never a candidate), what is and is not written, and a 12-step sequence of the
stop rule against its Python restatement (text_pick_ref.StopRule)."""
import pytest
import torch

from text_pick_ref import StopRule

pytestmark = pytest.mark.gpu

H = 64


def _state_of(state, R):
    s = state.cpu().tolist()
    return {"step": s[0], "remaining": s[1], "steps_used": s[2], "ticket": s[3], "done": s[4:4 + R]}


def _first_argmax(b):
    """lowest index attaining the row maximum, spelled out (no reliance on a library's tie rule)"""
    idx = torch.arange(b.shape[1], device=b.device).expand_as(b)
    return torch.where(b == b.max(-1, keepdim=True).values, idx, b.shape[1]).min(-1).values


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("R", [1, 5, 16, 32])
@pytest.mark.parametrize("V", [159867, 65537, 4097, 1000, 1])
def test_text_pick_is_the_lowest_argmax_of_the_bf16_values(dev, V, R, clear):
    from unigen_hip import ops
    ld = ops.round_up(V, 8)
    g = torch.Generator(device=dev).manual_seed(V + R)
    full = torch.full((R + 1, ld), 1e30, device=dev)                 # (a guard row behind the last one)
    full[:R, :V] = torch.randn(R, V, device=dev, generator=g)
    want_planted = {}
    for r in range(R):
        kind = r % 4
        if kind == 1 and V > 4096:                                   # the maximum three times: 4 095, 4 096 and V - 1
            full[r, 4095] = full[r, 4096] = full[r, V - 1] = 7.0
            want_planted[r] = 4095
        elif kind == 2 and V >= 1000:                                # equal after the bf16 rounding, the larger fp32 value behind
            full[r, V // 3] = 6.0
            full[r, V - 1] = 6.0 + 2.0 ** -10
            want_planted[r] = V // 3
        elif kind == 3 and V > 1:                                    # the maximum twice, the second time in the last column
            full[r, V - 2] = full[r, V - 1] = 7.5
            want_planted[r] = V - 2
    before = full.clone()
    emb = torch.randn(V, H, device=dev, generator=g)
    state = ops.text_state(R, dev)
    tok = torch.full((R,), -1, dtype=torch.long, device=dev)
    out = torch.full((R, 3), -1, dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    ops.text_pick_(full[:R], V, state, 3, emb, tok, out, x, clear=clear)
    want = _first_argmax(before[:R, :V].bfloat16().float())
    for r, w in want_planted.items():
        assert int(want[r]) == w, (r, int(want[r]), w)
    assert torch.equal(tok, want), (tok.tolist(), want.tolist())
    assert torch.equal(out[:, 0].long(), want) and bool((out[:, 1:] == -1).all())
    assert torch.equal(x, emb[want])
    assert torch.equal(full[:, V:], before[:, V:]) and torch.equal(full[R], before[R])            # padding and guard row untouched
    assert torch.equal(full[:R, :V], torch.zeros_like(full[:R, :V]) if clear else before[:R, :V])
    assert _state_of(state, R) == {"step": 1, "remaining": R, "steps_used": 0, "ticket": 0, "done": [0] * R}


@pytest.mark.parametrize("clear", [False, True])
def test_text_pick_takes_rows_off_sixteen_byte_boundaries(dev, clear):
    """ld = V odd (the contiguous [R, V] buffer the ordered head writes): the scalar form of the kernel"""
    from unigen_hip import ops
    R, V = 3, 4099
    g = torch.Generator(device=dev).manual_seed(1)
    lg = torch.randn(R + 1, V, device=dev, generator=g)
    lg[1, 4095] = lg[1, 4096] = lg[1, V - 1] = 7.0
    before = lg.clone()
    emb = torch.randn(V, H, device=dev, generator=g)
    state = ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, 2), dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    ops.text_pick_(lg[:R], V, state, 2, emb, tok, out, x, clear=clear)
    want = _first_argmax(before[:R].bfloat16().float())
    assert int(want[1]) == 4095 and torch.equal(tok, want) and torch.equal(x, emb[want]) and torch.equal(lg[R], before[R])
    assert torch.equal(lg[:R], torch.zeros_like(lg[:R]) if clear else before[:R])


@pytest.mark.parametrize("stops", [(7, 11), ()])
def test_text_pick_stop_rule_over_twelve_steps(dev, stops):
    """Rows finish at different steps (one on the first token, two on the same step, one on the second stop id, one never); a
    finished row emits pad_id whatever its logits say; without stop ids nothing ever finishes."""
    from unigen_hip import ops
    R, V, n, pad = 5, 1000, 12, 3
    ld = ops.round_up(V, 8)
    g = torch.Generator().manual_seed(5)
    script = torch.randint(20, V, (n, R), generator=g)               # raw picks: no stop id among them ...
    script[0, 0] = 7                                                 # ... except where a row is to finish
    script[4, 1] = 11
    script[4, 2] = 7
    script[9, 3] = 11
    script[6, 0] = 11                                                # (a stop id on a finished row's logits: it emits pad_id)
    emb = torch.randn(V, H, generator=g).to(dev)
    state = ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, n), dtype=torch.int32, device=dev)
    lengths = torch.full((R,), n, dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    stop_ids = torch.tensor(stops, dtype=torch.long, device=dev) if stops else None
    rule = StopRule(R, n, stops, pad if stops else None)
    for i in range(n):
        lg = torch.full((R, ld), 1e30)
        lg[:, :V] = 0.1 * torch.randn(R, V, generator=g)
        lg[torch.arange(R), script[i]] = 4.0
        lg = lg.to(dev)
        ops.text_pick_(lg, V, state, n, emb, tok, out, x, clear=bool(i & 1), stop_ids=stop_ids, pad_id=pad if stops else None, lengths=lengths)
        fed = rule.emit(script[i].tolist())
        assert tok.tolist() == fed, (i, tok.tolist(), fed)
        assert torch.equal(x.cpu(), emb.cpu()[torch.tensor(fed)])
        s = _state_of(state, R)
        assert s == {"step": rule.step, "remaining": rule.remaining, "steps_used": rule.steps_used, "ticket": 0, "done": rule.done}, (i, s)
        assert lengths.tolist() == rule.lengths
    assert out.tolist() == rule.out
    if stops:
        assert rule.done == [1, 1, 1, 1, 0] and rule.lengths == [1, 5, 5, 10, 12] and rule.steps_used == 0 and rule.remaining == 1
    else:
        assert rule.done == [0] * R and rule.remaining == R


def test_text_pick_reports_the_step_at_which_every_row_had_finished(dev):
    from unigen_hip import ops
    R, V, n = 3, 40, 6
    emb = torch.zeros(V, H, device=dev)
    state = ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, n), dtype=torch.int32, device=dev)
    lengths = torch.full((R,), n, dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    stop_ids = torch.tensor([9], dtype=torch.long, device=dev)
    rule = StopRule(R, n, [9], 9)
    picks = [[1, 9, 2], [3, 4, 5], [9, 6, 9], [7, 7, 7]]
    for i, p in enumerate(picks):
        lg = torch.zeros(R, V)
        lg[torch.arange(R), torch.tensor(p)] = 1.0
        ops.text_pick_(lg.to(dev), V, state, n, emb, tok, out, x, stop_ids=stop_ids, pad_id=9, lengths=lengths)
        assert tok.tolist() == rule.emit(p)
    s = _state_of(state, R)
    assert s["steps_used"] == rule.steps_used == 3 and s["remaining"] == 0 and s["step"] == 4
    assert lengths.tolist() == rule.lengths == [3, 1, 3] and out.tolist() == rule.out
    ops.text_state_reset_(state, R)
    assert _state_of(state, R) == {"step": 0, "remaining": R, "steps_used": 0, "ticket": 0, "done": [0] * R}


def test_text_pick_refuses_bad_arguments(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    V = 64
    emb = torch.zeros(V, H, device=dev)
    tok = torch.zeros(33, dtype=torch.long, device=dev)
    out = torch.zeros((33, 2), dtype=torch.int32, device=dev)
    x = torch.zeros(33, H, device=dev)
    state = ops.text_state(32, dev)
    with pytest.raises(UniGenHipError):                              # 33 rows
        ops.text_pick_(torch.zeros(33, V, device=dev), V, state, 2, emb, tok, out, x)
    with pytest.raises(UniGenHipError):                              # V beyond the row
        ops.text_pick_(torch.zeros(2, V, device=dev), V + 1, state, 2, emb, tok, out, x)
    with pytest.raises(UniGenHipError):                              # a pad id outside the table
        ops.text_pick_(torch.zeros(2, V, device=dev), V, state, 2, emb, tok, out, x, pad_id=V)
    with pytest.raises(UniGenHipError):                              # nine stop ids
        ops.text_pick_(torch.zeros(2, V, device=dev), V, state, 2, emb, tok, out, x, stop_ids=torch.zeros(9, dtype=torch.long, device=dev))
