"""Scoring a GIVEN continuation: Qwen2Engine.prefill_onto(hidden_at=...) / score_rows (engine) and UniGen.score (model).

Engine  the three-layer model of test_prefill_onto_gpu.py: asking prefill_onto for the last position of every row returns the bits
        of the row it returns anyway, and the default call returns what it returned before (a tensor, the same values).
Model   the tiny golden model (g2_tiny_unigen.pt), the prefix, tails and SEED of test_prefill_onto_gpu.py.  Oracle:
        oracle.qwen2_ref teacher-forced on the assembled rows [prefix | pads | context | targets[:-1]] under the dense mask of the
        same visibility, in fp32 and under bf16 autocast; token_logprobs at the real targets must pass helpers.fp32_yardstick (as
        close to the fp32 values as the oracle's own bf16 run is).
Bookkeeping  the continuation greedy mmu_generate_batch(prefix=...) emits has is_greedy True; with one token replaced by the
        oracle's second choice, False for that row only.  SEED was chosen on the CPU from the oracle alone (the rule and the seed of
        test_prefill_onto_gpu.py: oracle.qwen2_ref.mmu_generate_ref under bf16 autocast on the assembled rows; of seeds 0 .. 79 the
        first at which all three rows keep a top-2 margin >= 0.2 for all 8 steps; minima 0.23 / 0.46 / 0.62 under the prefix used
        here), so neither the emitted tokens nor the replaced one sit near a tie; the test asserts the condition.
Chunking  40 requests go through the call's 32-row chunks, 16 of them also alone: other rows change only the row-tile height of the
        head kernel and the row count of the backbone's launches.  Bar (set before any run): 1.5 x the error of the existing pair
        (logits_rows + ce_fwd(want_logp)) on the alone call's hidden rows against tests/head_score_ref.py, floor
        2^-22 max(1, |logprob|).
"""
import pytest
import torch

from head_score_ref import head_score_ref
from helpers import additive, fp32_yardstick
from test_prefill_onto_gpu import (ENGINE_CASES, LENS, MARGIN, NEW, PFX, S, _engine_inputs, _prefix_ids, _tails, m3, tiny)  # noqa: F401

pytestmark = pytest.mark.gpu

ROW_SPREAD, FLOOR = 1.5, 2.0 ** -22
# Continuation lengths of the three requests, right-padded to C = 400.  helpers.fp32_yardstick compares two error NORMS of equal
# expected size (two bf16 evaluations of one network) at a gate of 1.05; over n values each norm carries a sample spread of about
# 1 / sqrt(2 n), their ratio about 1 / sqrt(n).  A few dozen targets would leave that spread at 20 %, four times the gate's margin;
# 850 values bring it to 3.4 %, below it.  (The tiny model runs 410 positions in milliseconds.)
TARGET_LENS = (400, 150, 300)


# ====================================================================================== engine
def test_hidden_at_returns_the_rows_prefill_onto_returns_anyway(dev, m3):
    from unigen_hip.qwen2 import DecodeState
    model, _ = m3
    eng = model.llm.engine
    R, P, S_, = ENGINE_CASES["p61"][:3]
    prefix, tails, _, kv = _engine_inputs("p61")

    def fresh():
        st1 = DecodeState(eng.dims, 1, P, dev)
        eng.prefill(st1, prefix.to(dev), kv[:1, :P].to(dev))
        st = DecodeState(eng.dims, R, P + S_, dev, key_valid=kv)
        for l in range(eng.dims.num_hidden_layers):
            st.k[l][:, :, :P].copy_(st1.k[l])
            st.v[l][:, :, :P].copy_(st1.v[l])
        return st
    with torch.no_grad():
        plain = eng.prefill_onto(fresh(), tails.to(dev), P, kv.to(dev))
        assert torch.is_tensor(plain) and plain.shape == (R, 1536) and plain.dtype == torch.bfloat16      # the default: as before
        last = torch.arange(R) * S_ + (S_ - 1)
        at = torch.cat([last, torch.tensor([0, S_ - 2, R * S_ - 1])]).to(dev)
        out = eng.prefill_onto(fresh(), tails.to(dev), P, kv.to(dev), hidden_at=at)
        assert isinstance(out, tuple) and len(out) == 2
        hn, sel = out
        assert torch.equal(hn, plain)
        assert sel.shape == (R + 3, 1536) and sel.dtype == torch.bfloat16
        assert torch.equal(sel[:R], plain) and torch.equal(sel[R + 2], plain[R - 1])
        assert not torch.equal(sel[R], plain[0])                                                          # another position, another row
        logp, lse, best = eng.score_rows(sel, torch.zeros(R + 3, dtype=torch.int64, device=dev))
        # score_rows against the existing head on the same rows: the two round the same fp32 sums to bf16 behind different summation
        # orders, so a logit may differ by one bf16 step (2^-7 relative at most) and nothing else may
        logits = eng.logits_rows(sel)[:, :eng.dims.vocab_size].float()
        step = 2.0 ** -7 * logits.abs().max().item()
        assert (logits.max(dim=1).values - logits.gather(1, best[:, None])[:, 0]).abs().max().item() <= step
        assert (logp - torch.log_softmax(logits, dim=1)[:, 0]).abs().max().item() <= step + 1e-4
        assert (lse - torch.logsumexp(logits, dim=1)).abs().max().item() <= step + 1e-4
        eng.check_errors()


# ====================================================================================== model
def _requests(g):
    """contexts (left-padded tails of test_prefill_onto_gpu.py) and continuations [3, 400], right-padded with -100"""
    t, tv = _tails(g)
    gen = torch.Generator().manual_seed(77)
    targets = torch.full((len(LENS), max(TARGET_LENS)), -100, dtype=torch.long)
    for r, n in enumerate(TARGET_LENS):
        targets[r, :n] = torch.randint(0, 290, (n,), generator=gen)
    return t, tv, targets


def _assembled(g, pre, t, tv, targets):
    """rows [prefix | pads | context | targets[:-1] (pads as id 0)] and their dense masks: the prefix under its mmu mask (none: pre is
    empty), every later position causal over what the prefix mask's last row sees, the context's real tokens and the fed targets (a
    pad row attends to itself: no empty rows) -> (ids [R, L], allow [R, L, L], index of the position that predicts target 0)"""
    R, P = t.shape[0], pre.shape[0]
    fed = torch.where(targets == -100, torch.zeros_like(targets), targets)[:, :-1]
    ids = torch.cat([pre[None].expand(R, P), t, fed], 1)
    L = ids.shape[1]
    allow = torch.zeros(R, L, L, dtype=torch.bool)
    kv = torch.cat([torch.ones(R, P, dtype=torch.bool), tv, torch.ones_like(fed, dtype=torch.bool)], 1)
    if P:
        pre_allow = g["mask_allow"][-1, :P, :P]
        allow[:, :P, :P] = pre_allow
        kv[:, :P] = pre_allow[-1]
    allow[:, P:, :] = torch.tril(torch.ones(L, L, dtype=torch.bool))[P:][None] & kv[:, None, :]
    i = torch.arange(P, L)
    allow[:, i, i] = True
    return ids, allow, P + t.shape[1] - 1


def _oracle_token_logprobs(lm, ids, allow, first, targets, autocast):
    """teacher-forced log softmax at the targets, fp32 [R, C] (0.0 at pads), and the logits [R, C, V] of those positions"""
    from oracle import qwen2_ref
    C = targets.shape[1]
    with torch.no_grad(), qwen2_ref.autocast_ctx(autocast):
        logits = lm(ids, None, additive(allow))
    logits = logits[:, first:first + C].float()
    lp = torch.log_softmax(logits, dim=-1).gather(2, targets.clamp_min(0)[..., None])[..., 0]
    return torch.where(targets == -100, torch.zeros_like(lp), lp), logits


@pytest.mark.parametrize("with_prefix", [True, False])
def test_score_matches_the_teacher_forced_oracle(dev, tiny, with_prefix):
    model, lm, g = tiny
    t, tv, targets = _requests(g)
    pre = _prefix_ids(g, 0) if with_prefix else torch.zeros(0, dtype=torch.long)
    ids, allow, first = _assembled(g, pre, t, tv, targets)
    r32, _ = _oracle_token_logprobs(lm, ids, allow, first, targets, False)
    rbf, _ = _oracle_token_logprobs(lm, ids, allow, first, targets, True)
    prefix = None
    if with_prefix:
        pre_mask = additive(g["mask_allow"][-1:, :PFX, :PFX]).to(torch.float32).to(dev)
        prefix = model.mmu_prefix(idx=pre[None].to(dev), attention_mask=pre_mask)
        k0 = [k.clone() for k in prefix.st.k]
    sess = getattr(model.llm.engine, "_text_session", None)
    out = model.score(idx=t.to(dev), targets=targets.to(dev), prefix=prefix, tail_valid=tv.to(dev))
    assert type(out).__name__ == "ScoreResult" and out.token_logprobs.shape == targets.shape and out.logprob.shape == (3,)
    assert out.is_greedy.dtype == torch.bool and out.is_greedy.shape == (3,)
    got = out.token_logprobs.cpu()
    real = targets != -100
    assert (got[~real] == 0).all() and not torch.signbit(got[~real]).any() and (got[real] < 0).all()
    fp32_yardstick(f"score token_logprobs, prefix={with_prefix}", got[real], rbf[real], r32[real])
    assert torch.equal(out.logprob, out.token_logprobs.sum(dim=1))
    mean = model.score(idx=t.to(dev), targets=targets, prefix=prefix, tail_valid=tv.to(dev), average=True)      # (targets on the CPU: same call)
    assert torch.equal(mean.token_logprobs, out.token_logprobs) and torch.equal(mean.is_greedy, out.is_greedy)
    assert torch.equal(mean.logprob, out.token_logprobs.sum(dim=1) / torch.tensor(TARGET_LENS, dtype=torch.float32, device=dev))
    if with_prefix:                                                          # the prefix is the caller's: unchanged
        assert prefix.P == PFX and all(torch.equal(a, b) for a, b in zip(k0, prefix.st.k))
    assert getattr(model.llm.engine, "_text_session", None) is sess          # score keeps no session and touches none
    # embeddings instead of ids: the same rows
    emb = model.llm.model.embed_tokens(t.to(dev))
    again = model.score(input_embeddings=emb, targets=targets, prefix=prefix, tail_valid=tv.to(dev))
    assert torch.equal(again.token_logprobs, out.token_logprobs)


def test_is_greedy_follows_the_generated_continuation(dev, tiny):
    from oracle import qwen2_ref
    model, lm, g = tiny
    model.drop_decode_session()
    pre = _prefix_ids(g, 0)
    t, tv = _tails(g)
    pre_mask = additive(g["mask_allow"][-1:, :PFX, :PFX]).to(torch.float32).to(dev)
    prefix = model.mmu_prefix(idx=pre[None].to(dev), attention_mask=pre_mask)
    # the condition on SEED, from the oracle alone: every step of every row keeps a top-2 margin of at least MARGIN
    empty = torch.full((len(LENS), 1), -100, dtype=torch.long)
    ids0, allow0, _ = _assembled(g, pre, t, tv, empty)
    want, margins = [], []
    for r in range(len(LENS)):
        toks, m = qwen2_ref.mmu_generate_ref(lm, idx=ids0[r:r + 1], attention_mask=additive(allow0[r:r + 1]), max_new_tokens=NEW)
        want.append(toks)
        margins.append(min(m))
    print("    oracle top-2 margin minima per row:", [round(m, 2) for m in margins])
    assert min(margins) >= MARGIN, margins
    gen = model.mmu_generate_batch(idx=t.to(dev), prefix=prefix, tail_valid=tv.to(dev), max_new_tokens=NEW, temperature=0.0, on_device=False)
    model.drop_decode_session()
    targets = torch.tensor([[int(v) for v in row] for row in gen])
    assert targets.tolist() == want                                          # margins of 0.2: the HIP decode emits the oracle's tokens
    out = model.score(idx=t.to(dev), targets=targets, prefix=prefix, tail_valid=tv.to(dev))
    assert out.is_greedy.tolist() == [True, True, True]
    # row 1, step 3: the oracle's second choice there
    ids, allow, first = _assembled(g, pre, t, tv, targets)
    _, logits = _oracle_token_logprobs(lm, ids, allow, first, targets, True)
    top2 = logits[1, 3].topk(2).indices
    assert int(top2[0]) == int(targets[1, 3]) and float(logits[1, 3, top2[0]] - logits[1, 3, top2[1]]) >= MARGIN
    swapped = targets.clone()
    swapped[1, 3] = top2[1]
    out2 = model.score(idx=t.to(dev), targets=swapped, prefix=prefix, tail_valid=tv.to(dev))
    assert out2.is_greedy.tolist() == [True, False, True]
    assert torch.equal(out2.token_logprobs[[0, 2]], out.token_logprobs[[0, 2]])                  # the other rows: the same bits
    assert torch.equal(out2.token_logprobs[1, :3], out.token_logprobs[1, :3]) and float(out2.token_logprobs[1, 3]) < float(out.token_logprobs[1, 3])


def test_forty_requests_go_through_the_chunks(dev, tiny):
    from unigen_hip import ops
    model, _, g = tiny
    eng = model.llm.engine
    R, S_, C = 40, 6, 4
    gen = torch.Generator().manual_seed(40)
    idx = torch.randint(0, 290, (R, S_), generator=gen)
    targets = torch.randint(0, 290, (R, C), generator=gen)
    tv = torch.ones(R, S_, dtype=torch.bool)
    for r in range(R):
        tv[r, :r % 3] = False                                                # 0, 1 or 2 left pads
        if r % 4 == 1:
            targets[r, 2:] = -100
    alone = torch.arange(3, 35, 2)                                           # 16 rows from both sides of the 32-row boundary
    assert alone.numel() == 16 and int(alone.min()) < 32 <= int(alone.max())
    whole = model.score(idx=idx.to(dev), targets=targets, tail_valid=tv.to(dev))
    part = model.score(idx=idx[alone].to(dev), targets=targets[alone], tail_valid=tv[alone].to(dev))
    assert whole.logprob.shape == (R,) and torch.equal(whole.is_greedy[alone.to(dev)], part.is_greedy)
    # the existing pair's error on the alone call's hidden rows (recomputed here through the engine) against the fp64 restatement
    from unigen_hip.qwen2 import DecodeState
    with torch.no_grad():
        a = alone.to(dev)
        lab = torch.where(targets[alone] == -100, torch.zeros_like(targets[alone]), targets[alone])
        seq = torch.cat([model.llm.model.embed_tokens(idx[alone].to(dev)), model.llm.model.embed_tokens(lab[:, :-1].to(dev))], 1).float()
        L = S_ + C - 1
        kv = torch.cat([tv[alone], torch.ones(16, C - 1, dtype=torch.bool)], 1).to(dev)
        at = (torch.arange(16)[:, None] * L + (S_ - 1) + torch.arange(C)[None, :]).reshape(-1).to(dev)
        _, hn = eng.prefill_onto(DecodeState(eng.dims, 16, L, dev, key_valid=kv), seq, 0, kv, hidden_at=at)
        labels = targets[alone].reshape(-1)
        pair = ops.ce_fwd(eng.logits_rows(hn), eng.dims.vocab_size, labels.to(dev), want_logp=True)[3].view(16, C).sum(dim=1).cpu().double()
        o = head_score_ref(hn.cpu(), eng.fp.w("embed")[:eng.dims.vocab_size].cpu(), labels)
    oracle = o.logp.view(16, C).sum(dim=1)
    e_pair = (pair - oracle).abs().max().item()
    diff = (whole.logprob[a].cpu().double() - part.logprob.cpu().double()).abs()
    bar = torch.clamp(FLOOR * torch.clamp(part.logprob.cpu().double().abs(), min=1.0), min=ROW_SPREAD * e_pair)
    print(f"    40 vs 16 alone: max |d logprob| {diff.max().item():.3e}; existing pair against fp64 {e_pair:.3e}; "
          f"score against fp64 {(part.logprob.cpu().double() - oracle).abs().max().item():.3e}")
    assert (diff <= bar).all(), (diff.max().item(), e_pair)


def test_argument_errors_raise_before_any_launch(dev, tiny):
    from unigen_hip.lib import UniGenHipError
    from models import ScoreResult, UniGen                                   # noqa: F401  (exported)
    from oracle import weights                                                 # noqa: F401
    model, _, g = tiny
    t, tv, targets = _requests(g)
    emb = torch.zeros(3, S, model.llm.engine.dims.hidden_size, device=dev)
    with pytest.raises(UniGenHipError, match="one of the two"):
        model.score(idx=t.to(dev), input_embeddings=emb, targets=targets)
    with pytest.raises(UniGenHipError, match="one of the two"):
        model.score(targets=targets)
    bad = targets.clone()
    bad[1] = -100
    with pytest.raises(UniGenHipError, match="row 1 of targets has no real target"):
        model.score(idx=t.to(dev), targets=bad)
    with pytest.raises(UniGenHipError, match="RIGHT-padded"):
        model.score(idx=t.to(dev), targets=torch.tensor([[-100, 5]] * 3))
    with pytest.raises(UniGenHipError, match=r"must lie in \[0, "):
        model.score(idx=t.to(dev), targets=torch.full((3, 2), model.llm.engine.dims.vocab_size, dtype=torch.long))
    with pytest.raises(UniGenHipError, match="targets must be an int64"):
        model.score(idx=t.to(dev), targets=targets[:2])
    with pytest.raises(UniGenHipError, match="tail_valid must be"):
        model.score(idx=t.to(dev), targets=targets, tail_valid=tv[:, :5])
    with pytest.raises(UniGenHipError, match="prefix must be the object"):
        model.score(idx=t.to(dev), targets=targets, prefix=object())

    class _Other:                                                            # a prefix that belongs to another engine
        pass
    from models.unigen import MmuPrefix
    other = MmuPrefix.__new__(MmuPrefix)
    other.engine, other.device, other.P = _Other(), dev, 4
    with pytest.raises(UniGenHipError, match="built by another model"):
        model.score(idx=t.to(dev), targets=targets, prefix=other)
