"""The on-device text loop (UniGen._decode_text_on_device behind generate / mmu_generate / mmu_generate_batch with on_device=True;
Qwen2Engine.text_step): eager, captured and reused-session runs agree bit for bit in deterministic mode; the engine step, fed the
host loop's own tokens, picks the host loop's token wherever the step's top-2 margin clears the two heads' rounding; the stop rule,
the polling, sampling, eligibility and the session's life.

Fixtures: the 1.5B-width two-layer model of test_decode_step_forms_agree_at_1p5b_width (vocab 4 096, synth_llm_state seed 17) and the
H = 256 model of the deterministic decode tests (golden G9's config) for the wide forms."""
import pytest
import torch

from helpers import additive, golden, llm_config_dir
from text_pick_ref import StopRule

pytestmark = pytest.mark.gpu

MARGIN = 0.05          # the bar of test_generate_gpu.py: a top-2 margin below it may fall either way between two bf16 heads


@pytest.fixture(scope="module")
def m1p5(dev):
    from models import UniGen
    from oracle import qwen2_ref, weights
    cfg = dict(qwen2_ref.QWEN25_1P5B, num_hidden_layers=2, vocab_size=4096)
    model = UniGen(w_und_encoder=False, vocab_size=4096, llm_vocab_size=2048, llm_model_path=llm_config_dir(cfg), codebook_size=2047,
                   num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=-1).eval()
    names = [(n, tuple(p.shape)) for n, p in model.llm.named_parameters()]
    model.llm.load_state_dict(weights.synth_llm_state(names, seed=17), strict=False)
    return model


def _small_model(dev):
    from models import UniGen
    from oracle import weights
    g = golden("g9_generate.pt")
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=g["weight_std"]), strict=False)
    return m.eval()


@pytest.fixture(scope="module")
def msmall(dev):
    return _small_model(dev)


def _prompts(dev, lens=(40, 27, 33), hi=2000, seed=4, repeat=1):
    """left-padded rows -> (ids [R, L], attention mask [R, L], dense additive mmu masks [R, 1, L, L])"""
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.zeros((len(lens), L), dtype=torch.long)
    am = torch.zeros((len(lens), L), dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, L - n:] = torch.randint(1, hi, (n,), generator=g)
        am[r, L - n:] = 1
    ids, am = ids.repeat(repeat, 1), am.repeat(repeat, 1)
    allow = (torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & am.bool()[:, None, :]) | torch.eye(L, dtype=torch.bool)[None]
    return ids.to(dev), am.to(dev), additive(allow).reshape(len(lens) * repeat, 1, L, L).to(dev)


def _lists(rows):
    return [[int(t) for t in r] for r in rows]


# ------------------------------------------------------------------ deterministic mode: eager == captured == reused session
@pytest.mark.parametrize("which", ["m1p5", "msmall"])
def test_on_device_runs_agree_bit_for_bit_in_deterministic_mode(dev, request, which):
    model = request.getfixturevalue(which)
    eng = model.llm.engine
    hi = 2000 if which == "m1p5" else 300
    ids, am, mm = _prompts(dev, hi=hi)
    n = 12
    model.drop_decode_session()
    assert eng.decode_form(3, True) == ("ord_sw" if which == "m1p5" else "ord_wide")
    kw = dict(attention_mask=am, max_new_tokens=n, deterministic=True, on_device=True)
    free = model.generate(input_ids=ids, use_graph=False, **kw)[:, ids.shape[1]:]
    assert eng.last_text_decode_on_device and not eng.last_decode_graph and eng._text_session is None
    eos, pad = int(free[0, 3]), 0                                      # (a stop id taken from the run itself)
    c0 = getattr(eng, "text_graph_captures", 0)
    eager = model.generate(input_ids=ids, eos_token_id=eos, pad_token_id=pad, use_graph=False, **kw)
    captured = model.generate(input_ids=ids, eos_token_id=eos, pad_token_id=pad, **kw)
    assert eng.last_decode_graph and eng.text_graph_captures == c0 + 1
    sess = eng._text_session
    assert sess is not None and sess.st.deterministic
    kept = model.generate(input_ids=ids, eos_token_id=eos, pad_token_id=pad, **kw)
    assert eng._text_session is sess and eng.text_graph_captures == c0 + 1
    assert torch.equal(eager, captured) and torch.equal(eager, kept)
    rule = StopRule(3, n, [eos], pad)                                  # (deterministic rows are independent: the free run, cut)
    for i in range(n):
        rule.emit(free[:, i].tolist())
    assert torch.equal(eager[:, :ids.shape[1]], ids) and rule.done[0] == 1
    assert eager[:, ids.shape[1]:].tolist() == [r[:rule.steps_used or n] for r in rule.out]
    # another prompt length on the kept session: same graph, the output of a fresh session
    ids2, am2, _ = _prompts(dev, lens=(21, 35, 30), hi=hi, seed=9)
    kw2 = dict(kw, attention_mask=am2)
    reused = model.generate(input_ids=ids2, eos_token_id=eos, pad_token_id=pad, **kw2)
    assert eng._text_session is sess and eng.text_graph_captures == c0 + 1
    model.drop_decode_session()
    fresh = model.generate(input_ids=ids2, eos_token_id=eos, pad_token_id=pad, **kw2)
    assert eng.text_graph_captures == c0 + 2 and eng._text_session is not sess
    assert torch.equal(reused, fresh)
    # mmu_generate (one row) and mmu_generate_batch
    mkw = dict(max_new_tokens=n, temperature=0.0, deterministic=True, on_device=True)
    one = [model.mmu_generate(idx=ids[:1], attention_mask=mm[0], use_graph=g, **mkw) for g in (False, True, True)]
    assert eng.last_text_decode_on_device and len(one[0]) == n and one[0][0].dim() == 0 and one[0][0].is_cuda
    assert [int(t) for t in one[0]] == [int(t) for t in one[1]] == [int(t) for t in one[2]]
    eot = int(one[0][4])
    cut = [model.mmu_generate(idx=ids[:1], attention_mask=mm[0], eot_token=eot, use_graph=g, **mkw) for g in (False, True, True)]
    first = [int(t) for t in one[0]].index(eot)
    assert [int(t) for t in cut[0]] == [int(t) for t in one[0]][:first + 1] == [int(t) for t in cut[1]] == [int(t) for t in cut[2]]
    bfree = _lists(model.mmu_generate_batch(idx=ids, attention_mask=mm, **mkw))
    beot = bfree[1][2]
    batch = [_lists(model.mmu_generate_batch(idx=ids, attention_mask=mm, eot_token=beot, use_graph=g, **mkw)) for g in (False, True, True)]
    assert batch[0] == batch[1] == batch[2] and len(batch[0][1]) <= 3
    assert batch[0] == [r[:r.index(beot) + 1] if beot in r else r for r in bfree]
    model.drop_decode_session()


# ------------------------------------------------------------------ against the host loop, teacher-forced
def _teacher_forced(model, dev, ids, am, n, deterministic=False):
    """the host loop's tokens, then the engine's text step fed those tokens -> (compared, steps): the device pick must equal the host
    token wherever the step's own bf16 top-2 margin is >= MARGIN"""
    from unigen_hip import ops
    from unigen_hip.qwen2 import TextDecodeSession
    eng = model.llm.engine
    R, L = ids.shape
    host = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=n, deterministic=deterministic, on_device=False)[:, L:]
    assert not eng.last_text_decode_on_device and host.shape == (R, n)
    embed = model.llm.model.embed_tokens
    kv = am != 0
    sess = TextDecodeSession(eng, R, ops.round_up(L + n, 128), ops.round_up(n, 64), model.config.vocab_size, deterministic=deterministic, key_valid=kv)
    sess.begin(n)
    trace = []
    with torch.no_grad():
        eng.text_first_token(sess, eng.prefill(sess.st, embed(ids).float(), kv), trace)
        picks = [sess.tok.clone()]
        for i in range(1, n):
            sess.x.copy_(embed(host[:, i - 1:i])[:, 0])               # teacher forcing: the host loop's token, not the device's
            eng.text_step(sess, trace)
            picks.append(sess.tok.clone())
    assert int(sess.st.pos.item()) == L + n - 1 and int(sess.state[0]) == n
    assert torch.equal(sess.out_tokens[:, :n].long(), torch.stack(picks, 1))
    compared = 0
    for i in range(n):
        top2 = trace[i].bfloat16().float().topk(2, dim=-1).values
        margin = top2[:, 0] - top2[:, 1]
        for r in range(R):
            if float(margin[r]) >= MARGIN:
                assert int(picks[i][r]) == int(host[r, i]), (sess.form, r, i, float(margin[r]))
                compared += 1
    print(f"form {sess.form}, {R} rows: {compared} of {R * n} steps had a top-2 margin >= {MARGIN} and were compared")
    return compared, R * n, sess.form


@pytest.mark.parametrize("R", [1, 3, 24])
def test_engine_step_picks_the_host_loops_token_at_1p5b_width(dev, m1p5, R):
    """Three left-padded rows of 40 / 27 / 33 tokens (prompt seed 4, ids below 2 000), 12 new tokens: the CPU oracle has a top-2 margin
    >= 0.05 on 28 of these 36 steps; at least 20 must have been compared here (three borderline steps may fall either way).  One row:
    the first of them, and the same share (20 / 36) of its 12 steps; 24 rows: the three rows eight times (the split-K form: GEMV head
    into the accumulator the pick clears), the same share of 288."""
    lens, rep = ((40,), 1) if R == 1 else ((40, 27, 33), R // 3)
    ids, am, _ = _prompts(dev, lens=lens, repeat=rep)
    compared, total, form = _teacher_forced(m1p5, dev, ids, am, 12)
    assert form == {1: "sw", 3: "sw", 24: "splitk"}[R]
    assert compared >= total * 20 // 36, (compared, total)


@pytest.mark.parametrize("fused", [True, False])
def test_engine_step_picks_the_host_loops_token_on_the_small_model(dev, msmall, fused):
    """H = 256: the split-K form and (decode_fused = False) the wide form, both with the accumulator-clearing pick"""
    eng = msmall.llm.engine
    ids, am, _ = _prompts(dev, hi=300)
    eng.decode_fused = fused
    try:
        compared, total, form = _teacher_forced(msmall, dev, ids, am, 12)
    finally:
        eng.decode_fused = True
    assert form == ("splitk" if fused else "wide") and compared >= 1


# ------------------------------------------------------------------ stop rule and polling
@pytest.mark.parametrize("n", [5, 8, 9, 17])
def test_stop_id_cuts_the_run_as_the_host_loop_does(dev, m1p5, n):
    """deterministic mode: rows are independent, so the stopped run is the unstopped one put through the stop rule -- whatever the
    poll interval (8 tokens) makes of the steps behind the last row's stop"""
    model, eng = m1p5, m1p5.llm.engine
    ids, am, mm = _prompts(dev)
    L = ids.shape[1]
    kw = dict(attention_mask=am, deterministic=True, on_device=True)
    free = model.generate(input_ids=ids, max_new_tokens=17, **kw)[:, L:].cpu()
    stop, pad = int(free[0, 3]), 1
    rule = StopRule(3, n, [stop], pad)
    for i in range(n):
        rule.emit(free[:, i].tolist())
    steps = rule.steps_used or n
    got = model.generate(input_ids=ids, max_new_tokens=n, eos_token_id=stop, pad_token_id=pad, **kw)
    assert eng.last_text_decode_on_device
    assert got.shape == (3, L + steps) and got[:, L:].cpu().tolist() == [r[:steps] for r in rule.out]
    lists = model.mmu_generate_batch(idx=ids, attention_mask=mm, max_new_tokens=n, temperature=0.0, eot_token=stop, deterministic=True, on_device=True)
    host = model.mmu_generate_batch(idx=ids, attention_mask=mm, max_new_tokens=n, temperature=0.0, eot_token=stop, deterministic=True, on_device=False)
    assert len(lists) == len(host) == 3 and all(type(a) is type(b) and type(a[0]) is type(b[0]) and a[0].device == b[0].device for a, b in zip(lists, host))
    mfree = _lists(model.mmu_generate_batch(idx=ids, attention_mask=mm, max_new_tokens=n, temperature=0.0, deterministic=True, on_device=True))
    for r in range(3):
        want = mfree[r][:mfree[r].index(stop) + 1] if stop in mfree[r] else mfree[r]
        assert [int(t) for t in lists[r]] == want, r
    model.drop_decode_session()


# ------------------------------------------------------------------ sampling
def test_sampled_runs_repeat_with_the_seed_and_respect_top_k(dev, m1p5):
    model = m1p5
    ids, am, _ = _prompts(dev)
    L, n = ids.shape[1], 10
    kw = dict(input_ids=ids, attention_mask=am, max_new_tokens=n, deterministic=True, on_device=True)
    run = lambda seed, **k: model.generate(do_sample=True, generator=torch.Generator(device=dev).manual_seed(seed), **kw, **k)[:, L:]
    a, b, c = run(5, temperature=0.9, top_k=40, top_p=0.9), run(5, temperature=0.9, top_k=40, top_p=0.9), run(6, temperature=0.9, top_k=40, top_p=0.9)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # top_k = 1 keeps the maximum and everything TIED with it after the bf16 rounding (the rule keeps ties whole), and the draw then
    # chooses among the tied indices: the tokens are the greedy run's as long as the row's maximum is unique, which the greedy run's own
    # traced logits tell (rows are independent in deterministic mode, so each row is followed up to its first exact tie)
    gtrace = []
    greedy = model.generate(use_graph=False, trace=gtrace, **kw)[:, L:]
    one = run(7, temperature=0.7, top_k=1)
    followed = 0
    for r in range(3):
        for i in range(n):
            top2 = gtrace[i][r].bfloat16().float().topk(2).values
            if float(top2[0]) == float(top2[1]):
                break
            assert int(one[r, i]) == int(greedy[r, i]), (r, i)
            followed += 1
    print(f"top_k=1 against greedy: {followed} of {3 * n} tokens followed (up to each row's first exact bf16 tie of the top two)")
    assert followed >= 3                                              # (token 0 of every row at the least, unless it is itself a tie)
    trace = []
    got = run(8, temperature=1.5, top_k=5, use_graph=False, trace=trace)
    assert len(trace) == n
    off_argmax = 0
    for i in range(n):
        v = trace[i].bfloat16().float()
        fifth = v.topk(5, dim=-1).values[:, 4]
        assert bool((v.gather(1, got[:, i:i + 1])[:, 0] >= fifth).all()), i
        off_argmax += int((got[:, i] != v.argmax(-1)).sum())
    assert off_argmax > 0                                             # (temperature 1.5 over five candidates: not the greedy run)
    mm = model.mmu_generate(idx=ids[:1], attention_mask=_prompts(dev)[2][0], max_new_tokens=6, temperature=1.0, top_k=50, deterministic=True, on_device=True)
    assert len(mm) == 6 and model.llm.engine.last_text_decode_on_device
    model.drop_decode_session()


# ------------------------------------------------------------------ eligibility, default, the session's life
def test_eligibility_default_and_session_life(dev, msmall, monkeypatch):
    from unigen_hip.lib import UniGenHipError
    model, eng = msmall, msmall.llm.engine
    ids, am, mm = _prompts(dev, hi=300)
    L = ids.shape[1]
    kw = dict(max_new_tokens=6, deterministic=True)
    assert model.text_decode_on_device is False
    host = model.generate(input_ids=ids, attention_mask=am, **kw)
    assert eng.last_text_decode_on_device is False                    # default off
    wide = torch.randint(1, 300, (33, 9), generator=torch.Generator().manual_seed(2)).to(dev)
    host33 = model.generate(input_ids=wide, **kw)
    host1 = [int(t) for t in model.mmu_generate(idx=ids[:1], attention_mask=mm[0], use_cache=False, max_new_tokens=3, temperature=0.0)]
    with pytest.raises(UniGenHipError, match="33 rows"):
        model.generate(input_ids=wide, on_device=True, **kw)
    with pytest.raises(UniGenHipError, match="use_cache"):
        model.generate(input_ids=ids, attention_mask=am, use_cache=False, on_device=True, **kw)
    with pytest.raises(UniGenHipError, match="use_cache"):
        model.mmu_generate(idx=ids[:1], attention_mask=mm[0], use_cache=False, max_new_tokens=3, temperature=0.0, on_device=True)
    model.text_decode_on_device = True
    try:
        assert torch.equal(model.generate(input_ids=wide, **kw), host33) and eng.last_text_decode_on_device is False
        assert torch.equal(model.generate(input_ids=ids, attention_mask=am, use_cache=False, **kw), host) and eng.last_text_decode_on_device is False
        got1 = model.mmu_generate(idx=ids[:1], attention_mask=mm[0], use_cache=False, max_new_tokens=3, temperature=0.0)
        assert [int(t) for t in got1] == host1 and eng.last_text_decode_on_device is False
        on = model.generate(input_ids=ids, attention_mask=am, **kw)                               # the attribute alone turns it on
        assert eng.last_text_decode_on_device is True and on.shape == host.shape and eng._text_session is not None
        assert model.generate(input_ids=ids, attention_mask=am, on_device=False, **kw).shape == host.shape and eng.last_text_decode_on_device is False
    finally:
        model.text_decode_on_device = False
    model.generate(input_ids=ids, attention_mask=am, on_device=True, **kw)
    assert eng._text_session is not None
    model.drop_decode_session()
    assert eng._text_session is None
    model.generate(input_ids=ids, attention_mask=am, on_device=True, **kw)
    assert eng._text_session is not None
    model.train()
    assert eng._text_session is None
    model.eval()
    monkeypatch.setenv("UNIGEN_AR_GRAPH_CACHE", "0")
    model.generate(input_ids=ids, attention_mask=am, on_device=True, **kw)
    assert eng._text_session is None and eng.last_decode_graph
    monkeypatch.setenv("UNIGEN_TEXT_ON_DEVICE", "1")
    assert _small_model(dev).text_decode_on_device is True
