"""Prompt-lookup speculative decoding through the public calls (generate / mmu_generate / mmu_generate(prefix=...) with
prompt_lookup_num_tokens; UniGen._decode_text_spec, Qwen2Engine.spec_step): the tokens are the plain greedy step's wherever that step's
top-2 margin clears the rounding between step forms, acceptance happens and is counted, the session's life, the stop rule, every refusal
by name, and the calls without the arguments are what they were.

Fixture: the two-layer 1.5B-width model of test_text_generate_gpu.py (vocab 4 096, synth_llm_state seed 17): the sw form, and the
splitk form under UNIGEN_DECODE_SW=0.  Prompts: one row of 40 ids below 2 000 from torch seed 13 -- the CPU oracle (mmu_generate_ref
under bf16 autocast, 48 greedy tokens) has a top-2 margin >= 0.05 at 42 of the 48 steps (share 0.875; the others are steps 12, 18, 27,
44, 47 at 0.047 and step 29, an exact bf16 tie) -- and for the second prompt length 27 ids from seed 2 (43 of 48).  Acceptance is
COUNTED on the prompt of seed 1, where the oracle has 48 of 48 steps clear (smallest margin 0.14): at a near-tie a speculative run may
take the other pick and leave the plain run, which is right but changes what it finds to accept."""
import pytest
import torch

from helpers import additive, golden, llm_config_dir

pytestmark = pytest.mark.gpu

MARGIN = 0.05          # test_text_generate_gpu.py's: a top-2 margin below it may fall either way between two bf16 heads
N = 48


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


@pytest.fixture(scope="module")
def msmall(dev):
    """golden G9's config (H = 256): the splitk form, and with decode_fused = False the wide form"""
    from models import UniGen
    from oracle import weights
    g = golden("g9_generate.pt")
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=g["weight_std"]), strict=False)
    return m.eval()


@pytest.fixture(params=["sw", "splitk"])
def form(request, monkeypatch, m1p5):
    if request.param == "splitk":
        monkeypatch.setenv("UNIGEN_DECODE_SW", "0")
    m1p5.drop_decode_session()
    assert m1p5.llm.engine.decode_form(8, False) == request.param and m1p5.llm.engine.decode_form(1, False) == request.param
    yield request.param
    m1p5.drop_decode_session()


def _prompt(dev, seed=13, L=40):
    ids = torch.randint(1, 2000, (1, L), generator=torch.Generator().manual_seed(seed)).to(dev)
    allow = torch.tril(torch.ones(L, L, dtype=torch.bool))[None]
    return ids, additive(allow).reshape(1, 1, L, L).to(dev)


_PLAIN = {}


def _plain_run(model, ids, form):
    """the plain device loop's own N tokens for a prompt (computed once per prompt and form, never changed): what the lookup finds"""
    key = (form, tuple(ids[0].tolist()))
    if key not in _PLAIN:
        out = model.generate(input_ids=ids, max_new_tokens=N, on_device=True, use_graph=False)[:, ids.shape[1]:]
        assert model.llm.engine.last_text_decode_on_device and out.shape == (1, N)
        _PLAIN[key] = out[0].clone()
    return _PLAIN[key]


def _agrees_with_the_plain_step(model, ids, y):
    """Teacher forcing as test_text_generate_gpu.py: _teacher_forced: the plain engine text step fed y's own tokens must pick y[i]
    wherever its top-2 margin is >= MARGIN, and at least three quarters of the positions must clear the margin -> the margins"""
    from unigen_hip import ops
    from unigen_hip.qwen2 import TextDecodeSession
    eng, embed, n = model.llm.engine, model.llm.model.embed_tokens, int(y.numel())
    L = ids.shape[1]
    sess = TextDecodeSession(eng, 1, ops.round_up(L + n, 128), ops.round_up(n, 64), model.config.vocab_size)
    sess.begin(n)
    trace = []
    with torch.no_grad():
        eng.text_first_token(sess, eng.prefill(sess.st, embed(ids).float()), trace)
        picks = [int(sess.tok)]
        for i in range(1, n):
            sess.x.copy_(embed(y[i - 1:i][None])[:, 0])
            eng.text_step(sess, trace)
            picks.append(int(sess.tok))
    margins = []
    for i in range(n):
        top2 = trace[i][0].bfloat16().float().topk(2).values
        margins.append(float(top2[0] - top2[1]))
        if margins[-1] >= MARGIN:
            assert picks[i] == int(y[i]), (sess.form, i, margins[-1], picks[i], int(y[i]))
    clear = sum(m >= MARGIN for m in margins)
    print(f"form {sess.form}: {clear} of {n} positions had a top-2 margin >= {MARGIN} and were compared")
    assert clear * 4 >= n * 3, (clear, n)
    return margins


def test_tokens_are_the_plain_steps_and_acceptance_is_counted(dev, m1p5, form):
    model, eng = m1p5, m1p5.llm.engine
    ids, _ = _prompt(dev)
    L = ids.shape[1]
    plain = _plain_run(model, ids, form)
    _agrees_with_the_plain_step(model, ids, plain)                     # (the plain path alone satisfies the condition)
    # nothing to look up but the random prompt and the run's own tokens
    y = model.generate(input_ids=ids, max_new_tokens=N, prompt_lookup_num_tokens=7, use_graph=False)
    assert eng.last_text_decode_on_device and y.shape == (1, L + N) and torch.equal(y[:, :L], ids)
    st = eng.last_spec_stats
    assert st["emitted"] == N and 1 <= st["steps"] <= N and st["accepted"] <= st["drafted"] <= 7 * st["steps"]
    _agrees_with_the_plain_step(model, ids, y[0, L:])
    # the plain run's own output as extra searchable text.  On this prompt the count is reported, not asserted: a run may leave the
    # plain run at one of its near-ties (either pick is right there), and what it accepts from then on is its own business
    y2 = model.generate(input_ids=ids, max_new_tokens=N, prompt_lookup_num_tokens=7, lookup_ids=plain, use_graph=False)
    st = eng.last_spec_stats
    print(f"form {form}: seed 13, lookup = the plain run: {st}")
    assert st["emitted"] == N and st["steps"] <= N
    _agrees_with_the_plain_step(model, ids, y2[0, L:])
    # counted on the prompt of seed 1, whose greedy chain has no near-tie at all (CPU oracle: 48 of 48 margins clear, the smallest
    # 0.14; the model settles on one token, which is as much of a repetition as a lookup can find): the speculative run IS the plain
    # run, so with the plain run's output as lookup_ids acceptance is at its ceiling -- at least half the tokens, under half the steps
    ids1, _ = _prompt(dev, seed=1)
    plain1 = _plain_run(model, ids1, form)
    assert min(_agrees_with_the_plain_step(model, ids1, plain1)) >= MARGIN
    y4 = model.generate(input_ids=ids1, max_new_tokens=N, prompt_lookup_num_tokens=7, lookup_ids=plain1, use_graph=False)
    st = eng.last_spec_stats
    print(f"form {form}: seed 1, lookup = the plain run: {st}")
    assert torch.equal(y4[0, L:], plain1)
    assert st["emitted"] == N and st["accepted"] >= N // 2 and st["steps"] < N // 2
    # a longer n-gram and a shorter draft: the same property
    y3 = model.generate(input_ids=ids, max_new_tokens=N, prompt_lookup_num_tokens=3, max_matching_ngram_size=4, lookup_ids=plain, use_graph=False)
    assert eng.last_spec_stats["drafted"] <= 3 * eng.last_spec_stats["steps"]
    _agrees_with_the_plain_step(model, ids, y3[0, L:])


def test_session_life(dev, m1p5, form):
    model, eng = m1p5, m1p5.llm.engine
    ids, _ = _prompt(dev)
    L = ids.shape[1]
    plain = _plain_run(model, ids, form)
    kw = dict(max_new_tokens=N, prompt_lookup_num_tokens=7, lookup_ids=plain)
    c0 = getattr(eng, "text_graph_captures", 0)
    eager = model.generate(input_ids=ids, use_graph=False, **kw)
    assert not eng.last_decode_graph and eng._spec_session is None and getattr(eng, "text_graph_captures", 0) == c0
    captured = model.generate(input_ids=ids, **kw)
    sess = eng._spec_session
    assert eng.last_decode_graph and eng.text_graph_captures == c0 + 1 and sess is not None and sess.graph is not None and sess.form == form
    kept = model.generate(input_ids=ids, **kw)
    assert eng._spec_session is sess and eng.text_graph_captures == c0 + 1 and eng.last_spec_stats["emitted"] == N
    for out in (eager, captured, kept):
        assert out.shape == (1, L + N)
        _agrees_with_the_plain_step(model, ids, out[0, L:])
    # one capture serves a second prompt length (27 ids, seed 2): same capacity, same history capacity, same key
    ids2, _ = _prompt(dev, seed=2, L=27)
    plain2 = _plain_run(model, ids2, form)
    other = model.generate(input_ids=ids2, **dict(kw, lookup_ids=plain2))
    assert eng._spec_session is sess and eng.text_graph_captures == c0 + 1
    _agrees_with_the_plain_step(model, ids2, other[0, 27:])
    model.drop_decode_session()
    assert eng._spec_session is None and eng._text_session is None


def test_mmu_calls_and_the_stop_id(dev, m1p5, form):
    model, eng = m1p5, m1p5.llm.engine
    ids, mm = _prompt(dev)
    L = ids.shape[1]
    plain = _plain_run(model, ids, form)
    margins = _agrees_with_the_plain_step(model, ids, plain)
    kw = dict(max_new_tokens=N, temperature=0.0, prompt_lookup_num_tokens=7, lookup_ids=plain)
    free = model.mmu_generate(idx=ids, attention_mask=mm, **kw)
    assert eng.last_text_decode_on_device and len(free) == N and free[0].dim() == 0 and free[0].is_cuda
    free_t = torch.stack(free)
    _agrees_with_the_plain_step(model, ids, free_t)
    # top_k = 1 is greedy whatever the temperature
    _agrees_with_the_plain_step(model, ids, torch.stack(model.mmu_generate(idx=ids, attention_mask=mm, **dict(kw, temperature=0.7, top_k=1))))
    # behind a prefix (causal, 25 positions; the tail of 15 as ids): the same sequence
    prefix = model.mmu_prefix(idx=ids[:, :25])
    tail = model.mmu_generate(idx=ids[:, 25:], prefix=prefix, **kw)
    assert len(tail) == N
    _agrees_with_the_plain_step(model, ids, torch.stack(tail))
    # a prompt given as embeddings has no ids: lookup_ids is all there is to search
    emb = model.llm.model.embed_tokens(ids).float()
    as_emb = model.mmu_generate(input_embeddings=emb, attention_mask=mm, **kw)
    assert eng.last_spec_stats["accepted"] >= N // 2
    _agrees_with_the_plain_step(model, ids, torch.stack(as_emb))
    # a stop id taken from the free run (the first token at a position >= 8 that has not occurred before): the output is the free run
    # cut behind it, as the plain rule cuts.  The default decode mode is not bit-reproducible, so a run may leave the free run -- but
    # only at a position whose margin is unclear; a run that does not ends exactly at j, the stop id included
    toks = [int(t) for t in free_t]
    j = next(i for i in range(8, N) if toks[i] not in toks[:i])
    stop = toks[j]

    def cut_as_the_rule_cuts(out):
        out = [int(t) for t in out]
        assert 1 <= len(out) <= N and stop not in out[:-1] and (out[-1] == stop or len(out) == N)
        d = next((i for i in range(len(out)) if out[i] != toks[i]), None)
        if d is None:
            assert len(out) == j + 1, (len(out), j)
        else:
            assert margins[d] < MARGIN, ("left the free run at a position with a clear margin", d, margins[d])
        return d is None
    margins = _agrees_with_the_plain_step(model, ids, free_t)
    cut = model.mmu_generate(idx=ids, attention_mask=mm, eot_token=stop, **kw)
    if cut_as_the_rule_cuts(cut):
        assert eng.last_spec_stats["emitted"] == j + 1
    gen = model.generate(input_ids=ids, max_new_tokens=N, eos_token_id=stop, prompt_lookup_num_tokens=7, lookup_ids=plain)
    assert torch.equal(gen[:, :L], ids)
    cut_as_the_rule_cuts(gen[0, L:])
    cut_as_the_rule_cuts(model.generate(input_ids=ids, max_new_tokens=N, eos_token_id=stop, on_device=True)[0, L:])    # (the plain loop)


def test_every_refusal_by_name(dev, m1p5, msmall):
    from unigen_hip.lib import UniGenHipError
    model, eng = m1p5, m1p5.llm.engine
    model.drop_decode_session()
    ids, mm = _prompt(dev)
    two = torch.cat([ids, ids])
    look = dict(input_ids=ids, max_new_tokens=8, prompt_lookup_num_tokens=4)
    refused = dict(repetition_penalty=1.3, logit_bias={5: 1.0}, suppress_tokens=[5], min_new_tokens=2, no_repeat_ngram_size=2,
                   stop_sequences=[[3, 4]], return_logprobs=True, deterministic=True, num_return_sequences=2, on_device=False)
    for name, value in refused.items():
        with pytest.raises(UniGenHipError, match=name):
            model.generate(eos_token_id=9, **look, **{name: value})
    mlook = dict(idx=ids, attention_mask=mm, max_new_tokens=8, temperature=0.0, prompt_lookup_num_tokens=4)
    for name, value in refused.items():
        if name != "num_return_sequences":
            with pytest.raises(UniGenHipError, match=name):
                model.mmu_generate(eot_token=9, **mlook, **{name: value})
    with pytest.raises(UniGenHipError, match="one row"):
        model.generate(**dict(look, input_ids=two))
    for bad in (8, -1):
        with pytest.raises(UniGenHipError, match="prompt_lookup_num_tokens"):
            model.generate(**dict(look, prompt_lookup_num_tokens=bad))
    for bad in (0, 5):
        with pytest.raises(UniGenHipError, match="max_matching_ngram_size"):
            model.generate(max_matching_ngram_size=bad, **look)
    with pytest.raises(UniGenHipError, match="greedy"):
        model.generate(do_sample=True, **look)
    with pytest.raises(UniGenHipError, match="greedy"):
        model.mmu_generate(**dict(mlook, temperature=1.0, top_k=5))
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros((1, 4), dtype=torch.long), torch.tensor([1, 4096]), [1, 2]):
        with pytest.raises(UniGenHipError, match="lookup_ids"):
            model.generate(lookup_ids=bad, **look)
    with pytest.raises(UniGenHipError, match="use_cache"):
        model.mmu_generate(**dict(mlook, use_cache=False))
    # golden G9's config with decode_fused = False: the wide form, named in the message
    small, seng = msmall, msmall.llm.engine
    sids = torch.randint(1, 300, (1, 12), generator=torch.Generator().manual_seed(1)).to(dev)
    seng.decode_fused = False
    try:
        assert seng.decode_form(5, False) == "wide"
        with pytest.raises(UniGenHipError, match="wide"):
            small.generate(input_ids=sids, max_new_tokens=8, prompt_lookup_num_tokens=4)
    finally:
        seng.decode_fused = True
    assert eng._spec_session is None and getattr(seng, "_spec_session", None) is None


def test_arguments_off_change_nothing(dev, m1p5):
    """prompt_lookup_num_tokens None or 0 with the other two arguments present: the deterministic outputs of the same calls without them"""
    model, eng = m1p5, m1p5.llm.engine
    model.drop_decode_session()
    ids, mm = _prompt(dev)
    off = dict(max_matching_ngram_size=3, lookup_ids=torch.arange(5))
    for on_device in (True, False):
        kw = dict(input_ids=ids, max_new_tokens=12, deterministic=True, on_device=on_device)
        base = model.generate(**kw)
        for k in (None, 0):
            assert torch.equal(model.generate(prompt_lookup_num_tokens=k, **off, **kw), base)
            assert eng.last_text_decode_on_device is on_device and eng._spec_session is None
        mkw = dict(idx=ids, attention_mask=mm, max_new_tokens=12, temperature=0.0, deterministic=True, on_device=on_device)
        mbase = [int(t) for t in model.mmu_generate(**mkw)]
        assert [int(t) for t in model.mmu_generate(prompt_lookup_num_tokens=0, **off, **mkw)] == mbase
    model.drop_decode_session()
