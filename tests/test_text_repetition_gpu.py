"""`repetition_penalty` and `num_return_sequences` on both text loops (UniGen.generate / mmu_generate_batch; Qwen2Engine.text_step's
logits processor, csrc/text_sampler.hip: ug_text_penalize), on the H = 256 fixture model of test_text_generate_gpu.py (golden G9's
config, vocabulary 333): 16 new tokens, one and three left-padded rows (40 / 27 / 33 tokens, ids below 300), penalty 1.3.

The prompt seeds were chosen on the CPU with the oracle's forward of the same fixture (oracle.qwen2_ref.RefCausalLM under bf16
autocast, the prompt rows under their masks, the host rule on the fp32 copy of the logits):
  SEED_BITES = 11    at p = 1.0 row 0 emits [143, 6, 58, 201, 73, 119, 95, 225, 23, 115, 115, 115, 320, ...]: id 115 three times; at
                     p = 1.3 every row differs from its p = 1.0 run and no row repeats any id (of seeds 0 .. 15 only this one shows
                     a threefold repeat);
  SEED_LOOPS = 42    at p = 1.3 the host rule's processed top-2 margin first falls below 0.05 at step 12 of row 0 and never in rows 1
                     and 2; before that its minimum is 0.156 / 0.125 / 0.156 (of seeds 0 .. 79 the only one with at least ten such
                     steps in every row at a margin of 0.12 or more: the fixture's logits sit a few bf16 steps apart)."""
import pytest
import torch

import repetition_penalty_ref as ref
from helpers import additive, golden, llm_config_dir
from test_text_generate_gpu import MARGIN          # the bar of the existing host-against-device text test (0.05), not a new one

pytestmark = pytest.mark.gpu

P, NEW = 1.3, 16
SEED_BITES = 11
SEED_LOOPS = 42


@pytest.fixture(scope="module")
def model(dev):
    from models import UniGen
    from oracle import weights
    g = golden("g9_generate.pt")
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=g["weight_std"]), strict=False)
    return m.eval()


def _prompts(R, seed, hi=300):
    """left-padded rows (test_text_generate_gpu._prompts) -> (ids [R, L], attention mask [R, L], allow [R, L, L]) on the CPU"""
    lens = (40, 27, 33)[:R]
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.zeros((R, L), dtype=torch.long)
    am = torch.zeros((R, L), dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, L - n:] = torch.randint(1, hi, (n,), generator=g)
        am[r, L - n:] = 1
    allow = (torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & am.bool()[:, None, :]) | torch.eye(L, dtype=torch.bool)[None]
    return ids, am, allow


def _follows_the_rule(V, ids, valid, trace, tokens):
    """every emitted token = the reference rule on that step's traced RAW logits and the row's history so far; exact"""
    R = tokens.shape[0]
    bm = ref.Bitmap(R, V)
    if ids is not None:
        bm.mark(ids, valid)
    assert len(trace) == tokens.shape[1]
    for i, raw in enumerate(trace):
        want = ref.first_argmax(bm.penalize(raw.cpu(), P, tokens[:, i - 1].tolist() if i else None))
        assert tokens[:, i].tolist() == want.tolist(), (i, tokens[:, i].tolist(), want.tolist())
    return bm


# ------------------------------------------------------------------ (a) the processor and the pick against the device's own logits
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("R", [1, 3])
def test_every_on_device_token_follows_the_rule_on_its_traced_logits(dev, model, R, deterministic):
    V = model.config.vocab_size
    ids, am, _ = _prompts(R, SEED_BITES)
    trace = []
    out = model.generate(input_ids=ids.to(dev), attention_mask=am.to(dev), max_new_tokens=NEW, on_device=True, use_graph=False, trace=trace,
                         repetition_penalty=P, deterministic=deterministic)
    assert model.llm.engine.last_text_decode_on_device and out.shape == (R, ids.shape[1] + NEW)
    _follows_the_rule(V, ids, am, trace, out[:, ids.shape[1]:].cpu())
    # a prompt given as embeddings has no ids: the history is the emitted tokens alone
    trace = []
    emb = model.llm.model.embed_tokens(ids.to(dev))
    out = model.generate(input_embeddings=emb, attention_mask=am.to(dev), max_new_tokens=NEW, on_device=True, use_graph=False, trace=trace,
                         repetition_penalty=P, deterministic=deterministic)
    assert out.shape == (R, NEW)
    _follows_the_rule(V, None, None, trace, out.cpu())


# ------------------------------------------------------------------ (b) captured = eager = kept session; the penalty is in the key
@pytest.mark.parametrize("R", [1, 3])
def test_captured_eager_and_kept_session_agree_and_the_penalty_keys_the_graph(dev, model, R):
    eng = model.llm.engine
    ids, am, _ = _prompts(R, SEED_BITES)
    kw = dict(input_ids=ids.to(dev), attention_mask=am.to(dev), max_new_tokens=NEW, on_device=True, deterministic=True)
    model.drop_decode_session()
    eager = model.generate(use_graph=False, repetition_penalty=P, **kw)
    assert eng._text_session is None
    c0 = getattr(eng, "text_graph_captures", 0)
    captured = model.generate(repetition_penalty=P, **kw)
    sess = eng._text_session
    assert eng.last_decode_graph and eng.text_graph_captures == c0 + 1 and sess is not None and sess.seen is not None and sess.penalty == P
    kept = model.generate(repetition_penalty=P, **kw)
    assert eng._text_session is sess and eng.text_graph_captures == c0 + 1            # the same penalty: the same graph
    assert torch.equal(eager, captured) and torch.equal(eager, kept)
    other = model.generate(repetition_penalty=1.7, **kw)
    assert eng.text_graph_captures == c0 + 2 and eng._text_session is not sess        # another penalty: not the same graph
    off = model.generate(**kw)
    assert eng.text_graph_captures == c0 + 3 and eng._text_session.seen is None       # off: nothing allocated
    assert not torch.equal(other, eager) or not torch.equal(off, eager)
    back = model.generate(repetition_penalty=P, **kw)
    assert torch.equal(back, eager)
    model.drop_decode_session()


# ------------------------------------------------------------------ (c) the feature bites
@pytest.mark.parametrize("R", [1, 3])
def test_penalty_changes_the_greedy_output_and_ends_the_threefold_repeat(dev, model, R):
    """SEED_BITES: on the CPU oracle row 0 repeats id 115 three times at p = 1.0 and nothing at p = 1.3 (module docstring).  Whatever the
    device's own p = 1.0 run repeats three or more times, the p = 1.3 run must not repeat."""
    ids, am, _ = _prompts(R, SEED_BITES)
    L = ids.shape[1]
    kw = dict(input_ids=ids.to(dev), attention_mask=am.to(dev), max_new_tokens=NEW, on_device=True, deterministic=True)
    plain = model.generate(**kw)[:, L:].cpu().tolist()
    pen = model.generate(repetition_penalty=P, **kw)[:, L:].cpu().tolist()
    assert plain != pen
    threefold = 0
    for r in range(R):
        for t in set(plain[r]):
            if plain[r].count(t) >= 3:
                threefold += 1
                assert pen[r].count(t) <= 1, (r, t, plain[r], pen[r])
    print(f"{R} rows: {threefold} ids repeated three or more times at p = 1.0; rows that differ: {sum(a != b for a, b in zip(plain, pen))}")
    model.drop_decode_session()


# ------------------------------------------------------------------ (d) host loop against device loop
@pytest.mark.parametrize("R", [1, 3])
def test_host_and_device_loops_agree_up_to_the_first_near_tie(dev, model, R, monkeypatch):
    """Greedy, p = 1.3, step by step: tokens equal up to each row's first step at which the HOST loop's processed top-2 margin is below
    MARGIN; at least half of the 16 steps of every row must be compared (CPU oracle, SEED_LOOPS: 12 / 16 / 16 steps).  The two loops
    round differently (host: fp32 rule on the bf16 head's logits; device: the rule on the bf16-rounded fp32 head's logits), so behind a
    near tie they may part for good: the comparison of a row ends there.  On an MI355X: 15 of 16 steps compared with one row,
    15 / 16 / 16 with three."""
    from models import sampling
    ids, am, _ = _prompts(R, SEED_LOOPS)
    L = ids.shape[1]
    processed = []
    rule = sampling.apply_repetition_penalty

    def recording(logits, seen, penalty):
        out = rule(logits, seen, penalty)
        processed.append(out.clone())
        return out
    monkeypatch.setattr(sampling, "apply_repetition_penalty", recording)
    kw = dict(input_ids=ids.to(dev), attention_mask=am.to(dev), max_new_tokens=NEW, repetition_penalty=P)
    host = model.generate(on_device=False, **kw)[:, L:].cpu()
    assert not model.llm.engine.last_text_decode_on_device and len(processed) == NEW
    device = model.generate(on_device=True, **kw)[:, L:].cpu()
    assert model.llm.engine.last_text_decode_on_device and len(processed) == NEW         # (the device loop never calls the host rule)
    compared = []
    for r in range(R):
        k = 0
        for i in range(NEW):
            top2 = processed[i][r].float().topk(2).values
            if float(top2[0] - top2[1]) < MARGIN:
                break
            assert int(host[r, i]) == int(device[r, i]), (r, i, host[r].tolist(), device[r].tolist())
            k += 1
        compared.append(k)
    print(f"{R} rows, host against device at p = {P}: steps compared per row {compared} of {NEW}")
    assert min(compared) >= NEW // 2, compared
    model.drop_decode_session()


# ------------------------------------------------------------------ (e) num_return_sequences
@pytest.mark.parametrize("on_device", [True, False])
def test_num_return_sequences_repeats_every_prompt_consecutively(dev, model, on_device):
    from unigen_hip.lib import UniGenHipError
    ids, am, _ = _prompts(3, SEED_BITES)
    B, L = ids.shape
    kw = dict(input_ids=ids.to(dev), attention_mask=am.to(dev), max_new_tokens=NEW, do_sample=True, temperature=0.9, top_k=40, num_return_sequences=3,
              on_device=on_device, deterministic=True)
    run = lambda seed, **k: model.generate(generator=torch.Generator(device=dev).manual_seed(seed), **dict(kw, **k))
    a, b = run(5), run(5)
    assert model.llm.engine.last_text_decode_on_device is on_device
    assert a.shape == (B * 3, L + NEW) and torch.equal(a, b)
    assert torch.equal(a[:, :L].cpu(), ids.repeat_interleave(3, dim=0))
    for p in range(B):
        rows = a[3 * p:3 * p + 3, L:]
        assert not (torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])), p      # independent draws
    pen = run(5, repetition_penalty=P)
    assert pen.shape == a.shape and not torch.equal(pen, a)
    emb = model.llm.model.embed_tokens(ids.to(dev))
    e = model.generate(input_embeddings=emb, generator=torch.Generator(device=dev).manual_seed(5), **{k: v for k, v in kw.items() if k != "input_ids"})
    assert e.shape == (B * 3, NEW)
    wide = torch.randint(1, 300, (11, 9), generator=torch.Generator().manual_seed(2)).to(dev)
    if on_device:
        with pytest.raises(UniGenHipError, match="33 rows"):
            model.generate(input_ids=wide, max_new_tokens=4, do_sample=True, num_return_sequences=3, on_device=True)
        model.text_decode_on_device = True
        try:                                                       # default-derived: the host loop serves the 33 rows
            out = model.generate(input_ids=wide, max_new_tokens=4, do_sample=True, num_return_sequences=3)
        finally:
            model.text_decode_on_device = False
        assert out.shape == (33, 13) and model.llm.engine.last_text_decode_on_device is False
    with pytest.raises(UniGenHipError, match="do_sample"):
        model.generate(input_ids=wide, max_new_tokens=4, num_return_sequences=3, on_device=on_device)
    model.drop_decode_session()


# ------------------------------------------------------------------ (f) mmu_generate_batch
def test_mmu_generate_batch_marks_only_what_the_prompts_last_row_sees(dev, model):
    """Two left-padded rows whose masks also hide five REAL prompt positions from every later row: their ids are no part of the history.
    Eager with trace: every token follows the rule; captured: the same tokens, and the kept session's bitmap is the visible prompt ids +
    every emitted token but the last (which the next step's launch would add)."""
    from unigen_hip.lib import UniGenHipError
    V = model.config.vocab_size
    ids, am, allow = _prompts(2, SEED_BITES)
    L = ids.shape[1]
    hidden = torch.arange(L - 20, L - 15)
    allow[:, L - 15:, L - 20:L - 15] = False                      # rows behind the span do not see it (the span is real in both rows)
    mask = additive(allow).reshape(2, 1, L, L).to(dev)
    visible = allow[:, -1, :]
    assert bool(am[:, hidden].all()) and not bool(visible[:, hidden].any())
    for r in range(2):                                             # the hidden ids are found nowhere else in the row
        ids[r, hidden] = torch.tensor([301 + 5 * r + j for j in range(5)])
    kw = dict(idx=ids.to(dev), attention_mask=mask, max_new_tokens=NEW, temperature=0.0, on_device=True, repetition_penalty=P, deterministic=True)
    trace = []
    eager = model.mmu_generate_batch(use_graph=False, trace=trace, **kw)
    tokens = torch.tensor([[int(t) for t in row] for row in eager])
    assert tokens.shape == (2, NEW)
    _follows_the_rule(V, ids, visible, trace, tokens)
    model.drop_decode_session()
    captured = model.mmu_generate_batch(**kw)
    assert [[int(t) for t in row] for row in captured] == tokens.tolist()
    sess = model.llm.engine._text_session
    want = ref.Bitmap(2, V).mark(ids, visible)
    for i in range(NEW - 1):
        want.add(tokens[:, i].tolist())
    assert torch.equal(sess.seen.cpu(), want.tensor())
    prompt_only, every_real = ref.Bitmap(2, V).mark(ids, visible).seen(), ref.Bitmap(2, V).mark(ids, am).seen()
    assert not bool(prompt_only[0, 301:306].any()) and not bool(prompt_only[1, 306:311].any())
    assert bool(every_real[0, 301:306].all()) and bool(every_real[1, 306:311].all())
    host = model.mmu_generate_batch(**dict(kw, on_device=False))
    assert len(host) == 2 and all(len(h) == NEW for h in host)
    one = model.mmu_generate(idx=ids[:1].to(dev), attention_mask=mask[0], max_new_tokens=NEW, temperature=0.0, on_device=True, repetition_penalty=P,
                             deterministic=True)
    assert len(one) == NEW and model.llm.engine.last_text_decode_on_device
    with pytest.raises(UniGenHipError, match="recompute"):
        model.mmu_generate(idx=ids[:1].to(dev), attention_mask=mask[0], max_new_tokens=4, temperature=0.0, use_cache=False, repetition_penalty=P)
    model.drop_decode_session()
