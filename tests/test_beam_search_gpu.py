"""UniGen.beam_search on the GPU, on the two-layer 1.5B-width model of the text tests (vocab 4 096, synth_llm_state seed 17), in
deterministic mode: against a reference loop on the same engine that swaps the two new kernels for tests/beam_ref.py: candidates_ref
and an index copy of the cache; num_beams=1 against greedy `generate`; ids against embedding prompts; and no state left behind."""
import pytest
import torch

from beam_ref import candidates_ref, rank_gaps, tol
from helpers import additive, llm_config_dir

pytestmark = pytest.mark.gpu

V, NEW = 4096, 10


SPECIAL = list(range(16, 32))       # the tokens the head favours, in this order
ALPHA, GAIN = 0.01, 1000.0


def build_model(dev, gain=GAIN):
    """The text tests' model with a head made sharp on purpose.  bf16 logits keep 8 bits, so among the best K + 1 of B x 4 096 nearly
    Gaussian logits two are equal at almost every step, and a reference whose ranks tie says nothing.  Here channel 0 of the residual
    stream carries only the token's own embedding (row 0 of every o_proj / down_proj is zero), that embedding is -a[e] there, and the
    final norm's gain on the channel is -gain: logit[e] = -a[e] * (gain * a[token] / rms) + the other channels' Gaussian part (sigma
    about 0.8).  a = ALPHA * (1 + j / 2) for SPECIAL[j] and 30 ALPHA elsewhere: the best candidates are the first special tokens,
    one or several sigma apart, and the context still decides their order.  The gain and the prompts' seed were picked on the GPU among a
    few for rank gaps above the bound at all ten steps with 2 and with 4 beams; the test asserts the gaps, so a choice that stops holding
    fails loudly."""
    from models import UniGen
    from oracle import qwen2_ref, weights
    cfg = dict(qwen2_ref.QWEN25_1P5B, num_hidden_layers=2, vocab_size=V)
    m = UniGen(w_und_encoder=False, vocab_size=V, llm_vocab_size=2048, llm_model_path=llm_config_dir(cfg), codebook_size=2047,
               num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=-1).eval()
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    state = weights.synth_llm_state(names, seed=17)
    a = torch.full((V,), 30 * ALPHA)
    a[SPECIAL] = ALPHA * (1 + 0.5 * torch.arange(len(SPECIAL)))
    touched = 0
    for name, w in state.items():
        if name.endswith("embed_tokens.weight"):
            w[:, 0] = -a
            touched += 1
        elif name.endswith(("o_proj.weight", "down_proj.weight")):
            w[0, :] = 0
            touched += 1
        elif name.endswith("model.norm.weight"):
            w[0] = -gain
            touched += 1
    assert touched == 2 + 2 * cfg["num_hidden_layers"], (touched, [n for n, _ in names])
    m.llm.load_state_dict(state, strict=False)
    return m


@pytest.fixture(scope="module")
def model(dev):
    return build_model(dev)


def _prompts(dev, lens=(40, 27, 33), seed=6):
    """left-padded rows -> (ids [R, L], attention mask [R, L])"""
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.zeros((len(lens), L), dtype=torch.long)
    am = torch.zeros((len(lens), L), dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, L - n:] = torch.randint(1, 2000, (n,), generator=g)
        am[r, L - n:] = 1
    return ids.to(dev), am.to(dev)


@torch.no_grad()
def reference_loop(model, ids, am, B, eos, new, **how):
    """beam_search's loop with candidates_ref for the kernel and an index copy for the reorder -> (sequences, scores, smallest rank gap,
    whether a hypothesis entered a finished pool before the last step)"""
    from models.beam import BeamSearch
    from unigen_hip.qwen2 import DecodeState
    eng, embed = model.llm.engine, model.llm.model.embed_tokens
    G, L = ids.shape
    R = G * B
    rep = lambda t: t.repeat_interleave(B, dim=0)
    st = DecodeState(eng.dims, R, L + new, ids.device, key_valid=rep(am) != 0, deterministic=True)
    hn = eng.prefill(st, embed(rep(ids)).float(), rep(am) != 0)
    search = BeamSearch(G, B, eos, None, new, **how)
    gap, fired = float("inf"), False
    for i in range(new):
        logits = eng.head_slice(hn, 0, V).float()
        scores = search.running_scores()
        gap = min(gap, rank_gaps(logits, scores, G, B, V, search.k))
        cand = candidates_ref(logits, scores, G, B, V, search.k)[:3]
        parent, token, finished = search.step(*[c.to(ids.device) for c in cand])
        fired |= search.steps < new and bool(search.is_fin.any())
        if finished or i + 1 == new:
            break
        n = L + i
        for c in st.k + st.v:
            c[:, :, L:n] = c[parent.long()][:, :, L:n]
        hn = eng.decode_step(st, embed(token)[:, 0].float().contiguous())
    out, sc = search.finalize()
    return torch.cat([ids.repeat_interleave(search.n_ret, dim=0), out], dim=1), sc, gap, fired


# eos 0 never fires (the prompts' pad id: the model does not emit it within the steps taken); the other id is taken from the free run
@pytest.mark.parametrize("B,early", [(2, False), (4, False), (4, True)])
def test_beam_search_is_the_reference_loop(dev, model, B, early):
    ids, am = _prompts(dev)
    how = dict(length_penalty=1.0, early_stopping=False, num_return_sequences=B)
    eos = [0]
    if early:
        free = reference_loop(model, ids, am, B, [0], NEW, **how)[0]
        eos = [int(free[0, ids.shape[1] + 7])]                                # the eighth token of prompt 0's best free hypothesis
    want, want_scores, gap, fired = reference_loop(model, ids, am, B, eos, NEW, **how)
    got, scores = model.beam_search(input_ids=ids, attention_mask=am, max_new_tokens=NEW, num_beams=B, eos_token_id=eos, deterministic=True,
                                    return_scores=True, **how)
    print("B", B, "early", early, "gap", gap, "bound", 10 * tol(V), "max |score - ref|", float((scores - want_scores).abs().max()))
    assert gap >= 10 * tol(V), (gap, 10 * tol(V))
    assert got.shape == want.shape and torch.equal(got, want), (got[:, ids.shape[1]:], want[:, ids.shape[1]:])
    assert float((scores - want_scores).abs().max()) <= NEW * tol(V)
    assert fired == early                                                     # the eos id fired before the last step, or never


def test_one_beam_is_greedy_generate(dev, model):
    ids, am = _prompts(dev)
    free = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=NEW, do_sample=False, deterministic=True, on_device=False)
    eos = int(free[1, ids.shape[1] + 4])
    want = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=NEW, do_sample=False, eos_token_id=eos, deterministic=True,
                          on_device=False)
    got = model.beam_search(input_ids=ids, attention_mask=am, max_new_tokens=NEW, num_beams=1, eos_token_id=eos, deterministic=True)
    assert torch.equal(got, want)
    assert torch.equal(model.beam_search(input_ids=ids, attention_mask=am, max_new_tokens=NEW, num_beams=1, deterministic=True), free)


def test_ids_and_embedding_prompts_return_the_same_tokens(dev, model):
    ids, am = _prompts(dev)
    kw = dict(attention_mask=am, max_new_tokens=6, num_beams=3, num_return_sequences=2, deterministic=True, return_scores=True)
    a, sa = model.beam_search(input_ids=ids, **kw)
    b, sb = model.beam_search(input_embeddings=model.llm.model.embed_tokens(ids).float(), **kw)
    assert a.shape == (6, ids.shape[1] + 6) and b.shape == (6, 6)
    assert torch.equal(a[:, :ids.shape[1]], ids.repeat_interleave(2, dim=0)) and torch.equal(a[:, ids.shape[1]:], b) and torch.equal(sa, sb)
    assert (sa[0::2] >= sa[1::2]).all()                                       # best first within a prompt


def test_beam_search_leaves_no_state_behind(dev, model):
    ids, am = _prompts(dev)
    L = ids.shape[1]
    allow = (torch.tril(torch.ones(L, L, dtype=torch.bool, device=dev))[None] & am.bool()[:, None, :]) | torch.eye(L, dtype=torch.bool, device=dev)[None]
    mm = additive(allow.cpu()).reshape(3, 1, L, L).to(dev)

    def calls():
        out = [model.generate(input_ids=ids, attention_mask=am, max_new_tokens=8, do_sample=False, deterministic=True, on_device=on)
               for on in (False, True)]
        rows = model.mmu_generate_batch(ids, attention_mask=mm, max_new_tokens=8, temperature=0.0, deterministic=True)
        out.append([[int(t) for t in r] for r in rows])
        return out

    before = calls()
    model.beam_search(input_ids=ids, attention_mask=am, max_new_tokens=8, num_beams=4, deterministic=True)
    for x, y in zip(before, calls()):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y
