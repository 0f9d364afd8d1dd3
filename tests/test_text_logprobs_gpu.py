"""Per-token log-probabilities of text generation: ug_text_pick_logp / ug_text_sample_logp (csrc/text_sampler.hip) through
ops.text_pick_(..., logp=) / ops.text_sample_(..., logp=), and generate / mmu_generate / mmu_generate_batch with return_logprobs=True
on both loops, against the float64 restatement in logprob_ref.py.

Tolerance: logprob_ref.TOL = 1e-4 absolute, derived in the header of tests/test_ar_logprobs_gpu.py (the longest chain counted there is
this file's greedy pick over 159 867 entries: about 1e-5 on the sum, 2e-5 in all).  Inputs keep |v - max| below 64.  The two loops are
each held to their own formula -- the device loop on the bf16-rounded processed scores of its traced head logits, the host loop on the
scores it picks from -- and are not compared with each other: their heads round differently.

The kernel tests also hold the new entry points to the old ones bit for bit on everything the old ones write."""
import pytest
import torch

import logprob_ref as lref
import truncation_ref as ref
from helpers import additive, golden, llm_config_dir
from repetition_penalty_ref import Bitmap

pytestmark = pytest.mark.gpu

TOL = lref.TOL
SETTINGS = [(50, 1.0), (0, 0.9), (200, 0.8), (1, 1.0), (0, 0.5), (1000, 0.95)]          # tests/test_text_sample_gpu.py
TEMP = 0.8
FORMS = ["greedy"] + list(range(len(SETTINGS)))


# ------------------------------------------------------------------ kernels through ops
@pytest.mark.parametrize("V,vec", [(159867, True), (5000, True), (5001, False)])
@pytest.mark.parametrize("form", FORMS)
def test_text_logp_entries_match_restatement_and_the_old_entries(dev, V, vec, form):
    from unigen_hip import ops
    greedy = form == "greedy"
    top_k, top_p = (0, 1.0) if greedy else SETTINGS[form]
    R, H, n, pad = 6, 64, 5, 5
    ld = ops.round_up(V, 8) if vec else V                        # (ld = 5001: rows off 16-byte boundaries, the scalar form of the pick)
    g = torch.Generator().manual_seed(400 + FORMS.index(form))
    logits = torch.full((n, R, ld), 1e30)                        # entries V .. ld-1 must never count
    logits[:, :, :V] = 0.5 * torch.randn(n, R, V, generator=g)
    logits[:, 0, 17] = float("nan")                              # no candidate: adds nothing
    logits[:, 3, 23] = float("-inf")                             # adds 0
    logits[:, 4, 200:204] = 2.75                                 # a run of equal values near the top
    emb = torch.randn(V, H, generator=g)
    u = torch.rand(n, R, generator=g)
    u[0, 0] = 0.0
    u[1, 0] = 1.0 - 2.0 ** -24
    emb_d, u_d = emb.to(dev), u.to(dev)

    def run(with_logp, stop):
        ws = None if greedy else ops.text_sample_workspace(R, dev)
        state = ops.text_state(R, dev)
        tok = torch.zeros(R, dtype=torch.long, device=dev)
        out = torch.full((R, n), -1, dtype=torch.int32, device=dev)
        lengths = torch.full((R,), n, dtype=torch.int32, device=dev)
        x = torch.zeros(R, H, device=dev)
        logp = torch.full((R, n), 7.0, device=dev) if with_logp else None
        kw = dict(stop_ids=None if stop is None else torch.tensor([stop], dtype=torch.long, device=dev), pad_id=None if stop is None else pad,
                  lengths=lengths, logp=logp)
        steps = []
        for step in range(n):
            clear = step == n - 1
            lg = logits[step].to(dev)
            stats = torch.full((R, 2), -1.0, device=dev)
            if greedy:
                ops.text_pick_(lg, V, state, n, emb_d, tok, out, x, clear=clear, **kw)
            else:
                ops.text_sample_(lg, V, state, n, emb_d, tok, out, x, u_d, ws, temperature=TEMP, top_k=top_k, top_p=top_p, clear=clear, stats=stats, **kw)
                assert int(ws.abs().max()) == 0                                   # the workspace is all zero after every step
            lg = lg.cpu()
            assert torch.equal(lg[:, V:], logits[step][:, V:])
            want_lg = torch.zeros(R, V) if clear else logits[step][:, :V]         # `clear` behaves as before
            assert torch.equal(lg[:, :V].view(torch.int32), want_lg.contiguous().view(torch.int32))
            steps.append((tok.cpu().clone(), x.cpu().clone(), stats.cpu(), state.cpu().clone()))
        return steps, out.cpu(), lengths.cpu(), None if logp is None else logp.cpu()

    free = run(False, None)
    stop = int(free[1][2, 1])                                    # the token row 2 emits at step 1: that row finishes there
    old, new, again = run(False, stop), run(True, stop), run(True, stop)
    assert torch.equal(old[1], new[1]) and torch.equal(old[2], new[2]) and torch.equal(new[1], again[1])
    for step in range(n):
        for a, b_, c in zip(old[0][step], new[0][step], again[0][step]):
            assert torch.equal(a, b_) and torch.equal(a, c)                       # token, x, stats, state: bit-equal
    logp, tokens = new[3], new[1].long()
    assert torch.equal(logp, again[3])                                           # bit-reproducible
    done = lref.done_before(tokens, [stop])
    assert bool(done[2, 2:].all()) and not bool(done[2, 1]) and int(tokens[2, 1]) == stop and int(new[2][2]) <= 2
    picked = torch.stack([free[0][s][0] for s in range(n)], 1)                    # what the kernel picked before the pad rule
    worst = 0.0
    for step in range(n):
        v = lref.bf16_values(logits[step][:, :V], None if greedy else TEMP)
        stats = new[0][step][2]
        for r in range(R):
            got = float(logp[r, step])
            if bool(done[r, step]):
                assert got == 0.0 and int(tokens[r, step]) == pad, (form, V, step, r, got)
                continue
            tok = int(tokens[r, step])
            assert tok == int(picked[r, step])                                    # (rows are independent: the free run's token)
            tau = lref.NEG if greedy else float(stats[r, 0])
            want = lref.kept_logprob(v[r], tok, tau)
            ok = ~torch.isnan(v[r])
            print(f"{form} V {V} step {step} row {r}: token {tok}, logprob {got!r} (float64 {want!r}, diff {abs(got - want):.2e}), tau {tau!r}")
            assert float(v[r][ok & torch.isfinite(v[r])].max() - v[r][ok & torch.isfinite(v[r])].min()) < 64
            assert got <= 0.0 and abs(got - want) <= TOL, (form, V, step, r, got, want)
            worst = max(worst, abs(got - want))
    if top_k != 1:                                                                # (top_k = 1 keeps the maximum alone: its real value IS 0)
        assert float(logp[2, 1]) < 0.0                                            # the step that emits the stop id keeps its real value
    print(f"{form} V {V}: worst difference {worst:.2e}")


def test_text_logp_entries_reject_a_null_output(dev):
    from unigen_hip import lib, ops
    from unigen_hip.lib import UniGenHipError
    R, V, H, n = 2, 64, 64, 4
    logits = torch.ones(R, V, device=dev)
    emb = torch.zeros(V, H, device=dev)
    ws, state = ops.text_sample_workspace(R, dev), ops.text_state(R, dev)
    tok = torch.zeros(R, dtype=torch.long, device=dev)
    out = torch.zeros((R, n), dtype=torch.int32, device=dev)
    x = torch.zeros(R, H, device=dev)
    u = torch.zeros(n, R, device=dev)
    p, L = ops._p, lib.load()
    tail = (*ops._text_out(None, None, emb), p(state), n, p(tok), p(out), None, p(x))
    with pytest.raises(UniGenHipError, match="null logp"):
        lib.check(L.ug_text_pick_logp(p(logits), V, R, V, 1, *tail, None, ops._stream()), "ug_text_pick_logp")
    with pytest.raises(UniGenHipError, match="null logp"):
        lib.check(L.ug_text_sample_logp(p(logits), V, R, V, 1, 1.0, 0, 1.0, p(u), p(ws), None, *tail, None, ops._stream()), "ug_text_sample_logp")
    with pytest.raises(UniGenHipError, match="shape"):
        ops.text_pick_(logits, V, state, n, emb, tok, out, x, clear=True, logp=torch.zeros(R, n + 1, device=dev))
    with pytest.raises(UniGenHipError):
        ops.text_sample_(logits, V, state, n, emb, tok, out, x, u, ws, top_p=0.0, logp=torch.zeros(R, n, device=dev))
    torch.cuda.synchronize()
    assert int(state[0]) == 0 and float(logits.min()) == 1.0 and int(ws.abs().max()) == 0          # a refused call launches nothing


# ------------------------------------------------------------------ model level (fixtures of tests/test_text_generate_gpu.py)
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
    from models import UniGen
    from oracle import weights
    g = golden("g9_generate.pt")
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=g["weight_std"]), strict=False)
    return m.eval()


def _prompts(dev, lens=(40, 27, 33), hi=2000, seed=4):
    """left-padded rows -> (ids [R, L], attention mask [R, L], dense additive mmu masks [R, 1, L, L])"""
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.zeros((len(lens), L), dtype=torch.long)
    am = torch.zeros((len(lens), L), dtype=torch.long)
    for r, n in enumerate(lens):
        ids[r, L - n:] = torch.randint(1, hi, (n,), generator=g)
        am[r, L - n:] = 1
    allow = (torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & am.bool()[:, None, :]) | torch.eye(L, dtype=torch.bool)[None]
    return ids.to(dev), am.to(dev), additive(allow).reshape(len(lens), 1, L, L).to(dev)


MODES = {"greedy": dict(), "greedy_penalty": dict(repetition_penalty=1.3),
         "sampled": dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8)}


def _check_device_rows(trace, tokens, logp, V, ids, am, penalty=1.0, sampling=None, stops=(), tag=""):
    """the device loop's contract on its traced RAW head logits: the repetition penalty's device rule (repetition_penalty_ref.Bitmap),
    the bf16 rounding, for a sampled run the temperature and the kept set at either end of truncation_ref.tau_bracket.  tokens / logp
    [R, steps] as returned; a row that had emitted a stop id before a step has exactly 0.0 there."""
    tokens, logp = tokens.cpu(), logp.cpu()
    R, steps = tokens.shape
    assert logp.shape == tokens.shape and logp.dtype == torch.float32 and len(trace) >= steps
    done = lref.done_before(tokens, stops)
    bm = Bitmap(R, V).mark(ids.cpu(), am.cpu()) if penalty != 1.0 else None
    real = 0
    for i in range(steps):
        lg = trace[i].cpu().float()
        if bm is not None:
            lg = bm.penalize(lg, penalty, tok=None if i == 0 else tokens[:, i - 1])
        v = lref.bf16_values(lg, None if sampling is None else sampling[0])
        for r in range(R):
            got = float(logp[r, i])
            if bool(done[r, i]):
                assert got == 0.0, (tag, i, r, got)
                continue
            tok = int(tokens[r, i])
            taus = (lref.NEG,) if sampling is None else ref.tau_bracket(v[r].double(), sampling[1], sampling[2])
            wants = [lref.kept_logprob(v[r], tok, t) for t in taus if bool(v[r][tok] >= t)]
            print(f"{tag} step {i} row {r}: token {tok}, logprob {got!r} (float64 {wants!r})")
            assert wants and got <= 0.0 and min(abs(got - w) for w in wants) <= TOL, (tag, i, r, got, wants)
            real += 1
    return real


@pytest.mark.parametrize("which", ["m1p5", "msmall"])
@pytest.mark.parametrize("mode", list(MODES))
def test_on_device_generate_logprobs_eager_graph_session_and_stop(dev, request, which, mode):
    model = request.getfixturevalue(which)
    eng = model.llm.engine
    ids, am, _ = _prompts(dev, hi=2000 if which == "m1p5" else 300)
    L, n, V = ids.shape[1], 12, model.config.vocab_size
    mk = MODES[mode]
    penalty = mk.get("repetition_penalty", 1.0)
    sampling = (0.8, 50, 0.9) if "do_sample" in mk else None
    model.drop_decode_session()

    def run(**kw):
        gen = torch.Generator(device=dev).manual_seed(13) if sampling else None
        return model.generate(input_ids=ids, attention_mask=am, max_new_tokens=n, deterministic=True, on_device=True, generator=gen, **mk, **kw)
    plain = run(use_graph=False)
    trace = []
    seqs, lp = run(use_graph=False, trace=trace, return_logprobs=True)
    assert eng.last_text_decode_on_device and torch.equal(seqs, plain) and lp.shape == (3, n) and lp.is_cuda
    assert _check_device_rows(trace, seqs[:, L:], lp, V, ids, am, penalty, sampling, tag=f"{which} {mode}") == 3 * n
    c0 = getattr(eng, "text_graph_captures", 0)
    captured = run(return_logprobs=True)
    sess = eng._text_session
    assert eng.last_decode_graph and sess is not None and sess.logp is not None and sess.key[-1] == "logprobs"
    kept = run(return_logprobs=True)
    assert eng._text_session is sess and eng.text_graph_captures == c0 + 1
    for got in (captured, kept):
        assert torch.equal(got[0], seqs) and torch.equal(got[1], lp)             # bit for bit the eager run's
    off = run()                                                                  # flag off: another session, the same tokens
    assert torch.is_tensor(off) and torch.equal(off, seqs)
    assert eng._text_session is not sess and eng._text_session.logp is None and eng._text_session.key == sess.key[:-1]
    # a stop id taken from the free run: finished rows record 0.0 and the result is cut where the tokens are
    stop, pad = int(seqs[0, L + 3]), 0
    strace = []
    sseqs, slp = run(use_graph=False, trace=strace, return_logprobs=True, eos_token_id=stop, pad_token_id=pad)
    gseqs, glp = run(return_logprobs=True, eos_token_id=stop, pad_token_id=pad)
    assert torch.equal(sseqs, gseqs) and torch.equal(slp, glp) and slp.shape == (3, sseqs.shape[1] - L)
    first = (seqs[0, L:] == stop).nonzero()[0, 0].item()
    assert bool((slp[0, first + 1:] == 0).all()) and float(slp[0, first]) < 0.0
    _check_device_rows(strace, sseqs[:, L:], slp, V, ids, am, penalty, sampling, stops=[stop], tag=f"{which} {mode} stop")
    model.drop_decode_session()


@pytest.mark.parametrize("mode", list(MODES))
def test_host_loop_generate_logprobs(dev, m1p5, mode):
    """the host loop on the scores it picks from: engine.head_slice is wrapped on the instance to record them; fp32 copy -> penalty ->
    temperature -> top-k / top-p as -inf, then the restatement"""
    from models.sampling import apply_repetition_penalty, seen_mask_of, top_k_top_p_filtering
    model, eng = m1p5, m1p5.llm.engine
    ids, am, _ = _prompts(dev)
    L, n, V = ids.shape[1], 12, model.config.vocab_size
    mk = MODES[mode]
    penalty = mk.get("repetition_penalty", 1.0)

    def run(**kw):
        gen = torch.Generator(device=dev).manual_seed(13) if "do_sample" in mk else None
        return model.generate(input_ids=ids, attention_mask=am, max_new_tokens=n, deterministic=True, on_device=False, generator=gen, **mk, **kw)
    plain = run()
    seen_scores, orig = [], eng.head_slice
    eng.head_slice = lambda *a, **k: (seen_scores.append(orig(*a, **k)), seen_scores[-1])[1]
    try:
        seqs, lp = run(return_logprobs=True)
    finally:
        del eng.head_slice
    assert not eng.last_text_decode_on_device and torch.equal(seqs, plain) and lp.shape == (3, n) and len(seen_scores) == n
    toks = seqs[:, L:]
    seen = seen_mask_of(ids, am != 0, 3, V, dev)
    for i in range(n):
        s = seen_scores[i].float()
        if penalty != 1.0:
            s = apply_repetition_penalty(s, seen, penalty)
            seen.scatter_(1, toks[:, i:i + 1], True)
        if "do_sample" in mk:
            s = top_k_top_p_filtering(s / 0.8, top_k=50, top_p=0.9)
        for r in range(3):
            want = lref.kept_logprob(s[r].cpu(), int(toks[r, i]))
            got = float(lp[r, i])
            print(f"host {mode} step {i} row {r}: token {int(toks[r, i])}, logprob {got!r} (float64 {want!r})")
            assert got <= 0.0 and abs(got - want) <= TOL, (mode, i, r, got, want)
    # a stop id: the pad ids behind it record 0.0, cut with the tokens
    stop = int(toks[0, 3])
    sseqs, slp = run(return_logprobs=True, eos_token_id=stop, pad_token_id=0)
    assert slp.shape == (3, sseqs.shape[1] - L)
    done = lref.done_before(sseqs[:, L:].cpu(), [stop])
    assert bool(done.any()) or sseqs.shape[1] - L < n
    assert bool((slp.cpu()[done] == 0).all()) and bool((slp.cpu()[~done] < 0).all())
    assert torch.equal(slp[~done.to(dev)], lp[:, :slp.shape[1]][~done.to(dev)])   # (deterministic rows are independent)


def test_mmu_paths_and_num_return_sequences(dev, m1p5):
    model, eng = m1p5, m1p5.llm.engine
    ids, am, mm = _prompts(dev)
    n, V = 12, model.config.vocab_size
    model.drop_decode_session()
    for on_device in (True, False):
        mkw = dict(max_new_tokens=n, temperature=0.0, deterministic=True, on_device=on_device)
        plain = model.mmu_generate(idx=ids[:1], attention_mask=mm[0], **mkw)
        trace = []
        toks, lp = model.mmu_generate(idx=ids[:1], attention_mask=mm[0], return_logprobs=True, use_graph=False, trace=trace, **mkw)
        assert [int(t) for t in toks] == [int(t) for t in plain] and len(toks) == n and lp.shape == (n,) and lp.is_cuda and bool((lp < 0).all())
        eot = int(toks[4])
        ctoks, clp = model.mmu_generate(idx=ids[:1], attention_mask=mm[0], eot_token=eot, return_logprobs=True, **mkw)
        cut = [int(t) for t in toks].index(eot) + 1
        assert [int(t) for t in ctoks] == [int(t) for t in toks][:cut] and torch.equal(clp, lp[:cut])
        if on_device:
            one = torch.tensor([[int(t) for t in toks]])
            assert _check_device_rows(trace, one, lp[None], V, ids[:1], am[:1], tag="mmu_generate") == n
        # the batch: per-row cuts
        btrace = []
        lists, lps = model.mmu_generate_batch(idx=ids, attention_mask=mm, return_logprobs=True, use_graph=False, trace=btrace, **mkw)
        beot = int(lists[1][2])
        clists, clps = model.mmu_generate_batch(idx=ids, attention_mask=mm, eot_token=beot, return_logprobs=True, **mkw)
        assert len(lps) == len(clps) == 3 and len(clists[1]) <= 3
        for r in range(3):
            row = [int(t) for t in lists[r]]
            want = row[:row.index(beot) + 1] if beot in row else row
            assert [int(t) for t in clists[r]] == want and lps[r].shape == (n,) and clps[r].shape == (len(want),)
            assert torch.equal(clps[r], lps[r][:len(want)]) and bool((clps[r] < 0).all())
        if on_device:
            full = torch.tensor([[int(t) for t in r] for r in lists])
            assert _check_device_rows(btrace, full, torch.stack(lps), V, ids, am, tag="mmu_generate_batch") == 3 * n
        # a sampled mmu call: temperature and top-k reach the log-probability
        strace = []
        stoks, slp = model.mmu_generate(idx=ids[:1], attention_mask=mm[0], max_new_tokens=6, temperature=0.8, top_k=50, deterministic=True,
                                        on_device=on_device, use_graph=False, return_logprobs=True, trace=strace)
        assert len(stoks) == 6 and slp.shape == (6,) and bool((slp <= 0).all())
        if on_device:
            _check_device_rows(strace, torch.tensor([[int(t) for t in stoks]]), slp[None], V, ids[:1], am[:1], sampling=(0.8, 50, 1.0), tag="mmu sampled")
        # num_return_sequences = 2: 2 B rows of log-probabilities
        gen = torch.Generator(device=dev).manual_seed(3)
        seqs, glp = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=6, do_sample=True, top_k=50, temperature=0.8, generator=gen,
                                   num_return_sequences=2, deterministic=True, on_device=on_device, return_logprobs=True)
        assert seqs.shape == (6, ids.shape[1] + 6) and glp.shape == (6, 6) and bool((glp <= 0).all()) and eng.last_text_decode_on_device == on_device
    model.drop_decode_session()
