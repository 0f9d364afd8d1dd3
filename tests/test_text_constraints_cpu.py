"""logit_bias, suppress_tokens, min_new_tokens, no_repeat_ngram_size and stop_sequences without a GPU: the host functions
(models/sampling.py) against transformers' own logits processors and against the plain-Python restatement (text_constraints_ref.py),
the host token loop with every wrapper on a scripted head, the argument checks, and the new C entries' presence and validation."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import repetition_penalty_ref as pref
import text_constraints_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")
CPU = torch.device("cpu")


# ------------------------------------------------------------------ against transformers
def _scores(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    s = 4.0 * torch.randn(R, V, generator=g)
    s[:, 0], s[:, V - 1], s[:, 3] = -2.5, 3.25, 0.0
    return s


@pytest.mark.parametrize("L", [1, 2, 3, 12, 40])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_host_functions_are_transformers_processors(n, L):
    """rows whose prompt ids are all valid: input_ids IS the history.  Ids from {0 .. 4} so that n-grams repeat; L in {1, 2} is shorter
    than n - 1 for n in {3, 4} / {4}: nothing is banned there."""
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              SequenceBiasLogitsProcessor, SuppressTokensLogitsProcessor)
    from models.sampling import apply_constraints, apply_logit_bias, apply_repetition_penalty, history_of, ngram_banned, seen_mask_of
    R, V = 6, 50
    g = torch.Generator().manual_seed(100 * n + L)
    ids = torch.randint(0, 5, (R, L), generator=g)
    s = _scores(R, V, seed=L)
    hist = history_of(ids, None, R, V)
    assert hist == ids.tolist()
    # the n-gram block alone
    want = NoRepeatNGramLogitsProcessor(n)(ids, s.clone())
    got = apply_constraints(s, ngram=n, histories=hist)
    assert torch.equal(got, want), (n, L)
    if L < n - 1:
        assert torch.equal(got, s) and all(ngram_banned(h, n) == [] for h in hist)
    elif n == 1:
        assert all(bool((got[r, ids[r]] == NINF).all()) for r in range(R))
    # sequence bias with keys of length 1; suppress; min-new-tokens below, at and above the bound
    bias = {0: -1.75, 7: 2.5, V - 1: 0.3}
    want = SequenceBiasLogitsProcessor({(e,): b for e, b in bias.items()})(ids, s.clone())
    assert torch.equal(apply_logit_bias(s, list(bias), list(bias.values())), want)
    assert torch.equal(apply_constraints(s, bias=sorted(bias.items())), want)
    sup = [2, 9, V - 2]
    want = SuppressTokensLogitsProcessor(sup, device="cpu")(ids, s.clone())
    assert torch.equal(apply_constraints(s, bias=[(e, NINF) for e in sup]), want)
    eos, m = [4, 11], 3
    for emitted in (0, 2, 3, 5):
        so_far = torch.cat([ids, torch.ones((R, emitted), dtype=torch.long)], dim=1)       # (the processor reads cur_len - prompt length)
        want = MinNewTokensLengthLogitsProcessor(L, m, eos, device="cpu")(so_far, s.clone())
        assert torch.equal(apply_constraints(s, banned=eos if emitted < m else ()), want), emitted
        assert bool((want[:, eos] == NINF).all()) == (emitted < m)
    # everything in transformers' order (bias, penalty, n-gram, min-new, suppress) = all constraints first, then the penalty
    p = 1.3
    want = s.clone()
    for proc in (SequenceBiasLogitsProcessor({(e,): b for e, b in bias.items()}), RepetitionPenaltyLogitsProcessor(p),
                 NoRepeatNGramLogitsProcessor(n), MinNewTokensLengthLogitsProcessor(L, m, eos, device="cpu"),
                 SuppressTokensLogitsProcessor(sup, device="cpu")):
        want = proc(ids, want)
    both = sorted(list(bias.items()) + [(e, NINF) for e in sup])
    got = apply_repetition_penalty(apply_constraints(s, bias=both, banned=eos, histories=hist, ngram=n), seen_mask_of(ids, None, R, V, CPU), p)
    assert torch.equal(got, want), (n, L)


# ------------------------------------------------------------------ against the restatement, left-padded rows
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_host_functions_equal_the_restatement_on_left_padded_rows(n):
    from models.sampling import apply_constraints, history_of, ngram_banned, stop_sequence_hit
    R, V, L = 5, 77, 23
    g = torch.Generator().manual_seed(n)
    ids = torch.randint(0, 4, (R, L), generator=g)
    valid = torch.ones(R, L, dtype=torch.bool)
    for r in range(R):
        valid[r, :4 * r] = False                                     # left padding; row 4 keeps 7 ids
        ids[r, :4 * r] = 3                                           # (pads hold a real id: they must not count)
    ids[1, L - 3], ids[2, L - 2], ids[3, L - 5] = -1, V, 1 << 40     # ids the penalty does not count either
    hist = history_of(ids, valid, R, V)
    for r in range(R):
        want = [int(e) for e, ok in zip(ids[r].tolist(), valid[r].tolist()) if ok and 0 <= e < V]
        assert hist[r] == want and sorted(ngram_banned(hist[r], n)) == sorted(ref.ngram_bans(want, n)), r
    assert history_of(None, None, R, V) == [[] for _ in range(R)]
    s = _scores(R, V, seed=7)
    bias = sorted({0: 1.5, 5: -0.25, V - 1: 1e-3, 9: NINF, 2: NINF}.items())
    for banned in ((), (1, 76)):
        got = apply_constraints(s, bias=bias, banned=banned, histories=hist, ngram=n)
        for r in range(R):
            want = torch.tensor(ref.host_rule(s[r].tolist(), bias, banned, hist[r], n))
            assert pref.same_bits(got[r], want), (n, r, banned)
    assert pref.same_bits(apply_constraints(s), s)
    # the stop matcher
    seqs = [(1, 2), (3, 1, 2), (5,)]
    for emitted in ([], [2], [1, 2], [0, 1, 2], [3, 1, 2], [1, 2, 0], [5], [0, 5], [5, 0], [2, 1]):
        assert stop_sequence_hit(emitted, seqs) == ref.tail_matches(emitted, seqs), emitted
    assert stop_sequence_hit([1, 2], seqs) and not stop_sequence_hit([2], seqs) and not stop_sequence_hit([1, 2, 0], seqs)


# ------------------------------------------------------------------ the host loop with every wrapper, scripted head
EOS, PAD, P = 2, 0, 1.3
SEQS = [(21, 22), (20, 21, 22)]
CONS = dict(logit_bias={3: 2.0, 7: -1.5}, suppress_tokens=[5], min_new_tokens=3, no_repeat_ngram_size=2, stop_sequences=SEQS)


def _script():
    """10 steps x 3 rows x 40 ids: small noise, 10.0 at the step's target, 8.0 at a second choice, 9.0 at the biased id 3 now and then"""
    R, V, n = 3, 40, 10
    g = torch.Generator().manual_seed(5)
    targets = [[22, 5, 14, 15, 16, 17, EOS, 18, 19, 23],             # row 0: 22 completes both sequences only THROUGH the prompt
               [20, 21, 22, 24, 25, 26, 27, 28, 29, 30],             # row 1: 20 21 22 completes both sequences at step 2
               [31, EOS, 32, 6, 33, 14, 34, EOS, 35, 36]]            # row 2: EOS wanted at step 1 (held back), then at step 7
    second = [[24, 25, 26, 27, 28, 29, 30, 31, 32, 33], [10, 11, 12, 13, 14, 15, 16, 17, 18, 19], [10, 11, 12, 13, 15, 16, 17, 18, 19, 9]]
    script = 0.1 * torch.randn(n, R, V, generator=g)
    for i in range(n):
        for r in range(R):
            script[i, r, targets[r][i]] = 10.0
            script[i, r, second[r][i]] = 8.0
    script[3, 0, 3] = 9.0                                            # the bias (+2) lifts id 3 over row 0's target at step 3
    prompt = torch.tensor([[9, 20, 21], [8, 1, 4], [6, 6, 6]])
    valid = torch.tensor([[1, 1, 1], [0, 1, 1], [1, 1, 1]], dtype=torch.bool)
    return script, prompt, valid


def _simulate(script, prompt, valid, cons, eos, pad, penalty):
    """the whole loop in plain Python: per row the restated host rule, the penalty in fp32, the lowest argmax, the stop rules"""
    n, R, V = script.shape
    bias = sorted(list(cons["logit_bias"].items()) + [(e, NINF) for e in cons["suppress_tokens"]])
    hist = [[int(e) for e, ok in zip(prompt[r].tolist(), valid[r].tolist()) if ok] for r in range(R)]
    emitted, done, lengths = [[] for _ in range(R)], [False] * R, [n] * R
    toks, lps, procs = [], [], []
    for i in range(n):
        was = list(done)
        row_t, row_lp, row_p = [], [], []
        for r in range(R):
            s = ref.host_rule(script[i, r].tolist(), bias, eos if i < cons["min_new_tokens"] else [], hist[r], cons["no_repeat_ngram_size"])
            for e in set(hist[r]):
                with np.errstate(all="ignore"):
                    s[e] = float(np.float32(s[e]) * np.float32(penalty)) if s[e] < 0 else float(np.float32(s[e]) / np.float32(penalty))
            best = max(range(V), key=lambda e: (s[e], -e))
            lp = 0.0 if was[r] else float(torch.log_softmax(torch.tensor(s, dtype=torch.float64), -1)[best])
            tok = pad if was[r] else best
            row_t.append(tok), row_lp.append(lp), row_p.append(s)
        for r in range(R):
            hist[r].append(row_t[r]), emitted[r].append(row_t[r])
            if not was[r] and (row_t[r] in eos or ref.tail_matches(emitted[r], cons["stop_sequences"])):
                done[r], lengths[r] = True, i + 1
        toks.append(row_t), lps.append(row_lp), procs.append(row_p)
        if all(done):
            break
    return toks, lps, lengths, procs


def _stack_by_hand(V, out, logp, lengths, prompt, valid, process, choose):
    """the wrapper stack composed here, layer by layer -> (pick, emit, emit_until_stop's done)"""
    from models.sampling import history_of, seen_mask_of
    from models.unigen import checked_constraints, emit_until_stop, with_constraints, with_logprobs, with_repetition_penalty
    R = out.shape[0]
    cons, singles = checked_constraints("test", lambda: V, **CONS)
    assert singles == [] and cons["stop_seqs"] == SEQS and cons["bias"] == [(3, 2.0), (5, NINF), (7, -1.5)]
    emit = emit_until_stop(out, torch.tensor([EOS]), PAD, lengths=lengths)
    done = emit.done
    pick, emit = with_logprobs(process, choose, emit, logp)
    pick, emit = with_repetition_penalty(pick, emit, P, seen_mask_of(prompt, valid, R, V, CPU))
    pick, emit = with_constraints(pick, emit, cons, done, history_of(prompt, valid, R, V), stop_ids=[EOS], lengths=lengths)
    return pick, emit, done


def _stack_of_the_call(V, out, logp, lengths, prompt, valid, process, choose):
    """the stack the entry points run: text_pick_emit's, from the TextCall of the same arguments (done: read off the lengths)"""
    from models.unigen import text_call, text_pick_emit
    call = text_call("test", lambda: V, None, (process, choose), EOS, pad_finished=True, pad_token_id=PAD, repetition_penalty=P,
                     return_logprobs=True, **CONS)
    assert call.stop == [EOS] and call.constraints["stop_seqs"] == SEQS and call.constraints["bias"] == [(3, 2.0), (5, NINF), (7, -1.5)]
    pick, emit = text_pick_emit(call, out, V, logp, lengths, prompt, valid)
    return pick, emit, None


def test_host_token_loop_with_every_wrapper_on_a_scripted_head():
    for stack in (_stack_by_hand, _stack_of_the_call):           # the same expectations of both
        _scripted_head_run(stack)


def _scripted_head_run(stack):
    from models.unigen import text_token_loop
    script, prompt, valid = _script()
    n, R, V = script.shape
    out = torch.full((R, n), PAD, dtype=torch.long)
    lengths = torch.full((R,), n, dtype=torch.long)
    logp = torch.zeros((R, n))
    seen_scores = []
    pick, emit, done = stack(V, out, logp, lengths, prompt, valid, lambda last: (seen_scores.append(last.clone()), last)[1],
                             lambda s: s.argmax(-1, keepdim=True))
    counter = iter(range(n))
    steps = text_token_loop(n, None, pick, emit, head=lambda hn: script[next(counter)].clone(), embed=lambda ids: None, step=lambda x: None)
    toks, lps, want_len, procs = _simulate(script, prompt, valid, CONS, [EOS], PAD, P)
    assert steps == len(toks) == 8                                   # row 2's EOS at step 7 ends the loop
    assert out[:, :steps].t().tolist() == toks                       # token-exact
    assert lengths.tolist() == want_len == [7, 3, 8]
    # a sequence that is complete only through the prompt does not fire: row 0 emits 22 behind its prompt's 20 21 and goes on
    assert toks[0][0] == 22 and toks[1][0] != PAD and want_len[0] == 7 and toks[6][0] == EOS
    # both sequences complete at row 1's step 2: the row finishes once, there, and is pad from then on
    assert [t[1] for t in toks[:4]] == [20, 21, 22, PAD] and bool((lengths < n).all() if done is None else done.all())
    # min_new_tokens holds row 2's EOS back at step 1; suppress_tokens takes row 0's target 5 at step 1; the bias lifts 3 at step 3
    assert toks[1][2] == 11 and toks[1][0] == 25 and toks[3][0] == 3
    # the log-probabilities are those of the constrained and penalised scores, 0.0 for a finished row
    for i in range(steps):
        assert pref.same_bits(seen_scores[i], torch.tensor(procs[i])), i
        assert torch.allclose(logp[:, i], torch.tensor(lps[i]), rtol=0, atol=2e-6), (i, logp[:, i].tolist(), lps[i])
    assert logp[1, 3:].abs().max() == 0 and bool((seen_scores[1][:, 5] == NINF).all()) and bool((seen_scores[1][:, EOS] == NINF).all())
    plain = float(torch.log_softmax(script[1, 2], -1)[11])
    assert abs(float(logp[2, 1]) - plain) > 0.1                      # (not the unconstrained distribution's)


def test_a_stop_sequence_of_one_id_is_a_stop_id_and_the_off_state_is_none():
    from models.unigen import checked_constraints
    assert checked_constraints("t", lambda: 1 / 0) == (None, [])     # all off: V is not even asked for
    assert checked_constraints("t", lambda: 10, stop_sequences=[[4], (7,)]) == (None, [4, 7])
    assert checked_constraints("t", lambda: 10, min_new_tokens=0, no_repeat_ngram_size=0, logit_bias={}, suppress_tokens=[]) == (None, [])
    cons, singles = checked_constraints("t", lambda: 10, stop_sequences=[[4], [1, 2]], min_new_tokens=2)
    assert singles == [4] and cons == {"bias": [], "min_new": 2, "ngram": 0, "stop_seqs": [(1, 2)]}


# ------------------------------------------------------------------ argument checks, before any launch
def _fake_model(V=333, hidden=1536, default=False):
    from models.unigen import UniGen
    eng = types.SimpleNamespace(dims=types.SimpleNamespace(hidden_size=hidden))
    return types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=V), text_decode_on_device=default, llm=types.SimpleNamespace(engine=eng),
                                 _stop_list=UniGen._stop_list)


@pytest.mark.parametrize("kw, word", [
    (dict(logit_bias={5: 1.0}, suppress_tokens=[5]), "twice"), (dict(suppress_tokens=[4, 4]), "twice"),
    (dict(logit_bias={333: 1.0}), "outside"), (dict(suppress_tokens=[-1]), "outside"), (dict(stop_sequences=[[1, 400]]), "outside"),
    (dict(logit_bias={3: float("nan")}), "finite"), (dict(logit_bias={3: float("-inf")}), "finite"),
    (dict(min_new_tokens=-1), "at least 0"), (dict(no_repeat_ngram_size=-2), "at least 0"), (dict(stop_sequences=[[]]), "empty")])
def test_every_entry_point_refuses_bad_constraints_before_any_launch(kw, word):
    from models.unigen import UniGen
    from unigen_hip.lib import UniGenHipError
    ids = torch.zeros((1, 4), dtype=torch.long)
    fake = _fake_model()
    with pytest.raises(UniGenHipError, match=word):
        UniGen.generate(fake, input_ids=ids, eos_token_id=2, **kw)
    for fn in (UniGen.mmu_generate, UniGen.mmu_generate_batch):
        with pytest.raises(UniGenHipError, match=word):
            fn(fake, idx=ids, attention_mask=torch.zeros(1, 1, 4, 4), **kw)


def test_generate_needs_an_eos_or_a_pad_for_stop_sequences():
    from models.unigen import UniGen
    from unigen_hip.lib import UniGenHipError
    with pytest.raises(UniGenHipError, match="stop_sequences need"):
        UniGen.generate(_fake_model(), input_ids=torch.zeros((1, 4), dtype=torch.long), stop_sequences=[[1, 2]])


def test_on_device_limits_raise_when_explicit_and_fall_back_when_derived():
    from models.unigen import UniGen, text_call
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    assert (ops.TEXT_MAX_BIAS, ops.TEXT_MAX_NGRAM, ops.TEXT_MAX_STOP_SEQS, ops.TEXT_MAX_STOP_SEQ_LEN) == (1024, 16, 8, 16)
    V = 5000
    cases = [(dict(logit_bias={e: 0.5 for e in range(600)}, suppress_tokens=list(range(600, 1025))), "1025 logit_bias"),
             (dict(no_repeat_ngram_size=17), "no_repeat_ngram_size=17"),
             (dict(stop_sequences=[[e, e + 1] for e in range(9)]), "9 stop sequences"),
             (dict(stop_sequences=[list(range(17))]), "17 ids"),
             (dict(stop_sequences=[[e] for e in range(5)]), "9 stop ids")]      # with the four ids below: singles count as stop ids
    for kw, word in cases:
        call = text_call("generate", lambda: V, None, (None, None), [4000, 4001, 4002, 4003], **kw)
        with pytest.raises(UniGenHipError, match=word):
            UniGen._text_on_device(_fake_model(V), True, call, 3, True, 8)
        assert UniGen._text_on_device(_fake_model(V, default=True), None, call, 3, True, 8) is False
    ok = text_call("generate", lambda: V, None, (None, None), [1], logit_bias={e: 0.5 for e in range(1024)}, no_repeat_ngram_size=16,
                   stop_sequences=[list(range(e, e + 16)) for e in range(8)])
    assert UniGen._text_on_device(_fake_model(V), True, ok, 3, True, 8) is True


# ------------------------------------------------------------------ the C entries
def test_new_entries_are_in_the_library_the_header_and_the_binding():
    from unigen_hip import lib, ops
    header = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ("ug_text_constrain", "ug_text_stop_seq"):
        assert hasattr(L, name) and name in lib.SIGNATURES and f"int {name}(" in header, name
    assert callable(ops.text_constrain_) and callable(ops.text_stop_seq_)
    loaded = lib.load()
    assert loaded.ug_abi_version() == lib.ABI_VERSION == 7
    assert loaded.ug_text_constrain(*([0] * 17)) == -1 and b"ug_text_constrain" in loaded.ug_last_error()
    assert loaded.ug_text_stop_seq(*([0] * 10)) == -1 and b"ug_text_stop_seq" in loaded.ug_last_error()


def test_new_entries_validate_their_arguments_before_any_launch():
    """stand-in addresses (never dereferenced on the host): every call fails its checks, with the entry's name and the reason"""
    from unigen_hip import lib
    L = lib.load()
    p = 4096

    def constrain(**kw):
        a = dict(logits=p, ld=104, R=3, V=100, bias=p, n_bias=2, min_new=0, stop_ids=p, n_stop=1, ngram=2, hist=p, ld_hist=8, hist_len=p,
                 out_tokens=p, nsteps=64, state=p)
        a.update(kw)
        rc = L.ug_text_constrain(*a.values(), 0)
        return rc, L.ug_last_error().decode()

    for kw, word in [(dict(R=33), "bad sizes"), (dict(R=0), "bad sizes"), (dict(V=105), "bad sizes"), (dict(nsteps=0), "bad sizes"),
                     (dict(ld_hist=-1), "bad sizes"), (dict(ld=1 << 30), "bad sizes"), (dict(n_bias=1025), "bad constraints"),
                     (dict(ngram=17), "bad constraints"), (dict(ngram=-1), "bad constraints"), (dict(min_new=-1), "bad constraints"),
                     (dict(n_stop=9), "bad constraints"), (dict(logits=0), "null"), (dict(state=0), "null"), (dict(bias=0), "null"),
                     (dict(stop_ids=0), "null"), (dict(out_tokens=0), "null"), (dict(hist=0), "null"), (dict(hist_len=0), "null")]:
        rc, msg = constrain(**kw)
        assert rc == -1 and msg.startswith("ug_text_constrain") and word in msg, (kw, rc, msg)

    def stop_seq(**kw):
        a = dict(seq_ids=p, seq_off=p, ns=2, n_ids=5, out_tokens=p, nsteps=64, R=3, state=p, lengths=0)
        a.update(kw)
        rc = L.ug_text_stop_seq(*a.values(), 0)
        return rc, L.ug_last_error().decode()

    for kw, word in [(dict(ns=0), "bad sizes"), (dict(ns=9, n_ids=18), "bad sizes"), (dict(n_ids=3), "bad sizes"), (dict(n_ids=33), "bad sizes"),
                     (dict(R=33), "bad sizes"), (dict(nsteps=0), "bad sizes"), (dict(seq_ids=0), "null"), (dict(seq_off=0), "null"),
                     (dict(out_tokens=0), "null"), (dict(state=0), "null")]:
        rc, msg = stop_seq(**kw)
        assert rc == -1 and msg.startswith("ug_text_stop_seq") and word in msg, (kw, rc, msg)
