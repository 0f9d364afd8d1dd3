"""CPU: the yardsticks of the per-token log-probabilities.  (1) models/sampling.py: token_logprobs -- what the host text loops and
the unfused branch of t2i_generate_ar record -- against torch.log_softmax in float64 on the processed scores, within 1e-6: rows with
ties, -inf entries from top-k / top-p, a repetition penalty, finished rows (exactly 0.0).  The rows are 0.5 * randn over 37 entries,
so every log-probability lies in (-8, 0]: the fp32 formula rounds the difference to the maximum (half an ulp below 4: 1.2e-7), the sum
and its log (a few 1e-7 relative to a value below 4) and the final difference (half an ulp below 8: 2.4e-7) -- under 7e-7 together.
(2) logprob_ref.kept_logprob, the float64 restatement the GPU tests use, against truncation_ref on the kept set.  (3) with_logprobs
composed with emit_until_stop and with_repetition_penalty through text_token_loop on a stand-in engine: the recorded values are
those of the scores each pick saw, a finished row records 0.0 from the step after its stop id."""
import math

import torch

import logprob_ref as lref
import truncation_ref as ref


def _rows(seed=3, R=6, V=37):
    g = torch.Generator().manual_seed(seed)
    rows = 0.5 * torch.randn(R, V, generator=g)
    rows[1] = (rows[1] * 4).round() / 4                         # long runs of equal values
    rows[2, 5:9] = rows[2].max()                                # a run of equal maxima
    return rows, g


def test_token_logprobs_is_the_log_softmax_of_the_processed_scores():
    from models.sampling import apply_repetition_penalty, token_logprobs, top_k_top_p_filtering, truncate_logits
    rows, g = _rows()
    R, V = rows.shape
    seen = torch.rand(R, V, generator=g) < 0.3
    processed = {
        "plain": rows.clone(),
        "penalty": apply_repetition_penalty(rows, seen, 1.3),
        "top_k_top_p": top_k_top_p_filtering((apply_repetition_penalty(rows, seen, 1.3) / 0.8).clone(), top_k=9, top_p=0.9),
        "value_thresholds": truncate_logits(rows / 0.8, top_k=12, top_p=0.7, min_p=0.05),
    }
    assert bool(torch.isinf(processed["top_k_top_p"]).any()) and bool(torch.isinf(processed["value_thresholds"]).any())
    for name, s in processed.items():
        finite = torch.isfinite(s)
        picks = [s.argmax(-1), torch.stack([finite[r].nonzero()[-1, 0] for r in range(R)]),
                 torch.multinomial(torch.softmax(s, -1), 1, generator=g)[:, 0]]
        for tok in picks:
            want = torch.log_softmax(s.double(), -1).gather(1, tok[:, None])[:, 0]
            got = token_logprobs(s, tok)
            got2 = token_logprobs(s, tok[:, None])               # [R, 1], as the loops hand the picks over
            assert got.dtype == torch.float32 and got.shape == (R,) and torch.equal(got, got2)
            err = float((got.double() - want).abs().max())
            print(f"{name}: max |helper - float64 log_softmax| = {err:.3e}, values in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
            assert err <= 1e-6, (name, err)
            assert bool((got <= 0).all())
            for r in range(R):                                   # the float64 restatement of the GPU tests says the same
                assert abs(lref.kept_logprob(s[r], int(tok[r])) - float(want[r])) <= 1e-12
            done = torch.tensor([False, True, False, True, True, False])
            masked = token_logprobs(s, tok, done)
            assert torch.equal(masked[done], torch.zeros(3)) and torch.equal(masked[~done], got[~done])
            assert all(math.copysign(1.0, float(x)) == 1.0 for x in masked[done])       # exactly +0.0
    # a NaN is no candidate: it adds nothing
    s = rows.clone()
    s[0, 3] = float("nan")
    keep = torch.ones(V, dtype=torch.bool)
    keep[3] = False
    tok = torch.tensor([7])
    want = torch.log_softmax(s[0, keep].double(), -1)[6]         # (index 7 of the row is index 6 of the row without entry 3)
    assert abs(float(token_logprobs(s[:1], tok)[0]) - float(want)) <= 1e-6
    assert abs(lref.kept_logprob(s[0], 7) - float(want)) <= 1e-12


def test_restatement_agrees_with_truncation_ref_on_the_kept_set():
    rows, _ = _rows(seed=8, R=4, V=600)
    rows = rows.double() / 0.8
    for top_k, top_p, min_p in [(0, 1.0, 0.0), (50, 0.9, 0.05), (0, 0.5, 0.0), (1, 1.0, 0.0), (200, 0.8, 0.02)]:
        for b in range(rows.shape[0]):
            v = rows[b]
            t = ref.tau(v, top_k, top_p, min_p)
            keep = v >= t
            ex = torch.where(keep, torch.exp(v - v.max()), torch.zeros_like(v))
            T = float(ex.sum())
            for token in (int(v.argmax()), int(keep.nonzero()[-1, 0]), int(keep.nonzero()[len(keep.nonzero()) // 2, 0])):
                assert bool(keep[token])
                want = math.log(float(ex[token]) / T)            # the probability truncation_ref.draw_ok's intervals give the token
                got = lref.kept_logprob(v, token, t)
                assert abs(got - want) <= 1e-12 and got <= 0.0, (top_k, top_p, min_p, b, token)
            ls = torch.log_softmax(torch.where(keep, v, torch.full_like(v, float("-inf"))), -1)
            assert abs(lref.kept_logprob(v, int(v.argmax()), t) - float(ls.max())) <= 1e-12
    # done_before: zero from the step AFTER a row's first stop id
    toks = torch.tensor([[4, 9, 1, 1], [9, 1, 1, 1], [3, 4, 5, 6]])
    assert lref.done_before(toks, [9]).tolist() == [[False, False, True, True], [False, True, True, True], [False] * 4]


def test_with_logprobs_records_what_each_pick_saw():
    from models.sampling import apply_repetition_penalty
    from models.unigen import emit_until_stop, text_token_loop, with_logprobs, with_repetition_penalty
    g = torch.Generator().manual_seed(21)
    R, V, n, stop_id, pad = 3, 37, 6, 11, 0
    table = 0.5 * torch.randn(n, R, V, generator=g)              # the stand-in engine: step i's scores, whatever was fed
    table[2, 1, stop_id] = 9.0                                   # row 1 emits the stop id at step 2
    for penalty in (1.0, 1.3):
        out = torch.zeros((R, n), dtype=torch.long)
        logp = torch.full((R, n), 7.0)
        emit = emit_until_stop(out, torch.tensor([stop_id]), pad)
        pick, emit = with_logprobs(lambda last: last / 0.8, lambda s: s.argmax(-1, keepdim=True), emit, logp)
        seen = torch.zeros((R, V), dtype=torch.bool)
        seen[:, :5] = True
        want_seen = seen.clone()
        if penalty != 1.0:
            pick, emit = with_repetition_penalty(pick, emit, penalty, seen)
        steps = text_token_loop(n, 0, pick, emit, head=lambda i: table[i].clone(), embed=lambda ids: ids, step=lambda ids, c=[0]: c.__setitem__(0, c[0] + 1) or c[0])
        assert steps == n
        for i in range(n):
            s = table[i] if penalty == 1.0 else apply_repetition_penalty(table[i], want_seen, penalty)
            s = s / 0.8
            tok = s.argmax(-1)
            want = torch.log_softmax(s.double(), -1).gather(1, tok[:, None])[:, 0]
            for r in range(R):
                if r == 1 and i > 2:
                    assert float(logp[r, i]) == 0.0 and int(out[r, i]) == pad
                else:
                    assert int(out[r, i]) == int(tok[r]) and abs(float(logp[r, i]) - float(want[r])) <= 1e-6, (penalty, r, i)
            want_seen.scatter_(1, out[:, i:i + 1], True)
        assert int(out[1, 2]) == stop_id and float(logp[1, 2]) < 0.0           # the step that emits the stop id keeps its value
