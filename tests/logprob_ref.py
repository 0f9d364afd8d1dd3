"""Float64 restatements of the per-token log-probability contracts (include/unigen_hip.h: ug_ar_sample_logp,
ug_ar_sample_filtered_logp, ug_text_pick_logp, ug_text_sample_logp), beside truncation_ref.py and text_pick_ref.py.  Written from the
definitions, one row at a time; CPU only.

Every contract is one formula over a row of values v and a kept set {v >= tau}:
    logprob = v[tok] - max v - log(sum over the kept e of exp(v[e] - max v))
A NaN entry is no candidate and contributes nothing; -inf contributes 0.  What differs is how v is formed from the inputs:
  AR image tokens   v = (u~ + s * (c~ - u~)) * fp32(1 / temperature), c~ / u~ the bf16-rounded rows (truncation_ref.mixed_logits);
                    the conditional model's own value takes v = c~ and no threshold;
  text, greedy      v = the bf16-rounded (processed) score, no temperature, no threshold;
  text, sampled     v = bf16round(score) * fp32(1 / temperature), tau as ug_text_sample reports it."""
import math

import torch

NEG = float("-inf")
TOL = 1e-4          # the bound of the GPU tests; derived in tests/test_ar_logprobs_gpu.py's header


def kept_logprob(v, token, tau=NEG):
    """the formula above for one row v (any float dtype, taken to float64) -> python float"""
    v = v.double()
    ok = ~torch.isnan(v)
    mx = float(v[ok].max())
    kept = ok & (v >= tau)
    total = float(torch.exp(v[kept] - mx).sum())
    return float(v[int(token)]) - mx - math.log(total)


def bf16_values(scores, temperature=None):
    """the fp32 values the text kernels form from fp32 scores: rounded to bf16, times fp32(1 / temperature) when sampling"""
    v = scores.float().to(torch.bfloat16).float()
    if temperature is None:
        return v
    return v * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32))


def cond_values(acc, bsz):
    """c~: the bf16-rounded conditional rows of a raw [2 * bsz, V] head accumulator"""
    return acc[:bsz].float().to(torch.bfloat16).float()


def done_before(tokens, stop_ids):
    """tokens [R, n] as emitted (pad ids included) -> bool [R, n]: the row had emitted a stop id BEFORE step i (those entries are 0.0)"""
    hit = torch.zeros_like(tokens, dtype=torch.bool)
    for s in stop_ids:
        hit |= tokens == int(s)
    seen = hit.long().cumsum(1) > 0
    before = torch.zeros_like(seen)
    before[:, 1:] = seen[:, :-1]
    return before
