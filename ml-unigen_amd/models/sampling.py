"""MaskGIT sampling helpers with the reference's public names and results
(reference: models/sampling.py -- 13 public functions incl. the misspelt `get_mask_chedule`).
These are tiny per-step host-orchestrated tensor ops on [B, 256] tensors; the heavy part of a
generation step (the backbone + head) runs on the HIP kernels.
"""
import math
from functools import partial

import torch
import torch.nn.functional as F

_TINY = 1e-20


def log(t, eps=_TINY):
    """log with a floor (reference sampling.py:20-21)."""
    return t.clamp(min=eps).log()


def gumbel_noise(t, generator=None):
    """-log(-log(U)), U ~ U(0,1) drawn with `generator` in t's shape/dtype/device (reference :24-26)."""
    u = torch.zeros_like(t).uniform_(0, 1, generator=generator)
    return -log(-log(u))


def gumbel_sample(t, temperature=1.0, dim=-1, generator=None):
    """argmax of t/temperature + Gumbel noise (reference :29-30)."""
    scaled = t / max(temperature, 1e-10)
    return (scaled + gumbel_noise(t, generator=generator)).argmax(dim=dim)


def top_k(logits, thres=0.9):
    """keep the ceil((1-thres)*V) largest logits of a [B, N, V] tensor, -inf elsewhere (reference :33-38)."""
    k = math.ceil((1 - thres) * logits.shape[-1])
    vals, idx = logits.topk(k, dim=-1)
    out = torch.full_like(logits, float("-inf"))
    out.scatter_(2, idx, vals)
    return out


def mask_by_random_topk(mask_len, probs, temperature=1.0, generator=None):
    """Re-mask the `mask_len` least confident positions, confidence = log p + temperature * Gumbel
    (reference :41-46).  mask_len: [B, 1]; probs: [B, N]; returns bool [B, N]."""
    confidence = log(probs) + temperature * gumbel_noise(probs, generator=generator)
    ordered = torch.sort(confidence, dim=-1).values
    threshold = torch.gather(ordered, 1, mask_len.long())
    return confidence < threshold


def cosine_schedule(t):
    return torch.cos(t * math.pi * 0.5)


def linear_schedule(t):
    return (1 - t).clamp(min=1e-6, max=1.0)


def pow(t, method):
    """`method` = 'pow<exponent>' (reference :59-63)."""
    exponent = float(method.replace("pow", ""))
    return (1.0 - t ** exponent).clamp(min=1e-6, max=1.0)


def sigmoid_schedule(t, start=-3, end=3, tau=1.0, clip_min=1e-6):
    """gamma schedule built from a sigmoid (reference :66-75)."""
    lo = torch.sigmoid(torch.tensor(start / tau))
    hi = torch.sigmoid(torch.tensor(end / tau))
    cur = torch.sigmoid((t * (end - start) + start) / tau)
    return torch.clip((hi - cur) / (hi - lo), clip_min, 1.0)


def get_mask_chedule(method, **schedule_kwargs):
    if method == "cosine":
        return cosine_schedule
    if method == "linear":
        return linear_schedule
    if "pow" in method:
        return partial(pow, method=method)
    if method == "sigmoid":
        return partial(sigmoid_schedule, **schedule_kwargs)
    raise ValueError("Unknown schedule method: {}".format(method))


def truncate_logits(logits, top_k=0, top_p=1.0, min_p=0.0):
    """top-k -> top-p -> min-p truncation of [B, V] logits (already divided by the temperature) as VALUE thresholds: returns a new
    tensor with -inf outside the kept set {v >= tau}, tau = max(tau_k, tau_p, tau_m).  The rule of the fused AR sampler
    (include/unigen_hip.h: ug_ar_sample_filtered), in plain torch for the unfused paths, on CPU or GPU.
      top_k (0 or >= V: off): tau_k = the k-th largest value; every value tied at it is kept (`logits < topk[..., -1]` dropped, as in
        top_k_top_p_filtering).
      top_p (1: off): over S_k = {v >= tau_k} with ex = exp(v - max), Z = sum of ex over S_k: a value is kept iff the mass of the
        strictly greater values is <= top_p * Z.  For the first token of a run of equal values this is top_k_top_p_filtering's rule;
        where that function cuts THROUGH a run of equal logits (which of them survive depends on the sort's order of equal keys),
        this rule keeps the whole run.  The maximum is always kept.
      min_p (0: off): tau_m = max + log(min_p) (transformers' rule; the softmax normaliser cancels).
    Masses are summed in float64."""
    if logits.dim() != 2:
        raise ValueError("truncate_logits expects [B, V] logits")
    if not (top_k >= 0 and 0.0 < top_p <= 1.0 and 0.0 <= min_p <= 1.0):
        raise ValueError(f"truncate_logits: need top_k >= 0, 0 < top_p <= 1, 0 <= min_p <= 1 (got {top_k}, {top_p}, {min_p})")
    V = logits.shape[-1]
    v = logits.double()
    mx = v.max(-1, keepdim=True).values
    tau = torch.full_like(mx, float("-inf"))
    if 0 < top_k < V:
        tau = v.topk(int(top_k), dim=-1).values[..., -1:]
    if top_p < 1.0:
        ordered = torch.sort(v, dim=-1, descending=True).values
        ex = torch.where(ordered >= tau, torch.exp(ordered - mx), torch.zeros_like(ordered))
        cum = ex.cumsum(-1)
        before = cum - ex                                    # mass sorted in front of each entry (equal values in front included)
        first = torch.ones_like(ordered, dtype=torch.bool)
        first[..., 1:] = ordered[..., 1:] != ordered[..., :-1]
        pos = torch.arange(V, device=v.device).expand_as(ordered)
        run_start = torch.where(first, pos, torch.zeros_like(pos)).cummax(-1).values
        greater = before.gather(-1, run_start)               # mass of the strictly greater values
        ok = (greater <= top_p * cum[..., -1:]) & (ordered >= tau)
        tau_p = torch.where(ok, ordered, torch.full_like(ordered, float("inf"))).min(-1, keepdim=True).values
        tau = torch.maximum(tau, tau_p)
    if min_p > 0.0:
        tau = torch.maximum(tau, mx + math.log(min_p))
    return torch.where(v >= tau, logits, torch.full_like(logits, float("-inf")))


def top_k_top_p_filtering(logits, top_k=0, top_p=1.0, filter_value=-float("Inf"), min_tokens_to_keep=1):
    """In-place top-k / nucleus filtering of [B, V] logits (reference :90-128)."""
    if top_k > 0:
        k = min(max(top_k, min_tokens_to_keep), logits.size(-1))
        kth = torch.topk(logits, k)[0][..., -1, None]
        logits[logits < kth] = filter_value
    if top_p < 1.0:
        ordered, order = torch.sort(logits, descending=True)
        cum = torch.cumsum(F.softmax(ordered, dim=-1), dim=-1)
        drop = cum > top_p
        if min_tokens_to_keep > 1:
            drop[..., :min_tokens_to_keep] = 0
        drop[..., 1:] = drop[..., :-1].clone()    # keep the first token that crosses the threshold
        drop[..., 0] = 0
        logits[drop.scatter(1, order, drop)] = filter_value
    return logits


def apply_repetition_penalty(logits, seen_mask, penalty):
    """transformers' RepetitionPenaltyLogitsProcessor on fp32 [R, V] logits, ahead of temperature / top-k / top-p: every id the bool
    mask `seen_mask` [R, V] marks (it occurs in the row's sequence so far: real prompt ids + emitted tokens) has its score multiplied
    by `penalty` if negative, divided by it otherwise -- once per distinct id.  Returns a new tensor.  The host text loops use it; the
    on-device loop's kernel (include/unigen_hip.h: ug_text_penalize) applies the same rule to the bf16-rounded score."""
    return torch.where(seen_mask, torch.where(logits < 0, logits * penalty, logits / penalty), logits)


def seen_mask_of(ids, valid, rows, vocab, device):
    """the bool [rows, vocab] mask of apply_repetition_penalty at the start of a call: ids [rows, L] (None: no ids, nothing seen) at
    the positions `valid` [rows, L] marks real (None: all); ids outside [0, vocab) are ignored"""
    seen = torch.zeros((rows, vocab + 1), dtype=torch.bool, device=device)
    if ids is not None:
        ids = ids.to(device).long()
        ok = (ids >= 0) & (ids < vocab)
        if valid is not None:
            ok &= valid.to(device) != 0
        seen.scatter_(1, torch.where(ok, ids, torch.full_like(ids, vocab)), True)
    return seen[:, :vocab]


def apply_logit_bias(logits, ids, values):
    """transformers' SequenceBiasLogitsProcessor with keys of length 1 on [R, V] logits: values[j] is added to column ids[j] of every
    row (ids distinct).  Returns a new tensor.  The on-device loop's kernel adds to the bf16-rounded score (include/unigen_hip.h:
    ug_text_constrain)."""
    out = logits.clone()
    if len(ids):
        cols = torch.as_tensor(ids, dtype=torch.long, device=logits.device)
        out[:, cols] += torch.as_tensor(values, dtype=logits.dtype, device=logits.device)
    return out


def history_of(ids, valid, rows, vocab):
    """the rows' histories at the start of a call, as lists: the ids the repetition penalty counts (seen_mask_of), in order -- ids
    [rows, L] (None: no ids, empty histories) inside [0, vocab) at the positions `valid` [rows, L] marks real (None: all)"""
    if ids is None:
        return [[] for _ in range(rows)]
    ids = ids.long().cpu()
    ok = (ids >= 0) & (ids < vocab)
    if valid is not None:
        ok &= valid.cpu() != 0
    return [ids[r][ok[r]].tolist() for r in range(rows)]


def ngram_banned(history, n):
    """transformers' NoRepeatNGramLogitsProcessor for one row: the ids that would complete an n-gram the history (a list of ids)
    already holds -- every history[i + n - 1] with history[i : i + n - 1] == the history's last n - 1 ids, 0 <= i <= len - n; nothing
    while the history is shorter than n - 1.  n = 1 bans every id of the history.  -> a list (duplicates possible)."""
    T = len(history)
    if n < 1 or T < n - 1:
        return []
    tail = history[T - n + 1:]
    return [history[i + n - 1] for i in range(T - n + 1) if history[i:i + n - 1] == tail]


def stop_sequence_hit(emitted, sequences):
    """whether the emitted tokens of one row (a list; the prompt is no part of it) end with one of `sequences` (lists of ids)"""
    return any(0 < len(s) <= len(emitted) and emitted[len(emitted) - len(s):] == list(s) for s in sequences)


def apply_constraints(logits, bias=(), banned=None, histories=None, ngram=0):
    """The constraints of one step on [R, V] logits, ahead of the repetition penalty (the -inf stores commute with it): bias =
    [(id, b), ...] with b = -inf for a suppressed id (apply_logit_bias / transformers' SuppressTokensLogitsProcessor), `banned` = ids
    that score -inf in every row (the stop ids while min_new_tokens holds: MinNewTokensLengthLogitsProcessor), and ngram_banned of
    every row's history.  Returns a new tensor."""
    add = [(e, b) for e, b in bias if b != float("-inf")]
    out = apply_logit_bias(logits, [e for e, _ in add], [b for _, b in add])
    cols = [e for e, b in bias if b == float("-inf")] + list(banned or ())
    if cols:
        out[:, torch.as_tensor(cols, dtype=torch.long, device=out.device)] = float("-inf")
    if ngram:
        V = out.shape[1]
        for r, h in enumerate(histories):
            ban = [e for e in ngram_banned(h, ngram) if 0 <= e < V]
            if ban:
                out[r, torch.as_tensor(ban, dtype=torch.long, device=out.device)] = float("-inf")
    return out


def token_logprobs(scores, tokens, done=None):
    """The log-probability of every row's picked token under the distribution it was picked from: the log-softmax of the PROCESSED
    scores [R, V] (after the repetition penalty, the temperature and top-k / top-p / min-p written as -inf -- whatever the pick saw) at
    tokens [R] or [R, 1], in fp32: s[tok] - max s - log(sum of exp(s - max s)).  This is transformers' compute_transition_scores(...,
    normalize_logits=True) for one step.  -inf entries add 0 and a NaN entry adds nothing (it is no candidate).  done (bool [R], optional):
    rows that had finished BEFORE the step get exactly 0.0.  The host text loops and the unfused branch of t2i_generate_ar use it; the
    sampler kernels compute the same formula on the device (include/unigen_hip.h: ug_text_pick_logp, ug_ar_sample_logp).  -> fp32 [R]."""
    s = scores.float()
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    d = s - s.max(-1, keepdim=True).values
    lp = (d.gather(-1, tokens.reshape(-1, 1).long().to(s.device)) - torch.log(torch.exp(d).sum(-1, keepdim=True)))[:, 0]
    if done is not None:
        lp = torch.where(done.to(lp.device), torch.zeros_like(lp), lp)
    return lp
