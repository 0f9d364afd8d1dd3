"""UniGen on the MI355X kernels -- drop-in for the reference's `models/unigen.py` (same class name,
constructor, method signatures and return conventions), so `training/train*.py` and
`evaluation/inference_*.py` run against it unchanged.  The backbone the reference builds from
transformers (`Qwen2ForCausalLM`, models/unigen.py:56-69) is `unigen_hip.modules.HipQwen2ForCausalLM`:
hand-written HIP kernels behind a C ABI, no torch math on the hot path.

Behavioural notes (all mirror the reference unless stated):
  * forward() with labels returns (logits, loss_t2i, loss_lm, loss_mmu); the three losses are the
    masked cross-entropies of models/unigen.py:310-338 (same slices, mean over non-ignored labels).
    `logits` is a lazy view that evaluates the lm_head only for the positions a caller slices
    (the reference materialises [B, L, 159867]); `label_smoothing` is accepted and ignored exactly
    like the reference (it never reaches F.cross_entropy).
  * precision: the reference's bf16-autocast training mode (fp32 master weights / residual stream,
    bf16 matmuls, fp32 statistics) is what the kernels implement, with or without an enclosing
    torch.autocast.
  * gen_proj_depth > 0 (alternate image embedding gen_embed -> gen_projector and the 8192-way img_head,
    unigen.py:74-92; off in every shipped config) is implemented for forward / training and MaskGIT
    generation; t2i_generate_ar with it raises.
"""
import collections
import dataclasses
import json
import math
import os
import time
import weakref
from typing import Optional

import torch

from unigen_hip import ops
from unigen_hip.lib import UniGenHipError
from unigen_hip.modules import (HipProjector, HipQwen2ForCausalLM, LazyLogits, _CrossEntropyFn, _HeadLossFn, _LinearFn,
                                _TableEmbedFn)
from unigen_hip.qwen2 import Qwen2Dims

from .modeling_utils import ConfigMixin, ModelMixin, register_to_config
from .sampling import cosine_schedule, mask_by_random_topk

# public Qwen2.5-1.5B(-Instruct) architecture (its config.json), used when no local HF directory exists
_KNOWN_LLM = {
    "qwen2.5-1.5b": dict(hidden_size=1536, intermediate_size=8960, num_hidden_layers=28, num_attention_heads=12,
                         num_key_value_heads=2, rope_theta=1000000.0, rms_norm_eps=1e-6, vocab_size=151936),
}


def _load_llm_config(llm_model_path, ckpt_base_path=""):
    """The reference reads this with AutoConfig.from_pretrained (models/unigen.py:52)."""
    cands = [llm_model_path]
    if ckpt_base_path:
        cands.insert(0, os.path.join(ckpt_base_path, os.path.basename(str(llm_model_path).rstrip("/"))))
    for c in cands:
        f = os.path.join(str(c), "config.json")
        if os.path.exists(f):
            with open(f) as fh:
                return json.load(fh)
    low = str(llm_model_path).lower()
    for key, cfg in _KNOWN_LLM.items():
        if key in low:
            return dict(cfg)
    raise UniGenHipError(f"cannot find an LLM config for '{llm_model_path}' (no config.json, unknown name)")


def _drop_anchor_from_state_dict(module, state_dict, prefix, local_metadata):
    module.llm.engine.fp.wait_pending_update()             # an overlapped optimizer update must land before anyone reads the tensors
    state_dict.pop(prefix + "_ddp_anchor", None)          # not part of the reference checkpoint format
    return state_dict


def _forgive_missing_anchor(module, incompatible_keys):
    incompatible_keys.missing_keys[:] = [k for k in incompatible_keys.missing_keys if not k.endswith("_ddp_anchor")]


def text_token_loop(max_new_tokens, hn, pick, emit, head, embed, step):
    """The token loop of every cached text generation (generate, mmu_generate, mmu_generate_batch), from the prefill's final-norm
    hidden state `hn`: logits = head(hn) -> nxt = pick(logits) [R, 1] -> feed, stop = emit(i, nxt) -> hn = step(embed(feed)).
    `emit` records token i and returns the ids to feed back and whether every row has finished; no decode step follows the last
    token.  The engine comes in as the three callables, so the loop itself runs anywhere.  Returns the number of tokens emitted."""
    for i in range(max_new_tokens):
        feed, stop = emit(i, pick(head(hn)))
        if stop or i + 1 == max_new_tokens:
            return i + 1
        hn = step(embed(feed))
    return 0


def emit_until_stop(out, stop, pad_token_id=None, lengths=None):
    """The record and stop rule of the text loops: token i goes into out [R, new]; a row has finished once it has produced `stop` (an
    id, or a 0-d / 1-D tensor of ids), and the loop stops when every row has.  pad_token_id (`generate`): a finished row is filled with it from
    then on, before the token is recorded and fed back.  lengths [R] (`mmu_generate_batch`): a row's entry is set to end just after
    its stop token.  stop None: no host sync, never stops early."""
    done = torch.zeros(out.shape[0], dtype=torch.bool, device=out.device)

    def emit(i, nxt):
        if stop is not None and pad_token_id is not None:
            nxt = torch.where(done[:, None], torch.full_like(nxt, int(pad_token_id)), nxt)
        out[:, i] = nxt[:, 0]
        if stop is None:
            return nxt, False
        hit = (nxt == stop).any(-1) & ~done
        if lengths is not None:
            lengths.masked_fill_(hit, i + 1)
        done.logical_or_(hit)
        return nxt, bool(done.all())
    emit.done = done                               # (with_logprobs reads which rows had finished before a step)
    return emit


def checked_repetition_penalty(p, who):
    """a call's `repetition_penalty` as a float (None: 1.0 = off); anything not finite and > 0 raises, before any launch"""
    if p is None:
        return 1.0
    p = float(p)
    if not (math.isfinite(p) and p > 0.0):
        raise UniGenHipError(f"{who}: repetition_penalty={p} must be finite and > 0 (1 is off)")
    return p


def with_logprobs(process, choose, emit, logp):
    """`pick` and `emit` of text_token_loop that also record every emitted token's log-probability into logp fp32 [R, new]
    (models/sampling.py: token_logprobs): pick = choose(process(last)), where `process` turns the scores it is handed (behind the
    repetition penalty, if any) into the ones `choose` picks from (temperature, top-k / top-p as -inf).  `emit` is emit_until_stop's: a
    row that had finished before the step records 0.0.  The innermost wrapper (text_pick_emit holds the order)."""
    from .sampling import token_logprobs
    last_lp = [None]

    def pick(last):
        scores = process(last)
        nxt = choose(scores)
        last_lp[0] = token_logprobs(scores, nxt)
        return nxt

    def emit_and_record(i, nxt):
        logp[:, i] = torch.where(emit.done, torch.zeros_like(last_lp[0]), last_lp[0])          # (done BEFORE this step)
        return emit(i, nxt)
    return pick, emit_and_record


def with_repetition_penalty(pick, emit, penalty, seen):
    """`pick` and `emit` of text_token_loop with transformers' repetition penalty in front of the pick (models/sampling.py:
    apply_repetition_penalty): seen bool [R, V] holds the row's sequence so far and takes every token `emit` feeds back (a finished
    row's pad id included, as on the device)."""
    from .sampling import apply_repetition_penalty

    def emit_and_mark(i, nxt):
        feed, stop = emit(i, nxt)
        seen.scatter_(1, feed, True)
        return feed, stop
    return (lambda last: pick(apply_repetition_penalty(last, seen, penalty))), emit_and_mark


def checked_constraints(who, vocab, logit_bias=None, suppress_tokens=None, min_new_tokens=None, no_repeat_ngram_size=None,
                        stop_sequences=None):
    """A call's constraints, checked before any launch (include/unigen_hip.h: "Constraints of the text loops") -> (None when all five
    are off, else {"bias": [(id, bias), ...] sorted by id with -inf for a suppressed id, "min_new": m, "ngram": n, "stop_seqs": the
    stop sequences of two or more ids as tuples}, the ids of the stop sequences of length 1 -- they join the call's stop ids).
    vocab: a callable that returns V, asked only when there are ids to check.  An id in both lists, twice in one or outside [0, V), a
    bias that is not finite, a negative count or an empty stop sequence raises UniGenHipError."""
    bias = {}
    for name, items in (("logit_bias", list((logit_bias or {}).items())), ("suppress_tokens", [(e, float("-inf")) for e in (suppress_tokens or ())])):
        for e, b in items:
            e, b = int(e), float(b)
            if e in bias:
                raise UniGenHipError(f"{who}: id {e} occurs twice in logit_bias / suppress_tokens")
            if name == "logit_bias" and not math.isfinite(b):
                raise UniGenHipError(f"{who}: logit_bias[{e}]={b} must be finite (suppress_tokens bans an id)")
            bias[e] = b
    m = 0 if min_new_tokens is None else int(min_new_tokens)
    n = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
    if m < 0 or n < 0:
        raise UniGenHipError(f"{who}: min_new_tokens={m} and no_repeat_ngram_size={n} must be at least 0 (0 is off)")
    seqs = [tuple(int(t) for t in s) for s in (stop_sequences or ())]
    if any(len(s) == 0 for s in seqs):
        raise UniGenHipError(f"{who}: an empty stop sequence")
    ids = list(bias) + [t for s in seqs for t in s]
    if ids:
        V = int(vocab())
        bad = [e for e in ids if not 0 <= e < V]
        if bad:
            raise UniGenHipError(f"{who}: ids {sorted(set(bad))} of logit_bias / suppress_tokens / stop_sequences are outside [0, {V})")
    singles = [s[0] for s in seqs if len(s) == 1]
    longer = [s for s in seqs if len(s) > 1]
    if not (bias or m or n or longer):
        return None, singles
    return {"bias": sorted(bias.items()), "min_new": m, "ngram": n, "stop_seqs": longer}, singles


def with_constraints(pick, emit, constraints, done, histories, stop_ids=(), lengths=None):
    """`pick` and `emit` of text_token_loop with the constraints of checked_constraints in front of everything else (models/sampling.py:
    apply_constraints; the order is include/unigen_hip.h's: the -inf stores commute with the repetition penalty, so this is the
    outermost wrapper -- text_pick_emit holds the order -- and the log-probabilities are those of the fully processed scores).
    done: emit_until_stop's `emit.done`; histories: sampling.history_of's lists, which take every token `emit` feeds back (a finished
    row's pad id included, as on the device); stop_ids: the single stop ids min_new_tokens holds back; lengths: emit_until_stop's.
    A stop sequence is matched on the emitted tokens alone and finishes a row exactly as a stop id does -- once, at the step whose
    token completes it; a row a stop id finished at that very step is left alone."""
    from .sampling import apply_constraints, stop_sequence_hit
    bias, min_new, ngram, seqs = constraints["bias"], constraints["min_new"], constraints["ngram"], constraints["stop_seqs"]
    stop_ids = [int(s) for s in stop_ids]
    emitted = [[] for _ in histories]
    count = [0]

    def constrained_pick(last):
        return pick(apply_constraints(last, bias, stop_ids if count[0] < min_new else (), histories, ngram))

    def emit_and_match(i, nxt):
        feed, stop = emit(i, nxt)
        count[0] = i + 1
        if ngram or seqs:
            for r, t in enumerate(feed[:, 0].tolist()):
                histories[r].append(t)
                emitted[r].append(t)
        if seqs:
            was = done.tolist()
            hit = torch.tensor([not was[r] and stop_sequence_hit(emitted[r], seqs) for r in range(len(emitted))], device=done.device)
            if lengths is not None:
                lengths.masked_fill_(hit, i + 1)
            done.logical_or_(hit)
            stop = bool(done.all())
        return feed, stop
    return constrained_pick, emit_and_match


def stop_list(stop):
    """the stop ids of a call (None, an id, a list, or a 0-d / 1-D tensor of ids) as a list of ints"""
    if stop is None:
        return []
    if torch.is_tensor(stop):
        return [int(v) for v in stop.reshape(-1).tolist()]
    if isinstance(stop, (list, tuple)):
        return [int(v) for v in stop]
    return [int(stop)]


@dataclasses.dataclass(frozen=True)
class TextCall:
    """How one call of `generate` / `mmu_generate` / `mmu_generate_batch` decodes: everything that does not depend on the prompt,
    checked and resolved once (text_call) and read by both loops.  The entry points' docstrings say what each option means."""
    who: str                        # the entry point's name, for error messages
    sampling: Optional[tuple]       # the on-device loop's constants: None (greedy) or (temperature, top_k, top_p)
    process: object                 # the host loop's rule (generate_rule / mmu_rule): scores -> the scores `choose` picks from,
    choose: object                  # and those -> token ids [R, 1]
    generator: Optional[torch.Generator]
    stop: list                      # the stop ids, stop sequences of one id merged in
    host_stop: object               # what the host loop's emit_until_stop compares a token with (text_call)
    pad_token_id: Optional[int]
    penalty: float                  # checked_repetition_penalty's
    constraints: Optional[dict]     # checked_constraints' dict
    return_logprobs: bool
    deterministic: bool
    use_graph: bool
    trace: Optional[list]
    spec: Optional[tuple] = None    # prompt-lookup speculative decoding: None (off) or (K, G, lookup ids or None) (checked_prompt_lookup)

    @property
    def stops(self):
        """whether a row can finish before max_new_tokens (a stop id, or a stop sequence of two or more ids)"""
        return bool(self.stop or (self.constraints and self.constraints["stop_seqs"]))


def generate_rule(do_sample, temperature, top_k, top_p, generator):
    """`generate`'s host sampling rule -> (process, choose): temperature, then top_k_top_p_filtering, then torch.multinomial with the
    caller's generator on the generator's device; greedy: the scores as they are, argmax"""
    from .sampling import top_k_top_p_filtering

    def process(last):
        if not do_sample:
            return last
        if temperature is not None and temperature != 1.0:
            last = last / temperature
        return top_k_top_p_filtering(last, top_k=int(top_k or 0), top_p=float(1.0 if top_p is None else top_p))

    def choose(scores):
        if not do_sample:
            return scores.argmax(-1, keepdim=True)
        u_dev = scores.device if generator is None else generator.device
        return torch.multinomial(torch.softmax(scores, dim=-1).to(u_dev), num_samples=1, generator=generator).to(scores.device)
    return process, choose


def mmu_rule(temperature, top_k):
    """the mmu entry points' host sampling rule -> (process, choose): UniGen._process_next / _choose_next (temperature, an in-place
    top-k threshold, torch.multinomial from the default generator; temperature 0: argmax)"""
    return (lambda last: UniGen._process_next(last, temperature, top_k)), (lambda scores: UniGen._choose_next(scores, temperature))


SPEC_REFUSED = ("repetition_penalty", "logit_bias", "suppress_tokens", "min_new_tokens", "no_repeat_ngram_size", "stop_sequences",
                "return_logprobs", "deterministic", "num_return_sequences", "on_device")


def checked_prompt_lookup(who, vocab, sampling, given, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, lookup_ids=None):
    """The speculative-decoding option of a call -> None (prompt_lookup_num_tokens None or 0: off, and nothing else is looked at) or
    (K, G, lookup ids as a long 1-D tensor or None).  On: K = 1 .. 7 draft tokens per step, G = 1 .. 4 (default 2, transformers')
    ids at most matched; the call must pick greedily, and `given` -- the values of the options in SPEC_REFUSED as the call resolved
    them -- must all be off: each one that is not is refused by name, before any launch."""
    if prompt_lookup_num_tokens is None or int(prompt_lookup_num_tokens) == 0:
        return None
    K, G = int(prompt_lookup_num_tokens), 2 if max_matching_ngram_size is None else int(max_matching_ngram_size)
    if not 1 <= K <= ops.SPEC_MAX_ROWS - 1:
        raise UniGenHipError(f"{who}: prompt_lookup_num_tokens={K} must be between 1 and {ops.SPEC_MAX_ROWS - 1}")
    if not 1 <= G <= ops.SPEC_MAX_NGRAM:
        raise UniGenHipError(f"{who}: max_matching_ngram_size={G} must be between 1 and {ops.SPEC_MAX_NGRAM}")
    off = {"repetition_penalty": (None, 1, 1.0), "min_new_tokens": (None, 0), "no_repeat_ngram_size": (None, 0),
           "num_return_sequences": (None, 1), "on_device": (None, True)}
    refused = [k for k in SPEC_REFUSED if given.get(k) not in off.get(k, (None, False)) and given.get(k) != [] and given.get(k) != {}]
    if refused:
        raise UniGenHipError(f"{who}: {refused} are not implemented with prompt_lookup_num_tokens (one greedy row on the device loop, "
                             f"default decode mode)")
    if sampling is not None:
        raise UniGenHipError(f"{who}: prompt_lookup_num_tokens needs greedy picking (do_sample=False; temperature 0 or top_k=1 in the mmu "
                             f"calls): only tokens the model itself would pick are accepted")
    if lookup_ids is not None:
        if not torch.is_tensor(lookup_ids) or lookup_ids.dim() != 1 or lookup_ids.dtype != torch.long:
            raise UniGenHipError(f"{who}: lookup_ids must be a long 1-D tensor of token ids")
        V = int(vocab())
        if lookup_ids.numel() and not (0 <= int(lookup_ids.min()) and int(lookup_ids.max()) < V):
            raise UniGenHipError(f"{who}: lookup_ids outside [0, {V})")
    return K, G, lookup_ids


def check_spec_call(call, rows, engine):
    """what a speculative call checks once its prompt's shape is at hand, still before any launch: one row, and an engine whose
    verify step takes the sw or splitk form (Qwen2Engine.spec_form raises, naming the form)"""
    if rows != 1:
        raise UniGenHipError(f"{call.who}: prompt_lookup_num_tokens serves one row per call, got {rows} (rows > 1 need per-row cache "
                             f"positions)")
    engine.spec_form(call.spec[0] + 1)


def text_call(who, vocab, sampling, rule, stop, pad_finished=False, pad_token_id=None, generator=None, repetition_penalty=None,
              deterministic=None, return_logprobs=False, use_graph=True, trace=None, logit_bias=None, suppress_tokens=None,
              min_new_tokens=None, no_repeat_ngram_size=None, stop_sequences=None, prompt_lookup=None):
    """The TextCall of one public call, with every check that needs no prompt, before any launch.  vocab: a callable that returns V
    (checked_constraints).  rule: the (process, choose) of generate_rule / mmu_rule.  stop: the caller's stop ids in any form
    stop_list takes -- a device tensor is read here, once; the stop sequences of one id join them unless already there (the caller's
    own list is kept as given).  pad_finished (`generate`): finished rows are filled with pad_token_id, which defaults to the first
    stop id, and stop sequences need one of the two.
    host_stop keeps the operand of the host loop's per-token compare what each entry point has always handed emit_until_stop (the
    same launches): `generate` a tensor of the ids, or None when no row can finish; the mmu entry points the caller's own id or
    tensor while nothing was merged into it and no constraint is on, else the list (a list becomes a tensor: text_pick_emit).
    prompt_lookup: None, or the dict of the entry point's prompt_lookup_num_tokens / max_matching_ngram_size / lookup_ids with its
    on_device and num_return_sequences (checked_prompt_lookup: resolved here, where the other options are)."""
    from unigen_hip.qwen2 import resolve_deterministic
    det = resolve_deterministic(deterministic)
    spec = None
    if prompt_lookup:
        given = dict(repetition_penalty=repetition_penalty, logit_bias=logit_bias, suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens,
                     no_repeat_ngram_size=no_repeat_ngram_size, stop_sequences=stop_sequences, return_logprobs=bool(return_logprobs),
                     deterministic=det, num_return_sequences=prompt_lookup.get("num_return_sequences"), on_device=prompt_lookup.get("on_device"))
        spec = checked_prompt_lookup(who, vocab, sampling, given, **{k: prompt_lookup.get(k) for k in
                                                                      ("prompt_lookup_num_tokens", "max_matching_ngram_size", "lookup_ids")})
    penalty = checked_repetition_penalty(repetition_penalty, who)
    cons, singles = checked_constraints(who, vocab, logit_bias, suppress_tokens, min_new_tokens, no_repeat_ngram_size, stop_sequences)
    ids = stop_list(stop)
    if pad_finished:
        if stop_sequences and stop is None and pad_token_id is None:
            raise UniGenHipError(f"{who}: stop_sequences need an eos_token_id or a pad_token_id (a finished row is filled with it)")
        if ids and pad_token_id is None:
            pad_token_id = ids[0]
    ids = ids + [e for e in singles if e not in ids]
    if pad_finished:
        host_stop = ids if ids or (cons and cons["stop_seqs"]) else None
    else:
        host_stop = ids if cons is not None or singles or isinstance(stop, (list, tuple)) else stop
    return TextCall(who, sampling, rule[0], rule[1], generator, ids, host_stop, pad_token_id, penalty, cons, bool(return_logprobs),
                    det, bool(use_graph), trace, spec)


def generate_call(vocab, do_sample, temperature, top_k, top_p, eos_token_id, pad_token_id, generator, deterministic, return_logprobs,
                  kwargs, prompt_lookup=None):
    """`generate`'s arguments -> (TextCall, num_return_sequences).  prompt_lookup: text_call's, without num_return_sequences"""
    unsupported = [k for k in ("num_beams", "penalty_alpha") if kwargs.get(k) not in (None, 1, 1.0)]
    if unsupported:
        raise UniGenHipError(f"generate: {unsupported} are not implemented in generate (greedy / sampling only): call UniGen.beam_search")
    sampling = None
    if do_sample:
        sampling = (float(1.0 if temperature is None else temperature), int(top_k or 0), float(1.0 if top_p is None else top_p))
    call = text_call("generate", vocab, sampling, generate_rule(do_sample, temperature, top_k, top_p, generator), eos_token_id,
                     pad_finished=True, pad_token_id=pad_token_id, generator=generator, deterministic=deterministic,
                     return_logprobs=return_logprobs, use_graph=kwargs.get("use_graph", True), trace=kwargs.get("trace"),
                     prompt_lookup=prompt_lookup and dict(prompt_lookup, num_return_sequences=kwargs.get("num_return_sequences")),
                     **{k: kwargs.get(k) for k in ("repetition_penalty", "logit_bias", "suppress_tokens", "min_new_tokens",
                                                   "no_repeat_ngram_size", "stop_sequences")})
    n_ret = kwargs.get("num_return_sequences")
    n_ret = 1 if n_ret is None else int(n_ret)
    if n_ret < 1:
        raise UniGenHipError(f"generate: num_return_sequences={n_ret} must be at least 1")
    if n_ret > 1 and not do_sample:
        raise UniGenHipError(f"generate: num_return_sequences={n_ret} needs do_sample=True (greedy rows would all be equal)")
    return call, n_ret


BEAM_REFUSED = ("do_sample", "repetition_penalty", "logit_bias", "suppress_tokens", "min_new_tokens", "no_repeat_ngram_size",
                "stop_sequences", "return_logprobs", "num_beam_groups", "on_device")


def beam_call(rows, max_new_tokens, num_beams, num_return_sequences, length_penalty, early_stopping, eos_token_id, pad_token_id, kwargs):
    """`beam_search`'s arguments, checked before any launch -> (num_beams, num_return_sequences, eos ids, pad id).  rows: the number of
    prompts.  What the method does not serve is refused by name: the options that need per-beam histories reordered with the beams
    (the penalty, the constraints, log-probabilities), sampling, beam groups and the on-device loop."""
    off = {"repetition_penalty": (None, 1, 1.0), "num_beam_groups": (None, 1), "min_new_tokens": (None, 0), "no_repeat_ngram_size": (None, 0)}
    refused = [k for k in BEAM_REFUSED if k in kwargs and kwargs[k] not in off.get(k, (None, False)) and kwargs[k] != [] and kwargs[k] != {}]
    if refused:
        raise UniGenHipError(f"beam_search: {refused} are not implemented with beam search (greedy beams on the host loop only)")
    unknown = [k for k in kwargs if k not in BEAM_REFUSED]
    if unknown:
        raise UniGenHipError(f"beam_search: unknown arguments {unknown}")
    B, n = int(num_beams), int(num_return_sequences)
    if not 1 <= B <= ops.BEAM_MAX_BEAMS:
        raise UniGenHipError(f"beam_search: num_beams={B} must be between 1 and {ops.BEAM_MAX_BEAMS}")
    if rows < 1 or rows * B > ops.BEAM_MAX_ROWS:
        raise UniGenHipError(f"beam_search: {rows} prompts x num_beams={B} = {rows * B} rows (at least 1, at most {ops.BEAM_MAX_ROWS})")
    if not 1 <= n <= B:
        raise UniGenHipError(f"beam_search: num_return_sequences={n} must be between 1 and num_beams={B}")
    if int(max_new_tokens) < 1:
        raise UniGenHipError(f"beam_search: max_new_tokens={max_new_tokens} must be at least 1")
    if early_stopping not in (False, True, "never"):
        raise UniGenHipError(f"beam_search: early_stopping={early_stopping!r} must be False, True or 'never'")
    if not math.isfinite(float(length_penalty)):
        raise UniGenHipError(f"beam_search: length_penalty={length_penalty} must be finite")
    eos = list(dict.fromkeys(stop_list(eos_token_id)))
    if len(eos) > 7:
        raise UniGenHipError(f"beam_search: {len(eos)} eos ids (at most 7: a step keeps (1 + eos ids) x num_beams candidates, at most "
                             f"{ops.BEAM_MAX_K})")
    pad = int(pad_token_id) if pad_token_id is not None else (eos[0] if eos else 0)
    return B, n, eos, pad


def mmu_call(who, vocab, temperature, top_k, eot_token, **how):
    """the arguments of `mmu_generate` / `mmu_generate_batch` -> TextCall (temperature 0 is greedy; `how`: text_call's keywords)"""
    sampling = (float(temperature), int(top_k or 0), 1.0) if temperature > 0 else None
    lookup = how.get("prompt_lookup")
    if lookup and lookup.get("prompt_lookup_num_tokens") and top_k == 1:
        sampling = None                             # (top_k=1 keeps the maximum alone: greedy, whatever the temperature)
    return text_call(who, vocab, sampling, mmu_rule(temperature, top_k), eot_token, **how)


def text_pick_emit(call, out, vocab, logp=None, lengths=None, prompt_ids=None, prompt_valid=None):
    """`pick` and `emit` of text_token_loop for a call: the one place that holds the wrap order -- emit_until_stop, then with_logprobs,
    then with_repetition_penalty, then with_constraints, so that a step runs the constraints, the penalty, the call's process / choose
    and the log-probability of the fully processed scores (the order of include/unigen_hip.h: "Constraints of the text loops").
    out long [R, new] takes the tokens, logp fp32 [R, new] (or None) their log-probabilities, lengths [R] (or None) is
    emit_until_stop's; prompt_ids / prompt_valid [R, L] are what the penalty and the n-gram history count of the prompt."""
    from .sampling import history_of, seen_mask_of
    R, dev = out.shape[0], out.device
    stop = torch.tensor(call.host_stop, dtype=torch.long, device=dev) if isinstance(call.host_stop, list) else call.host_stop
    emit = emit_until_stop(out, stop, call.pad_token_id, lengths)
    done = emit.done
    if logp is None:
        pick = lambda last: call.choose(call.process(last))
    else:
        pick, emit = with_logprobs(call.process, call.choose, emit, logp)
    if call.penalty != 1.0:
        pick, emit = with_repetition_penalty(pick, emit, call.penalty, seen_mask_of(prompt_ids, prompt_valid, R, vocab, dev))
    if call.constraints is not None:
        pick, emit = with_constraints(pick, emit, call.constraints, done, history_of(prompt_ids, prompt_valid, R, vocab),
                                      stop_ids=call.stop, lengths=lengths)
    return pick, emit


MMU_MAX_ROWS = 32


class MmuPrefix:
    """A prompt prefix prefilled once and shared by many continuations (`UniGen.mmu_prefix`): a one-row DecodeState whose first P
    cache positions hold the prefix's keys / values of every layer, P itself, the key validity of the prefix mask's last row (bool
    [1, P]: what every later position sees of the prefix), and the prefix's ids (long [1, P]; None once any part of it came as
    embeddings) for the repetition penalty.  `mmu_generate_batch(prefix=...)` / `mmu_generate(prefix=...)` read it and leave it
    unchanged; `extend` grows it in place.  The object belongs to the model, device and WEIGHTS it was built with, and to the
    caller: nothing in the model keeps or drops it (`drop_decode_session()` does not touch it)."""

    def __init__(self, model, st, P, key_valid, ids):
        self.model, self.engine, self.device = model, model.llm.engine, model.llm.engine.device
        self.st, self.P, self.key_valid, self.ids = st, int(P), key_valid, ids
        self.all_valid = True if key_valid is None else bool(key_valid.all())

    @property
    def capacity(self):
        return self.st.Tmax

    @torch.no_grad()
    def extend(self, idx=None, input_embeddings=None):
        """Append a causal continuation of S positions (ids [1, S] or embeddings [1, S, H]) to the prefix through
        Qwen2Engine.prefill_onto: chunked prefill, or the next turn of a conversation on one row.  The new positions see what the
        prefix mask's last row saw plus everything appended since.  Beyond `capacity` it raises.  -> self."""
        if (idx is None) == (input_embeddings is None):
            raise UniGenHipError("MmuPrefix.extend: give idx or input_embeddings")
        new = idx if input_embeddings is None else input_embeddings
        if new.shape[0] != 1 or new.shape[1] < 1:
            raise UniGenHipError(f"MmuPrefix.extend: one row of at least one position, got {tuple(new.shape)}")
        S = int(new.shape[1])
        if self.P + S > self.capacity:
            raise UniGenHipError(f"MmuPrefix.extend: {self.P} + {S} positions exceed the prefix's capacity of {self.capacity}")
        x = (self.model.llm.model.embed_tokens(idx) if input_embeddings is None else input_embeddings).float()
        ones = torch.ones((1, S), dtype=torch.bool, device=self.key_valid.device)
        key_valid = torch.cat([self.key_valid, ones], dim=1)
        self.engine.prefill_onto(self.st, x, self.P, None if self.all_valid else key_valid)
        self.engine.check_errors()
        self.ids = None if self.ids is None or idx is None else torch.cat([self.ids, idx.to(self.ids.device).long()], dim=1)
        self.P, self.key_valid = self.P + S, key_valid
        return self


def check_prefix(who, engine, prefix, rows=None, what=None):
    """what every call that takes `prefix` checks of it: its type, that this engine built it, and (when the call's rows are at hand:
    a tensor, named `what` in the message) that they live on its device"""
    if not isinstance(prefix, MmuPrefix):
        raise UniGenHipError(f"{who}: prefix must be the object UniGen.mmu_prefix returns, got {type(prefix).__name__}")
    if prefix.engine is not engine:
        raise UniGenHipError(f"{who}: the prefix was built by another model")
    if rows is not None:
        pd, td = torch.device(prefix.device), rows.device
        if td.type != pd.type or (td.index is not None and pd.index is not None and td.index != pd.index):
            raise UniGenHipError(f"{who}: the prefix lives on another device ({pd}) than the {what} ({td})")


def _prefill_after_prefix(engine, st, prefix, tails, key_valid, hidden_at=None):
    """the prefill of a call that takes a prefix: the prefix's keys / values of every layer into positions [0, P) of every row of
    `st`, then the rows' tails [R, S, H] onto them (Qwen2Engine.prefill_onto) -> final-norm hidden of the last tail position
    (with hidden_at: prefill_onto's pair)"""
    P = prefix.P
    for i in range(len(st.k)):
        st.k[i][:, :, :P].copy_(prefix.st.k[i][:, :, :P])          # (one row, broadcast to the call's rows)
        st.v[i][:, :, :P].copy_(prefix.st.v[i][:, :, :P])
    if hidden_at is None:
        return engine.prefill_onto(st, tails, P, key_valid)
    return engine.prefill_onto(st, tails, P, key_valid, hidden_at=hidden_at)


@dataclasses.dataclass(frozen=True)
class TextPrompt:
    """The prompt of one text generation call, as both loops read it (built by UniGen._generate_prompt / _dense_prompt /
    _prefix_prompt)."""
    embeds: torch.Tensor                     # fp32 [R, L, H] to prefill; behind a prefix the rows' tails [R, S, H]
    L: int                                   # positions of the prompt (P + S with a prefix)
    key_valid: Optional[torch.Tensor]        # bool [R, L]: the keys every later position sees (None: all)
    mask_bits: Optional[object]              # the compressed dense mask to prefill under (None: causal with key_valid)
    prompt_ids: Optional[torch.Tensor]       # [R, L]: the ids the repetition penalty and the n-gram history count (None: no ids),
    prompt_valid: Optional[torch.Tensor]     # at the positions this marks real
    prefix: Optional[MmuPrefix] = None

    @property
    def rows(self):
        return int(self.embeds.shape[0])

    def prefill(self, engine, st):
        """prefill the prompt into `st` -> final-norm hidden state of its last position, bf16 [R, H]"""
        if self.prefix is not None:
            return _prefill_after_prefix(engine, st, self.prefix, self.embeds, self.key_valid)
        return engine.prefill(st, self.embeds, self.key_valid, mask_bits=self.mask_bits)


def check_mmu_prefix_call(who, engine, prefix, idx, input_embeddings, attention_mask, tail_valid):
    """The argument checks of a generation call that takes `prefix`, all on the host and before anything is launched
    -> (rows, tail length, tail_valid as a bool tensor or None)."""
    tail = idx if input_embeddings is None else input_embeddings
    check_prefix(who, engine, prefix, tail, "tails")
    if (idx is None) == (input_embeddings is None):
        raise UniGenHipError(f"{who}: with a prefix, give the rows' tails as idx [R, S] or input_embeddings [R, S, H]")
    if tail.dim() != (2 if input_embeddings is None else 3) or tail.shape[1] < 1:
        raise UniGenHipError(f"{who}: the tails must be [R, S] ids or [R, S, H] embeddings with S >= 1, got {tuple(tail.shape)}")
    R, S = int(tail.shape[0]), int(tail.shape[1])
    if R < 1 or R > MMU_MAX_ROWS:
        raise UniGenHipError(f"{who}: {R} rows (at most {MMU_MAX_ROWS} per call)")
    if attention_mask is not None:
        raise UniGenHipError(f"{who}: a dense attention_mask cannot be combined with a prefix (the tails are causal; mark their "
                             f"left pads with tail_valid)")
    if tail_valid is not None:
        tail_valid = torch.as_tensor(tail_valid)
        if tuple(tail_valid.shape) != (R, S):
            raise UniGenHipError(f"{who}: tail_valid must be [{R}, {S}], got {tuple(tail_valid.shape)}")
        tail_valid = tail_valid != 0
        if not bool(tail_valid.any(0).all()):
            raise UniGenHipError(f"{who}: a tail position is a pad in every row (left-pad the tails to the longest one only)")
    return R, S, tail_valid


ScoreResult = collections.namedtuple("ScoreResult", ["logprob", "is_greedy", "token_logprobs"])
ScoreResult.__doc__ = """What `UniGen.score` returns: logprob fp32 [R] (the continuation's log-probability: the sum over its tokens, or
their mean with average=True), is_greedy bool [R] (every token of the continuation is the argmax of its position: greedy decoding
would have emitted it), token_logprobs fp32 [R, C] (0.0 at the pads of `targets`)."""


def check_score_call(who, engine, prefix, idx, input_embeddings, targets, tail_valid, image_codes_from=None):
    """The argument checks of `UniGen.score`, all on the host and before anything is launched
    -> (rows, context length, continuation length, tail_valid as a bool tensor or None, the real-target mask bool [R, C] on the CPU)."""
    if (idx is None) == (input_embeddings is None):
        raise UniGenHipError(f"{who}: give the rows' contexts as idx [R, S] or input_embeddings [R, S, H] (one of the two)")
    ctx = idx if input_embeddings is None else input_embeddings
    if ctx.dim() != (2 if input_embeddings is None else 3) or ctx.shape[0] < 1 or ctx.shape[1] < 1:
        raise UniGenHipError(f"{who}: the contexts must be [R, S] ids or [R, S, H] embeddings with R, S >= 1, got {tuple(ctx.shape)}")
    R, S = int(ctx.shape[0]), int(ctx.shape[1])
    if input_embeddings is not None and ctx.shape[2] != engine.dims.hidden_size:
        raise UniGenHipError(f"{who}: input_embeddings must be {engine.dims.hidden_size} wide, got {tuple(ctx.shape)}")
    if not torch.is_tensor(targets) or targets.dim() != 2 or targets.shape[0] != R or targets.shape[1] < 1 or targets.dtype != torch.int64:
        raise UniGenHipError(f"{who}: targets must be an int64 [{R}, C] tensor of continuation ids, right-padded with -100, got "
                             f"{tuple(targets.shape) if torch.is_tensor(targets) else type(targets).__name__}")
    C = int(targets.shape[1])
    on_host = targets.device.type == "cpu"
    t = targets if on_host else targets.cpu()                # (a copy, not a launch: the pad pattern decides the shapes of the call)
    real = t != -100
    if not bool(real.any(1).all()):
        raise UniGenHipError(f"{who}: row {int((~real.any(1)).nonzero()[0])} of targets has no real target (only -100)")
    if not bool((real[:, 1:] <= real[:, :-1]).all()):
        raise UniGenHipError(f"{who}: targets must be RIGHT-padded with -100 (a real id follows a pad)")
    V = engine.dims.vocab_size
    if on_host and bool(((t < 0) | (t >= V))[real].any()):
        raise UniGenHipError(f"{who}: target ids must lie in [0, {V}) (or be the pad -100)")
    if image_codes_from is not None and on_host and bool((t >= image_codes_from)[real].any()):
        raise UniGenHipError(f"{who}: image-code targets (ids >= {image_codes_from}) cannot be scored on a model with a gen_projector: "
                             f"their inputs go through gen_embed, which this call does not apply")
    if prefix is not None:
        check_prefix(who, engine, prefix, ctx, "contexts")
    if tail_valid is not None:
        tail_valid = torch.as_tensor(tail_valid)
        if tuple(tail_valid.shape) != (R, S):
            raise UniGenHipError(f"{who}: tail_valid must be [{R}, {S}], got {tuple(tail_valid.shape)}")
        tail_valid = tail_valid != 0
        if not bool(tail_valid[:, -1].all()):
            raise UniGenHipError(f"{who}: contexts are LEFT-padded: every row's last context position must be a real one")
    return R, S, C, tail_valid, real


class UniGen(ModelMixin, ConfigMixin):
    _supports_gradient_checkpointing = True

    @register_to_config
    def __init__(
            self,
            w_und_encoder: bool,
            vocab_size: int,
            llm_vocab_size: int,
            llm_model_path: str = '',
            codebook_size: int = 8192,
            num_vq_tokens: int = 256,
            load_from_pretrained: bool = True,
            mm_input_dim: int = 1024,
            gen_input_dim: int = 16,
            und_proj_depth: int = 0,
            gen_proj_depth: int = 0,
            use_gen_dim: bool = False,
            rope_theta: Optional[float] = None,
            scaling_factor: float = 1.0,
            rope_type: str = 'linear',
            vision_tower_name: Optional[str] = None,
            ckpt_base_path: str = "",
            **kwargs,
    ):
        super().__init__()
        device = kwargs.get("device", None) or torch.device("cuda", torch.cuda.current_device())
        self.vocab_size = vocab_size
        self.num_vq_tokens = num_vq_tokens
        llm_cfg = _load_llm_config(llm_model_path, ckpt_base_path)
        self.register_to_config(hidden_size=llm_cfg["hidden_size"])
        llm_cfg["vocab_size"] = vocab_size          # reference: config.vocab_size = vocab_size / resize_token_embeddings
        # reference :58-64: rope_theta / scaling_factor / rope_type override the config ONLY in the load_from_pretrained=True
        # branch (random init from config); with load_from_pretrained=False (HF weights) the reference ignores all three
        if load_from_pretrained and rope_theta is not None:
            llm_cfg["rope_theta"] = rope_theta
        if load_from_pretrained and scaling_factor != 1:
            llm_cfg["rope_scaling"] = {"factor": float(scaling_factor), "type": rope_type}
        dims = Qwen2Dims(**llm_cfg)
        seed = kwargs.get("init_seed", None)
        if seed is None:
            seed = int(torch.initial_seed() % (2 ** 31))
        elif seed < 0:              # caller initialises / loads the weights itself (checkpoints, device-side init)
            seed = None
        # load_from_pretrained=True in the reference means "random-init from config" (sic, unigen.py:58-65);
        # False means "load HF weights from llm_model_path".
        self.llm = HipQwen2ForCausalLM(dims, device, seed=seed)
        if not load_from_pretrained:
            self._load_hf_llm_weights(llm_model_path, ckpt_base_path)
        self.output_size = self.vocab_size
        self.img_output_size = codebook_size
        if gen_proj_depth > 0:
            # separate image-token embedding + MLP into the backbone and an 8192-way head out of it (reference :74-90)
            hidden = llm_cfg["hidden_size"]
            if use_gen_dim:
                self.gen_embed = torch.nn.Embedding(codebook_size + 1, gen_input_dim)
                layers, width = [torch.nn.Linear(gen_input_dim, hidden)], hidden
            else:
                self.gen_embed = torch.nn.Embedding(codebook_size + 1, hidden)
                layers, width = [torch.nn.Linear(hidden, hidden * 2)], hidden * 2
            for _ in range(1, gen_proj_depth):
                layers += [torch.nn.GELU(), torch.nn.Linear(width, hidden)]
                width = hidden
            self.gen_projector = HipProjector(*layers)
            self.img_head = torch.nn.Linear(hidden, codebook_size, bias=False)
            for m in (self.gen_embed, self.gen_projector, self.img_head):
                m.to(device)
            self.register_to_config(mask_token_id=codebook_size)
        else:
            self.register_to_config(mask_token_id=vocab_size - 1)
        self._loss_idx_cache = {}
        # text decode on the device (generate / mmu_generate / mmu_generate_batch: `on_device=None` follows this); opt-in, so that
        # unchanged callers can turn it on from the environment
        self.text_decode_on_device = os.environ.get("UNIGEN_TEXT_ON_DEVICE", "0") == "1"
        # Data parallelism (reference: accelerator.prepare wraps the model in DistributedDataParallel, train.py:492).
        # The backbone's parameters are views of one flat buffer whose gradients the kernels write directly and
        # unigen_hip.ddp.FlatGradSync averages, so DDP's reducer must leave them alone (see
        # `_ddp_params_and_buffers_to_ignore`); `_ddp_anchor` is the one ordinary parameter DDP always finds (it refuses
        # a module with none) and the input that puts the engine's autograd Functions on every graph.  It receives a
        # zero gradient per backward and never changes.
        eng = self.llm.engine
        self._ddp_anchor = torch.nn.Parameter(torch.zeros(1, device=eng.device))
        eng._anchor = self._ddp_anchor
        eng.extra_grad_params = self._ordinary_grad_params
        self.__dict__["_ddp_wrapper"] = None          # weakref to the DistributedDataParallel instance wrapping this model, if any
        self._register_state_dict_hook(_drop_anchor_from_state_dict)
        self.register_load_state_dict_post_hook(_forgive_missing_anchor)
        if w_und_encoder:
            if vision_tower_name is not None:
                self.init_vision_tower(vision_tower_name)
            self.add_mm_projector(max(2, und_proj_depth), mm_input_dim)

    # ------------------------------------------------------------------ data parallel plumbing
    def _flat_view_ids(self):
        return {id(p) for p in self.llm.engine.named_param_views().values()}

    @property
    def _ddp_params_and_buffers_to_ignore(self):
        """Read by torch's DistributedDataParallel constructor (nn/parallel/distributed.py: parameters_to_ignore): every
        name under which a flat-view parameter is reachable, including the tied `llm.lm_head.weight`.  Side-effect free:
        whether a wrapper exists is recorded by `_note_ddp_wrapper` below when DistributedDataParallel registers this model
        as its `.module`, and the flat weights are aligned to rank 0 at the first training forward (`TrainEngine._dp_sync`),
        which every rank reaches together."""
        flat = self._flat_view_ids()
        return [f"{mn}.{pn}" if mn else pn for mn, m in self.named_modules() for pn, p in m.named_parameters(recurse=False)
                if id(p) in flat]

    def _is_ddp_wrapped(self):
        """True while a live DistributedDataParallel instance holds this model: its reducer then averages the ordinary
        parameters (mm_projector, gen_*) and FlatGradSync only moves the flat buffer."""
        ref = self.__dict__.get("_ddp_wrapper")
        return ref is not None and ref() is not None

    def _ordinary_grad_params(self):
        if self._is_ddp_wrapped():
            return []
        flat = self._flat_view_ids()
        return [p for p in self.parameters() if id(p) not in flat and p is not self._ddp_anchor and p.requires_grad]

    def no_sync(self):
        """Context manager for gradient-accumulation micro-steps outside accelerate (inside it, `accelerator.accumulate`
        is honoured automatically): backward passes run here add to the local gradients and exchange nothing."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            eng = self.llm.engine
            prev, eng.require_grad_sync = eng.require_grad_sync, False
            try:
                yield
            finally:
                eng.require_grad_sync = prev
        return ctx()

    # ------------------------------------------------------------------ construction helpers
    def _load_hf_llm_weights(self, llm_model_path, ckpt_base_path):
        path = llm_model_path
        if ckpt_base_path and not os.path.exists(str(path)):
            path = os.path.join(ckpt_base_path, os.path.basename(str(llm_model_path).rstrip("/")))
        files = [f for f in os.listdir(path) if f.endswith(".safetensors")]
        if not files:
            raise UniGenHipError(f"no *.safetensors under {path}")
        from safetensors.torch import load_file
        sd = {}
        for f in files:
            sd.update(load_file(os.path.join(path, f)))
        own = self.llm.state_dict()
        V_ckpt = sd["model.embed_tokens.weight"].shape[0]
        with torch.no_grad():
            for k, v in sd.items():
                if k == "lm_head.weight" or k not in own:
                    continue
                if k == "model.embed_tokens.weight":      # == resize_token_embeddings(vocab_size) (unigen.py:68-69)
                    n = min(V_ckpt, own[k].shape[0])
                    own[k][:n].copy_(v[:n])
                else:
                    own[k].copy_(v)

    def _set_gradient_checkpointing(self, module, value=False):
        self.gradient_checkpointing = True

    def resize_token_embeddings(self, vocab_size):
        self.vocab_size = vocab_size
        self.llm.resize_token_embeddings(self.vocab_size)
        self.output_size = self.vocab_size

    def init_vision_tower(self, vision_tower_name):
        from .multimodal_encoder.builder import get_vision_tower
        self.register_to_config(vision_tower_name=vision_tower_name)
        if self.config.ckpt_base_path:
            vision_tower_name = os.path.join(self.config.ckpt_base_path, os.path.basename(vision_tower_name.rstrip("/")))
        self.vision_tower = get_vision_tower(vision_tower_name, freeze=False)

    def add_vision_tower(self, config):
        vision_tower_name = config.model.vision_tower.name
        self.init_vision_tower(vision_tower_name)
        vt = self.vision_tower
        mm_input_dim = vt.config.hidden_size if hasattr(vt, 'config') else vt.hidden_size
        self.add_mm_projector(config.model.unigen.get('und_proj_depth', 2), mm_input_dim)

    def add_mm_projector(self, mlp_depth, mm_input_dim):
        self.register_to_config(w_und_encoder=True)
        self.register_to_config(mm_input_dim=mm_input_dim)
        self.register_to_config(und_proj_depth=mlp_depth)
        hidden = self.config.hidden_size
        layers = [torch.nn.Linear(mm_input_dim, hidden)]
        for _ in range(1, mlp_depth):
            layers += [torch.nn.GELU(), torch.nn.Linear(hidden, hidden)]
        from unigen_hip.modules import HipProjector
        self.mm_projector = HipProjector(*layers).to(self.llm.engine.device)

    def _use_gen(self):
        return self.config.get('gen_proj_depth', 0) > 0

    def get_gen_embed(self, img_tokens):
        """gen_projector(gen_embed(img_tokens)) (reference :130-131); img_tokens are raw codes 0..codebook_size (the
        last id is this path's mask token)."""
        if not self._use_gen():
            raise UniGenHipError("get_gen_embed needs a model built with gen_proj_depth > 0")
        eng = self.llm.engine
        e = _TableEmbedFn.apply(self.gen_embed.weight, img_tokens.to(eng.device), eng.err_flag)
        return self.gen_projector(e)

    def prepare_inputs_for_t2i(self, input_ids, num_vq_tokens):
        emb = self.llm.model.embed_tokens(input_ids)
        if self._use_gen():                       # image slots carry the projected gen embeddings instead (reference :230-238)
            img = self.get_gen_embed(input_ids[:, -(num_vq_tokens + 1):-1].contiguous()).to(emb.dtype)
            emb = torch.cat([emb[:, :-(num_vq_tokens + 1)], img, emb[:, -1:]], dim=1)
        return emb

    def _img_head(self, hn):
        return _LinearFn.apply(hn, self.img_head.weight, None)

    def prepare_inputs_for_mmu(self, image_feats, spatial_shapes, input_ids, label_ids, prompt_template, input_ids_system=None):
        """Understanding-sample assembly for variable-size image features (reference models/unigen.py:133-228; callers
        training/train_w_clip_vit.py:754,801).  Row i is
            [system] <|im_start|><|mmu|><|soi|> | mm_projector(image_feats[i, :h_i*w_i]) | <|eoi|> input_ids[i, 1:] | pad...
        cut to `prompt_template.max_seq_len`; labels are ignore_id up to and including <|eoi|>, then label_ids[i, 1:],
        pads ignored; the key-validity mask is cut after the last `eos_token_id` label of the first row that has one (sic).  Returns (embeddings [B, L, H],
        attention_mask bool [B, max_seq_len], labels [B, L], input_ids_part1 [B, L1]).  One index computation for the
        whole batch instead of the reference's per-row concatenations; the projector and the embedding lookup run on the
        HIP kernels and stay differentiable."""
        pt = prompt_template
        dev = input_ids.device
        B, Lt = input_ids.shape
        N = image_feats.shape[1]
        pad_id, ignore, max_len = pt.text_tokenizer.pad_token_id, pt.ignore_id, pt.max_seq_len
        sp = pt.sptids_dict
        head = ['<|mmu|>', '<|im_start|>', '<|soi|>'] if pt.task_token_first else ['<|im_start|>', '<|mmu|>', '<|soi|>']
        part1 = torch.tensor([int(sp[t]) for t in head], dtype=torch.long, device=dev)[None].expand(B, 3)
        if input_ids_system is not None:
            part1 = torch.cat([input_ids_system.to(dev).long(), part1], dim=1)
        part1 = part1.contiguous()
        L1 = part1.shape[1]
        n_img = (spatial_shapes[:, 0] * spatial_shapes[:, 1]).to(dev).long()                      # [B]
        # row lengths before the cut: embeddings carry N trailing pads when training, (max_i n_img - n_img[i]) otherwise;
        # the label rows always carry N trailing ignore entries (reference :176-203)
        emb_len = L1 + n_img + Lt + (N if self.training else int(n_img.max()) - n_img)
        lab_len = L1 + n_img + Lt + N

        def common_length(lens, what):
            lo, hi = int(lens.min()), int(lens.max())
            if lo < max_len and lo != hi:
                raise UniGenHipError(f"prepare_inputs_for_mmu: {what} rows shorter than max_seq_len differ in length")
            return min(lo, max_len)
        T, T_lab = common_length(emb_len, "embedding"), common_length(lab_len, "label")
        const = lambda v: torch.full((), int(v), dtype=torch.long, device=dev)

        p = torch.arange(T, device=dev)[None]                                                     # [1, T]
        q = p - L1 - n_img[:, None]                                                               # offset into the text part
        is_img = (p >= L1) & (q < 0)
        text = torch.cat([const(sp['<|eoi|>']).expand(B, 1), input_ids[:, 1:].long()], dim=1)     # <|eoi|> replaces column 0
        ids = torch.where((q >= 0) & (q < Lt), text.gather(1, q.clamp(0, Lt - 1)), const(pad_id))
        head_ids = torch.nn.functional.pad(part1, (0, max(0, T - L1)), value=pad_id)[:, :T]
        ids = torch.where(p < L1, head_ids, ids)
        image_embeds = self.mm_projector(image_feats)                                             # [B, N, H]
        emb = self.llm.model.embed_tokens(ids)                                                    # image slots: pad rows, replaced below
        slot = (p - L1).clamp(0, N - 1).expand(B, T)
        img_rows = image_embeds.gather(1, slot[..., None].expand(B, T, image_embeds.shape[-1])).to(emb.dtype)
        full_embeddings = torch.where(is_img[..., None], img_rows, emb)

        if label_ids is None:
            label_ids = input_ids.clone()
        ql = torch.arange(T_lab, device=dev)[None] - L1 - n_img[:, None]
        labels = torch.where((ql >= 1) & (ql < Lt), label_ids.to(dev).long().gather(1, ql.clamp(0, Lt - 1)), const(ignore))
        labels = torch.where(labels == pad_id, const(ignore), labels)
        # key-validity mask (:211-226).  The reference walks the (row, column) list of eos labels with a cursor that never
        # moves past the first row it matched, so ONLY the first row that contains an eos label is cut (after its last
        # eos); every other row -- with or without eos labels -- stays fully valid.  Reproduced as is.
        is_eos = labels == pt.eos_token_id
        has = is_eos.any(1)
        first_row = torch.where(has.any(), has.long().argmax(), const(-1))
        last_eos = T_lab - 1 - is_eos.flip(-1).long().argmax(1)
        cut = torch.where(torch.arange(B, device=dev) == first_row, last_eos, const(T_lab - 1))
        attention_mask = torch.arange(max_len, device=dev)[None] <= cut[:, None]
        return full_embeddings, attention_mask, labels, part1

    # ------------------------------------------------------------------ forward
    def _loss_rows(self, B, L, bt, blm, bmmu, n, mode, device, lm_start=None):
        """Row indices (into [B*L]) of the logits each loss reads and of the labels it compares to
        (the slices of models/unigen.py:310-338)."""
        lm0 = bt if lm_start is None else lm_start
        key = (B, L, bt, blm, bmmu, n, mode, lm0)
        if key not in self._loss_idx_cache:
            def grid(b0, b1, p0, p1):
                b = torch.arange(b0, b1, device=device)[:, None] * L
                return (b + torch.arange(p0, p1, device=device)[None, :]).reshape(-1)
            segs = []
            if mode == 'mask':
                segs.append((grid(0, bt, L - (n + 1), L - 1), 0))
            else:
                segs.append((grid(0, bt, L - (n + 2), L - 1), 1))
            if blm > 0:
                segs.append((grid(lm0, lm0 + blm, 0, L - 1), 1))
            if bmmu > 0:
                segs.append((grid(B - bmmu, B, 0, L - 1), 1))
            bounds, r = [], 0
            for ix, _ in segs:
                bounds.append((r, r + ix.numel()))
                r += ix.numel()
            idx = torch.cat([ix for ix, _ in segs]) if r > 0 else torch.zeros(0, dtype=torch.long, device=device)
            lab = torch.cat([ix + s for ix, s in segs]) if r > 0 else idx
            self._loss_idx_cache[key] = (idx, lab, bounds)
        return self._loss_idx_cache[key]

    def forward(
            self,
            input_ids: torch.LongTensor,
            input_embeddings: Optional[torch.Tensor] = None,
            attention_mask: Optional[torch.Tensor] = None,
            labels: Optional[torch.LongTensor] = None,
            label_smoothing: float = 0.0,
            batch_size_t2i: int = 0,
            batch_size_lm: int = 0,
            batch_size_mmu: int = 0,
            max_seq_length: int = 128,
            num_vq_tokens: int = 256,
            t2i_mode: str = 'mask',
            **kwargs,
    ):
        eng = self.llm.engine
        gen = self._use_gen() and batch_size_t2i > 0
        if gen and input_embeddings is None:
            # the gen_projector path embeds the image slots through gen_embed + gen_projector; their ids are the raw
            # codes there (mask id = codebook_size), so the token-table lookup runs with those slots neutralised
            n = num_vq_tokens
            safe = input_ids.clone()
            safe[:, -(n + 1):-1] = 0
            emb = self.llm.model.embed_tokens(safe)
            img = self.get_gen_embed(input_ids[:, -(n + 1):-1].contiguous()).to(emb.dtype)
            input_embeddings = torch.cat([emb[:, :-(n + 1)], img, emb[:, -1:]], dim=1)
        if input_embeddings is None:
            out = self.llm.model(input_ids=input_ids, attention_mask=attention_mask)
        else:
            out = self.llm.model(inputs_embeds=input_embeddings, attention_mask=attention_mask)
        hn = out.last_hidden_state                                  # bf16 [B, L, H] (final norm applied)
        if gen:
            return self._forward_gen_head(hn, labels, batch_size_t2i, batch_size_lm, batch_size_mmu, num_vq_tokens, t2i_mode)
        if labels is None:
            return LazyLogits(eng, hn)          # stays on the autograd graph: DPO differentiates through its slices
        logits = LazyLogits(eng, hn.detach())
        B, L, _ = hn.shape
        idx, lab_idx, bounds = self._loss_rows(B, L, batch_size_t2i, batch_size_lm, batch_size_mmu, num_vq_tokens,
                                               t2i_mode, hn.device)
        nan = torch.full((), float("nan"), device=hn.device)
        if idx.numel() == 0:
            return logits, nan, 0., 0.
        lab = labels.to(hn.device).reshape(-1)[lab_idx].contiguous()
        live = [(s, b) for s, b in enumerate(bounds) if b[1] > b[0]]
        losses = _HeadLossFn.apply(eng._anchor, hn, eng, idx, lab, tuple(b for _, b in live))
        by_seg = {s: losses[j] for j, (s, _) in enumerate(live)}
        s = 0
        loss_t2i = by_seg.get(s, nan)
        s += 1
        loss_lm = 0.
        if batch_size_lm > 0:
            loss_lm = by_seg[s]
            s += 1
        loss_mmu = 0.
        if batch_size_mmu > 0:
            loss_mmu = by_seg[s]
        return logits, loss_t2i, loss_lm, loss_mmu

    def _forward_gen_head(self, hn, labels, bt, blm, bmmu, n, t2i_mode):
        """gen_proj_depth > 0 branch of forward (reference :255-341): the t2i rows go through img_head (codebook-wide
        logits, labels are raw codes), lm / mmu rows through the tied lm_head exactly as in the default branch; the first
        return value is img_logits."""
        eng = self.llm.engine
        B, L, _ = hn.shape
        img_logits = self._img_head(hn[:bt])                          # bf16 [bt, L, codebook]
        if labels is None:
            return img_logits
        labels = labels.to(hn.device)
        C = self.img_output_size
        if t2i_mode == 'mask':
            lg, lb = img_logits[:, -(n + 1):-1], labels[:bt, -(n + 1):-1]
        else:
            lg, lb = img_logits[:, -(n + 2):-1], labels[:bt, -(n + 1):]
        loss_t2i = _CrossEntropyFn.apply(lg.reshape(-1, C), lb.reshape(-1).contiguous())
        loss_lm, loss_mmu = 0., 0.
        if blm > 0 or bmmu > 0:
            idx, lab_idx, bounds = self._loss_rows(B, L, 0, blm, bmmu, n, t2i_mode, hn.device, lm_start=bt)
            lab = labels.reshape(-1)[lab_idx].contiguous()
            live = [(s, b) for s, b in enumerate(bounds) if b[1] > b[0]]
            losses = _HeadLossFn.apply(eng._anchor, hn, eng, idx, lab, tuple(b for _, b in live))
            by_seg = {s: losses[j] for j, (s, _) in enumerate(live)}
            s = 1
            if blm > 0:
                loss_lm = by_seg[s]
                s += 1
            if bmmu > 0:
                loss_mmu = by_seg[s]
        return img_logits, loss_t2i, loss_lm, loss_mmu

    # ------------------------------------------------------------------ MaskGIT generation
    @torch.no_grad()
    def t2i_generate(
            self,
            input_ids: Optional[torch.LongTensor] = None,
            uncond_input_ids: Optional[torch.LongTensor] = None,
            input_embeddings: Optional[torch.Tensor] = None,
            uncond_input_embeddings: Optional[torch.Tensor] = None,
            attention_mask: Optional[torch.Tensor] = None,
            temperature: float = 1.0,
            timesteps: int = 18,
            guidance_scale: int = 0,
            noise_schedule=cosine_schedule,
            generator: Optional[torch.Generator] = None,
            image_token_num_per_image: int = 256,
            text_vocab_size: int = 151936,
            top_k: Optional[int] = 0,
            top_p: Optional[float] = 1.0,
            min_p: Optional[float] = 0.0,
            sampling_temperature: Optional[float] = 1.0,
            return_logprobs: bool = False,
            **kwargs,
    ):
        """Iterative parallel decoding; step-for-step the procedure of reference models/unigen.py:344-455
        (incl. its quirks: untempered multinomial, compounded Gumbel temperature, >=1 token re-masked
        even on the last step, `sampled_ids` returned).
        top_k / top_p / min_p / sampling_temperature: every round draws its tokens from the truncated, tempered distribution, in the
        order temperature -> top-k -> top-p -> min-p -> draw (0 / 1.0 / 0.0 / 1.0 or None: off, the reference's draw).  The filters are
        the value thresholds of `t2i_generate_ar` (ties at the top-k value all kept, a run of equal logits kept or dropped whole by
        top-p), found on the device by the round's one fused launch (include/unigen_hip.h: ug_maskgit_step_ex); the confidence that
        decides re-masking is the token's probability under the distribution it was drawn from.  `temperature` stays the
        Gumbel / confidence temperature.
        return_logprobs: returns (sampled_ids [bsz, n], logprobs [bsz, n], cond_logprobs [bsz, n]), the last two fp32 on the device.
        Entry [b, i] belongs to the round that drew the returned token -- the last round at whose start position i was still masked:
        logprobs is its natural-log probability under the drawn-from distribution (after CFG, sampling temperature and truncation),
        cond_logprobs the conditional model's own log-softmax at it.  Positions already known in `input_ids` get 0.0.  One buffer,
        zeroed once, that every round's launch overwrites at masked positions only: no extra pass over the logits, no host work per
        round.
        kwargs: incremental=False recomputes the prefix every round; trace=list receives (sampled_ids, next_ids) of every round,
        logit_trace=list a clone of every round's bf16 code-book logits."""
        top_k = 0 if top_k is None else top_k
        top_p = 1.0 if top_p is None else float(top_p)
        min_p = 0.0 if min_p is None else float(min_p)
        sampling_temperature = 1.0 if sampling_temperature is None else float(sampling_temperature)
        if not (isinstance(top_k, int) and top_k >= 0 and 0.0 < top_p <= 1.0 and 0.0 <= min_p <= 1.0 and sampling_temperature > 0.0):
            raise UniGenHipError(f"t2i_generate: need an int top_k >= 0, 0 < top_p <= 1, 0 <= min_p <= 1 and sampling_temperature > 0 "
                                 f"(got top_k={top_k!r}, top_p={top_p!r}, min_p={min_p!r}, sampling_temperature={sampling_temperature!r})")
        n = image_token_num_per_image
        mask_token_id = self.config.mask_token_id
        embed = self.llm.model.embed_tokens
        cur_ids = input_ids[:, -(n + 1):-1].clone()
        gen = self._use_gen()                        # gen_projector path: raw codes in, gen embeddings, img_head out (:372-373)
        if input_embeddings is None:
            input_embeddings = embed(input_ids)
        image_embeddings = (self.get_gen_embed(cur_ids).to(input_embeddings.dtype) if gen
                            else input_embeddings[:, -(n + 1):-1])
        bsz = image_embeddings.shape[0]
        prefix = input_embeddings[:, :-(n + 1)]
        suffix = input_embeddings[:, -1:]
        cfg = guidance_scale > 1
        if cfg:
            un_prefix = (embed(uncond_input_ids[:, :-(n + 1)]) if uncond_input_embeddings is None
                         else uncond_input_embeddings[:, :-(n + 1)])
            prefix = torch.cat([prefix, un_prefix])
            suffix = torch.cat([suffix, suffix])
        sampled_ids = None
        eng = self.llm.engine
        L = prefix.shape[1] + n + 1
        seg_start = L - n - 2                        # <soi> | n image tokens | <eoi>
        # Prefix rows (padding + text) must not see the image segment for their keys / values to be round-invariant;
        # true for every mask the reference builds (create_attention_mask_predict_next), checked on the mask given.
        incremental = bool(kwargs.get("incremental", True)) and not torch.is_grad_enabled() and attention_mask is not None
        if incremental and isinstance(attention_mask, ops.MaskBits):
            # compressed mask (ops.mask_from_ids): no bit of a prefix row may be set at or beyond the segment's first column
            w0, sh = seg_start // 64, seg_start % 64
            words = attention_mask.bits[:, :seg_start, w0:]
            keep = torch.full((words.shape[-1],), -1, dtype=torch.int64, device=words.device)
            keep[0] = -1 << sh                           # the straddling word: only columns >= seg_start count
            incremental = not bool(((words & keep) != 0).any())
        elif incremental:
            incremental = torch.is_tensor(attention_mask) and attention_mask.dim() == 4 \
                and not bool((attention_mask[:, 0, :seg_start, seg_start:] == 0).any())
        sess = None
        trace = kwargs.get("trace", None)
        logit_trace = kwargs.get("logit_trace", None)
        logp = torch.zeros((bsz * n, 2), dtype=torch.float32, device=image_embeddings.device) if return_logprobs else None
        for step in range(timesteps):
            img = torch.cat([image_embeddings, image_embeddings]) if cfg else image_embeddings
            if incremental:
                R = img.shape[0]
                if sess is None:
                    seq = torch.cat([prefix, img, suffix], 1).float()
                    mb = eng.mask_bits(attention_mask, R, L)
                    sess, hn = eng.maskgit_begin(seq.reshape(R * L, -1).contiguous(), mb, L, seg_start)
                    eng.check_errors()
                else:
                    seg = torch.cat([prefix[:, -1:], img, suffix], 1).float()
                    hn = eng.maskgit_step(sess, seg.reshape(R * (n + 2), -1).contiguous())
                rows = hn.view(R, n + 2, -1)[:, 1:n + 1].reshape(R * n, -1).contiguous()
                lg = (self._img_head(rows) if gen else eng.head_slice(rows, text_vocab_size, self.vocab_size - 1)).reshape(R, n, -1)
            elif gen:
                seq = torch.cat([prefix, img, suffix], 1)
                hn = self.llm.model(inputs_embeds=seq, attention_mask=attention_mask).last_hidden_state
                lg = self._img_head(hn[:, -(n + 1):-1].contiguous())
            else:
                seq = torch.cat([prefix, img, suffix], 1)
                out = self(input_ids=input_ids, input_embeddings=seq, attention_mask=attention_mask)
                # only the image positions x codebook columns are ever read (reference slices the dense logits)
                lg = out[:, -(n + 1):-1, text_vocab_size:-1]
            ratio = 1.0 * (step + 1) / timesteps
            mask_len = int(torch.floor(n * noise_schedule(torch.tensor(ratio))).item())
            temperature = temperature * (1.0 - ratio)
            # one fused step on the device: CFG mix, softmax, categorical draw (inverse CDF on uniforms from `generator`),
            # confidence + Gumbel noise, re-masking of the max(1, min(#unknown - 1, mask_len)) least confident positions
            u_dev = lg.device if generator is None else generator.device
            u = torch.rand((2, bsz, n), device=u_dev, generator=generator).to(lg.device)
            lg = lg.contiguous()
            if logit_trace is not None:
                logit_trace.append(lg.clone())
            sampled_ids, cur_ids, next_ids = ops.maskgit_step(lg, bsz, n, cfg, guidance_scale, u[0], u[1], cur_ids,
                                                              mask_token_id, 0 if gen else text_vocab_size, mask_len, temperature,
                                                              top_k=top_k, top_p=top_p, min_p=min_p,
                                                              sample_temperature=sampling_temperature, logp=logp)
            if trace is not None:                        # parity tests follow the trajectory round by round
                trace.append((sampled_ids.clone(), next_ids.clone()))
            image_embeddings = self.get_gen_embed(next_ids).to(input_embeddings.dtype) if gen else embed(next_ids)
        if return_logprobs:
            logp = logp.view(bsz, n, 2)
            return sampled_ids, logp[..., 0].contiguous(), logp[..., 1].contiguous()
        return sampled_ids

    # ------------------------------------------------------------------ autoregressive generation
    def drop_decode_session(self):
        """Release the decode step kept from the last `t2i_generate_ar` call: the static KV cache of every layer (rows x (prefix + n)
        tokens), the decode scratch, and the captured graph with its private memory pool -- hundreds of MB that otherwise stay
        allocated until a call with different shapes replaces them.  `train(True)` calls this (periodic evaluation inside a training
        run must not keep generation buffers for the rest of it); `UNIGEN_AR_GRAPH_CACHE=0` disables keeping a session at all.
        Prefix objects (`mmu_prefix`) are not touched: the caller owns them and drops them by dropping the reference."""
        eng = getattr(getattr(self, "llm", None), "engine", None)
        if eng is not None:
            eng._ar_session = None
            eng._text_session = None              # (the on-device text loop keeps one too: _decode_text_on_device)
            eng._spec_session = None              # (and its speculative form: _decode_text_spec)

    def train(self, mode: bool = True):
        if mode:
            self.drop_decode_session()
        return super().train(mode)

    @torch.no_grad()
    def t2i_generate_ar(
            self,
            input_ids: Optional[torch.LongTensor] = None,
            uncond_input_ids: Optional[torch.LongTensor] = None,
            input_embeddings: Optional[torch.Tensor] = None,
            uncond_input_embeddings: Optional[torch.Tensor] = None,
            attention_mask: Optional[torch.Tensor] = None,
            guidance_scale: int = 0,
            temperature: float = 1.0,
            text_vocab_size: int = 151936,
            image_token_num_per_image: int = 256,
            generator: Optional[torch.Generator] = None,
            deterministic: Optional[bool] = None,
            top_k: Optional[int] = 0,
            top_p: Optional[float] = 1.0,
            min_p: Optional[float] = 0.0,
            return_logprobs: bool = False,
            **kwargs,
    ):
        """Token-by-token image generation with CFG (reference models/unigen.py:457-521).  The reference
        only works when both embedding tensors are supplied; ids are accepted here too
        and embedded, which is what its callers intend.
        deterministic: decode with the ordered (atomic-free) kernels, so the same inputs, seed and generator give the same tokens on
        every call; None follows torch.are_deterministic_algorithms_enabled().
        top_k / top_p / min_p: truncated sampling in the order temperature -> top-k -> top-p -> min-p -> draw (0 / 1.0 / 0.0 or None:
        off).  Each is a value threshold (models/sampling.py: truncate_logits; in the captured step the fused sampler kernel finds
        it on the device): values tied at the top-k threshold are all kept, and top-p keeps or drops a run of equal logits as a
        whole, where a sorted cut would split it by the sort's order of equal keys.  `greedy` ignores them (the argmax is always
        kept).
        return_logprobs: returns (tokens [bsz, n], logprobs [bsz, n], cond_logprobs [bsz, n]), the last two fp32 on the device
        (include/unigen_hip.h: ug_ar_sample_logp).  logprobs[b, i] is the natural-log probability of token i under the distribution it
        was drawn from -- after CFG, temperature and truncation (greedy: the untruncated softmax at the call's temperature);
        cond_logprobs[b, i] is the conditional model's own log-softmax at that token, what a teacher-forced pass would score.  The
        captured step's sampler launch writes both (no extra pass over the logits, no host work per token); the unfused branch uses
        models/sampling.py: token_logprobs.  The flag is part of the kept session: a call with it never replays the graph of a call
        without it, nor the reverse."""
        from unigen_hip.qwen2 import ArDecodeSession, decode_loop, put_session, resolve_deterministic, take_session
        want_lp = bool(return_logprobs)
        top_k = 0 if top_k is None else top_k
        top_p = 1.0 if top_p is None else float(top_p)
        min_p = 0.0 if min_p is None else float(min_p)
        if not (isinstance(top_k, int) and top_k >= 0 and 0.0 < top_p <= 1.0 and 0.0 <= min_p <= 1.0):
            raise UniGenHipError(f"t2i_generate_ar: need an int top_k >= 0, 0 < top_p <= 1 and 0 <= min_p <= 1 "
                                 f"(got top_k={top_k!r}, top_p={top_p!r}, min_p={min_p!r})")
        det = resolve_deterministic(deterministic)
        gen = self._use_gen()          # gen_projector path (reference :486-495,512-514): img_head on the last hidden state, the next
        n = image_token_num_per_image  # input is gen_projector(gen_embed(raw code)); no text-vocabulary offset anywhere
        embed = self.llm.model.embed_tokens
        eng = self.llm.engine
        dev = eng.device
        if input_embeddings is None:
            input_embeddings = embed(input_ids)
        if uncond_input_embeddings is None:
            uncond_input_embeddings = embed(uncond_input_ids)
        bsz = input_embeddings.shape[0]
        prefix = torch.cat([input_embeddings[:, :-(n + 1)], uncond_input_embeddings[:, :-(n + 1)]]).float()
        R, P, _ = prefix.shape
        key_valid = None
        if attention_mask is not None:
            if attention_mask.dim() != 2:
                raise UniGenHipError("t2i_generate_ar expects the 2-D [rows, L] attention mask the reference slices")
            key_valid = attention_mask[:, :P].to(dev) != 0
        greedy = bool(kwargs.get("greedy", False))          # argmax instead of multinomial: deterministic parity tests
        logit_trace = kwargs.get("trace")                   # optional list: fp32 [rows, V] head logits of every eager step
        use_graph = bool(kwargs.get("use_graph", True))
        V = self.vocab_size - 1 - text_vocab_size                        # logits[..., text_vocab_size:-1]
        if top_k >= V:
            top_k = 0
        filt = (top_k, top_p, min_p) if not greedy and (top_k > 0 or top_p < 1.0 or min_p > 0.0) else None
        # fused: the lm-head as a weight-streaming GEMV into a raw fp32 accumulator + ONE sampling kernel per step
        # (Qwen2Engine.ar_step); otherwise the host sampler on the bf16 head slice (_ar_host_token)
        fused = (R <= 32 and eng.dims.hidden_size >= 256 and eng.dims.hidden_size % 32 == 0 and not kwargs.get("torch_sampler", False)
                 and not gen)
        # The captured decode step is kept ACROSS calls (round 5): Best-of-N generation calls this method once per prompt with the
        # same shapes (evaluation/inference_unigen_cot.py:318-331), and capturing costs ~6 ms of a 330 ms call (an eager warm-up
        # step + the capture).  A session (unigen_hip/qwen2.py: ArDecodeSession) = every buffer the graph reads or writes + the
        # graph; it is reused only when every size, every sampling constant baked into a kernel argument and the weight storage
        # are the same (UNIGEN_AR_GRAPH_CACHE=0 turns the reuse off), and dropped on any error.  Only the fused branch keeps one.
        form = eng.decode_form(R, det)               # (a captured step belongs to one layer form: its launches and scratch differ)
        sess_key = (R, P, n, bsz, V, int(text_vocab_size), greedy, float(guidance_scale), float(temperature), key_valid is None, str(dev),
                    form) + eng.storage_key(P + n) + (filt,)     # (the filter constants are kernel arguments of the captured sampler)
        if want_lp:
            sess_key += ("logprobs",)                        # (another sampler entry point and one more buffer in the captured step)
        sess = take_session(eng, "_ar_session", sess_key, use_graph and fused)
        if sess is not None:
            sess.begin(key_valid, generator)
        else:
            sess = ArDecodeSession(eng, R, bsz, P, n, V, text_vocab_size, guidance_scale, temperature, greedy, filt, deterministic=det,
                                   key_valid=key_valid, generator=generator, logprobs=want_lp, fused=fused)
            sess.key = sess_key
        timing = kwargs.get("timing")               # optional dict: wall seconds per phase (adds host syncs; measurement runs only)

        def mark(name, t0=[None]):
            if timing is not None:
                torch.cuda.synchronize()
                now = time.perf_counter()
                if t0[0] is not None:
                    timing[name] = timing.get(name, 0.0) + now - t0[0]
                t0[0] = now

        def record(i):                              # the host sampler's token and pair of step i (outside the captured step)
            sess.out_tokens[:, i] = sess.tok[:, 0]
            if want_lp:
                sess.logp[:, i] = sess.lp_now

        mark("setup")
        hn = eng.prefill(sess.st, prefix, key_valid)       # (capturing the prefill too was measured: 10.3 vs 10.6 ms, it is GPU-bound at 2 208 tokens)
        if fused:
            eng.ar_first_token(sess, hn, logit_trace)
            mark("prefill")
            decode_loop(sess, lambda: eng.ar_step(sess, logit_trace), range(1, n), use_graph, mark=mark)
        else:
            self._ar_host_token(sess, hn, generator, logit_trace)
            mark("prefill")
            record(0)
            # (the host sampler draws from `generator` on the host side of every step: a captured step could not)
            decode_loop(sess, lambda: self._ar_host_token(sess, eng.decode_step(sess.st, sess.x), generator, logit_trace), range(1, n),
                        use_graph and generator is None, mark=mark, after=record)
        eng.last_decode_graph = sess.graph is not None
        eng.last_decode_deterministic = det
        kept = put_session(eng, "_ar_session", sess, use_graph and fused)
        tokens = sess.out_tokens.clone() if kept else sess.out_tokens        # (a kept session's buffer is overwritten by the next call)
        return (tokens, sess.logp[..., 0].clone(), sess.logp[..., 1].clone()) if want_lp else tokens

    def _ar_host_token(self, sess, hn, generator, trace=None):
        """The host sampler's step of `t2i_generate_ar` (more than 32 rows, torch_sampler=True, the gen_projector path, hidden sizes the
        fused kernels refuse): from the final-norm hidden state `hn`, the bf16 head slice, CFG mix, temperature, truncation and
        torch.multinomial (greedy: argmax) -> sess.tok, the next input sess.x and, with log-probabilities, the step's pair sess.lp_now
        (models/sampling.py: token_logprobs).  Capturable when `generator` is None."""
        from .sampling import token_logprobs, truncate_logits
        gen, bsz = self._use_gen(), sess.bsz
        # (gen path: the reference mixes the bf16 img_head outputs in bf16 under autocast, :498-500)
        lg = self._img_head(hn) if gen else self.llm.engine.head_slice(hn, sess.code_lo, sess.code_lo + sess.V).float()
        cond, uncond = lg[:bsz], lg[bsz:]
        lg = (uncond + sess.guidance_scale * (cond - uncond)).float()
        if trace is not None and sess.lp_now is not None and not torch.cuda.is_current_stream_capturing():
            trace.append(torch.cat([cond, uncond]).float())
        if sess.greedy:
            nxt = lg.argmax(-1, keepdim=True)
            if sess.lp_now is not None:
                lg = lg / sess.temperature              # (the greedy log-probability is taken at the call's temperature)
        else:
            lg = lg / sess.temperature
            if sess.filt is not None:
                lg = truncate_logits(lg, top_k=sess.filt[0], top_p=sess.filt[1], min_p=sess.filt[2])
            nxt = torch.multinomial(torch.softmax(lg, dim=-1), num_samples=1, generator=generator)
        if sess.lp_now is not None:
            sess.lp_now[:, 0].copy_(token_logprobs(lg, nxt))
            sess.lp_now[:, 1].copy_(token_logprobs(cond, nxt))
        sess.tok.copy_(nxt)
        if gen:
            sess.x.copy_(self.get_gen_embed(torch.cat([nxt, nxt]))[:, 0])
        else:
            sess.x.copy_(self.llm.model.embed_tokens(torch.cat([nxt, nxt]) + sess.code_lo)[:, 0])

    # ------------------------------------------------------------------ plain causal generation
    @torch.no_grad()
    def generate(self, input_ids=None, input_embeddings=None, attention_mask=None, max_new_tokens=20, do_sample=False,
                 temperature=1.0, top_k=None, top_p=None, eos_token_id=None, pad_token_id=None, use_cache=True,
                 generator=None, deterministic=None, on_device=None, return_logprobs=False, prompt_lookup_num_tokens=None,
                 max_matching_ngram_size=None, lookup_ids=None, **kwargs):
        """Causal text generation with the conventions of transformers' `generate`, which the reference delegates to
        (models/unigen.py:584-588; caller evaluation/inference_unigen_cot.py:360): prompts as ids [B, L] or as
        `input_embeddings` [B, L, H] with an optional 2-D [B, L] key-validity mask (left padding); greedy when
        `do_sample` is false, otherwise temperature -> top-k -> top-p -> multinomial; a row that produced
        `eos_token_id` is filled with `pad_token_id` from then on and decoding stops when every row has finished.
        Returns prompt + continuation [B, L + new] for ids, the continuation alone [B, new] for embeddings (HF rule).
        One prefill into the static KV cache, then one decode step per token (`use_cache` is accepted and ignored: the
        recompute form would return the same tokens).  deterministic: ordered decode kernels (the same tokens on every call for the
        same inputs and generator); None follows torch.are_deterministic_algorithms_enabled().
        on_device: the token loop on the device (`_decode_text_on_device`: head over the whole vocabulary, pick, stop rule and next
        input as launches of a captured step kept across calls); None follows `self.text_decode_on_device` (False unless
        UNIGEN_TEXT_ON_DEVICE=1 at construction).  Greedy tokens are the host loop's wherever the top-2 margin exceeds the two heads'
        rounding.  SAMPLED tokens differ from the host loop's for the same seed: the uniforms are drawn up front as
        torch.rand((max_new_tokens, rows), generator=...) and used by an inverse CDF over the kept entries (top-k ties all kept, a
        run of equal logits kept or dropped whole by top-p), where the host loop calls torch.multinomial -- the feature is opt-in
        for that reason.  An explicit True on a call the loop cannot serve (more than 32 rows, use_cache=False, more than 8 stop
        ids, a hidden size below 256 or no multiple of 32) raises; a default-derived True falls back to the host loop.
        kwargs: use_graph=False runs the on-device steps eagerly; trace=list receives every eager step's raw fp32 head logits.
        repetition_penalty=p (finite, > 0; None or 1: off): transformers' RepetitionPenaltyLogitsProcessor ahead of temperature /
        top-k / top-p -- every id in the row's sequence so far (prompt ids at the positions the mask marks real + the tokens emitted;
        with an `input_embeddings` prompt the emitted tokens only) has its score multiplied by p if negative, divided by p otherwise.
        The host loop applies it in fp32 to the fp32 copy of the head's bf16 logits, the on-device loop to the bf16-rounded logit with
        the fp32 result stored back (include/unigen_hip.h: ug_text_penalize), so greedy tokens of the two loops can differ only where
        two processed values fall within one bf16 step of each other.
        num_return_sequences=n: every prompt row, with its mask row, is repeated n times consecutively before the prefill
        (transformers' order); the result has B * n rows.  n > 1 needs do_sample.  On the device the B * n rows draw independent
        uniforms from the one torch.rand((max_new_tokens, B * n)); the 32-row limit applies to B * n.
        return_logprobs: returns (sequences, logprobs fp32 [B * n, new]) -- transformers' compute_transition_scores(...,
        normalize_logits=True): the natural-log softmax of the PROCESSED scores (behind the repetition penalty, and when sampling the
        temperature and top-k / top-p) at every emitted token, aligned with the continuation columns and cut at the same step; a row
        that had finished before a step has 0.0 there (its pad ids), the step that emits the stop id its real value.  Greedy applies
        no temperature.  The host loop computes it in fp32 on the scores it picks from (models/sampling.py: token_logprobs), the
        on-device loop in its pick launches (include/unigen_hip.h: ug_text_pick_logp, ug_text_sample_logp) on the bf16-rounded
        scores; each is exact to its own formula, the two heads round differently.
        logit_bias={id: b}, suppress_tokens=[ids], min_new_tokens=m, no_repeat_ngram_size=n, stop_sequences=[[ids], ...] (kwargs; the
        semantics are stated once, in include/unigen_hip.h: "Constraints of the text loops"): transformers' SequenceBiasLogitsProcessor
        with keys of length 1, SuppressTokensLogitsProcessor, MinNewTokensLengthLogitsProcessor (every eos id scores -inf while fewer than
        m tokens have been emitted; stop sequences are not held back) and NoRepeatNGramLogitsProcessor on the row's history (the ids the
        repetition penalty counts, in order), in transformers' order: bias, repetition penalty, the -inf writers, then temperature /
        top-k / top-p.  A stop sequence of one id is an eos id; a longer one finishes a row at the step whose token completes it, matched
        on the emitted tokens only, the completing token kept, pad fill from the next step on; it needs an eos_token_id or a pad_token_id.
        return_logprobs reports the log-softmax of the constrained scores.  Both loops; the on-device loop serves 1024 bias + suppress
        entries, n <= 16 and 8 stop sequences of at most 16 ids (an explicit on_device=True beyond that raises, a default-derived one
        falls back to the host loop).  An id in both lists, twice in one, or outside [0, V) raises before any launch.
        prompt_lookup_num_tokens=K (1 .. 7; None or 0: off, the paths above untouched), max_matching_ngram_size=G (1 .. 4, default 2),
        lookup_ids (a long 1-D tensor or None): prompt-lookup speculative decoding, transformers' option of the same name.  Every
        decode step runs K + 1 positions of the one row -- the last token and a draft of up to K tokens copied from behind the earliest
        earlier occurrence of the sequence's last G' <= G ids -- and keeps the longest prefix of the draft that the model's own greedy
        picks confirm, plus the pick behind it: the tokens are the plain device loop's, up to near-ties between the step forms.  The
        searched history is `lookup_ids` (extra text that is not part of the prompt: for prompts given as embeddings, whose image span
        has no ids), then the prompt's ids, then everything emitted.  Selects the on-device loop; needs one row and do_sample=False, the
        sw or splitk decode form and the default decode mode; repetition_penalty, logit_bias, suppress_tokens, min_new_tokens,
        no_repeat_ngram_size, stop_sequences, return_logprobs, deterministic, num_return_sequences > 1 and on_device=False are refused
        by name.  `engine.last_spec_stats` = {steps, drafted, accepted, emitted} of the call (Qwen2Engine.spec_step).
        num_beams and penalty_alpha are refused."""
        lookup = dict(prompt_lookup_num_tokens=prompt_lookup_num_tokens, max_matching_ngram_size=max_matching_ngram_size,
                      lookup_ids=lookup_ids, on_device=on_device)
        call, n_ret = generate_call(lambda: self.config.vocab_size, do_sample, temperature, top_k, top_p, eos_token_id, pad_token_id, generator,
                                    deterministic, return_logprobs, kwargs, prompt_lookup=lookup)
        if call.spec is not None:
            check_spec_call(call, int((input_ids if input_embeddings is None else input_embeddings).shape[0]), self.llm.engine)
            on_device = True
        if n_ret > 1:
            input_ids = None if input_ids is None else input_ids.repeat_interleave(n_ret, dim=0)
            input_embeddings = None if input_embeddings is None else input_embeddings.repeat_interleave(n_ret, dim=0)
            attention_mask = None if attention_mask is None else attention_mask.repeat_interleave(n_ret, dim=0)
        if "max_length" in kwargs and kwargs["max_length"] is not None and input_ids is not None:
            max_new_tokens = int(kwargs["max_length"]) - input_ids.shape[1]
        eng = self.llm.engine
        prompt = self._generate_prompt(input_ids, input_embeddings, attention_mask)
        eng.last_decode_deterministic = call.deterministic
        eng.last_text_decode_on_device = self._text_on_device(on_device, call, prompt.rows, bool(use_cache), max_new_tokens)
        run = self._decode_text_on_device if eng.last_text_decode_on_device else self._run_text_host
        out, _, steps, logp = run(call, prompt, max_new_tokens)
        out = out[:, :steps]
        seqs = torch.cat([prompt.prompt_ids, out], dim=1) if input_embeddings is None else out
        return (seqs, logp[:, :steps]) if return_logprobs else seqs

    @torch.no_grad()
    def beam_search(self, input_ids=None, input_embeddings=None, attention_mask=None, max_new_tokens=20, num_beams=4,
                    num_return_sequences=1, length_penalty=1.0, early_stopping=False, eos_token_id=None, pad_token_id=None,
                    deterministic=None, return_scores=False, **kwargs):
        """Beam search with the rule of transformers' `generate(num_beams=B, do_sample=False)` (stated once, in include/unigen_hip.h:
        "Beam search of the text loop"; the bookkeeping is models/beam.py: BeamSearch).  Prompts as `generate` takes them: ids [G, L]
        or `input_embeddings` [G, L, H] with an optional 2-D [G, L] key-validity mask (left padding).  Every prompt row, with its mask
        row, is repeated num_beams times consecutively before the one prefill; a step is the head over the whole vocabulary,
        ops.beam_candidates (log-softmax of the bf16-rounded logits + running score, the K best per prompt), BeamSearch.step on the
        [G, K] candidates (the step's one host read), ops.beam_kv_reorder on the generated positions [L, len) of the cache -- the
        prompt part is the same in all beams of a prompt and never moves -- and the decode step on the chosen tokens.
        Returns each prompt's num_return_sequences <= num_beams best hypotheses, best first, padded behind their eos with
        pad_token_id (default: the first eos id): prompt + continuation [G * n, L + new] for ids, the continuation alone [G * n, new]
        for embeddings; with return_scores also sequence_scores fp32 [G * n] (sum of log-probabilities / length ** length_penalty).
        num_beams=1 is greedy search.  Refused before any launch: more than 32 rows (G * num_beams), num_beams > 8,
        num_return_sequences > num_beams, more than 7 eos ids, max_new_tokens < 1, and do_sample, repetition_penalty, logit_bias,
        suppress_tokens, min_new_tokens, no_repeat_ngram_size, stop_sequences, return_logprobs, num_beam_groups, on_device=True."""
        from unigen_hip.qwen2 import DecodeState, resolve_deterministic
        from .beam import BeamSearch
        src = input_ids if input_embeddings is None else input_embeddings
        if src is None:
            raise UniGenHipError("beam_search: give input_ids or input_embeddings")
        G, n_new = int(src.shape[0]), int(max_new_tokens)
        B, n_ret, eos, pad = beam_call(G, max_new_tokens, num_beams, num_return_sequences, length_penalty, early_stopping, eos_token_id,
                                       pad_token_id, kwargs)
        det = resolve_deterministic(deterministic)
        rep = lambda t: None if t is None else t.repeat_interleave(B, dim=0)
        eng, embed, V = self.llm.engine, self.llm.model.embed_tokens, self.config.vocab_size
        prompt = self._generate_prompt(rep(input_ids), rep(input_embeddings), rep(attention_mask))
        dev, R, L = prompt.embeds.device, prompt.rows, prompt.L
        eng.last_decode_deterministic, eng.last_text_decode_on_device = det, False
        st = DecodeState(eng.dims, R, L + n_new, dev, key_valid=prompt.key_valid, deterministic=det)
        hn = prompt.prefill(eng, st)
        eng.check_errors()
        search = BeamSearch(G, B, eos, pad, n_new, length_penalty, early_stopping, n_ret)
        spare = ops.beam_kv_spare(st, n_new) if B > 1 else None
        x = torch.empty((R, eng.dims.hidden_size), dtype=torch.float32, device=dev)
        scores = search.running_scores().to(dev)

        def pick(logits):
            return ops.beam_candidates(logits, scores, G, B, V, search.k)

        def emit(i, cand):
            parent, token, finished = search.step(*cand)
            if not finished and i + 1 < n_new:
                if i > 0 and B > 1:                                     # (step 0: nothing generated is in the cache yet)
                    ops.beam_kv_reorder(st, parent, L, spare)
                scores.copy_(search.running_scores())
            return token, finished

        text_token_loop(n_new, hn, pick, emit, head=lambda hn: eng.head_slice(hn, 0, V).float(),
                        embed=lambda ids: x.copy_(embed(ids)[:, 0]), step=lambda x: eng.decode_step(st, x))
        out, seq_scores = search.finalize()
        seqs = torch.cat([input_ids.to(dev).repeat_interleave(n_ret, dim=0), out], dim=1) if input_embeddings is None else out
        return (seqs, seq_scores) if return_scores else seqs

    # ------------------------------------------------------------------ text decoding for understanding
    @torch.no_grad()
    def mmu_prefix(self, idx=None, input_embeddings=None, attention_mask=None, capacity=None):
        """Prefill one prompt prefix (ids [1, P] or embeddings [1, P, H]) ONCE, for many continuations: the rating loop of CoT-V asks
        several questions about one image, and every row of such a call starts with the same [system | image] positions.
        attention_mask: the prefix's dense additive [1, 1, P, P] mask, any the reference builds (the mmu mask with its bidirectional
        image block, ...); None: causal.  The prefix is prefilled under it by the ordinary prefill; every later position sees the
        keys the mask's LAST row sees.  capacity: cache positions of the object (default: P rounded up to 128) -- what `extend` may
        grow it to; calls that take the prefix copy its rows into their own state and need no spare capacity.
        -> MmuPrefix, for `mmu_generate_batch(prefix=...)`, `mmu_generate(prefix=...)` and its own `extend`.  The caller owns it:
        `drop_decode_session()` and `train()` do not touch it, and it is only valid for the weights it was built with."""
        from unigen_hip.qwen2 import DecodeState
        if (idx is None) == (input_embeddings is None):
            raise UniGenHipError("mmu_prefix: give idx [1, P] or input_embeddings [1, P, H]")
        src = idx if input_embeddings is None else input_embeddings
        if src.shape[0] != 1 or src.shape[1] < 1:
            raise UniGenHipError(f"mmu_prefix: one row of at least one position, got {tuple(src.shape)}")
        P = int(src.shape[1])
        if attention_mask is not None and tuple(attention_mask.shape) != (1, 1, P, P):
            raise UniGenHipError(f"mmu_prefix: attention_mask must be the prefix's dense [1, 1, {P}, {P}] additive mask")
        cap = ops.round_up(P, 128) if capacity is None else int(capacity)
        if cap < P:
            raise UniGenHipError(f"mmu_prefix: capacity {cap} is below the prefix length {P}")
        eng = self.llm.engine
        prompt = (self.llm.model.embed_tokens(idx) if input_embeddings is None else input_embeddings).float()
        dev = prompt.device
        mb = eng.mask_bits(attention_mask, 1, P)
        key_valid = torch.ones((1, P), dtype=torch.bool, device=dev) if attention_mask is None else (attention_mask[:, 0, -1, :] == 0).to(dev)
        st = DecodeState(eng.dims, 1, cap, dev)
        eng.prefill(st, prompt, mask_bits=mb)
        eng.check_errors()
        return MmuPrefix(self, st, P, key_valid, None if idx is None else idx.to(dev).long())

    @torch.no_grad()
    def score(self, idx=None, input_embeddings=None, targets=None, prefix=None, tail_valid=None, average=False):
        """Log-probability of GIVEN continuations (lmms-eval's `loglikelihood`; P("yes") against P("no") of a rating; the answers
        of a multiple-choice question; DPO candidates): row r's context is idx[r] (ids [R, S]) or input_embeddings[r] ([R, S, H]),
        LEFT-padded to a common length with tail_valid [R, S] marking the real positions (None: all), and behind an optional
        `mmu_prefix` object shared by every row, as in `mmu_generate_batch(prefix=...)`; targets int64 [R, C] holds the
        continuations' ids, RIGHT-padded with -100.  One teacher-forced pass over [context | targets[:, :-1]] (pads fed as id 0:
        they sit behind every real position, causality hides them) through Qwen2Engine.prefill_onto, then ONE ug_head_score launch
        pair over the R * C positions that predict a target: the [R * C, vocab] logits are never formed.
        -> ScoreResult(logprob [R], is_greedy [R], token_logprobs [R, C]); every token's log-probability is log softmax of the
        bf16-rounded head logits at its label -- the number `generate(return_logprobs=True)` reports for a token it drew greedily.
        average=True: logprob is the mean over the row's real targets instead of the sum.  Any number of rows: beyond 32 they go
        through the backbone 32 at a time inside the call.  Leaves the prefix unchanged and keeps no session.  Wrong arguments
        (shapes, a row without a real target, a prefix of another model or device, target ids outside the vocabulary when
        `targets` is on the CPU) raise UniGenHipError before any launch.  On a model with a gen_projector image-code targets raise."""
        from unigen_hip.qwen2 import DecodeState
        eng = self.llm.engine
        codes_from = self.config.get("llm_vocab_size", None) if self._use_gen() else None
        R, S, C, tail_valid, real = check_score_call("score", eng, prefix, idx, input_embeddings, targets, tail_valid, codes_from)
        dev = eng.device
        ctx = (self.llm.model.embed_tokens(idx.to(dev)) if input_embeddings is None else input_embeddings.to(dev)).float()
        real = real.to(dev)
        labels = torch.where(real, targets.to(dev), torch.full_like(real, -100, dtype=torch.int64))
        seq = ctx
        if C > 1:
            fed = torch.where(real, labels, torch.zeros_like(labels))[:, :-1].contiguous()
            seq = torch.cat([ctx, self.llm.model.embed_tokens(fed).float()], dim=1)
        P, L = (0 if prefix is None else prefix.P), S + C - 1
        tv = torch.ones((R, S), dtype=torch.bool, device=dev) if tail_valid is None else tail_valid.to(dev)
        pre = torch.ones((R, 0), dtype=torch.bool, device=dev) if prefix is None else prefix.key_valid.to(dev).expand(R, P)
        key_valid = torch.cat([pre, tv, torch.ones((R, C - 1), dtype=torch.bool, device=dev)], dim=1)
        at = (S - 1) + torch.arange(C, device=dev)
        token_logprobs = torch.empty((R, C), dtype=torch.float32, device=dev)
        best = torch.empty((R, C), dtype=torch.int64, device=dev)
        for r0 in range(0, R, MMU_MAX_ROWS):
            n = min(MMU_MAX_ROWS, R - r0)
            st = DecodeState(eng.dims, n, P + L, dev, key_valid=key_valid[r0:r0 + n])
            hidden_at = (torch.arange(n, device=dev)[:, None] * L + at[None, :]).reshape(-1)
            if prefix is None:
                _, hn = eng.prefill_onto(st, seq[r0:r0 + n], 0, key_valid[r0:r0 + n], hidden_at=hidden_at)
            else:
                _, hn = _prefill_after_prefix(eng, st, prefix, seq[r0:r0 + n], key_valid[r0:r0 + n], hidden_at=hidden_at)
            logp, _, b = eng.score_rows(hn, labels[r0:r0 + n].reshape(-1))
            token_logprobs[r0:r0 + n] = logp.view(n, C)
            best[r0:r0 + n] = b.view(n, C)
        eng.check_errors()
        logprob = token_logprobs.sum(dim=1)
        if average:
            logprob = logprob / real.sum(dim=1).to(torch.float32)
        return ScoreResult(logprob, ((best == labels) | ~real).all(dim=1), token_logprobs)

    @torch.no_grad()
    def mmu_generate(self, idx=None, input_embeddings=None, attention_mask=None, max_new_tokens=100, temperature=1.0,
                     top_k=None, eot_token=None, use_cache=True, deterministic=None, on_device=None, use_graph=True, repetition_penalty=1.0,
                     return_logprobs=False, trace=None, prefix=None, logit_bias=None, suppress_tokens=None, min_new_tokens=None,
                     no_repeat_ngram_size=None, stop_sequences=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=None,
                     lookup_ids=None):
        """Greedy / top-k text continuation (reference models/unigen.py:523-581).  The reference re-runs the whole
        growing sequence every step and extends the additive mask by one row that copies the previous last row;
        here the prompt is prefilled once under its mask into the static KV cache and every new token is one decode
        step that attends to the keys the prompt's last row could see plus everything generated since (the same
        function of the inputs; `use_cache=False` keeps the step-by-step recomputation for comparison).  deterministic: ordered
        decode kernels for the cached form; None follows torch.are_deterministic_algorithms_enabled().
        on_device / use_graph: the token loop on the device, as in `generate` (temperature 0 is greedy; with temperature > 0 the draw is
        temperature -> top-k -> inverse CDF on uniforms drawn up front, so sampled tokens differ from the host loop's for the same
        seed).  Cached form only: an explicit True with use_cache=False raises.
        repetition_penalty: as in `generate`, cached form only (both loops); the prompt ids are `idx` at the keys the prompt's last row
        sees, nothing with an `input_embeddings` prompt.  The recompute form raises for a penalty other than 1.
        return_logprobs: returns (token list, fp32 1-D device tensor of the same length): every token's log-probability as in `generate`
        (temperature 0: the greedy form; temperature > 0: behind temperature and top-k).  Cached form only.
        trace: a list that receives every eager on-device step's raw fp32 head logits (use_graph=False).
        logit_bias, suppress_tokens, min_new_tokens, no_repeat_ngram_size, stop_sequences: as in `generate`, cached form only (both loops);
        min_new_tokens holds `eot_token` back, a stop sequence ends the list like `eot_token` does.  The recompute form raises for them.
        prefix: an `mmu_prefix` object; `idx` / `input_embeddings` are then only the continuation [1, S], which is causal (no
        attention_mask) and sees of the prefix what its mask's last row saw.  Cached form only; everything else as without.
        prompt_lookup_num_tokens, max_matching_ngram_size, lookup_ids: prompt-lookup speculative decoding as in `generate`, cached form
        only, with or without a prefix; needs temperature == 0 or top_k == 1.  The searched history is lookup_ids, then the ids the
        repetition penalty would count (the prefix's and `idx` at the keys the last row sees), then everything emitted -- with an
        `input_embeddings` prompt (an image span has no ids) lookup_ids is all there is to search at first, e.g. the generation prompt's
        tokens when an image is rated against it."""
        lookup = dict(prompt_lookup_num_tokens=prompt_lookup_num_tokens, max_matching_ngram_size=max_matching_ngram_size,
                      lookup_ids=lookup_ids, on_device=on_device)
        if prefix is not None:
            check_mmu_prefix_call("mmu_generate", self.llm.engine, prefix, idx, input_embeddings, attention_mask, None)
            if (idx if input_embeddings is None else input_embeddings).shape[0] != 1:
                raise UniGenHipError("mmu_generate: one row per call (mmu_generate_batch takes several)")
            if not use_cache:
                raise UniGenHipError("mmu_generate: a prefix needs the cached form (use_cache=True)")
        call = mmu_call("mmu_generate", lambda: self.config.vocab_size, temperature, top_k, eot_token, repetition_penalty=repetition_penalty,
                        deterministic=deterministic, return_logprobs=return_logprobs, use_graph=use_graph, trace=trace, logit_bias=logit_bias,
                        suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens, no_repeat_ngram_size=no_repeat_ngram_size,
                        stop_sequences=stop_sequences, prompt_lookup=lookup)
        if call.spec is not None:
            check_spec_call(call, int((idx if input_embeddings is None else input_embeddings).shape[0]), self.llm.engine)
            on_device = True
        eng = self.llm.engine
        eng.last_decode_deterministic = call.deterministic
        cached = prefix is not None or bool(use_cache and attention_mask is not None and attention_mask.shape[0] == 1)
        eng.last_text_decode_on_device = self._text_on_device(on_device, call, 1, cached, max_new_tokens)
        if cached:
            mask = None if prefix is not None else attention_mask.reshape(1, 1, attention_mask.shape[-1], attention_mask.shape[-1])
            tokens, _, steps, logp = self._mmu_decode(call, idx, input_embeddings, mask, max_new_tokens, eng.last_text_decode_on_device, prefix)
            # (one row: it ends at its `eot_token`, so every step counts)
            return (list(tokens[0, :steps]), logp[0, :steps].clone()) if return_logprobs else list(tokens[0, :steps])
        if call.constraints is not None or stop_sequences:
            raise UniGenHipError("mmu_generate: logit_bias / suppress_tokens / min_new_tokens / no_repeat_ngram_size / stop_sequences need "
                                 "the cached form (use_cache=True and a one-row mask); the recompute form does not apply them")
        if return_logprobs:
            raise UniGenHipError("mmu_generate: return_logprobs needs the cached form (use_cache=True and a one-row mask)")
        if call.penalty != 1.0:
            raise UniGenHipError("mmu_generate: repetition_penalty needs the cached form (use_cache=True and a one-row mask); the recompute "
                                 "form does not apply it")
        return self._mmu_generate_recompute(idx, input_embeddings, attention_mask, max_new_tokens, temperature, top_k, eot_token)

    @staticmethod
    def _process_next(last, temperature, top_k):
        """the scores `_choose_next` picks from: temperature, then top-k as -inf (temperature 0: greedy, the scores as they are)"""
        if temperature > 0:
            last = last / temperature
            if top_k is not None:
                v, _ = torch.topk(last, min(top_k, last.size(-1)))
                last[last < v[:, [-1]]] = -float('Inf')
        return last

    @staticmethod
    def _choose_next(scores, temperature):
        if temperature > 0:
            return torch.multinomial(torch.softmax(scores, dim=-1), num_samples=1)
        return torch.argmax(scores, dim=-1).reshape(-1, 1)

    @staticmethod
    def _pick_next(last, temperature, top_k):
        return UniGen._choose_next(UniGen._process_next(last, temperature, top_k), temperature)

    _stop_list = staticmethod(stop_list)

    def _text_on_device(self, on_device, call, rows, cached, max_new_tokens):
        """Whether this call (a TextCall) runs the on-device token loop.  An explicit bool wins over `self.text_decode_on_device`; the
        loop serves what the AR path's fused step serves (up to 32 rows, hidden size >= 256 and a multiple of 32, cached path) with up
        to 8 stop ids and constraints within ops.TEXT_MAX_BIAS / TEXT_MAX_NGRAM / TEXT_MAX_STOP_SEQS / TEXT_MAX_STOP_SEQ_LEN.  An
        explicit True on anything else raises with the reason; a default-derived True falls back to the host loop."""
        if not (self.text_decode_on_device if on_device is None else bool(on_device)):
            return False
        H = self.llm.engine.dims.hidden_size
        n_stop = len(call.stop)
        why = None
        if not cached:
            why = "the recompute form (use_cache=False, or several rows / no mask in mmu_generate) has no on-device loop"
        elif rows > ops.TEXT_MAX_ROWS:
            why = f"{rows} rows (at most {ops.TEXT_MAX_ROWS})"
        elif H < 256 or H % 32:
            why = f"hidden size {H} (at least 256 and a multiple of 32)"
        elif n_stop > ops.TEXT_MAX_STOP:
            why = f"{n_stop} stop ids (at most {ops.TEXT_MAX_STOP})"
        elif max_new_tokens < 1:
            why = f"max_new_tokens={max_new_tokens}"
        elif call.constraints is not None:
            c = call.constraints
            longest = max([len(q) for q in c["stop_seqs"]], default=0)
            if len(c["bias"]) > ops.TEXT_MAX_BIAS:
                why = f"{len(c['bias'])} logit_bias + suppress_tokens entries (at most {ops.TEXT_MAX_BIAS})"
            elif c["ngram"] > ops.TEXT_MAX_NGRAM:
                why = f"no_repeat_ngram_size={c['ngram']} (at most {ops.TEXT_MAX_NGRAM})"
            elif len(c["stop_seqs"]) > ops.TEXT_MAX_STOP_SEQS:
                why = f"{len(c['stop_seqs'])} stop sequences (at most {ops.TEXT_MAX_STOP_SEQS})"
            elif longest > ops.TEXT_MAX_STOP_SEQ_LEN:
                why = f"a stop sequence of {longest} ids (at most {ops.TEXT_MAX_STOP_SEQ_LEN})"
        if why is None:
            return True
        if on_device is None:
            return False
        raise UniGenHipError(f"{call.who}: on_device=True cannot serve this call: {why}")

    def _decode_text_on_device(self, call, prompt, max_new_tokens):
        """The token loop of `text_token_loop` + `emit_until_stop` for a TextCall and a TextPrompt with nothing but launches per token:
        prefill, token 0 eagerly from the prefill's hidden state (GEMV head + pick), then unigen_hip/qwen2.py: decode_loop (step 1
        eagerly, step 2 captured, replays from there).  The pick launch applies the stop rule on the device; when a row can finish the
        host reads `remaining` every 8 tokens and stops replaying at zero.  The result is cut at `steps_used` (the step at which the
        last row finished), else at max_new_tokens: rows that overshoot a poll interval emit pad ids / have their lengths set exactly
        as the host loop's rows, so the cut result is the host loop's.  No decode step follows the last token.
        The session (TextDecodeSession: Qwen2Engine.text_step's buffers + the graph) is kept across calls like the AR path's and reused
        when `key` below agrees -- every size and every constant of the call that is a kernel argument of the captured step or decides
        which launches it holds; `drop_decode_session()` and `train()` drop it, UNIGEN_AR_GRAPH_CACHE=0 turns the reuse off.  What the
        options launch: include/unigen_hip.h and TextDecodeSession.
        -> (tokens int64 [R, steps], lengths int64 [R], steps, log-probabilities fp32 [R, steps] or None)."""
        from unigen_hip.qwen2 import TextDecodeSession, decode_loop, put_session, take_session
        if call.spec is not None:
            return self._decode_text_spec(call, prompt, max_new_tokens)
        eng = self.llm.engine
        dev = eng.device
        R, L, key_valid, cons, det = prompt.rows, prompt.L, prompt.key_valid, call.constraints, call.deterministic
        n, V = int(max_new_tokens), self.config.vocab_size
        sampling = call.sampling
        if sampling is not None and sampling[1] >= V:
            sampling = (sampling[0], 0, sampling[2])
        if sampling is not None and not (sampling[0] > 0 and sampling[1] >= 0 and 0.0 < sampling[2] <= 1.0):
            raise UniGenHipError(f"on-device sampling needs temperature > 0, top_k >= 0 and 0 < top_p <= 1 (got {sampling})")
        cap, width = ops.round_up(L + n, 128), ops.round_up(n, 64)
        pad = None if call.pad_token_id is None or not call.stops else int(call.pad_token_id)
        key = (R, cap, width, V, eng.decode_form(R, det), det, sampling, call.penalty, tuple(call.stop), pad, key_valid is None,
               str(dev)) + eng.storage_key(cap)
        if call.return_logprobs:
            key += ("logprobs",)
        if cons is not None:
            key += ("constraints", tuple(cons["bias"]), cons["min_new"], cons["ngram"], tuple(cons["stop_seqs"]))
        sess = take_session(eng, "_text_session", key, call.use_graph)
        if sess is None:
            sess = TextDecodeSession(eng, R, cap, width, V, deterministic=det, sampling=sampling, stop_ids=call.stop, pad_id=pad, key_valid=key_valid,
                                     repetition_penalty=call.penalty, logprobs=call.return_logprobs, constraints=cons)
            sess.key = key
            sess.begin(n, prompt_ids=prompt.prompt_ids, prompt_valid=prompt.prompt_valid)
        else:
            sess.begin(n, key_valid, L, prompt_ids=prompt.prompt_ids, prompt_valid=prompt.prompt_valid)
        if sampling is not None:
            u_dev = dev if call.generator is None else call.generator.device
            sess.uniforms[:n].copy_(torch.rand((n, R), device=u_dev, generator=call.generator))
        hn = prompt.prefill(eng, sess.st)
        eng.check_errors()
        eng.text_first_token(sess, hn, call.trace)
        done = (lambda emitted: emitted % 8 == 0 and int(sess.state[1]) == 0) if call.stops else None   # (the one host read per 8 tokens)
        if decode_loop(sess, lambda: eng.text_step(sess, call.trace), range(1, n), call.use_graph, stop=done):
            eng.text_graph_captures = getattr(eng, "text_graph_captures", 0) + 1
        used = int(sess.state[2]) if call.stops else 0
        steps = used if used > 0 else n
        eng.last_decode_graph = sess.graph is not None
        tokens, lengths = sess.out_tokens[:, :steps].long(), sess.lengths.long()       # (copies: the next call overwrites the session's)
        logp = sess.logp[:, :steps].clone() if call.return_logprobs else None
        put_session(eng, "_text_session", sess, call.use_graph)
        return tokens, lengths, steps, logp

    def _decode_text_spec(self, call, prompt, max_new_tokens):
        """_decode_text_on_device for a call with prompt-lookup speculative decoding (call.spec = (K, G, lookup ids)): prefill, token 0
        eagerly from the prefill's hidden state (Qwen2Engine.spec_first_token), then decode_loop over verify steps of K + 1 rows
        (Qwen2Engine.spec_step: step 1 eagerly, step 2 captured, replays from there).  A step emits between one and K + 1 tokens and the
        device cuts the emission at the stop id and at max_new_tokens, so the host only needs to know when to stop launching: it reads
        `done` every 4 steps.  The session (SpecDecodeSession) is kept on the engine like the plain loop's, under a key of every size
        and constant the captured step holds.  Sets eng.last_spec_stats.  -> _decode_text_on_device's tuple."""
        from unigen_hip.qwen2 import SpecDecodeSession, decode_loop, put_session, take_session
        eng = self.llm.engine
        dev = eng.device
        (K, G, lookup), L, key_valid = call.spec, prompt.L, prompt.key_valid
        n, V = int(max_new_tokens), self.config.vocab_size
        history = [torch.zeros(0, dtype=torch.long, device=dev) if lookup is None else lookup.to(dev)]
        if prompt.prompt_ids is not None:
            ids = prompt.prompt_ids[0].to(dev).long()
            ok = (ids >= 0) & (ids < V)
            if prompt.prompt_valid is not None:
                ok &= prompt.prompt_valid[0].to(dev) != 0
            history.append(ids[ok])
        history = torch.cat(history).int()
        cap = ops.round_up(L + n + K, 128)
        hist_cap = ops.round_up(int(history.numel()) + n, 256)
        key = (cap, n, V, eng.spec_form(K + 1), K, G, hist_cap, tuple(call.stop), key_valid is None, str(dev)) + eng.storage_key(cap)
        sess = take_session(eng, "_spec_session", key, call.use_graph)
        if sess is None:
            sess = SpecDecodeSession(eng, cap, n, V, K, G, hist_cap, stop_ids=call.stop, key_valid=key_valid)
            sess.key = key
            sess.begin(history)
        else:
            sess.begin(history, key_valid, L)
        hn = prompt.prefill(eng, sess.st)
        eng.check_errors()
        eng.spec_first_token(sess, hn)
        done = lambda i: i % 4 == 1 and int(sess.state[ops.SPEC_DONE]) != 0        # (asked before step i: one host read per 4 steps)
        if decode_loop(sess, lambda: eng.spec_step(sess), range(1, n), call.use_graph, stop=done):
            eng.text_graph_captures = getattr(eng, "text_graph_captures", 0) + 1
        eng.last_spec_stats = sess.stats()
        steps = eng.last_spec_stats["emitted"]
        eng.last_decode_graph = sess.graph is not None
        tokens, lengths = sess.out_tokens[None, :steps].long(), sess.lengths.long()    # (copies: the next call overwrites the session's)
        put_session(eng, "_spec_session", sess, call.use_graph)
        return tokens, lengths, steps, None

    def _decode_text(self, st, hn, max_new_tokens, pick, emit):
        """text_token_loop on this model's engine from a prefilled state: vocabulary logits, embedding table, decode_step."""
        eng, embed, V = self.llm.engine, self.llm.model.embed_tokens, self.config.vocab_size
        x = torch.empty((st.rows, eng.dims.hidden_size), dtype=torch.float32, device=hn.device)
        return text_token_loop(max_new_tokens, hn, pick, emit, head=lambda hn: eng.head_slice(hn, 0, V).float(),
                               embed=lambda ids: x.copy_(embed(ids)[:, 0]),
                               step=lambda x: eng.decode_step(st, x))            # (also advances the cache position)

    def _run_text_host(self, call, prompt, max_new_tokens, lengths=False):
        """The host token loop for a TextCall and a TextPrompt: prefill, then text_token_loop with text_pick_emit's pick / emit.
        -> (tokens long [R, max_new_tokens]: zeros, or the call's pad id, behind the last step taken; with `lengths` the rows' lengths
        cut after their stop [R], else None; the number of steps taken; the tokens' log-probabilities fp32 [R, max_new_tokens] (0.0
        behind a row's stop and behind the last step taken) or None)."""
        from unigen_hip.qwen2 import DecodeState
        eng = self.llm.engine
        dev, R = prompt.embeds.device, prompt.rows
        st = DecodeState(eng.dims, R, prompt.L + max_new_tokens, dev, key_valid=prompt.key_valid, deterministic=call.deterministic)
        hn = prompt.prefill(eng, st)
        if prompt.mask_bits is None:               # (under a dense mask the flags were read where it was compressed: _dense_prompt)
            eng.check_errors()
        tokens = torch.full((R, max_new_tokens), int(call.pad_token_id or 0), dtype=torch.long, device=dev)
        lengths = torch.full((R,), max_new_tokens, dtype=torch.long, device=dev) if lengths else None
        logp = torch.zeros((R, max_new_tokens), dtype=torch.float32, device=dev) if call.return_logprobs else None
        pick, emit = text_pick_emit(call, tokens, self.config.vocab_size, logp, lengths, prompt.prompt_ids, prompt.prompt_valid)
        return tokens, lengths, self._decode_text(st, hn, max_new_tokens, pick, emit), logp

    def _generate_prompt(self, input_ids, input_embeddings, attention_mask):
        """`generate`'s prompt: ids [R, L] or embeddings [R, L, H] under a 2-D [R, L] key-validity mask (None: all real)"""
        dev = self.llm.engine.device
        embeds = (self.llm.model.embed_tokens(input_ids.to(dev)) if input_embeddings is None else input_embeddings.to(dev)).float()
        key_valid = None
        if attention_mask is not None:
            if attention_mask.dim() != 2:
                raise UniGenHipError("generate expects a 2-D [rows, L] attention mask (1 = real token)")
            key_valid = attention_mask.to(dev) != 0
        return TextPrompt(embeds, int(embeds.shape[1]), key_valid, None, None if input_embeddings is not None else input_ids.to(dev), key_valid)

    def _dense_prompt(self, idx, input_embeddings, attention_mask):
        """the mmu entry points' prompt without a prefix: R left-padded rows under their dense additive [R, 1, L, L] masks; the keys
        every later position sees, and the ids that count, are those of the mask's last row"""
        eng = self.llm.engine
        embeds = (self.llm.model.embed_tokens(idx) if input_embeddings is None else input_embeddings).float()
        R, L = int(embeds.shape[0]), int(embeds.shape[1])
        mb = eng.mask_bits(attention_mask, R, L)
        eng.check_errors()
        key_valid = attention_mask[:, 0, -1, :] == 0
        return TextPrompt(embeds, L, key_valid, mb, idx if input_embeddings is None else None, key_valid)

    def _prefix_prompt(self, prefix, idx, input_embeddings, tail_valid):
        """the mmu entry points' prompt behind a prefix (already checked: check_mmu_prefix_call): the rows' tails [R, S], causal and
        left-padded where tail_valid [R, S] is False.  Key validity = the prefix's, then tail_valid; the ids that count = the prefix's
        (if it has any) and the tails' (if given as ids), zero-filled and marked invalid where one side came as embeddings."""
        embeds = (self.llm.model.embed_tokens(idx) if input_embeddings is None else input_embeddings).float()
        dev = embeds.device
        R, S, P = int(embeds.shape[0]), int(embeds.shape[1]), prefix.P
        tv = torch.ones((R, S), dtype=torch.bool, device=dev) if tail_valid is None else tail_valid.to(dev)
        key_valid = torch.cat([prefix.key_valid.to(dev).expand(R, P), tv], dim=1)
        prompt_ids = prompt_valid = None
        if prefix.ids is not None or input_embeddings is None:
            nothing = torch.zeros((R, 1), dtype=torch.long, device=dev)
            prompt_ids = torch.cat([(nothing if prefix.ids is None else prefix.ids.to(dev)).expand(R, P),
                                    idx.to(dev).long() if input_embeddings is None else nothing.expand(R, S)], dim=1)
            prompt_valid = key_valid.clone()
            if prefix.ids is None:
                prompt_valid[:, :P] = False
            if input_embeddings is not None:
                prompt_valid[:, P:] = False
        return TextPrompt(embeds, P + S, key_valid, None, prompt_ids, prompt_valid, prefix)

    def _mmu_decode(self, call, idx, input_embeddings, attention_mask, max_new_tokens, on_device, prefix=None, tail_valid=None):
        """The cached form of the mmu entry points: the prompt (behind `prefix`, or under its dense masks), then one of the two loops
        -> _run_text_host's tuple; the on-device loop's result is padded to the same max_new_tokens width."""
        prompt = self._dense_prompt(idx, input_embeddings, attention_mask) if prefix is None \
            else self._prefix_prompt(prefix, idx, input_embeddings, tail_valid)
        if not on_device:
            return self._run_text_host(call, prompt, max_new_tokens, lengths=True)
        tokens, lengths, steps, logp = self._decode_text_on_device(call, prompt, max_new_tokens)
        if steps < max_new_tokens:
            tokens = torch.cat([tokens, tokens.new_zeros((prompt.rows, max_new_tokens - steps))], dim=1)
            if logp is not None:
                logp = torch.cat([logp, logp.new_zeros((prompt.rows, max_new_tokens - steps))], dim=1)
        return tokens, lengths, steps, logp

    @torch.no_grad()
    def mmu_generate_batch(self, idx=None, input_embeddings=None, attention_mask=None, max_new_tokens=100, temperature=0.0,
                           top_k=None, eot_token=None, deterministic=None, on_device=None, use_graph=True, repetition_penalty=1.0, trace=None,
                           return_logprobs=False, prefix=None, tail_valid=None, logit_bias=None, suppress_tokens=None, min_new_tokens=None,
                           no_repeat_ngram_size=None, stop_sequences=None):
        """`mmu_generate` for up to 32 prompts at once -- the rating loop of CoT-V (reference
        evaluation/inference_unigen_cot.py:308-415 calls mmu_generate once per (image, question) pair; every decode
        step streams the whole backbone whatever the row count, so R pairs cost about one).  Rows are LEFT-padded to a
        common length L: idx [R, L] (or input_embeddings [R, L, H]) and the rows' dense additive masks [R, 1, L, L] with
        the pad columns blocked (the reference's mask builders do that for left-padded rows).  Each row follows the
        procedure of `mmu_generate`: prefill under its mask, then one decode step per token attending to the keys its
        last prompt row could see plus everything generated since.  Returns R lists of tokens, each cut after its
        `eot_token`.  deterministic: ordered decode kernels; None follows torch.are_deterministic_algorithms_enabled().
        on_device / use_graph: the token loop on the device, as in `mmu_generate`.  repetition_penalty: as in `mmu_generate`, both
        loops.  trace: a list that receives every eager on-device step's raw fp32 head logits (use_graph=False).
        return_logprobs: returns (the token lists, a list of fp32 1-D device tensors, row r's cut at its length): every token's
        log-probability as in `mmu_generate`.
        logit_bias, suppress_tokens, min_new_tokens, no_repeat_ngram_size, stop_sequences: as in `mmu_generate`, both loops; a row's list is
        cut behind the token that completes a stop sequence.
        prefix: an `mmu_prefix` object shared by every row -- one image, R questions: the image is prefilled once, not R times.
        `idx` / `input_embeddings` are then only the rows' tails [R, S], causal behind the prefix (no attention_mask: a dense one
        raises) and seeing of the prefix what its mask's last row saw.  tail_valid [R, S] (bool, None: all) marks the real tokens of
        tails LEFT-padded to the longest one, so every row's next position is P + S; pads count as positions, as the left pads of the
        rows do without a prefix.  The repetition penalty's prompt ids are the tail ids and, if the prefix was given as ids, those.
        The call copies the prefix's keys / values into its own state and leaves the object unchanged.  Wrong arguments (a prefix of
        another model or device, more than 32 rows, a tail position that is a pad in every row) raise UniGenHipError before any
        launch."""
        if prefix is not None:
            R, _, tail_valid = check_mmu_prefix_call("mmu_generate_batch", self.llm.engine, prefix, idx, input_embeddings, attention_mask,
                                                     tail_valid)
        elif tail_valid is not None:
            raise UniGenHipError("mmu_generate_batch: tail_valid belongs to a call with a prefix")
        call = mmu_call("mmu_generate_batch", lambda: self.config.vocab_size, temperature, top_k, eot_token, repetition_penalty=repetition_penalty,
                        deterministic=deterministic, return_logprobs=return_logprobs, use_graph=use_graph, trace=trace, logit_bias=logit_bias,
                        suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens, no_repeat_ngram_size=no_repeat_ngram_size,
                        stop_sequences=stop_sequences)
        eng = self.llm.engine
        eng.last_decode_deterministic = call.deterministic
        if prefix is None:
            R, L = (idx if input_embeddings is None else input_embeddings).shape[:2]
            if R > 32:
                raise ValueError("mmu_generate_batch: at most 32 rows per call")
            if attention_mask is None or tuple(attention_mask.shape) != (R, 1, L, L):
                raise ValueError("mmu_generate_batch: attention_mask must be the rows' dense [R, 1, L, L] additive masks")
        eng.last_text_decode_on_device = self._text_on_device(on_device, call, R, True, max_new_tokens)
        tokens, lengths, _, logp = self._mmu_decode(call, idx, input_embeddings, attention_mask, max_new_tokens, eng.last_text_decode_on_device,
                                                    prefix, tail_valid)
        tokens, lengths = tokens.cpu(), lengths.cpu()
        lists = [list(tokens[r, :int(lengths[r])]) for r in range(R)]
        if return_logprobs:
            return lists, [logp[r, :int(lengths[r])].clone() for r in range(R)]
        return lists

    def _mmu_generate_recompute(self, idx, input_embeddings, attention_mask, max_new_tokens, temperature, top_k, eot_token):
        device = idx.device if idx is not None else input_embeddings.device
        result = []
        neg = torch.finfo(torch.bfloat16).min
        for _ in range(max_new_tokens):
            logits = self(idx, input_embeddings=input_embeddings, attention_mask=attention_mask)
            last = logits[:, -1, :].float()
            L = attention_mask.shape[-1]
            m = attention_mask.reshape(L, L)
            grown = torch.full((L + 1, L + 1), float(neg), device=m.device, dtype=m.dtype)
            grown[:L, :L] = m
            grown[L, :L] = m[-1]
            grown[L, L] = 0
            attention_mask = grown[None, None]
            idx_next = self._pick_next(last, temperature, top_k)
            result.append(idx_next[0][0])
            if self.config.w_und_encoder:
                input_embeddings = torch.cat([input_embeddings, self.llm.model.embed_tokens(idx_next)], dim=1)
            else:
                idx = torch.cat((idx, idx_next), dim=1)
            if eot_token is not None and idx_next.cpu() == eot_token:
                break
        return result


def _note_ddp_wrapper(parent, name, sub):
    """Global module-registration hook: `DistributedDataParallel.__init__` does `self.module = module` (reference:
    accelerator.prepare, training/train.py:492).  The weak reference dies with the wrapper, so a model that is unwrapped
    again goes back to averaging its ordinary parameters itself."""
    if isinstance(sub, UniGen) and isinstance(parent, torch.nn.parallel.DistributedDataParallel):
        sub.__dict__["_ddp_wrapper"] = weakref.ref(parent)
    return None


torch.nn.modules.module.register_module_module_registration_hook(_note_ddp_wrapper)
