"""Restatements of the text loops' constraints (include/unigen_hip.h: "Constraints of the text loops", ug_text_constrain,
ug_text_stop_seq), beside repetition_penalty_ref.py.  CPU only, plain Python: loops over lists, one row at a time; numpy only for the
IEEE fp32 sum.

  bf16round            one fp32 number rounded to bf16 (nearest even), from its bits;
  ngram_bans           NoRepeatNGramLogitsProcessor on one history, spelled out;
  host_rule            the host loop's rule on one row: bias, then the -inf stores (suppress, held-back stop ids, n-gram bans);
  device_rule          ug_text_constrain on one row of the logits buffer: the bf16 rounding at the biased entries, ids outside
                       [0, V) compared and never used as an index, nothing else touched;
  tail_matches         the host loop's stop-sequence matcher on one row's emitted tokens;
  stop_seq_step        ug_text_stop_seq on the state block, the token buffer and the lengths, as lists."""
import struct

import numpy as np

NINF = float("-inf")


def bf16round(x):
    """fp32 -> the fp32 value of its bf16 rounding (round to nearest even; NaN stays NaN, an infinity itself)"""
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    if (bits & 0x7fffffff) > 0x7f800000:
        return x
    bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def add_f32(a, b):
    with np.errstate(all="ignore"):
        return float(np.float32(a) + np.float32(b))


def ngram_bans(history, n):
    """the ids that would complete an n-gram `history` already holds; nothing while it is shorter than n - 1"""
    T = len(history)
    bans = []
    if n < 1 or T < n - 1:
        return bans
    for i in range(0, T - n + 1):
        same = True
        for k in range(n - 1):
            if history[i + k] != history[T - n + 1 + k]:
                same = False
        if same:
            bans.append(history[i + n - 1])
    return bans


def host_rule(row, bias, banned, history, n):
    """row: list of fp32 scores [V]; bias: [(id, b)] with b = -inf for a suppressed id; banned: the stop ids min_new_tokens holds back
    at this step (empty otherwise); history: the row's ids so far -> the processed row (a new list)"""
    out = list(row)
    for e, b in bias:
        out[e] = NINF if b == NINF else add_f32(out[e], b)
    for e in banned:
        out[e] = NINF
    for e in ngram_bans(history, n):
        if 0 <= e < len(out):
            out[e] = NINF
    return out


def device_rule(row, V, bias, min_new, stop_ids, n, prompt_hist, emitted, step):
    """row: numpy fp32 [ld >= V], changed IN PLACE at the named entries only; prompt_hist: the prompt part of the history; emitted: the
    row of the token buffer (entries 0 .. step - 1 count).  Phase 1 (bias on the bf16-rounded score), then phase 2 (the -inf stores)."""
    for e, b in bias:
        if 0 <= e < V:
            row[e] = NINF if b == NINF else add_f32(bf16round(float(row[e])), b)
    if step < min_new:
        for e in stop_ids:
            if 0 <= e < V:
                row[e] = NINF
    if n > 0:
        for e in ngram_bans(list(prompt_hist) + [int(t) for t in emitted[:step]], n):
            if 0 <= e < V:
                row[e] = NINF
    return row


def tail_matches(emitted, sequences):
    """whether the list `emitted` ends with one of `sequences`"""
    for s in sequences:
        m = len(s)
        if 0 < m <= len(emitted):
            same = True
            for k in range(m):
                if emitted[len(emitted) - m + k] != s[k]:
                    same = False
            if same:
                return True
    return False


def stop_seq_step(state, out_tokens, lengths, sequences, R):
    """state: list [step, remaining, steps_used, ticket, done[0..]] AFTER the pick of a step (state[0] = step + 1); out_tokens: R lists;
    lengths: list or None.  Changes state / lengths in place as the kernel does."""
    step = state[0] - 1
    if step < 0 or step >= len(out_tokens[0]):
        return
    for r in range(R):
        if state[4 + r]:
            continue
        for s in sequences:
            m = len(s)
            if m > step + 1:
                continue
            if out_tokens[r][step - m + 1:step + 1] == list(s):
                if lengths is not None:
                    lengths[r] = step + 1
                state[4 + r] = 1
                state[1] -= 1
                if state[1] == 0:
                    state[2] = step + 1
                break
