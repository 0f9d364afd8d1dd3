"""Restatements of the repetition penalty (include/unigen_hip.h: "THE RULE", ug_text_seen_mark, ug_text_penalize), beside
text_pick_ref.py.  CPU only, numpy for the arithmetic (IEEE fp32 products and quotients, round to nearest):

  host_rule            the host loop's rule: fp32, on the logits as they are;
  transformers_rule    RepetitionPenaltyLogitsProcessor's gather / where / scatter, literally, one row at a time;
  device_rule          the device loop's rule: s = bf16round(logit), fp32 product / quotient, unseen entries untouched;
  Bitmap               the seen bitmap [R][W] of the kernels: mark (prompt ids under a validity mask), add (an emitted token), and
                       penalize = add + device_rule on the bits below V;
  first_argmax         lowest index attaining the maximum of the bf16-rounded row (ug_text_pick's rule)."""
import numpy as np
import torch


def bf16round(x):
    """fp32 tensor -> the fp32 values of its bf16 rounding (round to nearest even, NaN stays NaN)"""
    return x.float().bfloat16().float()


def host_rule(logits, seen, p):
    """logits fp32 [R, V], seen bool [R, V] -> processed copy: s * p if s < 0 else s / p at the seen entries"""
    s = logits.float().numpy()
    p = np.float32(p)
    with np.errstate(all="ignore"):
        out = np.where(seen.numpy(), np.where(s < 0, s * p, s / p), s)
    return torch.from_numpy(out.astype(np.float32))


def transformers_rule(input_ids, scores, p):
    """transformers.RepetitionPenaltyLogitsProcessor.__call__ on one batch whose rows all have len(input_ids[r]) real ids:
    score = gather(scores, 1, input_ids); score = where(score < 0, score * p, score / p); scores.scatter(1, input_ids, score)"""
    score = torch.gather(scores, 1, input_ids)
    score = torch.where(score < 0, score * p, score / p)
    return scores.scatter(1, input_ids, score)


def device_rule(logits, seen, p):
    """logits fp32 [R, n >= V], seen bool [R, V] -> copy with the seen entries replaced by the penalised bf16-rounded value; every other
    entry (unseen ids, the columns behind V) keeps its bits"""
    V = seen.shape[1]
    out = logits.clone()
    s = bf16round(logits[:, :V]).numpy()
    p = np.float32(p)
    with np.errstate(all="ignore"):
        proc = np.where(s < 0, s * p, s / p).astype(np.float32)
    out[:, :V] = torch.where(seen, torch.from_numpy(proc), logits[:, :V])
    return out


class Bitmap:
    """words int32 [R, W], W = ceil(V / 32): bit (e & 31) of word (e >> 5) of row r = id e is in row r's sequence so far"""

    def __init__(self, rows, V, words=None):
        self.R, self.V, self.W = rows, V, (V + 31) // 32
        self.words = np.zeros((rows, self.W), dtype=np.uint32) if words is None else words.contiguous().numpy().view(np.uint32).reshape(rows, self.W).copy()

    def _set(self, r, e):
        self.words[r, e >> 5] |= np.uint32(1 << (e & 31))

    def mark(self, ids, valid=None):
        """prompt ids [R, L] at the positions valid [R, L] marks real (None: all); ids outside [0, V) are ignored"""
        for r in range(self.R):
            for l, e in enumerate(ids[r].tolist()):
                if (valid is None or bool(valid[r, l])) and 0 <= e < self.V:
                    self._set(r, e)
        return self

    def add(self, tok):
        """the tokens [R] one step emitted"""
        for r, e in enumerate([int(t) for t in tok]):
            if 0 <= e < self.V:
                self._set(r, e)
        return self

    def seen(self):
        """bool [R, V]: the bits below V (bits at or above V in the last word are never acted on)"""
        bits = (self.words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
        return torch.from_numpy(bits.reshape(self.R, self.W * 32)[:, :self.V].astype(bool))

    def tensor(self):
        return torch.from_numpy(self.words.view(np.int32).copy())

    def penalize(self, logits, p, tok=None):
        """ug_text_penalize: the previous step's tokens join the bitmap, then the device rule on the seen entries"""
        if tok is not None:
            self.add(tok)
        return device_rule(logits, self.seen(), p)


def first_argmax(row):
    """lowest index attaining the maximum of the bf16-rounded entries, spelled out"""
    b = bf16round(row)
    idx = torch.arange(b.shape[-1]).expand_as(b)
    return torch.where(b == b.max(-1, keepdim=True).values, idx, b.shape[-1]).min(-1).values


def same_bits(a, b):
    """fp32 tensors equal bit for bit (-0.0 is not 0.0, a NaN equals the same NaN)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
