"""Restatement of ug_head_score (include/unigen_hip.h) on the CPU, for tests/test_head_score_cpu.py and tests/test_head_score_gpu.py.

  s[e]       = bf16round(fp64 sum over k of x[r][k] * W[e][k]), e < V      (the bf16 operands widened exactly; fp64 carries a
               1536-term sum of bf16 products to about 2^-45 relative, so the only rounding that counts is the one to bf16)
  lse        = max s + log(sum exp(s - max s))                              in fp64
  best       = the lowest index attaining max s (torch.argmax's rule)
  best_logit = max s
  logp       = s[label] - lse;  0.0 where the label is ignore_index or outside [0, V)

Beside the results it returns, for the label and for the maximum, the UNROUNDED fp64 sum and sum |x_k W_ek|: what the GPU test's
exemption for a logit that sits on a bf16 rounding midpoint is stated in."""
import types

import torch


def bf16_round64(t):
    """fp64 -> the nearest bf16 (8 significant bits, ties to even), returned as fp64.  One rounding: fp64 -> fp32 -> bf16 would round
    twice.  Normal range only (logits are nowhere near bf16's subnormals or its overflow)."""
    mant, exp = torch.frexp(t)                                # t = mant * 2^exp, |mant| in [0.5, 1)
    return torch.ldexp(torch.round(mant * 256.0), exp - 8)    # torch.round: half to even


def bf16_steps(a, b):
    """how many bf16 values lie between two bf16-representable tensors (any float dtype) -> int64; 0 = equal"""
    def ordered(t):
        i = t.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)       # sign-magnitude -> monotone integers (+0 and -0 both 0)
    return (ordered(a) - ordered(b)).abs()


def head_score_ref(x, W, labels, ignore_index=-100, chunk=16384):
    """x bf16 [R, K], W bf16 [V, K] (exactly V rows), labels int64 [R] -> namespace of fp64 / int64 tensors [R]:
    logp, lse, best, best_logit, label_logit (0 where ignored), valid, and label_raw / label_abs / best_raw / best_abs."""
    assert x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and labels.dtype == torch.int64
    R, V = x.shape[0], W.shape[0]
    xd = x.double()
    m = torch.full((R,), float("-inf"), dtype=torch.float64)
    best = torch.zeros((R,), dtype=torch.int64)
    best_raw = torch.zeros((R,), dtype=torch.float64)
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    rows = torch.arange(R)
    tiles = []
    for v0 in range(0, V, chunk):
        raw = xd @ W[v0:v0 + chunk].double().t()
        s = bf16_round64(raw)
        cm, ci = s.max(dim=1)                                 # torch.max returns the first index of the maximum on the CPU ...
        ci = (s == cm[:, None]).to(torch.int8).argmax(dim=1)  # ... restated so that the rule does not rest on it
        take = cm > m                                         # chunks ascend: strict keeps the lowest index
        best = torch.where(take, ci + v0, best)
        best_raw = torch.where(take, raw[rows, ci], best_raw)
        m = torch.where(take, cm, m)
        tiles.append(s)
    total = torch.zeros((R,), dtype=torch.float64)
    for s in tiles:
        total += torch.exp(s - m[:, None]).sum(dim=1)
    lse = m + torch.log(total)
    wl = W[lab].double()
    label_raw = (xd * wl).sum(dim=1)
    label_logit = bf16_round64(label_raw)
    return types.SimpleNamespace(
        logp=torch.where(valid, label_logit - lse, torch.zeros_like(lse)), lse=lse, best=best, best_logit=m, valid=valid,
        label_logit=torch.where(valid, label_logit, torch.zeros_like(lse)), label_raw=label_raw, label_abs=(xd * wl).abs().sum(dim=1),
        best_raw=best_raw, best_abs=(xd * W[best].double()).abs().sum(dim=1))
