"""Float64 restatement of the truncated-sampling rule (include/unigen_hip.h: ug_ar_sample_filtered), written from its definition --
one row at a time over the row's DISTINCT values, no sort-and-shift -- for tests/test_truncate_cpu.py and the GPU sampler tests.

Per row v: mx = max v, ex = exp(v - mx); the kept set is {v >= tau}, tau = max(tau_k, tau_p, tau_m)."""
import math

import torch

NEG = float("-inf")
D = 1e-5          # ten times the ~1e-6 relative error of an fp32 sum of 8 192 terms, plus expf


def tau_top_k(v, k):
    """the k-th largest value, duplicates counted (-inf when off)"""
    if not 0 < k < v.numel():
        return NEG
    return float(torch.sort(v, descending=True).values[k - 1])


def tau_top_p(v, p, tau_k=NEG):
    """the smallest value of S_k = {v >= tau_k} whose mass of strictly greater values of S_k is <= p * Z (-inf when off)"""
    if p >= 1.0:
        return NEG
    s = v[v >= tau_k]
    ex = torch.exp(s - v.max())
    vals, inv = torch.unique(s, return_inverse=True)                 # ascending distinct values
    mass = torch.zeros_like(vals).index_add_(0, inv, ex)
    ge = mass.flip(0).cumsum(0).flip(0)                              # mass of the values >= each distinct value
    ok = (ge - mass) <= p * ex.sum()
    return float(vals[ok].min())


def tau_min_p(v, min_p, shift=0.0):
    """the smallest value >= max + log(min_p) + shift (-inf when off)"""
    if min_p <= 0.0:
        return NEG
    return float(v[v >= float(v.max()) + math.log(min_p) + shift].min())


def tau(v, top_k=0, top_p=1.0, min_p=0.0):
    """the rule's threshold for one float64 row"""
    tk = tau_top_k(v, top_k)
    return max(tk, tau_top_p(v, top_p, tk), tau_min_p(v, min_p))


def tau_bracket(v, top_k=0, top_p=1.0, min_p=0.0, d=D):
    """(low, high) ends between which a threshold found in fp32 must lie: top-k exact, top-p at top_p + d and top_p - d, min-p at
    log(min_p) - d and + d; the ends of the three filters are combined by max"""
    tk = tau_top_k(v, top_k)
    lo = max(tk, tau_top_p(v, top_p + d, tk) if top_p < 1.0 else NEG, tau_min_p(v, min_p, -d))
    hi = max(tk, tau_top_p(v, top_p - d, tk) if top_p < 1.0 else NEG, tau_min_p(v, min_p, +d))
    return lo, hi


def draw_ok(v, t, token, u, d=D):
    """is `token` a legitimate inverse-CDF draw on the uniform u over {v >= t} (index order, dropped entries count 0)?  It must be
    kept, and cdf[g] - ex[g] - d*T <= u*T < cdf[g] + d*T"""
    keep = v >= t
    if not bool(keep[token]):
        return False
    ex = torch.where(keep, torch.exp(v - v.max()), torch.zeros_like(v))
    cdf = ex.cumsum(0)
    T = float(cdf[-1])
    g = int(token)
    return float(cdf[g] - ex[g]) - d * T <= float(u) * T < float(cdf[g]) + d * T


def mixed_logits(acc, bsz, scale, temperature):
    """the sampler's fp32 mixed logit from a raw [2*bsz, V] head accumulator: bf16-rounded rows, CFG mix, times fp32(1/temperature)"""
    lf = acc.float().to(torch.bfloat16).float()
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    return (lf[bsz:] + torch.tensor(scale, dtype=torch.float32) * (lf[:bsz] - lf[bsz:])) * inv_t
