"""Reference of ug_beam_candidates (include/unigen_hip.h: "Beam search of the text loop") on the CPU, shared by the beam tests.

candidates_ref restates the definition: s = bf16round(logit); lse in fp64 over the entries that are neither NaN nor -inf, rounded once
to fp32; total = (s - lse) + score as two fp32 operations in that order; candidates of a group ordered by (total descending, flat index
b * V + e ascending); dead beams (score <= -1e8), NaN and -inf entries supply none; missing slots are (-inf, -1, -1).

tol(V): bound on |kernel - reference| for cand_score and lse.  The issue's bound is 4 * 2^-17 + (ceil(V / 256) + 16) * 2^-23, whose second
term allows for an fp32 sum of V terms.  The kernel does not sum V terms: it sums one product count * expf(s - m) per bf16 PATTERN in
fp64 (csrc/beam.hip: beam_select_kernel), so the sum carries only the error of expf (a few fp32 ulp, relative) and log of it moves by
that much absolutely: under 8 * 2^-24.  The smaller derived bound is used, and it no longer grows with V:
    tol(V) = 4 * 2^-17 + 16 * 2^-23
first term: the fp32 roundings of lse, s - lse and the sum with the score, each of a value below 128 in magnitude (half an ulp = 2^-18
each, 3 * 2^-18 < 4 * 2^-17); second term: expf / log error of the lse with a factor of 2 to spare."""
import math

import numpy as np
import torch


def tol(V):
    return 4 * 2.0 ** -17 + 16 * 2.0 ** -23


def bf16_round(logits):
    return torch.as_tensor(logits, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def _row_lse(s64):
    """fp64 [V] (bf16 values) -> fp32 lse by the contract's special cases"""
    ok = ~np.isnan(s64)
    v = s64[ok]
    if v.size == 0 or v.max() == -np.inf:
        return np.float32(-np.inf)
    if v.max() == np.inf:
        return np.float32(np.inf)
    m = v.max()
    return np.float32(m + math.log(np.exp(v - m).sum()))


def _group_totals(logits, beam_scores, g, B, V):
    """-> (totals fp32 [n], flat index int64 [n]) of group g's candidates, sorted by (total descending, flat ascending); lse fp32 [B]"""
    tot, flat, lses = [], [], []
    for b in range(B):
        r = g * B + b
        s = bf16_round(logits[r, :V]).numpy()
        lse = _row_lse(s.astype(np.float64))
        lses.append(lse)
        score = np.float32(beam_scores[r])
        if not score > np.float32(-1e8) or not np.isfinite(lse):
            continue
        ok = np.isfinite(s)
        with np.errstate(all="ignore"):
            t = ((s[ok] - lse).astype(np.float32) + score).astype(np.float32)
        tot.append(t)
        flat.append(b * V + np.nonzero(ok)[0].astype(np.int64))
    if not tot:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.array(lses, np.float32)
    tot, flat = np.concatenate(tot), np.concatenate(flat)
    order = np.lexsort((flat, -tot.astype(np.float64)))          # stable on (-total, flat index)
    return tot[order], flat[order], np.array(lses, np.float32)


def candidates_ref(logits, beam_scores, G, B, V, K):
    """logits fp32 [G * B, >= V], beam_scores fp32 [G * B] -> (cand_score fp32 [G, K], cand_beam int32 [G, K], cand_token int32 [G, K],
    lse fp32 [G * B]) as CPU tensors"""
    logits = torch.as_tensor(logits).detach().float().cpu()
    beam_scores = torch.as_tensor(beam_scores).detach().float().cpu().numpy()
    cs = np.full((G, K), -np.inf, np.float32)
    cb = np.full((G, K), -1, np.int32)
    ct = np.full((G, K), -1, np.int32)
    lse = np.zeros(G * B, np.float32)
    for g in range(G):
        tot, flat, lses = _group_totals(logits, beam_scores, g, B, V)
        lse[g * B:(g + 1) * B] = lses
        n = min(K, tot.size)
        cs[g, :n], cb[g, :n], ct[g, :n] = tot[:n], flat[:n] // V, flat[:n] % V
    return torch.from_numpy(cs), torch.from_numpy(cb), torch.from_numpy(ct), torch.from_numpy(lse)


def rank_gaps(logits, beam_scores, G, B, V, K):
    """the smallest difference between consecutive totals among ranks 1 .. K + 1 of any group (inf where a group holds fewer than two)"""
    logits = torch.as_tensor(logits).detach().float().cpu()
    beam_scores = torch.as_tensor(beam_scores).detach().float().cpu().numpy()
    gap = math.inf
    for g in range(G):
        tot = _group_totals(logits, beam_scores, g, B, V)[0][:K + 1].astype(np.float64)
        if tot.size >= 2:
            gap = min(gap, float((tot[:-1] - tot[1:]).min()))
    return gap
