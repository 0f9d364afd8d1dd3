"""ug_beam_candidates on the GPU against tests/beam_ref.py: candidates_ref (the definition, lse in fp64).  Beams and tokens must be
exactly the reference's, scores and lse within tol(V); every toleranced case asserts that the reference's own rank gaps are at least
10 tol(V), so that no rounding the tolerance allows could reorder it.  The exact cases are about ties, dead beams, NaN / -inf entries,
short groups, reproducibility and row independence."""
import numpy as np
import pytest
import torch

from beam_ref import candidates_ref, rank_gaps, tol

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 300, 2, 304), (1, 2, 257, 4, 264), (2, 4, 1003, 8, 1008), (4, 8, 4101, 16, 4104), (1, 8, 5000, 64, 5000),
          (2, 3, 159867, 9, 159872)]


def make_case(G, B, V, K, ld, seed=0):
    """Logits whose K + 1 best totals are well apart although bf16 keeps 8 bits: a body of noise (sigma 0.5, so below 2.5) and, per row,
    K + 2 planted entries 3 + 0.05 j (+ a jitter far below the bf16 step there), j a permutation -- distinct after rounding.  Between
    beams the running scores (uniform in [-3, 0], beam 0 at 0) separate the totals; rank_gaps has the last word."""
    g = torch.Generator().manual_seed(1234 + seed)
    R = G * B
    logits = torch.full((R, ld), float("nan"))                       # entries V .. ld - 1 are never read as candidates
    logits[:, :V] = torch.randn((R, V), generator=g) * 0.5
    n = min(K + 2, V)
    for r in range(R):
        where = torch.randperm(V, generator=g)[:n]
        logits[r, where] = 3.0 + 0.05 * torch.randperm(n, generator=g).float() + torch.rand(n, generator=g) * 1e-3
    scores = -3.0 * torch.rand(R, generator=g)
    scores[::B] = 0.0
    return logits, scores


def run(dev, logits, scores, G, B, V, K):
    from unigen_hip import ops
    out = ops.beam_candidates(logits.to(dev), scores.to(dev), G, B, V, K, want_lse=True)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize("G,B,V,K,ld", SHAPES)
def test_candidates_match_the_reference(dev, G, B, V, K, ld):
    logits, scores = make_case(G, B, V, K, ld)
    rs, rb, rt, rl = candidates_ref(logits, scores, G, B, V, K)
    gap = rank_gaps(logits, scores, G, B, V, K)
    assert gap >= 10 * tol(V), (gap, tol(V))
    cs, cb, ct, lse = run(dev, logits, scores, G, B, V, K)
    print("V", V, "max |score - ref|", float((cs - rs).abs().max()), "max |lse - ref|", float((lse - rl).abs().max()), "tol", tol(V), "gap", gap)
    assert torch.equal(cb, rb) and torch.equal(ct, rt)
    assert float((cs - rs).abs().max()) <= tol(V) and float((lse - rl).abs().max()) <= tol(V)


def _assert_order(out, ref):
    assert torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2]), (out[1], ref[1], out[2], ref[2])
    fin = torch.isfinite(ref[0])
    assert torch.equal(torch.isfinite(out[0]), fin) and torch.equal(out[0][~fin], ref[0][~fin])
    assert float((out[0][fin] - ref[0][fin]).abs().max()) <= tol(0) if fin.any() else True


def test_equal_rows_tie_exactly_and_the_lower_beam_wins(dev):
    G, B, V, K = 1, 2, 300, 6
    logits, _ = make_case(G, B, V, K, 304)
    logits[1] = logits[0]
    scores = torch.tensor([-0.75, -0.75])
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    assert out[1].tolist() == [[0, 1, 0, 1, 0, 1]] and torch.equal(out[2][0, 0::2], out[2][0, 1::2])
    assert torch.equal(out[0][0, 0::2], out[0][0, 1::2]) and out[3][0].item() == out[3][1].item()         # the same bits: row independence


def test_equal_bf16_logits_go_by_token(dev):
    G, B, V, K = 1, 1, 300, 4
    logits, scores = make_case(G, B, V, K, 304)
    logits[0, 211] = 7.001                                           # both round to 7.0
    logits[0, 17] = 6.999
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    assert out[2][0, :2].tolist() == [17, 211] and out[0][0, 0].item() == out[0][0, 1].item()


def test_more_ties_than_slots_are_taken_in_index_order(dev):
    """5 entries at 2.0, 500 at 1.0, the rest at 0: K = 8 takes the five, then the three lowest indices of the 500 -- in both beams,
    whose equal scores put beam 0's ties first; and a row of equal logits gives tokens 0 .. K - 1"""
    G, B, V, K = 2, 2, 1003, 8
    g = torch.Generator().manual_seed(5)
    logits = torch.zeros((G * B, 1008))
    perm = torch.randperm(V, generator=g)
    logits[:2, perm[:5]] = 2.0
    logits[:2, perm[5:505]] = 1.0
    scores = torch.tensor([-1.0, -1.0, 0.0, -1e9])
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    twos = sorted(perm[:5].tolist())
    assert out[2][0].tolist() == twos + twos[:3] and out[1][0].tolist() == [0] * 5 + [1] * 3
    assert out[2][1].tolist() == list(range(8)) and out[1][1].tolist() == [0] * 8
    K = 16                                                           # 10 twos over the two beams, then the six lowest ones of beam 0
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    assert out[2][0].tolist() == twos + twos + sorted(perm[5:505].tolist())[:6] and out[1][0].tolist() == [0] * 5 + [1] * 5 + [0] * 6


def test_step_zero_scores_take_every_candidate_from_beam_zero(dev):
    G, B, V, K = 2, 4, 1003, 8
    logits, _ = make_case(G, B, V, K, 1008)
    scores = torch.tensor([0.0, -1e9, -1e9, -1e9] * G)
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    assert (out[1] == 0).all() and torch.isfinite(out[0]).all()


def test_nan_and_minus_inf_entries_are_never_candidates(dev):
    G, B, V, K = 1, 2, 257, 64
    logits, scores = make_case(G, B, V, K, 264, seed=3)
    g = torch.Generator().manual_seed(9)
    bad = torch.randperm(V, generator=g)
    logits[0, bad[:100]] = float("nan")
    logits[0, bad[100:240]] = float("-inf")
    logits[1, bad[:120]] = float("-inf")
    logits[1, bad[120:250]] = float("nan")
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    n = (257 - 240) + (257 - 250)                                    # every finite entry of the two rows, then the empty tail
    assert torch.isfinite(out[0][0, :n]).all() and (out[1][0, n:] == -1).all() and (out[2][0, n:] == -1).all()
    assert (out[0][0, n:] == float("-inf")).all()
    for b, e in zip(out[1][0, :n].tolist(), out[2][0, :n].tolist()):
        assert np.isfinite(logits[b, e].item())
    assert float((out[3] - ref[3]).abs().max()) <= tol(V)


def test_short_groups_end_in_the_empty_tail(dev):
    G, B, V, K = 2, 2, 300, 8
    logits = torch.full((G * B, 304), float("-inf"))
    logits[0, [5, 250, 299]] = torch.tensor([0.5, 1.5, -2.0])
    logits[1, :V] = torch.randn(V, generator=torch.Generator().manual_seed(2))     # a dead beam: supplies nothing
    logits[2, 7] = 1.0
    logits[3, 8] = float("nan")                                                      # a row without any finite entry
    scores = torch.tensor([-0.5, -1e9, 0.0, -0.25])
    out, ref = run(dev, logits, scores, G, B, V, K), candidates_ref(logits, scores, G, B, V, K)
    _assert_order(out, ref)
    assert out[2].tolist() == [[250, 5, 299, -1, -1, -1, -1, -1], [7, -1, -1, -1, -1, -1, -1, -1]]
    assert out[1].tolist() == [[0, 0, 0, -1, -1, -1, -1, -1], [0, -1, -1, -1, -1, -1, -1, -1]]
    assert out[3][3].item() == float("-inf") and out[0][1, 0].item() == 0.0          # a single finite entry: log-probability 0


def test_same_bits_on_every_run_and_whatever_the_other_groups_hold(dev):
    G, B, V, K, ld = 4, 8, 4101, 16, 4104
    logits, scores = make_case(G, B, V, K, ld, seed=1)
    a = run(dev, logits, scores, G, B, V, K)
    b = run(dev, logits, scores, G, B, V, K)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    other, other_scores = make_case(G, B, V, K, ld, seed=2)
    other[B:2 * B], other_scores[B:2 * B] = logits[B:2 * B], scores[B:2 * B]        # group 1 as before, every other group changed
    c = run(dev, other, other_scores, G, B, V, K)
    for x, y in zip(a[:3], c[:3]):
        assert torch.equal(x[1], y[1])
    assert torch.equal(a[3][B:2 * B], c[3][B:2 * B]) and not torch.equal(a[2][0], c[2][0])
    # and as a group of its own, in another place of a smaller launch
    d = run(dev, logits[B:2 * B], scores[B:2 * B], 1, B, V, K)
    for x, y in zip(a[:3], d[:3]):
        assert torch.equal(x[1], y[0])
    assert torch.equal(a[3][B:2 * B], d[3])
