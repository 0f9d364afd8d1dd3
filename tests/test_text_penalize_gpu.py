"""ug_text_seen_mark + ug_text_penalize (csrc/text_sampler.hip) through ops.text_seen_mark_ / ops.text_penalize_: exact, against
repetition_penalty_ref.Bitmap.  Every pair of V in {77 (one partial last word), 4 099 (a word count that is no multiple of the block),
159 867 (the real vocabulary: 27 bits in the last word)} and R in {1, 3, 32}; both row layouts (ld = V rounded up to 8, and ld = V, the
deterministic head's); tok null and non-null with the three kinds of token (in an otherwise empty word, in the last word, an id seen
already) rotating over the rows.

Logits: 3 x randn (not bf16-representable) with 0.0, -0.0, a negative and (two rows in three) +inf planted at seen ids; distinct
patterns behind V and in a guard row.  Prompts: ids below V / 3 with duplicates, ids 0 and V - 1, out-of-range ids, masked positions
holding ids found nowhere else.  Bits at or above V are planted in the last bitmap word."""
import pytest
import torch

import repetition_penalty_ref as ref

pytestmark = pytest.mark.gpu

P = 1.3
L = 37
H = 64


def _case(V, R, seed):
    g = torch.Generator().manual_seed(seed)
    W = (V + 31) // 32
    ids = torch.randint(1, max(2, V // 3), (R, L), generator=g)
    valid = torch.ones(R, L, dtype=torch.bool)
    special = {}
    for r in range(R):
        npad = (r * 5) % 11
        valid[r, :npad] = False
        ids[r, :npad] = V // 3 + 1 + r % 3                          # masked: ids the real positions never hold
        ids[r, 12], ids[r, 13] = int(ids[r, 14]), int(ids[r, 14])   # duplicates
        ids[r, 15], ids[r, 16] = 0, V - 1
        ids[r, 17], ids[r, 18], ids[r, 19], ids[r, 20] = -1, V, V + 5, 1 << 40      # out of range
        special[r] = [int(ids[r, 21 + j]) for j in range(4)]
    return ids, valid, special, W


def _logits(V, R, ld, special, seed):
    g = torch.Generator().manual_seed(seed + 1)
    full = torch.empty(R + 1, ld)
    full[:, :V] = 3.0 * torch.randn(R + 1, V, generator=g)
    full[:, V:] = 1e30 + 1e24 * torch.arange(ld - V)[None]        # distinct patterns behind V
    full[R] = 7e29 + 1e24 * torch.arange(ld)                        # the guard row
    for r in range(R):
        a, b, c, d = special[r]
        full[r, a], full[r, b], full[r, c] = 0.0, -0.0, -1.00390625
        if r % 3:
            full[r, d] = float("inf")
        full[r, 0], full[r, V - 1] = -2.7, 5.3
    return full


def _tok(V, R, W, ids, kind):
    """the three kinds of previous-step token, rotating over the rows from `kind`"""
    tok = torch.zeros(R, dtype=torch.long)
    for r in range(R):
        k = (r + kind) % 3
        tok[r] = (32 * (W // 2) + 5, V - 2, int(ids[r, 14]))[k]   # empty word (prompt ids stay below V / 3) / last word / seen already
    return tok


@pytest.mark.parametrize("R", [1, 3, 32])
@pytest.mark.parametrize("V", [77, 4099, 159867])
def test_mark_and_penalize_are_exact(dev, V, R):
    from unigen_hip import ops
    ids, valid, special, W = _case(V, R, seed=V + R)
    assert (32 * (W // 2) + 5) // 32 > (V // 3 + 3) // 32 and (V - 2) // 32 == W - 1 and V % 32 != 0
    ids_d, valid_d = ids.to(dev), valid.to(dev)
    emb = torch.zeros(V, H, device=dev)
    for ld in (ops.round_up(V, 8), V):
        full = _logits(V, R, ld, special, seed=V + R)
        for kind in (None, 0, 1, 2):
            tok = None if kind is None else _tok(V, R, W, ids, kind)
            # ---- reference
            bm = ref.Bitmap(R, V).mark(ids, valid)
            high = 1 << (V % 32 + 1)                                # an id at or above V in the last word: kept, never acted on
            bm.words[R - 1, W - 1] |= high
            want = full.clone()
            want[:R] = bm.penalize(full[:R], P, tok)
            assert not ref.same_bits(want, full) and ref.same_bits(want[R], full[R]) and ref.same_bits(want[:, V:], full[:, V:])
            # ---- device, twice on the same inputs
            got = []
            for _ in range(2):
                seen = ops.text_seen(R, V, dev)
                assert tuple(seen.shape) == (R, W)
                ops.text_seen_mark_(seen, ids_d, V, valid_d)
                seen[R - 1, W - 1] |= high
                lg = full.to(dev)
                ops.text_penalize_(lg[:R], V, P, seen, tok=None if tok is None else tok.to(dev))
                got.append((seen.cpu(), lg.cpu(), lg))
            assert torch.equal(got[0][0], got[1][0]) and ref.same_bits(got[0][1], got[1][1])
            assert torch.equal(got[0][0], bm.tensor()), (ld, kind)
            assert ref.same_bits(got[0][1], want), (ld, kind, int((got[0][1].view(torch.int32) != want.view(torch.int32)).sum()))
            # ---- the picks behind it: lowest index of the maximum of the processed, bf16-rounded row
            arg = ref.first_argmax(want[:R, :V])
            state = ops.text_state(R, dev)
            tk = torch.full((R,), -1, dtype=torch.long, device=dev)
            out = torch.zeros((R, 2), dtype=torch.int32, device=dev)
            x = torch.zeros(R, H, device=dev)
            ops.text_pick_(got[0][2][:R], V, state, 2, emb, tk, out, x)
            assert torch.equal(tk.cpu(), arg), (ld, kind, tk.tolist(), arg.tolist())
            state = ops.text_state(R, dev)
            tk.fill_(-1)
            ops.text_sample_(got[1][2][:R], V, state, 2, emb, tk, out, x, torch.zeros(2, R, device=dev), ops.text_sample_workspace(R, dev),
                             temperature=0.8, top_k=1)
            assert torch.equal(tk.cpu(), arg), (ld, kind, tk.tolist(), arg.tolist())
            assert ref.same_bits(got[0][2].cpu(), want) and ref.same_bits(got[1][2].cpu(), want)      # the picks wrote nothing


def test_mark_without_a_mask_and_over_several_blocks(dev):
    """valid = None marks every position; 700 positions span three blocks of the mark launch; a strided ids view is taken as it is"""
    from unigen_hip import ops
    R, V, n = 3, 4099, 700
    g = torch.Generator().manual_seed(3)
    wide = torch.randint(-5, V + 5, (R, n + 9), generator=g)
    ids = wide[:, 4:4 + n]
    seen = ops.text_seen(R, V, dev)
    ops.text_seen_mark_(seen, wide.to(dev)[:, 4:4 + n], V)
    assert torch.equal(seen.cpu(), ref.Bitmap(R, V).mark(ids).tensor())


def test_penalize_and_mark_refuse_bad_arguments(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    V = 100
    lg = torch.zeros(2, V, device=dev)
    seen = ops.text_seen(2, V, dev)
    for p in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(UniGenHipError, match="finite"):
            ops.text_penalize_(lg, V, p, seen)
    with pytest.raises(UniGenHipError):                              # a bitmap too narrow for V
        ops.text_penalize_(lg, V, P, ops.text_seen(2, 64, dev))
    with pytest.raises(UniGenHipError):                              # V beyond the row
        ops.text_penalize_(lg, V + 1, P, ops.text_seen(2, V + 1, dev))
    with pytest.raises(UniGenHipError):                              # 33 rows
        ops.text_penalize_(torch.zeros(33, V, device=dev), V, P, ops.text_seen(33, V, dev))
    with pytest.raises(UniGenHipError):                              # rows disagree
        ops.text_seen_mark_(seen, torch.zeros(3, 4, dtype=torch.long, device=dev), V)
    with pytest.raises(UniGenHipError):                              # mask shape
        ops.text_seen_mark_(seen, torch.zeros(2, 4, dtype=torch.long, device=dev), V, torch.ones(2, 5, device=dev))
    assert not bool(seen.any()) and not bool(lg.any())
