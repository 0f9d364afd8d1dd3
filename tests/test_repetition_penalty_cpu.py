"""The repetition penalty without a GPU: the host rule (models/sampling.py: apply_repetition_penalty) against a literal restatement of
transformers' RepetitionPenaltyLogitsProcessor, the host token loop with the processor in it, the device rule's restatement
(repetition_penalty_ref.py) on the special values, the argument checks of `generate`, and the new C entries' presence."""
import ctypes
import math
import os

import pytest
import torch

import repetition_penalty_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(R=5, V=211, L=23, seed=0):
    """logits with zeros, -0.0, negatives and positives; prompts with duplicate ids, ids 0 and V - 1, out-of-range ids, and masked
    (left-padding) positions that hold ids found nowhere else in the row"""
    g = torch.Generator().manual_seed(seed)
    logits = 4.0 * torch.randn(R, V, generator=g)
    ids = torch.randint(0, V // 2, (R, L), generator=g)
    valid = torch.ones(R, L, dtype=torch.bool)
    for r in range(R):
        valid[r, :r * 3] = False                                  # left padding, row 0 has none
        ids[r, :r * 3] = V // 2 + 7 + r                           # (an id the real positions never hold)
        ids[r, L - 1], ids[r, L - 2], ids[r, L - 3] = 0, V - 1, int(ids[r, L - 4])       # ids 0 and V - 1, a duplicate
        logits[r, int(ids[r, L - 4])] = 0.0
        logits[r, int(ids[r, L - 5])] = -0.0
        logits[r, 0] = -2.5
        logits[r, V - 1] = 3.25
    return logits, ids, valid


def test_host_rule_is_transformers_processor():
    from models.sampling import apply_repetition_penalty, seen_mask_of
    logits, ids, valid = _inputs()
    R, V = logits.shape
    for p in (1.3, 0.7, 2.0):
        seen = seen_mask_of(ids, valid, R, V, torch.device("cpu"))
        got = apply_repetition_penalty(logits, seen, p)
        for r in range(R):                                         # transformers sees the row's real ids, duplicates and all
            real = ids[r][valid[r]][None]
            want = ref.transformers_rule(real, logits[r:r + 1].clone(), p)
            assert ref.same_bits(got[r:r + 1], want), (p, r)
            masked_only = ids[r][~valid[r]]
            assert not bool(seen[r][masked_only].any())            # a masked position marks nothing
        assert ref.same_bits(got, ref.host_rule(logits, seen, p))
        assert ref.same_bits(apply_repetition_penalty(logits, torch.zeros_like(seen), p), logits)
    # ids outside [0, V) are ignored, no ids: nothing seen
    wild = ids.clone()
    wild[:, 5], wild[:, 6] = -1, V
    assert not bool(seen_mask_of(None, None, R, V, torch.device("cpu")).any())
    assert torch.equal(seen_mask_of(wild, None, R, V, torch.device("cpu")), ref.Bitmap(R, V).mark(wild).seen())


def test_bitmap_and_device_rule_restatement():
    logits, ids, valid = _inputs(V=77)
    R, V = logits.shape
    logits[0, 5], logits[1, 5], logits[2, 5], logits[3, 5] = float("inf"), float("nan"), float("-inf"), 1.00390625   # (not a bf16 value)
    ids[:, ids.shape[1] - 6] = 5                                  # (a real position of every row)
    bm = ref.Bitmap(R, V).mark(ids, valid)
    assert bm.words.shape == (R, 3) and torch.equal(bm.seen(), __import__("models.sampling", fromlist=["x"]).seen_mask_of(ids, valid, R, V, torch.device("cpu")))
    full = torch.cat([logits, torch.full((R, 3), 9.0)], 1)       # columns behind V
    out = bm.penalize(full, 1.3)
    seen = bm.seen()
    assert ref.same_bits(out[:, V:], full[:, V:]) and ref.same_bits(out[:, :V][~seen], logits[~seen])
    assert out[0, 5] == float("inf") and math.isnan(float(out[1, 5])) and out[2, 5] == float("-inf")
    assert float(out[3, 5]) == float(torch.tensor(1.0) / torch.tensor(1.3))                 # rounded to bf16 first: 1.0
    z = out[:, :V][seen & (logits == 0)]
    assert bool((z == 0).all()) and bool(torch.signbit(z).any()) and not bool(torch.signbit(z).all())
    assert ref.same_bits(out[:, :V][seen & (logits == 0)], logits[seen & (logits == 0)])      # 0 stays 0, -0.0 stays -0.0
    neg = seen & (logits < 0) & torch.isfinite(logits)
    assert ref.same_bits(out[:, :V][neg], ref.bf16round(logits)[neg] * torch.tensor(1.3))
    # a token joins once; bits at or above V are kept and never acted on
    before = bm.words.copy()
    bm.add([0] * R)
    assert (bm.words == before).all()
    bm.words[:, 2] |= 1 << 20                                     # id 84 >= V
    assert torch.equal(bm.seen(), seen)


def test_host_token_loop_applies_the_penalty_before_the_pick():
    """text_token_loop with with_repetition_penalty on a toy head whose logits do not depend on the input: without the penalty the
    greedy loop emits the same token forever; with it every step follows the rule on the history so far"""
    from models.unigen import emit_until_stop, text_token_loop, with_repetition_penalty
    from models.sampling import seen_mask_of
    R, V, n, p = 2, 50, 6, 1.5
    base = torch.linspace(1.0, 3.0, V)[None].repeat(R, 1)
    base[1] = base[1].flip(0)
    prompt = torch.tensor([[49, 3], [0, 1]])
    valid = torch.tensor([[1, 1], [0, 1]])
    out = torch.zeros((R, n), dtype=torch.long)
    seen = seen_mask_of(prompt, valid, R, V, torch.device("cpu"))
    pick, emit = with_repetition_penalty(lambda last: last.argmax(-1, keepdim=True), emit_until_stop(out, None), p, seen)
    steps = text_token_loop(n, None, pick, emit, head=lambda hn: base.clone(), embed=lambda ids: None, step=lambda x: None)
    assert steps == n
    hist = [{49, 3}, {1}]
    for i in range(n):
        for r in range(R):
            s = base[r].clone()
            for e in hist[r]:
                s[e] = s[e] * p if s[e] < 0 else s[e] / p
            assert int(out[r, i]) == int(s.argmax()), (i, r)
            hist[r].add(int(out[r, i]))
    assert len(set(out[0].tolist())) > 1 and int(out[1, 0]) == 0     # (row 1's id 0 was masked: not penalised at step 0)


@pytest.mark.parametrize("p", [0, 0.0, -1.3, float("nan"), float("inf"), float("-inf")])
def test_generate_refuses_a_bad_penalty_before_any_launch(p):
    """the check runs on the arguments alone: `self` is an object without a model behind it"""
    from models.unigen import UniGen
    from unigen_hip.lib import UniGenHipError
    ids = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(UniGenHipError, match="repetition_penalty"):
        UniGen.generate(object(), input_ids=ids, repetition_penalty=p)
    for fn in (UniGen.mmu_generate, UniGen.mmu_generate_batch):
        with pytest.raises(UniGenHipError, match="repetition_penalty"):
            fn(object(), idx=ids, attention_mask=torch.zeros(1, 1, 4, 4), repetition_penalty=p)


def test_generate_argument_rules():
    from models.unigen import UniGen, checked_repetition_penalty
    from unigen_hip.lib import UniGenHipError
    ids = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(UniGenHipError, match="do_sample"):
        UniGen.generate(object(), input_ids=ids, num_return_sequences=2)
    with pytest.raises(UniGenHipError, match="num_return_sequences"):
        UniGen.generate(object(), input_ids=ids, num_return_sequences=0, do_sample=True)
    with pytest.raises(UniGenHipError, match="num_beams.*not implemented"):
        UniGen.generate(object(), input_ids=ids, num_beams=2)
    with pytest.raises(UniGenHipError, match="penalty_alpha.*not implemented"):
        UniGen.generate(object(), input_ids=ids, penalty_alpha=0.6)
    assert checked_repetition_penalty(None, "x") == 1.0 and checked_repetition_penalty(1, "x") == 1.0 and checked_repetition_penalty(1.3, "x") == 1.3


def test_new_entries_are_in_the_library_the_header_and_the_binding():
    from unigen_hip import lib
    header = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ("ug_text_seen_mark", "ug_text_penalize"):
        assert hasattr(L, name) and name in lib.SIGNATURES and f"int {name}(" in header, name
    assert lib.load().ug_abi_version() == lib.ABI_VERSION == 7
    loaded = lib.load()
    assert loaded.ug_text_penalize(0, 0, 0, 0, 1.3, 0, 0, 0, 0) != 0 and b"ug_text_penalize" in loaded.ug_last_error()
    assert loaded.ug_text_seen_mark(0, 0, 0, 0, 0, 0, 0, 0, 0) != 0 and b"ug_text_seen_mark" in loaded.ug_last_error()
