"""Beam search without a GPU: models/beam.py: BeamSearch pinned to transformers' generate(num_beams=B, do_sample=False) on a random
Qwen2 model; the launch plans of csrc/beam_plan.h (compiled alone for the host under ASan + UBSan, as tests/test_head_score_cpu.py
does it); the three entry points declared, bound, exported and refusing what is outside their limits; UniGen.beam_search's refusals."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from beam_ref import candidates_ref, rank_gaps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ml-unigen_amd", "csrc")

# ------------------------------------------------------------------ 1. BeamSearch against transformers
V, L, NEW = 97, 6, 12
GAP = 1e-4
# (num_beams, prompts, eos ids) -> (prompt seed, eos ids) found on the CPU: in the first a hypothesis ends before max_new_tokens, in
# the second none does; in both the reference's rank gaps stay above GAP at all 12 steps.
EARLY = {(1, 1, 1): (14, [48]), (1, 1, 2): (14, [48, 92]), (1, 3, 1): (14, [48]), (1, 3, 2): (14, [48, 92]),
         (2, 1, 1): (0, [78]), (2, 1, 2): (0, [78, 34]), (2, 3, 1): (0, [90]), (2, 3, 2): (0, [90, 34]),
         (4, 1, 1): (0, [78]), (4, 1, 2): (0, [78, 34]), (4, 3, 1): (0, [78]), (4, 3, 2): (4, [74, 69])}
NONE = {(1, 1, 1): (0, [34]), (1, 1, 2): (0, [34, 48]), (1, 3, 1): (0, [34]), (1, 3, 2): (0, [34, 48]),
        (2, 1, 1): (0, [34]), (2, 1, 2): (0, [34, 48]), (2, 3, 1): (3, [58]), (2, 3, 2): (3, [58, 9]),
        (4, 1, 1): (0, [34]), (4, 1, 2): (7, [67, 53]), (4, 3, 1): (0, [34]), (4, 3, 2): (64, [83, 89])}
SEEN = {}                        # early_stopping value -> {True, False}: whether a hypothesis ended early in a case that ran


@pytest.fixture(scope="module")
def hf_model():
    transformers = pytest.importorskip("transformers", reason="transformers is needed to pin BeamSearch to its beam search")
    torch.manual_seed(0)
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(2.0)
        m.lm_head.weight.mul_(20.0)           # logits with a spread of about 5: distinct candidates, few bf16 ties
    # the head's rounding of the precision contract, applied to the model itself so that both sides see the same logits (shifted so the
    # row maximum is 0, where bf16 is finest; log_softmax does not see the shift)
    m.lm_head.register_forward_hook(lambda mod, i, o: (o - o.amax(-1, keepdim=True)).to(torch.bfloat16).to(torch.float32))
    return m


def _prompts(G, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (G, L), generator=g)
    mask = torch.ones((G, L), dtype=torch.long)
    for r in range(G):
        mask[r, :r % 3] = 0                    # left padding: 0, 1, 2 positions
        ids[r, :r % 3] = 0
    return ids, mask


@torch.no_grad()
def _ours(m, ids, mask, B, eos, lp, es, n_ret):
    """BeamSearch driven by candidates_ref on the model's full-recompute logits -> (sequences, scores, smallest rank gap, early)"""
    from models.beam import BeamSearch
    G = ids.shape[0]
    bs = BeamSearch(G, B, eos, eos[0], NEW, lp, es, n_ret)
    seq, msk = ids.repeat_interleave(B, 0), mask.repeat_interleave(B, 0)
    gap, early = float("inf"), False
    for _ in range(NEW):
        pos = (msk.cumsum(-1) - 1).masked_fill(msk == 0, 1)
        logits = m(input_ids=seq, attention_mask=msk, position_ids=pos, use_cache=False).logits[:, -1].float()
        scores = bs.running_scores()
        gap = min(gap, rank_gaps(logits, scores, G, B, V, bs.k))
        parent, tok, finished = bs.step(*candidates_ref(logits, scores, G, B, V, bs.k)[:3])
        early |= bs.steps < NEW and bool(bs.is_fin.any())          # a hypothesis entered the pool before the last step
        if finished:
            break
        seq, msk = torch.cat([seq[parent.long()], tok], 1), torch.cat([msk, torch.ones_like(msk[:, :1])], 1)
    out, sc = bs.finalize()
    return torch.cat([ids.repeat_interleave(n_ret, 0), out], 1), sc, gap, early


@pytest.mark.parametrize("B,G", [(1, 1), (1, 3), (2, 1), (2, 3), (4, 1), (4, 3)])
def test_beam_search_is_transformers_beam_search(hf_model, B, G):
    """Every length_penalty x early_stopping x eos count for this (num_beams, prompts); the early / none flavour of the eos ids and
    num_return_sequences in {1, B} alternate over them so that each early_stopping value meets both of each."""
    for (li, lp), (ei, es), (ni, n_eos) in itertools.product(enumerate((0.0, 1.0, 2.0)), enumerate((False, True, "never")), enumerate((1, 2))):
        flavour = EARLY if (li + ni) % 2 == 0 else NONE
        n_ret = B if (li + ei + ni) % 2 == 0 else 1
        seed, eos = flavour[(B, G, n_eos)]
        ids, mask = _prompts(G, seed)
        seqs, scores, gap, early = _ours(hf_model, ids, mask, B, eos, lp, es, n_ret)
        ref = hf_model.generate(input_ids=ids, attention_mask=mask, num_beams=B, do_sample=False, max_new_tokens=NEW, length_penalty=lp,
                                early_stopping=es, eos_token_id=eos, pad_token_id=eos[0], num_return_sequences=n_ret, use_cache=False,
                                return_dict_in_generate=True, output_scores=True)
        what = (B, G, lp, es, eos, n_ret)
        assert gap > GAP, (what, gap)                                          # no case is skipped for a small gap: the seeds hold
        assert early == (flavour is EARLY), what
        assert seqs.shape == ref.sequences.shape and torch.equal(seqs, ref.sequences), (what, seqs, ref.sequences)
        if B > 1:                                                              # (greedy search reports no sequence scores)
            assert float((scores - ref.sequences_scores).abs().max()) <= NEW * 8 * 2.0 ** -19, (what, scores, ref.sequences_scores)
        SEEN.setdefault(es, set()).add(early)


def test_every_early_stopping_value_met_an_early_end_and_none(hf_model):
    """runs behind the cases above (file order): each early_stopping value saw a hypothesis end early in one case and none in another"""
    assert SEEN == {False: {True, False}, True: {True, False}, "never": {True, False}}, SEEN


def test_beam_search_class_basics():
    from models.beam import BeamSearch, beams_to_keep
    assert [beams_to_keep(4, n) for n in (0, 1, 2, 7)] == [8, 8, 12, 32] and BeamSearch(2, 3, [5, 9], None, 4).k == 9
    bs = BeamSearch(2, 3, [5], None, 4)
    assert bs.running_scores().tolist() == [0.0, -1e9, -1e9] * 2 and bs.pad == 5
    with pytest.raises(ValueError):
        BeamSearch(1, 2, [5], None, 4, early_stopping="always")
    # one step by hand: two prompts, two beams, eos 5.  Prompt 0's best candidate is the eos: it enters the pool, the next two run on.
    bs = BeamSearch(2, 2, [5], 0, 3, length_penalty=1.0)
    cs = torch.tensor([[-0.1, -0.5, -0.9, -2.0], [-0.2, -0.3, -0.4, -float("inf")]])
    cb = torch.tensor([[0, 0, 0, 0], [0, 0, 0, -1]], dtype=torch.int32)
    ct = torch.tensor([[5, 7, 8, 9], [1, 2, 5, -1]], dtype=torch.int32)
    parent, tok, finished = bs.step(cs, cb, ct)
    assert parent.dtype == torch.int32 and parent.tolist() == [0, 0, 2, 2] and tok.tolist() == [[7], [8], [1], [2]] and not finished
    assert torch.allclose(bs.running_scores(), torch.tensor([-0.5, -0.9, -0.2, -0.3]))
    assert bs.is_fin.tolist() == [[True, False], [False, False]] and abs(float(bs.fin_scores[0, 0]) + 0.1) < 1e-7
    seqs, scores = bs.finalize()
    assert seqs.tolist()[0] == [5] and abs(float(scores[0]) + 0.1) < 1e-7


# ------------------------------------------------------------------ 2. csrc/beam_plan.h
@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/beam_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("beam_plan") / "beam_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "beam_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [[int(v) for v in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


CAND = ["rows", "segs", "select_grid", "merge_grid", "hist_off", "count_off", "zero_bytes", "meta_off", "list_total_off", "list_token_off",
        "ws_bytes", "seg", "seg_threads", "select_threads", "merge_threads", "bins", "max_k", "max_rows", "meta_ints"]


def test_candidate_plan_grids_and_workspace(dumper):
    from unigen_hip import lib
    lb = lib.load()
    cases = [(G, B, Vv, K) for G in range(1, 33) for B in range(1, 9) if G * B <= 32
             for Vv in (1, 8191, 8192, 8193, 159867, 262144) for K in (1, 2, 16, 63, 64)]
    for (G, B, Vv, K), row in zip(cases, dumper(["cand %d %d %d %d" % c for c in cases])):
        pl = dict(zip(CAND, row))
        R = G * B
        assert pl["rows"] == R == pl["select_grid"] and pl["merge_grid"] == G                    # a workgroup per row / per group
        assert pl["segs"] >= 1 and pl["segs"] * pl["seg"] >= Vv > (pl["segs"] - 1) * pl["seg"]   # the segments cover [0, V), none is empty
        assert pl["bins"] == 65536 and pl["bins"] % pl["select_threads"] == 0 and (pl["bins"] // pl["select_threads"]) % 4 == 0
        assert pl["merge_threads"] == 8 * pl["max_k"] and K <= pl["max_k"] and B * pl["max_k"] <= pl["merge_threads"]
        # the regions the kernels index, in order, none overlapping, all inside; the cleared part is the histogram and the counters
        regions = [("hist_off", R * pl["bins"] * 4), ("count_off", pl["max_rows"] * 4), ("meta_off", R * pl["meta_ints"] * 4),
                   ("list_total_off", R * pl["max_k"] * 4), ("list_token_off", R * pl["max_k"] * 4)]
        end = 0
        for name, size in regions:
            assert pl[name] == end and pl[name] % 16 == 0, (name, pl)
            end += size
        assert pl["ws_bytes"] == end == lb.ug_beam_candidates_ws_bytes(G, B, Vv, K) and R <= pl["max_rows"] and pl["meta_ints"] >= 5
        assert pl["zero_bytes"] == pl["meta_off"]
    outside = [(0, 1, 5, 1), (1, 0, 5, 1), (1, 9, 5, 1), (5, 7, 5, 1), (33, 1, 5, 1), (1, 1, 0, 1), (1, 1, 262145, 1), (1, 1, 5, 0),
               (1, 1, 5, 65), (-1, -1, -1, -1), (2 ** 40, 2 ** 40, 5, 1)]
    for c, row in zip(outside, dumper(["cand %d %d %d %d" % c for c in outside])):
        assert row[:11] == [0] * 11, (c, row)
        assert lb.ug_beam_candidates_ws_bytes(*c) == -1 and "ug_beam_candidates_ws_bytes" in lb.ug_last_error().decode()


def test_kv_reorder_plan(dumper):
    cases = [(n, R, HKV, Tmax, 128, first, span) for n in (1, 3, 28) for R in (1, 2, 8, 32) for HKV in (1, 2, 8)
             for Tmax, first, span in ((256, 0, 1), (256, 37, 70), (256, 128, 128), (4096, 1000, 64), (1, 0, 1))]
    for (n, R, HKV, Tmax, hd, first, span), (gx, gy, gz, pieces, spare, threads, per) in zip(cases, dumper(["kv %d %d %d %d %d %d %d" % c for c in cases])):
        assert per * 16 == hd * 2 and pieces == HKV * span * per                 # a lane per 16 bytes of every (head, position)
        assert gx >= 1 and gx * threads >= pieces > (gx - 1) * threads and (gy, gz) == (R, 2 * n)
        assert spare == 2 * n * R * HKV * span * hd * 2
    outside = [(0, 2, 2, 256, 128, 0, 8), (1, 0, 2, 256, 128, 0, 8), (1, 33, 2, 256, 128, 0, 8), (1, 2, 0, 256, 128, 0, 8), (1, 2, 2, 256, 64, 0, 8),
               (1, 2, 2, 256, 128, -1, 8), (1, 2, 2, 256, 128, 0, 0), (1, 2, 2, 256, 128, 250, 8), (1, 2, 2, 256, 128, 2 ** 62, 2 ** 62),
               (1, 2, 2, 0, 128, 0, 0), (2000, 2, 2, 256, 128, 0, 8)]
    for c, row in zip(outside, dumper(["kv %d %d %d %d %d %d %d" % c for c in outside])):
        assert row[:5] == [0] * 5, (c, row)


# ------------------------------------------------------------------ 3. the entry points
def test_entry_points_are_declared_bound_exported_and_check_their_arguments():
    from unigen_hip import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unigen_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in (("ug_beam_candidates_ws_bytes", 4), ("ug_beam_candidates", 13), ("ug_beam_kv_reorder", 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert len(lib.SIGNATURES[name]) == nargs and hasattr(so, name) and hasattr(lib.api(), name)
    assert "ug_beam_candidates_ws_bytes" in lib.VALUE_RETURNS
    lb = lib.load()
    assert lb.ug_abi_version() == lib.ABI_VERSION == 7                          # additions do not bump the version
    buf = np.zeros(4096, dtype=np.uint8)
    p = (buf.ctypes.data + 15) & ~15                                             # a host address stands in: nothing is dereferenced before the checks

    def cand(logits=p, ld=304, G=1, B=2, Vv=300, scores=p, K=4, ws=p, cs=p, cb=p, ct=p):
        return lb.ug_beam_candidates(logits, ld, G, B, Vv, scores, K, ws, cs, cb, ct, None, None), lb.ug_last_error().decode()

    def kv(k=p, v=p, n=3, R=4, HKV=2, Tmax=256, hd=128, parent=p, ln=p, first=10, spare=p, span=20):
        return lb.ug_beam_kv_reorder(k, v, n, R, HKV, Tmax, hd, parent, ln, first, spare, span, None), lb.ug_last_error().decode()

    assert lb.ug_beam_candidates(*[0] * 13) == -1 and lb.ug_last_error() and lb.ug_beam_kv_reorder(*[0] * 13) == -1 and lb.ug_last_error()
    assert lb.ug_beam_candidates_ws_bytes(0, 0, 0, 0) == -1 and lb.ug_last_error()
    for kw, word in ((dict(B=0), "1 <= B <= 8"), (dict(B=9), "1 <= B <= 8"), (dict(G=5, B=7), "G*B <= 32"), (dict(K=0), "1 <= K <= 64"),
                     (dict(K=65), "1 <= K <= 64"), (dict(Vv=0), "1 <= V"), (dict(Vv=262145, ld=262152), "V <= 262144"), (dict(ld=299), "V <= ld"),
                     (dict(logits=None), "logits and beam_scores"), (dict(scores=None), "logits and beam_scores"), (dict(ws=None), "ws must not be null"),
                     (dict(ws=p + 4), "16B aligned"), (dict(cs=None), "cand_score"), (dict(cb=None), "cand_beam"), (dict(ct=None), "cand_token")):
        rc, msg = cand(**kw)
        assert rc == -1 and word in msg and msg.startswith("ug_beam_candidates:"), (kw, rc, msg)
    for kw, word in ((dict(hd=64), "head_dim must be 128"), (dict(R=33), "R <= 32"), (dict(R=0), "R <= 32"), (dict(first=250, span=20), "first + span <= Tmax"),
                     (dict(span=0), "span >= 1"), (dict(first=-1), "first >= 0"), (dict(n=0), "n_layers"), (dict(HKV=0), "HKV >= 1"),
                     (dict(k=None), "must not be null"), (dict(v=None), "must not be null"), (dict(parent=None), "must not be null"),
                     (dict(ln=None), "must not be null"), (dict(spare=None), "spare must not be null"), (dict(spare=p + 8), "16B aligned")):
        rc, msg = kv(**kw)
        assert rc == -1 and word in msg and msg.startswith("ug_beam_kv_reorder:"), (kw, rc, msg)
    with pytest.raises(lib.UniGenHipError):
        from unigen_hip import ops
        ops.beam_candidates(torch.zeros(2, 304), torch.zeros(2), 1, 2, 300, 4)        # host tensors: no CPU fallback


# ------------------------------------------------------------------ 4. refusals of UniGen.beam_search, before the engine is touched
def test_beam_search_refuses_before_touching_the_engine():
    from models.unigen import UniGen, generate_call
    from unigen_hip.lib import UniGenHipError
    ids = torch.zeros((4, 5), dtype=torch.long)

    def refuse(match, **kw):
        kw.setdefault("input_ids", ids)
        with pytest.raises(UniGenHipError, match=match):
            UniGen.beam_search(object(), **kw)          # an object() has no engine: anything but the refusal is an AttributeError

    refuse("5 prompts x num_beams=8 = 40 rows", input_ids=torch.zeros((5, 5), dtype=torch.long), num_beams=8)
    refuse("num_beams=9 must be between 1 and 8", num_beams=9, input_ids=ids[:1])
    refuse("num_beams=0 must be between 1 and 8", num_beams=0)
    refuse("num_return_sequences=5 must be between 1 and num_beams=4", num_return_sequences=5)
    refuse("num_return_sequences=0", num_return_sequences=0)
    refuse("8 eos ids", eos_token_id=list(range(8)), num_beams=2)
    refuse("max_new_tokens=0 must be at least 1", max_new_tokens=0)
    refuse("early_stopping", early_stopping="always")
    refuse("give input_ids or input_embeddings", input_ids=None)
    for name, value in (("do_sample", True), ("repetition_penalty", 1.3), ("logit_bias", {3: 1.0}), ("suppress_tokens", [3]), ("min_new_tokens", 2),
                        ("no_repeat_ngram_size", 2), ("stop_sequences", [[1, 2]]), ("return_logprobs", True), ("num_beam_groups", 2),
                        ("on_device", True)):
        refuse(r"beam_search: \['%s'\] are not implemented" % name, **{name: value})
    refuse("unknown arguments", temperature=0.5)
    with pytest.raises(AttributeError):                 # the defaults of the refused options pass the checks and reach the engine
        UniGen.beam_search(object(), input_ids=ids, do_sample=False, repetition_penalty=1.0, on_device=False, num_beam_groups=1)
    with pytest.raises(UniGenHipError, match="num_beams.*not implemented"):
        generate_call(lambda: 100, False, 1.0, None, None, None, None, None, None, False, {"num_beams": 2})
