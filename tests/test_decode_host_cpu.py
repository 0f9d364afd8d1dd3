"""Host side of decoding, no GPU: the table of `Qwen2Engine.decode_form` (the one place that picks a decode layer form) and the
shared text token loop of `generate` / `mmu_generate` / `mmu_generate_batch` driven by stub callables and scripted logits."""
import os
import types

import pytest
import torch

QWEN_1P5B = dict(hidden_size=1536, intermediate_size=8960, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2,
                 head_dim=128)


def _engine(**over):
    """a Qwen2Engine with nothing but `dims` (decode_form reads sizes, `decode_fused` and the environment only)"""
    from unigen_hip import lib
    from unigen_hip.qwen2 import Qwen2Engine
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    eng = object.__new__(Qwen2Engine)
    eng.dims = types.SimpleNamespace(**dict(QWEN_1P5B, **over))
    return eng


# (dims overrides, decode_fused, UNIGEN_DECODE_SW, rows, deterministic) -> form
FORM_TABLE = [
    ({}, True, None, 1, False, "sw"),
    ({}, True, None, 16, False, "sw"),
    ({}, True, None, 17, False, "splitk"),
    ({}, True, None, 32, False, "splitk"),
    ({}, True, None, 33, False, "wide"),
    ({}, False, None, 1, False, "wide"),
    ({}, True, "0", 1, False, "splitk"),
    ({}, True, "0", 16, False, "splitk"),
    ({}, True, None, 1, True, "ord_sw"),
    ({}, True, None, 16, True, "ord_sw"),
    ({}, True, None, 17, True, "ord_wide"),
    ({}, False, None, 1, True, "ord_wide"),
    (dict(head_dim=64, num_attention_heads=24), True, None, 1, False, "wide"),
    (dict(intermediate_size=8976), True, None, 1, False, "wide"),                 # 1536-wide, intermediate no multiple of 32
    (dict(hidden_size=256, intermediate_size=512, num_attention_heads=2), True, None, 1, False, "splitk"),
    (dict(hidden_size=5120, num_attention_heads=40), True, None, 1, False, "wide"),     # wider than the split-K step's finisher takes
]


@pytest.mark.parametrize("over,fused,sw_env,rows,det,want", FORM_TABLE)
def test_decode_form_table(monkeypatch, over, fused, sw_env, rows, det, want):
    eng = _engine(**over)
    eng.decode_fused = fused
    if sw_env is None:
        monkeypatch.delenv("UNIGEN_DECODE_SW", raising=False)
    else:
        monkeypatch.setenv("UNIGEN_DECODE_SW", sw_env)
    assert eng.decode_form(rows, det) == want
    # the predicates read nothing but `.rows` and answer for their own mode
    st = type("S", (), {"rows": rows})()
    assert eng.decode_sw(st) == (eng.decode_form(rows, False) == "sw")
    assert eng.decode_ord_sw(st) == (eng.decode_form(rows, True) == "ord_sw")


def test_decode_form_default_is_fused_and_not_stored(monkeypatch):
    """`decode_fused` defaults to True, and the form is recomputed on every call: flipping the switches changes the next answer."""
    eng = _engine()
    monkeypatch.delenv("UNIGEN_DECODE_SW", raising=False)
    assert eng.decode_form(4, False) == "sw"
    monkeypatch.setenv("UNIGEN_DECODE_SW", "0")
    assert eng.decode_form(4, False) == "splitk" and eng.decode_form(4, True) == "ord_wide"
    eng.decode_fused = False
    assert eng.decode_form(4, False) == "wide"


# ------------------------------------------------------------------------------------------ the text token loop
V = 11


class _Stub:
    """head / embed / step over a script of token ids [steps][R]: the "hidden state" is the step index, `head` turns the script's row of
    ids into one-hot logits, `embed` and `step` record what they were given"""

    def __init__(self, script):
        self.script = torch.tensor(script)
        self.fed, self.steps = [], 0

    def head(self, hn):
        return torch.nn.functional.one_hot(self.script[hn], V).float()

    def embed(self, ids):
        self.fed.append(ids[:, 0].tolist())
        return ids

    def step(self, x):
        self.steps += 1
        return self.steps

    def run(self, n, emit):
        from models.unigen import text_token_loop
        return text_token_loop(n, 0, lambda lg: lg.argmax(-1, keepdim=True), emit, head=self.head, embed=self.embed, step=self.step)


def test_token_loop_takes_one_step_fewer_than_tokens():
    from models.unigen import emit_until_stop
    script = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]]
    for n in (0, 1, 3, 5):
        stub, out = _Stub(script), torch.full((2, 5), -1)
        assert stub.run(n, emit_until_stop(out, None)) == n
        assert stub.steps == max(n - 1, 0) and stub.fed == script[:max(n - 1, 0)]          # no step after the last token
        assert out[:, :n].t().tolist() == script[:n] and bool((out[:, n:] == -1).all())


def test_token_loop_stops_the_step_every_row_has_finished():
    from models.unigen import emit_until_stop
    EOS = 9
    script = [[1, EOS, 2], [EOS, 3, 4], [5, 6, EOS], [7, 7, 7], [8, 8, 8]]               # rows finish at steps 1, 0, 2
    stub, out = _Stub(script), torch.zeros((3, 5), dtype=torch.long)
    assert stub.run(5, emit_until_stop(out, torch.tensor([EOS, 10]))) == 3
    assert stub.steps == 2 and len(stub.fed) == 2


def test_generate_fills_finished_rows_with_pad_before_feeding_them_back():
    from models.unigen import emit_until_stop
    EOS, PAD = 9, 0
    script = [[1, EOS, 2], [3, 4, 5], [6, 7, EOS], [8, 8, 8]]                             # row 1 finishes first, row 0 never does
    stub, out = _Stub(script), torch.full((3, 4), PAD)
    assert stub.run(4, emit_until_stop(out, torch.tensor([EOS]), PAD)) == 4
    assert out.tolist() == [[1, 3, 6, 8], [EOS, PAD, PAD, PAD], [2, 5, EOS, PAD]]
    assert stub.fed == [[1, EOS, 2], [3, PAD, 5], [6, PAD, EOS]]                         # (the pad, not the raw pick, is embedded)
    # without a stop id nothing is filled and nothing stops
    stub, out = _Stub(script), torch.full((3, 4), PAD)
    assert stub.run(4, emit_until_stop(out, None, PAD)) == 4 and out.t().tolist() == script


def test_mmu_batch_cuts_each_row_after_its_own_stop_token():
    from models.unigen import emit_until_stop
    EOT, n = 9, 5
    script = [[1, EOT, 2], [3, 4, 5], [EOT, 6, 7], [8, EOT, 8], [1, 1, 1]]                # row 0 ends at 3 tokens, row 1 at 1, row 2 never
    stub = _Stub(script)
    tokens, lengths = torch.zeros((3, n), dtype=torch.long), torch.full((3,), n)
    assert stub.run(n, emit_until_stop(tokens, EOT, lengths=lengths)) == n                 # (row 2 keeps the loop going)
    assert lengths.tolist() == [3, 1, n]                                                  # row 1's second EOT does not move its cut
    assert tokens.t().tolist() == script and stub.fed == script[:n - 1]                   # recorded and fed back unpadded
    # every row has one -> the loop ends there; a 0-d tensor serves as the stop id (mmu_generate hands over a sampled token)
    stub = _Stub([[1, EOT], [EOT, 2], [3, 3]])
    tokens, lengths = torch.zeros((2, 3), dtype=torch.long), torch.full((2,), 3)
    assert stub.run(3, emit_until_stop(tokens, torch.tensor(EOT), lengths=lengths)) == 2
    assert lengths.tolist() == [2, 1] and stub.steps == 1
