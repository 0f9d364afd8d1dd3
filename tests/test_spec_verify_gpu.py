"""ug_spec_verify (csrc/spec_decode.hip) on crafted logits against tests/spec_ref.py: the pick (bf16-rounded values, lowest index on
ties), accept, emit with the stop rule and the width cut, the history, the position, the counters, the next draft and the next inputs --
tok and the embedding rows x, padding rows included, bit for bit.  V = 4 096 and 1 003 (no multiple of 8; the tie test gives it an odd
leading dimension, 1 017, which takes the pick kernel that reads one entry at a time)."""
import pytest
import torch

from spec_ref import SpecRef

pytestmark = pytest.mark.gpu

S, K, G, H = 8, 7, 2, 64


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t

HISTORY = list(range(100, 120)) + [100]              # every id once, then the first again: the text behind it is the draft


class _Dev:
    """the device side of one session + the reference state, advanced together and compared after every call"""

    def __init__(self, dev, V, width, stop=(), pos=40, history=HISTORY, ld=None):
        from unigen_hip import ops
        self.ops, self.dev, self.V, self.width = ops, dev, V, width
        g = torch.Generator().manual_seed(V)
        self.embed = torch.randn(V + 5, H, generator=g).to(dev)
        self.ld = ops.round_up(V, 8) if ld is None else ld
        self.state = torch.zeros(ops.SPEC_STATE_INTS, dtype=torch.int32, device=dev)
        self.state[ops.SPEC_HIST_LEN] = len(history)
        self.hist = torch.zeros(len(history) + width + 3, dtype=torch.int32, device=dev)
        self.hist[:len(history)] = torch.tensor(history, dtype=torch.int32)
        self.tok = torch.zeros(S, dtype=torch.long, device=dev)
        self.x = torch.full((S, H), float("nan"), device=dev)
        self.out = torch.full((width + 3,), -1, dtype=torch.int32, device=dev)
        self.lengths = torch.full((1,), width, dtype=torch.int32, device=dev)
        self.pos = torch.tensor([pos], dtype=torch.int32, device=dev)
        self.len = torch.tensor([pos + 1], dtype=torch.int32, device=dev)
        self.stop = torch.tensor(list(stop), dtype=torch.long, device=dev) if stop else None
        self.ref = SpecRef(history, S, G, K, width, stop, pos=pos)
        self.gen = g

    def logits_for(self, picks, rows):
        """fp32 [S, ld]: bf16-exact noise in [-1, 1], 5.0 at the pick of each of the first `rows` rows"""
        lg = torch.rand(S, self.ld, generator=self.gen).mul(2).sub(1).bfloat16().float()
        for s in range(rows):
            lg[s, picks[s]] = 5.0
        return lg

    def snapshot(self):
        return [t.clone() for t in (self.state[:8], self.tok, self.x, self.out, self.hist, self.pos, self.len, self.lengths)]

    def call(self, lg, rows=S, advance=True, clear=False):
        ops = self.ops
        lg = lg.to(self.dev)
        want = lg[:rows, :self.V].bfloat16().float().argmax(-1).tolist()          # (torch.argmax: the first maximal index)
        tok_in = self.tok.tolist()
        ops.spec_verify_(lg, rows, self.V, self.state, self.width, self.embed, self.tok, self.out, self.x, self.hist, G, K, clear=clear,
                         stop_ids=self.stop, lengths=self.lengths, advance=(self.pos, self.len) if advance else None)
        torch.cuda.synchronize()
        st = self.state.tolist()
        assert st[ops.SPEC_PICK:ops.SPEC_PICK + rows] == want, "picks"
        was_done = self.ref.done
        nxt = self.ref.verify(want, tok_in, advance=advance)
        r = self.ref
        assert st[ops.SPEC_EMITTED] == len(r.out) and st[ops.SPEC_DONE] == int(r.done)
        assert (st[ops.SPEC_STEPS], st[ops.SPEC_DRAFTED], st[ops.SPEC_ACCEPTED]) == (r.steps, r.drafted, r.accepted)
        assert st[ops.SPEC_HIST_LEN] == len(r.h) and self.hist[:len(r.h)].tolist() == r.h
        assert self.out[:len(r.out)].tolist() == r.out and bool((self.out[len(r.out):] == -1).all())
        assert int(self.pos) == r.pos and int(self.len) == r.pos + 1
        assert int(self.lengths) == (r.length if r.done else self.width)
        if nxt is not None:
            assert st[ops.SPEC_NDRAFT] == r.n_draft and self.tok.tolist() == nxt
            assert torch.equal(self.x, self.embed[self.tok]), "x rows are not the embedding rows of tok"
        else:
            assert self.tok.tolist() == tok_in
        return lg, want, was_done

    def agree(self, m, then, junk=7):
        """picks that confirm the first m draft tokens of the current tok, then pick `then`, then noise ids"""
        tok = self.tok.tolist()
        return (tok[1:m + 1] + [then] + [junk] * S)[:S]


@pytest.mark.parametrize("V", [4096, 1003])
def test_accept_emit_draft_and_counters(dev, V):
    d = _Dev(dev, V, width=64)
    ops = d.ops
    # the first token: one row of logits, no advance; it completes [100, 101] and the draft behind the first occurrence is 102 .. 108
    d.call(d.logits_for([101], 1), rows=1, advance=False)
    assert d.ref.n_draft == 7 and d.tok.tolist() == [101] + list(range(102, 109)) and d.ref.pos == 40 and d.ref.steps == 0
    # all accepted: the seven drafted tokens and the pick behind them
    d.call(d.logits_for(d.agree(7, 109), S))
    assert d.ref.out == list(range(101, 110)) and d.ref.pos == 48 and d.ref.accepted == 7 and d.ref.n_draft == 7
    # the first draft token wrong: the model's own pick alone; 555 occurs nowhere, so no draft follows and the rows repeat it
    d.call(d.logits_for(d.agree(0, 555), S))
    assert d.ref.pos == 49 and d.ref.accepted == 7 and d.ref.n_draft == 0 and d.tok.tolist() == [555] * S
    # n_draft = 0: rows 1 .. 7 are padding, whatever they pick
    d.call(d.logits_for([100] + [101] * 7, S))
    assert d.ref.out[-1] == 100 and d.ref.pos == 50 and d.ref.n_draft == 7 and d.ref.drafted == 14
    # a wrong draft in the middle: three confirmed, the fourth replaced by the pick
    d.call(d.logits_for(d.agree(3, 999), S))
    assert d.ref.out[-4:] == [101, 102, 103, 999] and d.ref.pos == 54 and d.ref.accepted == 10 and d.ref.steps == 4
    assert int(d.state[ops.SPEC_DONE]) == 0


@pytest.mark.parametrize("V", [4096, 1003])
def test_stop_id_inside_an_accepted_run_then_a_done_session(dev, V):
    d = _Dev(dev, V, width=64, stop=(777, 104))
    d.call(d.logits_for([101], 1), rows=1, advance=False)
    before_tok = d.tok.clone()
    d.call(d.logits_for(d.agree(7, 109), S))                    # 102, 103, 104 | 105 ... : cut after the stop id
    assert d.ref.done and d.ref.out == [101, 102, 103, 104] and d.ref.length == 4 and d.ref.pos == 43 and d.ref.accepted == 7
    assert torch.equal(d.tok, before_tok)
    # a step on the finished session: picks are taken (and the logits cleared on request), nothing else changes, bit for bit
    snap = d.snapshot()
    lg, _, was_done = d.call(d.logits_for(d.agree(2, 300), S), clear=True)
    assert was_done and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(snap, d.snapshot()))
    assert bool((lg[:, :V] == 0).all())


@pytest.mark.parametrize("V", [4096, 1003])
def test_cut_at_width(dev, V):
    d = _Dev(dev, V, width=6)
    d.call(d.logits_for([101], 1), rows=1, advance=False)
    d.call(d.logits_for(d.agree(7, 109), S))                    # eight confirmed picks, five slots left
    assert d.ref.done and d.ref.out == list(range(101, 107)) and d.ref.length == 6 and d.ref.pos == 45
    # a width the first token alone fills
    d1 = _Dev(dev, V, width=1)
    d1.call(d1.logits_for([101], 1), rows=1, advance=False)
    assert d1.ref.done and d1.ref.out == [101] and d1.ref.pos == 40


@pytest.mark.parametrize("V", [4096, 1003])
@pytest.mark.parametrize("clear", [False, True])
def test_ties_padding_columns_and_clear(dev, V, clear):
    d = _Dev(dev, V, width=64, ld=V + 14 if V % 8 else None)
    d.call(d.logits_for([101], 1), rows=1, advance=False)
    lg = d.logits_for(d.agree(7, 109), S)
    t = d.tok.tolist()
    lg[0, t[1]] = 5.0
    lg[0, t[1] + 50] = 5.0                                      # an exact tie: the lowest index wins
    lg[1, t[2]] = 5.0
    lg[1, t[2] + 9] = 5.0078125                                 # fp32-larger at a higher index, the same bf16 value: still the lowest
    lg[2, 3] = -7.0                                             # (the pick stays the crafted one)
    lg[:, V:] = 9.0                                             # columns V .. ld - 1 are never candidates
    lg0 = lg.clone()
    lg_dev, want, _ = d.call(lg, clear=clear)
    assert want[:3] == t[1:4] and d.ref.accepted == 7
    if clear:
        assert bool((lg_dev[:, :V] == 0).all()) and torch.equal(lg_dev[:, V:].cpu(), lg0[:, V:])
    else:
        assert torch.equal(lg_dev.cpu(), lg0)


def test_argument_checks(dev):
    from unigen_hip.lib import UniGenHipError
    d = _Dev(dev, 1003, width=8)
    ops = d.ops
    lg = d.logits_for([1] * S, S).to(dev)

    def call(**kw):
        a = dict(rows=S, ngram=G, num_draft=K, tok=d.tok)
        a.update(kw)
        ops.spec_verify_(lg, a["rows"], d.V, d.state, d.width, d.embed, a["tok"], d.out, d.x, d.hist, a["ngram"], a["num_draft"],
                         advance=(d.pos, d.len))
    for bad in (dict(rows=9), dict(rows=0), dict(ngram=5), dict(ngram=0), dict(num_draft=8), dict(tok=torch.zeros(9, dtype=torch.long, device=dev))):
        with pytest.raises(UniGenHipError, match="ug_spec_verify"):
            call(**bad)
    assert int(d.state[ops.SPEC_EMITTED]) == 0
