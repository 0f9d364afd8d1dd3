"""ug_beam_kv_reorder on the GPU: positions [first, len) of every row become its parent's, in every layer's keys and values, exactly;
every other byte of every cache stays as it was (the whole cache when len == first); out-of-limit arguments are refused."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS, HKV, HD, TMAX = 3, 2, 128, 256


def _parents(R):
    """name -> parent rows (absolute), within groups of min(R, 4) beams"""
    B = min(R, 4)
    ident = list(range(R))
    swap = ident[:]
    swap[0], swap[1] = 1, 0
    out = {"identity": ident, "swap": swap, "all from beam 0": [r - r % B for r in range(R)]}
    if R >= 3:
        cyc = ident[:]
        cyc[0], cyc[1], cyc[2] = 1, 2, 0
        out["3-cycle"] = cyc
    g = torch.Generator().manual_seed(R)
    out["random within groups"] = [r - r % B + int(torch.randint(0, B, (1,), generator=g)) for r in range(R)]
    return out


def _state(dev, R):
    """a stand-in for DecodeState: caches of distinct bit patterns (every 16-bit word differs from its neighbours in row, head, position)"""
    g = torch.Generator().manual_seed(77 + R)
    mk = lambda: torch.randint(-32768, 32767, (R, HKV, TMAX, HD), generator=g, dtype=torch.int16).view(torch.bfloat16).to(dev)
    st = types.SimpleNamespace(k=[mk() for _ in range(LAYERS)], v=[mk() for _ in range(LAYERS)], len=torch.zeros(1, dtype=torch.int32, device=dev))
    return st


@pytest.mark.parametrize("R", [2, 8, 32])
def test_reorder_moves_exactly_the_generated_positions(dev, R):
    from unigen_hip import ops
    st = _state(dev, R)
    bits = lambda t: t.view(torch.int16)
    for first in (0, 37, 128):
        spare = ops.beam_kv_spare(st, 80)
        for extra in (0, 1, 70):
            for name, parent in _parents(R).items():
                before = [bits(t).clone() for t in st.k + st.v]
                st.len.fill_(first + extra)                              # set on the device: the host never reads it
                p = torch.tensor(parent, dtype=torch.int32, device=dev)
                ops.beam_kv_reorder(st, p, first, spare)
                for old, new in zip(before, st.k + st.v):
                    want = old.clone()
                    want[:, :, first:first + extra] = old[p.long()][:, :, first:first + extra]
                    assert torch.equal(bits(new), want), (R, first, extra, name)
    # a length beyond the spare's span moves the span only; the pointer tables are built once per state
    st.len.fill_(200)
    spare = ops.beam_kv_spare(st, 16)
    before = [bits(t).clone() for t in st.k + st.v]
    tables = st._beam_kv_tables
    p = torch.tensor(_parents(R)["swap"], dtype=torch.int32, device=dev)
    ops.beam_kv_reorder(st, p, 100, spare)
    assert st._beam_kv_tables is tables
    for old, new in zip(before, st.k + st.v):
        want = old.clone()
        want[:, :, 100:116] = old[p.long()][:, :, 100:116]
        assert torch.equal(bits(new), want)


def test_reorder_refuses_what_is_outside_its_limits(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    st = _state(dev, 2)
    p = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    spare = ops.beam_kv_spare(st, 80)
    before = [t.clone() for t in st.k + st.v]
    st.len.fill_(250)
    with pytest.raises(UniGenHipError, match="first \\+ span <= Tmax"):
        ops.beam_kv_reorder(st, p, 200, spare)                            # 200 + 80 > 256
    with pytest.raises(UniGenHipError, match="first >= 0"):
        ops.beam_kv_reorder(st, p, -1, spare)
    with pytest.raises(UniGenHipError, match="int32 parent"):
        ops.beam_kv_reorder(st, p.long(), 0, spare)
    with pytest.raises(UniGenHipError, match="spare"):
        ops.beam_kv_reorder(st, p, 0, spare[:, :, :1])
    half = types.SimpleNamespace(k=[t[..., :64].contiguous() for t in st.k], v=[t[..., :64].contiguous() for t in st.v], len=st.len)
    with pytest.raises(UniGenHipError, match="head_dim must be 128"):
        ops.beam_kv_reorder(half, p, 0, ops.beam_kv_spare(half, 8))
    for old, new in zip(before, st.k + st.v):
        assert torch.equal(old.view(torch.int16), new.view(torch.int16))
