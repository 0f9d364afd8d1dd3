"""Host logic of the on-device text loop's switch (UniGen._text_on_device, UniGen._stop_list): no GPU needed."""
import types

import pytest
import torch


def _fake(hidden=1536, default=False):
    from models.unigen import UniGen
    eng = types.SimpleNamespace(dims=types.SimpleNamespace(hidden_size=hidden))
    fake = types.SimpleNamespace(text_decode_on_device=default, llm=types.SimpleNamespace(engine=eng), _stop_list=UniGen._stop_list)

    def on_device(flag, who, rows, cached, stop, new):          # (the switch reads the stop ids off the call's record)
        from models.unigen import text_call
        return UniGen._text_on_device(fake, flag, text_call(who, lambda: 1000, None, (None, None), stop), rows, cached, new)
    return on_device


def test_stop_list_normalises_every_form_the_callers_pass():
    from models.unigen import UniGen
    assert UniGen._stop_list(None) == [] and UniGen._stop_list(7) == [7] and UniGen._stop_list([3, 4]) == [3, 4]
    assert UniGen._stop_list(torch.tensor(5)) == [5] and UniGen._stop_list(torch.tensor([5, 6])) == [5, 6]


def test_explicit_bool_wins_and_only_an_explicit_true_raises():
    from unigen_hip.lib import UniGenHipError
    off, on = _fake(default=False), _fake(default=True)
    assert off(None, "generate", 3, True, [], 8) is False and on(None, "generate", 3, True, [], 8) is True
    assert off(True, "generate", 3, True, [1], 8) is True and on(False, "generate", 3, True, [1], 8) is False
    cases = [(33, True, [], 8, "33 rows"), (3, False, [], 8, "use_cache"), (3, True, list(range(9)), 8, "9 stop ids"), (3, True, [], 0, "max_new_tokens")]
    for rows, cached, stop, new, word in cases:
        assert on(None, "generate", rows, cached, stop, new) is False          # default-derived: the host loop
        with pytest.raises(UniGenHipError, match=word):
            off(True, "generate", rows, cached, stop, new)
    with pytest.raises(UniGenHipError, match="hidden size 200"):
        _fake(hidden=200)(True, "mmu_generate", 1, True, None, 4)
    assert _fake(hidden=200, default=True)(None, "mmu_generate", 1, True, None, 4) is False
