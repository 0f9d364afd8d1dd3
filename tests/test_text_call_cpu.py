"""The resolved description of a text generation call (models/unigen.py: text_call, generate_call, mmu_call -> TextCall): what the three
entry points used to work out on their way down, checked here without a GPU."""
import pytest
import torch

V = 100


def _vocab():
    return V


def _never():
    raise AssertionError("vocab was asked for although there is no id to check")


def _call(stop, **kw):
    from models.unigen import text_call
    return text_call("mmu_generate", _vocab, None, (None, None), stop, **kw)


STOP_FORMS = [(None, []), (7, [7]), ([3, 4], [3, 4]), ((3, 4), [3, 4]), (torch.tensor(5), [5]), (torch.tensor([5, 6]), [5, 6]), ([], [])]


@pytest.mark.parametrize("stop, ids", STOP_FORMS, ids=[str(i) for i in range(len(STOP_FORMS))])
def test_stop_ids_are_one_list_with_the_single_id_stop_sequences_merged_in_once(stop, ids):
    assert _call(stop).stop == ids and _call(stop, stop_sequences=[]).stop == ids
    # singles behind the caller's ids in the order given, the ones already there dropped; longer sequences stay sequences
    seqs = [[9], [4], [5], [7], [1, 2], [8]]
    want = ids + [e for e in (9, 4, 5, 7, 8) if e not in ids]
    call = _call(stop, stop_sequences=seqs)
    assert call.stop == want and len(set(call.stop)) == len(call.stop) and all(type(e) is int for e in call.stop)
    assert call.constraints["stop_seqs"] == [(1, 2)] and call.stops
    only_singles = _call(stop, stop_sequences=[[4], [9]])
    assert only_singles.stop == ids + [e for e in (4, 9) if e not in ids] and only_singles.constraints is None
    assert _call(stop).stops == bool(ids)


def test_mmu_generate_counts_a_stop_id_given_twice_once():
    from models.unigen import mmu_call
    call = mmu_call("mmu_generate", _vocab, 0.0, None, 5, stop_sequences=[[5]])
    assert call.stop == [5] and call.sampling is None


def test_the_host_loop_compares_with_what_each_entry_point_always_handed_it():
    """(the operand decides the compare kernel: a scalar, the caller's tensor, or a tensor of the list)"""
    from models.unigen import text_call
    t = torch.tensor([5, 6])
    assert _call(None).host_stop is None and _call(7).host_stop == 7 and _call(t).host_stop is t
    assert _call([3, 4]).host_stop == [3, 4] and _call(7, stop_sequences=[[9]]).host_stop == [7, 9]
    assert _call(None, logit_bias={1: 0.5}).host_stop == [] and _call(t, min_new_tokens=2).host_stop == [5, 6]
    gen = lambda stop, **kw: text_call("generate", _vocab, None, (None, None), stop, pad_finished=True, **kw).host_stop
    assert gen(None) is None and gen(7) == [7] and gen(None, logit_bias={1: 0.5}) is None
    assert gen(None, pad_token_id=0, stop_sequences=[[1, 2]]) == [] and gen(None, pad_token_id=0, stop_sequences=[[4]]) == [4]


def _generate_call(do_sample=False, temperature=1.0, top_k=None, top_p=None, eos_token_id=None, pad_token_id=None, generator=None,
                   deterministic=None, return_logprobs=False, vocab=_vocab, **kwargs):
    from models.unigen import generate_call
    return generate_call(vocab, do_sample, temperature, top_k, top_p, eos_token_id, pad_token_id, generator, deterministic, return_logprobs, kwargs)


def test_generate_pads_with_the_first_eos_id_unless_told_otherwise():
    call, n_ret = _generate_call(eos_token_id=[11, 12], stop_sequences=[[13]])
    assert (call.pad_token_id, call.stop, n_ret) == (11, [11, 12, 13], 1)
    assert _generate_call(eos_token_id=11)[0].pad_token_id == 11 and _generate_call(eos_token_id=11, pad_token_id=0)[0].pad_token_id == 0
    assert _generate_call()[0].pad_token_id is None and _generate_call(pad_token_id=3)[0].pad_token_id == 3
    # a stop sequence of one id is no eos id: it does not become the pad
    assert _generate_call(pad_token_id=3, stop_sequences=[[13]])[0].stop == [13]


def test_generate_refuses_stop_sequences_without_an_eos_or_a_pad_id():
    from unigen_hip.lib import UniGenHipError
    for seqs in ([[1, 2]], [[4]]):
        with pytest.raises(UniGenHipError, match="generate: stop_sequences need an eos_token_id or a pad_token_id"):
            _generate_call(stop_sequences=seqs)
        assert _generate_call(stop_sequences=seqs, pad_token_id=0)[0].stops and _generate_call(stop_sequences=seqs, eos_token_id=9)[0].stops


def test_generate_checks_num_return_sequences():
    from unigen_hip.lib import UniGenHipError
    for n in (0, -2):
        with pytest.raises(UniGenHipError, match=f"generate: num_return_sequences={n} must be at least 1"):
            _generate_call(num_return_sequences=n, do_sample=True)
    with pytest.raises(UniGenHipError, match="generate: num_return_sequences=3 needs do_sample=True"):
        _generate_call(num_return_sequences=3)
    assert _generate_call(num_return_sequences=3, do_sample=True)[1] == 3 and _generate_call(num_return_sequences=None)[1] == 1
    with pytest.raises(UniGenHipError, match="num_beams"):
        _generate_call(num_beams=4)


def test_the_sampling_constants_of_the_on_device_loop():
    from models.unigen import mmu_call
    assert _generate_call(do_sample=False, temperature=0.7, top_k=5)[0].sampling is None
    assert _generate_call(do_sample=True, temperature=None, top_k=None, top_p=None)[0].sampling == (1.0, 0, 1.0)
    assert _generate_call(do_sample=True, temperature=0.5, top_k=7, top_p=0.9)[0].sampling == (0.5, 7, 0.9)
    assert mmu_call("mmu_generate_batch", _vocab, 0.0, 50, None).sampling is None
    assert mmu_call("mmu_generate_batch", _vocab, 0.8, None, None).sampling == (0.8, 0, 1.0)
    assert mmu_call("mmu_generate_batch", _vocab, 0.8, 50, None).sampling == (0.8, 50, 1.0)


def test_vocab_is_asked_only_when_there_are_ids_to_check():
    from models.unigen import mmu_call
    _generate_call(vocab=_never, eos_token_id=[1, 2], pad_token_id=0, repetition_penalty=1.3, min_new_tokens=2, no_repeat_ngram_size=3,
                   do_sample=True, return_logprobs=True)
    mmu_call("mmu_generate", _never, 1.0, 5, torch.tensor([1, 2]), repetition_penalty=1.3, min_new_tokens=2, logit_bias={}, stop_sequences=[])
    for kw in (dict(logit_bias={1: 0.5}), dict(suppress_tokens=[1]), dict(stop_sequences=[[1]])):
        with pytest.raises(AssertionError, match="vocab was asked"):
            mmu_call("mmu_generate", _never, 1.0, 5, None, **kw)


@pytest.mark.parametrize("who", ["generate", "mmu_generate", "mmu_generate_batch"])
def test_error_messages_name_the_public_entry_point(who):
    from models.unigen import mmu_call
    from unigen_hip.lib import UniGenHipError
    build = (lambda **kw: _generate_call(eos_token_id=2, **kw)[0]) if who == "generate" else (lambda **kw: mmu_call(who, _vocab, 0.0, None, 2, **kw))
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf")), dict(logit_bias={V: 1.0}), dict(suppress_tokens=[4, 4]),
               dict(min_new_tokens=-1), dict(stop_sequences=[[]]), dict(logit_bias={3: float("nan")})):
        with pytest.raises(UniGenHipError, match=f"^{who}: "):
            build(**kw)
    assert build().who == who


def test_the_record_is_resolved_and_immutable():
    import dataclasses
    call, _ = _generate_call(eos_token_id=2, repetition_penalty=None, deterministic=True, return_logprobs=1, use_graph=0, trace=[])
    assert (call.penalty, call.deterministic, call.return_logprobs, call.use_graph, call.trace) == (1.0, True, True, False, [])
    assert _generate_call(deterministic=None)[0].deterministic == torch.are_deterministic_algorithms_enabled()
    assert _generate_call(repetition_penalty=1.3)[0].penalty == 1.3 and _generate_call()[0].use_graph is True
    with pytest.raises(dataclasses.FrozenInstanceError):
        call.penalty = 2.0


def test_the_builder_checks_the_constraints_exactly_once(monkeypatch):
    import models.unigen as mu
    counts = {"constraints": 0, "penalty": 0}
    real_c, real_p = mu.checked_constraints, mu.checked_repetition_penalty

    def counted_c(*a, **kw):
        counts["constraints"] += 1
        return real_c(*a, **kw)

    def counted_p(*a, **kw):
        counts["penalty"] += 1
        return real_p(*a, **kw)
    monkeypatch.setattr(mu, "checked_constraints", counted_c)
    monkeypatch.setattr(mu, "checked_repetition_penalty", counted_p)
    all_five = dict(logit_bias={3: 2.0}, suppress_tokens=[5], min_new_tokens=3, no_repeat_ngram_size=2, stop_sequences=[[21, 22], [9]])
    _generate_call(eos_token_id=2, repetition_penalty=1.3, **all_five)
    assert counts == {"constraints": 1, "penalty": 1}
    mu.mmu_call("mmu_generate", _vocab, 0.0, None, 2, repetition_penalty=1.3, **all_five)
    assert counts == {"constraints": 2, "penalty": 2}


def test_the_two_host_rules_stay_two():
    """generate's: temperature, top_k_top_p_filtering, multinomial with the caller's generator; the mmu one: temperature, the top-k
    threshold with ties kept, the default generator.  Greedy forms: the scores untouched, the lowest argmax."""
    from models.unigen import UniGen, generate_rule, mmu_rule
    s = torch.tensor([[0.5, 2.0, 2.0, -1.0, 1.0], [3.0, 0.0, 1.0, 3.0, -2.0]])
    for process, choose in (generate_rule(False, 0.5, 2, 0.5, None), mmu_rule(0.0, 2)):
        assert process(s) is s and choose(s).tolist() == [[1], [0]]
    process, choose = mmu_rule(0.5, 2)
    got = process(s.clone())
    assert torch.equal(got, UniGen._process_next(s.clone(), 0.5, 2)) and torch.equal(got[0], torch.tensor([float("-inf"), 4.0, 4.0, float("-inf"), float("-inf")]))
    torch.manual_seed(3)
    a = choose(got)
    torch.manual_seed(3)
    assert torch.equal(a, UniGen._choose_next(got, 0.5))
    g = torch.Generator().manual_seed(11)
    process, choose = generate_rule(True, 0.5, 3, 1.0, g)
    kept = process(s.clone())
    assert torch.equal(torch.isinf(kept), torch.tensor([[True, False, False, True, False], [False, True, False, False, True]]))
    assert torch.equal(kept[~torch.isinf(kept)], (s / 0.5)[~torch.isinf(kept)])
    a = choose(kept)
    want = torch.multinomial(torch.softmax(kept, dim=-1), num_samples=1, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a, want)
