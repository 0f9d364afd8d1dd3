"""models.sampling.truncate_logits (the host form of the AR sampler's top-k / top-p / min-p rule) against the float64 restatement
in truncation_ref.py, on CPU.  Half of the rows are quantised so that equal values are common (ties at the thresholds are the point
where the value-threshold rule and a sorted cut differ)."""
import math

import pytest
import torch

import truncation_ref as ref

SETTINGS = [(50, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (200, 0.8, 0.02), (1, 1.0, 0.0), (0, 0.5, 0.0), (1000, 0.95, 0.0)]


def _logits(V, seed):
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(6, V, generator=g) * 1.25
    x[3:] = (x[3:] * 16).round() / 16                 # rows 3-5: a 1/16 grid, long runs of equal values
    return x


@pytest.mark.parametrize("V", [8192, 5000])
@pytest.mark.parametrize("case", range(len(SETTINGS)))
def test_truncate_logits_matches_float64_restatement(V, case):
    from models.sampling import top_k_top_p_filtering, truncate_logits
    top_k, top_p, min_p = SETTINGS[case]
    x = _logits(V, 100 + case)
    before = x.clone()
    out = truncate_logits(x, top_k=top_k, top_p=top_p, min_p=min_p)
    assert torch.equal(x, before) and out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    kept = out != ref.NEG
    assert torch.equal(out[kept], x[kept])
    compared = 0
    for b in range(x.shape[0]):
        v = x[b].double()
        t = ref.tau(v, top_k, top_p, min_p)
        assert torch.equal(kept[b], v >= t), (case, V, b)
        assert bool(kept[b][v.argmax()])
        if top_k:
            kth = ref.tau_top_k(v, top_k)
            n_gt, n_eq = int((v > kth).sum()), int((v == kth).sum())
            assert n_gt < top_k <= n_gt + n_eq
            if top_p == 1.0 and min_p == 0.0:
                assert int(kept[b].sum()) == n_gt + n_eq >= top_k
            if top_k == 1:
                assert torch.equal(kept[b], v == v.max())
        # the reference's sorted cut, in float64, plus min-p on top: the same set wherever it does not cut through equal values
        want = top_k_top_p_filtering(v.clone()[None], top_k=top_k, top_p=top_p)[0] != ref.NEG
        if min_p > 0.0:
            want &= v >= float(v.max()) + math.log(min_p)
        if int((v == v[kept[b]].min()).sum()) == 1 and int((v == v[want].min()).sum()) == 1:
            assert torch.equal(kept[b], want), (case, V, b)
            compared += 1
        else:
            assert bool((kept[b] | ~want).all())        # a run of equal values is kept whole: never fewer than the sorted cut
    assert compared >= 3, compared


def test_truncate_logits_off_and_argument_checks():
    from models.sampling import truncate_logits
    x = _logits(300, 7)
    assert torch.equal(truncate_logits(x), x)
    assert torch.equal(truncate_logits(x, top_k=300, top_p=1.0, min_p=0.0), x)
    assert int((truncate_logits(x, min_p=1.0) != ref.NEG).sum(-1).min()) >= 1
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": -0.1}, {"top_k": -1}):
        with pytest.raises(ValueError):
            truncate_logits(x, **kw)
