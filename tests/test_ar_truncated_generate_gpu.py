"""UniGen.t2i_generate_ar with top_k / top_p / min_p on the tiny G9 model: the arguments, the uniforms' step indexing and the
prefill draw reach the fused sampler (every token of an eager run is checked against that step's traced logits and uniform with
the acceptance rule of tests/test_ar_sample_filtered_gpu.py); the captured and the kept-session runs give the eager run's tokens;
the filter constants are part of the session key; filters switched off change nothing; the unfused path applies the same rule."""
import pytest
import torch

import truncation_ref as ref
from helpers import golden, llm_config_dir

pytestmark = pytest.mark.gpu
MARGIN = 0.05          # the stop rule and value of tests/test_generate_gpu.py


def _model(g, dev, std=0.02):          # as tests/test_generate_gpu.py::_model
    from models import UniGen
    from oracle import weights
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=std), strict=False)
    return m.eval()


@pytest.fixture(scope="module")
def setup(dev):
    g = golden("g9_generate.pt")
    model = _model(g, dev, g["weight_std"])
    ar, tv = g["ar"], g["ids"]["text_vocab"]

    def run(seed=None, **kw):
        gen = None if seed is None else torch.Generator(device=dev).manual_seed(seed)
        return model.t2i_generate_ar(input_ids=ar["cond"].to(dev), uncond_input_ids=ar["uncond"].to(dev),
                                     attention_mask=ar["attention_mask"].to(dev), guidance_scale=ar["scale"], temperature=1.0,
                                     text_vocab_size=tv, image_token_num_per_image=ar["n"], generator=gen, **kw).cpu()
    return model, ar, run


def _mixed64(acc, bsz, scale):
    lf = acc.cpu().float().to(torch.bfloat16).double()
    return lf[bsz:] + scale * (lf[:bsz] - lf[bsz:])


def test_truncated_ar_generation_eager_graph_and_session(dev, setup, monkeypatch):
    model, ar, run = setup
    eng = model.llm.engine
    n, bsz = ar["n"], ar["cond"].shape[0]
    kw = dict(deterministic=True, top_k=3, top_p=0.7)
    trace = []
    eager = run(seed=11, use_graph=False, trace=trace, **kw)
    u = torch.rand((n, bsz), device=dev, generator=torch.Generator(device=dev).manual_seed(11)).cpu()
    assert len(trace) == n and eager.shape == (bsz, n)
    dropped = 0
    for i in range(n):
        v = _mixed64(trace[i], bsz, float(ar["scale"]))
        for b in range(bsz):
            lo, hi = ref.tau_bracket(v[b], 3, 0.7, 0.0)
            tok = int(eager[b, i])
            print(f"step {i} row {b}: token {tok}, u {float(u[i, b])!r}, tau in [{lo!r}, {hi!r}], kept {int((v[b] >= lo).sum())} of {v.shape[1]}")
            assert 0 <= tok < v.shape[1]
            assert ref.draw_ok(v[b], lo, tok, u[i, b].double()) or ref.draw_ok(v[b], hi, tok, u[i, b].double()), (i, b, tok)
            dropped += int((v[b] < lo).sum())
    assert dropped > 0                                  # the filters did cut something
    # the captured step, then the kept session
    first = run(seed=11, use_graph=True, **kw)
    sess = eng._ar_session
    assert sess is not None and eng.last_decode_graph
    second = run(seed=11, use_graph=True, **kw)
    assert eng._ar_session.graph is sess.graph
    assert torch.equal(first, eager) and torch.equal(second, eager)
    # another filter constant: a new graph, and back again gives what a fresh capture gives
    run(seed=11, use_graph=True, deterministic=True, top_k=4, top_p=0.7)
    s4 = eng._ar_session
    assert s4.graph is not sess.graph
    back = run(seed=11, use_graph=True, **kw)
    assert eng._ar_session.graph is not s4.graph
    kept = run(seed=11, use_graph=True, **kw)
    monkeypatch.setenv("UNIGEN_AR_GRAPH_CACHE", "0")
    fresh = run(seed=11, use_graph=True, **kw)
    monkeypatch.delenv("UNIGEN_AR_GRAPH_CACHE")
    assert torch.equal(back, fresh) and torch.equal(kept, fresh) and torch.equal(fresh, eager)
    model.drop_decode_session()


def test_filters_off_is_the_unfiltered_call(dev, setup):
    model, ar, run = setup
    plain = run(seed=5, deterministic=True)
    off = run(seed=5, deterministic=True, top_k=0, top_p=1.0, min_p=0.0)
    none = run(seed=5, deterministic=True, top_k=None, top_p=None, min_p=None)
    assert torch.equal(plain, off) and torch.equal(plain, none)
    model.drop_decode_session()


def test_unfused_path_applies_the_same_rule(dev, setup):
    """torch_sampler=True with top_k=1 keeps the argmax (and its ties) only, so the draw is the greedy token wherever the greedy
    run's own top-2 gap is above bf16 noise."""
    model, ar, run = setup
    n, bsz = ar["n"], ar["cond"].shape[0]
    trace = []
    run(use_graph=False, deterministic=True, greedy=True, trace=trace)
    gaps = torch.stack([_mixed64(t, bsz, float(ar["scale"])).topk(2, -1).values for t in trace], 1)      # [bsz, n, 2]
    gap = gaps[..., 0] - gaps[..., 1]
    want = run(use_graph=False, deterministic=True, greedy=True, torch_sampler=True)
    got = run(seed=3, use_graph=False, deterministic=True, top_k=1, torch_sampler=True)
    compared = 0
    for b in range(bsz):
        for i in range(n):
            if gap[b, i] < MARGIN:
                break
            assert int(got[b, i]) == int(want[b, i]), (b, i, got[b].tolist(), want[b].tolist())
            compared += 1
    print(f"unfused top_k=1 vs greedy: {compared}/{bsz * n} tokens compared, all equal")
    assert compared >= 24, compared


def test_out_of_range_filters_raise_before_any_launch(dev, setup):
    from unigen_hip.lib import UniGenHipError
    model, ar, run = setup
    for kw in ({"top_p": 0}, {"top_p": 1.5}, {"min_p": -0.1}, {"top_k": -1}):
        with pytest.raises(UniGenHipError):
            run(**kw)
