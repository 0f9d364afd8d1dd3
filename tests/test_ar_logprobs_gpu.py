"""Per-token log-probabilities of AR image generation: ug_ar_sample_logp / ug_ar_sample_filtered_logp (csrc/sampler.hip) through
ops.ar_sample_(..., logp=) / ops.ar_sample_filtered_(..., logp=), and UniGen.t2i_generate_ar(return_logprobs=True) on the tiny G9
model, against the float64 restatement in logprob_ref.py.

Tolerance TOL = 1e-4 absolute on every log-probability, for inputs with |v - max| < 64 (logprob_ref.TOL; the text tests use it too).
A log-probability is (v[tok] - max) - log(sum of exp(v[e] - max)):
  * one rounding for v - max: half an ulp of a value below 64, at most 2^-19 = 1.9e-6;
  * the relative error of the sum: one rounding per addition in the kernel's fixed order plus ~1 ulp of expf per term (whose argument
    carries the rounding above).  The AR samplers add a chunk of at most 8 entries in index order, then 6 levels over the wave, then
    the 16 wave partials: 30 roundings, 1.8e-6.  The text selection launch counts 77 * 2^-24 = 4.6e-6 (tests/test_text_sample_gpu.py).
    The longest chain is the greedy text pick's: ceil(159 867 / 1024) = 157 additions per thread, each behind an expf, a rescaling
    product whenever the thread's running maximum moves and once more onto the row's maximum, then 6 + 4 merge levels: about
    (157 + 10 + 3) * 2^-24 = 1.0e-5.  A relative error of the sum is an absolute error of its logarithm;
  * logf and the final subtraction: about 2e-6 each (half an ulp of a value below 16 is 4.8e-7; logf is good to ~1 ulp).
Roughly 2e-5 in the worst case, so 1e-4 carries a five-fold margin; the conditional log-softmax adds one product per thread (its sum
rescaled to the block maximum) to the first chain and stays under the same count.

The kernel tests also hold the new entry points to the old ones bit for bit on everything the old ones write."""
import pytest
import torch

import logprob_ref as lref
import truncation_ref as ref
from helpers import golden, llm_config_dir

pytestmark = pytest.mark.gpu

TOL = lref.TOL
SCALE, TEMP = 2.0, 0.8          # (a power-of-two scale: the mixed logit is exact in fp32 and the restatement reproduces it bit for bit)
SETTINGS = {"draw": None, "greedy": "greedy", "k50_p0.9_m0.05": (50, 0.9, 0.05), "p0.5": (0, 0.5, 0.0)}


def _inputs(V, seed):
    bsz, H, n, off = 3, 64, 3, 100
    g = torch.Generator().manual_seed(seed)
    acc = 0.5 * torch.randn(n, 2 * bsz, V, generator=g)
    acc[:, 1, 100:108] = 3.0                                     # row 1: a run of equal maxima, in the conditional row and in the mix
    acc[:, bsz + 1, 100:108] = 1.0
    emb = torch.randn(off + V, H, generator=g)
    u = torch.rand(n, bsz, generator=g)
    u[0, 0] = 0.0
    u[1, 0] = 1.0 - 2.0 ** -24
    u[2, 1] = 0.0
    return bsz, H, n, off, acc, emb, u


@pytest.mark.parametrize("V", [8192, 5000, 1000])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_ar_sampler_logp_entries_match_restatement_and_the_old_entries(dev, V, setting):
    from unigen_hip import ops
    filt = SETTINGS[setting]
    greedy = filt == "greedy"
    filtered = isinstance(filt, tuple)
    bsz, H, n, off, acc, emb, u = _inputs(V, 300 + list(SETTINGS).index(setting))
    P = 40
    emb_d, u_d = emb.to(dev), u.to(dev)

    def run(with_logp):
        acc_d = torch.zeros(2 * bsz, V, device=dev)              # one accumulator: refilled per step, cleared by the sampler
        tok = torch.zeros(bsz, 1, dtype=torch.long, device=dev)
        out = torch.full((bsz, n), -1, dtype=torch.int32, device=dev)
        x = torch.zeros(2 * bsz, H, device=dev)
        logp = torch.full((bsz, n, 2), 7.0, device=dev) if with_logp else None
        steps = []
        for step in range(n):
            acc_d.copy_(acc[step])
            pos = torch.tensor([P + step], dtype=torch.int32).to(dev)
            stats = torch.full((bsz, 2), -1.0, device=dev)
            if filtered:
                ops.ar_sample_filtered_(acc_d, bsz, V, SCALE, TEMP, False, u_d, pos, P, n, emb_d, off, tok, out, x,
                                        top_k=filt[0], top_p=filt[1], min_p=filt[2], stats=stats, logp=logp)
            else:
                ops.ar_sample_(acc_d, bsz, V, SCALE, TEMP, greedy, None if greedy else u_d, pos, P, n, emb_d, off, tok, out, x, logp=logp)
            steps.append((tok.cpu().clone(), x.cpu().clone(), acc_d.cpu().clone(), stats.cpu()))
        return steps, out.cpu(), None if logp is None else logp.cpu()

    old, new, again = run(False), run(True), run(True)
    assert torch.equal(old[1], new[1])
    for step in range(n):
        for a, b_, c in zip(old[0][step], new[0][step], again[0][step]):
            assert torch.equal(a, b_) and torch.equal(a, c)                       # tokens, x, the cleared accumulator, stats: bit-equal
        assert float(new[0][step][2].abs().max()) == 0.0
    logp = new[2]
    assert torch.equal(logp, again[2])                                           # bit-reproducible
    assert bool((logp <= 0).all())
    worst = 0.0
    for step in range(n):
        v = ref.mixed_logits(acc[step], bsz, SCALE, TEMP)
        cv = lref.cond_values(acc[step], bsz)
        tok, stats = new[0][step][0][:, 0], new[0][step][3]
        for b in range(bsz):
            tau = float(stats[b, 0]) if filtered else lref.NEG
            want = lref.kept_logprob(v[b], int(tok[b]), tau)
            want_c = lref.kept_logprob(cv[b], int(tok[b]))
            got, got_c = float(logp[b, step, 0]), float(logp[b, step, 1])
            print(f"{setting} V {V} step {step} row {b}: token {int(tok[b])}, logprob {got!r} (float64 {want!r}, diff {abs(got - want):.2e}), "
                  f"cond {got_c!r} (float64 {want_c!r}, diff {abs(got_c - want_c):.2e}), max - v[tok] {float(v[b].max() - v[b][tok[b]]):.3f}")
            assert float(v[b].max() - v[b].min()) < 64
            assert abs(got - want) <= TOL, (setting, V, step, b, got, want)
            assert abs(got_c - want_c) <= TOL, (setting, V, step, b, got_c, want_c)
            worst = max(worst, abs(got - want), abs(got_c - want_c))
    print(f"{setting} V {V}: worst difference {worst:.2e}")
    if greedy:
        assert int(new[0][0][0][1, 0]) == 100                                    # the lowest index of the run of maxima


def test_ar_sampler_logp_entries_reject_a_null_output_and_a_wide_slice(dev):
    from unigen_hip import lib, ops
    from unigen_hip.lib import UniGenHipError
    bsz, V, H, n, P = 2, 64, 64, 4, 8
    acc = torch.ones(2 * bsz, V, device=dev)
    emb = torch.zeros(V, H, device=dev)
    u = torch.zeros(n, bsz, device=dev)
    pos = torch.tensor([P], dtype=torch.int32, device=dev)
    tok = torch.zeros(bsz, 1, dtype=torch.long, device=dev)
    out = torch.zeros(bsz, n, dtype=torch.int32, device=dev)
    x = torch.zeros(2 * bsz, H, device=dev)
    p = ops._p
    args = (p(acc), acc.stride(0), bsz, V, 1.0, 1.0, 0, p(u), p(pos), P, n, p(emb), emb.stride(0), H, 0, p(tok), p(out), p(x))
    L = lib.load()
    with pytest.raises(UniGenHipError, match="null logp"):
        lib.check(L.ug_ar_sample_logp(*args, None, ops._stream()), "ug_ar_sample_logp")
    with pytest.raises(UniGenHipError, match="null logp"):
        lib.check(L.ug_ar_sample_filtered_logp(*args, 5, 0.9, 0.0, None, None, ops._stream()), "ug_ar_sample_filtered_logp")
    wide = torch.ones(2 * bsz, 8200, device=dev)
    wemb = torch.zeros(8200, H, device=dev)
    logp = torch.zeros(bsz, n, 2, device=dev)
    with pytest.raises(UniGenHipError, match="exceeds"):
        ops.ar_sample_(wide, bsz, 8200, 1.0, 1.0, False, u, pos, P, n, wemb, 0, tok, out, x, logp=logp)
    with pytest.raises(UniGenHipError, match="exceeds"):
        ops.ar_sample_filtered_(wide, bsz, 8200, 1.0, 1.0, False, u, pos, P, n, wemb, 0, tok, out, x, top_k=5, logp=logp)
    with pytest.raises(UniGenHipError, match="shape"):                           # a buffer the kernel would overrun
        ops.ar_sample_(acc, bsz, V, 1.0, 1.0, False, u, pos, P, n, emb, 0, tok, out, x, logp=torch.zeros(bsz, n, device=dev))
    torch.cuda.synchronize()
    assert float(acc.min()) == 1.0 and float(wide.min()) == 1.0 and int(out.abs().sum()) == 0      # a refused call launches nothing


# ------------------------------------------------------------------ model level: the tiny G9 model (tests/test_ar_truncated_generate_gpu.py)
def _model(g, dev, std=0.02):
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
                                     text_vocab_size=tv, image_token_num_per_image=ar["n"], generator=gen, **kw)
    return model, ar, run


def _mixed64(acc, bsz, scale):
    lf = acc.cpu().float().to(torch.bfloat16).double()
    return lf[bsz:] + scale * (lf[:bsz] - lf[bsz:])


def _check_against_trace(trace, tokens, logprobs, cond_logprobs, bsz, scale, filt, tag):
    """every entry against the restatement on that step's traced logits (conditional rows first).  The temperature is 1 and the mixed
    logit is taken in float64 from the bf16 rows: the kernel's fp32 mix (one or two roundings of values below 8, 5e-7 each) stays far
    inside TOL.  With filters: the restatement at either end of truncation_ref.tau_bracket."""
    tokens, logprobs, cond_logprobs = tokens.cpu(), logprobs.cpu(), cond_logprobs.cpu()
    n = tokens.shape[1]
    assert len(trace) == n and logprobs.shape == tokens.shape == cond_logprobs.shape
    assert logprobs.dtype == torch.float32 and cond_logprobs.dtype == torch.float32
    for i in range(n):
        v = _mixed64(trace[i], bsz, scale)
        cv = trace[i].cpu().float().to(torch.bfloat16).double()[:bsz]
        for b in range(bsz):
            tok = int(tokens[b, i])
            taus = (lref.NEG,) if filt is None else ref.tau_bracket(v[b], *filt)
            wants = [lref.kept_logprob(v[b], tok, t) for t in taus if bool(v[b][tok] >= t)]
            want_c = lref.kept_logprob(cv[b], tok)
            got, got_c = float(logprobs[b, i]), float(cond_logprobs[b, i])
            print(f"{tag} step {i} row {b}: token {tok}, logprob {got!r} (float64 {wants!r}), cond {got_c!r} (float64 {want_c!r})")
            assert wants and min(abs(got - w) for w in wants) <= TOL, (tag, i, b, got, wants)
            assert abs(got_c - want_c) <= TOL, (tag, i, b, got_c, want_c)
            assert got <= 0.0 and got_c <= 0.0


@pytest.mark.parametrize("mode", ["draw", "greedy", "top_k3_top_p0.7"])
def test_ar_generation_logprobs_eager_graph_and_session(dev, setup, mode):
    model, ar, run = setup
    eng = model.llm.engine
    n, bsz, scale = ar["n"], ar["cond"].shape[0], float(ar["scale"])
    kw = {"draw": {}, "greedy": {"greedy": True}, "top_k3_top_p0.7": {"top_k": 3, "top_p": 0.7}}[mode]
    filt = (3, 0.7, 0.0) if "top_k" in kw else None
    kw = dict(kw, deterministic=True)
    model.drop_decode_session()
    plain = run(seed=11, use_graph=False, **kw)
    assert torch.is_tensor(plain)
    trace = []
    tokens, lp, clp = run(seed=11, use_graph=False, trace=trace, return_logprobs=True, **kw)
    assert torch.equal(tokens, plain) and tokens.shape == (bsz, n) and lp.is_cuda and clp.is_cuda
    _check_against_trace(trace, tokens, lp, clp, bsz, scale, filt, mode)
    # the captured step, then the kept session: the eager run's bits
    first = run(seed=11, use_graph=True, return_logprobs=True, **kw)
    sess = eng._ar_session
    assert sess is not None and eng.last_decode_graph and sess.key[-1] == "logprobs"
    second = run(seed=11, use_graph=True, return_logprobs=True, **kw)
    assert eng._ar_session.graph is sess.graph
    for got in (first, second):
        assert torch.equal(got[0], tokens) and torch.equal(got[1], lp) and torch.equal(got[2], clp)
    assert second[1].data_ptr() != eng._ar_session.logp.data_ptr()            # clones: the next call overwrites the session's buffer
    # a flag-off call in between takes no part in the flag-on session, and the next flag-on call still returns the same bits
    off = run(seed=11, use_graph=True, **kw)
    s_off = eng._ar_session
    assert torch.is_tensor(off) and torch.equal(off, tokens)
    assert s_off.graph is not sess.graph and s_off.logp is None and s_off.key == sess.key[:-1]
    third = run(seed=11, use_graph=True, return_logprobs=True, **kw)
    assert eng._ar_session.graph is not s_off.graph
    assert torch.equal(third[0], tokens) and torch.equal(third[1], lp) and torch.equal(third[2], clp)
    model.drop_decode_session()


@pytest.mark.parametrize("mode", ["draw", "greedy", "top_k3_top_p0.7"])
def test_unfused_ar_path_returns_the_same_quantities(dev, setup, mode):
    """torch_sampler=True: models/sampling.py: token_logprobs on the scores torch.multinomial draws from, checked on the unfused
    branch's own traced head rows (bf16 head output, conditional rows first)"""
    model, ar, run = setup
    n, bsz, scale = ar["n"], ar["cond"].shape[0], float(ar["scale"])
    kw = {"draw": {}, "greedy": {"greedy": True}, "top_k3_top_p0.7": {"top_k": 3, "top_p": 0.7}}[mode]
    filt = (3, 0.7, 0.0) if "top_k" in kw else None
    trace = []
    plain = run(seed=4, use_graph=False, deterministic=True, torch_sampler=True, **kw)
    tokens, lp, clp = run(seed=4, use_graph=False, deterministic=True, torch_sampler=True, trace=trace, return_logprobs=True, **kw)
    assert torch.equal(tokens, plain)
    _check_against_trace(trace, tokens, lp, clp, bsz, scale, filt, "unfused " + mode)
