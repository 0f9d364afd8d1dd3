"""ug_maskgit_step_ex (csrc/sampler.hip: maskgit_sample_filtered_kernel, maskgit_sample_kernel<true>) through ops.maskgit_step and
UniGen.t2i_generate: the kept set, the draw, the log-probabilities and the re-masking of every masked position against the float64
restatements in truncation_ref.py / logprob_ref.py.

Kernel inputs are flat on purpose (0.5 * randn, guidance scale 2, sampling temperature 0.8): truncation then changes most draws, so the
unfiltered sampler fails.  Scale 2 is a power of two, so the mixed logit is exact in fp32 and the test reproduces it bit for bit.
Acceptance per masked position, no exclusions (D = 1e-5, truncation_ref.D; TOL = 1e-4, logprob_ref.TOL): the reported threshold lies
in the float64 bracket, the reported count is the size of {v >= tau}, the token is in that set and is a legitimate inverse-CDF draw
over it, both log-probabilities are within TOL of the restatement.  Re-masking is compared teacher-forced on the kernel's own tokens
wherever the float64 confidence is further than 1e-4 from the threshold; at most two positions per image may lie inside that band
(the holder of the threshold and one neighbour)."""
import math

import pytest
import torch

import logprob_ref as lref
import truncation_ref as ref
from helpers import additive, golden, llm_config_dir
from test_ar_sample_filtered_gpu import SETTINGS

pytestmark = pytest.mark.gpu

SCALE, TEMP, GUMBEL_T = 2.0, 0.8, 0.6
SENTINEL = -7.0

# (N, n, V, pad columns behind V, cfg, index into SETTINGS)
CASES = [(3, 64, V, 0, True, c) for V in (8192, 5000) for c in range(len(SETTINGS))]
CASES += [(3, 16, 20, 0, True, c) for c in range(len(SETTINGS))]          # fewer values than threads
CASES += [(3, 64, 5000, 3, True, c) for c in (1, 3)]                      # ld = V + 3: rows start on odd 2-byte addresses
CASES += [(3, 64, 5000, 0, False, c) for c in (1, 3)]                     # cfg off


def _inputs(N, n, V, cfg, case):
    g = torch.Generator().manual_seed(200 + case)
    rows = N * n
    logits = (0.5 * torch.randn((2 if cfg else 1) * rows, V, generator=g)).to(torch.bfloat16)
    u1, u2 = torch.rand(N, n, generator=g), torch.rand(N, n, generator=g)
    u1[0, 0] = 0.0
    u1[0, 1] = 1.0 - 2.0 ** -24
    mask_id = V + 7
    cur = torch.full((N, n), mask_id, dtype=torch.int64)
    known = torch.rand(N, n, generator=g) < 0.3
    known[0, :2] = False                                   # the two edge uniforms belong to masked positions
    cur[known] = torch.randint(0, V, (int(known.sum()),), generator=g)
    return logits, u1, u2, cur, known, mask_id


def _values(logits, rows, cfg, temp):
    """(v, c): the fp32 mixed value of every conditional row (as float64) and the conditional rows themselves"""
    lf = logits.float()
    c = lf[:rows]
    v = ref.mixed_logits(lf if cfg else torch.cat([c, c]), rows, SCALE, temp)       # (cfg off: u + 2 * (c - c) = c, exactly)
    return v.double(), c.double()


def _remask_reference(lp0, u2, known, sched):
    """float64 confidence, threshold and decision of the re-masking launch, teacher-forced on the kernel's own log-probabilities"""
    N, n = known.shape
    gum = -torch.log((-torch.log(u2.double().clamp(min=1e-20))).clamp(min=1e-20))
    conf = torch.where(known, torch.full((N, n), math.log(3.402823466e+38), dtype=torch.float64), lp0.double()) + GUMBEL_T * gum
    k = torch.clamp(torch.minimum((~known).sum(-1, keepdim=True) - 1, torch.tensor(sched)), min=1)
    thr = conf.sort(-1).values.gather(1, k)
    return conf, thr, conf < thr


@pytest.mark.parametrize("N,n,V,pad,cfg,case", CASES)
def test_maskgit_filtered_kernel_matches_restatement(dev, N, n, V, pad, cfg, case):
    from unigen_hip import ops
    top_k, top_p, min_p = SETTINGS[case]
    rows, off, sched = N * n, 300, n // 3
    logits, u1, u2, cur, known, mask_id = _inputs(N, n, V, cfg, case)
    v, c = _values(logits, rows, cfg, TEMP)
    wide = torch.full((logits.shape[0], V + pad), 30.0, dtype=torch.bfloat16, device=dev)      # (a read past V would win every draw)
    wide[:, :V] = logits.to(dev)
    lg_d = wide[:, :V]
    assert lg_d.stride(0) == V + pad
    res = []
    for _ in range(2):
        lp = torch.full((rows, 2), SENTINEL, device=dev)
        st = torch.full((rows, 2), SENTINEL, device=dev)
        out = ops.maskgit_step(lg_d, N, n, cfg, SCALE, u1.to(dev), u2.to(dev), cur.to(dev), mask_id, off, sched, GUMBEL_T,
                               want_masking=True, top_k=top_k, top_p=top_p, min_p=min_p, sample_temperature=TEMP, logp=lp, stats=st)
        res.append([t.cpu() for t in out] + [lp.cpu(), st.cpu()])
    for a, b in zip(*res):
        assert torch.equal(a, b)                                                                # bit-reproducible
    s, nc, ni, mk, lp, st = res[0]
    lp, st = lp.view(N, n, 2), st.view(N, n, 2)
    # known positions: token kept, never re-masked, outputs untouched
    assert torch.equal(s[known], cur[known]) and not bool((mk & known).any())
    assert bool((lp[known] == SENTINEL).all()) and bool((st[known] == SENTINEL).all())
    worst = [0.0, 0.0]
    for bi in torch.nonzero(~known.reshape(-1)).reshape(-1).tolist():
        b, i = divmod(bi, n)
        t, cnt, tok = float(st[b, i, 0]), int(st[b, i, 1]), int(s[b, i])
        lo, hi = ref.tau_bracket(v[bi], top_k, top_p, min_p)
        hi = max(hi, float(v[bi].min()))          # (every filter off -- top_k >= V alone: the bracket is -inf and the smallest kept value the row's minimum)
        assert lo <= t <= hi, (case, V, bi, t, lo, hi)
        assert cnt == int((v[bi] >= t).sum()) and cnt >= 1, (case, V, bi, cnt)
        assert 0 <= tok < V and bool(v[bi][tok] >= t), (case, V, bi, tok)
        assert ref.draw_ok(v[bi], t, tok, u1[b, i].double()), (case, V, bi, tok, float(u1[b, i]))
        e0 = abs(float(lp[b, i, 0]) - lref.kept_logprob(v[bi], tok, t))
        e1 = abs(float(lp[b, i, 1]) - lref.kept_logprob(c[bi], tok))
        worst = [max(worst[0], e0), max(worst[1], e1)]
        assert e0 <= lref.TOL and e1 <= lref.TOL, (case, V, bi, tok, e0, e1)
    # re-masking, teacher-forced on the kernel's own tokens and log-probabilities
    conf, thr, want_mask = _remask_reference(lp[..., 0], u2, known, sched)
    band = (conf - thr).abs() <= 1e-4
    print(f"case {case} V {V} pad {pad} cfg {cfg}: logp errors {worst[0]:.2e} / {worst[1]:.2e}, positions in the band per image "
          f"{band.sum(-1).tolist()}, kept counts {int(st[..., 1][~known].min())}..{int(st[..., 1][~known].max())}")
    assert int(band.sum(-1).max()) <= 2, band.sum(-1)
    assert torch.equal(mk[~band], want_mask[~band])
    assert torch.equal(nc, torch.where(mk, torch.tensor(mask_id), s)) and torch.equal(ni, torch.where(mk, torch.tensor(mask_id), s + off))
    assert int(mk.sum(-1).min()) >= 1


@pytest.mark.parametrize("N,n,V", [(3, 256, 8192), (2, 16, 20)])
def test_maskgit_logp_with_filters_off_is_the_parent_draw_bit_for_bit(dev, N, n, V):
    """filters off, sampling temperature 1: the launch with logp / stats returns the very tensors of the launch without, and logp is
    the untruncated restatement's"""
    from unigen_hip import ops
    g = torch.Generator().manual_seed(N * 1000 + n)
    rows = N * n
    logits = (2.0 * torch.randn(2 * rows, V, generator=g)).to(torch.bfloat16)
    u1, u2 = torch.rand(N, n, generator=g), torch.rand(N, n, generator=g)
    mask_id, off, scale, sched = V + 7, 300, 3.0, n // 3
    cur = torch.full((N, n), mask_id, dtype=torch.int64)
    known = torch.rand(N, n, generator=g) < 0.3
    cur[known] = torch.randint(0, V, (int(known.sum()),), generator=g)
    args = (logits.to(dev), N, n, True, scale, u1.to(dev), u2.to(dev), cur.to(dev), mask_id, off, sched, GUMBEL_T)
    plain = ops.maskgit_step(*args, want_masking=True)
    lp = torch.full((rows, 2), SENTINEL, device=dev)
    st = torch.full((rows, 2), SENTINEL, device=dev)
    for kw in ({"logp": lp}, {"logp": lp, "stats": st}, {"stats": st}, {"logp": lp, "top_k": V}):
        got = ops.maskgit_step(*args, want_masking=True, **kw)
        for a, b in zip(plain, got):
            assert torch.equal(a, b), kw
    s, lp, st = plain[0].cpu(), lp.cpu().view(N, n, 2), st.cpu().view(N, n, 2)
    assert bool((lp[known] == SENTINEL).all()) and bool((st[known] == SENTINEL).all())
    lf = logits.double()
    v, c = scale * (lf[:rows] - lf[rows:]) + lf[rows:], lf[:rows]
    worst = [0.0, 0.0]
    for bi in torch.nonzero(~known.reshape(-1)).reshape(-1).tolist():
        b, i = divmod(bi, n)
        tok = int(s[b, i])
        worst[0] = max(worst[0], abs(float(lp[b, i, 0]) - lref.kept_logprob(v[bi], tok)))
        worst[1] = max(worst[1], abs(float(lp[b, i, 1]) - lref.kept_logprob(c[bi], tok)))
        assert int(st[b, i, 1]) == V and abs(float(st[b, i, 0]) - float(v[bi].min())) <= 1e-5 * max(1.0, abs(float(v[bi].min())))
    print(f"N {N} n {n} V {V}: logp errors {worst[0]:.2e} / {worst[1]:.2e}")
    assert worst[0] <= lref.TOL and worst[1] <= lref.TOL


def test_maskgit_step_rejects_bad_filters(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    N, n, V = 2, 8, 64
    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)
    args = lambda V: (z(2 * N * n, V, dtype=torch.bfloat16), N, n, True, 2.0, z(N, n), z(N, n), torch.full((N, n), V + 7, device=dev), V + 7, 0,
                      2, GUMBEL_T)
    bad = [{"top_p": 0.0}, {"top_p": 1.5}, {"min_p": -0.1}, {"top_k": -1}, {"sample_temperature": 0.0}, {"logp": z(N * n, 3)},
           {"logp": z(N, n, 2)}, {"logp": z(N * n, 2, dtype=torch.float64)}, {"stats": z(N * n + 1, 2)}, {"logp": torch.zeros(N * n, 2)}]
    for kw in bad:
        with pytest.raises(UniGenHipError):
            ops.maskgit_step(*args(V), **kw)
    for kw in ({"top_k": 5}, {"sample_temperature": 0.8}):
        with pytest.raises(UniGenHipError, match="8192"):
            ops.maskgit_step(*args(8200), **kw)
    ops.maskgit_step(*args(8200), logp=z(N * n, 2))                    # filters off: the parent's kernel has no such limit
    torch.cuda.synchronize()


# ------------------------------------------------------------------ model level: the tiny golden model of tests/test_generate_gpu.py
def _model(g, dev, std=0.02):
    from models import UniGen
    from oracle import weights
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"], std=std), strict=False)
    return m.eval()


N_IMG, T_ROUNDS, V_IMG = 16, 4, 20
FILT = dict(top_k=5, top_p=0.8, sampling_temperature=0.7)


def _generate(model, g, dev, input_ids, gen, incremental, **kw):
    m, ids = g["maskgit"], g["ids"]
    return model.t2i_generate(input_ids=input_ids.to(dev), uncond_input_ids=m["uncond_ids"].to(dev), attention_mask=additive(m["mask_allow"]).to(dev),
                              guidance_scale=m["scale"], temperature=1.0, timesteps=T_ROUNDS, noise_schedule=lambda t: torch.cos(t * math.pi * 0.5),
                              generator=gen, image_token_num_per_image=N_IMG, text_vocab_size=ids["text_vocab"], incremental=incremental, **kw)


@pytest.mark.parametrize("incremental", [True, False])
def test_t2i_generate_default_tokens_do_not_depend_on_return_logprobs(dev, incremental):
    g = golden("g2_tiny_unigen.pt")
    model = _model(g, dev)
    ids0 = g["maskgit"]["input_ids"]
    for seed in (77, 78):
        plain = _generate(model, g, dev, ids0, torch.Generator(device=dev).manual_seed(seed), incremental)
        tok, lp, clp = _generate(model, g, dev, ids0, torch.Generator(device=dev).manual_seed(seed), incremental, return_logprobs=True)
        assert torch.equal(plain, tok)
        assert lp.shape == clp.shape == tok.shape and lp.dtype == clp.dtype == torch.float32 and lp.is_cuda
        assert bool((lp < 0).all()) and bool((clp < 0).all())                       # every position was masked: every entry written


@pytest.mark.parametrize("incremental", [True, False])
def test_t2i_generate_truncated_rounds_match_restatement(dev, incremental):
    """top_k 5, top_p 0.8, sampling temperature 0.7 on the tiny model (V = 20, n = 16, 4 rounds, CFG 2): every round restated in float64
    from that round's traced logits, the call's uniforms and the previous round's traced next_ids."""
    from unigen_hip.lib import UniGenHipError
    g = golden("g2_tiny_unigen.pt")
    model = _model(g, dev)
    m, ids = g["maskgit"], g["ids"]
    N, n, V, tv, mask_id = m["input_ids"].shape[0], N_IMG, V_IMG, ids["text_vocab"], ids["mask"]
    scale = float(m["scale"])
    off = 0 if model._use_gen() else tv                      # what t2i_generate adds to a drawn code to form next_ids
    assert scale == 2.0                                      # (a power of two: the fp32 mix is exact, as in the kernel test)
    known_in = m["input_ids"].clone()                        # the same prompt with 4 positions already known (raw codes, as cur_ids holds them)
    img0 = known_in.shape[1] - (n + 1)
    for b, i, code in ((0, 2, 3), (0, 9, 17), (1, 0, 5), (1, 15, 11)):
        known_in[b, img0 + i] = code
    differ = total = 0
    for input_ids in (m["input_ids"], known_in):
        for seed in (77, 78, 79):
            gen = torch.Generator(device=dev).manual_seed(seed)
            state = gen.get_state()
            u = torch.stack([torch.rand((2, N, n), device=dev, generator=gen) for _ in range(T_ROUNDS)]).cpu()      # [T, 2, N, n]
            gen.set_state(state)
            trace, lgs = [], []
            tok, lp, clp = _generate(model, g, dev, input_ids, gen, incremental, return_logprobs=True, trace=trace, logit_trace=lgs, **FILT)
            tok, lp, clp = tok.cpu(), lp.cpu(), clp.cpu()
            assert len(trace) == len(lgs) == T_ROUNDS and torch.equal(tok, trace[-1][0].cpu())
            cur = input_ids[:, -(n + 1):-1]
            want_lp, want_clp = torch.zeros(N, n, dtype=torch.float64), torch.zeros(N, n, dtype=torch.float64)
            for r in range(T_ROUNDS):
                lg = lgs[r].cpu()
                assert lg.dtype == torch.bfloat16 and lg.numel() == 2 * N * n * V
                lg = lg.reshape(2 * N * n, V)
                v = ref.mixed_logits(lg, N * n, scale, FILT["sampling_temperature"]).double()
                c = lg[:N * n].double()
                plain = (scale * (lg[:N * n].double() - lg[N * n:].double()) + lg[N * n:].double())        # the unfiltered rule's values
                s_r = trace[r][0].cpu()
                masked = cur == mask_id
                assert torch.equal(s_r[~masked], cur[~masked])
                for b, i in torch.nonzero(masked).tolist():
                    bi, t_ok = b * n + i, int(s_r[b, i])
                    tau = ref.tau(v[bi], FILT["top_k"], FILT["top_p"], 0.0)
                    assert 0 <= t_ok < V and bool(v[bi][t_ok] >= tau), (seed, r, b, i, t_ok)
                    assert ref.draw_ok(v[bi], tau, t_ok, u[r, 0, b, i].double()), (seed, r, b, i, t_ok)
                    want_lp[b, i] = lref.kept_logprob(v[bi], t_ok, tau)
                    want_clp[b, i] = lref.kept_logprob(c[bi], t_ok)
                    ex = torch.exp(plain[bi] - plain[bi].max())
                    cdf = ex.cumsum(0)
                    free = min(int((cdf <= u[r, 0, b, i].double() * cdf[-1]).sum()), V - 1)
                    differ += free != t_ok
                    total += 1
                nxt = trace[r][1].cpu()
                cur = torch.where(nxt == mask_id, nxt, nxt - off)
            err = max(float((lp.double() - want_lp).abs().max()), float((clp.double() - want_clp).abs().max()))
            print(f"incremental {incremental} seed {seed}: log-probability error {err:.2e}")
            assert err <= lref.TOL, (seed, err)
            first = input_ids[:, -(n + 1):-1] != mask_id
            assert int(first.sum()) in (0, 4) and bool((lp[first] == 0.0).all()) and bool((clp[first] == 0.0).all())
            assert torch.equal(tok[first], input_ids[:, -(n + 1):-1][first])
    print(f"incremental {incremental}: truncation changed {differ}/{total} = {differ / total:.3f} of the masked draws")
    assert 3 * differ >= total, (differ, total)
    with pytest.raises(UniGenHipError):
        _generate(model, g, dev, m["input_ids"], None, incremental, top_p=0.0)
