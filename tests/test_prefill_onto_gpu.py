"""Prefill onto a filled cache: Qwen2Engine.prefill_onto (engine) and UniGen.mmu_prefix / mmu_generate_batch(prefix=...) /
mmu_generate(prefix=...) (model).

Engine  the three-layer model at the 1.5B width of test_decode_parity_gpu.py (vocab 4096, the oracle bound to the same weights): one
        row of P positions is prefilled, broadcast to R rows, the rows' left-padded tails go onto it through prefill_onto, then four
        decode steps.  Oracle: lm.backbone stepped through its concatenating cache (prefix, tail at pos_offset = P under the causal-plus-
        validity mask, steps).  Returned hidden, every step's hidden and every layer's K / V rows at the tail's valid positions and at
        the appended positions, per row against fp32: ROW_BAR, or ROW_YARDSTICK x the oracle's own bf16 path (the rule of
        test_decode_parity_gpu.py, restated here).
Model   the tiny golden model (g2_tiny_unigen.pt): a prefix of 20 ids under the fixture's mmu mask (bidirectional image block), three
        tails of 10 / 6 / 8 ids left-padded to 10, greedy, 8 new tokens; mmu_generate_batch(prefix=...) row by row against the existing
        mmu_generate_batch on the assembled rows [prefix | pads | tail] under the dense masks of the same visibility.  Tokens must be
        equal up to the first step at which the CPU oracle's top-2 margin of that row is below MARGIN; every row must be compared over
        at least 4 of its 8 tokens.  SEED was chosen on the CPU from the oracle alone (oracle.qwen2_ref.mmu_generate_ref under bf16
        autocast on the assembled rows): of seeds 0 .. 79 it is the first at which all three rows keep a margin >= 0.2 for all 8
        steps under BOTH prefixes (first prefix: minima 0.23 / 0.46 / 0.62; second: 0.48 / 0.38 / 0.40) and row 0's tokens differ
        between the two prefixes (274 against 208), so a stale prefix row would show."""
import pytest
import torch

from helpers import additive, golden, llm_config_dir, oracle_lm

pytestmark = pytest.mark.gpu

# ====================================================================================== engine
TV, VOCAB = 2048, 4096
NV = VOCAB - 1 - TV
ROW_BAR, ROW_YARDSTICK = 1e-2, 1.5          # test_decode_parity_gpu.py: 1e-2, or 1.5 x the oracle's own bf16 path where that is larger
STEPS = 4
# name: (R, P, S, left pads in the prefix, pads per tail, seed)
ENGINE_CASES = {"p61": (4, 61, 9, 0, (0, 0, 3, 8), 11), "p125": (3, 125, 70, 5, (0, 1, 64), 12)}
P1 = 64                                     # chunking: prefill(P1) + prefill_onto(P - P1) against prefill(P), P = 125


@pytest.fixture(scope="module")
def m3(dev):
    """UniGen at the 1.5B width with THREE layers, vocab 4 096, seeded weights, and the oracle bound to the same tensors (as m3 of
    test_decode_parity_gpu.py)"""
    from models import UniGen
    from oracle import qwen2_ref, weights
    cfg = dict(qwen2_ref.QWEN25_1P5B, num_hidden_layers=3, vocab_size=VOCAB)
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TV, llm_model_path=llm_config_dir(cfg), codebook_size=NV,
                   num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=-1).eval()
    names = [(n, tuple(p.shape)) for n, p in model.llm.named_parameters()]
    sd = weights.synth_llm_state(names, seed=23)
    model.llm.load_state_dict(sd, strict=False)
    with torch.device("meta"):
        lm = qwen2_ref.RefCausalLM(qwen2_ref.Qwen2Cfg(**cfg))
    lm.load_state_dict(sd, strict=False, assign=True)
    lm.lm_head.weight = lm.model.embed_tokens.weight
    return model, lm


def _engine_inputs(name):
    R, P, S, pre_pads, tail_pads, seed = ENGINE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    prefix = 0.02 * torch.randn(1, P, 1536, generator=g)
    tails = 0.02 * torch.randn(R, S, 1536, generator=g)
    xs = [0.02 * torch.randn(R, 1536, generator=g) for _ in range(STEPS)]
    kv = torch.ones(R, P + S, dtype=torch.bool)
    kv[:, :pre_pads] = False
    for r in range(R):
        kv[r, P:P + tail_pads[r]] = False
    return prefix, tails, xs, kv


def _mask(allow):
    """additive mask of a boolean one, a row that sees nothing left open (it is a pad row: nothing reads it)"""
    mask = torch.where(allow, 0.0, float("-inf"))
    return torch.where(allow.any(-1, keepdim=True), mask, torch.zeros(()))


def _oracle_run(lm, name, autocast):
    """-> dict: prefix K / V [L][Hk, P, 128] and last hidden of the prefix alone, tail hidden [R, H], K / V of every layer [R, Hk, P+S+STEPS,
    128] at the end, every step's hidden; all fp32"""
    from oracle import qwen2_ref
    R, P, S = ENGINE_CASES[name][:3]
    prefix, tails, xs, kv = _engine_inputs(name)
    caches = [dict() for _ in lm.model.layers]
    out = {"steps": []}
    with torch.no_grad(), qwen2_ref.autocast_ctx(autocast):
        r = torch.arange(P)
        allow = (r[None, :] <= r[:, None])[None, None] & kv[:, None, None, :P]
        h = lm.backbone(inputs_embeds=prefix.expand(R, P, -1), mask=_mask(allow), caches=caches)
        out["prefix_h"] = h[0, -1].float()
        out["prefix_k"] = [c["k"][0].float() for c in caches]
        out["prefix_v"] = [c["v"][0].float() for c in caches]
        s = torch.arange(S)
        allow = (torch.arange(P + S)[None, :] <= (P + s)[:, None])[None, None] & kv[:, None, None, :]
        out["h"] = lm.backbone(inputs_embeds=tails, mask=_mask(allow), caches=caches, pos_offset=P)[:, -1].float()
        for i, x in enumerate(xs):
            allow = torch.ones(R, P + S + i + 1, dtype=torch.bool)
            allow[:, :P + S] = kv
            h = lm.backbone(inputs_embeds=x[:, None], mask=_mask(allow[:, None, None, :]), caches=caches, pos_offset=P + S + i)[:, -1]
            out["steps"].append(h.float())
        out["k"] = [c["k"].float() for c in caches]
        out["v"] = [c["v"].float() for c in caches]
    return out


_ORACLE = {}


def _oracle(lm, name):
    """fp32 (exact) and bf16-autocast (control) runs, once per case"""
    if name not in _ORACLE:
        _ORACLE[name] = (_oracle_run(lm, name, False), _oracle_run(lm, name, True))
    return _ORACLE[name]


def _row_errs(got, ref):
    a, b = got.reshape(got.shape[0], -1).double(), ref.reshape(ref.shape[0], -1).double()
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)


class _Rows:
    """collects the comparisons that fail: rows of `got` against fp32, each within max(ROW_BAR, ROW_YARDSTICK x the bf16 oracle's row)"""

    def __init__(self):
        self.failed, self.worst = [], 0.0

    def check(self, tag, got, r32, rbf):
        e, e_ref = _row_errs(got.float().cpu(), r32), _row_errs(rbf, r32)
        self.worst = max(self.worst, float((e / torch.clamp(ROW_YARDSTICK * e_ref, min=ROW_BAR)).max()))
        bad = (e > torch.clamp(ROW_YARDSTICK * e_ref, min=ROW_BAR)).nonzero().flatten().tolist()
        if bad:
            self.failed.append(f"{tag}: rows {bad[:8]} errors {[round(float(e[r]), 4) for r in bad[:8]]} vs the oracle bf16 path's "
                               f"{[round(float(e_ref[r]), 4) for r in bad[:8]]}")

    def done(self):
        print(f"    worst row at {self.worst:.2f} of its bar")
        assert not self.failed, f"{len(self.failed)} comparisons failed:\n" + "\n".join(self.failed[:16])


def _kv_rows(t, sel):
    """cache tensor [R, Hk, T, 128] -> the (row, position) pairs sel [R, T] marks, as rows [N, Hk * 128]"""
    return t.permute(0, 2, 1, 3)[sel.to(t.device)].reshape(int(sel.sum()), -1)


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_prefill_onto_and_decode_match_oracle(dev, m3, case):
    from unigen_hip.qwen2 import DecodeState
    model, lm = m3
    eng = model.llm.engine
    R, P, S = ENGINE_CASES[case][:3]
    prefix, tails, xs, kv = _engine_inputs(case)
    r32, rbf = _oracle(lm, case)
    nl = eng.dims.num_hidden_layers
    rows = _Rows()
    with torch.no_grad():
        st1 = DecodeState(eng.dims, 1, P, dev)
        eng.prefill(st1, prefix.to(dev), kv[:1, :P].to(dev))
        st = DecodeState(eng.dims, R, P + S + STEPS, dev, key_valid=kv)
        for l in range(nl):
            st.k[l][:, :, :P].copy_(st1.k[l])
            st.v[l][:, :, :P].copy_(st1.v[l])
        hn = eng.prefill_onto(st, tails.to(dev), P, kv.to(dev))
        assert (int(st.pos.item()), int(st.len.item())) == (P + S, P + S + 1)
        rows.check(f"{case} tail hidden", hn, r32["h"], rbf["h"])
        sel = torch.zeros(R, P + S + STEPS, dtype=torch.bool)
        sel[:, P:P + S] = kv[:, P:]
        x = torch.empty(R, 1536, device=dev)
        for i, xi in enumerate(xs):
            x.copy_(xi)
            hn = eng.decode_step(st, x)
            assert (int(st.pos.item()), int(st.len.item())) == (P + S + i + 1, P + S + i + 2)
            rows.check(f"{case} step {i + 1} hidden", hn, r32["steps"][i], rbf["steps"][i])
        sel[:, P + S:] = True
        for l in range(nl):
            for name, cache in (("k", st.k[l]), ("v", st.v[l])):
                rows.check(f"{case} layer {l} {name} rows at the tail's valid and the appended positions", _kv_rows(cache.float().cpu(), sel),
                           _kv_rows(r32[name][l], sel), _kv_rows(rbf[name][l], sel))
        eng.check_errors()
    rows.done()


def test_chunked_prefill_matches_whole_prefill(dev, m3):
    """prefill(64) + prefill_onto(61) against prefill(125): the same K / V rows and last hidden within the same bars (both against the
    fp32 oracle of the whole prefix, 5 left pads), and prefill_onto(st, x, 0) as a plain causal prefill"""
    from unigen_hip.qwen2 import DecodeState
    model, lm = m3
    eng = model.llm.engine
    P = ENGINE_CASES["p125"][1]
    prefix, _, _, kv = _engine_inputs("p125")
    r32, rbf = _oracle(lm, "p125")
    kv1 = kv[:1, :P]
    sel = kv1.clone()
    rows = _Rows()
    with torch.no_grad():
        whole, chunked, onto0 = (DecodeState(eng.dims, 1, P, dev) for _ in range(3))
        h_whole = eng.prefill(whole, prefix.to(dev), kv1.to(dev))
        eng.prefill(chunked, prefix[:, :P1].to(dev), kv1[:, :P1].to(dev))
        assert int(chunked.pos.item()) == P1
        h_chunked = eng.prefill_onto(chunked, prefix[:, P1:].to(dev), P1, kv1.to(dev))
        h_onto0 = eng.prefill_onto(onto0, prefix.to(dev), 0, kv1.to(dev))
        for tag, st, h in (("prefill(125)", whole, h_whole), ("prefill(64) + prefill_onto(61)", chunked, h_chunked),
                           ("prefill_onto(125) at 0", onto0, h_onto0)):
            assert (int(st.pos.item()), int(st.len.item())) == (P, P + 1), tag
            rows.check(f"{tag} last hidden", h, r32["prefix_h"][None], rbf["prefix_h"][None])
            for l in range(eng.dims.num_hidden_layers):
                for name, cache in (("k", st.k[l]), ("v", st.v[l])):
                    rows.check(f"{tag} layer {l} {name}", _kv_rows(cache.float().cpu(), sel), _kv_rows(r32[f"prefix_{name}"][l][None], sel),
                               _kv_rows(rbf[f"prefix_{name}"][l][None], sel))
        eng.check_errors()
    rows.done()


# ====================================================================================== model
MARGIN = 0.2
SEED = 6
PFX, S, NEW = 20, 10, 8
LENS = (10, 6, 8)


@pytest.fixture(scope="module")
def tiny(dev):
    from models import UniGen
    from oracle import weights
    g = golden("g2_tiny_unigen.pt")
    cfg, ids = g["cfg"], g["ids"]
    m = UniGen(w_und_encoder=False, vocab_size=cfg["vocab_size"], llm_vocab_size=ids["text_vocab"], llm_model_path=llm_config_dir(cfg),
               codebook_size=20, num_vq_tokens=16, load_from_pretrained=True, device=dev, init_seed=1)
    names = [(n, tuple(p.shape)) for n, p in m.llm.named_parameters()]
    m.llm.load_state_dict(weights.synth_llm_state(names, seed=g["weight_seed"]), strict=False)
    lm, _ = oracle_lm(cfg, g["weight_seed"])
    return m.eval(), lm, g


def _prefix_ids(g, which):
    """the mmu row of the fixture up to its end-of-image id (system, start of image, 16 image ids, end of image); which = 1: other
    image ids"""
    ids = g["input_ids"][-1, :PFX].clone()
    if which:
        ids[3:19] = torch.randint(312, 332, (16,), generator=torch.Generator().manual_seed(1000 + SEED))
    return ids


def _tails(g):
    gen = torch.Generator().manual_seed(SEED)
    t = torch.full((len(LENS), S), g["ids"]["pad"], dtype=torch.long)
    tv = torch.zeros(len(LENS), S, dtype=torch.bool)
    for r, n in enumerate(LENS):
        t[r, S - n:] = torch.randint(0, 290, (n,), generator=gen)
        tv[r, S - n:] = True
    return t, tv


def _assembled(g, pre, t, tv):
    """rows [prefix | pads | tail] and the dense masks of the same visibility: the prefix under its mmu mask, every later position
    causal over what the prefix mask's last row sees and the tail's real tokens (a pad row attends to itself: no empty rows)"""
    R, L = t.shape[0], PFX + S
    pre_allow = g["mask_allow"][-1, :PFX, :PFX]
    ids = torch.cat([pre[None].expand(R, PFX), t], 1)
    allow = torch.zeros(R, L, L, dtype=torch.bool)
    allow[:, :PFX, :PFX] = pre_allow
    kv = torch.cat([pre_allow[-1][None].expand(R, PFX), tv], 1)
    allow[:, PFX:, :] = torch.tril(torch.ones(L, L, dtype=torch.bool))[PFX:][None] & kv[:, None, :]
    i = torch.arange(PFX, L)
    allow[:, i, i] = True
    return ids, allow


_MARGINS = {}


def _compare_to(tiny, which):
    """-> per row, the number of leading steps at which the CPU oracle's top-2 margin stays >= MARGIN (tokens are compared there)"""
    if which not in _MARGINS:
        from oracle import qwen2_ref
        _, lm, g = tiny
        t, tv = _tails(g)
        ids, allow = _assembled(g, _prefix_ids(g, which), t, tv)
        ks = []
        for r in range(len(LENS)):
            _, margins = qwen2_ref.mmu_generate_ref(lm, idx=ids[r:r + 1], attention_mask=additive(allow[r:r + 1]), max_new_tokens=NEW)
            ks.append(next((i for i, m in enumerate(margins) if m < MARGIN), NEW))
        assert min(ks) >= NEW // 2, ks                    # the condition on SEED (module docstring)
        _MARGINS[which] = ks
    return _MARGINS[which]


def _same_up_to(got, want, ks):
    for r, k in enumerate(ks):
        a, b = [int(v) for v in got[r]][:k], [int(v) for v in want[r]][:k]
        assert a == b, (r, k, a, b)


def _setup(tiny, dev, which=0):
    model, _, g = tiny
    pre = _prefix_ids(g, which)
    t, tv = _tails(g)
    ids, allow = _assembled(g, pre, t, tv)
    pre_mask = additive(g["mask_allow"][-1:, :PFX, :PFX]).to(torch.float32).to(dev)
    prefix = model.mmu_prefix(idx=pre[None].to(dev), attention_mask=pre_mask)
    dense = dict(idx=ids.to(dev), attention_mask=additive(allow).to(torch.float32).to(dev))
    shared = dict(idx=t.to(dev), prefix=prefix, tail_valid=tv.to(dev))
    return prefix, dense, shared


@pytest.mark.parametrize("loop", ["host", "device_eager", "device_graph"])
def test_batch_with_prefix_matches_dense_rows(dev, tiny, loop):
    model = tiny[0]
    model.drop_decode_session()
    prefix, dense, shared = _setup(tiny, dev)
    assert prefix.P == PFX and prefix.capacity == 128 and prefix.ids is not None
    kw = dict(max_new_tokens=NEW, temperature=0.0, on_device=loop != "host", use_graph=loop == "device_graph")
    want = model.mmu_generate_batch(**dense, **kw)
    got = model.mmu_generate_batch(**shared, **kw)
    assert model.llm.engine.last_text_decode_on_device == (loop != "host")
    assert len(got) == len(LENS) and all(len(r) == NEW for r in got)
    _same_up_to(got, want, _compare_to(tiny, 0))
    model.drop_decode_session()
    assert prefix.P == PFX and prefix.st.k[0].shape[2] == 128        # drop_decode_session leaves the caller's prefix alone


def test_kept_session_takes_a_second_prefix(dev, tiny):
    """the captured session of a call with one prefix serves a call with another: no prefix row of the first survives"""
    model = tiny[0]
    eng = model.llm.engine
    model.drop_decode_session()
    kw = dict(max_new_tokens=NEW, temperature=0.0, on_device=True, use_graph=True)
    _, _, shared_a = _setup(tiny, dev, 0)
    _, dense_b, shared_b = _setup(tiny, dev, 1)
    model.mmu_generate_batch(**shared_a, **kw)
    sess, c0 = eng._text_session, getattr(eng, "text_graph_captures", 0)
    assert sess is not None and sess.graph is not None
    got = model.mmu_generate_batch(**shared_b, **kw)
    assert eng._text_session is sess and eng.text_graph_captures == c0           # replayed, not captured again
    model.drop_decode_session()
    want = model.mmu_generate_batch(**dense_b, **kw)
    _same_up_to(got, want, _compare_to(tiny, 1))
    model.drop_decode_session()


@pytest.mark.parametrize("on_device", [False, True])
def test_deterministic_calls_return_the_same_tokens_and_logprobs(dev, tiny, on_device):
    model = tiny[0]
    model.drop_decode_session()
    _, dense, shared = _setup(tiny, dev)
    kw = dict(max_new_tokens=NEW, temperature=0.0, on_device=on_device, deterministic=True, return_logprobs=True, repetition_penalty=1.3)
    (a, la), (b, lb) = model.mmu_generate_batch(**shared, **kw), model.mmu_generate_batch(**shared, **kw)
    assert model.llm.engine.last_decode_deterministic
    for r in range(len(LENS)):
        assert [int(v) for v in a[r]] == [int(v) for v in b[r]] and torch.equal(la[r], lb[r])
        assert la[r].shape == (len(a[r]),) and bool((la[r] <= 0).all())
    model.drop_decode_session()


def test_one_row_equals_mmu_generate_on_the_concatenated_prompt(dev, tiny):
    from unigen_hip.lib import UniGenHipError
    model = tiny[0]
    model.drop_decode_session()
    prefix, dense, shared = _setup(tiny, dev)
    k0 = _compare_to(tiny, 0)[:1]
    tail = shared["idx"][:1]                                                        # row 0: 10 ids, no pads
    want = model.mmu_generate(idx=dense["idx"][:1], attention_mask=dense["attention_mask"][:1], max_new_tokens=NEW, temperature=0.0)
    got = model.mmu_generate(idx=tail, prefix=prefix, max_new_tokens=NEW, temperature=0.0)
    assert len(got) == NEW
    _same_up_to([got], [want], k0)
    # the same continuation with 9 of the 10 ids appended to a copy of the prefix first (extend), the last one as the call's tail
    pre_mask = additive(tiny[2]["mask_allow"][-1:, :PFX, :PFX]).to(torch.float32).to(dev)
    grown = model.mmu_prefix(idx=prefix.ids, attention_mask=pre_mask, capacity=40)
    assert grown.extend(idx=tail[:, :9]) is grown and grown.P == PFX + 9 and grown.ids.shape == (1, PFX + 9)
    _same_up_to([model.mmu_generate(idx=tail[:, 9:], prefix=grown, max_new_tokens=NEW, temperature=0.0)], [want], k0)
    with pytest.raises(UniGenHipError, match="capacity"):
        grown.extend(idx=tail[:, :9].repeat(1, 2))                                 # 29 + 18 > 40
    assert grown.P == PFX + 9


def test_eot_token_cuts_rows_as_without_a_prefix(dev, tiny):
    model = tiny[0]
    model.drop_decode_session()
    _, _, shared = _setup(tiny, dev)
    for on_device in (False, True):
        kw = dict(max_new_tokens=NEW, temperature=0.0, on_device=on_device)
        full = [[int(v) for v in row] for row in model.mmu_generate_batch(**shared, **kw)]
        eot = full[1][3]
        cut = model.mmu_generate_batch(**shared, eot_token=eot, **kw)
        for r in range(len(LENS)):
            want = full[r][:full[r].index(eot) + 1] if eot in full[r] else full[r]
            assert [int(v) for v in cut[r]] == want[:len(cut[r])] and (eot not in want or len(cut[r]) == len(want)), (r, cut[r], want)
    model.drop_decode_session()


@pytest.mark.parametrize("prefix_as", ["ids", "embeddings"])
def test_repetition_penalty_sees_the_tail_ids_and_a_prefix_given_as_ids(dev, tiny, prefix_as):
    """every on-device token = the reference rule (tests/repetition_penalty_ref.py, as test_text_repetition_gpu.py applies it) on that
    step's traced raw logits and the row's history: the tail ids at their real positions, the prefix's ids only if it was given as ids"""
    import repetition_penalty_ref as ref
    model, _, g = tiny
    model.drop_decode_session()
    V, p = model.config.vocab_size, 1.3
    pre = _prefix_ids(g, 0)
    t, tv = _tails(g)
    pre_mask = additive(g["mask_allow"][-1:, :PFX, :PFX]).to(torch.float32).to(dev)
    if prefix_as == "ids":
        prefix = model.mmu_prefix(idx=pre[None].to(dev), attention_mask=pre_mask)
        ids, valid = torch.cat([pre[None].expand(len(LENS), PFX), t], 1), torch.cat([torch.ones(len(LENS), PFX, dtype=torch.bool), tv], 1)
    else:
        prefix = model.mmu_prefix(input_embeddings=model.llm.model.embed_tokens(pre[None].to(dev)), attention_mask=pre_mask)
        assert prefix.ids is None
        ids, valid = t, tv
    trace = []
    out = model.mmu_generate_batch(idx=t.to(dev), prefix=prefix, tail_valid=tv.to(dev), max_new_tokens=NEW, temperature=0.0, on_device=True,
                                   use_graph=False, trace=trace, repetition_penalty=p)
    tokens = torch.tensor([[int(v) for v in row] for row in out])
    assert tokens.shape == (len(LENS), NEW) and len(trace) == NEW
    bm = ref.Bitmap(len(LENS), V)
    bm.mark(ids, valid)
    for i, raw in enumerate(trace):
        want = ref.first_argmax(bm.penalize(raw.cpu(), p, tokens[:, i - 1].tolist() if i else None))
        assert tokens[:, i].tolist() == want.tolist(), (i, tokens[:, i].tolist(), want.tolist())
    model.drop_decode_session()
