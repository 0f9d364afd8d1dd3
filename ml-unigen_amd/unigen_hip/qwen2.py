"""Qwen2.5 backbone engine on the gfx950 kernels: flat parameter storage, decoder-stack forward /
backward, tied lm_head + cross-entropy.  This is the arithmetic behind `UniGen.llm`
(reference: models/unigen.py:56-69 builds transformers' Qwen2ForCausalLM; call sites :274-287).

Memory plan (sized for 288 GB HBM3E, no activation recompute):
  * ONE flat fp32 buffer holds every parameter (q/k/v and gate/up stored fused so one GEMM serves
    each), ONE flat fp32 gradient buffer mirrors it (this is also what the data-parallel
    all-reduce moves), ONE flat bf16 compute copy plus per-matrix transposed bf16 copies feed the
    matrix cores.  `nn.Parameter`s with the reference checkpoint's names are views into the flat
    buffers, so optimizers / state_dict / named_parameters() see the reference layout.
  * precision = the reference's accelerate-DDP bf16-autocast mode: fp32 master weights and residual
    stream, bf16 GEMM operands, fp32 accumulation / statistics / gradients.
"""
import math
import os

import types

import torch
import torch.nn as nn

from . import ops
from .lib import UniGenHipError


class Qwen2Dims:
    def __init__(self, vocab_size, hidden_size=1536, intermediate_size=8960, num_hidden_layers=28,
                 num_attention_heads=12, num_key_value_heads=2, rope_theta=1e6, rms_norm_eps=1e-6,
                 initializer_range=0.02, rope_scaling=None, max_position_embeddings=32768, **_unused):
        self.vocab_size = int(vocab_size)
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.num_key_value_heads = num_key_value_heads
        self.head_dim = hidden_size // num_attention_heads
        self.rope_theta = float(rope_theta)
        self.rope_scaling = None
        if rope_scaling:
            self.rope_scaling = dict(rope_scaling, max_position_embeddings=int(max_position_embeddings))
        self.rms_norm_eps = float(rms_norm_eps)
        self.initializer_range = initializer_range
        if self.head_dim != 128:
            raise UniGenHipError(f"attention kernels are specialised for head_dim 128 (got {self.head_dim})")
        if hidden_size % 64 or intermediate_size % 64:
            raise UniGenHipError("hidden / intermediate sizes must be multiples of 64 for the MFMA GEMM")
        self.vocab_pad = ops.round_up(self.vocab_size, 64)
        self.qkv_out = (num_attention_heads + 2 * num_key_value_heads) * self.head_dim


class FlatParams:
    """Flat fp32 master / grad buffers + bf16 compute copies, with named views."""

    ALIGN = 64

    def __init__(self, dims, device):
        d, self.dims, self.device = dims, dims, device
        H, I = d.hidden_size, d.intermediate_size
        self.spec = []   # (key, shape)
        self.spec.append(("embed", (d.vocab_size, H)))
        for i in range(d.num_hidden_layers):
            self.spec += [(f"l{i}.wqkv", (d.qkv_out, H)), (f"l{i}.bqkv", (d.qkv_out,)), (f"l{i}.wo", (H, H)),
                          (f"l{i}.wgu", (2 * I, H)), (f"l{i}.wdown", (H, I)), (f"l{i}.ln1", (H,)), (f"l{i}.ln2", (H,))]
        self.spec.append(("norm", (H,)))
        self.off = {}
        n = 0
        for k, shp in self.spec:
            self.off[k] = (n, shp)
            n += ops.round_up(math.prod(shp), self.ALIGN)
        self.numel = n
        self.master = torch.zeros(n, dtype=torch.float32, device=device)
        self.grad = torch.zeros(n, dtype=torch.float32, device=device)
        self.bf16 = torch.zeros(n, dtype=torch.bfloat16, device=device)
        self._seen_version = -1
        self.pending_update = None                 # event of an optimizer update running on a side stream (FusedAdamW overlap)
        ops.register_bf16_mirror(self)
        # gradients of the big per-layer matrices are written by exactly one GEMM per backward pass: after a
        # zero_grad they are not cleared but marked "fresh", and that GEMM overwrites (beta = 0) instead of adding
        self.fresh = set()
        # the tied embedding's gradient is first written by the lm-head weight-gradient GEMM (every vocabulary row), so it is
        # "fresh" too: 983 MB that are neither zero-filled nor read back; writers that only ADD call ensure_zeroed first
        self._big = [k for k, shp in self.spec if len(shp) == 2]
        big = set(self._big)
        self._small_runs = []                      # maximal runs of the remaining (small / multi-writer) tensors
        run = None
        for k, shp in self.spec:
            o, _ = self.off[k]
            end = o + ops.round_up(math.prod(shp), self.ALIGN)
            if k in big:
                run = None
            elif run is None:
                run = [o, end]
                self._small_runs.append(run)
            else:
                run[1] = end
        self._small_table = torch.tensor([[lo, hi - lo] for lo, hi in self._small_runs], dtype=torch.int64, device=device)
        self._small_max = max(hi - lo for lo, hi in self._small_runs)

    def view(self, buf, key):
        o, shp = self.off[key]
        return buf[o:o + math.prod(shp)].view(shp)

    def p(self, key):
        return self.view(self.master, key)

    def g(self, key):
        return self.view(self.grad, key)

    def wait_pending_update(self):
        """Order the current stream behind an overlapped optimizer update before it touches weights or gradients."""
        if self.pending_update is not None:
            torch.cuda.current_stream().wait_event(self.pending_update)
            self.pending_update = None

    def clear_grads(self):
        """Start of a gradient pass after zero_grad: clear what is accumulated into (embedding, norms, biases) and
        mark the big matrices fresh (their single weight-gradient GEMM overwrites them): 5.2 of the 6.2 GB are never
        zero-filled nor read back."""
        self.wait_pending_update()
        ops.zero_ranges_(self.grad, self._small_table, self._small_max)     # one launch instead of one fill per run
        self.fresh = set(self._big)

    def beta_for(self, key):
        """1 (accumulate) or 0 (first and only write of this pass) for the weight-gradient GEMM of `key`."""
        if key in self.fresh:
            self.fresh.discard(key)
            return 0
        return 1

    def ensure_zeroed(self, key):
        """For writers that accumulate into part of `key` (embedding scatter-add, a vocabulary slice of the head): if no
        full overwrite has happened yet in this pass, clear it now."""
        if key in self.fresh:
            self.fresh.discard(key)
            self.g(key).zero_()

    def flush_fresh(self):
        """End of the backbone's backward: a matrix that received no gradient in this pass must read as zero."""
        for k in self.fresh:
            self.g(k).zero_()
        self.fresh = set()

    def w(self, key):
        return self.view(self.bf16, key)

    def refresh_compute_copies(self, force=False):
        """bf16 compute copy of the fp32 master weights (one HBM pass per optimizer step; dgrad / wgrad read
        the same copy through the GEMM's k-major operand mode, so no transposed copies exist)."""
        self.wait_pending_update()
        ver = self.master._version
        if not force and ver == self._seen_version:
            return
        ops.cast_bf16(self.master, self.bf16)
        self._seen_version = ver


def _hf_name_map(dims):
    """reference checkpoint key (under `llm.`) -> (flat key, row slice | None)."""
    d = dims
    hd, Hq, Hk = d.head_dim, d.num_attention_heads, d.num_key_value_heads
    q_end, k_end = Hq * hd, (Hq + Hk) * hd
    m = {"model.embed_tokens.weight": ("embed", None), "model.norm.weight": ("norm", None)}
    for i in range(d.num_hidden_layers):
        p = f"model.layers.{i}."
        m[p + "self_attn.q_proj.weight"] = (f"l{i}.wqkv", (0, q_end))
        m[p + "self_attn.k_proj.weight"] = (f"l{i}.wqkv", (q_end, k_end))
        m[p + "self_attn.v_proj.weight"] = (f"l{i}.wqkv", (k_end, d.qkv_out))
        m[p + "self_attn.q_proj.bias"] = (f"l{i}.bqkv", (0, q_end))
        m[p + "self_attn.k_proj.bias"] = (f"l{i}.bqkv", (q_end, k_end))
        m[p + "self_attn.v_proj.bias"] = (f"l{i}.bqkv", (k_end, d.qkv_out))
        m[p + "self_attn.o_proj.weight"] = (f"l{i}.wo", None)
        m[p + "mlp.gate_proj.weight"] = (f"l{i}.wgu", (0, d.intermediate_size))
        m[p + "mlp.up_proj.weight"] = (f"l{i}.wgu", (d.intermediate_size, 2 * d.intermediate_size))
        m[p + "mlp.down_proj.weight"] = (f"l{i}.wdown", None)
        m[p + "input_layernorm.weight"] = (f"l{i}.ln1", None)
        m[p + "post_attention_layernorm.weight"] = (f"l{i}.ln2", None)
    return m


def resolve_deterministic(deterministic=None):
    """The decode mode of a generation call: `deterministic` if given, else torch's global flag
    (torch.use_deterministic_algorithms)."""
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


class DecodeState:
    """Static KV cache for autoregressive generation: per layer K,V [rows][HKV][Tmax][128] bf16, the write
    position and visible length as DEVICE ints (so one captured graph serves every step).
    deterministic: the decode steps on this state use the ORDERED forms (no float atomics: every split-K partial lands in a slot
    of its own and its consumer sums the slots in ascending order), so the same inputs give the same bits on every run, eager or
    captured.  The state's scratch is then partial slots instead of accumulators, so a captured step belongs to one mode.
    step_rows: the rows of a decode step's operands and scratch -- `rows` (the default) everywhere except in a speculative session
    (SpecDecodeSession), whose step rows are consecutive positions of its ONE cache row."""

    def __init__(self, dims, rows, Tmax, device, key_valid=None, deterministic=False, step_rows=None):
        self.rows, self.Tmax = rows, Tmax
        self.step_rows = rows if step_rows is None else int(step_rows)
        self.deterministic = bool(deterministic)
        n, hk, hd = dims.num_hidden_layers, dims.num_key_value_heads, dims.head_dim
        self.k = [torch.zeros((rows, hk, Tmax, hd), dtype=torch.bfloat16, device=device) for _ in range(n)]
        self.v = [torch.zeros((rows, hk, Tmax, hd), dtype=torch.bfloat16, device=device) for _ in range(n)]
        self.pos = torch.zeros(1, dtype=torch.int32, device=device)
        self.len = torch.zeros(1, dtype=torch.int32, device=device)
        self.key_valid = None
        if key_valid is not None:
            kv = torch.ones((rows, Tmax), dtype=torch.uint8, device=device)
            kv[:, :key_valid.shape[1]] = key_valid.to(device=device, dtype=torch.uint8)
            self.key_valid = kv

    def advance(self):
        self.pos.add_(1)
        self.len.add_(1)

    def ensure_scratch(self, dims, form):
        """Persistent scratch of one decode layer form (Qwen2Engine.decode_form), allocated on first use.
        splitk: one raw fp32 accumulator per split-K projection (row-major [rows][N]; each is cleared by a later launch once fully
        consumed), the second residual-stream buffer, and the row sum-of-squares slots that carry the RMSNorm statistics to the
        accumulators' consumers.
        sw: the o and gate/up projections are single-writer launches (csrc/decode_sw.hip) -- no gate/up or o accumulator, a finished
        bf16 `act` instead, and two down-projection accumulators that alternate by layer: layer l adds into acc_down (l even) or
        acc_down2 (l odd) and clears the other one, which layer l - 1 left and layer l's q/k/v launch has consumed.  The last layer's
        accumulator is cleared by its reader when that is the final-norm launch of decode_step; the head launch of decode_step_logits
        leaves it as it is, so at odd depth (where it is acc_down, the one layer 0 adds into) layer 0's q/k/v launch of the next step
        clears it.
        ord_sw: the q/k/v k-slab slots [6][rows][q/k/v width] with their row statistics [6][32], ONE set of down-projection k-block
        slots [5][rows][hidden] (layer l + 1's q/k/v launch consumes them before layer l + 1's down projection rewrites them: no second
        set, no clears), the second residual-stream buffer and `act`.  The wide forms keep no scratch."""
        if getattr(self, {"splitk": "acc_gu", "sw": "acc_down2", "ord_sw": "qkv_part"}[form], None) is not None:
            return                                 # (every step asks; the buffer only this form has says it is all there)
        dev = self.pos.device
        R, H, I = self.step_rows, dims.hidden_size, dims.intermediate_size
        nqkv = (dims.num_attention_heads + 2 * dims.num_key_value_heads) * dims.head_dim
        z = lambda *shape: lambda: torch.zeros(shape, dtype=torch.float32, device=dev)
        e = lambda *shape: lambda: torch.empty(shape, dtype=torch.float32, device=dev)
        act = lambda: torch.empty((R, I), dtype=torch.bfloat16, device=dev)
        acc = {"acc_qkv": z(R, nqkv), "acc_down": z(R, H), "x_mid": z(R, H), "ss_attn": z(32), "ss_mlp": z(32)}
        want = {"splitk": {**acc, "acc_o": z(R, H), "acc_gu": z(R, 2 * I)},
                "sw": {**acc, "zeros": z(R, H), "act": act, "acc_down2": z(R, H)},
                "ord_sw": {"ss_part": e(ops.ORD_QKV_SLABS, 32), "down_part": e(ops.ORD_DOWN_KBLOCKS, R, H), "x_mid": z(R, H), "act": act,
                           "qkv_part": e(ops.ORD_QKV_SLABS, R, nqkv)}}[form]               # (the form's own buffer last)
        for name, make in want.items():
            if getattr(self, name, None) is None:
                setattr(self, name, make())


class TextDecodeSession:
    """Everything a text decode step on the device reads or writes, kept across calls with the captured step: the decode state (KV
    cache of `capacity` positions), the pick kernels' state block, the next input `x`, the last token, the token buffer [rows, width],
    the rows' lengths, the head's fp32 logits, and for sampling the histogram workspace and the uniforms [width, rows].
    sampling: None (greedy) or (temperature, top_k, top_p).  The logits' leading dimension is the vocabulary rounded up to 8, except in
    deterministic mode, where the ordered head writes a contiguous [rows, vocab] result.
    repetition_penalty p != 1: the session owns the logits processor's `seen` bitmap [rows, ceil(vocab / 32)] (include/unigen_hip.h:
    ug_text_penalize) and every step launches the processor between head and pick; p == 1 allocates and launches nothing.
    logprobs: the session owns `logp` fp32 [rows, width] and every pick launch is the entry point that also writes the emitted token's
    log-probability into it (ug_text_pick_logp / ug_text_sample_logp); off: no buffer, the entry points without the output.
    constraints: None, or the dict models/unigen.py: checked_constraints returns (bias = [(id, bias or -inf), ...], min_new, ngram,
    stop_seqs = [[ids], ...] of two or more ids each).  With a bias list, min_new or ngram the session owns the bias pairs and, for
    ngram, the prompt history `hist` int32 [rows, capacity] + `hist_len` [rows], and every step launches ug_text_constrain ahead of the
    penalty; with stop sequences it owns their packed ids and offsets and every step launches ug_text_stop_seq behind the pick.  All
    off: nothing allocated, nothing launched."""

    def __init__(self, eng, rows, capacity, width, vocab, deterministic=False, sampling=None, stop_ids=(), pad_id=None, key_valid=None,
                 repetition_penalty=1.0, logprobs=False, constraints=None):
        dev, d = eng.device, eng.dims
        self.rows, self.width, self.V, self.sampling = rows, width, vocab, sampling
        self.form = eng.decode_form(rows, deterministic)
        self.st = DecodeState(d, rows, capacity, dev, key_valid=key_valid, deterministic=deterministic)
        self.state = ops.text_state(rows, dev)
        self.x = torch.zeros((rows, d.hidden_size), dtype=torch.float32, device=dev)
        self.tok = torch.zeros((rows,), dtype=torch.long, device=dev)
        self.out_tokens = torch.zeros((rows, width), dtype=torch.int32, device=dev)
        self.lengths = torch.zeros((rows,), dtype=torch.int32, device=dev)
        self.logits = torch.zeros((rows, vocab if deterministic else ops.round_up(vocab, 8)), dtype=torch.float32, device=dev)
        self.stop_ids = torch.tensor([int(s) for s in stop_ids], dtype=torch.long, device=dev) if len(stop_ids) else None
        self.pad_id = pad_id
        self.workspace = self.uniforms = None
        if sampling is not None:
            self.workspace = ops.text_sample_workspace(rows, dev)
            self.uniforms = torch.zeros((width, rows), dtype=torch.float32, device=dev)
        self.penalty = float(repetition_penalty)
        self.seen = ops.text_seen(rows, vocab, dev) if self.penalty != 1.0 else None
        self.logp = torch.zeros((rows, width), dtype=torch.float32, device=dev) if logprobs else None
        c = constraints or {}
        self.bias = ops.text_bias_pairs(c.get("bias"), dev)
        self.min_new, self.ngram = int(c.get("min_new", 0)) if len(stop_ids) else 0, int(c.get("ngram", 0))
        self.constrained = self.bias is not None or self.min_new > 0 or self.ngram > 0
        self.hist = torch.zeros((rows, capacity), dtype=torch.int32, device=dev) if self.ngram else None
        self.hist_len = torch.zeros((rows,), dtype=torch.int32, device=dev) if self.ngram else None
        self.stop_seqs = ops.text_stop_seqs(c["stop_seqs"], dev) if c.get("stop_seqs") else None
        self.graph, self.key = None, None

    def begin(self, new_tokens, key_valid=None, prompt_len=0, prompt_ids=None, prompt_valid=None):
        """the host's part of a call's start: state block reset, lengths, and (a reused session) the key-validity columns -- the
        prompt's, ones behind them.  The prefill sets position and length.  With a repetition penalty: `seen` zeroed, then the bits
        of prompt_ids [rows, L] (None: a prompt given as embeddings has no ids) at the positions prompt_valid [rows, L] marks real
        (None: all)."""
        ops.text_state_reset_(self.state, self.rows)
        self.lengths.fill_(int(new_tokens))
        if self.logp is not None:
            self.logp.zero_()
        if key_valid is not None:
            self.st.key_valid[:, :prompt_len].copy_(key_valid)
            self.st.key_valid[:, prompt_len:].fill_(1)
        if self.seen is not None:
            self.seen.zero_()
            if prompt_ids is not None and prompt_ids.shape[1] > 0:
                ops.text_seen_mark_(self.seen, prompt_ids, self.V, prompt_valid)
        if self.hist is not None:                   # the n-gram block's prompt history: the ids the penalty counts, compacted, in order
            self.hist_len.zero_()
            if prompt_ids is not None and prompt_ids.shape[1] > 0:
                ids = prompt_ids.to(self.hist.device).long()
                ok = (ids >= 0) & (ids < self.V)
                if prompt_valid is not None:
                    ok &= prompt_valid.to(ok.device) != 0
                order = torch.argsort((~ok).to(torch.int8), dim=1, stable=True)
                self.hist[:, :ids.shape[1]].copy_(torch.gather(ids, 1, order))
                self.hist_len.copy_(ok.sum(1))


class ArDecodeSession:
    """Everything an AR image decode step reads or writes, kept across `t2i_generate_ar` calls with the captured step: the decode state
    (KV cache of prefix + steps positions), the next input `x` (static: next token's embedding), the last sampled token `tok`, the token
    buffer [bsz, steps], and the constants the sampler launch takes as kernel arguments (rows = conditional then unconditional,
    vocabulary slice [code_lo, code_lo + V), CFG scale, temperature, greedy, filt = None or (top_k, top_p, min_p)).
    fused: the head's raw fp32 accumulator `acc_head` [rows, V] (the sampler launch leaves it zeroed) and, unless greedy, the
    `uniforms` [steps, bsz] of the call, drawn from `generator` up front.  Not fused (the host sampler, UniGen._ar_host_token): neither.
    logprobs: `logp` fp32 [bsz, steps, 2] = (logprobs, cond_logprobs) of every token, written by the sampler launch (fused) or copied
    per step from `lp_now` [bsz, 2], the host sampler's pair of the step."""

    def __init__(self, eng, rows, bsz, prefix_len, steps, V, code_lo, guidance_scale, temperature, greedy=False, filt=None, deterministic=False,
                 key_valid=None, generator=None, logprobs=False, fused=True):
        dev = eng.device
        self.fused = fused
        self.bsz, self.P, self.n, self.V, self.code_lo = bsz, prefix_len, steps, V, code_lo
        self.guidance_scale, self.temperature, self.greedy, self.filt = guidance_scale, temperature, greedy, filt
        self.form = eng.decode_form(rows, deterministic)
        self.st = DecodeState(eng.dims, rows, prefix_len + steps, dev, key_valid=key_valid, deterministic=deterministic)
        self.out_tokens = torch.zeros((bsz, steps), dtype=torch.int, device=dev)
        self.x = torch.empty((rows, eng.dims.hidden_size), dtype=torch.float32, device=dev)
        self.tok = torch.zeros((bsz, 1), dtype=torch.long, device=dev)
        self.logp = torch.zeros((bsz, steps, 2), dtype=torch.float32, device=dev) if logprobs else None
        self.uniforms = self.draw_uniforms(generator)
        self.acc_head = torch.zeros((rows, V), dtype=torch.float32, device=dev) if fused else None
        self.lp_now = torch.zeros((bsz, 2), dtype=torch.float32, device=dev) if logprobs and not fused else None
        self.graph, self.key = None, None

    def draw_uniforms(self, generator):
        """the call's uniforms for the fused sampler's inverse-CDF draw, on the generator's device (default: the engine's) and then
        here: once per call, ahead of the prefill; None when greedy or not fused (the host sampler draws by itself)"""
        if self.greedy or not self.fused:
            return None
        dev = self.st.pos.device
        return torch.rand((self.n, self.bsz), device=dev if generator is None else generator.device, generator=generator).to(dev)

    def begin(self, key_valid=None, generator=None):
        """what a reused session needs at a call's start: the new prompt's key-validity columns and the call's uniforms in the buffer
        the graph reads.  The prefill sets position and length."""
        if key_valid is not None:
            self.st.key_valid[:, :self.P].copy_(key_valid)
        if self.uniforms is not None:
            self.uniforms.copy_(self.draw_uniforms(generator))


class SpecDecodeSession:
    """Everything a verify step of prompt-lookup speculative decoding reads or writes (Qwen2Engine.spec_step), kept across calls with
    the captured step like TextDecodeSession: ONE greedy row whose step runs S = num_draft + 1 rows -- the last emitted token and a draft
    of up to num_draft tokens, at consecutive positions of the one cache row.  A one-row DecodeState of `capacity` >= prompt +
    max_new_tokens + num_draft positions with S step rows, the inputs `x` fp32 [S, H] and `tok` int64 [S], the head's logits
    [S, round_up(vocab, 8)], the state block (ops.SPEC_*: emitted, done, the counters, the draft length of `tok`, the history's
    length), the searchable history `hist` int32 [hist_cap] (lookup ids, then the prompt's, then everything emitted), the token
    buffer and the row's length.  new_tokens is a kernel argument of the captured step (the width the emission is cut at)."""

    def __init__(self, eng, capacity, new_tokens, vocab, num_draft, ngram, hist_cap, stop_ids=(), key_valid=None):
        dev, d = eng.device, eng.dims
        self.S, self.K, self.G, self.V, self.n = num_draft + 1, int(num_draft), int(ngram), vocab, int(new_tokens)
        self.form = eng.spec_form(self.S)
        self.st = DecodeState(d, 1, capacity, dev, key_valid=key_valid, step_rows=self.S)
        self.state = torch.zeros(ops.SPEC_STATE_INTS, dtype=torch.int32, device=dev)
        self.x = torch.zeros((self.S, d.hidden_size), dtype=torch.float32, device=dev)
        self.tok = torch.zeros((self.S,), dtype=torch.long, device=dev)
        self.logits = torch.zeros((self.S, ops.round_up(vocab, 8)), dtype=torch.float32, device=dev)
        self.out_tokens = torch.zeros((ops.round_up(self.n, 64),), dtype=torch.int32, device=dev)
        self.lengths = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.hist = torch.zeros((int(hist_cap),), dtype=torch.int32, device=dev)
        self.stop_ids = torch.tensor([int(s) for s in stop_ids], dtype=torch.long, device=dev) if len(stop_ids) else None
        self.graph, self.key = None, None

    def begin(self, history, key_valid=None, prompt_len=0):
        """the host's part of a call's start: the state block zeroed, the history = `history` (int 1-D: lookup ids, then the prompt's
        valid ids), and (a reused session) the key-validity columns.  The prefill sets position and length."""
        n = int(history.numel())
        if n + self.n > self.hist.numel():
            raise UniGenHipError(f"SpecDecodeSession: a history of {n} ids + {self.n} new tokens exceeds the session's {self.hist.numel()}")
        self.state.zero_()
        self.state[ops.SPEC_HIST_LEN:ops.SPEC_HIST_LEN + 1].fill_(n)
        self.hist[:n].copy_(history)
        self.lengths.fill_(self.n)
        self.logits.zero_()                         # (the first token's GEMV head adds into row 0; the splitk head into all rows)
        if key_valid is not None:
            self.st.key_valid[:, :prompt_len].copy_(key_valid)
            self.st.key_valid[:, prompt_len:].fill_(1)

    def stats(self):
        """-> {steps, drafted, accepted, emitted} of the call so far (one host read)"""
        s = self.state.tolist()
        return {"steps": s[ops.SPEC_STEPS], "drafted": s[ops.SPEC_DRAFTED], "accepted": s[ops.SPEC_ACCEPTED], "emitted": s[ops.SPEC_EMITTED]}


def _keeping(wanted):
    """the keep policy of both decode sessions: a call that asks for it keeps its session unless UNIGEN_AR_GRAPH_CACHE=0"""
    return bool(wanted) and os.environ.get("UNIGEN_AR_GRAPH_CACHE", "1") != "0"


def take_session(eng, attr, key, wanted):
    """The session kept on eng.<attr> if this call may reuse one and `key` is its key, else None.  The attribute is cleared either
    way: put_session puts the session back at the end of a call that completed, so a call that raises leaves none."""
    sess = getattr(eng, attr, None) if _keeping(wanted) else None
    setattr(eng, attr, None)
    return sess if sess is not None and sess.key == key else None


def put_session(eng, attr, sess, wanted):
    """at the end of a completed call: keep the session if it has a captured step -> whether it was kept (the results then have to be
    copies: the next call overwrites the session's buffers)"""
    kept = _keeping(wanted) and sess.graph is not None
    if kept:
        setattr(eng, attr, sess)
    return kept


def decode_loop(sess, step, steps, use_graph, stop=None, mark=None, after=None):
    """The token loop of both on-device decodes behind the first token: for every i of `steps` (1, 2, ...), `step()` eagerly, except
    that with use_graph step 1 alone runs eagerly (warm-up: allocations, lazy inits), step 2 is captured into sess.graph -- capture
    only records, so its first replay IS step 2 -- and every later step, and every step of a session that comes with a graph, is a
    replay.  stop(i), asked before step i, ends the loop early; after(i) runs behind step i, outside the captured step; mark(name)
    closes the timing phases eager_step / capture / replay.  -> whether this call captured."""
    mark = mark or (lambda name: None)
    captured = False
    for i in steps:
        if stop is not None and stop(i):
            break
        if sess.graph is None and use_graph and i == 2:
            mark("eager_step")
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            sess.graph, captured = graph, True
            mark("capture")
            graph.replay()
        elif sess.graph is not None:
            sess.graph.replay()
        else:
            step()
        if after is not None:
            after(i)
    mark("replay")
    return captured


class _Saved:
    __slots__ =("h", "rstd1", "xn1", "qkv", "o", "lse", "h_mid", "rstd2", "xn2", "gu", "act")


class Qwen2Engine:
    """Decoder stack + head on the HIP kernels.  Not an nn.Module: the module tree lives in
    `modules.py`; this object owns buffers and orchestrates kernel launches."""

    def __init__(self, dims, device):
        self.dims, self.device = dims, device
        self.fp = FlatParams(dims, device)
        self._rope_cache = {}
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.grad_ready_hook = None      # callable(layer_index | 'embed' | 'norm') fired as grads complete (DDP)

    # ---------------------------------------------------------------- helpers
    def rope(self, L):
        if L not in self._rope_cache:
            self._rope_cache[L] = ops.rope_tables(L, self.dims.head_dim, self.dims.rope_theta, self.device, self.dims.rope_scaling)
        return self._rope_cache[L]

    def check_errors(self):
        """Device-side error flags (out-of-range token id = 1, non-binary attention mask = 2, bad VQ code = 4)."""
        v = int(self.err_flag.item())
        if v:
            self.err_flag.zero_()
            raise UniGenHipError(f"device-side input check failed (flags={v}): 1=token id out of range, "
                                 f"2=attention mask value neither 0 nor <= -1e9, 4=VQ code out of range")

    # ---------------------------------------------------------------- forward
    def layer_fwd(self, i, h, mb, L, save):
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        cos, sin = self.rope(L)
        xn1, rstd1 = ops.rmsnorm_fwd(h, fp.p(f"l{i}.ln1"), d.rms_norm_eps)
        qkv = ops.gemm_qkv_rope(xn1, fp.w(f"l{i}.wqkv"), fp.w(f"l{i}.bqkv"), cos, sin, L, Hq + Hk, hd)     # projection + RoPE, one launch
        o, lse = ops.attn_fwd(qkv, mb, Hq, Hk, hd)
        h_mid = ops.gemm_nt(o, fp.w(f"l{i}.wo"), epilogue=ops.UG_EPI_RESID, resid=h)
        xn2, rstd2 = ops.rmsnorm_fwd(h_mid, fp.p(f"l{i}.ln2"), d.rms_norm_eps)
        gu, act = ops.gemm_swiglu(xn2, fp.w(f"l{i}.wgu"))           # projection + SwiGLU in its epilogue (one launch; UNIGEN_FUSED_SWIGLU=0: two)
        h_out = ops.gemm_nt(act, fp.w(f"l{i}.wdown"), epilogue=ops.UG_EPI_RESID, resid=h_mid)
        if save is not None:
            s = _Saved()
            s.h, s.rstd1, s.xn1, s.qkv, s.o, s.lse = h, rstd1, xn1, qkv, o, lse
            s.h_mid, s.rstd2, s.xn2, s.gu, s.act = h_mid, rstd2, xn2, gu, act
            save.append(s)
        return h_out

    def stack_fwd(self, h0, mb, L, save):
        """h0 fp32 [B*L, H] -> (h_last fp32, hn bf16 = final-norm output, rstd of the final norm)."""
        self.fp.refresh_compute_copies()
        h = h0
        for i in range(self.dims.num_hidden_layers):
            h = self.layer_fwd(i, h, mb, L, save)
        hn, rstd = ops.rmsnorm_fwd(h, self.fp.p("norm"), self.dims.rms_norm_eps)
        return h, hn, rstd

    # ---------------------------------------------------------------- incremental MaskGIT rounds
    def maskgit_begin(self, h0, mb, L, seg_start):
        """First round of UniGen.t2i_generate: a full forward that keeps every layer's (post-RoPE) q/k/v.  The rows before
        `seg_start` (padding + text) are causal and never see the image segment, so their keys / values are the same in
        every later round; only the segment rows [seg_start, L) are recomputed by maskgit_step.
        h0 fp32 [B*L, H] -> (session, final-norm hidden of the segment rows bf16 [B*S, H])."""
        self.fp.refresh_compute_copies()
        B = h0.shape[0] // L
        saved, h = [], h0
        for i in range(self.dims.num_hidden_layers):
            h = self.layer_fwd(i, h, mb, L, saved)
        sess = types.SimpleNamespace()
        sess.qkv = [s.qkv for s in saved]
        sess.mb, sess.B, sess.L, sess.P, sess.S = mb, B, L, seg_start, L - seg_start
        r = torch.arange(seg_start, L, device=self.device)
        sess.rows = (torch.arange(B, device=self.device)[:, None] * L + r[None, :]).reshape(-1).contiguous()
        cos, sin = self.rope(L)
        sess.cos, sess.sin = cos[seg_start:].contiguous(), sin[seg_start:].contiguous()
        hn, _ = ops.rmsnorm_fwd(h.view(B, L, -1)[:, seg_start:].reshape(B * sess.S, -1).contiguous(), self.fp.p("norm"),
                                self.dims.rms_norm_eps, want_rstd=False)
        return sess, hn

    def maskgit_step(self, sess, seg):
        """seg fp32 [B*S, H] = embeddings of the segment rows this round -> final-norm hidden bf16 [B*S, H].  All GEMMs and
        norms run on the B*S segment rows only; attention runs over the full sequence from the per-layer q/k/v buffers
        (prefix rows cached, segment rows refreshed in place)."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        h = seg
        for i in range(d.num_hidden_layers):
            xn1, _ = ops.rmsnorm_fwd(h, fp.p(f"l{i}.ln1"), d.rms_norm_eps, want_rstd=False)
            qkv_s = ops.gemm_qkv_rope(xn1, fp.w(f"l{i}.wqkv"), fp.w(f"l{i}.bqkv"), sess.cos, sess.sin, sess.S, Hq + Hk, hd)   # row r sits at position seg_start + r % S
            ops.scatter_rows_(qkv_s, sess.rows, sess.qkv[i])
            o, _ = ops.attn_fwd(sess.qkv[i], sess.mb, Hq, Hk, hd)
            o_s = ops.gather_rows(o, sess.rows)
            h_mid = ops.gemm_nt(o_s, fp.w(f"l{i}.wo"), epilogue=ops.UG_EPI_RESID, resid=h)
            xn2, _ = ops.rmsnorm_fwd(h_mid, fp.p(f"l{i}.ln2"), d.rms_norm_eps, want_rstd=False)
            _, act = ops.gemm_swiglu(xn2, fp.w(f"l{i}.wgu"))
            h = ops.gemm_nt(act, fp.w(f"l{i}.wdown"), epilogue=ops.UG_EPI_RESID, resid=h_mid)
        hn, _ = ops.rmsnorm_fwd(h, fp.p("norm"), d.rms_norm_eps, want_rstd=False)
        return hn

    # ---------------------------------------------------------------- backward
    def layer_bwd(self, i, s, dh, mb, L, dh_bf16=None):
        """dh fp32 [M,H]: grad w.r.t. the layer output on entry, w.r.t. the layer input on exit (in place).
        Weight gradients accumulate into the flat fp32 grad buffer.  dh_bf16: bf16(dh) if the producer already has it.
        Returns (dh, bf16(dh)): every RMSNorm backward also emits the bf16 operand of the GEMMs that follow."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        cos, sin = self.rope(L)
        F32 = ops.UG_EPI_F32
        # ---- MLP   (wgrad: both operands k-major over the token axis; dgrad: weight read k-major)
        # The four weight gradients (dW = dY^T X, both operands token-major) are leaves of the backward graph: they are
        # collected and issued as ONE grouped launch at the end of the layer (3 rounds of the chip instead of 2 + 1 + two
        # k-sliced launches, ops.gemm_wgrad_group).
        wg = lambda key, dy, x: (dy, x, fp.g(key), fp.beta_for(key))
        dyd = dh_bf16 if dh_bf16 is not None else ops.cast_bf16(dh)
        w_down = wg(f"l{i}.wdown", dyd, s.act)
        dgu = ops.gemm_swiglu_bwd(dyd, fp.w(f"l{i}.wdown"), s.gu)          # down dgrad + SwiGLU backward in its epilogue: d(act) never stored
        w_gu = wg(f"l{i}.wgu", dgu, s.xn2)
        dxn2 = ops.gemm(dgu, fp.w(f"l{i}.wgu"), b_kmajor=True)
        dyo = ops.rmsnorm_bwd(dxn2, s.h_mid, s.rstd2, fp.p(f"l{i}.ln2"), dh, fp.g(f"l{i}.ln2"), want_bf16=True)
        # ---- attention
        w_o = wg(f"l{i}.wo", dyo, s.o)
        do = ops.gemm(dyo, fp.w(f"l{i}.wo"), b_kmajor=True)
        # RoPE transposed and the bias gradient (column sums) where the attention backward stores dq / dk / dv
        dqkv = ops.attn_bwd(s.qkv, s.o, s.lse, do, mb, Hq, Hk, hd, rope=(cos, sin), dbias=fp.g(f"l{i}.bqkv"))
        w_qkv = wg(f"l{i}.wqkv", dqkv, s.xn1)
        dxn1 = ops.gemm(dqkv, fp.w(f"l{i}.wqkv"), b_kmajor=True)
        dnext = ops.rmsnorm_bwd(dxn1, s.h, s.rstd1, fp.p(f"l{i}.ln1"), dh, fp.g(f"l{i}.ln1"), want_bf16=True)
        # ... plus a slice of the tied head's weight gradient when one is waiting (head_bwd): its 128-k-tile tiles run on the CUs
        # the group's partial third round (714 tiles = 2.79 rounds) leaves idle, so most of the head's 1.7 ms weight-gradient
        # launch disappears from the step
        self._wgrad_tokens = dyd.shape[0]
        ops.gemm_wgrad_group([w_gu, w_down, w_qkv, w_o] + self._head_wgrad_slice())
        return dh, dnext

    def stack_bwd(self, saved, h_last, rstd_last, dhn, mb, L):
        """dhn bf16 [M,H] (grad of the final-norm output) -> dh0 fp32 [M,H]."""
        dh = torch.zeros_like(h_last)
        dh16 = ops.rmsnorm_bwd(dhn, h_last, rstd_last, self.fp.p("norm"), dh, self.fp.g("norm"), want_bf16=True)
        if self.grad_ready_hook:
            self.grad_ready_hook("norm")
        for i in reversed(range(self.dims.num_hidden_layers)):
            dh, dh16 = self.layer_bwd(i, saved[i], dh, mb, L, dh16)
            saved[i] = None                       # release this layer's activations
            if self.grad_ready_hook:
                self.grad_ready_hook(i)
        self.flush_deferred_head()
        self.fp.flush_fresh()
        return dh

    # ---------------------------------------------------------------- head
    def logits_rows(self, hn_rows):
        """hn_rows bf16 [R, H] -> logits bf16 [R, vocab_pad] (columns >= vocab_size are unspecified)."""
        d = self.dims
        out = torch.empty((hn_rows.shape[0], d.vocab_pad), dtype=torch.bfloat16, device=self.device)
        return ops.gemm_nt(hn_rows, self.fp.w("embed"), out=out, N=d.vocab_size, K=d.hidden_size)

    def score_rows(self, hn_rows, labels, ignore_index=-100):
        """hn_rows bf16 [R, H], labels int64 [R] -> (logp fp32 [R], lse fp32 [R], best int64 [R]) against the tied table, without the
        [R, vocab] logits logits_rows would write (ops.head_score); logp is 0.0 where the label is ignore_index."""
        self.fp.refresh_compute_copies()
        return ops.head_score(hn_rows, self.fp.w("embed"), self.dims.vocab_size, labels, ignore_index=ignore_index, want=("lse", "best"))

    def head_bwd(self, dlogits, hn_rows):
        """dlogits bf16 [R, vocab_pad] (pad columns zero) -> dhn_rows bf16 [R,H]; embed grad accumulated."""
        d, fp = self.dims, self.fp
        R = hn_rows.shape[0]
        sync = getattr(self, "grad_sync", None)
        if sync is not None:
            sync.before_dense_embed_write()       # (data parallel: a table already handed over is waited for and re-exchanged)
        # dW[V,H] += dlogits^T hn : both k-major over the R selected rows (dlogits' leading dim is vocab_pad)
        if self._may_defer_head_wgrad(R):
            # a leaf of the backward graph: handed to the decoder layers' grouped weight-gradient launches slice by slice
            # (layer_bwd), whatever is left is launched by flush_deferred_head before any other writer of the table runs
            self.flush_deferred_head()
            self._deferred_head = [dlogits, hn_rows, fp.beta_for("embed"), 0]
            torch.autograd.Variable._execution_engine.queue_callback(self.flush_deferred_head)
        else:
            ops.gemm(dlogits, hn_rows, out=fp.g("embed"), M=d.vocab_size, N=d.hidden_size, K=R, a_kmajor=True, b_kmajor=True,
                     epilogue=ops.UG_EPI_F32, beta=fp.beta_for("embed"))
        # dhn[R,H] = dlogits[R,V] W[V,H] : W read k-major; its rows >= V come from the zero page and the
        # dlogits pad columns are zero (ug_ce_bwd), so K = V needs no padding
        return ops.gemm(dlogits, fp.w("embed"), M=R, N=d.hidden_size, K=d.vocab_size, b_kmajor=True)

    def _may_defer_head_wgrad(self, R):
        """Only inside a backward pass (the end-of-backward callback is the safety net), on the single-GPU path (with a gradient
        exchange the table's dense part is handed over right after the head instead, unigen_hip/ddp.py), and when the layers'
        grouped launches exist to carry the slices (the grouped form needs a round of tiles)."""
        if os.environ.get("UNIGEN_DEFER_HEAD_WGRAD", "1") != "1" or not torch.is_tensor(self.fp.grad) or not self.fp.grad.is_cuda:
            return False
        sync = getattr(self, "grad_sync", None)
        if sync is not None and sync.active and sync.enabled:
            return False
        d = self.dims
        layer_tiles = sum(-(-a // 256) * -(-b // 256) for a, b in ((2 * d.intermediate_size, d.hidden_size), (d.hidden_size, d.intermediate_size),
                                                                   (d.qkv_out, d.hidden_size), (d.hidden_size, d.hidden_size)))
        return layer_tiles >= ops.WGRAD_GROUP_MIN_TILES and ops.GEMM_POLICY == -1

    def _head_wgrad_slice(self):
        """the next slice of a waiting head weight gradient as a problem of ops.gemm_wgrad_group, or []"""
        st = getattr(self, "_deferred_head", None)
        if not st:
            return []
        dlogits, hn_rows, beta, v0 = st
        V = self.dims.vocab_size
        # Row tiles of the table per layer launch: what fits on the CUs the layer's own tiles leave idle in their last round --
        # idle x (cost of a layer tile / cost of a head tile), costs in k-tiles of 32 plus ~60 for a tile's prologue and fp32
        # epilogue, 80 % of it (measured at the 1.5B shape, 12 336 tokens, 4 096 label rows: 54 idle CUs -> 16 row tiles = 96
        # tiles; 23 -- the whole table over 28 layers -- spills into a fourth round: +45 us per launch).  The rest of the table
        # goes out as one launch at the end of the stack's backward.
        d = self.dims
        layer_tiles = sum(-(-a // 256) * -(-b // 256) for a, b in ((2 * d.intermediate_size, d.hidden_size), (d.hidden_size, d.intermediate_size),
                                                                   (d.qkv_out, d.hidden_size), (d.hidden_size, d.hidden_size)))
        idle = -layer_tiles % 256
        cols = -(-d.hidden_size // 256)
        fit = int(0.8 * idle * (self._wgrad_tokens / 32 + 60) / (hn_rows.shape[0] / 32 + 60) / cols)
        per = int(os.environ.get("UNIGEN_HEAD_SLICE_TILES", "0")) or fit
        if per <= 0:
            return []
        per *= 256
        v1 = min(V, v0 + per)
        prob = (dlogits[:, v0:v1], hn_rows, self.fp.g("embed")[v0:v1], beta)
        if v1 >= V:
            self._deferred_head = None
        else:
            st[3] = v1
        return [prob]

    def flush_deferred_head(self):
        """what is left of a waiting head weight gradient, as one launch (before any other writer of the tied table; end of the
        decoder stack's backward; end of the backward pass)"""
        st = getattr(self, "_deferred_head", None)
        if not st:
            return
        dlogits, hn_rows, beta, v0 = st
        self._deferred_head = None
        V, H = self.dims.vocab_size, self.dims.hidden_size
        ops.gemm(dlogits[:, v0:], hn_rows, out=self.fp.g("embed")[v0:], M=V - v0, N=H, K=hn_rows.shape[0], a_kmajor=True,
                 b_kmajor=True, epilogue=ops.UG_EPI_F32, beta=beta)

    # ---------------------------------------------------------------- autoregressive decode
    def prefill(self, st, embeds, key_valid=None, mask_bits=None):
        """embeds fp32 [rows, P, H] -> final-norm hidden of the LAST position, bf16 [rows, H]; fills the cache.
        mask_bits: compressed [rows, P, P] mask of the prompt (default: causal with `key_valid` columns)."""
        d = self.dims
        R, P, H = embeds.shape
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        self.fp.refresh_compute_copies()
        mb = mask_bits if mask_bits is not None else ops.mask_causal(R, P, self.device, key_valid=key_valid)
        h = embeds.reshape(R * P, H).float().contiguous()
        for i in range(d.num_hidden_layers):
            saved = []
            h = self.layer_fwd(i, h, mb, P, saved)
            ops.kv_store(saved[0].qkv, st.k[i], st.v[i], R, P, Hq, Hk, hd, st.Tmax, None, 0)
        st.pos.fill_(P)
        st.len.fill_(P + 1)
        hn, _ = ops.rmsnorm_fwd(h, self.fp.p("norm"), d.rms_norm_eps, want_rstd=False)
        return hn.view(R, P, H)[:, -1].contiguous()

    def prefill_onto(self, st, embeds, P, key_valid=None, hidden_at=None):
        """Causal prefill of S more positions onto a cache whose first P positions are filled (a shared prompt prefix, the next
        chunk of a chunked prefill, the next turn of a conversation): embeds fp32 [rows, S, H], P + S <= st.Tmax, key_valid
        [rows, P+S] (0 = a key no row may see) or None -> final-norm hidden of the last new position, bf16 [rows, H].  New row s
        sits at position P + s and sees the cache keys [0, P + s] that key_valid allows (ug_attn_prefill_cached, the only
        multi-row attention that reads the cache).  Leaves st.pos = P + S, st.len = P + S + 1 -- what prefill leaves for a prompt
        of P + S positions, so every decode form continues unchanged; prefill_onto(st, x, 0) is a plain causal prefill.
        hidden_at (optional): int64 indices into the flattened [rows * S] new positions -> (hn_last, hn_sel), hn_sel bf16 [n, H] the
        final-norm hidden of those positions (the same ug_rmsnorm_fwd on the gathered rows: asking for a row's last position gives
        the bits of hn_last's row); what score_rows scores a given continuation from."""
        d, fp = self.dims, self.fp
        R, S, H = embeds.shape
        P = int(P)
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        if R != st.rows or S < 1 or P < 0 or P + S > st.Tmax:
            raise UniGenHipError(f"prefill_onto: {R} rows of {S} positions at {P} do not fit a state of {st.rows} rows, {st.Tmax} positions")
        if hidden_at is not None and (hidden_at.dtype != torch.int64 or hidden_at.dim() != 1 or hidden_at.numel() < 1):
            raise UniGenHipError(f"prefill_onto: hidden_at must be a non-empty int64 vector of indices into the {R * S} new positions")
        kv = None
        if key_valid is not None:
            if tuple(key_valid.shape) != (R, P + S):
                raise UniGenHipError(f"prefill_onto: key_valid must be [{R}, {P + S}], got {tuple(key_valid.shape)}")
            kv = torch.ones((R, st.Tmax), dtype=torch.uint8, device=self.device)
            kv[:, :P + S] = key_valid.to(device=self.device, dtype=torch.uint8)
        fp.refresh_compute_copies()
        cos, sin = self.rope(P + S)
        cos, sin = cos[P:].contiguous(), sin[P:].contiguous()
        h = embeds.reshape(R * S, H).float().contiguous()
        for i in range(d.num_hidden_layers):
            xn1, _ = ops.rmsnorm_fwd(h, fp.p(f"l{i}.ln1"), d.rms_norm_eps, want_rstd=False)
            qkv = ops.gemm_qkv_rope(xn1, fp.w(f"l{i}.wqkv"), fp.w(f"l{i}.bqkv"), cos, sin, S, Hq + Hk, hd)   # row r sits at position P + r % S
            ops.kv_store(qkv, st.k[i], st.v[i], R, S, Hq, Hk, hd, st.Tmax, None, P)
            o = ops.attn_prefill_cached(qkv, st.k[i], st.v[i], kv, S, P, Hq, Hk, hd, st.Tmax)
            h_mid = ops.gemm_nt(o, fp.w(f"l{i}.wo"), epilogue=ops.UG_EPI_RESID, resid=h)
            xn2, _ = ops.rmsnorm_fwd(h_mid, fp.p(f"l{i}.ln2"), d.rms_norm_eps, want_rstd=False)
            _, act = ops.gemm_swiglu(xn2, fp.w(f"l{i}.wgu"))
            h = ops.gemm_nt(act, fp.w(f"l{i}.wdown"), epilogue=ops.UG_EPI_RESID, resid=h_mid)
        st.pos.fill_(P + S)
        st.len.fill_(P + S + 1)
        hn, _ = ops.rmsnorm_fwd(h.view(R, S, H)[:, -1].contiguous(), fp.p("norm"), d.rms_norm_eps, want_rstd=False)
        if hidden_at is None:
            return hn
        hn_sel, _ = ops.rmsnorm_fwd(h.index_select(0, hidden_at.to(self.device)), fp.p("norm"), d.rms_norm_eps, want_rstd=False)
        return hn, hn_sel

    def decode_form(self, rows, deterministic):
        """The layer form of a decode step on `rows` rows -- the ONE place that chooses it; recomputed on every call, since
        `decode_fused` and UNIGEN_DECODE_SW may change between states on one engine:
          sw        split-K q/k/v and down, single-writer o / gate-up / head launches (csrc/decode_sw.hip): <= 16 rows at the widths
                    those kernels are built for
          splitk    five split-K launches per layer: up to 32 rows, or UNIGEN_DECODE_SW=0
          wide      separate kernels around skinny GEMMs: `decode_fused = False`, > 32 rows, or sizes the GEMV kernels do not take
          ord_sw    deterministic: the ordered single-writer layer (hidden 1536, intermediate 5 x 1792)
          ord_wide  deterministic, everything else: the wide form on ordered skinny linears
        An intermediate size that is below 256 or no multiple of 32 takes the wide form whatever else holds (decode_sw() used to
        answer True there at the 1536-wide dims, and t2i_generate_ar then ran into a launch that refuses the size)."""
        d = self.dims
        H, I, hd, q_dim = d.hidden_size, d.intermediate_size, d.head_dim, d.num_attention_heads * d.head_dim
        fused = getattr(self, "decode_fused", True)
        sw_ok = (fused and os.environ.get("UNIGEN_DECODE_SW", "1") != "0" and rows <= 16
                 and ops.decode_sw_supported(H, I, q_dim, hd))
        if deterministic:
            ord_dims = H == 256 * ops.ORD_QKV_SLABS and I == 1792 * ops.ORD_DOWN_KBLOCKS and d.num_hidden_layers >= 1
            return "ord_sw" if sw_ok and ord_dims else "ord_wide"
        if not fused or rows > 32 or hd != 128 or min(H, I, q_dim) < 256 or H % 32 or I % 32 or H > 4096:
            return "wide"                                   # (H > 4096: ug_decode_finish_resid_norm holds a row of at most 4096 columns)
        return "sw" if sw_ok else "splitk"

    def decode_sw(self, st):
        """Whether a default-mode decode state of st.rows rows runs the single-writer layer."""
        return self.decode_form(st.rows, False) == "sw"

    def decode_ord_sw(self, st):
        """Whether a deterministic decode state of st.rows rows runs the ordered single-writer layer."""
        return self.decode_form(st.rows, True) == "ord_sw"

    def _decode_layers_ord(self, st, x):
        """The decoder stack of one deterministic decode step, five launches per layer as _decode_layers_sw, without float atomics:
          q/k/v      ordered split-K: operand = the stream + bf16(sum of the previous layer's down k-block slots, in order);
                     stores one partial tile per k-slab (6 slots) and the slabs' row sums of squares
          attention  sums the 6 slots in slab order in its prologue, then finishes q/k/v as the default form does
          o, gate/up the single-writer launches of the default form (already one writer per element)
          down       k-blocks with the partial tile STORED into the k-block's slot (5 slots)
        -> (stream, pending): the residual stream after the last layer is stream + bf16round(sum of pending = st.down_part)."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        H = d.hidden_size
        cos, sin = self.rope(st.Tmax)
        st.ensure_scratch(d, "ord_sw")
        eps = d.rms_norm_eps
        o = torch.empty((st.rows, Hq * hd), dtype=torch.bfloat16, device=x.device)
        bufs = (x, st.x_mid)
        n = d.num_hidden_layers
        for i in range(n):
            xin, xout = bufs[i & 1], bufs[(i + 1) & 1]
            ops.decode_gemv_resid_norm_ord_(xin, None if i == 0 else st.down_part, fp.p(f"l{i}.ln1"), xout, st.ss_part, fp.w(f"l{i}.wqkv"),
                                            st.qkv_part)
            ops.attn_decode_fused_ord(st.qkv_part, st.ss_part, eps, H, fp.w(f"l{i}.bqkv"), cos, sin, st.pos, st.k[i], st.v[i], st.key_valid, o,
                                      Hq, Hk, hd, st.Tmax)
            ops.decode_sw_resid_(o, fp.w(f"l{i}.wo"), xout)
            ops.decode_sw_gate_up_(xout, fp.p(f"l{i}.ln2"), eps, fp.w(f"l{i}.wgu"), st.act)
            ops.decode_sw_kblock_ord_(st.act, fp.w(f"l{i}.wdown"), st.down_part)
        return bufs[n & 1], st.down_part

    def _decode_layers_sw(self, st, x, attn=ops.attn_decode_fused):
        """The decoder stack of one decode step, five launches per layer (measured forms: profiles/r06_decode_forms.md):
          q/k/v      split-K (operand = the stream + the previous layer's pending down projection; leaves a raw accumulator)
          attention  finishes q/k/v from that accumulator, appends k / v, attends to the cache
          o          single writer: the stream is FINISHED in place
          gate/up    single writer: act = SwiGLU, finished bf16
          down       split-K (k-blocks, LDS pre-reduction) on act into this layer's accumulator; clears the accumulators consumed so far
        -> (stream, pending): the residual stream after the last layer is stream + bf16round(pending).
        Accumulators: layer i adds into accd[i & 1] and clears accd[(i + 1) & 1].  `pending` is accd[(n - 1) & 1]; its reader may
        leave it uncleared (the head launch of decode_step_logits does).  At even depth that is accd[1], which layer 0's down projection
        clears; at odd depth it is accd[0], the one layer 0 adds into, so layer 0's q/k/v launch clears it first (even depth: no clear).
        attn: the attention launch -- ops.attn_decode_fused, or ops.attn_decode_seq for a speculative verify step (spec_step); the two
        take the same arguments."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        R, H = st.step_rows, d.hidden_size
        cos, sin = self.rope(st.Tmax)
        st.ensure_scratch(d, "sw")
        eps = d.rms_norm_eps
        o = torch.empty((R, Hq * hd), dtype=torch.bfloat16, device=x.device)
        bufs, accd = (x, st.x_mid), (st.acc_down, st.acc_down2)
        n = d.num_hidden_layers
        # down projection: k-blocks of seven slabs with the partial tiles pre-reduced in LDS (5 atomics per output for the 1.5B model
        # instead of 35: 7.6 vs 8.9 us) when the intermediate size is a whole number of them, else one slab per wave
        down = ops.decode_sw_kblock_ if d.intermediate_size % 1792 == 0 else ops.decode_gemv_
        for i in range(n):
            xin, xout = bufs[i & 1], bufs[(i + 1) & 1]
            pend = st.zeros if i == 0 else accd[(i - 1) & 1]
            # odd depth: the last layer's accumulator is accd[0], which layer 0's down projection adds into next; the previous step's
            # head reads it without clearing it, so layer 0's q/k/v launch clears it (even depth: layer 0's down clears accd[1] itself)
            clr = accd[0] if i == 0 and n & 1 else None
            ops.decode_gemv_resid_norm_(xin, pend, fp.p(f"l{i}.ln1"), xout, st.ss_attn, fp.w(f"l{i}.wqkv"), st.acc_qkv, zero1=clr)
            attn(st.acc_qkv, st.ss_attn, eps, H, fp.w(f"l{i}.bqkv"), cos, sin, st.pos, st.k[i], st.v[i], st.key_valid, o, Hq, Hk, hd, st.Tmax)
            ops.decode_sw_resid_(o, fp.w(f"l{i}.wo"), xout)
            ops.decode_sw_gate_up_(xout, fp.p(f"l{i}.ln2"), eps, fp.w(f"l{i}.wgu"), st.act)
            down(st.act, fp.w(f"l{i}.wdown"), accd[i & 1], zero0=st.acc_qkv, zero1=accd[(i + 1) & 1], ss_zero=st.ss_attn)
        return bufs[n & 1], accd[(n - 1) & 1]

    def _decode_layers_splitk(self, st, x, attn=ops.attn_decode_fused):
        """The decoder stack of one decode step as five split-K launches per layer (see include/unigen_hip.h): a split-K projection leaves
        its raw fp32 accumulator behind and the NEXT kernel applies bias / RoPE / residual add / RMSNorm / SiLU-mul while it builds its
        own operand, so kernel boundaries are the only synchronisation.
        -> (stream, pending): the residual stream after the last layer is stream + bf16round(pending = st.acc_down).  attn: as in _decode_layers_sw."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        R, H, eps = st.step_rows, d.hidden_size, d.rms_norm_eps
        cos, sin = self.rope(st.Tmax)
        st.ensure_scratch(d, "splitk")
        o = torch.empty((R, Hq * hd), dtype=torch.bfloat16, device=x.device)
        for i in range(d.num_hidden_layers):
            # x (+ pending down_proj of the previous layer) -> x_mid ; q/k/v accumulator ; clears gate_up acc
            ops.decode_gemv_resid_norm_(x, st.acc_down, fp.p(f"l{i}.ln1"), st.x_mid, st.ss_attn, fp.w(f"l{i}.wqkv"), st.acc_qkv,
                                        zero0=st.acc_gu, ss_zero=st.ss_mlp)
            attn(st.acc_qkv, st.ss_attn, eps, H, fp.w(f"l{i}.bqkv"), cos, sin, st.pos, st.k[i], st.v[i], st.key_valid, o, Hq, Hk, hd, st.Tmax)
            ops.decode_gemv_(o, fp.w(f"l{i}.wo"), st.acc_o, zero0=st.acc_qkv, zero1=st.acc_down, ss_zero=st.ss_attn)
            # x_mid + pending o_proj -> x ; gate/up accumulator
            ops.decode_gemv_resid_norm_(st.x_mid, st.acc_o, fp.p(f"l{i}.ln2"), x, st.ss_mlp, fp.w(f"l{i}.wgu"), st.acc_gu)
            ops.decode_gemv_swiglu_(st.acc_gu, st.ss_mlp, eps, H, fp.w(f"l{i}.wdown"), st.acc_down, zero0=st.acc_o)
        return x, st.acc_down

    def _decode_layers(self, form, st, x, **how):
        layers = {"sw": self._decode_layers_sw, "splitk": self._decode_layers_splitk, "ord_sw": self._decode_layers_ord}
        return layers[form](st, x, **how)

    def decode_step_logits(self, st, x, w_head, logits):
        """decode_step + the head slice in one go: logits fp32 [rows, N] = rows `w_head` of the tied embedding applied to the final-norm
        hidden state; advances st.pos / st.len.  Exists for the forms sw, ord_sw and ord_wide; splitk and wide have no head launch and
        are refused before anything is launched (nothing is appended to the cache).
        sw: the final RMSNorm and the last layer's pending residual add ride in the head launch's prologue.  ord_sw: the last layer's
        down slots are summed in order by their own launch ahead of the head.  ord_wide: the wide step, then an ordered skinny GEMV."""
        d, fp = self.dims, self.fp
        form = self.decode_form(st.rows, st.deterministic)
        if form in ("splitk", "wide"):
            raise UniGenHipError(f"decode_step_logits: {st.rows} rows on this engine take the {form} decode form, which has no head "
                                 f"launch (decode_step + a head GEMV serve it)")
        self.last_decode_deterministic = st.deterministic
        if form == "ord_wide":
            return ops.skinny_linear_ord(self._decode_step_wide(st, x), w_head, out_f32=logits)
        stream, pending = self._decode_layers(form, st, x)
        if form == "ord_sw":
            ops.decode_finish_resid_norm_ord_(pending, stream, fp.p("norm"), None, d.rms_norm_eps)
            pending = None
        ops.decode_sw_head_(stream, fp.p("norm"), d.rms_norm_eps, w_head, logits, pend=pending, advance=(st.pos, st.len))
        return logits

    def decode_step_head(self, form, st, x, w_head, logits):
        """One decode step on (st, x) that leaves the fp32 head logits for the rows `w_head` of the tied embedding in `logits`; advances
        the cache position.  The ONE statement of which layer forms end in a head launch: sw, ord_sw and ord_wide do
        (decode_step_logits); splitk and wide run decode_step and the atomic GEMV head, which ADDS into `logits` -- the consumer
        (sampler or pick launch) leaves it zeroed."""
        if form in ("splitk", "wide"):
            return ops.decode_gemv_(self.decode_step(st, x), w_head, logits)
        return self.decode_step_logits(st, x, w_head, logits)

    def first_head(self, st, hn, w_head, logits):
        """The first token's head, from the prefill's final-norm hidden state: the ordered skinny linear on a deterministic state, else
        the atomic GEMV, which adds into `logits` (zeroed by the caller or left zeroed by the previous sampler launch)."""
        if st.deterministic:
            return ops.skinny_linear_ord(hn, w_head, out_f32=logits)
        return ops.decode_gemv_(hn, w_head, logits)

    def storage_key(self, capacity):
        """What both decode sessions' keys end in, standing for "the weights were not reallocated": every pointer a captured step bakes
        in lives in the two flat buffers, so their first tensors, the last layer's weights and the RoPE tables for `capacity` serve."""
        fp = self.fp
        return (fp.w("embed").data_ptr(), fp.w("l0.wqkv").data_ptr(), fp.p("embed").data_ptr(), fp.p("norm").data_ptr(),
                fp.w(f"l{self.dims.num_hidden_layers - 1}.wdown").data_ptr(), tuple(t.data_ptr() for t in self.rope(capacity)))

    # ---- AR image decode on the device: head slice into a raw accumulator + ONE sampler launch per token (CFG mix, temperature,
    # softmax, truncation, inverse-CDF draw on the call's uniforms, log-probabilities, next input embedding)
    def ar_draw(self, sess):
        """the sampler launch of an AR step on sess.acc_head (include/unigen_hip.h: ug_ar_sample / ug_ar_sample_filtered and their
        _logp entry points); leaves the accumulator zeroed"""
        args = (sess.acc_head, sess.bsz, sess.V, sess.guidance_scale, sess.temperature, sess.greedy, sess.uniforms, sess.st.pos, sess.P,
                sess.n, self.fp.p("embed"), sess.code_lo, sess.tok, sess.out_tokens, sess.x)
        if sess.filt is None:
            ops.ar_sample_(*args, logp=sess.logp)
        else:
            ops.ar_sample_filtered_(*args, top_k=sess.filt[0], top_p=sess.filt[1], min_p=sess.filt[2], logp=sess.logp)

    def _ar_head_rows(self, sess):
        return self.fp.w("embed")[sess.code_lo:sess.code_lo + sess.V]

    def _ar_trace(self, sess, trace):
        # parity tests follow the head's raw logits step by step (eager runs only)
        if trace is not None and not torch.cuda.is_current_stream_capturing():
            trace.append(sess.acc_head.clone())

    def ar_first_token(self, sess, hn, trace=None):
        """token 0 from the prefill's final-norm hidden state: first_head into the accumulator + the sampler launch"""
        self.first_head(sess.st, hn, self._ar_head_rows(sess), sess.acc_head)
        self._ar_trace(sess, trace)
        self.ar_draw(sess)

    def ar_step(self, sess, trace=None):
        """One AR decode step into the session's static buffers: decode_step_head on sess.x into the accumulator, then the sampler
        launch (token, record, next sess.x).  No host sync, no shape depends on the step: capturable."""
        self.decode_step_head(sess.form, sess.st, sess.x, self._ar_head_rows(sess), sess.acc_head)
        self._ar_trace(sess, trace)
        self.ar_draw(sess)

    # ---- text decode on the device: head + pick over the whole vocabulary, the token loop's state in device memory
    def text_pick(self, sess):
        """the pick launch(es) of a text step on sess.logits (include/unigen_hip.h: ug_text_pick / ug_text_sample).  The atomic GEMV
        head of the splitk and wide forms needs its accumulator back zeroed: clear=1 there."""
        kw = dict(clear=sess.form in ("splitk", "wide"), stop_ids=sess.stop_ids, pad_id=sess.pad_id, lengths=sess.lengths)
        if sess.logp is not None:
            kw["logp"] = sess.logp                  # (the _logp entry points; without the buffer the launches are what they were)
        emb = self.fp.p("embed")
        if sess.sampling is None:
            ops.text_pick_(sess.logits, sess.V, sess.state, sess.width, emb, sess.tok, sess.out_tokens, sess.x, **kw)
        else:
            t, k, p = sess.sampling
            ops.text_sample_(sess.logits, sess.V, sess.state, sess.width, emb, sess.tok, sess.out_tokens, sess.x, sess.uniforms, sess.workspace,
                             temperature=t, top_k=k, top_p=p, **kw)

    def text_penalize(self, sess, first=False):
        """the logits processor of a text step, between head and pick: the session's repetition penalty on sess.logits (nothing without
        one).  Token 0 has no previous step (tok = null); every later step passes sess.tok, a constant of the captured graph."""
        if sess.seen is not None:
            ops.text_penalize_(sess.logits, sess.V, sess.penalty, sess.seen, tok=None if first else sess.tok)

    def text_constrain(self, sess):
        """the constraints of a text step, ahead of the penalty (include/unigen_hip.h: ug_text_constrain); nothing without any"""
        if sess.constrained:
            ops.text_constrain_(sess.logits, sess.V, sess.state, sess.out_tokens, bias=sess.bias, min_new=sess.min_new,
                                stop_ids=sess.stop_ids if sess.min_new else None, ngram=sess.ngram, hist=sess.hist, hist_len=sess.hist_len)

    def text_stop_seq(self, sess):
        """the stop sequences of a text step, behind the pick (include/unigen_hip.h: ug_text_stop_seq); nothing without any"""
        if sess.stop_seqs is not None:
            ops.text_stop_seq_(sess.stop_seqs[0], sess.stop_seqs[1], sess.out_tokens, sess.state, lengths=sess.lengths)

    def text_first_token(self, sess, hn, trace=None):
        """token 0 from the prefill's final-norm hidden state: the GEMV head (ordered in deterministic mode) + the constraints + the
        logits processor + the pick + the stop sequences.  trace takes the RAW head logits."""
        if not sess.st.deterministic:
            sess.logits.zero_()                     # (the atomic GEMV adds into it)
        self.first_head(sess.st, hn, self.fp.w("embed")[:sess.V], sess.logits)
        if trace is not None:
            trace.append(sess.logits[:, :sess.V].clone())
        self.text_constrain(sess)
        self.text_penalize(sess, first=True)
        self.text_pick(sess)
        self.text_stop_seq(sess)

    def text_step(self, sess, trace=None):
        """One text decode step into the session's static buffers: the decoder stack on sess.x, the head over the whole vocabulary and
        the pick (token, stop rule, records, next sess.x), the session's constraints and logits processor between them, its stop
        sequences behind the pick; advances the cache position.  No host sync, no shape depends on the step:
        capturable.  The head is decode_step_head's, into the logits the pick leaves zeroed where the form's head adds.  trace: optional
        list taking the step's raw head logits (eager runs only)."""
        self.decode_step_head(sess.form, sess.st, sess.x, self.fp.w("embed")[:sess.V], sess.logits)
        if trace is not None and not torch.cuda.is_current_stream_capturing():
            trace.append(sess.logits[:, :sess.V].clone())
        self.text_constrain(sess)
        self.text_penalize(sess)
        self.text_pick(sess)
        self.text_stop_seq(sess)

    # ---- prompt-lookup speculative decoding of one greedy row: a verify step runs the decoder stack on S consecutive positions
    def spec_form(self, S):
        """The layer form of a verify step on S rows: sw or splitk.  The other forms are refused by name before any launch (wide has
        no fused attention launch to stand ug_attn_decode_seq in for; there is no ordered ug_attn_decode_seq)."""
        form = self.decode_form(S, False)
        if form not in ("sw", "splitk"):
            raise UniGenHipError(f"prompt_lookup_num_tokens: this engine's decode steps take the {form} form; speculative decoding "
                                 f"serves the sw and splitk forms only")
        return form

    def _spec_verify(self, sess, rows, advance):
        ops.spec_verify_(sess.logits, rows, sess.V, sess.state, sess.n, self.fp.p("embed"), sess.tok, sess.out_tokens, sess.x, sess.hist,
                         sess.G, sess.K, clear=sess.form == "splitk", stop_ids=sess.stop_ids, lengths=sess.lengths, advance=advance)

    def spec_first_token(self, sess, hn):
        """token 0 from the prefill's final-norm hidden state, as text_first_token picks it (the GEMV head into the zeroed row 0), pushed
        through the verify entry with no draft and no advance: it lands in the history, so the first draft exists before step 1."""
        self.first_head(sess.st, hn, self.fp.w("embed")[:sess.V], sess.logits[:1])
        self._spec_verify(sess, 1, None)

    def spec_step(self, sess):
        """One verify step into the session's static buffers: the decoder stack on the S rows of sess.x in the session's form with
        ug_attn_decode_seq where the form has ug_attn_decode_fused, the head with NO position advance, then ug_spec_verify, which owns
        the advance (by the number of tokens emitted).  Always all S rows -- the weight stream dominates, and a fixed shape gives one
        captured graph.  No host sync, no shape depends on the step: capturable.
        Stale keys: a rejected row's k / v stay in the cache at positions >= the new position p'.  Nothing reads at or past p' (a step
        attends to the cache keys below its position and to its own rows from the accumulator), and the next step overwrites
        [p', p' + S), which covers every row this step wrote: a stale key is never visible."""
        d, fp, st = self.dims, self.fp, sess.st
        self.last_decode_deterministic = False
        stream, pending = self._decode_layers(sess.form, st, sess.x, attn=ops.attn_decode_seq)
        w_head = fp.w("embed")[:sess.V]
        if sess.form == "sw":
            ops.decode_sw_head_(stream, fp.p("norm"), d.rms_norm_eps, w_head, sess.logits, pend=pending, advance=None)
        else:
            hn = torch.empty((sess.S, d.hidden_size), dtype=torch.bfloat16, device=stream.device)
            ops.decode_finish_resid_norm_(pending, stream, fp.p("norm"), hn, d.rms_norm_eps, advance=None)
            ops.decode_gemv_(hn, w_head, sess.logits)
        self._spec_verify(sess, sess.S, (st.pos, st.len))

    def decode_step(self, st, x):
        """x fp32 [rows, H] = embedding of the newest token (updated in place as the residual stream);
        appends its K/V at st.pos, ADVANCES st.pos / st.len by one and returns the final-norm hidden bf16 [rows, H].  No host sync, no
        shape depends on the step: capturable.  decode_form picks the layer form; its finisher adds the last layer's pending down
        projection, applies the final RMSNorm and clears what the next step expects cleared."""
        d, fp = self.dims, self.fp
        self.last_decode_deterministic = st.deterministic
        form = self.decode_form(st.rows, st.deterministic)
        if form in ("wide", "ord_wide"):
            return self._decode_step_wide(st, x)
        hn = torch.empty((st.rows, d.hidden_size), dtype=torch.bfloat16, device=x.device)
        stream, pending = self._decode_layers(form, st, x)
        finish = ops.decode_finish_resid_norm_ord_ if form == "ord_sw" else ops.decode_finish_resid_norm_
        finish(pending, stream, fp.p("norm"), hn, d.rms_norm_eps, advance=(st.pos, st.len))
        return hn

    def _decode_step_wide(self, st, x):
        """The wide and ord_wide forms: the GEMV kernels do not apply; split-K GEMMs + separate finishing kernels.  Deterministic state: every
        projection is the ordered skinny linear (per-k-slice partial slots in blocks of 32 rows, summed in slice order)."""
        d, fp = self.dims, self.fp
        Hq, Hk, hd = d.num_attention_heads, d.num_key_value_heads, d.head_dim
        cos, sin = self.rope(st.Tmax)
        lin = ops.skinny_linear_ord if st.deterministic else ops.skinny_linear
        for i in range(d.num_hidden_layers):
            xn, _ = ops.rmsnorm_fwd(x, fp.p(f"l{i}.ln1"), d.rms_norm_eps, want_rstd=False)
            qkv = lin(xn, fp.w(f"l{i}.wqkv"), bias=fp.w(f"l{i}.bqkv"))
            ops.rope_at_(qkv, cos, sin, Hq + Hk, hd, st.pos)
            ops.kv_store(qkv, st.k[i], st.v[i], st.rows, 1, Hq, Hk, hd, st.Tmax, st.pos, 0)
            o = ops.attn_decode(qkv, st.k[i], st.v[i], st.key_valid, Hq, Hk, hd, st.Tmax, st.len)
            lin(o, fp.w(f"l{i}.wo"), resid=x)
            xn2, _ = ops.rmsnorm_fwd(x, fp.p(f"l{i}.ln2"), d.rms_norm_eps, want_rstd=False)
            gu = lin(xn2, fp.w(f"l{i}.wgu"))
            act = ops.swiglu_fwd(gu)
            lin(act, fp.w(f"l{i}.wdown"), resid=x)
        hn, _ = ops.rmsnorm_fwd(x, fp.p("norm"), d.rms_norm_eps, want_rstd=False)
        st.advance()
        return hn

    def head_slice(self, hn, v0, v1):
        """logits bf16 [rows, v1-v0] for vocabulary rows [v0, v1) of the tied embedding."""
        n = v1 - v0
        out = torch.empty((hn.shape[0], ops.round_up(n, 8)), dtype=torch.bfloat16, device=self.device)
        ops.gemm(hn, self.fp.w("embed")[v0:v1], out=out, N=n, K=self.dims.hidden_size)
        return out[:, :n]
