"""What sharing the image prefix buys the CoT-V rating loop (reference evaluation/inference_unigen_cot.py:308-415) on ONE GPU: the
28-layer 1.5B dims with seeded weights, one prefix of 760 positions (20 system ids, a 729-position bidirectional image block, 11
more ids), 8 questions of 24 .. 40 ids left-padded to 40, 4 new tokens each, greedy, token loop on the device.  Median of 5 calls
after 2 warm-ups, in ms per question set:
  (a) mmu_generate_batch on the full rows [prefix | pads | question] under dense masks -- every row prefills the prefix again;
  (b) mmu_prefix once + mmu_generate_batch(prefix=...);
  (c) (b) with the prefix kept from a previous call.
and the parts of (b): prefix prefill, the copy of the prefix rows into the call's cache, the tail prefill, the rest (decode).
Every phase runs under a time limit of its own.  Prints a markdown record (and writes it to --out).

    python3 tools/mmu_prefix_rate.py --commit <hash> --out profiles/mmu_shared_prefix.md"""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ml-unigen_amd"))
import torch
from bench import CODEBOOK, NVQ, TEXT_VOCAB, VOCAB, PowerSampler
from models import UniGen

P, IMG0, IMG1 = 760, 20, 749
R, S, NEW = 8, 40, 4
WARM, CALLS = 2, 5
PHASE_LIMIT_S = 120


class _Limit:
    """a phase that runs longer than its limit raises TimeoutError"""

    def __init__(self, name, seconds=PHASE_LIMIT_S):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def fire(*_):
            raise TimeoutError(f"phase '{self.name}' ran past its limit of {self.seconds} s")
        signal.signal(signal.SIGALRM, fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def median_ms(name, fn):
    with _Limit(name):
        out = []
        for i in range(WARM + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with _Limit("model", 300):
        model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                       codebook_size=CODEBOOK, num_vq_tokens=NVQ, device=dev, init_seed=-1)
        model.llm.init_weights_device(1)
        model.eval()
    eng = model.llm.engine
    g = torch.Generator().manual_seed(3)
    pre = torch.randint(0, 151643, (1, P), generator=g)
    lens = [24 + (16 * r) // (R - 1) for r in range(R)]                                   # 24 .. 40
    tails = torch.zeros((R, S), dtype=torch.long)
    tv = torch.zeros((R, S), dtype=torch.bool)
    for r, n in enumerate(lens):
        tails[r, S - n:] = torch.randint(0, 151643, (n,), generator=g)
        tv[r, S - n:] = True
    L = P + S
    r_ = torch.arange(L)
    causal = r_[None, :] <= r_[:, None]
    image = (r_[None, :] >= IMG0) & (r_[None, :] < IMG1) & (r_[:, None] >= IMG0)          # the image block: visible from its start on
    kv = torch.cat([torch.ones(R, P, dtype=torch.bool), tv], 1)
    allow = ((causal | image)[None] & kv[:, None, :]) | torch.eye(L, dtype=torch.bool)[None]
    neg = torch.finfo(torch.float32).min
    dense_mask = torch.where(allow, 0.0, neg)[:, None].contiguous().to(dev)
    pre_mask = torch.where((causal | image)[:P, :P], 0.0, neg)[None, None].contiguous().to(dev)
    full = torch.cat([pre.expand(R, P), tails], 1).to(dev)
    pre, tails, tv = pre.to(dev), tails.to(dev), tv.to(dev)
    kw = dict(max_new_tokens=NEW, temperature=0.0, on_device=True)

    sampler = PowerSampler()
    w0 = time.time()
    a = median_ms("a: full rows", lambda: model.mmu_generate_batch(idx=full, attention_mask=dense_mask, **kw))
    rows_a = model.mmu_generate_batch(idx=full, attention_mask=dense_mask, **kw)
    b = median_ms("b: prefix + tails", lambda: model.mmu_generate_batch(
        idx=tails, prefix=model.mmu_prefix(idx=pre, attention_mask=pre_mask), tail_valid=tv, **kw))
    prefix = model.mmu_prefix(idx=pre, attention_mask=pre_mask)
    c = median_ms("c: kept prefix", lambda: model.mmu_generate_batch(idx=tails, prefix=prefix, tail_valid=tv, **kw))
    rows_c = model.mmu_generate_batch(idx=tails, prefix=prefix, tail_valid=tv, **kw)
    # ---- the parts of (b)
    from unigen_hip.qwen2 import DecodeState
    t_prefix = median_ms("prefix prefill", lambda: model.mmu_prefix(idx=pre, attention_mask=pre_mask))
    st = DecodeState(eng.dims, R, 896, dev, key_valid=kv)

    def copy():
        for i in range(len(st.k)):
            st.k[i][:, :, :P].copy_(prefix.st.k[i][:, :, :P])
            st.v[i][:, :, :P].copy_(prefix.st.v[i][:, :, :P])
    t_copy = median_ms("copy", copy)
    emb = model.llm.model.embed_tokens(tails).float()
    kvd = kv.to(dev)
    t_tail = median_ms("tail prefill", lambda: eng.prefill_onto(st, emb, P, kvd))
    power = sampler.report(w0, time.time())
    same = sum(int([int(t) for t in x] == [int(t) for t in y]) for x, y in zip(rows_a, rows_c))

    lines = ["# Shared-prefix mmu generation: one image prefix, 8 questions", "",
             f"`tools/mmu_prefix_rate.py`, commit {args.commit}, one MI355X.  28-layer 1.5B dims, seeded weights; prefix {P} positions "
             f"({IMG1 - IMG0}-position bidirectional image block), {R} questions of {lens[0]} .. {lens[-1]} ids left-padded to {S}, {NEW} new "
             f"tokens, greedy, token loop on the device (captured step).  Median of {CALLS} calls after {WARM} warm-ups.", "",
             "| form | ms per question set |", "|---|---|",
             f"| (a) `mmu_generate_batch` on the full rows ({R} x {L}, dense masks) | {a:.1f} |",
             f"| (b) `mmu_prefix` + `mmu_generate_batch(prefix=...)` | {b:.1f} |",
             f"| (c) (b) with the prefix kept from a previous call | {c:.1f} |", "",
             f"(b) / (a) = {b / a:.2f}, (c) / (a) = {c / a:.2f}.  " +
             ("(b) is below (a), the direction expected." if b < a else "(b) is NOT below (a): the expected direction does not hold here."), "",
             f"Parts of (b), each timed alone: prefix prefill {t_prefix:.1f} ms, copy of the prefix rows into the call's cache "
             f"({R} rows x {eng.dims.num_hidden_layers} layers) {t_copy:.1f} ms, tail prefill ({R} x {S} rows onto {P}) {t_tail:.1f} ms, "
             f"rest (first token, {NEW - 1} decode steps, host side) {b - t_prefix - t_copy - t_tail:.1f} ms.", "",
             f"Rows whose {NEW} tokens are equal between (a) and (c): {same} of {R} (random weights: near-ties may fall either way).", "",
             f"Power: {power}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
