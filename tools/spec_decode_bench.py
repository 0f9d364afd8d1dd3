"""Prompt-lookup speculative decoding at full scale on ONE GPU: the 28-layer 1.5B model (device-side random init, as
tools/text_bench.py), one row, a causal prompt of 768 ids, 256 new greedy tokens through `generate(on_device=True)`.  Four runs,
alternating in one process:

  plain       the plain device loop (one row per step)
  spec_high   prompt_lookup_num_tokens=7 with lookup_ids = the plain run's own output: acceptance near its ceiling
  spec_self   the same with lookup_ids = the output of a speculative call of its own.  With random weights nearly every step of the
              greedy chain is a near-tie, so the 8-row step leaves the one-row step's chain within a few tokens and spec_high finds
              little to accept; the verify step's own chain is what a verify step reproduces (up to the atomics' order)
  spec_low    prompt_lookup_num_tokens=7, max_matching_ngram_size=4 on a prompt given as EMBEDDINGS with no lookup_ids: nothing to look
              up but the run's own tokens, acceptance as low as this model's output allows (random weights repeat themselves; the
              figure is reported, not assumed)

Every visit to a run makes two calls and times the second (it replays the graph the first one captured: the kept session's key
holds the call's constants), then a one-token call of the same run for the prefill + first token.  One untimed visit each, then five
timed.  A call's decode time is its wall time (host clock between device synchronisations) minus the median one-token call; the time
per step divides it by the steps behind the first token -- 255 for the plain loop, `last_spec_stats["steps"]` for the speculative ones
-- and tokens/s by the 255 tokens those steps emitted.

One JSON line: per run every call's time, ms per step and tokens/s, the speculative runs' counters, and from the medians
verify_step_over_plain_step (what an 8-row verify step costs against a one-row step) and the speed-up in tokens/s.

    python tools/spec_decode_bench.py
"""
import json
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ml-unigen_amd"))
import torch
from bench import CODEBOOK, NVQ, TEXT_VOCAB, VOCAB
from models import UniGen

NEW, L, K = 256, 768, 7


def main(rounds=5):
    dev = torch.device("cuda:0")
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                   codebook_size=CODEBOOK, num_vq_tokens=NVQ, device=dev, init_seed=-1)
    model.llm.init_weights_device(1)
    model.eval()
    eng = model.llm.engine
    ids = torch.randint(0, 151643, (1, L), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    emb = model.llm.model.embed_tokens(ids).float()
    plain_out = model.generate(input_ids=ids, max_new_tokens=NEW, on_device=True)[0, L:].clone()
    spec_out = model.generate(input_ids=ids, max_new_tokens=NEW, prompt_lookup_num_tokens=K)[0, L:].clone()
    runs = {"plain": dict(input_ids=ids),
            "spec_high": dict(input_ids=ids, prompt_lookup_num_tokens=K, lookup_ids=plain_out),
            "spec_self": dict(input_ids=ids, prompt_lookup_num_tokens=K, lookup_ids=spec_out),
            "spec_low": dict(input_embeddings=emb, prompt_lookup_num_tokens=K, max_matching_ngram_size=4)}

    def call(name, new=NEW):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(max_new_tokens=new, on_device=True, **runs[name])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert out.shape[1] == new + (0 if "input_embeddings" in runs[name] else L) and eng.last_text_decode_on_device
        return dt, (dict(eng.last_spec_stats) if name != "plain" else {"steps": new - 1, "emitted": new})

    times, first, stats = ({name: [] for name in runs} for _ in range(3))
    for visit in range(rounds + 1):
        for name in runs:
            call(name)                                   # captures: another run's session was the kept one
            (t, st), (t1, _) = call(name), call(name, 1)
            if visit:
                times[name].append(t)
                first[name].append(t1)
                stats[name].append(st)
    rec = {}
    for name in runs:
        f = statistics.median(first[name])
        steps = [st["steps"] for st in stats[name]]
        step_ms = [1e3 * (t - f) / s for t, s in zip(times[name], steps)]
        rec[name] = {"call_s": [round(t, 4) for t in times[name]], "first_token_call_s": round(f, 4), "steps": steps,
                     "ms_per_step": [round(m, 4) for m in step_ms],
                     "tokens_per_s": [round((NEW - 1) / (t - f), 1) for t in times[name]]}
        if name != "plain":
            rec[name]["stats"] = stats[name]
            rec[name]["tokens_per_step"] = round((NEW - 1) / statistics.median(steps), 3)
    med = lambda name, field: statistics.median(rec[name][field])
    for name in ("spec_high", "spec_self", "spec_low"):
        rec[name]["verify_step_over_plain_step"] = round(med(name, "ms_per_step") / med("plain", "ms_per_step"), 4)
        rec[name]["tokens_per_s_over_plain"] = round(med(name, "tokens_per_s") / med("plain", "tokens_per_s"), 4)
    same = (plain_out == spec_out).int().tolist()
    prefix = same.index(0) if 0 in same else NEW         # how far the two greedy chains run together before a near-tie parts them
    print(json.dumps({"prompt": L, "new_tokens": NEW, "prompt_lookup_num_tokens": K, "form": eng.decode_form(K + 1, False),
                      "plain_and_spec_common_prefix": prefix, **rec}))


if __name__ == "__main__":
    main()
