"""Text decode at full scale on ONE GPU: the host token loop against the on-device loop (on_device=True), alternating in one
process.  Model and prompts as tools/mmu_bench.py: the 1.5B model, device-side random init, R prompts of 768 tokens under the mmu
mask; 64 new tokens, no stop id, through mmu_generate_batch.  Rows 1 and 16 (ROWS=1,16).  Per setting: two warm-up calls of each
loop, then five timed calls of each, alternating.  A call's decode time is its wall time minus the same loop's one-token call
(prefill + first token, the median of three), over the 63 steps behind the first token.

Settings: greedy; greedy in deterministic mode; sampled (temperature 1.0, top_k 50: the shape of the CoT-V call); greedy with a stop
id no row produces (prices the on-device loop's poll of `remaining` every 8 tokens against the host loop's sync per token).

One JSON line: per rows and setting, every call's tokens/s and ms per step for both loops, and the ratio of the medians.

    python tools/text_bench.py --repetition-penalty P

times the ON-DEVICE loop alone, greedy, with the logits processor (repetition_penalty=P: one ug_text_penalize launch per step, one
ug_text_seen_mark per call) against the same build without it, alternating in one process.  The penalty is part of the kept
session's key, so each visit to a mode makes two calls and times the second (it replays the graph the first one captured), then
one one-token call of the same session for the prefill + first token.  Five visits per mode after one untimed visit each.

    python tools/text_bench.py --constraints

the same pairing for the constraints (one ug_text_constrain launch per step ahead of the penalty, one ug_text_stop_seq launch behind the
pick): all off against logit_bias (64 ids), suppress_tokens (64 ids), min_new_tokens (with a stop id no row produces, which the "off"
of that pair carries too), no_repeat_ngram_size=3 (the 768 prompt ids are the history), stop_sequences (8 of 16 ids no row produces), and
all five at once.

    python tools/text_bench.py --beam

beam_search(num_beams=4) on 8 prompts (32 rows) against the host loop of generate(do_sample=True, num_return_sequences=4) on the same
32 rows, alternating in one process: causal prompts of 768 ids, 64 new tokens, no eos.  Two warm-up calls of each, five timed; a
call's decode time is its wall time minus the median of three one-token calls of the same entry point.  The line carries the power and
clock sample of bench.py's PowerSampler over the timed calls (null where the hwmon files are missing or the card stayed under 300 W)."""
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

NEW, L = 64, 768
SETTINGS = {
    "greedy": dict(temperature=0.0),
    "greedy_deterministic": dict(temperature=0.0, deterministic=True),
    "sampled_t1_k50": dict(temperature=1.0, top_k=50),
    "greedy_stop_never_hit": dict(temperature=0.0, eot_token=VOCAB - 1),          # (the mask token: the backbone's argmax never lands there)
}


def penalty_pair(penalty, rounds=5):
    paired((("off", {}), ("on", dict(repetition_penalty=float(penalty)))), {"repetition_penalty": penalty}, rounds)


def constraint_modes():
    ids = list(range(1000, 1064))
    never = VOCAB - 1                                # (the mask token: the backbone's argmax never lands there)
    seqs = [[never - 1 - j for j in range(16)] for _ in range(8)]
    each = {"logit_bias": dict(logit_bias={e: 0.5 for e in ids}), "suppress_tokens": dict(suppress_tokens=[e + 1000 for e in ids]),
            "min_new_tokens": dict(min_new_tokens=32, eot_token=never), "no_repeat_ngram_size": dict(no_repeat_ngram_size=3),
            "stop_sequences": dict(stop_sequences=seqs)}
    every = {k: v for kw in each.values() for k, v in kw.items()}
    return (("off", {}), ("off_with_stop_id", dict(eot_token=never))) + tuple(each.items()) + (("all", every),)


def paired(modes, label, rounds=5):
    dev = torch.device("cuda:0")
    rows = [int(r) for r in os.environ.get("ROWS", "1,16").split(",")]
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                   codebook_size=CODEBOOK, num_vq_tokens=NVQ, device=dev, init_seed=-1)
    model.llm.init_weights_device(1)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(2)
    r = torch.arange(L, device=dev)
    allow = (r[None, :] <= r[:, None]) | ((r[None, :] >= 20) & (r[None, :] < 749))
    result = {"prompt": L, "new_tokens": NEW, **label, "loop": "device", "setting": "greedy", "rows": {}}
    for R in rows:
        idx = torch.randint(0, 151643, (R, L), device=dev, generator=g)
        mask = torch.where(allow, 0.0, torch.finfo(torch.float32).min)[None, None].expand(R, 1, L, L).contiguous()

        def call(kw, new=NEW):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.mmu_generate_batch(idx=idx, attention_mask=mask, max_new_tokens=new, temperature=0.0, on_device=True, **kw)
            torch.cuda.synchronize()
            assert all(len(o) == new for o in out) and model.llm.engine.last_text_decode_on_device
            return time.perf_counter() - t0

        times, first = {name: [] for name, _ in modes}, {name: [] for name, _ in modes}
        for visit in range(rounds + 1):
            for name, p in modes:
                call(p)                                  # captures: the other mode's session was the kept one
                t, t1 = call(p), call(p, 1)
                if visit:
                    times[name].append(t)
                    first[name].append(t1)
        rec = {}
        for name, _ in modes:
            f = statistics.median(first[name])
            step_ms = [1e3 * (t - f) / (NEW - 1) for t in times[name]]
            rec[name] = {"call_s": [round(t, 4) for t in times[name]], "first_token_call_s": round(f, 4),
                         "ms_per_step": [round(m, 4) for m in step_ms], "tokens_per_s": [round(1e3 * R / m, 1) for m in step_ms]}
        med = lambda name: statistics.median(rec[name]["ms_per_step"])
        for name, _ in modes[1:]:
            rec[name]["over_off_tokens_per_s"] = round(med("off") / med(name), 4)
            rec[name]["extra_us_per_step"] = round(1e3 * (med(name) - med("off")), 2)
        result["rows"][str(R)] = rec
        model.drop_decode_session()
    print(json.dumps(result))


def beam_pair(prompts=8, beams=4, rounds=5):
    from bench import PowerSampler
    dev = torch.device("cuda:0")
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                   codebook_size=CODEBOOK, num_vq_tokens=NVQ, device=dev, init_seed=-1)
    model.llm.init_weights_device(1)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(2)
    ids = torch.randint(0, 151643, (prompts, L), device=dev, generator=g)
    R = prompts * beams

    def call(beam, new=NEW):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if beam:
            out = model.beam_search(input_ids=ids, max_new_tokens=new, num_beams=beams, num_return_sequences=beams)
        else:
            out = model.generate(input_ids=ids, max_new_tokens=new, do_sample=True, top_k=50, num_return_sequences=beams, on_device=False)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (R, L + new)
        return time.perf_counter() - t0

    for _ in range(2):
        call(False), call(True)
    first = {b: statistics.median(call(b, 1) for _ in range(3)) for b in (False, True)}
    times = {False: [], True: []}
    sampler, w0 = PowerSampler(), time.time()
    for _ in range(rounds):
        for b in (False, True):
            times[b].append(call(b))
    power = sampler.report(w0, time.time())
    rec = {}
    for b, tag in ((False, "sampled_host_loop"), (True, "beam_search")):
        step_ms = [1e3 * (t - first[b]) / (NEW - 1) for t in times[b]]
        rec[tag] = {"call_s": [round(t, 4) for t in times[b]], "first_token_call_s": round(first[b], 4),
                    "ms_per_step": [round(m, 4) for m in step_ms], "tokens_per_s": [round(1e3 * R / m, 1) for m in step_ms],
                    "median_tokens_per_s": round(1e3 * R / statistics.median(step_ms), 1)}
    med = lambda tag: statistics.median(rec[tag]["ms_per_step"])
    rec["beam_over_sampled_step_time"] = round(med("beam_search") / med("sampled_host_loop"), 3)
    print(json.dumps({"prompt": L, "new_tokens": NEW, "prompts": prompts, "num_beams": beams, "rows": R, "power": power, **rec}))


def main():
    dev = torch.device("cuda:0")
    rows = [int(r) for r in os.environ.get("ROWS", "1,16").split(",")]
    only = os.environ.get("SETTINGS")
    model = UniGen(w_und_encoder=False, vocab_size=VOCAB, llm_vocab_size=TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                   codebook_size=CODEBOOK, num_vq_tokens=NVQ, device=dev, init_seed=-1)
    model.llm.init_weights_device(1)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(2)
    r = torch.arange(L, device=dev)
    allow = (r[None, :] <= r[:, None]) | ((r[None, :] >= 20) & (r[None, :] < 749))      # mmu_vit mask: image block visible
    result = {"prompt": L, "new_tokens": NEW, "rows": {}}
    for R in rows:
        idx = torch.randint(0, 151643, (R, L), device=dev, generator=g)
        mask = torch.where(allow, 0.0, torch.finfo(torch.float32).min)[None, None].expand(R, 1, L, L).contiguous()
        result["rows"][str(R)] = per_rows = {}
        for name, kw in SETTINGS.items():
            if only and name not in only.split(","):
                continue

            def call(on_device, new=NEW):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.mmu_generate_batch(idx=idx, attention_mask=mask, max_new_tokens=new, on_device=on_device, **kw)
                torch.cuda.synchronize()
                assert all(len(o) == new for o in out)
                return time.perf_counter() - t0

            for _ in range(2):
                call(False), call(True)
            first = {od: statistics.median(call(od, 1) for _ in range(3)) for od in (False, True)}
            times = {False: [], True: []}
            for _ in range(5):
                for od in (False, True):
                    times[od].append(call(od))
            rec = {}
            for od, tag in ((False, "host"), (True, "device")):
                step_ms = [1e3 * (t - first[od]) / (NEW - 1) for t in times[od]]
                rec[tag] = {"call_s": [round(t, 4) for t in times[od]], "first_token_call_s": round(first[od], 4),
                            "ms_per_step": [round(m, 4) for m in step_ms], "tokens_per_s": [round(1e3 * R / m, 1) for m in step_ms]}
            med = lambda tag: statistics.median(rec[tag]["ms_per_step"])
            rec["device_over_host_tokens_per_s"] = round(med("host") / med("device"), 3)
            rec["call_time_ratio_host_over_device"] = round(statistics.median(times[False]) / statistics.median(times[True]), 3)
            per_rows[name] = rec
        model.drop_decode_session()
    print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--repetition-penalty":
        penalty_pair(float(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--constraints":
        paired(constraint_modes(), {"constraints": True})
    elif len(sys.argv) > 1 and sys.argv[1] == "--beam":
        beam_pair()
    else:
        main()
