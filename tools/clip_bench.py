"""Gradient-norm clipping on the 1.5 B model of bench.py (stage-1 configuration): what the step between backward and the optimizer
costs in each form, and the sum-of-squares kernel alone.

    python tools/clip_bench.py [--reps 21] [--json OUT]

1. backward's end -> the optimizer update's end (in-stream update, so one pair of events brackets it), forms alternating in one
   process, median of --reps after 3 warm-ups, each at a threshold that clips (half the norm) and one that does not (twice):
     a  torch.nn.utils.clip_grad_norm_ + FusedAdamW.step()          (the form before the fused kernels)
     b  unigen_hip.optim.clip_grad_norm_ + FusedAdamW.step()        (in place)
     c  FusedAdamW(max_grad_norm=...).step()                        (deferred: the update kernels take the factor)
     d  FusedAdamW.step()                                           (no clipping)
   The gradients are restored from a copy before every timed run (outside the events): the in-place forms rewrite them.
2. ug_sumsq_spans_f32 alone over the backbone's gradient (one span of 1.56 G elements): grids of 256 ... 4096 workgroups, fp64
   against fp32-chain accumulation, bytes per second."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ml-unigen_amd"))
import torch  # noqa: E402

import bench  # noqa: E402  (workload constants and the prompt glue)


def med(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4),
            "iqr_ms": round(xs[(3 * len(xs)) // 4] - xs[len(xs) // 4], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from models import UniGen
    from unigen_hip import ops, optim
    dev = torch.device("cuda:0")
    torch.manual_seed(bench.SEED)
    model = UniGen(w_und_encoder=False, vocab_size=bench.VOCAB, llm_vocab_size=bench.TEXT_VOCAB, llm_model_path="Qwen2.5-1.5B-Instruct",
                   codebook_size=bench.CODEBOOK, num_vq_tokens=bench.NVQ, load_from_pretrained=True, device=dev, init_seed=-1)
    model.llm.init_weights_device(bench.SEED)
    model.train()
    # one small real backward: every parameter gets its gradient view of the flat buffer
    B, T = 1, 61
    g = torch.Generator(device=dev).manual_seed(bench.SEED)
    text = torch.randint(0, 151643, (B, T), device=dev, generator=g)
    codes = torch.randint(0, bench.CODEBOOK, (B, bench.NVQ), device=dev, generator=g) + bench.TEXT_VOCAB
    ids, labels, mask = bench.t2i_rows(ops, text, torch.full_like(codes, bench.MASK_ID), codes)
    _, loss, _, _ = model(input_ids=ids, attention_mask=mask, labels=labels, batch_size_t2i=B, max_seq_length=T + 1, num_vq_tokens=bench.NVQ)
    loss.backward()
    fp = model.llm.engine.fp
    fp.grad.normal_(0.0, 1e-3, generator=g)                 # every gradient "written": dense values of a plausible size
    saved = fp.grad.clone()
    params = list(model.parameters())
    decay = [p for n, p in model.named_parameters() if "bias" not in n]
    nodecay = [p for n, p in model.named_parameters() if "bias" in n]
    opt = optim.FusedAdamW([{"params": decay, "weight_decay": 0.01}, {"params": nodecay, "weight_decay": 0.0}], lr=1e-4)
    n_grad = sum(p.grad.numel() for p in params if p.grad is not None)
    norm0 = optim.clip_grad_norm_(params, 1e30).item()
    ref0 = torch.nn.utils.clip_grad_norm_(params, 1e30).item()
    n_spans = len(optim._plan_for(optim._split_grads([p.grad for p in params if p.grad is not None])[0]).table)
    print(f"{n_grad / 1e9:.3f} G gradient elements in {sum(p.grad is not None for p in params)} tensors, {n_spans} span(s); "
          f"norm {norm0:.6g} (torch {ref0:.6g})")

    def form_a(mx):
        torch.nn.utils.clip_grad_norm_(params, mx)
        opt.step()

    def form_b(mx):
        optim.clip_grad_norm_(params, mx)
        opt.step()

    def form_c(mx):
        opt.max_grad_norm = mx
        opt.step()
        opt.max_grad_norm = None

    def form_d(mx):
        opt.step()
    forms = [("a torch clip + step", form_a), ("b fused clip in place + step", form_b), ("c step(max_grad_norm)", form_c), ("d step, no clip", form_d)]
    out = {"elements": n_grad, "spans": n_spans, "norm": norm0, "step_forms": {}, "sum_kernel": {}}
    for case, mx in (("clips", 0.5 * norm0), ("does_not_clip", 2.0 * norm0)):
        times = {name: [] for name, _ in forms}
        for rep in range(args.reps + 3):
            for name, fn in forms:
                fp.grad.copy_(saved)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(mx)
                e1.record()
                times[name].append((e0, e1))
        torch.cuda.synchronize()
        out["step_forms"][case] = {}
        for name, evs in times.items():
            r = med([a.elapsed_time(b) for a, b in evs[3:]])
            out["step_forms"][case][name] = r
            print(f"{case:14s} {name:30s} {r['median_ms']:8.3f} ms  (min {r['min_ms']:.3f} max {r['max_ms']:.3f} iqr {r['iqr_ms']:.3f})")

    # ---- the sum kernel alone on the whole flat gradient buffer (one span)
    fp.grad.copy_(saved)
    table = torch.tensor([[fp.grad.data_ptr(), fp.grad.numel()]], dtype=torch.int64, device=dev)
    partials = torch.zeros(4096, dtype=torch.float64, device=dev)
    block = torch.zeros(8, dtype=torch.float32, device=dev)
    variants = [(b, a) for b in (256, 512, 1024, 2048, 4096) for a in (0, 1)]
    times = {v: [] for v in variants}
    extra = {"finish(1024 partials)": [], "scale in place (clips)": [], "scale in place (coef 1.0)": []}
    half, one = torch.tensor([0.5], device=dev), torch.tensor([1.0], device=dev)
    for rep in range(args.reps + 3):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.sumsq_spans(table, partials, v[0], v[1])
            e1.record()
            times[v].append((e0, e1))
        for name, fn in (("finish(1024 partials)", lambda: ops.clip_finish(partials, 1024, 1.0, block)),
                         ("scale in place (clips)", lambda: ops.scale_spans_(table, half)),
                         ("scale in place (coef 1.0)", lambda: ops.scale_spans_(table, one))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            extra[name].append((e0, e1))
        fp.grad.copy_(saved)
    torch.cuda.synchronize()
    nbytes = 4.0 * fp.grad.numel()
    for v, evs in times.items():
        r = med([a.elapsed_time(b) for a, b in evs[3:]])
        r["TBps"] = round(nbytes / r["median_ms"] / 1e9, 3)
        out["sum_kernel"]["blocks=%d accum=%s" % (v[0], "fp64" if v[1] == 0 else "fp32chain")] = r
        print(f"sumsq blocks {v[0]:5d} {'fp64     ' if v[1] == 0 else 'fp32chain'} {r['median_ms']:8.3f} ms  {r['TBps']:.2f} TB/s  (min {r['min_ms']:.3f} max {r['max_ms']:.3f})")
    for name, evs in extra.items():
        r = med([a.elapsed_time(b) for a, b in evs[3:]])
        out["sum_kernel"][name] = r
        print(f"{name:30s} {r['median_ms']:8.3f} ms  (min {r['min_ms']:.3f} max {r['max_ms']:.3f})")
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
