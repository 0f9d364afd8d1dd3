"""Label log-probabilities over the tied vocabulary, fused against the existing pair, at the 1.5 B model's head shape.

    python tools/head_score_bench.py [--rows 16,256,4096] [--reps 15] [--json OUT]

For every row count R (V = 159 867, K = 1536, random bf16 operands -- zero-filled ones read high on this chip), in a child process of
its own under a time limit (a hung or faulted step ends the run there; nothing further is started on the card):
  fused   ops.head_score: ug_head_score's launch pair, no logits                                  (csrc/head_score.hip)
  pair    ops.gemm_nt into a bf16 [R, vocab_pad] matrix + ops.ce_fwd(want_logp=True)                (Qwen2Engine.logits_rows + the DPO path)
Time: HIP events around each form, the two alternating in one process, median of --reps after 3 warm-ups.  Memory: peak allocated
bytes of one call of each form above what was allocated before it (operands excluded; the fused form's cached workspace is dropped
first, so its allocation counts).  Stand-alone: does not go through bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ml-unigen_amd"))

V, K = 159867, 1536
VOCAB_PAD = (V + 255) // 256 * 256
STEP_TIMEOUT_S = 240


def med(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4)}


def child(R, reps):
    import torch
    from unigen_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(R)
    x = torch.randn((R, K), device=dev, generator=g).to(torch.bfloat16)
    W = torch.zeros((VOCAB_PAD, K), dtype=torch.bfloat16, device=dev)
    for v0 in range(0, V, 16384):                              # (in pieces: no 1 GB fp32 temporary)
        n = min(16384, V - v0)
        W[v0:v0 + n] = (torch.randn((n, K), device=dev, generator=g) * 0.02).to(torch.bfloat16)
    labels = torch.randint(0, V, (R,), device=dev, generator=g)

    def fused():
        return ops.head_score(x, W, V, labels, want=("lse", "best"))[0]

    def pair():
        logits = torch.empty((R, VOCAB_PAD), dtype=torch.bfloat16, device=dev)
        ops.gemm_nt(x, W, out=logits, N=V, K=K)
        return ops.ce_fwd(logits, V, labels, want_logp=True)[3]
    forms = [("fused", fused), ("pair", pair)]
    out = {"R": R, "V": V, "K": K, "ws_bytes": ops.head_score_ws_bytes(R, V), "logits_bytes": R * VOCAB_PAD * 2}
    res = {}
    for name, fn in forms:                                     # memory first: one call each from a clean allocator
        ops._HEAD_SCORE_WS.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res[name] = fn().float().cpu()
        torch.cuda.synchronize()
        out[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
    out["max_abs_logp_difference"] = float((res["fused"] - res["pair"]).abs().max())
    times = {name: [] for name, _ in forms}
    for rep in range(reps + 3):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            times[name].append((e0, e1))
    torch.cuda.synchronize()
    for name, evs in times.items():
        out[name] = med([a.elapsed_time(b) for a, b in evs[3:]])
    flops = 2.0 * R * V * K
    out["fused_tflops"] = round(flops / out["fused"]["median_ms"] / 1e9, 1)
    out["pair_tflops"] = round(flops / out["pair"]["median_ms"] / 1e9, 1)
    out["fused_over_pair"] = round(out["fused"]["median_ms"] / out["pair"]["median_ms"], 3)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16,256,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    results = []
    for R in [int(r) for r in args.rows.split(",")]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(R), "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"R={R}: no result within {STEP_TIMEOUT_S} s; stopping here")
            return 1
        line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"R={R}: child ended with status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        r = json.loads(line[7:])
        results.append(r)
        print(f"R={R:5d}  fused {r['fused']['median_ms']:8.3f} ms ({r['fused_tflops']:6.1f} TFLOP/s)   pair {r['pair']['median_ms']:8.3f} ms "
              f"({r['pair_tflops']:6.1f} TFLOP/s)   fused/pair {r['fused_over_pair']:.3f}   peak bytes fused {r['fused_peak_bytes']:,} "
              f"(workspace {r['ws_bytes']:,})  pair {r['pair_peak_bytes']:,} (logits {r['logits_bytes']:,})   max |d logp| {r['max_abs_logp_difference']:.2e}",
              flush=True)
    print(json.dumps(results))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
