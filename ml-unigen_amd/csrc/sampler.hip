// MaskGIT parallel-decoding step (UniGen.t2i_generate, reference models/unigen.py:404-451 with
// models/sampling.py:24-46): classifier-free-guidance mix of the code-book logits, softmax, one categorical draw
// per image position, the confidence of the drawn token, and the re-masking of the least confident positions.
// Randomness is SUPPLIED as uniforms (drawn by the caller's generator), so a step is a deterministic function of
// its inputs: token = first index whose running sum of exp(logit - max) exceeds u * total (inverse CDF over the
// code book in index order); Gumbel noise = -log(-log(u2)).  torch.multinomial draws from the same distribution
// with a different use of the stream; the oracle restates this rule (oracle/qwen2_ref.py: InverseCdfSampler).
#include "common.h"
#include "unigen_hip.h"
#include "vmem_asm.h"

namespace {

constexpr int SMP_T = 256;

// one workgroup per (image, position); thread t owns code-book indices [t*C, (t+1)*C)
// EX (ug_maskgit_step_ex with every filter off and sample_temperature 1): the same draw, bit for bit -- nothing below that forms
// `sampled` or `sel` depends on EX -- plus the token's log-probabilities (logp) and the kept set's smallest value and size (stats);
// either may be null.  The conditional row's own softmax rides along the two passes: its maximum in pass 1, its chunk sums in pass 2,
// summed in thread order like `part`.
template <bool EX>
__global__ __launch_bounds__(SMP_T) void maskgit_sample_kernel(const bf16_t* __restrict__ logits, int64_t ld, int V, int N, int n,
                                                              int cfg, float scale, const float* __restrict__ u_sample,
                                                              const int64_t* __restrict__ cur_ids, int64_t mask_id,
                                                              int64_t* __restrict__ sampled, float* __restrict__ sel,
                                                              float* __restrict__ logp, float* __restrict__ stats) {
  __shared__ float red[SMP_T / 64];
  __shared__ float part[SMP_T];
  __shared__ float cpart[EX ? SMP_T : 1];
  __shared__ int hit;
  const int bi = blockIdx.x, t = threadIdx.x;
  const int64_t cur = cur_ids[bi];
  if (cur != mask_id) {                      // known token: kept, never re-masked (confidence = float max)
    if (t == 0) { sampled[bi] = cur; sel[bi] = 3.402823466e+38f; }
    return;
  }
  const int C = (V + SMP_T - 1) / SMP_T;
  const bf16_t* c = logits + (int64_t)bi * ld;
  const bf16_t* u = logits + ((int64_t)N * n + bi) * ld;
  const int lo = t * C, hi = min(V, lo + C);
  float mx = -INFINITY, cmx = -INFINITY, vmn = INFINITY;      // (cmx, vmn: EX only)
  for (int e = lo; e < hi; ++e) {
    const float cv = bf2f(c[e]);
    float v = cv;
    if (cfg) { const float uv = bf2f(u[e]); v = scale * (cv - uv) + uv; }
    mx = fmaxf(mx, v);
    if (EX) { cmx = fmaxf(cmx, cv); vmn = fminf(vmn, v); }
  }
  mx = block_max<SMP_T / 64>(mx, red);
  if (EX) {
    cmx = block_max<SMP_T / 64>(cmx, red);
    vmn = -block_max<SMP_T / 64>(-vmn, red);
  }
  float local = 0.f, clocal = 0.f;
  for (int e = lo; e < hi; ++e) {
    const float cv = bf2f(c[e]);
    float v = cv;
    if (cfg) { const float uv = bf2f(u[e]); v = scale * (cv - uv) + uv; }
    local += expf(v - mx);
    if (EX) clocal += expf(cv - cmx);
  }
  part[t] = local;
  if (EX) cpart[t] = clocal;
  if (t == 0) hit = SMP_T - 1;
  __syncthreads();
  // exclusive prefix over the 256 chunk sums: every thread sums its predecessors (256 LDS reads, negligible)
  float excl = 0.f, total = 0.f;
  for (int j = 0; j < SMP_T; ++j) { const float pj = part[j]; if (j < t) excl += pj; total += pj; }
  const float target = u_sample[bi] * total;
  if (excl <= target && target < excl + local) atomicMin(&hit, t);      // first chunk whose range holds the target
  __syncthreads();
  if (t == hit) {
    float run = excl, ex = 0.f;
    int idx = hi - 1;
    for (int e = lo; e < hi; ++e) {
      const float cv = bf2f(c[e]);
      float v = cv;
      if (cfg) { const float uv = bf2f(u[e]); v = scale * (cv - uv) + uv; }
      ex = expf(v - mx);
      run += ex;
      if (run > target) { idx = e; break; }
    }
    if (idx == hi - 1 && !(run > target)) {       // rounding pushed the target past the end of the chunk / vocabulary
      const float cv = bf2f(c[idx]);
      float v = cv;
      if (cfg) { const float uv = bf2f(u[idx]); v = scale * (cv - uv) + uv; }
      ex = expf(v - mx);
    }
    sampled[bi] = idx;
    sel[bi] = ex / total;
    if (EX) {
      const float cv = bf2f(c[idx]);
      float v = cv;
      if (cfg) { const float uv = bf2f(u[idx]); v = scale * (cv - uv) + uv; }
      if (logp) {
        float ctotal = 0.f;
        for (int j = 0; j < SMP_T; ++j) ctotal += cpart[j];
        logp[2 * (int64_t)bi] = (v - mx) - logf(total);
        logp[2 * (int64_t)bi + 1] = (cv - cmx) - logf(ctotal);
      }
      if (stats) { stats[2 * (int64_t)bi] = vmn; stats[2 * (int64_t)bi + 1] = (float)V; }
    }
  }
}

// one workgroup per image: confidence, rank of every position, threshold = (mask_len)-th smallest, re-mask below it
__global__ __launch_bounds__(1024) void maskgit_remask_kernel(const float* __restrict__ sel, const float* __restrict__ u_conf,
                                                              const int64_t* __restrict__ cur_ids, const int64_t* __restrict__ sampled,
                                                              int64_t mask_id, int64_t id_offset, int mask_len_sched,
                                                              float temperature, int n, int64_t* __restrict__ next_cur,
                                                              int64_t* __restrict__ next_ids, uint8_t* __restrict__ masking_out) {
  extern __shared__ float conf_s[];
  __shared__ int unknown_cnt;
  __shared__ float thr_s;
  const int b = blockIdx.x, i = threadIdx.x;
  if (i == 0) unknown_cnt = 0;
  __syncthreads();
  float conf = INFINITY;
  if (i < n) {
    const int64_t g = (int64_t)b * n + i;
    const float uu = fmaxf(u_conf[g], 1e-20f);
    const float gum = -logf(fmaxf(-logf(uu), 1e-20f));
    conf = logf(fmaxf(sel[g], 1e-20f)) + temperature * gum;
    conf_s[i] = conf;
    if (cur_ids[g] == mask_id) atomicAdd(&unknown_cnt, 1);
  }
  __syncthreads();
  const int k = max(1, min(unknown_cnt - 1, mask_len_sched));
  if (i < n) {
    int less = 0, eq = 0;
    for (int j = 0; j < n; ++j) { const float cj = conf_s[j]; less += cj < conf; eq += cj == conf; }
    if (less <= k && k < less + eq) thr_s = conf;        // sorted[k] (all writers hold the same value)
  }
  __syncthreads();
  if (i < n) {
    const int64_t g = (int64_t)b * n + i;
    const bool m = (k < n) && conf < thr_s;
    const int64_t s = sampled[g];
    next_cur[g] = m ? mask_id : s;
    next_ids[g] = m ? mask_id : s + id_offset;
    if (masking_out) masking_out[g] = m;
  }
}

// ------------------------------------------------------------------ autoregressive image-token sampling
// One decode step of UniGen.t2i_generate_ar after the backbone (reference models/unigen.py:503-519): code-book logits
// of the conditional / unconditional rows (raw fp32 accumulator of the lm-head GEMV, rounded to bf16 like the head's
// output), CFG mix, temperature, softmax, one categorical draw (inverse CDF on a supplied uniform) or argmax, then the
// next step's input: the embedding row of (token + id_offset) for both halves.  One workgroup per image; the
// accumulator rows are cleared for the next step.
constexpr int AR_MAXV = 8192;          // code-book slice staged in LDS (33 KiB incl. padding)
__device__ __forceinline__ int ar_pad(int e) { return e + (e >> 5); }      // chunk starts land on different banks

// 1 024 threads (round 5; was 256 with an O(threads) serial scan of the partial sums: 16.7 us per step): eight loads per row per
// thread, the inverse CDF through a wave scan (shuffles) + sixteen wave totals, the rest unchanged.
constexpr int ARS_T = 1024;
constexpr int AR_PER = AR_MAXV / ARS_T;

// LOGP instantiations (ug_ar_sample_logp / ug_ar_sample_filtered_logp): the conditional model's own log-softmax at the chosen token.
// Thread t keeps the bf16-rounded conditional values it loaded in pass 1 (entries t + j * ARS_T) in registers: the accumulator rows are
// cleared by then and `mix` holds the mixed values only.  Per thread (max, sum of exp(value - max)) over those registers; the block
// maximum through `cmx_w`, the sum rescaled to it through an xor tree over the wave and the sixteen wave partials in wave order: fixed
// order, no atomics.
struct ArCond { float mx, sum; };
__device__ __forceinline__ ArCond ar_cond_local(const float (&cv)[AR_PER], int t, int V) {
  ArCond c{-INFINITY, 0.f};
#pragma unroll
  for (int j = 0; j < AR_PER; ++j)
    if (t + j * ARS_T < V) c.mx = fmaxf(c.mx, cv[j]);
#pragma unroll
  for (int j = 0; j < AR_PER; ++j)
    if (t + j * ARS_T < V) c.sum += expf(cv[j] - c.mx);
  return c;
}
// behind the barrier that published cmx_w: the block maximum; the wave's partial of the rescaled sum goes to csum_w (read it behind the
// next barrier with ar_cond_total)
__device__ __forceinline__ float ar_cond_merge(const ArCond& c, const float* cmx_w, float* csum_w, int lane, int wave) {
  float cmax = cmx_w[0];
#pragma unroll
  for (int w = 1; w < ARS_T / 64; ++w) cmax = fmaxf(cmax, cmx_w[w]);
  float part = c.sum > 0.f ? __fmul_rn(c.sum, expf(c.mx - cmax)) : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) csum_w[wave] = part;
  return cmax;
}
__device__ __forceinline__ float ar_cond_total(const float* csum_w) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < ARS_T / 64; ++w) s += csum_w[w];
  return s;
}
// logp[(b * nsteps + step) * 2 + {0, 1}]: thread 0 writes the log-probability under the drawn-from distribution, the thread that loaded
// the token's conditional value writes the conditional log-softmax
__device__ __forceinline__ void ar_write_logp(float* __restrict__ logp, int b, int nsteps, int step, int token, float v_tok, float bmx,
                                              float total, const float (&cv)[AR_PER], float cmax, float ctotal, int t) {
  float* out = logp + ((int64_t)b * nsteps + step) * 2;
  if (t == 0) out[0] = (v_tok - bmx) - logf(total);
  if (t == (token & (ARS_T - 1))) {
    uint32_t bits = 0u;                                        // (an OR of selected patterns: the values stay in registers, where an
#pragma unroll                                                 //  indexed read of cv[token >> 10] would move the array to memory)
    for (int j = 0; j < AR_PER; ++j) bits |= (token >> 10) == j ? __float_as_uint(cv[j]) : 0u;
    out[1] = (__uint_as_float(bits) - cmax) - logf(ctotal);
  }
}
static_assert(ARS_T == 1024, "ar_write_logp: token >> 10 is the slot of the thread that loaded it");

template <bool LOGP>
__global__ __launch_bounds__(ARS_T) void ar_sample_kernel(float* __restrict__ acc, int64_t lda, int bsz, int V, float scale,
                                                         float inv_temp, int greedy, const float* __restrict__ uniforms,
                                                         const int* __restrict__ pos_dev, int pos0, int nsteps,
                                                         const float* __restrict__ embed, int64_t lde, int H, int64_t id_offset,
                                                         int64_t* __restrict__ tok, int* __restrict__ out_tokens,
                                                         float* __restrict__ x, float* __restrict__ logp) {
  __shared__ float mix[AR_MAXV + AR_MAXV / 32];
  __shared__ float red[ARS_T / 64];
  __shared__ float wtot[ARS_T / 64];
  __shared__ int hit;
  __shared__ int best_i[ARS_T / 64];
  __shared__ int chosen;
  __shared__ float cmx_w[LOGP ? ARS_T / 64 : 1], csum_w[LOGP ? ARS_T / 64 : 1];
  float cvr[AR_PER] = {};                                        // (LOGP: the conditional values this thread loaded)
  ArCond cl{-INFINITY, 0.f};
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // the position word (written by the head launch in front of us): a hand-issued SCALAR load (vmem_asm.h: hipcc reads such a word with a
  // vector load and waits vmcnt(0) for it on the spot, a serialised round trip ahead of the logits' loads); used behind pass 1
  int pos_now;
  sld4(pos_now, pos_dev);
  float* c = acc + (int64_t)b * lda;
  float* u = acc + (int64_t)(bsz + b) * lda;
  // pass 1 (coalesced): mixed logits into LDS, accumulator rows cleared, running max / first argmax per thread
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  {
    constexpr int PER = AR_MAXV / ARS_T;                     // every load of the two rows in flight at once
    float cr[PER], ur[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = min(t + j * ARS_T, V - 1);
      cr[j] = c[e]; ur[j] = u[e];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = t + j * ARS_T;
      if (e < V) {
        c[e] = 0.f; u[e] = 0.f;
        const float cv = bf2f(f2bf(cr[j])), uv = bf2f(f2bf(ur[j]));
        const float v = (uv + scale * (cv - uv)) * inv_temp;
        mix[ar_pad(e)] = v;
        if (v > mx) { mx = v; arg = e; }
        if (LOGP) cvr[j] = cv;
      }
    }
    if (LOGP) cl = ar_cond_local(cvr, t, V);
  }
  wait_lgkm0();
  tie_s(pos_now);
  const int step = min(max(pos_now - pos0, 0), nsteps - 1);
  const float u01 = greedy ? 0.f : uniforms[(int64_t)step * bsz + b];      // (requested here: its round trip hides under the reductions)
  // block max + smallest index attaining it
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(arg, o, 64);
    if (om > mx || (om == mx && oi < arg)) { mx = om; arg = oi; }
  }
  if (LOGP) {
    float cm = cl.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
    if (lane == 0) cmx_w[wave] = cm;
  }
  if (lane == 0) { red[wave] = mx; best_i[wave] = arg; }
  if (t == 0) hit = ARS_T - 1;
  __syncthreads();
  float bmx = red[0]; int bi = best_i[0];
#pragma unroll
  for (int w = 1; w < ARS_T / 64; ++w) if (red[w] > bmx || (red[w] == bmx && best_i[w] < bi)) { bmx = red[w]; bi = best_i[w]; }
  float cmax = 0.f, total_all = 0.f;
  if (LOGP) cmax = ar_cond_merge(cl, cmx_w, csum_w, lane, wave);
  if (greedy) {
    if (t == 0) chosen = bi;
    if (LOGP) {
      // the one block sum the greedy pick skips: the chunk sums of the draw below, an xor tree over the wave, the wave partials in order
      const int C = (V + ARS_T - 1) / ARS_T;
      const int lo = t * C, hi = min(V, lo + C);
      float local = 0.f;
      for (int e = lo; e < hi; ++e) local += expf(mix[ar_pad(e)] - bmx);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
      if (lane == 0) wtot[wave] = local;
    }
  } else {
    // inverse CDF in index order: thread t owns the contiguous chunk [t*C, (t+1)*C); exclusive prefix of the chunk sums by a
    // wave scan + the totals of the waves in front
    const int C = (V + ARS_T - 1) / ARS_T;
    const int lo = t * C, hi = min(V, lo + C);
    float local = 0.f;
    for (int e = lo; e < hi; ++e) local += expf(mix[ar_pad(e)] - bmx);
    float incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    float base = 0.f, total = 0.f;
#pragma unroll
    for (int w = 0; w < ARS_T / 64; ++w) { const float wv = wtot[w]; if (w < wave) base += wv; total += wv; }
    const float excl = base + (incl - local);
    // The chunks' ranges must TILE [0, total): a thread's upper bound is its neighbour's lower bound, not its own excl + local (the two
    // differ by an ulp, so a target could fall into a gap, match nobody and force the token to the last chunk: ~3e-5 per token,
    // ADVICE r5).  Next lane's excl within the wave; the next wave's base (= base + this wave's total, the very sum that wave forms)
    // across waves; the grand total for the last thread.
    float upper = __shfl_down(excl, 1, 64);
    if (lane == 63) upper = (wave == ARS_T / 64 - 1) ? total : base + wtot[wave];
    const float target = u01 * total;
    if (excl <= target && target < upper) atomicMin(&hit, t);
    __syncthreads();
    if (t == hit) {
      float run = excl;
      int idx = max(hi - 1, lo);
      for (int e = lo; e < hi; ++e) { run += expf(mix[ar_pad(e)] - bmx); if (run > target) { idx = e; break; } }
      chosen = min(idx, V - 1);
    }
    if (LOGP) total_all = total;
  }
  __syncthreads();
  const int token = chosen;
  if (t == 0) { tok[b] = token; out_tokens[(int64_t)b * nsteps + step] = token; }
  if (LOGP) {
    if (greedy) {
#pragma unroll
      for (int w = 0; w < ARS_T / 64; ++w) total_all += wtot[w];
    }
    ar_write_logp(logp, b, nsteps, step, token, mix[ar_pad(token)], bmx, total_all, cvr, cmax, ar_cond_total(csum_w), t);
  }
  const float4* er = reinterpret_cast<const float4*>(embed + (token + id_offset) * lde);
  float4* x0 = reinterpret_cast<float4*>(x + (int64_t)b * H);
  float4* x1 = reinterpret_cast<float4*>(x + (int64_t)(bsz + b) * H);
  for (int i = t; i < (H >> 2); i += ARS_T) { const float4 v = er[i]; x0[i] = v; x1[i] = v; }
}

// ------------------------------------------------------------------ the same step with top-k / top-p / min-p truncation
// Every filter is a VALUE threshold (include/unigen_hip.h: ug_ar_sample_filtered), so nothing is sorted: the kept set is
// {v >= tau}, tau = max(tau_k, tau_p, tau_m).  Values are compared through an order-preserving 32-bit key.  Thread t holds the keys
// and exp(v - max) of its contiguous chunk in registers (exp is evaluated once per element); every float sum has a fixed order
// (chunk in index order, xor tree over the wave, the sixteen wave partials in wave order), so the step is a function of its inputs.
__device__ __forceinline__ uint32_t ar_key(float v) {
  uint32_t b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;                                   // -0 and +0 compare equal: one key
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ar_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

struct ArProbe { float mass; uint32_t le, gt; };
// Over the elements with key >= lo: mass = sum of ex over key >= bound; le = the largest key in [lo, bound) (lo if none); gt = the
// smallest key in [bound, hi] (hi if none).  One barrier; consecutive calls alternate `par` (a wave can be one call ahead, not two).
__device__ __forceinline__ ArProbe ar_probe(const uint32_t (&key)[AR_PER], const float (&ex)[AR_PER], uint32_t lo, uint32_t bound,
                                            uint32_t hi, float (*s_mass)[ARS_T / 64], uint32_t (*s_le)[ARS_T / 64],
                                            uint32_t (*s_gt)[ARS_T / 64], int par, int lane, int wave) {
  float m = 0.f;
  uint32_t le = lo, gt = hi;
#pragma unroll
  for (int j = 0; j < AR_PER; ++j) {
    const uint32_t k = key[j];
    m += (k >= bound && k >= lo) ? ex[j] : 0.f;
    if (k < bound) le = max(le, k);
    else if (k <= hi) gt = min(gt, k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m += __shfl_xor(m, o, 64);
    le = max(le, (uint32_t)__shfl_xor((int)le, o, 64));
    gt = min(gt, (uint32_t)__shfl_xor((int)gt, o, 64));
  }
  if (lane == 0) { s_mass[par][wave] = m; s_le[par][wave] = le; s_gt[par][wave] = gt; }
  __syncthreads();
  ArProbe r{0.f, lo, hi};
#pragma unroll
  for (int w = 0; w < ARS_T / 64; ++w) { r.mass += s_mass[par][w]; r.le = max(r.le, s_le[par][w]); r.gt = min(r.gt, s_gt[par][w]); }
  return r;
}

// The threshold search and the draw, shared by ar_sample_filtered_kernel (one row per image, fp32 accumulator) and
// maskgit_sample_filtered_kernel (one row per masked position, bf16 logits).  The caller has the row's mixed values in `mix` (ar_pad
// layout), its maximum bmx, and has called ar_search_init ahead of the barrier that published them.  stats (nullable): the row's two
// floats.  Returns behind a barrier: every thread holds the token and the kept mass.
struct ArSearchLds {
  float wtot[ARS_T / 64];
  __attribute__((aligned(16))) int hist[4][256];
  float s_mass[2][ARS_T / 64];
  uint32_t s_le[2][ARS_T / 64], s_gt[2][ARS_T / 64];
  int s_cnt[ARS_T / 64];
  uint32_t s_min[ARS_T / 64];
  int hit, last_el, chosen;
};
struct ArDraw { int token; float total; };
__device__ __forceinline__ void ar_search_init(ArSearchLds& lds, int t) {
  (&lds.hist[0][0])[t] = 0;                                       // 4 x 256 digit counters, one per thread
  if (t == 0) { lds.hit = ARS_T; lds.last_el = -1; lds.chosen = 0; }
}
__device__ __forceinline__ ArDraw ar_truncated_draw(const float* mix, int V, float bmx, float u01, int top_k, float top_p,
                                                    float log_min_p, float* __restrict__ stats, ArSearchLds& lds, int t, int lane,
                                                    int wave) {
  // thread t owns the contiguous chunk [t*C, t*C + nv): keys and exp in registers from here on (slots past nv: key 0, mass 0)
  const int C = (V + ARS_T - 1) / ARS_T;
  const int e0 = t * C, nv = min(max(V - e0, 0), C);
  uint32_t key[AR_PER];
  float ex[AR_PER];
#pragma unroll
  for (int j = 0; j < AR_PER; ++j) {
    key[j] = 0u; ex[j] = 0.f;
    if (j < nv) { const float v = mix[ar_pad(e0 + j)]; key[j] = ar_key(v); ex[j] = expf(v - bmx); }
  }
  // top-k: radix select of the k-th largest key, 8 bits per pass; every wave scans the 256 counters itself (one barrier per pass)
  uint32_t tau_k = 0u;
  if (top_k > 0) {
    int kk = top_k;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int sh = 24 - 8 * p;
#pragma unroll
      for (int j = 0; j < AR_PER; ++j)
        if (j < nv && (p == 0 || (key[j] >> ((sh + 8) & 31)) == (tau_k >> ((sh + 8) & 31)))) atomicAdd(&lds.hist[p][(key[j] >> sh) & 255], 1);
      __syncthreads();
      const int4 h = reinterpret_cast<const int4*>(lds.hist[p])[lane];              // digits 4*lane .. 4*lane+3
      const int s = h.x + h.y + h.z + h.w;
      int incl = s;                                                             // elements with a digit >= 4*lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += v;
      }
      int above = __shfl_down(incl, 1, 64);                                     // ... with a digit >= 4*lane+4
      if (lane == 63) above = 0;
      const int src = __ffsll((unsigned long long)__ballot(incl >= kk && above < kk)) - 1;       // the lane that holds the k-th
      int d = 4 * lane + 3, cnt = h.w;
      if (above + cnt < kk) { above += cnt; --d; cnt = h.z;
        if (above + cnt < kk) { above += cnt; --d; cnt = h.y;
          if (above + cnt < kk) { above += cnt; --d; } } }
      const int digit = __shfl(d, src, 64);
      kk = __shfl(kk - above, src, 64);
      tau_k |= (uint32_t)digit << sh;
    }
  }
  // top-p over S_k = {key >= tau_k}: the smallest value whose mass of strictly greater values is <= top_p * Z.  Bisection on the key;
  // each probe also returns the present values next to the cut, so both ends move onto present values and the search stops when the
  // interval holds one distinct value.  The mass is monotone in the cut under the fixed summation order, so the search is consistent.
  uint32_t tau_p = tau_k;
  if (top_p < 1.f) {
    uint32_t lo = tau_k, hi = ar_key(bmx);
    const float lim = top_p * ar_probe(key, ex, lo, lo, hi, lds.s_mass, lds.s_le, lds.s_gt, 0, lane, wave).mass;
    int par = 1;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      const ArProbe r = ar_probe(key, ex, lo, mid + 1u, hi, lds.s_mass, lds.s_le, lds.s_gt, par, lane, wave);
      par ^= 1;
      if (r.mass <= lim) hi = r.le; else lo = r.gt;
    }
    tau_p = hi;
  }
  // min-p: one compare (log_min_p = -inf when off: key below every finite value)
  const uint32_t thr = max(tau_p, ar_key(bmx + log_min_p));
  // inverse CDF in index order over the kept entries (dropped ones count 0)
  unsigned kept = 0;
  float local = 0.f;
#pragma unroll
  for (int j = 0; j < AR_PER; ++j)
    if (j < nv && key[j] >= thr) { kept |= 1u << j; local += ex[j]; }
  float incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) lds.wtot[wave] = incl;
  if (stats) {                                                  // diagnostics: smallest kept key and kept count
    int cnt = __popc(kept);
    uint32_t mn = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) if (kept >> j & 1) mn = min(mn, key[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64)); }
    if (lane == 0) { lds.s_cnt[wave] = cnt; lds.s_min[wave] = mn; }
  }
  __syncthreads();
  float base = 0.f, total = 0.f;
#pragma unroll
  for (int w = 0; w < ARS_T / 64; ++w) { const float wv = lds.wtot[w]; if (w < wave) base += wv; total += wv; }
  // The drawn token must be a kept one whatever the rounding of the running sums: only a thread with kept mass can be hit (the first
  // whose inclusive bound exceeds the target; the last such thread if rounding leaves none), and it walks its kept entries only.
  const float target = u01 * total;
  if (local > 0.f) {
    atomicMax(&lds.last_el, t);
    if (target < base + incl) atomicMin(&lds.hit, t);
  }
  __syncthreads();
  if (t == (lds.hit < ARS_T ? lds.hit : lds.last_el)) {
    float run = base + (incl - local);
    int idx = e0;
    bool done = false;
#pragma unroll
    for (int j = 0; j < AR_PER; ++j)
      if (!done && (kept >> j & 1) && ex[j] > 0.f) { run += ex[j]; idx = e0 + j; done = run > target; }
    lds.chosen = idx;
  }
  if (stats && t == 0) {
    int cnt = 0;
    uint32_t mn = 0xffffffffu;
    for (int w = 0; w < ARS_T / 64; ++w) { cnt += lds.s_cnt[w]; mn = min(mn, lds.s_min[w]); }
    stats[0] = ar_unkey(mn);
    stats[1] = (float)cnt;
  }
  __syncthreads();
  return ArDraw{lds.chosen, total};
}

template <bool LOGP>
__global__ __launch_bounds__(ARS_T) void ar_sample_filtered_kernel(float* __restrict__ acc, int64_t lda, int bsz, int V, float scale,
                                                                  float inv_temp, const float* __restrict__ uniforms,
                                                                  const int* __restrict__ pos_dev, int pos0, int nsteps,
                                                                  const float* __restrict__ embed, int64_t lde, int H,
                                                                  int64_t id_offset, int top_k, float top_p, float log_min_p,
                                                                  int64_t* __restrict__ tok, int* __restrict__ out_tokens,
                                                                  float* __restrict__ x, float* __restrict__ stats,
                                                                  float* __restrict__ logp) {
  __shared__ float cmx_w[LOGP ? ARS_T / 64 : 1], csum_w[LOGP ? ARS_T / 64 : 1];
  float cvr[AR_PER] = {};                                        // (LOGP: the conditional values this thread loaded)
  ArCond cl{-INFINITY, 0.f};
  __shared__ float mix[AR_MAXV + AR_MAXV / 32];
  __shared__ float red[ARS_T / 64];
  __shared__ ArSearchLds srch;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int pos_now;                                                  // (scalar load of the position word: see ar_sample_kernel)
  sld4(pos_now, pos_dev);
  float* c = acc + (int64_t)b * lda;
  float* u = acc + (int64_t)(bsz + b) * lda;
  // pass 1 (coalesced), as in ar_sample_kernel: mixed logits into LDS, accumulator rows cleared, running max per thread
  float mx = -INFINITY;
  {
    float cr[AR_PER], ur[AR_PER];
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) {
      const int e = min(t + j * ARS_T, V - 1);
      cr[j] = c[e]; ur[j] = u[e];
    }
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) {
      const int e = t + j * ARS_T;
      if (e < V) {
        c[e] = 0.f; u[e] = 0.f;
        const float cv = bf2f(f2bf(cr[j])), uv = bf2f(f2bf(ur[j]));
        const float v = (uv + scale * (cv - uv)) * inv_temp;
        mix[ar_pad(e)] = v;
        mx = fmaxf(mx, v);
        if (LOGP) cvr[j] = cv;
      }
    }
    if (LOGP) cl = ar_cond_local(cvr, t, V);
  }
  wait_lgkm0();
  tie_s(pos_now);
  const int step = min(max(pos_now - pos0, 0), nsteps - 1);
  const float u01 = uniforms[(int64_t)step * bsz + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  if (LOGP) {
    float cm = cl.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
    if (lane == 0) cmx_w[wave] = cm;
  }
  ar_search_init(srch, t);
  __syncthreads();
  float bmx = red[0];
#pragma unroll
  for (int w = 1; w < ARS_T / 64; ++w) bmx = fmaxf(bmx, red[w]);
  float cmax = 0.f;
  if (LOGP) cmax = ar_cond_merge(cl, cmx_w, csum_w, lane, wave);          // (csum_w: published by the barriers below)
  const ArDraw d = ar_truncated_draw(mix, V, bmx, u01, top_k, top_p, log_min_p, stats ? stats + 2 * b : nullptr, srch, t, lane, wave);
  const int token = d.token;
  const float total = d.total;
  if (t == 0) { tok[b] = token; out_tokens[(int64_t)b * nsteps + step] = token; }
  // (total = the kept mass: the drawn token is a kept one, so this is its log-probability under the truncated distribution)
  if (LOGP) ar_write_logp(logp, b, nsteps, step, token, mix[ar_pad(token)], bmx, total, cvr, cmax, ar_cond_total(csum_w), t);
  const float4* er = reinterpret_cast<const float4*>(embed + (token + id_offset) * lde);
  float4* x0 = reinterpret_cast<float4*>(x + (int64_t)b * H);
  float4* x1 = reinterpret_cast<float4*>(x + (int64_t)(bsz + b) * H);
  for (int i = t; i < (H >> 2); i += ARS_T) { const float4 v = er[i]; x0[i] = v; x1[i] = v; }
}

// ------------------------------------------------------------------ MaskGIT draw with temperature and truncation
// ug_maskgit_step_ex with a filter on or a sampling temperature: maskgit_sample_kernel's job under the rule of
// ar_sample_filtered_kernel.  One workgroup per (image, position), known positions leave at once; the two bf16 rows are read from
// memory ONCE (maskgit_sample_kernel walks them three times), mixed into LDS, and ar_truncated_draw does the rest.  vec (ld % 8 == 0
// and a 16-byte aligned base, so every row starts on 16 bytes): thread t loads entries 8t .. 8t+7 in one 16-byte load per row; a
// trailing group that would reach past V, and every group without vec, goes through 2-byte loads (entries t + j * ARS_T).
// logp / stats (nullable): two floats per position each, masked positions only.
__global__ __launch_bounds__(ARS_T) void maskgit_sample_filtered_kernel(const bf16_t* __restrict__ logits, int64_t ld, int V, int N, int n,
                                                                       int cfg, float scale, float inv_temp, int vec,
                                                                       const float* __restrict__ u_sample,
                                                                       const int64_t* __restrict__ cur_ids, int64_t mask_id, int top_k,
                                                                       float top_p, float log_min_p, int64_t* __restrict__ sampled,
                                                                       float* __restrict__ sel, float* __restrict__ logp,
                                                                       float* __restrict__ stats) {
  __shared__ float mix[AR_MAXV + AR_MAXV / 32];
  __shared__ float red[ARS_T / 64];
  __shared__ float cmx_w[ARS_T / 64], csum_w[ARS_T / 64];
  __shared__ ArSearchLds srch;
  const int bi = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t cur = cur_ids[bi];
  if (cur != mask_id) {                      // known token: kept, never re-masked (confidence = float max); logp / stats untouched
    if (t == 0) { sampled[bi] = cur; sel[bi] = 3.402823466e+38f; }
    return;
  }
  const bf16_t* c = logits + (int64_t)bi * ld;
  const bf16_t* u = cfg ? logits + ((int64_t)N * n + bi) * ld : c;
  const float u01 = u_sample[bi];
  // the one pass over memory: every load of the two rows in flight at once
  const bool group = vec && 8 * t + 8 <= V;                    // a whole 16-byte group inside the row
  const int first = vec ? 8 * t : t, stride = vec ? 1 : ARS_T;
  bf16_t cr[AR_PER], ur[AR_PER];
  if (group) {
    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(c + 8 * t);
    bf16x8_t b = a;
    if (cfg) b = *reinterpret_cast<const bf16x8_t*>(u + 8 * t);
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) { cr[j] = (bf16_t)a[j]; ur[j] = (bf16_t)b[j]; }
  } else {
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) {
      const int e = min(first + j * stride, V - 1);
      cr[j] = c[e];
      ur[j] = cfg ? u[e] : cr[j];
    }
  }
  static_assert(AR_PER == 8, "maskgit_sample_filtered_kernel: one 16-byte load is the thread's eight entries");
  float mx = -INFINITY;
  ArCond cl{-INFINITY, 0.f};
  float cvr[AR_PER];
#pragma unroll
  for (int j = 0; j < AR_PER; ++j) {
    const int e = first + j * stride;
    cvr[j] = -INFINITY;
    if (e < V) {
      const float cv = bf2f(cr[j]);
      float v = cv;
      if (cfg) { const float uv = bf2f(ur[j]); v = scale * (cv - uv) + uv; }
      v *= inv_temp;
      mix[ar_pad(e)] = v;
      mx = fmaxf(mx, v);
      cvr[j] = cv;
      cl.mx = fmaxf(cl.mx, cv);
    }
  }
  if (logp) {                                                   // the conditional row's own softmax: per-thread (max, sum) in slot order
#pragma unroll
    for (int j = 0; j < AR_PER; ++j)
      if (first + j * stride < V) cl.sum += expf(cvr[j] - cl.mx);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float cm = cl.mx;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
  if (lane == 0) { red[wave] = mx; cmx_w[wave] = cm; }
  ar_search_init(srch, t);
  __syncthreads();
  float bmx = red[0];
#pragma unroll
  for (int w = 1; w < ARS_T / 64; ++w) bmx = fmaxf(bmx, red[w]);
  float cmax = 0.f;
  if (logp) cmax = ar_cond_merge(cl, cmx_w, csum_w, lane, wave);          // (csum_w: published by the barriers of the draw)
  const ArDraw d = ar_truncated_draw(mix, V, bmx, u01, top_k, top_p, log_min_p, stats ? stats + 2 * (int64_t)bi : nullptr, srch, t, lane,
                                     wave);
  if (t == 0) {
    // the confidence of the re-masking launch is the probability under the distribution drawn from (d.total = the kept mass)
    const float vt = mix[ar_pad(d.token)];
    sampled[bi] = d.token;
    sel[bi] = expf(vt - bmx) / d.total;
    if (logp) {
      logp[2 * (int64_t)bi] = (vt - bmx) - logf(d.total);
      logp[2 * (int64_t)bi + 1] = (bf2f(c[d.token]) - cmax) - logf(ar_cond_total(csum_w));      // (one 2-byte re-read, an L2 hit)
    }
  }
}

// argument checks + launch of ug_ar_sample / ug_ar_sample_logp (logp null: the kernel without the output)
int ar_sample_launch(const char* who, float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                     const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed, int64_t ld_embed,
                     int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, float* logp, hipStream_t st) {
  UG_REQUIRE(acc && pos_dev && embed && tok && out_tokens && x && (greedy || uniforms), "%s: null argument", who);
  UG_REQUIRE(V <= AR_MAXV, "%s: code-book slice of %ld columns exceeds the %d this build stages in LDS", who, (long)V, AR_MAXV);
  UG_REQUIRE(bsz > 0 && V > 0 && ldacc >= V && nsteps > 0 && H > 0 && H % 4 == 0 && ld_embed % 4 == 0 && temperature > 0.f &&
                 ug_aligned16(embed) && ug_aligned16(x),
             "%s: bad sizes (bsz=%ld V=%ld H=%ld temperature=%g)", who, (long)bsz, (long)V, (long)H, (double)temperature);
  if (logp)
    hipLaunchKernelGGL(ar_sample_kernel<true>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V, guidance_scale,
                       1.f / temperature, greedy, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, tok,
                       out_tokens, x, logp);
  else
    hipLaunchKernelGGL(ar_sample_kernel<false>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V, guidance_scale,
                       1.f / temperature, greedy, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, tok,
                       out_tokens, x, (float*)nullptr);
  UG_CHECK_LAUNCH(who);
  return UG_OK;
}

int ar_sample_filtered_launch(const char* who, float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature,
                              int greedy, const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed,
                              int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, int64_t top_k,
                              float top_p, float min_p, float* stats, float* logp, hipStream_t st) {
  UG_REQUIRE(acc && pos_dev && embed && tok && out_tokens && x && (greedy || uniforms), "%s: null argument", who);
  UG_REQUIRE(V <= AR_MAXV, "%s: code-book slice of %ld columns exceeds the %d this build stages in LDS", who, (long)V, AR_MAXV);
  UG_REQUIRE(bsz > 0 && V > 0 && ldacc >= V && nsteps > 0 && H > 0 && H % 4 == 0 && ld_embed % 4 == 0 && temperature > 0.f &&
                 ug_aligned16(embed) && ug_aligned16(x),
             "%s: bad sizes (bsz=%ld V=%ld H=%ld temperature=%g)", who, (long)bsz, (long)V, (long)H, (double)temperature);
  UG_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p <= 1.f,
             "%s: bad filter (top_k=%ld >= 0, 0 < top_p=%g <= 1, 0 <= min_p=%g <= 1)", who, (long)top_k, (double)top_p, (double)min_p);
  const int k = top_k >= V ? 0 : (int)top_k;
  const float lmp = min_p > 0.f ? logf(min_p) : -INFINITY;
  if (greedy) {                                       // the argmax is always kept: the filters change nothing (stats stay unwritten)
    if (logp)
      hipLaunchKernelGGL(ar_sample_kernel<true>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V, guidance_scale,
                         1.f / temperature, 1, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, tok,
                         out_tokens, x, logp);
    else
      hipLaunchKernelGGL(ar_sample_kernel<false>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V, guidance_scale,
                         1.f / temperature, 1, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, tok,
                         out_tokens, x, (float*)nullptr);
  } else if (logp) {
    hipLaunchKernelGGL(ar_sample_filtered_kernel<true>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V,
                       guidance_scale, 1.f / temperature, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, k,
                       top_p, lmp, tok, out_tokens, x, stats, logp);
  } else {
    hipLaunchKernelGGL(ar_sample_filtered_kernel<false>, dim3((unsigned)bsz), dim3(ARS_T), 0, st, acc, ldacc, (int)bsz, (int)V,
                       guidance_scale, 1.f / temperature, uniforms, pos_dev, (int)pos0, (int)nsteps, embed, ld_embed, (int)H, id_offset, k,
                       top_p, lmp, tok, out_tokens, x, stats, (float*)nullptr);
  }
  UG_CHECK_LAUNCH(who);
  return UG_OK;
}

}  // namespace

// the re-masking launch of ug_maskgit_step / ug_maskgit_step_ex
static int maskgit_remask_launch(const char* who, const float* sel_ws, const float* u_conf, const int64_t* cur_ids, const int64_t* sampled,
                                 int64_t mask_id, int64_t id_offset, int64_t mask_len_sched, float temperature, int64_t N, int64_t n,
                                 int64_t* next_cur, int64_t* next_ids, uint8_t* masking_out, hipStream_t st) {
  const int threads = (int)((n + 63) / 64 * 64);
  hipLaunchKernelGGL(maskgit_remask_kernel, dim3((unsigned)N), dim3(threads), n * sizeof(float), st, sel_ws, u_conf, cur_ids, sampled,
                     mask_id, id_offset, (int)mask_len_sched, temperature, (int)n, next_cur, next_ids, masking_out);
  UG_CHECK_LAUNCH(who);
  return UG_OK;
}

extern "C" int ug_maskgit_step(const void* logits, int64_t ld, int64_t V, int64_t N, int64_t n, int cfg, float guidance_scale,
                               const float* u_sample, const float* u_conf, const int64_t* cur_ids, int64_t mask_id,
                               int64_t id_offset, int64_t mask_len_sched, float temperature, int64_t* sampled, float* sel_ws,
                               int64_t* next_cur, int64_t* next_ids, uint8_t* masking_out, hipStream_t st) {
  UG_REQUIRE(logits && u_sample && u_conf && cur_ids && sampled && sel_ws && next_cur && next_ids, "ug_maskgit_step: null argument");
  UG_REQUIRE(N > 0 && n > 0 && n <= 1024 && V > 0 && ld >= V, "ug_maskgit_step: bad sizes (N=%ld n=%ld V=%ld ld=%ld; n <= 1024)",
             (long)N, (long)n, (long)V, (long)ld);
  hipLaunchKernelGGL(maskgit_sample_kernel<false>, dim3((unsigned)(N * n)), dim3(SMP_T), 0, st, (const bf16_t*)logits, ld, (int)V, (int)N,
                     (int)n, cfg, guidance_scale, u_sample, cur_ids, mask_id, sampled, sel_ws, (float*)nullptr, (float*)nullptr);
  UG_CHECK_LAUNCH("ug_maskgit_step(sample)");
  return maskgit_remask_launch("ug_maskgit_step(remask)", sel_ws, u_conf, cur_ids, sampled, mask_id, id_offset, mask_len_sched, temperature,
                               N, n, next_cur, next_ids, masking_out, st);
}

extern "C" int ug_maskgit_step_ex(const void* logits, int64_t ld, int64_t V, int64_t N, int64_t n, int cfg, float guidance_scale,
                                  const float* u_sample, const float* u_conf, const int64_t* cur_ids, int64_t mask_id,
                                  int64_t id_offset, int64_t mask_len_sched, float temperature, float sample_temperature, int64_t top_k,
                                  float top_p, float min_p, int64_t* sampled, float* sel_ws, int64_t* next_cur, int64_t* next_ids,
                                  uint8_t* masking_out, float* logp, float* stats, hipStream_t st) {
  UG_REQUIRE(logits && u_sample && u_conf && cur_ids && sampled && sel_ws && next_cur && next_ids, "ug_maskgit_step_ex: null argument");
  UG_REQUIRE(N > 0 && n > 0 && n <= 1024 && V > 0 && ld >= V, "ug_maskgit_step_ex: bad sizes (N=%ld n=%ld V=%ld ld=%ld; n <= 1024)",
             (long)N, (long)n, (long)V, (long)ld);
  UG_REQUIRE(sample_temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p <= 1.f,
             "ug_maskgit_step_ex: bad filter (sample_temperature=%g > 0, top_k=%ld >= 0, 0 < top_p=%g <= 1, 0 <= min_p=%g <= 1)",
             (double)sample_temperature, (long)top_k, (double)top_p, (double)min_p);
  const int k = top_k >= V ? 0 : (int)top_k;
  const dim3 grid((unsigned)(N * n));
  if (k > 0 || top_p < 1.f || min_p > 0.f || sample_temperature != 1.f) {
    UG_REQUIRE(V <= AR_MAXV, "ug_maskgit_step_ex: a filter or a sampling temperature needs V=%ld <= %d (the row is staged in LDS)", (long)V,
               AR_MAXV);
    const int vec = ld % 8 == 0 && ug_aligned16(logits);
    hipLaunchKernelGGL(maskgit_sample_filtered_kernel, grid, dim3(ARS_T), 0, st, (const bf16_t*)logits, ld, (int)V, (int)N, (int)n, cfg,
                       guidance_scale, 1.f / sample_temperature, vec, u_sample, cur_ids, mask_id, k, top_p,
                       min_p > 0.f ? logf(min_p) : -INFINITY, sampled, sel_ws, logp, stats);
  } else if (logp || stats) {                         // the parent's draw, bit for bit, with the two outputs riding along
    hipLaunchKernelGGL(maskgit_sample_kernel<true>, grid, dim3(SMP_T), 0, st, (const bf16_t*)logits, ld, (int)V, (int)N, (int)n, cfg,
                       guidance_scale, u_sample, cur_ids, mask_id, sampled, sel_ws, logp, stats);
  } else {
    hipLaunchKernelGGL(maskgit_sample_kernel<false>, grid, dim3(SMP_T), 0, st, (const bf16_t*)logits, ld, (int)V, (int)N, (int)n, cfg,
                       guidance_scale, u_sample, cur_ids, mask_id, sampled, sel_ws, (float*)nullptr, (float*)nullptr);
  }
  UG_CHECK_LAUNCH("ug_maskgit_step_ex(sample)");
  return maskgit_remask_launch("ug_maskgit_step_ex(remask)", sel_ws, u_conf, cur_ids, sampled, mask_id, id_offset, mask_len_sched,
                               temperature, N, n, next_cur, next_ids, masking_out, st);
}

extern "C" int ug_ar_sample(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                            const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed,
                            int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, hipStream_t st) {
  return ar_sample_launch("ug_ar_sample", acc, ldacc, bsz, V, guidance_scale, temperature, greedy, uniforms, pos_dev, pos0, nsteps, embed,
                          ld_embed, H, id_offset, tok, out_tokens, x, nullptr, st);
}

extern "C" int ug_ar_sample_logp(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                                 const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed,
                                 int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, float* logp,
                                 hipStream_t st) {
  UG_REQUIRE(logp, "ug_ar_sample_logp: null logp (ug_ar_sample is the entry point without the output)");
  return ar_sample_launch("ug_ar_sample_logp", acc, ldacc, bsz, V, guidance_scale, temperature, greedy, uniforms, pos_dev, pos0, nsteps,
                          embed, ld_embed, H, id_offset, tok, out_tokens, x, logp, st);
}

extern "C" int ug_ar_sample_filtered(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature,
                                     int greedy, const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps,
                                     const float* embed, int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens,
                                     float* x, int64_t top_k, float top_p, float min_p, float* stats, hipStream_t st) {
  return ar_sample_filtered_launch("ug_ar_sample_filtered", acc, ldacc, bsz, V, guidance_scale, temperature, greedy, uniforms, pos_dev, pos0,
                                   nsteps, embed, ld_embed, H, id_offset, tok, out_tokens, x, top_k, top_p, min_p, stats, nullptr, st);
}

extern "C" int ug_ar_sample_filtered_logp(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature,
                                          int greedy, const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps,
                                          const float* embed, int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok,
                                          int* out_tokens, float* x, int64_t top_k, float top_p, float min_p, float* stats, float* logp,
                                          hipStream_t st) {
  UG_REQUIRE(logp, "ug_ar_sample_filtered_logp: null logp (ug_ar_sample_filtered is the entry point without the output)");
  return ar_sample_filtered_launch("ug_ar_sample_filtered_logp", acc, ldacc, bsz, V, guidance_scale, temperature, greedy, uniforms, pos_dev,
                                   pos0, nsteps, embed, ld_embed, H, id_offset, tok, out_tokens, x, top_k, top_p, min_p, stats, logp, st);
}
