// Token pick of a text decode step over the WHOLE vocabulary, on the device (UniGen.generate / mmu_generate / mmu_generate_batch with
// on_device=True): the head's fp32 logits [R][ld] -> one token per row, the stop rule of models/unigen.py: emit_until_stop, the
// token's slot in the output buffer and the embedding row that feeds the next step.  Contract: include/unigen_hip.h (ug_text_pick,
// ug_text_sample; the repetition penalty in front of the pick: ug_text_seen_mark, ug_text_penalize; the constraints in front of the
// penalty and the stop sequences behind the pick: ug_text_constrain, ug_text_stop_seq).  Plain HIP C++: no inline assembly,
// no float atomics; integer atomics only where their order cannot change the result (histogram counts, a maximum, a minimum, the count
// of unfinished rows, the arrival ticket that advances the step counter, the OR of a prompt id's bit into the seen bitmap).
//
// State block (int32, device memory, reset by the host at the start of a call to {0, R, 0, 0, 0...}):
//   [0] step        the kernels' own step counter: read by every workgroup at its start, advanced by the LAST workgroup of the
//                   finishing launch to arrive (so every workgroup of a step has read it before it moves)
//   [1] remaining   rows not yet done
//   [2] steps_used  step + 1 of the step in which `remaining` reached zero (0: not yet)
//   [3] arrived     the arrival ticket (0 between launches)
//   [4 + r] done[r]
#include "common.h"
#include "unigen_hip.h"

namespace {

constexpr int TXT_T = 1024;            // one workgroup per row
constexpr int TXT_W = TXT_T / 64;
constexpr int TXT_MAX_ROWS = 32;
constexpr int TXT_MAX_STOP = 8;
constexpr int TXT_BINS = 65536;        // one bin per bf16 pattern
constexpr int TXT_MAXV = 262144;       // ug_text_sample: launch C keeps one 64-bit match mask per 64 entries in LDS (32 KiB)
constexpr int TXT_SEG = 8192;          // entries per workgroup of the histogram launch
constexpr int TXT_HT = 256;
constexpr int TXT_NEGINF_POS = TXT_BINS - 1 - 0x7f;   // text_select_kernel's position of the key of -inf (bf16 0xff80 -> key 0x007f)

struct TextOut {
  const int64_t* stop_ids;
  int n_stop;
  int64_t pad_id;
  const float* embed;
  int64_t lde;
  int H;
  int* state;
  int nsteps;
  int R;
  int64_t* tok;
  int* out_tokens;
  int* lengths;
  float* x;
  float* logp;                         // [R][nsteps] log-probability of every emitted token (the _logp entry points; else null)
};

// bf16 pattern -> 16-bit key whose unsigned order is the order of the values (-0 and +0 share a key)
__device__ __forceinline__ uint32_t txt_key(bf16_t b) {
  uint32_t k = b;
  if (k == 0x8000u) k = 0u;
  return (k ^ ((k >> 15) ? 0xffffu : 0x8000u)) & 0xffffu;
}
__device__ __forceinline__ float txt_unkey(uint32_t k) { return bf2f((bf16_t)(k ^ ((k >> 15) ? 0x8000u : 0xffffu))); }

// v of a key: bf16 value x fp32(1 / temperature), ROUNDED (never contracted into the subtraction of the maximum that follows it:
// v is the fp32 number the contract defines, and every use sees the same one)
__device__ __forceinline__ float txt_val(uint32_t key, float inv_temp) { return __fmul_rn(txt_unkey(key), inv_temp); }

// The end of a step for row r (every thread of the row's workgroup calls it; `picked` is uniform): pad rule, records, stop rule, next
// input, then the arrival ticket.  s_token: one int of LDS.  LOGP: lp = the log-probability of `picked` under the step's distribution;
// a row that had finished before the step records 0.
template <bool LOGP>
__device__ __forceinline__ void txt_finish_row(const TextOut& o, int r, int picked, int step, int* s_token, float lp = 0.f) {
  const int t = threadIdx.x;
  if (t == 0) {
    int* done = o.state + 4;
    const int was = done[r];
    const int64_t token = (was && o.pad_id >= 0) ? o.pad_id : (int64_t)picked;
    o.tok[r] = token;
    if (step < o.nsteps) o.out_tokens[(int64_t)r * o.nsteps + step] = (int)token;
    if (LOGP && step < o.nsteps) o.logp[(int64_t)r * o.nsteps + step] = was ? 0.f : lp;
    bool stop = false;
    for (int i = 0; i < o.n_stop; ++i) stop |= o.stop_ids[i] == token;
    if (stop && !was) {
      if (o.lengths) o.lengths[r] = step + 1;
      done[r] = 1;
      if (atomicSub(&o.state[1], 1) == 1) o.state[2] = step + 1;
    }
    *s_token = (int)token;
  }
  __syncthreads();
  const int token = *s_token;
  const float4* er = reinterpret_cast<const float4*>(o.embed + (int64_t)token * o.lde);
  float4* xr = reinterpret_cast<float4*>(o.x + (int64_t)r * o.H);
  for (int i = t; i < (o.H >> 2); i += blockDim.x) xr[i] = er[i];
  if (t == 0) {
    __threadfence();
    if (atomicAdd(&o.state[3], 1) == o.R - 1) { o.state[3] = 0; o.state[0] = step + 1; }
  }
}

__device__ __forceinline__ int txt_read_step(const int* state, int* s_step) {
  if (threadIdx.x == 0) *s_step = *reinterpret_cast<const volatile int*>(state);
  __syncthreads();
  return *s_step;
}

// ------------------------------------------------------------------ greedy: argmax of the bf16-rounded logits, lowest index on ties
// VEC: rows that start on 16-byte boundaries (ld % 4 == 0) are read four entries at a time
// LOGP: the log-softmax of the bf16 values at the picked token, formed in the same single pass (the row is cleared on the way): thread t
// keeps sum = the sum of exp(value - mx) over the candidates it has seen, rescaled whenever its running maximum mx moves; -inf adds 0, a
// NaN is no candidate.  Behind the block maximum: every thread's sum rescaled to it, an xor tree over the wave, the sixteen wave partials
// in wave order -- a fixed order.  The picked token holds the maximum, so its log-probability is -log(total).
template <bool VEC, bool LOGP>
__global__ __launch_bounds__(TXT_T) void text_pick_kernel(float* __restrict__ logits, int64_t ld, int V, int clear, TextOut o) {
  __shared__ float red[TXT_W];
  __shared__ int best_i[TXT_W];
  __shared__ int s_step, s_token;
  __shared__ float sum_w[LOGP ? TXT_W : 1];
  float sum = 0.f;
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int step = txt_read_step(o.state, &s_step);
  float* row = logits + (int64_t)r * ld;
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  if (VEC) {
    float4* row4 = reinterpret_cast<float4*>(row);
    const int n4 = (V + 3) >> 2;                                  // (ld is a multiple of 4: the last vector stays inside the row)
    for (int i = t; i < n4; i += TXT_T) {                         // ascending indices per thread: `>` keeps the lowest
      const float4 q = row4[i];
      const float vv[4] = {q.x, q.y, q.z, q.w};
      const int e0 = 4 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = bf2f(f2bf(vv[j]));
        if (LOGP) {
          if (e0 + j < V) {
            if (v > mx) { sum = __fmaf_rn(sum, expf(mx - v), 1.f); mx = v; arg = e0 + j; }
            else if (v > -INFINITY) sum += expf(v - mx);
          }
        } else if (e0 + j < V && v > mx) { mx = v; arg = e0 + j; }      // (entries V .. ld-1 are read, never candidates)
      }
      if (clear) {
        if (e0 + 3 < V) row4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else
          for (int j = 0; e0 + j < V; ++j) row[e0 + j] = 0.f;    // nothing is written past the V read entries
      }
    }
  } else {
#pragma unroll 8
    for (int e = t; e < V; e += TXT_T) {
      const float v = bf2f(f2bf(row[e]));
      if (v > mx) { if (LOGP) sum = __fmaf_rn(sum, expf(mx - v), 1.f); mx = v; arg = e; }
      else if (LOGP && v > -INFINITY) sum += expf(v - mx);
      if (clear) row[e] = 0.f;
    }
  }
  const float mx_t = mx;                                          // (LOGP: this thread's own maximum, before the wave's replaces it)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mx, off, 64);
    const int oi = __shfl_xor(arg, off, 64);
    if (om > mx || (om == mx && oi < arg)) { mx = om; arg = oi; }
  }
  if (lane == 0) { red[wave] = mx; best_i[wave] = arg; }
  __syncthreads();
  float bmx = red[0];
  int bi = best_i[0];
#pragma unroll
  for (int w = 1; w < TXT_W; ++w)
    if (red[w] > bmx || (red[w] == bmx && best_i[w] < bi)) { bmx = red[w]; bi = best_i[w]; }
  if (bi >= V) bi = 0;                                            // (no finite candidate: torch.argmax answers 0 for a row of -inf)
  float lp = 0.f;
  if (LOGP) {
    float part = sum > 0.f ? __fmul_rn(sum, expf(mx_t - bmx)) : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == 0) sum_w[wave] = part;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int w = 0; w < TXT_W; ++w) total += sum_w[w];
    lp = -logf(total);
  }
  txt_finish_row<LOGP>(o, r, bi, step, &s_token, lp);
}

// ------------------------------------------------------------------ sampled pick, launch A: per-row histogram of the 16-bit keys
// grid (segments, R).  hist [R][65536] int32 and rowmax [R] are zero on entry (launch B leaves them so).
__global__ __launch_bounds__(TXT_HT) void text_hist_kernel(const float* __restrict__ logits, int64_t ld, int V, int* __restrict__ hist,
                                                          int* __restrict__ rowmax) {
  const int r = blockIdx.y, t = threadIdx.x;
  const float* row = logits + (int64_t)r * ld;
  int* h = hist + (int64_t)r * TXT_BINS;
  const int e0 = blockIdx.x * TXT_SEG, e1 = min(V, e0 + TXT_SEG);
  int mk = 0;
  for (int e = e0 + t; e < e1; e += TXT_HT) {
    const float f = row[e];
    if (f != f) continue;                                          // a NaN logit is no candidate
    const int k = (int)txt_key(f2bf(f));
    atomicAdd(&h[k], 1);
    mk = max(mk, k);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mk = max(mk, __shfl_xor(mk, off, 64));
  if ((t & 63) == 0) atomicMax(&rowmax[r], mk);
}

// exclusive prefix of `v` over the workgroup's threads in thread order (wave scan, then a four-level scan of the sixteen wave totals);
// total = the sum over all threads.  Fixed order: a function of the inputs.  One barrier pair; `wt` is TXT_W slots of LDS.
template <typename T>
__device__ __forceinline__ T txt_scan_excl(T v, T* wt, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T n = __shfl_up(incl, off, 64);
    if (lane >= off) incl += n;
  }
  __syncthreads();
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  T w = lane < TXT_W ? wt[lane] : (T)0;
  T winc = w;
#pragma unroll
  for (int off = 1; off < TXT_W; off <<= 1) {
    const T n = __shfl_up(winc, off, 64);
    if (lane >= off) winc += n;
  }
  total = __shfl(winc, TXT_W - 1, 64);
  const T base = __shfl(winc - w, wave, 64);
  return base + (incl - v);
}

// ------------------------------------------------------------------ launch B: the whole selection of one row on its histogram
// Positions p = 0 .. 65535 run over the keys in DESCENDING order (key = 65535 - p); thread t holds p in [64 t, 64 t + 64).
// meta (int32): rowmax [32] | sel_key [32] | sel_rank [32].
// LOGP: the drawn token's log-probability (v of the drawn key - max v - log T, T the kept mass formed below) travels to the locate launch
// as the bits of rowmax[r], which that launch zeroes again.
template <bool LOGP>
__global__ __launch_bounds__(TXT_T) void text_select_kernel(int* __restrict__ hist, int* __restrict__ meta, int V, float inv_temp, int top_k,
                                                           float top_p, const float* __restrict__ uniforms, const int* __restrict__ state,
                                                           int nsteps, int R, float* __restrict__ stats) {
  __shared__ int wt_i[TXT_W];
  __shared__ float wt_f[TXT_W];
  __shared__ int s_step, s_pk, s_pc, s_kept, s_hit, s_pf;
  __shared__ float s_T;
  const int r = blockIdx.x, t = threadIdx.x;
  const int step = min(txt_read_step(state, &s_step), nsteps - 1);
  int4* h4 = reinterpret_cast<int4*>(hist + (int64_t)r * TXT_BINS);
  // thread t: keys 65535 - 64 t down to 65535 - 64 t - 63 = the 16 int4 at [16 (1023 - t), +16), read back to front
  int cnt[64];
  const int v0 = 16 * (TXT_T - 1 - t);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int4 q = h4[v0 + 15 - j];
    cnt[4 * j] = q.w; cnt[4 * j + 1] = q.z; cnt[4 * j + 2] = q.y; cnt[4 * j + 3] = q.x;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) h4[v0 + j] = make_int4(0, 0, 0, 0);                 // the bins are ready for the next step
  const float vmax = txt_val((uint32_t)meta[r], inv_temp);
  const float u01 = uniforms[(int64_t)step * R + r];
  if (t == 0) { s_pk = TXT_BINS - 1; s_pc = 0; s_kept = 0; s_hit = TXT_BINS; s_pf = -1; }
  const int p0 = 64 * t;
  // ---- top-k: the position of the k-th largest entry, duplicates counted (exact: integer sums)
  int nloc = 0;
#pragma unroll
  for (int i = 0; i < 64; ++i) nloc += cnt[i];
  int ntot;
  const int nbase = txt_scan_excl<int>(nloc, wt_i, ntot);        // (its barriers also publish the initial values above)
  if (top_k > 0 && top_k < ntot && nbase < top_k && top_k <= nbase + nloc) {
    int run = nbase, pk = p0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      run += cnt[i];
      if (!found && run >= top_k) { pk = p0 + i; found = true; }
    }
    s_pk = pk;
  }
  __syncthreads();
  const int pk = s_pk;
  // ---- masses over S_k = {p <= pk}: count x exp(v - max), chunk in key order, scan in the wave, wave totals
  auto mass = [&](int i) -> float {
    return (float)cnt[i] * expf(txt_val((uint32_t)(TXT_BINS - 1 - (p0 + i)), inv_temp) - vmax);
  };
  float mloc = 0.f;
#pragma unroll
  for (int i = 0; i < 64; ++i)
    if (cnt[i] > 0 && p0 + i <= pk) mloc += mass(i);
  float Z;
  const float mbase = txt_scan_excl<float>(mloc, wt_f, Z);
  // ---- top-p: a value is kept iff the mass of the strictly greater values of S_k is <= top_p * Z (a prefix of the positions);
  // the cut pc = the last kept non-empty position, `kept` = the entries up to it
  const float lim = top_p * Z;
  {
    float run = mbase;
    int last = -1, lastf = -1, kept = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i)
      if (cnt[i] > 0 && p0 + i <= pk) {
        if (top_p >= 1.f || run <= lim) {
          last = p0 + i; kept += cnt[i];
          if (p0 + i != TXT_NEGINF_POS) lastf = last;                // (the last kept key that is not -inf: see `hit` below)
        }
        run += mass(i);
      }
    if (last >= 0) { atomicMax(&s_pc, last); atomicAdd(&s_kept, kept); }
    if (lastf >= 0) atomicMax(&s_pf, lastf);
  }
  __syncthreads();
  const int pc = s_pc;
  // total kept mass T = the running sum just behind pc, formed by the thread that owns pc exactly as the walk below forms it
  if (pc >= p0 && pc < p0 + 64) {
    float run = mbase;
#pragma unroll
    for (int i = 0; i < 64; ++i)
      if (cnt[i] > 0 && p0 + i <= pc) run += mass(i);
    s_T = run;
  }
  __syncthreads();
  // ---- draw: the first kept position whose running sum passes u * T (value descending); the rank inside the key from the residual
  const float target = u01 * s_T;
  {
    float run = mbase;
    int hit = TXT_BINS;
#pragma unroll
    for (int i = 0; i < 64; ++i)
      if (cnt[i] > 0 && p0 + i <= pc) {
        run += mass(i);
        if (hit == TXT_BINS && target < run) hit = p0 + i;
      }
    if (hit < TXT_BINS) atomicMin(&s_hit, hit);
  }
  __syncthreads();
  // rounding left the target behind the last bound: the last kept key -- but never the key of -inf while another is kept: an entry a
  // logits processor wrote -inf into (ug_text_constrain) has mass 0 and is never drawn
  const int hit = s_hit < TXT_BINS ? s_hit : (pc == TXT_NEGINF_POS && s_pf >= 0 ? s_pf : pc);
  if (hit >= p0 && hit < p0 + 64) {
    float run = mbase, e = 1.f;
    int c = 1;
    bool seen = false;
#pragma unroll
    for (int i = 0; i < 64; ++i)
      if (cnt[i] > 0 && p0 + i <= pc && !seen) {
        if (p0 + i == hit) {
          seen = true; c = cnt[i];
          e = expf(txt_val((uint32_t)(TXT_BINS - 1 - hit), inv_temp) - vmax);
        } else {
          run += mass(i);
        }
      }
    int j = s_hit < TXT_BINS ? (int)floorf(fmaxf(target - run, 0.f) / e) : c - 1;
    j = max(0, min(c - 1, j));
    meta[32 + r] = TXT_BINS - 1 - hit;
    meta[64 + r] = j;
  }
  if (t == 0) {
    meta[r] = LOGP ? __float_as_int((txt_val((uint32_t)(TXT_BINS - 1 - hit), inv_temp) - vmax) - logf(s_T)) : 0;
    if (stats) {
      stats[2 * r] = txt_val((uint32_t)(TXT_BINS - 1 - pc), inv_temp);
      stats[2 * r + 1] = (float)s_kept;
    }
  }
}

// ------------------------------------------------------------------ launch C: the rank-th index holding the selected key, in index order
// Wave w owns the contiguous entries [w CW, (w + 1) CW), CW a multiple of 64; iteration i covers 64 consecutive entries.
template <bool LOGP>
__global__ __launch_bounds__(TXT_T) void text_locate_kernel(float* __restrict__ logits, int64_t ld, int V, int clear, int* __restrict__ meta,
                                                           TextOut o) {
  __shared__ unsigned long long masks[TXT_MAXV / 64];
  __shared__ int wtot[TXT_W];
  __shared__ int s_step, s_token, s_pick;
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int step = txt_read_step(o.state, &s_step);
  const int key = meta[32 + r], rank = meta[64 + r];
  const float lp = LOGP ? __int_as_float(meta[r]) : 0.f;           // (read by every thread ahead of the barriers; zeroed behind them)
  float* row = logits + (int64_t)r * ld;
  const int iters = (V + 64 * TXT_W - 1) / (64 * TXT_W);           // per wave
  const int w0 = wave * iters * 64;
  int mine = 0;
  for (int i = 0; i < iters; ++i) {
    const int e = w0 + i * 64 + lane;
    bool m = false;
    if (e < V) {
      const float f = row[e];
      m = f == f && (int)txt_key(f2bf(f)) == key;
      if (clear) row[e] = 0.f;
    }
    const unsigned long long b = __ballot(m);
    if (lane == 0) masks[wave * iters + i] = b;
    mine += __popcll(b);                                           // (uniform over the wave)
  }
  if (lane == 0) wtot[wave] = mine;
  if (t == 0) s_pick = -1;
  __syncthreads();
  int total = 0, wsel = -1, before = 0;
#pragma unroll
  for (int w = 0; w < TXT_W; ++w) {
    const int c = wtot[w];
    if (wsel < 0 && rank < total + c) { wsel = w; before = total; }
    total += c;
  }
  int want = rank - before;
  if (wsel < 0) { wsel = -2; }                                     // (fewer holders than the rank: cannot happen on unchanged logits)
  if (wave == wsel) {
    int run = 0;
    for (int c0 = 0; c0 < iters; c0 += 64) {
      const int i = c0 + lane;
      const unsigned long long b = i < iters ? masks[wave * iters + i] : 0ull;
      const int c = __popcll(b);
      int incl = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int n = __shfl_up(incl, off, 64);
        if (lane >= off) incl += n;
      }
      const int excl = run + incl - c;
      if (excl <= want && want < excl + c) {
        unsigned long long bb = b;
        for (int s = want - excl; s > 0; --s) bb &= bb - 1;        // drop the lower set bits
        s_pick = w0 + i * 64 + (__ffsll((long long)bb) - 1);
      }
      run += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
  int pick = s_pick;
  if (pick < 0 || pick >= V) pick = 0;
  if (t == 0) { meta[32 + r] = 0; meta[64 + r] = 0; if (LOGP) meta[r] = 0; }
  txt_finish_row<LOGP>(o, r, pick, step, &s_token, lp);
}

// ------------------------------------------------------------------ repetition penalty: the logits processor in front of the pick
// seen [R][ld_words]: bit (e & 31) of word (e >> 5) is set iff id e occurs in the row's sequence so far.  Mark: one thread per prompt
// position; an integer OR, whose order cannot matter.
__global__ __launch_bounds__(TXT_HT) void text_seen_mark_kernel(int* __restrict__ seen, int64_t ld_words, const int64_t* __restrict__ ids,
                                                               int64_t ld_ids, int L, const uint8_t* __restrict__ valid, int V) {
  const int r = blockIdx.y, l = blockIdx.x * TXT_HT + threadIdx.x;
  if (l >= L) return;
  if (valid && !valid[(int64_t)r * L + l]) return;
  const int64_t id = ids[(int64_t)r * ld_ids + l];
  if (id < 0 || id >= V) return;
  atomicOr(&seen[(int64_t)r * ld_words + (id >> 5)], (int)(1u << (id & 31)));
}

// Penalize: grid (word blocks, R); a thread owns ONE bitmap word of one row (a wave reads 256 contiguous bytes of the bitmap) and the up
// to 32 logits its bits name -- nobody else reads or writes either, so plain loads and stores, no atomics, no reductions: the launch is
// a function of its inputs.  The logits of unseen ids are never loaded.
__global__ __launch_bounds__(TXT_HT) void text_penalize_kernel(float* __restrict__ logits, int64_t ld, int V, float penalty, int* __restrict__ seen,
                                                              int64_t ld_words, const int64_t* __restrict__ tok) {
  const int r = blockIdx.y, w = blockIdx.x * TXT_HT + threadIdx.x;
  const int W = (V + 31) >> 5;
  if (w >= W) return;
  int* sw = seen + (int64_t)r * ld_words + w;
  uint32_t word = (uint32_t)*sw;
  if (tok) {                                                       // the token the previous step emitted joins the row's sequence
    const int64_t tk = tok[r];
    if (tk >= 0 && tk < V && (int)(tk >> 5) == w) {
      word |= 1u << (tk & 31);
      *sw = (int)word;
    }
  }
  if (w == W - 1 && (V & 31)) word &= (1u << (V & 31)) - 1u;       // bits at or above V are never acted on
  float* row = logits + (int64_t)r * ld + 32 * w;
  while (word) {
    const int b = __ffs((int)word) - 1;
    word &= word - 1;
    const float s = bf2f(f2bf(row[b]));                            // the value the pick sees; NaN < 0 is false and NaN / p is NaN
    row[b] = s < 0.f ? __fmul_rn(s, penalty) : __fdiv_rn(s, penalty);
  }
}

// ------------------------------------------------------------------ constraints: the logits processor in front of the penalty
// One workgroup per row; a row's logits are touched by its workgroup alone.  Phase 1: thread j owns bias entry j (the ids of the list are
// distinct, so no two threads share a logit).  Barrier.  Phase 2: the -inf stores -- several threads may store -inf into one entry, the
// same bits whatever their order.  Plain loads and stores, no atomics, no float reductions: the launch is a function of its inputs.
constexpr int TXT_MAX_BIAS = 1024;
constexpr int TXT_MAX_NGRAM = 16;
constexpr int TXT_MAX_SEQS = 8;
constexpr int TXT_MAX_SEQ_LEN = 16;

struct TextBias { int id; float bias; };

__global__ __launch_bounds__(TXT_HT) void text_constrain_kernel(float* __restrict__ logits, int64_t ld, int V, const TextBias* __restrict__ bias,
                                                               int n_bias, int min_new, const int64_t* __restrict__ stop_ids, int n_stop,
                                                               int n, const int* __restrict__ hist, int64_t ld_hist,
                                                               const int* __restrict__ hist_len, const int* __restrict__ out_tokens,
                                                               int nsteps, const int* __restrict__ state) {
  __shared__ int s_suf[TXT_MAX_NGRAM];
  const int r = blockIdx.x, t = threadIdx.x;
  const int step = max(0, min(*reinterpret_cast<const volatile int*>(state), nsteps));      // (read, never advanced: the pick does that)
  float* row = logits + (int64_t)r * ld;
  const int P = (hist && hist_len) ? max(0, min(hist_len[r], (int)ld_hist)) : 0;
  const int T = P + step;                                          // the combined history: prompt ids, then out_tokens[r][0 .. step)
  const int* hp = P ? hist + (int64_t)r * ld_hist : nullptr;
  const int* ho = out_tokens ? out_tokens + (int64_t)r * nsteps : nullptr;        // (null only with n == 0: h is then never called)
  auto h = [&](int j) -> int { return j < P ? hp[j] : ho[j - P]; };
  for (int j = t; j < n_bias; j += TXT_HT) {
    const TextBias b = bias[j];
    if (b.id < 0 || b.id >= V) continue;
    row[b.id] = b.bias == -INFINITY ? -INFINITY : __fadd_rn(bf2f(f2bf(row[b.id])), b.bias);
  }
  const bool grams = n > 0 && T >= n - 1;
  if (grams && t < n - 1) s_suf[t] = h(T - n + 1 + t);             // the last n - 1 ids of the history
  __syncthreads();
  if (step < min_new && t < n_stop) {
    const int64_t e = stop_ids[t];
    if (e >= 0 && e < V) row[e] = -INFINITY;
  }
  if (!grams) return;
  for (int i = t; i + n <= T; i += TXT_HT) {
    bool same = true;
    for (int k = 0; k < n - 1; ++k) same &= h(i + k) == s_suf[k];
    if (!same) continue;
    const int e = h(i + n - 1);
    if (e >= 0 && e < V) row[e] = -INFINITY;                       // (an id outside [0, V) is compared, never used as an index)
  }
}

// Stop sequences: thread r owns row r.  The row's last m emitted tokens against every sequence of length m <= step + 1; what a match
// does is txt_finish_row's stop branch.  One workgroup: `remaining` needs an atomic only for the symmetry with the pick.
__global__ __launch_bounds__(64) void text_stop_seq_kernel(const int* __restrict__ seq_ids, const int* __restrict__ seq_off, int ns, int n_ids,
                                                          const int* __restrict__ out_tokens, int nsteps, int R, int* __restrict__ state,
                                                          int* __restrict__ lengths) {
  const int r = threadIdx.x;
  const int step = *reinterpret_cast<const volatile int*>(state) - 1;        // the step the pick launch has just finished
  if (r >= R || step < 0 || step >= nsteps) return;
  int* done = state + 4;
  if (done[r]) return;                                             // (a row never finishes twice)
  const int* row = out_tokens + (int64_t)r * nsteps;
  for (int s = 0; s < ns; ++s) {
    const int o0 = seq_off[s], m = seq_off[s + 1] - o0;
    if (o0 < 0 || m < 1 || m > TXT_MAX_SEQ_LEN || o0 + m > n_ids || m > step + 1) continue;      // (never a column before 0)
    bool same = true;
    for (int k = 0; k < m; ++k) same &= row[step - m + 1 + k] == seq_ids[o0 + k];
    if (!same) continue;
    if (lengths) lengths[r] = step + 1;
    done[r] = 1;
    if (atomicSub(&state[1], 1) == 1) state[2] = step + 1;
    return;
  }
}

int txt_check_out(const char* who, float* logits, int64_t ld, int64_t R, int64_t V, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                  const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                  int* out_tokens, float* x) {
  UG_REQUIRE(logits && embed && state && tok && out_tokens && x && (n_stop == 0 || stop_ids), "%s: null argument", who);
  UG_REQUIRE(R > 0 && R <= TXT_MAX_ROWS && V > 0 && ld >= V && R * ld < (1ll << 31) && nsteps > 0 && n_stop >= 0 &&
                 n_stop <= TXT_MAX_STOP,
             "%s: bad sizes (R=%ld <= %d, V=%ld <= ld=%ld, R*ld < 2^31, nsteps=%ld, n_stop=%ld <= %d)", who, (long)R,
             TXT_MAX_ROWS, (long)V, (long)ld, (long)nsteps, (long)n_stop, TXT_MAX_STOP);
  UG_REQUIRE(H > 0 && H % 4 == 0 && ld_embed % 4 == 0 && ld_embed >= H && embed_rows >= V && pad_id < embed_rows && ug_aligned16(embed) &&
                 ug_aligned16(x),
             "%s: bad table (H=%ld, ld_embed=%ld, rows=%ld >= V, pad_id=%ld below rows; 16-byte aligned table / x)", who, (long)H,
             (long)ld_embed, (long)embed_rows, (long)pad_id);
  return UG_OK;
}

}  // namespace

extern "C" int ug_text_pick(float* logits, int64_t ld, int64_t R, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop,
                            int64_t pad_id, const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state,
                            int64_t nsteps, int64_t* tok, int* out_tokens, int* lengths, float* x, hipStream_t st) {
  const int rc = txt_check_out("ug_text_pick", logits, ld, R, V, stop_ids, n_stop, pad_id, embed, ld_embed, embed_rows, H, state, nsteps, tok,
                               out_tokens, x);
  if (rc != UG_OK) return rc;
  const TextOut o{stop_ids, (int)n_stop, pad_id, embed, ld_embed, (int)H, state, (int)nsteps, (int)R, tok, out_tokens, lengths, x, nullptr};
  if (ld % 4 == 0 && ug_aligned16(logits))
    hipLaunchKernelGGL((text_pick_kernel<true, false>), dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, o);
  else
    hipLaunchKernelGGL((text_pick_kernel<false, false>), dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, o);
  UG_CHECK_LAUNCH("ug_text_pick");
  return UG_OK;
}

extern "C" int ug_text_pick_logp(float* logits, int64_t ld, int64_t R, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop,
                                 int64_t pad_id, const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state,
                                 int64_t nsteps, int64_t* tok, int* out_tokens, int* lengths, float* x, float* logp, hipStream_t st) {
  UG_REQUIRE(logp, "ug_text_pick_logp: null logp (ug_text_pick is the entry point without the output)");
  const int rc = txt_check_out("ug_text_pick_logp", logits, ld, R, V, stop_ids, n_stop, pad_id, embed, ld_embed, embed_rows, H, state, nsteps,
                               tok, out_tokens, x);
  if (rc != UG_OK) return rc;
  const TextOut o{stop_ids, (int)n_stop, pad_id, embed, ld_embed, (int)H, state, (int)nsteps, (int)R, tok, out_tokens, lengths, x, logp};
  if (ld % 4 == 0 && ug_aligned16(logits))
    hipLaunchKernelGGL((text_pick_kernel<true, true>), dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, o);
  else
    hipLaunchKernelGGL((text_pick_kernel<false, true>), dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, o);
  UG_CHECK_LAUNCH("ug_text_pick_logp");
  return UG_OK;
}

extern "C" int ug_text_sample_workspace_ints(int64_t R) {
  if (R <= 0 || R > TXT_MAX_ROWS) {
    ug_set_error("ug_text_sample_workspace_ints: R=%ld must be in 1..%d", (long)R, TXT_MAX_ROWS);
    return UG_ERR_ARG;
  }
  return (int)(R * TXT_BINS + 96);
}

namespace {
// argument checks + the three launches of ug_text_sample / ug_text_sample_logp (logp null: the kernels without the output)
int txt_sample_launch(const char* who, float* logits, int64_t ld, int64_t R, int64_t V, int clear, float temperature, int64_t top_k, float top_p,
                      const float* uniforms, int* workspace, float* stats, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                      const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                      int* out_tokens, int* lengths, float* x, float* logp, hipStream_t st) {
  const int rc = txt_check_out(who, logits, ld, R, V, stop_ids, n_stop, pad_id, embed, ld_embed, embed_rows, H, state, nsteps, tok, out_tokens, x);
  if (rc != UG_OK) return rc;
  UG_REQUIRE(uniforms && workspace && ug_aligned16(workspace), "%s: null or misaligned uniforms / workspace", who);
  UG_REQUIRE(V <= TXT_MAXV, "%s: V=%ld exceeds the %d entries this build locates a token among", who, (long)V, TXT_MAXV);
  UG_REQUIRE(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f,
             "%s: bad filter (temperature=%g > 0, top_k=%ld >= 0, 0 < top_p=%g <= 1)", who, (double)temperature, (long)top_k, (double)top_p);
  const TextOut o{stop_ids, (int)n_stop, pad_id, embed, ld_embed, (int)H, state, (int)nsteps, (int)R, tok, out_tokens, lengths, x, logp};
  int* meta = workspace + R * TXT_BINS;
  const int k = top_k >= V ? 0 : (int)top_k;
  hipLaunchKernelGGL(text_hist_kernel, dim3((unsigned)((V + TXT_SEG - 1) / TXT_SEG), (unsigned)R), dim3(TXT_HT), 0, st, logits, ld, (int)V,
                     workspace, meta);
  UG_CHECK_LAUNCH(who);
  if (logp)
    hipLaunchKernelGGL(text_select_kernel<true>, dim3((unsigned)R), dim3(TXT_T), 0, st, workspace, meta, (int)V, 1.f / temperature, k, top_p,
                       uniforms, state, (int)nsteps, (int)R, stats);
  else
    hipLaunchKernelGGL(text_select_kernel<false>, dim3((unsigned)R), dim3(TXT_T), 0, st, workspace, meta, (int)V, 1.f / temperature, k, top_p,
                       uniforms, state, (int)nsteps, (int)R, stats);
  UG_CHECK_LAUNCH(who);
  if (logp)
    hipLaunchKernelGGL(text_locate_kernel<true>, dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, meta, o);
  else
    hipLaunchKernelGGL(text_locate_kernel<false>, dim3((unsigned)R), dim3(TXT_T), 0, st, logits, ld, (int)V, clear, meta, o);
  UG_CHECK_LAUNCH(who);
  return UG_OK;
}
}  // namespace

extern "C" int ug_text_sample(float* logits, int64_t ld, int64_t R, int64_t V, int clear, float temperature, int64_t top_k, float top_p,
                              const float* uniforms, int* workspace, float* stats, const int64_t* stop_ids, int64_t n_stop,
                              int64_t pad_id, const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state,
                              int64_t nsteps, int64_t* tok, int* out_tokens, int* lengths, float* x, hipStream_t st) {
  return txt_sample_launch("ug_text_sample", logits, ld, R, V, clear, temperature, top_k, top_p, uniforms, workspace, stats, stop_ids, n_stop,
                           pad_id, embed, ld_embed, embed_rows, H, state, nsteps, tok, out_tokens, lengths, x, nullptr, st);
}

extern "C" int ug_text_sample_logp(float* logits, int64_t ld, int64_t R, int64_t V, int clear, float temperature, int64_t top_k, float top_p,
                                   const float* uniforms, int* workspace, float* stats, const int64_t* stop_ids, int64_t n_stop,
                                   int64_t pad_id, const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state,
                                   int64_t nsteps, int64_t* tok, int* out_tokens, int* lengths, float* x, float* logp, hipStream_t st) {
  UG_REQUIRE(logp, "ug_text_sample_logp: null logp (ug_text_sample is the entry point without the output)");
  return txt_sample_launch("ug_text_sample_logp", logits, ld, R, V, clear, temperature, top_k, top_p, uniforms, workspace, stats, stop_ids,
                           n_stop, pad_id, embed, ld_embed, embed_rows, H, state, nsteps, tok, out_tokens, lengths, x, logp, st);
}

extern "C" int ug_text_seen_mark(int* seen, int64_t ld_words, const int64_t* ids, int64_t ld_ids, int64_t R, int64_t L, const uint8_t* valid,
                                 int64_t V, hipStream_t st) {
  UG_REQUIRE(seen && ids, "ug_text_seen_mark: null argument");
  UG_REQUIRE(R > 0 && R <= TXT_MAX_ROWS && L > 0 && L < (1ll << 31) && ld_ids >= L && V > 0 && V < (1ll << 31) && ld_words >= (V + 31) / 32,
             "ug_text_seen_mark: bad sizes (R=%ld <= %d, 0 < L=%ld <= ld_ids=%ld, V=%ld, ld_words=%ld >= ceil(V / 32))", (long)R, TXT_MAX_ROWS,
             (long)L, (long)ld_ids, (long)V, (long)ld_words);
  hipLaunchKernelGGL(text_seen_mark_kernel, dim3((unsigned)((L + TXT_HT - 1) / TXT_HT), (unsigned)R), dim3(TXT_HT), 0, st, seen, ld_words, ids,
                     ld_ids, (int)L, valid, (int)V);
  UG_CHECK_LAUNCH("ug_text_seen_mark");
  return UG_OK;
}

extern "C" int ug_text_penalize(float* logits, int64_t ld, int64_t R, int64_t V, float penalty, int* seen, int64_t ld_words,
                                const int64_t* tok, hipStream_t st) {
  UG_REQUIRE(logits && seen, "ug_text_penalize: null argument");
  UG_REQUIRE(R > 0 && R <= TXT_MAX_ROWS && V > 0 && ld >= V && R * ld < (1ll << 31) && ld_words >= (V + 31) / 32,
             "ug_text_penalize: bad sizes (R=%ld <= %d, V=%ld <= ld=%ld, R*ld < 2^31, ld_words=%ld >= ceil(V / 32))", (long)R, TXT_MAX_ROWS,
             (long)V, (long)ld, (long)ld_words);
  UG_REQUIRE(penalty > 0.f && penalty <= 3.402823466e38f, "ug_text_penalize: penalty=%g must be finite and > 0", (double)penalty);
  const int64_t W = (V + 31) / 32;
  hipLaunchKernelGGL(text_penalize_kernel, dim3((unsigned)((W + TXT_HT - 1) / TXT_HT), (unsigned)R), dim3(TXT_HT), 0, st, logits, ld, (int)V,
                     penalty, seen, ld_words, tok);
  UG_CHECK_LAUNCH("ug_text_penalize");
  return UG_OK;
}

extern "C" int ug_text_constrain(float* logits, int64_t ld, int64_t R, int64_t V, const void* bias, int64_t n_bias, int64_t min_new,
                                 const int64_t* stop_ids, int64_t n_stop, int64_t ngram, const int* hist, int64_t ld_hist,
                                 const int* hist_len, const int* out_tokens, int64_t nsteps, const int* state, hipStream_t st) {
  UG_REQUIRE(logits && state && (n_bias == 0 || bias) && (n_stop == 0 || stop_ids) && (ngram == 0 || out_tokens) &&
                 (ld_hist == 0 || (hist && hist_len)),
             "ug_text_constrain: null argument");
  UG_REQUIRE(R > 0 && R <= TXT_MAX_ROWS && V > 0 && V < (1ll << 31) && ld >= V && R * ld < (1ll << 31) && nsteps > 0 && nsteps < (1ll << 31) &&
                 ld_hist >= 0 && R * ld_hist < (1ll << 31),
             "ug_text_constrain: bad sizes (R=%ld <= %d, V=%ld <= ld=%ld, R*ld < 2^31, nsteps=%ld, ld_hist=%ld, R*ld_hist < 2^31)", (long)R,
             TXT_MAX_ROWS, (long)V, (long)ld, (long)nsteps, (long)ld_hist);
  UG_REQUIRE(n_bias >= 0 && n_bias <= TXT_MAX_BIAS && min_new >= 0 && min_new < (1ll << 31) && n_stop >= 0 && n_stop <= TXT_MAX_STOP &&
                 ngram >= 0 && ngram <= TXT_MAX_NGRAM,
             "ug_text_constrain: bad constraints (n_bias=%ld <= %d, min_new=%ld >= 0, n_stop=%ld <= %d, ngram=%ld <= %d)", (long)n_bias,
             TXT_MAX_BIAS, (long)min_new, (long)n_stop, TXT_MAX_STOP, (long)ngram, TXT_MAX_NGRAM);
  hipLaunchKernelGGL(text_constrain_kernel, dim3((unsigned)R), dim3(TXT_HT), 0, st, logits, ld, (int)V, static_cast<const TextBias*>(bias),
                     (int)n_bias, (int)min_new, stop_ids, (int)n_stop, (int)ngram, hist, ld_hist, hist_len, out_tokens, (int)nsteps, state);
  UG_CHECK_LAUNCH("ug_text_constrain");
  return UG_OK;
}

extern "C" int ug_text_stop_seq(const int* seq_ids, const int* seq_off, int64_t ns, int64_t n_ids, const int* out_tokens, int64_t nsteps,
                                int64_t R, int* state, int* lengths, hipStream_t st) {
  UG_REQUIRE(seq_ids && seq_off && out_tokens && state, "ug_text_stop_seq: null argument");
  UG_REQUIRE(R > 0 && R <= TXT_MAX_ROWS && nsteps > 0 && nsteps < (1ll << 31) && R * nsteps < (1ll << 31) && ns > 0 && ns <= TXT_MAX_SEQS &&
                 n_ids >= 2 * ns && n_ids <= ns * TXT_MAX_SEQ_LEN,
             "ug_text_stop_seq: bad sizes (R=%ld <= %d, nsteps=%ld, 0 < ns=%ld <= %d sequences of 2 .. %d ids, n_ids=%ld)", (long)R,
             TXT_MAX_ROWS, (long)nsteps, (long)ns, TXT_MAX_SEQS, TXT_MAX_SEQ_LEN, (long)n_ids);
  hipLaunchKernelGGL(text_stop_seq_kernel, dim3(1), dim3(64), 0, st, seq_ids, seq_off, (int)ns, (int)n_ids, out_tokens, (int)nsteps, (int)R,
                     state, lengths);
  UG_CHECK_LAUNCH("ug_text_stop_seq");
  return UG_OK;
}
