// Beam search of the text loop, the two per-step pieces that are not the decode step itself (include/unigen_hip.h: "Beam search of
// the text loop"): ug_beam_candidates turns the head's fp32 logits of G groups x B beams into each group's K best continuations by
// log_softmax + running score, and ug_beam_kv_reorder moves the generated part of the KV cache to follow the parent beams.
// Plain HIP C++: no inline assembly, no float atomics; integer atomics only where their order cannot change the result (histogram
// counts, and the slot an entry takes in a list that is ranked by a total order afterwards).  Geometry and workspace: beam_plan.h.
//
// Candidates.  s[e] = bf16round(logit[e]) takes at most 65536 values, so a row's histogram over the bf16 patterns holds all that
// log_softmax needs: lse = m + log(sum over patterns of count * exp(value - m)), summed in pattern order -- a function of the
// histogram alone, which is why a row's lse bits know nothing of the other rows.  The same histogram gives the threshold: the
// pattern at which the count from the top reaches K.  total = (s - lse) + score is monotone in s but not strictly (distinct s can
// round to one total), so the threshold is the TOTAL of that pattern, the patterns that share it are found by bisection, and the
// second pass over the row keeps every entry whose total is above it.  Entries that tie with it are kept too when they all fit;
// when they do not, the merge workgroup takes them in index order.  The merge ranks the B lists by (total descending, flat index
// ascending), so neither the order of the atomics nor the launch geometry shows in the output.
#include "common.h"
#include "beam_plan.h"
#include "unigen_hip.h"
#include <limits.h>

namespace {

using namespace ug_plan;

constexpr int BM_W = BEAM_SELECT_THREADS / 64;
constexpr int BM_BPT = BEAM_BINS / BEAM_SELECT_THREADS;   // histogram bins per thread of the select launch
constexpr int BM_P_LO = 0x80;              // positions (65535 - key) of the finite bf16 values, both ends included:
constexpr int BM_P_HI = 0xff7f;            // +inf sits at 0x7f, -inf at 0xff80, NaN patterns outside and never counted
constexpr float BM_DEAD = -1e8f;           // a running score at or below it is a dead beam

// bf16 pattern -> 16-bit key whose unsigned order is the order of the values (-0 and +0 share a key); text_sampler.hip's
__device__ __forceinline__ uint32_t bm_key(bf16_t b) {
  uint32_t k = b;
  if (k == 0x8000u) k = 0u;
  return (k ^ ((k >> 15) ? 0xffffu : 0x8000u)) & 0xffffu;
}
__device__ __forceinline__ float bm_value_at(int p) {
  const uint32_t k = 65535u - (uint32_t)p;
  return bf2f((bf16_t)(k ^ ((k >> 15) ? 0x8000u : 0xffffu)));
}
// the candidate's total, in exactly this order, never contracted: every launch forms the same fp32 number
__device__ __forceinline__ float bm_total(float s, float lse, float score) { return __fadd_rn(__fsub_rn(s, lse), score); }

// ------------------------------------------------------------------ launch 1: per-row histogram of the bf16 patterns
__global__ __launch_bounds__(BEAM_SEG_THREADS) void beam_count_kernel(const float* __restrict__ logits, int64_t ld, int V, int* __restrict__ hist) {
  const int r = blockIdx.y;
  const float* row = logits + (int64_t)r * ld;
  int* h = hist + (int64_t)r * BEAM_BINS;
  const int e0 = blockIdx.x * BEAM_SEG, e1 = min(V, e0 + BEAM_SEG);
  for (int e = e0 + (int)threadIdx.x; e < e1; e += BEAM_SEG_THREADS) {
    const float f = row[e];
    if (f != f) continue;                                            // a NaN logit contributes nothing and is no candidate
    atomicAdd(&h[65535 - (int)bm_key(f2bf(f))], 1);                  // stored by position: descending value
  }
}

// block-wide reductions over BEAM_SELECT_THREADS threads in a fixed order (xor tree in the wave, then the waves in order);
// every thread gets the result.  `red` is BM_W slots of LDS.
template <typename T, typename F>
__device__ __forceinline__ T bm_block_reduce(T v, T* red, F op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = red[0];
#pragma unroll
  for (int i = 1; i < BM_W; ++i) t = op(t, red[i]);
  return t;
}

// the body sees this thread's bins one by one, in ascending position: `p` the position, `c` its count
#define BM_FOR_BINS(...)                                   \
  for (int i4__ = 0; i4__ < BM_BPT / 4; ++i4__) {          \
    const int4 q__ = h4[i4__];                             \
    const int cs__[4] = {q__.x, q__.y, q__.z, q__.w};      \
    _Pragma("unroll") for (int u__ = 0; u__ < 4; ++u__) {  \
      const int p = p0 + 4 * i4__ + u__, c = cs__[u__];    \
      __VA_ARGS__                                          \
    }                                                      \
  }

// ------------------------------------------------------------------ launch 2: one workgroup per row on its histogram
// Thread t walks positions [BM_BPT t, BM_BPT t + BM_BPT), re-read from L2 by each pass (256 KiB per row).
// meta[r]: lse bits | threshold total bits | flags (1: ties by index, 2: no candidates) | ties wanted | entries above the threshold.
__global__ __launch_bounds__(BEAM_SELECT_THREADS) void beam_select_kernel(const int* __restrict__ hist, const float* __restrict__ beam_scores,
                                                                         int K, int* __restrict__ meta, float* __restrict__ lse_out) {
  __shared__ int red_i[BM_W];
  __shared__ double red_d[BM_W];
  __shared__ int s_pt;
  const int r = blockIdx.x, t = threadIdx.x, p0 = t * BM_BPT;
  const int4* h4 = reinterpret_cast<const int4*>(hist + (int64_t)r * BEAM_BINS) + t * (BM_BPT / 4);
  if (t == 0) s_pt = -1;
  const auto imin = [](int a, int b) { return min(a, b); };
  const auto imax = [](int a, int b) { return max(a, b); };
  const auto iadd = [](int a, int b) { return a + b; };
  const auto dadd = [](double a, double b) { return a + b; };

  // the maximum (infinities included), the last finite position that holds anything, the finite entries of this thread
  int first_p = INT_MAX, last_fin = -1, cnt = 0;
  BM_FOR_BINS({
    if (c > 0 && first_p == INT_MAX) first_p = p;
    if (p >= BM_P_LO && p <= BM_P_HI && c > 0) { last_fin = p; cnt += c; }
  });
  first_p = bm_block_reduce(first_p, red_i, imin);
  last_fin = bm_block_reduce(last_fin, red_i, imax);

  // lse: count * exp(value - m) per pattern in fp64, patterns in descending order within the thread
  float lse = -INFINITY;
  const bool has_max = first_p >= BM_P_LO && first_p <= BM_P_HI;      // a finite maximum
  if (first_p < BM_P_LO) lse = INFINITY;                               // a +inf entry: the row's log-softmax is -inf or NaN everywhere
  if (has_max) {
    const float m = bm_value_at(first_p);
    double sum = 0.0;
    BM_FOR_BINS({
      if (c > 0 && p <= BM_P_HI) sum += (double)c * (double)expf(__fsub_rn(bm_value_at(p), m));
    });
    sum = bm_block_reduce(sum, red_d, dadd);
    lse = (float)((double)m + log(sum));
  }

  // the position at which the count from the top reaches K
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(incl, o, 64);
    if ((t & 63) >= o) incl += n;
  }
  __syncthreads();
  if ((t & 63) == 63) red_i[t >> 6] = incl;
  __syncthreads();
  int base = 0, total_cnt = 0;
#pragma unroll
  for (int w = 0; w < BM_W; ++w) {
    if (w < (t >> 6)) base += red_i[w];
    total_cnt += red_i[w];
  }
  const int pre = base + incl - cnt;
  if (pre < K && K <= pre + cnt) {
    int run = pre, found = -1;
    BM_FOR_BINS({
      if (p >= BM_P_LO && p <= BM_P_HI) run += c;
      if (found < 0 && run >= K) found = p;
    });
    s_pt = found;
  }
  __syncthreads();
  const int pt = total_cnt < K ? last_fin : s_pt;
  const float score = beam_scores[r];
  const bool none = !has_max || pt < 0 || !(score > BM_DEAD);

  // the band of positions whose total equals the threshold's: totals fall (weakly) with the position
  float thr = INFINITY;
  int pu = pt, pl = pt;
  if (!none) {
    thr = bm_total(bm_value_at(pt), lse, score);
    int lo = BM_P_LO, hi = pt;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bm_total(bm_value_at(mid), lse, score) == thr) hi = mid; else lo = mid + 1;
    }
    pu = lo;
    lo = pt; hi = BM_P_HI;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (bm_total(bm_value_at(mid), lse, score) == thr) lo = mid; else hi = mid - 1;
    }
    pl = lo;
  }
  int n_gt = 0, n_eq = 0;
  if (!none) {
    BM_FOR_BINS({
      if (p >= BM_P_LO && p < pu) n_gt += c;
      if (p >= pu && p <= pl) n_eq += c;
    });
  }
  n_gt = bm_block_reduce(n_gt, red_i, iadd);
  n_eq = bm_block_reduce(n_eq, red_i, iadd);
  if (t == 0) {
    // n_gt < K: every entry above the threshold's total lies above the threshold's pattern, and fewer than K do
    const bool bad = none || n_gt >= K;
    const int want = bad ? 0 : min(K - n_gt, n_eq);
    int* mr = meta + r * BEAM_META_INTS;
    mr[0] = __float_as_int(lse);
    mr[1] = __float_as_int(thr);
    mr[2] = bad ? 2 : (n_eq > want ? 1 : 0);
    mr[3] = want;
    mr[4] = bad ? 0 : n_gt;
    if (lse_out) lse_out[r] = lse;
  }
}

#undef BM_FOR_BINS

// ------------------------------------------------------------------ launch 3: the entries above the threshold into the row's list
__global__ __launch_bounds__(BEAM_SEG_THREADS) void beam_collect_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                                       const float* __restrict__ beam_scores, const int* __restrict__ meta,
                                                                       int* __restrict__ count, float* __restrict__ list_total,
                                                                       int* __restrict__ list_token) {
  const int r = blockIdx.y;
  const int* mr = meta + r * BEAM_META_INTS;
  const int flags = mr[2];
  if (flags & 2) return;
  const float lse = __int_as_float(mr[0]), thr = __int_as_float(mr[1]), score = beam_scores[r];
  const bool ties_here = !(flags & 1);
  const float* row = logits + (int64_t)r * ld;
  const int e0 = blockIdx.x * BEAM_SEG, e1 = min(V, e0 + BEAM_SEG);
  for (int e = e0 + (int)threadIdx.x; e < e1; e += BEAM_SEG_THREADS) {
    const float f = row[e];
    if (f != f) continue;
    const float s = bf2f(f2bf(f));
    if (fabsf(s) == INFINITY) continue;
    const float tot = bm_total(s, lse, score);
    if (tot > thr || (ties_here && tot == thr)) {
      const int slot = atomicAdd(&count[r], 1);
      if (slot < BEAM_MAX_K) {                                       // (the select launch counted: at most K fit the rule)
        list_total[r * BEAM_MAX_K + slot] = tot;
        list_token[r * BEAM_MAX_K + slot] = e;
      }
    }
  }
}

// ------------------------------------------------------------------ launch 4: one workgroup per group
// Thread j owns list slot j & 63 of beam j >> 6.  Rows whose ties did not all fit take them here, lowest index first: the row is
// walked in index order, 512 entries at a time, until the wanted number is found.
__global__ __launch_bounds__(BEAM_MERGE_THREADS) void beam_merge_kernel(const float* __restrict__ logits, int64_t ld, int B, int V, int K,
                                                                       const float* __restrict__ beam_scores, const int* __restrict__ meta,
                                                                       const int* __restrict__ count, const float* __restrict__ list_total,
                                                                       const int* __restrict__ list_token, float* __restrict__ cand_score,
                                                                       int* __restrict__ cand_beam, int* __restrict__ cand_token) {
  constexpr int NW = BEAM_MERGE_THREADS / 64;
  __shared__ float s_tot[BEAM_MERGE_THREADS];
  __shared__ int s_flat[BEAM_MERGE_THREADS];                          // b * V + e; -1: an empty slot
  __shared__ int s_cnt[BEAM_MAX_B];
  __shared__ int s_wc[NW];
  const int g = blockIdx.x, j = threadIdx.x, jb = j >> 6, ji = j & 63, lane = j & 63, wave = j >> 6;

  if (j < BEAM_MAX_B) {
    int n = 0;
    if (j < B) {
      const int r = g * B + j;
      const int* mr = meta + r * BEAM_META_INTS;
      n = (mr[2] & 2) ? 0 : ((mr[2] & 1) ? min(mr[4], BEAM_MAX_K) : min(count[r], BEAM_MAX_K));
    }
    s_cnt[j] = n;
  }
  __syncthreads();
  {
    const bool have = jb < B && ji < s_cnt[jb];
    const int r = g * B + jb;
    s_tot[j] = have ? list_total[r * BEAM_MAX_K + ji] : -INFINITY;
    s_flat[j] = have ? jb * V + list_token[r * BEAM_MAX_K + ji] : -1;
  }
  __syncthreads();

  for (int b = 0; b < B; ++b) {                                       // uniform: every thread walks the same rows and tiles
    const int r = g * B + b;
    const int* mr = meta + r * BEAM_META_INTS;
    if (!(mr[2] & 1)) continue;
    const float lse = __int_as_float(mr[0]), thr = __int_as_float(mr[1]), score = beam_scores[r];
    const int want = min(mr[3], BEAM_MAX_K - s_cnt[b]), at = s_cnt[b];
    const float* row = logits + (int64_t)r * ld;
    int taken = 0;
    for (int e0 = 0; e0 < V && taken < want; e0 += BEAM_MERGE_THREADS) {
      const int e = e0 + j;
      bool hit = false;
      if (e < V) {
        const float f = row[e];
        const float s = bf2f(f2bf(f));
        hit = f == f && fabsf(s) != INFINITY && bm_total(s, lse, score) == thr;
      }
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) s_wc[wave] = __popcll(bal);
      __syncthreads();
      int off = 0, tile = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < wave) off += s_wc[w];
        tile += s_wc[w];
      }
      off += __popcll(bal & ((1ull << lane) - 1ull));
      if (hit && taken + off < want) {
        s_tot[b * 64 + at + taken + off] = thr;
        s_flat[b * 64 + at + taken + off] = b * V + e;
      }
      taken += tile;
      __syncthreads();
    }
    __syncthreads();
    if (j == 0) s_cnt[b] = at + min(taken, want);
    __syncthreads();
  }

  int n_all = 0;
#pragma unroll
  for (int b = 0; b < BEAM_MAX_B; ++b) n_all += s_cnt[b];
  const float my = s_tot[j];
  const int mf = s_flat[j];
  if (mf >= 0) {
    int rank = 0;
    for (int q = 0; q < BEAM_MERGE_THREADS; ++q) {
      const float ot = s_tot[q];
      const int of = s_flat[q];
      rank += (of >= 0 && (ot > my || (ot == my && of < mf))) ? 1 : 0;
    }
    if (rank < K) {
      cand_score[g * K + rank] = my;
      cand_beam[g * K + rank] = mf / V;
      cand_token[g * K + rank] = mf % V;
    }
  }
  if (j >= n_all && j < K) {                                          // fewer than K candidates among the live beams
    cand_score[g * K + j] = -INFINITY;
    cand_beam[g * K + j] = -1;
    cand_token[g * K + j] = -1;
  }
}

// ------------------------------------------------------------------ KV reorder
// One lane, one 16-byte piece (beam_plan.h: plan_beam_kv).  GATHER: spare <- cache[parent[r]]; else cache[r] <- spare.  Rows that
// keep their own history (parent[r] == r) move nothing; a parent outside [0, R) is treated the same (nothing is read out of bounds).
template <bool GATHER>
__global__ __launch_bounds__(BEAM_KV_THREADS) void beam_kv_move_kernel(uint4* const* __restrict__ k_ptrs, uint4* const* __restrict__ v_ptrs,
                                                                      int R, int HKV, int Tmax, const int* __restrict__ parent,
                                                                      const int* __restrict__ len, int first, int span, int pieces,
                                                                      uint4* __restrict__ spare) {
  const int i = blockIdx.x * BEAM_KV_THREADS + threadIdx.x;
  if (i >= pieces) return;
  const int r = blockIdx.y, pr = parent[r];
  if (pr == r || pr < 0 || pr >= R) return;
  const int end = min(*len, first + span);
  const int h = i / (span * BEAM_KV_PIECES), tt = (i / BEAM_KV_PIECES) % span, p = i % BEAM_KV_PIECES, t = first + tt;
  if (t >= end) return;
  const int z = blockIdx.z;
  uint4* cache = (z & 1) ? v_ptrs[z >> 1] : k_ptrs[z >> 1];
  const int64_t si = ((((int64_t)z * R + r) * HKV + h) * span + tt) * BEAM_KV_PIECES + p;
  const int64_t src_row = GATHER ? pr : r;
  const int64_t ci = ((src_row * HKV + h) * Tmax + t) * BEAM_KV_PIECES + p;
  if (GATHER) spare[si] = cache[ci];
  else cache[ci] = spare[si];
}

int beam_cand_shape_ok(const char* who, int64_t G, int64_t B, int64_t V, int64_t K) {
  UG_REQUIRE(beam_cand_in_limits(G, B, V, K),
             "%s: need 1 <= B <= %d, 1 <= G*B <= %d, 1 <= K <= %d and 1 <= V <= %d (G=%ld B=%ld V=%ld K=%ld)", who, BEAM_MAX_B, BEAM_MAX_ROWS,
             BEAM_MAX_K, BEAM_MAX_V, (long)G, (long)B, (long)V, (long)K);
  return UG_OK;
}

}  // namespace

extern "C" int ug_beam_candidates_ws_bytes(int64_t G, int64_t B, int64_t V, int64_t K) {
  const int rc = beam_cand_shape_ok("ug_beam_candidates_ws_bytes", G, B, V, K);
  if (rc != UG_OK) return rc;
  return (int)plan_beam_candidates(G, B, V, K).ws_bytes;
}

extern "C" int ug_beam_candidates(const float* logits, int64_t ld, int64_t G, int64_t B, int64_t V, const float* beam_scores, int64_t K,
                                  void* ws, float* cand_score, int* cand_beam, int* cand_token, float* lse, hipStream_t st) {
  const int rc = beam_cand_shape_ok("ug_beam_candidates", G, B, V, K);
  if (rc != UG_OK) return rc;
  UG_REQUIRE(ld >= V && ld <= (1ll << 31), "ug_beam_candidates: need V <= ld <= 2^31 (ld=%ld V=%ld)", (long)ld, (long)V);
  UG_REQUIRE(logits && beam_scores, "ug_beam_candidates: logits and beam_scores must not be null");
  UG_REQUIRE(ws && ug_aligned16(ws), "ug_beam_candidates: ws must not be null and 16B aligned (ug_beam_candidates_ws_bytes(G, B, V, K) bytes)");
  UG_REQUIRE(cand_score && cand_beam && cand_token, "ug_beam_candidates: cand_score, cand_beam and cand_token must not be null");
  const BeamCandPlan pl = plan_beam_candidates(G, B, V, K);
  char* w = reinterpret_cast<char*>(ws);
  int* hist = reinterpret_cast<int*>(w + pl.hist_off);
  int* count = reinterpret_cast<int*>(w + pl.count_off);
  int* meta = reinterpret_cast<int*>(w + pl.meta_off);
  float* list_total = reinterpret_cast<float*>(w + pl.list_total_off);
  int* list_token = reinterpret_cast<int*>(w + pl.list_token_off);
  UG_HIP(hipMemsetAsync(w, 0, (size_t)pl.zero_bytes, st));
  const dim3 seg_grid((unsigned)pl.segs, (unsigned)pl.rows);
  hipLaunchKernelGGL(beam_count_kernel, seg_grid, dim3(BEAM_SEG_THREADS), 0, st, logits, ld, (int)V, hist);
  UG_CHECK_LAUNCH("ug_beam_candidates(count)");
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)pl.select_grid), dim3(BEAM_SELECT_THREADS), 0, st, (const int*)hist, beam_scores, (int)K,
                     meta, lse);
  UG_CHECK_LAUNCH("ug_beam_candidates(select)");
  hipLaunchKernelGGL(beam_collect_kernel, seg_grid, dim3(BEAM_SEG_THREADS), 0, st, logits, ld, (int)V, beam_scores, (const int*)meta, count,
                     list_total, list_token);
  UG_CHECK_LAUNCH("ug_beam_candidates(collect)");
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)pl.merge_grid), dim3(BEAM_MERGE_THREADS), 0, st, logits, ld, (int)B, (int)V, (int)K,
                     beam_scores, (const int*)meta, (const int*)count, (const float*)list_total, (const int*)list_token, cand_score, cand_beam,
                     cand_token);
  UG_CHECK_LAUNCH("ug_beam_candidates(merge)");
  return UG_OK;
}

extern "C" int ug_beam_kv_reorder(const void* const* k_ptrs, const void* const* v_ptrs, int64_t n_layers, int64_t R, int64_t HKV,
                                  int64_t Tmax, int64_t hd, const int* parent, const int* len, int64_t first, void* spare, int64_t span,
                                  hipStream_t st) {
  UG_REQUIRE(hd == BEAM_KV_HD, "ug_beam_kv_reorder: head_dim must be %d (hd=%ld)", BEAM_KV_HD, (long)hd);
  const BeamKvPlan pl = plan_beam_kv(n_layers, R, HKV, Tmax, hd, first, span);
  UG_REQUIRE(pl.grid_x > 0,
             "ug_beam_kv_reorder: need 1 <= n_layers <= %d, 1 <= R <= %d, HKV >= 1, first >= 0, span >= 1 and first + span <= Tmax "
             "(n_layers=%ld R=%ld HKV=%ld Tmax=%ld first=%ld span=%ld)",
             BEAM_KV_MAX_LAYERS, BEAM_MAX_ROWS, (long)n_layers, (long)R, (long)HKV, (long)Tmax, (long)first, (long)span);
  UG_REQUIRE(k_ptrs && v_ptrs && parent && len, "ug_beam_kv_reorder: k_ptrs, v_ptrs, parent and len must not be null");
  UG_REQUIRE(spare && ug_aligned16(spare), "ug_beam_kv_reorder: spare must not be null and 16B aligned");
  const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z);
  uint4* const* kp = reinterpret_cast<uint4* const*>(const_cast<void* const*>(k_ptrs));
  uint4* const* vp = reinterpret_cast<uint4* const*>(const_cast<void* const*>(v_ptrs));
  hipLaunchKernelGGL(beam_kv_move_kernel<true>, grid, dim3(BEAM_KV_THREADS), 0, st, kp, vp, (int)R, (int)HKV, (int)Tmax, parent, len, (int)first,
                     (int)span, (int)pl.pieces, reinterpret_cast<uint4*>(spare));
  UG_CHECK_LAUNCH("ug_beam_kv_reorder(gather)");
  hipLaunchKernelGGL(beam_kv_move_kernel<false>, grid, dim3(BEAM_KV_THREADS), 0, st, kp, vp, (int)R, (int)HKV, (int)Tmax, parent, len, (int)first,
                     (int)span, (int)pl.pieces, reinterpret_cast<uint4*>(spare));
  UG_CHECK_LAUNCH("ug_beam_kv_reorder(write back)");
  return UG_OK;
}
