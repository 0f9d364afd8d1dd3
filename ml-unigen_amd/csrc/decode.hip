// Autoregressive decode support for UniGen.t2i_generate_ar (reference models/unigen.py:457-521, which
// drives transformers' DynamicCache + SDPA one token at a time).  Static KV cache sized for the whole
// generation, position / length read from DEVICE memory so one captured hipGraph replays all 256 steps.
//   cache layout: K,V [rows][HKV][Tmax][128] bf16 (keys of one (row, kv-head) contiguous)
#include "common.h"
#include "decode_common.h"
#include "decode_plan.h"
#include "unigen_hip.h"
#include "vmem_asm.h"
#include <stdlib.h>

namespace {

constexpr int DHD = 128;
typedef const __attribute__((address_space(1))) void* gptr_t;      // LDS-DMA operands (global_load_lds)
typedef __attribute__((address_space(3))) void* lptr_t;

// qkv rows (r*L + t) -> cache[r][hk][pos0 + t][:]   (k already rotated).  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void kv_store_kernel(const bf16_t* __restrict__ qkv, int64_t ldq, int k_col, int v_col,
                                                       bf16_t* __restrict__ ck, bf16_t* __restrict__ cv, int R, int L,
                                                       int HKV, int Tmax, const int* __restrict__ pos_dev, int pos_host) {
  const int pos0 = pos_dev ? *pos_dev : pos_host;
  const int64_t total = (int64_t)R * L * HKV * (DHD / 8);
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % (DHD / 8));
    const int hk = (int)((idx / (DHD / 8)) % HKV);
    const int64_t tok = idx / ((DHD / 8) * HKV);
    const int r = (int)(tok / L), t = (int)(tok % L);
    if (pos0 + t >= Tmax) continue;
    const bf16_t* src = qkv + tok * ldq + hk * DHD + c * 8;
    const int64_t dst = (((int64_t)r * HKV + hk) * Tmax + pos0 + t) * DHD + c * 8;
    *reinterpret_cast<bf16x8_t*>(ck + dst) = *reinterpret_cast<const bf16x8_t*>(src + k_col);
    *reinterpret_cast<bf16x8_t*>(cv + dst) = *reinterpret_cast<const bf16x8_t*>(src + v_col);
  }
}

// RoPE for single-token rows at position *pos_dev (rope_pair, common.h: the arithmetic of rope_kernel in elementwise.hip)
__global__ __launch_bounds__(256) void rope_at_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ cs,
                                                      const float* __restrict__ sn, int rows, int ldq, int nheads, int hd,
                                                      const int* __restrict__ pos_dev, int max_pos) {
  const int half = hd >> 1, per_head = half >> 2;
  const int pos = min(*pos_dev, max_pos - 1);
  const int total = rows * nheads * per_head;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int p4 = idx % per_head;
    const int h = (idx / per_head) % nheads;
    const int t = idx / (per_head * nheads);
    bf16_t* base = qkv + (int64_t)t * ldq + h * hd + p4 * 4;
    const uint2 lo = *reinterpret_cast<const uint2*>(base);
    const uint2 hi = *reinterpret_cast<const uint2*>(base + half);
    const float4 c = *reinterpret_cast<const float4*>(cs + (int64_t)pos * half + p4 * 4);
    const float4 s = *reinterpret_cast<const float4*>(sn + (int64_t)pos * half + p4 * 4);
    const float x1[4] = {bf2f(lo.x & 0xffff), bf2f(lo.x >> 16), bf2f(lo.y & 0xffff), bf2f(lo.y >> 16)};
    const float x2[4] = {bf2f(hi.x & 0xffff), bf2f(hi.x >> 16), bf2f(hi.y & 0xffff), bf2f(hi.y >> 16)};
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
    float o1[4], o2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rope_pair(x1[k], x2[k], cc[k], ss[k], o1[k], o2[k]);
    uint2 olo, ohi;
    olo.x = pack_bf2(o1[0], o1[1]); olo.y = pack_bf2(o1[2], o1[3]);
    ohi.x = pack_bf2(o2[0], o2[1]); ohi.y = pack_bf2(o2[2], o2[3]);
    *reinterpret_cast<uint2*>(base) = olo;
    *reinterpret_cast<uint2*>(base + half) = ohi;
  }
}

// ---- steps the three cache-attention kernels share (attn_decode_kernel, attn_decode_fused_kernel, attn_decode_seq_kernel): one
// definition each, so the kernels cannot drift apart (tests/test_attn_decode_seq_gpu.py, tests/test_decode_parity_gpu.py)
// A pass's score maximum mc joins the wave's running maximum m: returns the exponent offset mu of the pass (p = exp(s - mu); 0 while
// every key so far is masked) and sets alpha, the rescale of what l and O hold from earlier passes.
__device__ __forceinline__ float softmax_offset(float& m, float mc, float& alpha) {
  const float mn = fmaxf(m, mc);
  const float mu = (mn == -INFINITY) ? 0.f : mn;
  alpha = __expf(m - mu);
  m = mn;
  return mu;
}
// Online-softmax step with one key per lane: score s (-inf: no key) joins (m, l); returns this lane's p.
__device__ __forceinline__ float online_softmax_step(float s, float& m, float& l, float& alpha) {
  const float mu = softmax_offset(m, wave_max(s), alpha);
  const float p = __expf(s - mu);
  l = l * alpha + wave_sum(p);
  return p;
}
// Fold the four key phases (lane >> 4) of a wave's O and park its (m, l, O) partial in LDS (dc = lane & 15, the lane's 8-dim chunk).
template <int NW>
__device__ __forceinline__ void park_partial(float (&acc)[8], float m, float l, float (&om)[NW][DHD], float (&ml)[NW][2], int lane, int wave, int dc) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] += __shfl_xor(acc[e], 16, 64);
    acc[e] += __shfl_xor(acc[e], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int e = 0; e < 8; ++e) om[wave][dc * 8 + e] = acc[e];
  }
  if (lane == 0) { ml[wave][0] = m; ml[wave][1] = l; }
}
// Merge the NW parked partials into (L, O) of output dim d, relative to the overall maximum M (flash-decoding style split over keys).
template <int NW>
__device__ __forceinline__ void merge_partials(const float (&om)[NW][DHD], const float (&ml)[NW][2], float M, int d, float& L, float& O) {
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float wgt = (ml[w][0] == -INFINITY) ? 0.f : __expf(ml[w][0] - M);
    L += wgt * ml[w][1];
    O += wgt * om[w][d];
  }
}

// Consumer-side finishing of one rotate-half pair (a1, a2) of the raw q/k/v accumulator: x = bf16(rstd * acc + bias) with rstd from the
// row's sum of squares ssr over norm_cols columns, then (q and k heads: rope) rope_pair on the rounded values and one more bf16 rounding.
// attn_decode_fused_kernel and attn_decode_seq_kernel both call it: the cache rows they append must be the same bits.
__device__ __forceinline__ void qkv_finish_pair(float a1, float a2, float ssr, int norm_cols, float eps, bool has_bias, float b1, float b2,
                                                bool rope, float c, float s, float& x1, float& x2) {
#pragma clang fp contract(off)
  const float rs = rsqrtf(ssr / (float)norm_cols + eps);
  float v1 = rs * a1, v2 = rs * a2;
  if (has_bias) { v1 += b1; v2 += b2; }
  x1 = bf2f(f2bf(v1)); x2 = bf2f(f2bf(v2));
  if (rope) {
    float r1, r2;
    rope_pair(x1, x2, c, s, r1, r2);
    x1 = bf2f(f2bf(r1)); x2 = bf2f(f2bf(r2));
  }
}

// One workgroup (4 waves) per (row, query head).  Wave w takes key chunks w, w+4, ... of 64 keys: lane j scores
// key (t0 + j) against q (fp32 in LDS) and the wave keeps its own online-softmax state; for P.V the lanes regroup
// as (key phase = lane>>4, 8-dim chunk = lane&15) so every V read is a 16-byte load with 16 of them in flight.
// The four partial (m, l, O) states are merged through LDS (flash-decoding style split over keys).
// key_valid: optional [rows][Tmax] bytes (0 = padding key, never attended), like HF's 2-D attention_mask.
constexpr int AD_WAVES = 4;
__global__ __launch_bounds__(64 * AD_WAVES) void attn_decode_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ ck,
                                                          const bf16_t* __restrict__ cv, const uint8_t* __restrict__ key_valid,
                                                          bf16_t* __restrict__ o, int64_t ldo, int H, int HKV, int Tmax,
                                                          const int* __restrict__ len_dev, float scale) {
  __shared__ float qs[DHD];
  __shared__ float om[AD_WAVES][DHD];
  __shared__ float ml[AD_WAVES][2];
  const int r = blockIdx.y, h = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hk = h / (H / HKV);
  const int len = min(*len_dev, Tmax);
  const bf16_t* qp = q + (int64_t)r * ldq + h * DHD;
  if (threadIdx.x < DHD) qs[threadIdx.x] = bf2f(qp[threadIdx.x]);
  __syncthreads();
  const bf16_t* kb = ck + ((int64_t)r * HKV + hk) * Tmax * DHD;
  const bf16_t* vb = cv + ((int64_t)r * HKV + hk) * Tmax * DHD;
  const int kq = lane >> 4, dc = lane & 15;
  float m = -INFINITY, l = 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int t0 = wave * 64; t0 < len; t0 += 64 * AD_WAVES) {
    const int t = t0 + lane;
    float s = -INFINITY;
    // K row of this lane's key and the V pieces of its (key phase, dim chunk) all go out before any is consumed
    bf16x8_t kf[DHD / 8], vf[16];
    {
      const bf16_t* kr = kb + (int64_t)min(t, len - 1) * DHD;
#pragma unroll
      for (int c = 0; c < DHD / 8; ++c) kf[c] = *reinterpret_cast<const bf16x8_t*>(kr + c * 8);
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int tt = min(t0 + jj * 4 + kq, len - 1);
        vf[jj] = *reinterpret_cast<const bf16x8_t*>(vb + (int64_t)tt * DHD + dc * 8);
      }
    }
    if (t < len && (!key_valid || key_valid[(int64_t)r * Tmax + t])) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < DHD / 8; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += bf2f((bf16_t)kf[c][e]) * qs[c * 8 + e];
      s = d * scale;
    }
    float alpha;
    const float p = online_softmax_step(s, m, l, alpha);
    const float pb = bf2f(f2bf(p));          // P is rounded to bf16 before P.V like the bf16 SDPA paths
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const float pj = __shfl(pb, jj * 4 + kq, 64);   // 0 for keys past len / masked keys
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pj * bf2f((bf16_t)vf[jj][e]);
    }
  }
  park_partial(acc, m, l, om, ml, lane, wave, dc);
  __syncthreads();
  if (threadIdx.x < DHD) {
    float M = ml[0][0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) M = fmaxf(M, ml[w][0]);
    float L = 0.f, O = 0.f;
    merge_partials(om, ml, M, threadIdx.x, L, O);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    o[(int64_t)r * ldo + h * DHD + threadIdx.x] = f2bf(O * inv);
  }
}

typedef __bf16 bf16pair_t __attribute__((ext_vector_type(2)));
constexpr int ADF_WAVES = 8;            // one 64-key chunk per wave up to 512 keys: no serialized second chunk
// Cache attention of one decode step fed by the RAW qkv accumulator: every (row, query head) workgroup rebuilds
// q and its kv head's new k / v row itself (no dependency between workgroups; the first query head of each kv head
// also appends the row to the cache), attends to cache keys [0, pos) exactly like attn_decode_kernel, and merges
// the new token as one more (m, l, O) partial.
// (Argument order: the first 14 dwords are what the kernel's first loads need -- with -mllvm -amdgpu-kernarg-preload-count=16 hipcc preloads
// that many, they arrive in SGPRs with the wave; the rest comes by one batch of scalar loads.)
// NQP > 0: the ORDERED form (deterministic decode, ug_attn_decode_fused_ord): acc_qkv holds NQP k-slab partial slots [NQP][R][lda] and
// ss NQP slots of 32 row sums of squares; the prologue requests all of them with its first loads and sums them in ascending slab order.
template <int NQP = 0>
__global__ __launch_bounds__(64 * ADF_WAVES) void attn_decode_fused_kernel(
    const float* __restrict__ acc_qkv, const float* __restrict__ ss, const int* __restrict__ pos_dev, bf16_t* __restrict__ ck,
    bf16_t* __restrict__ cv, int R, int HKV, int H, int lda, int Tmax, int max_pos,
    const bf16_t* __restrict__ bias, const float* __restrict__ cs, const float* __restrict__ sn, const uint8_t* __restrict__ key_valid,
    bf16_t* __restrict__ o, int64_t ldo, float eps, int norm_cols, float scale) {
  __shared__ float qs[DHD], kn[DHD], vn[DHD];
  __shared__ __attribute__((aligned(16))) bf16_t qb[DHD];       // q again, as bf16 pairs (q IS bf16-rounded): the B operand of v_dot2c_f32_bf16
  __shared__ float om[ADF_WAVES][DHD];
  __shared__ float ml[ADF_WAVES][2];
  // K rows of a wave's 64-key chunk: 16 KB, CONTIGUOUS in the cache ([row][kv head][t][128]).  Round 3 let lane j load "its" key
  // row piece by piece (16 loads of 16 B at a 256-byte lane stride): every instruction touched 64 cache lines and the 256 KB a
  // workgroup walks do not stay in the CU's 32 KB L1, so each line came up from L2 up to eight times -- 5.3 of the kernel's
  // 10.7 us (ablation, profiles/r04_ar_decode.md).  Now the chunk goes HBM/L2 -> LDS by LDS-DMA, 1 KB of contiguous source per
  // instruction, and lane j reads its row back from LDS.  LDS-DMA writes lane-linear, so the bank swizzle is applied on the
  // SOURCE side: LDS slot s of key k holds 16-byte chunk s ^ (k & 15); the 16 lanes of a ds_read_b128 service group hold 16
  // different k & 15, so the reads are conflict-free.
  __shared__ __attribute__((aligned(1024))) char ktile[ADF_WAVES][64 * DHD * 2];
  // Workgroup -> (row, query head): the H / HKV query heads that share one (row, kv head)'s K / V are placed on ONE XCD (workgroup
  // b runs on XCD b % 8 and every XCD has its own L2): dealt out head-major they landed on six different XCDs and each XCD
  // fetched the same K / V from HBM -- 36 MB per layer instead of 6, the part of this kernel that grew with the context
  // (8.2 us at 171 keys, 11.2 at 363).
  // Grid (8, H / HKV, ceil(R HKV / 8)): x = XCD, y = query head inside the kv group, z = block of eight groups -- the linear
  // workgroup id is what it was (8 (z per + y) + x), and no division is left ahead of the first load (round 5).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hq = blockIdx.y;
  const int grp = blockIdx.x + 8 * blockIdx.z;            // (row, kv head) group
  // Arguments in two batches (vmem_asm.h, argument hoisting): the early exit, the power-of-two test and the position load used to be three
  // DEPENDENT round trips to the kernarg segment ahead of the first vector load.  Batch 1 = the kernel's first 14 argument dwords --
  // everything the accumulator loads (the ~2 us chain) need -- which arrive in SGPRs with the wave when the
  // code object is built with kernarg preload; batch 2 is requested behind the accumulator loads.
  asm volatile("" ::"s"(acc_qkv), "s"(ss), "s"(pos_dev), "s"(ck), "s"(cv), "s"(R), "s"(HKV), "s"(H), "s"(lda));
  if (grp >= R * HKV) return;
  int r, hk, per;
  if ((HKV & (HKV - 1)) == 0) { const int sh = 31 - __builtin_clz(HKV); r = grp >> sh; hk = grp & (HKV - 1); per = H >> sh; }
  else { r = grp / HKV; hk = grp - r * HKV; per = H / HKV; }          // (= gridDim.y, but that is an implicit ARGUMENT: one more scalar load)
  const int h = hk * per + hq;
  const int kq = lane >> 4, dc = lane & 15;
  const bf16_t *kb, *vb;                                   // this (row, kv head)'s cache rows: set behind the second argument batch
  // the first key chunk's K rows / V pieces do not depend on the new token: request them before the prologue's own
  // round trip (accumulator, bias, RoPE table) so the two latencies overlap.  (Requesting them before the position word
  // as well -- clamped to the cache instead of the visible length, masked afterwards -- measured SLOWER, 5 730 vs 5 885
  // tokens/s: every wave then loads a chunk at every step, visible or not.)
  // Every load of this kernel is hand-issued (vmem_asm.h): with the builtins the prologue's LDS writes were preceded by a compiler-inserted
  // s_waitcnt vmcnt(0), i.e. the new token's q / k / v were built only after the wave's whole K / V chunk had landed.
  bf16x8_t vf[16];
  const uint32_t kt_lds = __builtin_amdgcn_readfirstlane(lds_addr_of(ktile[wave]));
  auto load_chunk = [&](int t0, int last) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = i * 4 + kq;                                    // key of the chunk this lane's 16 bytes belong to
      const bf16_t* src = kb + (int64_t)min(t0 + k, last) * DHD + ((dc ^ (k & 15)) << 3);
      dma16(src, kt_lds + i * 1024);
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int tt = min(t0 + jj * 4 + kq, last);
      ld16(vf[jj], vb + (int64_t)tt * DHD + dc * 8);
    }
  };
  int pos0;
  sld4(pos0, pos_dev);                                     // (hand-issued scalar load: vmem_asm.h)
  // The new token's q / k / v pair of this lane (waves 0-2): its loads -- the raw accumulator the projection's atomics left at
  // the device coherence point, bias, RoPE table: one ~2 us round trip -- go out FIRST, the chunk's K / V requests behind them.
  const float* arow = acc_qkv + (int64_t)r * lda;
  const int col0 = wave == 0 ? h * DHD : wave == 1 ? (H + hk) * DHD : (H + HKV + hk) * DHD;
  float a1 = 0.f, a2 = 0.f, rc = 1.f, rsn = 0.f, ssr = 1.f;
  uint32_t bb1 = 0, bb2 = 0;
  if (wave < 3) {
    ld4(ssr, ss + r);
    ld4(a1, arow + col0 + lane); ld4(a2, arow + col0 + lane + DHD / 2);
  }
  float pss[NQP > 1 ? NQP - 1 : 1], pa1[NQP > 1 ? NQP - 1 : 1], pa2[NQP > 1 ? NQP - 1 : 1];     // ordered: slots 1 .. NQP - 1
  if constexpr (NQP > 1) {
    if (wave < 3) {
#pragma unroll
      for (int p = 1; p < NQP; ++p) {
        const float* prow = arow + (int64_t)p * R * lda;
        ld4(pss[p - 1], ss + p * 32 + r);
        ld4(pa1[p - 1], prow + col0 + lane); ld4(pa2[p - 1], prow + col0 + lane + DHD / 2);
      }
    }
  }
  asm volatile("" ::"s"(Tmax), "s"(max_pos), "s"(bias), "s"(cs), "s"(sn), "s"(key_valid), "s"(o), "s"(ldo), "s"(__float_as_int(eps)),
               "s"(norm_cols), "s"(__float_as_int(scale)));  // batch 2
  wait_lgkm0();                                            // (the position word; the batch above is behind the same counter)
  tie_s(pos0);
  kb = ck + ((int64_t)r * HKV + hk) * Tmax * DHD;
  vb = cv + ((int64_t)r * HKV + hk) * Tmax * DHD;
  const int len = min(pos0, Tmax);                         // cache keys visible to the new token
  const int rpos = min(pos0, max_pos - 1);
  if (wave < 3) {
    if (bias) { ld2u(bb1, bias + col0 + lane); ld2u(bb2, bias + col0 + lane + DHD / 2); }
    if (wave < 2) { ld4(rc, cs + (int64_t)rpos * (DHD / 2) + lane); ld4(rsn, sn + (int64_t)rpos * (DHD / 2) + lane); }
  }
  const bool has_chunk = wave * 64 < len;
  if (has_chunk) load_chunk(wave * 64, len - 1);
  if (wave < 3) {
    if (has_chunk) wait_vm<32>(); else wait_vm<0>();       // the prologue's loads are older than the chunk's 16 + 16
    tie(ssr); tie(a1); tie(a2); tie(bb1); tie(bb2); tie(rc); tie(rsn);
    if constexpr (NQP > 1) {
#pragma unroll
      for (int p = 0; p < NQP - 1; ++p) {                  // ascending slab order, fp32
        tie(pss[p]); tie(pa1[p]); tie(pa2[p]);
        ssr += pss[p]; a1 += pa1[p]; a2 += pa2[p];
      }
    }
    const float b1 = bf2f((bf16_t)bb1), b2 = bf2f((bf16_t)bb2);
    float x1, x2;
    qkv_finish_pair(a1, a2, ssr, norm_cols, eps, bias != nullptr, b1, b2, wave < 2, rc, rsn, x1, x2);
    float* dst = wave == 0 ? qs : wave == 1 ? kn : vn;
    dst[lane] = x1; dst[lane + DHD / 2] = x2;
    if (wave == 0) { qb[lane] = f2bf(x1); qb[lane + DHD / 2] = f2bf(x2); }
    if (wave > 0 && hq == 0 && pos0 < Tmax) {
      bf16_t* row = (wave == 1 ? ck : cv) + (((int64_t)r * HKV + hk) * Tmax + pos0) * DHD;
      row[lane] = f2bf(x1); row[lane + DHD / 2] = f2bf(x2);
    }
  }
  lds_barrier();                                           // (LDS hand-off only: __syncthreads() would also drain the chunk's loads)
  float m = -INFINITY, l = 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll 1
  for (int t0 = wave * 64; t0 < len; t0 += 64 * ADF_WAVES) {
    const int t = t0 + lane;
    float s = -INFINITY;
    if (t0 != wave * 64) {                               // later chunks (contexts beyond 512 keys): the wave's own reads of the
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); //  previous chunk have returned before the DMA overwrites the tile
      load_chunk(t0, len - 1);
    }
    wait_vm<0>();                                        // the chunk's K rows have landed in LDS (this wave's own DMA), its V pieces in vf
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) tie(vf[jj]);
    if (t < len && (!key_valid || key_valid[(int64_t)r * Tmax + t])) {
      // 64 v_dot2c_f32_bf16 (two bf16 products + fp32 add each) instead of 128 conversions + 128 fmas: K pairs straight from the
      // tile, q pairs from its bf16 image (broadcast reads: hoisting all 64 pairs would not fit 8 waves' registers)
      float d = 0.f;
      const char* krow = ktile[wave] + lane * (DHD * 2);
#pragma unroll
      for (int c = 0; c < DHD / 8; ++c) {
        const uint4 kf = *reinterpret_cast<const uint4*>(krow + ((c ^ (lane & 15)) << 4));
        const uint4 qq = *reinterpret_cast<const uint4*>(&qb[c * 8]);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, kf.x), __builtin_bit_cast(bf16pair_t, qq.x), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, kf.y), __builtin_bit_cast(bf16pair_t, qq.y), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, kf.z), __builtin_bit_cast(bf16pair_t, qq.z), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, kf.w), __builtin_bit_cast(bf16pair_t, qq.w), d, false);
      }
      s = d * scale;
    }
    float alpha;
    const float p = online_softmax_step(s, m, l, alpha);
    const float pb = bf2f(f2bf(p));
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
    // P.V two keys at a time: the two keys' values of a dim pair are interleaved by v_perm_b32 into (v[j][d], v[j+1][d]) and meet
    // the probability pair (p_j, p_j+1; both bf16-exact) in one v_dot2c_f32_bf16 -- 8 perm + 8 dot2 per key pair instead of 16
    // conversions + 16 fmas
#pragma unroll
    for (int jj = 0; jj < 16; jj += 2) {
      const uint32_t pp = pack_bf2(__shfl(pb, jj * 4 + kq, 64), __shfl(pb, (jj + 1) * 4 + kq, 64));
      const uint4 va = __builtin_bit_cast(uint4, vf[jj]), vb = __builtin_bit_cast(uint4, vf[jj + 1]);
      const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t lo = __builtin_amdgcn_perm(wb[i], wa[i], 0x05040100u);      // (a.lo16, b.lo16): dim 2 i of keys j, j + 1
        const uint32_t hi = __builtin_amdgcn_perm(wb[i], wa[i], 0x07060302u);      // (a.hi16, b.hi16): dim 2 i + 1
        acc[2 * i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, lo), __builtin_bit_cast(bf16pair_t, pp), acc[2 * i], false);
        acc[2 * i + 1] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair_t, hi), __builtin_bit_cast(bf16pair_t, pp), acc[2 * i + 1], false);
      }
    }
  }
  park_partial(acc, m, l, om, ml, lane, wave, dc);
  // the new token's own score (every wave computes it; no extra barrier)
  const float s_new = wave_sum(qs[lane] * kn[lane] + qs[lane + DHD / 2] * kn[lane + DHD / 2]) * scale;
  __syncthreads();
  if (threadIdx.x < DHD) {
    float M = s_new;
#pragma unroll
    for (int w = 0; w < ADF_WAVES; ++w) M = fmaxf(M, ml[w][0]);
    const float wn = __expf(s_new - M);
    float L = wn, O = wn * vn[threadIdx.x];
    merge_partials(om, ml, M, threadIdx.x, L, O);
    o[(int64_t)r * ldo + h * DHD + threadIdx.x] = f2bf(O / L);
  }
}

// Cache attention of one VERIFY step of speculative decoding (ug_attn_decode_seq): the S rows of the raw qkv accumulator are S
// CONSECUTIVE positions p, p + 1, ... of ONE sequence (one cache row), where attn_decode_fused_kernel's rows are independent sequences at
// one position.  One workgroup per (row s, query head): it finishes q of row s and k / v of rows 0 .. s of its kv head from the
// accumulator itself, by qkv_finish_pair like attn_decode_fused_kernel (the appended rows are the bits S one-row launches of that kernel
// append), so no new key or value is ever read back from the cache -- another workgroup writes it and nothing orders the two.  The first
// query head of a kv head appends ITS row's k / v at p + s.  Row s attends to the cache keys [0, min(p, Tmax)) that key_valid allows and
// to the new keys 0 .. s; what the workgroup of row s computes does not depend on S or on rows > s.
// Cache keys, 64 per wave and pass: lane (kq = lane >> 4, dc = lane & 15) loads the 16-byte piece dc of the keys 4 jj + kq -- every
// load instruction covers four whole 256-byte rows, contiguous in the cache -- for K and V alike; a score is the 16-lane sum of the
// pieces' partial dot products, after which every lane of the group holds the probability its V pieces need.  Plain loads and stores, no
// atomics, 9.6 KB of LDS (no K tile: the 128 KB of the fused kernel would leave one workgroup per CU for S x H of them).
constexpr int ADS_WAVES = 4;
constexpr int ADS_MAX_ROWS = UG_SPEC_MAX_ROWS;
__global__ __launch_bounds__(64 * ADS_WAVES) void attn_decode_seq_kernel(
    const float* __restrict__ acc_qkv, const float* __restrict__ ss, const int* __restrict__ pos_dev, bf16_t* __restrict__ ck,
    bf16_t* __restrict__ cv, int HKV, int H, int lda, int Tmax, int max_pos, const bf16_t* __restrict__ bias,
    const float* __restrict__ cs, const float* __restrict__ sn, const uint8_t* __restrict__ key_valid, bf16_t* __restrict__ o, int64_t ldo,
    float eps, int norm_cols, float scale) {
  __shared__ float qs[DHD];
  __shared__ float kn[ADS_MAX_ROWS][DHD], vn[ADS_MAX_ROWS][DHD];
  __shared__ float om[ADS_WAVES][DHD];
  __shared__ float ml[ADS_WAVES][2];
  __shared__ float sc[ADS_MAX_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x, s = blockIdx.y;
  const int per = H / HKV;
  const int hk = h / per, hq = h - hk * per;
  const int pos0 = max(*pos_dev, 0);
  // task 0: q of row s; tasks 1 + 2 j, 2 + 2 j: k, v of row j <= s.  A wave per task, lane l builds the rotate-half pair (l, l + 64).
  for (int task = wave; task < 3 + 2 * s; task += ADS_WAVES) {
    const int j = task == 0 ? s : (task - 1) >> 1;
    const int kind = task == 0 ? 0 : 1 + ((task - 1) & 1);          // 0 q, 1 k, 2 v
    const int col0 = kind == 0 ? h * DHD : kind == 1 ? (H + hk) * DHD : (H + HKV + hk) * DHD;
    const float* arow = acc_qkv + (int64_t)j * lda;
    const float ssr = ss[j];
    const float a1 = arow[col0 + lane], a2 = arow[col0 + lane + DHD / 2];
    const int rpos = min(pos0 + j, max_pos - 1);
    float b1 = 0.f, b2 = 0.f, rc = 1.f, rsn = 0.f;
    if (bias) { b1 = bf2f(bias[col0 + lane]); b2 = bf2f(bias[col0 + lane + DHD / 2]); }
    if (kind < 2) { rc = cs[(int64_t)rpos * (DHD / 2) + lane]; rsn = sn[(int64_t)rpos * (DHD / 2) + lane]; }
    float x1, x2;
    qkv_finish_pair(a1, a2, ssr, norm_cols, eps, bias != nullptr, b1, b2, kind < 2, rc, rsn, x1, x2);
    float* dst = kind == 0 ? qs : kind == 1 ? kn[j] : vn[j];
    dst[lane] = x1; dst[lane + DHD / 2] = x2;
    if (kind > 0 && j == s && hq == 0 && pos0 + s < Tmax) {
      bf16_t* row = (kind == 1 ? ck : cv) + ((int64_t)hk * Tmax + pos0 + s) * DHD;
      row[lane] = f2bf(x1); row[lane + DHD / 2] = f2bf(x2);
    }
  }
  __syncthreads();
  const int len = min(pos0, Tmax);                          // cache keys visible to every row of the step
  const bf16_t* kb = ck + (int64_t)hk * Tmax * DHD;
  const bf16_t* vb = cv + (int64_t)hk * Tmax * DHD;
  const int kq = lane >> 4, dc = lane & 15;
  float qf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] = qs[dc * 8 + e];
  float m = -INFINITY, l = 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int t0 = wave * 64; t0 < len; t0 += 64 * ADS_WAVES) {
    bf16x8_t kf[16], vf[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int64_t tt = min(t0 + jj * 4 + kq, len - 1);    // (nothing at or past len is ever read)
      kf[jj] = *reinterpret_cast<const bf16x8_t*>(kb + tt * DHD + dc * 8);
      vf[jj] = *reinterpret_cast<const bf16x8_t*>(vb + tt * DHD + dc * 8);
    }
    float sj[16];
    float mc = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d += bf2f((bf16_t)kf[jj][e]) * qf[e];
      d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 8, 64);
      const int t = t0 + jj * 4 + kq;
      sj[jj] = (t < len && (!key_valid || key_valid[t])) ? d * scale : -INFINITY;
      mc = fmaxf(mc, sj[jj]);
    }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    float alpha;
    const float mu = softmax_offset(m, mc, alpha);
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const float p = __expf(sj[jj] - mu);                  // 0 for keys past len / masked keys
      ps += p;
      const float pb = bf2f(f2bf(p));                       // P is rounded to bf16 before P.V like the bf16 SDPA paths
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pb * bf2f((bf16_t)vf[jj][e]);
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
  }
  park_partial(acc, m, l, om, ml, lane, wave, dc);
  // the scores of the step's own keys 0 .. s (a wave each)
  for (int j = wave; j <= s; j += ADS_WAVES) {
    const float d = wave_sum(qs[lane] * kn[j][lane] + qs[lane + DHD / 2] * kn[j][lane + DHD / 2]) * scale;
    if (lane == 0) sc[j] = d;
  }
  __syncthreads();
  if (threadIdx.x < DHD) {
    float M = sc[0];
    for (int j = 1; j <= s; ++j) M = fmaxf(M, sc[j]);
#pragma unroll
    for (int w = 0; w < ADS_WAVES; ++w) M = fmaxf(M, ml[w][0]);
    float L = 0.f, O = 0.f;
    for (int j = 0; j <= s; ++j) {
      const float wn = __expf(sc[j] - M);
      L += wn;
      O += wn * vn[j][threadIdx.x];
    }
    merge_partials(om, ml, M, threadIdx.x, L, O);
    o[(int64_t)s * ldo + h * DHD + threadIdx.x] = f2bf(O / L);
  }
}

// Finish a split-K fp32 accumulation of a skinny GEMM: np partial slots parts[p * slot + ...] summed in ascending slot order in fp32 (the
// ordered forms of the deterministic decode; np == 1: the one accumulator of the default form, ug_skinny_finish), then
//   out_bf16 = bf16(sum + bias) | resid += bf16round(sum) (in place) | out_f32 = sum      (whichever is given)
__global__ __launch_bounds__(256) void skinny_finish_kernel(const float* __restrict__ parts, int np, int64_t slot,
                                                            const bf16_t* __restrict__ bias, bf16_t* __restrict__ out_bf16,
                                                            float* __restrict__ out_f32, float* __restrict__ resid, int64_t total, int N) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float v = parts[i];
    for (int p = 1; p < np; ++p) v += parts[p * slot + i];
    if (out_bf16) {
      if (bias) v += bf2f(bias[i % N]);
      out_bf16[i] = f2bf(v);
    } else if (resid) {
      resid[i] += bf2f(f2bf(v));
    } else {
      out_f32[i] = v;
    }
  }
}

// ------------------------------------------------------------------ weight-streaming GEMV for decode
// acc[r][n] += sum_k x[r][k] W[n][k]   for a handful of rows r (<= 16*RB) and a weight matrix read ONCE.
// HBM-bound and latency-sensitive (a whole projection is a few MB): the launch is cut into as many waves as
// it takes for (nearly) the whole matrix to be in flight at once.  One wave owns 16 weight rows x 32*U k,
// issues its U 16-byte non-temporal loads back to back, then feeds mfma_f32_16x16x32_bf16 with A = activation
// fragment (a few KiB, L2-resident) and B = weight fragment, so a lane ends up holding 4 rows x 1 column and
// every atomic instruction of a wave covers 4 rows x 64 contiguous bytes of a ROW-MAJOR accumulator.  The 4 waves of a workgroup
// take consecutive k-slices of the same 16 columns, reduce through LDS, then one fp32 atomic per output.
// acc is addressed acc[r*sr + n*sn]; the decode path uses row-major accumulators (sn = 1).
template <int RB, int U>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ x, int64_t ldx, int R,
                                                   const bf16_t* __restrict__ W, int64_t ldw, float* __restrict__ acc,
                                                   int64_t sr, int64_t sn, int N, int K) {
  __shared__ float red[3][64][4 * RB];
  // wave: through readfirstlane, so that `kbase + u * 32 < K` below is a scalar branch.  As a per-lane condition the compiler put the
  // second MFMA of gemv_kernel<1, 2> into an EXEC-masked region without a skip; an MFMA does not honour EXEC, and the waves past K
  // added a product of stale registers (K = 96: tests/test_gemv_exact_gpu.py, (2, 16369, 96)).
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrow = min(n0 + (lane & 15), N - 1);
  const int kbase = (blockIdx.y * 4 + wave) * (32 * U);
  const bf16_t* wp = W + (int64_t)nrow * ldw + g * 8 + kbase;
  f32x4_t d[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) d[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  bf16x8_t wf[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (kbase + u * 32 < K) wf[u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(wp + u * 32));
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const bf16_t* xp = x + (int64_t)min(rb * 16 + (lane & 15), R - 1) * ldx + g * 8 + kbase;
    bf16x8_t xf[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kbase + u * 32 < K) xf[u] = *reinterpret_cast<const bf16x8_t*>(xp + u * 32);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kbase + u * 32 < K) d[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[u], wf[u], d[rb], 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave - 1][lane][rb * 4 + j] = d[rb][j];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int n = n0 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rb * 16 + g * 4 + j;
        const float v = d[rb][j] + red[0][lane][rb * 4 + j] + red[1][lane][rb * 4 + j] + red[2][lane][rb * 4 + j];
        if (r < R && n < N) atomicAdd(acc + (int64_t)r * sr + (int64_t)n * sn, v);
      }
    }
  }
}

// Main form (K >= 256: every projection of the backbone and the lm-head slices).  Per-instruction coalescing
// decides the achieved HBM rate, and the MFMA operand layout (lane = weight row) only lets a direct load touch
// 64 bytes per row (measured 2.8 TB/s on gate_up).  So weight tiles go HBM -> LDS with 16-byte LDS-DMA, each
// instruction covering two rows x 512 contiguous bytes, and the fragments come back out of LDS.  LDS-DMA writes
// lane-linear, so the bank swizzle (16-byte chunk index ^ row) is applied to the SOURCE address.

// ------------------------------------------------------------------ fused finishers of the decode step
// Every finisher consumes a row-major fp32 accumulator filled by the GEMV (acc[r*lda + n]) and leaves it ZEROED
// for the next step, so the captured graph carries no memset nodes.

// o / down projection:  x[r] += bf16round(delta[r]);  xn[r] = bf16(rmsnorm(x[r]) * w)   (next sub-block's input).
// One wave per row.  The tail of both finishers below, once the row's x (v), norm weight (gw) and delta (dl) are in registers: the
// same per-lane accumulation order as rmsnorm_fwd_kernel so both paths agree bit for bit.
// ACC (finish_resid_norm_kernel): the delta came from the accumulator row `ar`, which is cleared as it is consumed, and xn is always
// written; !ACC (the ordered form): ar is not used and xn may be null.  (A compile-time distinction: a run-time one costs the
// accumulator form 52 / 100 instructions.)
template <int MAXV, bool ACC>
__device__ __forceinline__ void resid_norm_tail(float4 (&v)[MAXV], const float4 (&gw)[MAXV], const float4 (&dl)[MAXV], float4* xr, float4* ar,
                                                bf16_t* __restrict__ xn, int cols, float eps, int row, int lane) {
  const int nv = cols >> 2;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < MAXV; ++c) {
    const int i = lane + c * 64;
    if (i < nv) {
      if constexpr (ACC) ar[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      v[c].x += bf2f(f2bf(dl[c].x)); v[c].y += bf2f(f2bf(dl[c].y));
      v[c].z += bf2f(f2bf(dl[c].z)); v[c].w += bf2f(f2bf(dl[c].w));
      xr[i] = v[c];
      ss += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
    }
  }
  if (ACC || xn) {
    ss = wave_sum(ss);
    const float rs = rsqrtf(ss / (float)cols + eps);
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
      const int i = lane + c * 64;
      if (i < nv) {
        uint2 o;
        o.x = pack_bf2(gw[c].x * (v[c].x * rs), gw[c].y * (v[c].y * rs));
        o.y = pack_bf2(gw[c].z * (v[c].z * rs), gw[c].w * (v[c].w * rs));
        reinterpret_cast<uint2*>(xn + (int64_t)row * cols)[i] = o;
      }
    }
  }
}

// delta = the projection's accumulator acc[r * lda + n], left ZEROED
template <int MAXV>
__global__ __launch_bounds__(64) void finish_resid_norm_kernel(float* __restrict__ acc, int64_t lda, float* __restrict__ x,
                                                               const float* __restrict__ w, bf16_t* __restrict__ xn, int cols,
                                                               float eps, int* __restrict__ pos_inc, int* __restrict__ len_inc) {
  const int row = blockIdx.x, lane = threadIdx.x, nv = cols >> 2;
  float4* xr = reinterpret_cast<float4*>(x + (int64_t)row * cols);
  float4* ar = reinterpret_cast<float4*>(acc + (int64_t)row * lda);
  const float4* wr = reinterpret_cast<const float4*>(w);
  float4 v[MAXV], gw[MAXV], dl[MAXV];
#pragma unroll
  for (int c = 0; c < MAXV; ++c) {              // every load of the row in flight at once
    const int i = lane + c * 64;
    if (i < nv) { v[c] = xr[i]; gw[c] = wr[i]; dl[c] = ar[i]; }
  }
  resid_norm_tail<MAXV, true>(v, gw, dl, xr, ar, xn, cols, eps, row, lane);
  // the step's last launch that comes after every reader of the write position: advance it here (was two one-element torch
  // kernels per decode step)
  if (pos_inc && blockIdx.x == 0 && threadIdx.x == 0) { ++*pos_inc; ++*len_inc; }
}

// Ordered form (deterministic decode): delta = np partial slots parts[p][rows][ldp] (the last layer's down k-blocks) summed in ascending
// slot order in fp32; xn is written when given.
template <int MAXV>
__global__ __launch_bounds__(64) void finish_resid_norm_ord_kernel(const float* __restrict__ parts, int ldp, int np, float* __restrict__ x,
                                                                   const float* __restrict__ w, bf16_t* __restrict__ xn, int cols, float eps,
                                                                   int* __restrict__ pos_inc, int* __restrict__ len_inc) {
  const int row = blockIdx.x, lane = threadIdx.x, nv = cols >> 2;
  const int64_t slot = (int64_t)gridDim.x * ldp;
  float4* xr = reinterpret_cast<float4*>(x + (int64_t)row * cols);
  const float4* wr = reinterpret_cast<const float4*>(w);
  float4 v[MAXV], gw[MAXV], dl[MAXV];
#pragma unroll
  for (int c = 0; c < MAXV; ++c) {
    const int i = lane + c * 64;
    if (i < nv) { v[c] = xr[i]; gw[c] = wr[i]; dl[c] = reinterpret_cast<const float4*>(parts + (int64_t)row * ldp)[i]; }
  }
  for (int p = 1; p < np; ++p) {
    const float4* pr = reinterpret_cast<const float4*>(parts + p * slot + (int64_t)row * ldp);
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
      const int i = lane + c * 64;
      if (i < nv) { const float4 t = pr[i]; dl[c].x += t.x; dl[c].y += t.y; dl[c].z += t.z; dl[c].w += t.w; }
    }
  }
  resid_norm_tail<MAXV, false>(v, gw, dl, xr, nullptr, xn, cols, eps, row, lane);
  if (pos_inc && blockIdx.x == 0 && threadIdx.x == 0) { ++*pos_inc; ++*len_inc; }
}

// One wave per workgroup owns ONE 256-wide k-slab and KW consecutive 16-row weight groups.  The
// activation fragments of the slab are built once and stay in registers; the KW weight tiles walk through a
// two-slot LDS ring (tile t+2's DMA is issued as soon as tile t's fragments are in registers).  No workgroup
// barrier, no cross-wave reduction; ~10 independent waves per CU keep 16 KiB each in flight.
//
// Decode fusion.  A decode step is bound by the ~4 us floor of every launch, not by bytes, and on this multi-XCD
// part any in-kernel cross-wave hand-off costs several trips to the device coherence point (a completion-counter
// "last wave finishes" variant was measured SLOWER than separate finishing kernels).  So all finishing work moves
// to the CONSUMER side: a projection leaves its raw fp32 accumulator behind and the next kernel applies the
// finisher while building its own operand fragments; kernel boundaries are the only synchronisation.
//   XIN_BF16        operand = bf16 activations (o_proj after attention)
//   XIN_RESID_NORM  operand = bf16(w[k] * xnew[r][k]),  xnew = x_in + bf16round(pending accumulator)
//                   (residual add of the previous projection + the elementwise half of RMSNorm; the per-row
//                   rsqrt(mean(xnew^2)) factor is a scalar of the output row, so it is applied by the consumer of
//                   THIS projection's accumulator).  The waves of weight group 0 also write xnew to x_out and add
//                   their slab's sum of squares to ss_out[r].
//   XIN_SWIGLU      operand = bf16( bf16(silu(g)) * u ),  g, u = bf16(rstd[r] * gate/up accumulator)
// Every launch also clears up to two accumulators that earlier kernels have fully consumed and one 32-float
// statistics slot (spread over all waves), so the captured graph carries no memset nodes.
enum { XIN_BF16 = 0, XIN_RESID_NORM = 1, XIN_SWIGLU = 2 };

struct DecodeIn {
  const float* x_in; const float* pend; int64_t ld_pend; const float* norm_w; float* x_out; float* ss_out;   // RESID_NORM
  const float* gu; int64_t ld_gu; const float* ss_in; float eps; int norm_cols;                              // SWIGLU
  float* zero0; float* zero1; float* ss_zero;                                                               // clears
  int n0_4, per0, n1_4, per1;           // float4 counts and every workgroup's share of them (decode_clear, decode_common.h)
  int part_slot;                        // ordered forms: floats between two k-slabs' partial tiles (gemv_ring_kernel)
};

// linear workgroup id (x fastest: the order the dispatcher deals workgroups out to the XCDs in)
__device__ __forceinline__ int linear_block() { return (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// Request this lane's operand pieces (row `ar`, 8 k-values at k0) for the fp32-operand modes -- hand-issued loads (vmem_asm.h): the
// values may be used only behind the caller's wait + tie.
template <int XIN>
__device__ __forceinline__ void decode_operand_load(const float* p0, const float* p1, int ld1, const float* nw, int ar, int k0, int K,
                                                    f32x4_t (&a)[2], f32x4_t (&b)[2], f32x4_t (&w)[2]) {
  if constexpr (XIN == XIN_RESID_NORM) {          // p0 = x_in [.][K], p1 = pending accumulator [.][ld1], nw = norm weight
    const float* xp = p0 + (__umul24(ar, K) + k0);
    const float* pp = p1 + (__umul24(ar, ld1) + k0);
    ld16(a[0], xp); ld16(a[1], xp + 4);
    ld16(b[0], pp); ld16(b[1], pp + 4);
    ld16(w[0], nw + k0); ld16(w[1], nw + k0 + 4);
  } else {                                        // p0 = gate / up accumulator [.][ld1]
    const float* gp = p0 + (__umul24(ar, ld1) + k0);
    ld16(a[0], gp); ld16(a[1], gp + 4);
    ld16(b[0], gp + K); ld16(b[1], gp + K + 4);
  }
}

template <int XIN>
__device__ __forceinline__ bf16x8_t decode_operand_make(const DecodeIn& f, f32x4_t (&a)[2], const f32x4_t (&b)[2], const f32x4_t (&w)[2],
                                                        float rs, float& ssq) {
  const float av[8] = {a[0][0], a[0][1], a[0][2], a[0][3], a[1][0], a[1][1], a[1][2], a[1][3]};
  const float bv[8] = {b[0][0], b[0][1], b[0][2], b[0][3], b[1][0], b[1][1], b[1][2], b[1][3]};
  bf16x8_t o;
  if constexpr (XIN == XIN_RESID_NORM) {
    const float wv[8] = {w[0][0], w[0][1], w[0][2], w[0][3], w[1][0], w[1][1], w[1][2], w[1][3]};
    float xn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xn[e] = av[e] + bf2f(f2bf(bv[e]));
      o[e] = (short)f2bf(wv[e] * xn[e]);
      ssq += xn[e] * xn[e];
    }
    // the updated residual values stay in `a`: the workgroups of weight group 0 store them at the kernel's END (a store issued here
    // would sit between the weight tiles' loads in the memory queue)
    a[0] = f32x4_t{xn[0], xn[1], xn[2], xn[3]};
    a[1] = f32x4_t{xn[4], xn[5], xn[6], xn[7]};
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(silu_bf(bf2f(f2bf(rs * av[e]))) * bf2f(f2bf(rs * bv[e])));
  }
  return o;
}

// Addressing shared by the two ring kernels (round 5: 32-bit, 24-bit multiplies at full VALU rate; the host checks the ranges).
// A weight tile = 16 rows x 256 k of W [N][K] (row stride ldw elements); DMA instruction i of a tile covers rows 2i, 2i + 1 x 512
// bytes: lane -> row 2i + (lane >> 5), 16-byte chunk (lane & 31) ^ row (the bank swizzle, applied on the SOURCE side).
struct TileAddr {
  uint32_t lane_off[8];                          // BYTE offset of this lane inside a tile for DMA instruction i (row clamp aside)
  __device__ __forceinline__ void init(int lane, int kbase, int K, int ldw) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = 2 * i + (lane >> 5);
      lane_off[i] = (uint32_t)(__umul24(r, ldw) + min(kbase + ((lane & 31) ^ r) * 8, K - 8)) * 2u;       // chunks past K are never consumed
    }
  }
  // N % 16 != 0: the last group's missing rows re-read row N - 1 (their products are never stored)
  static __device__ __forceinline__ uint32_t ragged(int lane, int row0, int i, int kbase, int N, int K, int ldw) {
    const int r = 2 * i + (lane >> 5);
    return (uint32_t)(__umul24(min(row0 + r, N - 1), ldw) + min(kbase + ((lane & 31) ^ r) * 8, K - 8)) * 2u;
  }
};

// XIN_BF16: one wave per workgroup (see above).  Grid (k-slabs, groups of KW weight-row groups).
// ORD (deterministic decode): no clears, and the wave's partial tile is STORED into k-slab blockIdx.x's slot
// acc[blockIdx.x * f.part_slot + r * sr + n * sn] instead of added: one writer per slot element, the consumer sums the slots in order.
template <int RB, int KW, bool ORD = false>
__global__ __launch_bounds__(64) void gemv_ring_kernel(const bf16_t* __restrict__ x, int ldx, int R, const bf16_t* __restrict__ W,
                                                       int ldw, float* __restrict__ acc, int sr, int sn, int N, int K, DecodeIn f) {
  __shared__ __attribute__((aligned(1024))) char tile[2][8192];
  const int lane = threadIdx.x, g = lane >> 4, row = lane & 15;
  const int grp0 = blockIdx.y * KW;
  const int kbase = blockIdx.x * 256;
  const bool whole = (N & 15) == 0;                                 // every 16-row group is complete: no per-row clamp
  // the clears this launch carries go out first: stores behind the loads would sit between them in the memory queue
  if constexpr (!ORD) decode_clear(f, lane, linear_block(), blockDim.x);
  TileAddr ta;
  ta.init(lane, kbase, K, ldw);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(tile[0]));
  auto stage = [&](int t) {
    // nt: every weight byte is read once per step by one CU; leaving it out of the caches shortens issue -> landed (guide, row nt-weights)
    const uint32_t dst = lds0 + (t & 1) * 8192;
    if (whole) {
      const uint64_t base = (uint64_t)(W + (int64_t)min((grp0 + t) * 16, N - 16) * ldw);
#pragma unroll
      for (int i = 0; i < 8; ++i) dma16_nt(base, ta.lane_off[i], dst + i * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) dma16_nt((uint64_t)W, ta.ragged(lane, (grp0 + t) * 16, i, kbase, N, K, ldw), dst + i * 1024);
    }
  };
  // the activation fragments' loads go out AHEAD of the weight DMA (round 5, same-box A/B: +0.8 % tokens/s; the other order queues
  // them behind 8-16 tile instructions in the CU's vector-memory pipeline, and the MFMAs need both)
  bf16x8_t xf[RB][8];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const bf16_t* xp = x + (__umul24(min(rb * 16 + row, R - 1), ldx) + g * 8);
#pragma unroll
    for (int u = 0; u < 8; ++u) ld16(xf[rb][u], xp + min(kbase + u * 32, K - 32));
  }
  stage(0);
  if constexpr (KW > 1) stage(1);
#pragma unroll
  for (int t = 0; t < KW; ++t) {
    if (t + 1 < KW) wait_vm<8>(); else wait_vm<0>();               // loads issued behind tile t: tile t + 1's eight
    if (t == 0) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int u = 0; u < 8; ++u) tie(xf[rb][u]);
    }
    const char* tr = tile[t & 1] + row * 512;
    bf16x8_t wf[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) wf[u] = *reinterpret_cast<const bf16x8_t*>(tr + (((u * 4 + g) ^ row) << 4));
    if (t + 2 < KW) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage(t + 2);
    }
    f32x4_t d[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) d[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (kbase + u * 32 < K) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) d[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[rb][u], wf[u], d[rb], 0, 0, 0);
      }
    const int n = (grp0 + t) * 16 + row;
    float* ap = acc + __umul24(n, sn);
    if constexpr (ORD) ap += (int64_t)blockIdx.x * f.part_slot;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rb * 16 + g * 4 + j;
        if (r < R && n < N) {
          if constexpr (ORD) ap[__umul24(r, sr)] = d[rb][j];
          else atomicAdd(ap + __umul24(r, sr), d[rb][j]);
        }
      }
    }
  }
}

// fp32-operand modes: FOUR waves per workgroup share one k-slab (each owns KW weight groups and its own LDS ring).
// The operand fragments are built cooperatively -- wave w converts k-steps 2w, 2w+1 for all rows and parks them in
// LDS -- because every wave re-reading the fp32 slab itself costs more L2 bandwidth than the weights cost HBM
// (measured: gate_up 14.5 -> 28.8 us).
// Grid: (k-slabs, chunks of NW x KW weight-row groups), or -- many slabs (the down projection) -- (8, chunks, ceil(slabs / 8)):
// the workgroups that share a slab -- and therefore its fp32 operand, which the previous launch's atomics left at the device
// coherence point -- then sit on ONE XCD (workgroups go to the XCDs round robin in x-fastest linear order), so the slab comes
// through the slow path once per XCD instead of once per workgroup (7.7 -> 1.1 MB per launch); surplus workgroups of the padded
// grid (slab >= nslabs) only take part in the clears.  Either way slab = x + 8 z, chunk = y: no division in the kernel.
// Argument order: the 14 dwords in front are what the operand loads and the weight tiles need (p0 / p1 / ld1 / nw: see
// decode_operand_load; p1 = the statistics slot for XIN_SWIGLU); built with kernarg preload (Makefile) they arrive in SGPRs with the wave.
// CLR = the launch carries clears (its first memory operations, so their arguments are fetched up front); a launch without them
// fetches the rest of its arguments behind the first tiles' requests.
// NPEND >= 0: the ORDERED form of the XIN_RESID_NORM launch (deterministic decode, ug_decode_gemv_resid_norm_ord).  The pending term is
// NPEND partial slots p1[p][R][ld1] (the k-block partials of the previous down projection; 0 = none), summed in ascending p in fp32 and
// then rounded to bf16 like the raw accumulator; the workgroup's partial tile is STORED into k-slab `slab`'s slot acc[slab][R][sr], and
// weight group 0's workgroups store their slab's row sums of squares (waves summed in ascending order through LDS) into ss_out[slab][32].
// No float atomics, no clears.
template <int RB, int KW, int XIN, int NW, bool CLR, int NPEND = -1>
__global__ __launch_bounds__(64 * NW) void gemv_ring4_kernel(const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ nw,
                                                             const bf16_t* __restrict__ W, int R, int K, int ld1, int ldw, int N, int nslabs,
                                                             float* __restrict__ acc, int sr, int sn, DecodeIn f) {
  __shared__ __attribute__((aligned(1024))) char tile[NW][2][8192];
  __shared__ __attribute__((aligned(16))) bf16x8_t frag[RB][8][64];
  constexpr int UPW = (8 + NW - 1) / NW;           // k-steps of the operand each wave converts
  constexpr bool ORD = NPEND >= 0;
  static_assert(!ORD || (XIN == XIN_RESID_NORM && !CLR), "the ordered form is the q/k/v launch, which carries no clears");
  __shared__ float ssl[ORD ? NW : 1][RB * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, row = lane & 15;
  const int slab = blockIdx.x + 8 * blockIdx.z, chunk = blockIdx.y;
  asm volatile("" ::"s"(p0), "s"(p1), "s"(nw), "s"(W), "s"(R), "s"(K), "s"(ld1), "s"(ldw), "s"(N), "s"(nslabs));      // batch 1 (vmem_asm.h, argument hoisting)
  auto rest_of_args = [&] {                        // batch 2: ONE asm statement (gridDim / blockDim are implicit arguments)
    if constexpr (CLR)
      asm volatile("" ::"s"(acc), "s"(sr), "s"(sn), "s"(gridDim.x), "s"(gridDim.y), "s"(blockDim.x), "s"(f.zero0), "s"(f.zero1), "s"(f.ss_zero),
                   "s"(f.n0_4), "s"(f.per0), "s"(f.n1_4), "s"(f.per1), "s"(f.x_out), "s"(f.ss_out), "s"(__float_as_int(f.eps)), "s"(f.norm_cols));
    else
      asm volatile("" ::"s"(acc), "s"(sr), "s"(sn), "s"(f.x_out), "s"(f.ss_out), "s"(__float_as_int(f.eps)), "s"(f.norm_cols));
  };
  if constexpr (CLR) {
    rest_of_args();
    decode_clear(f, threadIdx.x, linear_block(), blockDim.x);  // the clears this launch carries go out first (see gemv_ring_kernel)
  }
  if (slab >= nslabs) return;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int grp0 = (chunk * NW + wave_u) * KW;
  const int kbase = slab * 256;
  const bool whole = (N & 15) == 0;
  // Every load of this kernel is hand-issued (vmem_asm.h).  With the builtins the operand image below -- an LDS write -- was preceded by
  // a compiler-inserted s_waitcnt vmcnt(0): it was built only after BOTH weight tiles had landed (5-6 us into the gate/up launch), and
  // the ring's third tile could only be requested after that.  Now the image is built as soon as the operand's own round trip ends.
  // operand loads of this wave's k-steps go out first, then the weight DMA
  f32x4_t a[RB][UPW][2], b[RB][UPW][2], w[RB][UPW][2];
  f32x4_t pp[ORD && NPEND > 0 ? NPEND : 1][RB][UPW][2];       // ORD: the pending partial slots
  float rs[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int ar = min(rb * 16 + row, R - 1);
    rs[rb] = 0.f;
    if constexpr (XIN == XIN_SWIGLU) ld4(rs[rb], p1 + ar);
#pragma unroll
    for (int uu = 0; uu < UPW; ++uu) {
      const int u = min(wave + uu * NW, 7);
      const int k0 = min(kbase + u * 32, K - 32) + g * 8;
      if constexpr (ORD) {
        const float* xp = p0 + (__umul24(ar, K) + k0);
        ld16(a[rb][uu][0], xp); ld16(a[rb][uu][1], xp + 4);
        ld16(w[rb][uu][0], nw + k0); ld16(w[rb][uu][1], nw + k0 + 4);
#pragma unroll
        for (int p = 0; p < NPEND; ++p) {
          const float* q = p1 + ((p * R + ar) * ld1 + k0);
          ld16(pp[p][rb][uu][0], q); ld16(pp[p][rb][uu][1], q + 4);
        }
      } else {
        decode_operand_load<XIN>(p0, p1, ld1, nw, ar, k0, K, a[rb][uu], b[rb][uu], w[rb][uu]);
      }
    }
  }
  TileAddr ta;
  ta.init(lane, kbase, K, ldw);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(tile[wave][0]));
  auto stage = [&](int t) {
    const uint32_t dst = lds0 + (t & 1) * 8192;
    if (whole) {
      const uint64_t base = (uint64_t)(W + (int64_t)min((grp0 + t) * 16, N - 16) * ldw);
#pragma unroll
      for (int i = 0; i < 8; ++i) dma16_nt(base, ta.lane_off[i], dst + i * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) dma16_nt((uint64_t)W, ta.ragged(lane, (grp0 + t) * 16, i, kbase, N, K, ldw), dst + i * 1024);
    }
  };
  stage(0);
  if constexpr (KW > 1) stage(1);
  if constexpr (!CLR) rest_of_args();               // (their round trip hides under the operand's)
  wait_vm<(KW > 1 ? 16 : 8)>();                     // the operand's loads are older than the tiles' DMA
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    if constexpr (XIN == XIN_SWIGLU) tie(rs[rb]);
#pragma unroll
    for (int uu = 0; uu < UPW; ++uu) {
      if constexpr (ORD) {
        tie(a[rb][uu][0]); tie(a[rb][uu][1]); tie(w[rb][uu][0]); tie(w[rb][uu][1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {              // pending term: slots summed in ascending order (bf16-rounded in decode_operand_make)
          b[rb][uu][h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < NPEND; ++p) { tie(pp[p][rb][uu][h]); b[rb][uu][h] = p == 0 ? pp[0][rb][uu][h] : b[rb][uu][h] + pp[p][rb][uu][h]; }
        }
      } else {
        tie(a[rb][uu][0]); tie(a[rb][uu][1]); tie(b[rb][uu][0]); tie(b[rb][uu][1]);
        if constexpr (XIN == XIN_RESID_NORM) { tie(w[rb][uu][0]); tie(w[rb][uu][1]); }
      }
    }
  }
  float ssq_row[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    if constexpr (XIN == XIN_SWIGLU) rs[rb] = rsqrtf(rs[rb] / (float)f.norm_cols + f.eps);
    float ssq = 0.f;
#pragma unroll
    for (int uu = 0; uu < UPW; ++uu) {
      const int u = wave + uu * NW;
      if (u < 8) {
        const bool in_k = kbase + u * 32 < K;                        // clamped (re-read) steps carry no new data
        float part = 0.f;
        frag[rb][u][lane] = decode_operand_make<XIN>(f, a[rb][uu], b[rb][uu], w[rb][uu], rs[rb], part);
        if (in_k) ssq += part;
      }
    }
    if constexpr (XIN == XIN_RESID_NORM) {
      ssq += __shfl_xor(ssq, 16, 64);
      ssq += __shfl_xor(ssq, 32, 64);
    }
    ssq_row[rb] = ssq;
  }
  lds_barrier();
  bf16x8_t xf[RB][8];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int u = 0; u < 8; ++u) xf[rb][u] = frag[rb][u][lane];
#pragma unroll
  for (int t = 0; t < KW; ++t) {
    if (t + 1 < KW) wait_vm<8>(); else wait_vm<0>();               // loads issued behind tile t: tile t + 1's eight
    const char* tr = tile[wave][t & 1] + row * 512;
    bf16x8_t wf[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) wf[u] = *reinterpret_cast<const bf16x8_t*>(tr + (((u * 4 + g) ^ row) << 4));
    if (t + 2 < KW) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage(t + 2);
    }
    f32x4_t d[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) d[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (kbase + u * 32 < K) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) d[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[rb][u], wf[u], d[rb], 0, 0, 0);
      }
    const int n = (grp0 + t) * 16 + row;
    float* ap = acc + __umul24(n, sn);
    if constexpr (ORD) ap += (int64_t)slab * R * sr;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rb * 16 + g * 4 + j;
        if (r < R && n < N) {
          if constexpr (ORD) ap[__umul24(r, sr)] = d[rb][j];
          else atomicAdd(ap + __umul24(r, sr), d[rb][j]);
        }
      }
    }
  }
  // the updated residual stream and its row statistics (weight group 0's workgroups) leave last: no store sits between the loads above
  if constexpr (XIN == XIN_RESID_NORM) {
    if (chunk == 0) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const bool live = rb * 16 + row < R;
#pragma unroll
        for (int uu = 0; uu < UPW; ++uu) {
          const int u = wave + uu * NW;
          if (u < 8 && live && kbase + u * 32 < K) {
            float* op = f.x_out + (__umul24(rb * 16 + row, K) + kbase + u * 32 + g * 8);
            *reinterpret_cast<f32x4_t*>(op) = a[rb][uu][0];
            *reinterpret_cast<f32x4_t*>(op + 4) = a[rb][uu][1];
          }
        }
        if constexpr (ORD) { if (g == 0) ssl[wave][rb * 16 + row] = ssq_row[rb]; }
        else if (live && g == 0 && f.ss_out && ssq_row[rb] != 0.f) atomicAdd(f.ss_out + rb * 16 + row, ssq_row[rb]);
      }
      if constexpr (ORD) {
        __syncthreads();
        const int r = threadIdx.x;
        if (r < RB * 16 && r < R) {
          float s = ssl[0][r];
#pragma unroll
          for (int ww = 1; ww < NW; ++ww) s += ssl[ww][r];
          f.ss_out[slab * 32 + r] = s;
        }
      }
    }
  }
}

// ---- host side: the entry points check their arguments, decode_plan.h says what to launch, and one dispatch function per kernel
// family names each instantiation once (ug_launch, common.h).  A plan that no case names is an error, never another kernel.
using ug_plan::RingPlan;
static_assert(XIN_BF16 == ug_plan::DEC_XIN_BF16, "plan_ring4 tells the one-wave ring form by this value");
dim3 to_dim3(const ug_plan::Grid3& g) { return dim3(g.x, g.y, g.z); }

// gemv_kernel<RB, U>
int launch_gemv(const char* name, const ug_plan::GemvPlan& pl, hipStream_t st, const bf16_t* x, int64_t ldx, int R, const bf16_t* W, int64_t ldw,
                float* acc, int64_t sr, int64_t sn, int N, int K) {
  auto go = [&](auto kern) { return ug_launch(name, kern, to_dim3(pl.grid), dim3(pl.block), st, x, ldx, R, W, ldw, acc, sr, sn, N, K); };
  switch (pl.RB * 16 + pl.U) {
    case 16 + 8: return go(gemv_kernel<1, 8>);
    case 16 + 4: return go(gemv_kernel<1, 4>);
    case 16 + 2: return go(gemv_kernel<1, 2>);
    case 16 + 1: return go(gemv_kernel<1, 1>);
    case 32 + 8: return go(gemv_kernel<2, 8>);
    case 32 + 4: return go(gemv_kernel<2, 4>);
    case 32 + 2: return go(gemv_kernel<2, 2>);
    case 32 + 1: return go(gemv_kernel<2, 1>);
  }
  return ug_no_kernel(name);
}

// gemv_ring_kernel<RB, KW, ORD>: the one-wave ring over a finished bf16 operand; ORD = the ordered form (one slot per k-slab)
int launch_ring1(const char* name, int RB, int KW, bool ord, dim3 grid, hipStream_t st, const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw,
                 float* acc, int sr, int sn, int N, int K, const DecodeIn& f) {
  auto go = [&](auto kern) { return ug_launch(name, kern, grid, dim3(64), st, x, ldx, R, W, ldw, acc, sr, sn, N, K, f); };
  switch ((RB * 4 + KW) * 2 + (ord ? 1 : 0)) {
    case (4 + 1) * 2: return go(gemv_ring_kernel<1, 1>);
    case (4 + 2) * 2: return go(gemv_ring_kernel<1, 2>);
    case (8 + 1) * 2: return go(gemv_ring_kernel<2, 1>);
    case (8 + 2) * 2: return go(gemv_ring_kernel<2, 2>);
    case (4 + 1) * 2 + 1: return go(gemv_ring_kernel<1, 1, true>);
    case (8 + 1) * 2 + 1: return go(gemv_ring_kernel<2, 1, true>);
  }
  return ug_no_kernel(name);
}

// gemv_ring4_kernel<RB, KW, XIN, NW, CLR, NPEND>.  npend < 0: the accumulator forms of the plan; 0 | 5: the ordered form of
// ug_decode_gemv_resid_norm_ord.  (p0, p1, nw, ld1: the kernel's leading arguments, see there.)  <., 2, ., 4, .> is not here: no shape
// selects it (decode_plan.h, DEC_RING_CANDS).
template <int XIN>
int launch_ring4(const char* name, const RingPlan& pl, int npend, hipStream_t st, const float* p0, const float* p1, const float* nw,
                 const bf16_t* W, int R, int K, int ld1, int ldw, int N, float* acc, int sr, int sn, const DecodeIn& f) {
  auto go = [&](auto kern) {
    return ug_launch(name, kern, to_dim3(pl.grid), dim3(pl.block), st, p0, p1, nw, W, R, K, ld1, ldw, N, (int)ug_plan::dec_slabs(K), acc, sr, sn, f);
  };
  auto go2 = [&](auto with_clears, auto without) { return go(pl.CLR ? with_clears : without); };
  if constexpr (XIN == XIN_RESID_NORM) {
    if (npend == 0) return go(gemv_ring4_kernel<1, 1, XIN_RESID_NORM, 4, false, 0>);
    if (npend == ug_plan::DEC_ORD_DOWN_KBLOCKS) return go(gemv_ring4_kernel<1, 1, XIN_RESID_NORM, 4, false, 5>);
  }
  if (npend >= 0) return ug_no_kernel(name);
  switch ((pl.RB * 4 + pl.KW) * 16 + pl.NW) {
    case (4 + 3) * 16 + 9: return go2(gemv_ring4_kernel<1, 3, XIN, 9, true>, gemv_ring4_kernel<1, 3, XIN, 9, false>);
    case (4 + 2) * 16 + 8: return go2(gemv_ring4_kernel<1, 2, XIN, 8, true>, gemv_ring4_kernel<1, 2, XIN, 8, false>);
    case (4 + 2) * 16 + 7: return go2(gemv_ring4_kernel<1, 2, XIN, 7, true>, gemv_ring4_kernel<1, 2, XIN, 7, false>);
    case (4 + 1) * 16 + 4: return go2(gemv_ring4_kernel<1, 1, XIN, 4, true>, gemv_ring4_kernel<1, 1, XIN, 4, false>);
    case (8 + 1) * 16 + 4: return go2(gemv_ring4_kernel<2, 1, XIN, 4, true>, gemv_ring4_kernel<2, 1, XIN, 4, false>);
  }
  return ug_no_kernel(name);
}

// the three ug_decode_gemv* entries and the ring form of ug_gemv_bf16: plan, every workgroup's share of the clears, launch
template <int XIN>
int launch_ring_auto(const char* name, hipStream_t st, const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, float* acc, int sr, int sn,
                     int N, int K, DecodeIn f, float* zero0 = nullptr, int64_t n0 = 0, float* zero1 = nullptr, int64_t n1 = 0,
                     float* ss_zero = nullptr) {
  const RingPlan pl = ug_plan::plan_ring4(XIN, R, N, K, zero0 || zero1 || ss_zero);
  const ug_plan::ClearShares c = ug_plan::clear_shares(n0, n1, pl.nblocks());
  f.zero0 = zero0; f.zero1 = zero1; f.ss_zero = ss_zero;
  f.n0_4 = c.n0_4; f.per0 = c.per0; f.n1_4 = c.n1_4; f.per1 = c.per1;
  if constexpr (XIN == XIN_BF16) {
    return launch_ring1(name, pl.RB, pl.KW, false, to_dim3(pl.grid), st, x, ldx, R, W, ldw, acc, sr, sn, N, K, f);
  } else {
    // leading arguments: see the kernel
    const float* p0 = XIN == XIN_RESID_NORM ? f.x_in : f.gu;
    const float* p1 = XIN == XIN_RESID_NORM ? f.pend : f.ss_in;
    const int64_t ld1 = XIN == XIN_RESID_NORM ? f.ld_pend : f.ld_gu;          // (< 2^24: checked by the entry points)
    return launch_ring4<XIN>(name, pl, -1, st, p0, p1, f.norm_w, W, R, K, (int)ld1, ldw, N, acc, sr, sn, f);
  }
}

// attn_decode_fused_kernel<NQP>: nparts == 0 reads the raw accumulator, nparts == 6 that many k-slab slots in ascending order
int launch_attn_decode_fused(const char* name, int64_t nparts, const float* qkv, int64_t ld, const float* ss, float eps, int64_t norm_cols,
                             const void* bias, const float* cos_tab, const float* sin_tab, const int* pos_dev, void* cache_k, void* cache_v,
                             const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows, int H, int HKV, int64_t Tmax, int64_t max_pos,
                             float scale, hipStream_t st) {
  auto go = [&](auto kern) {
    return ug_launch(name, kern, to_dim3(ug_plan::attn_decode_fused_grid(rows, H, HKV)), dim3(64 * ADF_WAVES), st, qkv, ss, pos_dev,
                     (bf16_t*)cache_k, (bf16_t*)cache_v, (int)rows, HKV, H, (int)ld, (int)Tmax, (int)max_pos, (const bf16_t*)bias, cos_tab,
                     sin_tab, key_valid, (bf16_t*)o, ldo, eps, (int)norm_cols, scale);
  };
  if (nparts == 0) return go(attn_decode_fused_kernel<0>);
  if (nparts == ug_plan::DEC_ORD_QKV_SLABS) return go(attn_decode_fused_kernel<6>);
  return ug_no_kernel(name);
}

// finish_resid_norm_kernel<MAXV> (nparts == 0: src is the accumulator, which the kernel also clears) or
// finish_resid_norm_ord_kernel<MAXV> (src holds nparts slots of rows x ld floats)
int launch_finish_resid_norm(const char* name, int64_t nparts, const float* src, int64_t ld, float* x, const float* w, void* xn, int64_t rows,
                             int64_t cols, float eps, int* pos_inc, int* len_inc, hipStream_t st) {
  const dim3 grid((unsigned)rows), block(64);
  auto acc_form = [&](auto kern) {
    return ug_launch(name, kern, grid, block, st, const_cast<float*>(src), ld, x, w, (bf16_t*)xn, (int)cols, eps, pos_inc, len_inc);
  };
  auto ord_form = [&](auto kern) {
    return ug_launch(name, kern, grid, block, st, src, (int)ld, (int)nparts, x, w, (bf16_t*)xn, (int)cols, eps, pos_inc, len_inc);
  };
  switch (ug_plan::finish_vectors(cols) + (nparts ? 1 : 0)) {
    case 8: return acc_form(finish_resid_norm_kernel<8>);
    case 16: return acc_form(finish_resid_norm_kernel<16>);
    case 8 + 1: return ord_form(finish_resid_norm_ord_kernel<8>);
    case 16 + 1: return ord_form(finish_resid_norm_ord_kernel<16>);
  }
  return ug_no_kernel(name);
}

// 32-bit / 24-bit ranges of the ring kernels' addressing (weights up to 2^31 elements, strides below 2^24)
// ... and of their grids: weight-row groups ride in grid.y (at most 65 535 workgroups: N <= 16 x 65 535 rows with one group per
// workgroup, the smallest unit any launch shape uses), k-slabs in grid.x or, eight at a time, in grid.z
#define UG_RING_RANGES(name, N, K, ldw, sr, sn)                                                                                      \
  UG_REQUIRE((N) < (1 << 24) && (K) < (1 << 24) && (ldw) < (1 << 24) && (int64_t)(N) * (ldw) < (1ll << 31) && (sr) < (1 << 24) &&    \
                 (sn) < (1 << 24) && (int64_t)(N) * (sn) + 32 * (int64_t)(sr) < (1ll << 31),                                         \
             name ": sizes beyond the kernels' 32-bit addressing (N=%ld K=%ld ldw=%ld)", (long)(N), (long)(K), (long)(ldw));         \
  UG_REQUIRE(((N) + 15) / 16 <= 65535 && ((K) + 255) / 256 <= 65535 * 8,                                                              \
             name ": N = %ld weight rows / K = %ld exceed the launch grid (16 x 65 535 rows, 2 048 x 65 535 columns)", (long)(N), (long)(K))

}  // namespace

extern "C" int ug_gemv_bf16(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* acc, int64_t acc_stride_r,
                            int64_t acc_stride_n, int64_t N, int64_t K, hipStream_t st) {
  UG_REQUIRE(R > 0 && R <= 32 && N > 0 && K > 0 && K % 32 == 0, "ug_gemv_bf16: need 1 <= rows <= 32 and K %% 32 == 0 (rows=%ld K=%ld)", (long)R, (long)K);
  UG_REQUIRE(ldx % 8 == 0 && ldw % 8 == 0 && ug_aligned16(x) && ug_aligned16(W), "ug_gemv_bf16: 16-byte aligned rows required");
  const bf16_t* xb = (const bf16_t*)x;
  const bf16_t* wb = (const bf16_t*)W;
  const ug_plan::GemvPlan pl = ug_plan::plan_gemv((int)R, N, K);
  if (pl.ring) {
    UG_RING_RANGES("ug_gemv_bf16", N, K, ldw, acc_stride_r, acc_stride_n);
    UG_REQUIRE(ldx < (1 << 24), "ug_gemv_bf16: ldx beyond 2^24");
    return launch_ring_auto<XIN_BF16>("ug_gemv_bf16", st, xb, (int)ldx, (int)R, wb, (int)ldw, acc, (int)acc_stride_r, (int)acc_stride_n, (int)N,
                                      (int)K, DecodeIn{});
  }
  return launch_gemv("ug_gemv_bf16", pl, st, xb, ldx, (int)R, wb, ldw, acc, acc_stride_r, acc_stride_n, (int)N, (int)K);
}

#define UG_DECODE_COMMON(name)                                                                                              \
  UG_REQUIRE(R > 0 && R <= 32 && K >= 256 && K % 32 == 0 && N > 0 && ldw % 8 == 0 && ug_aligned16(W) && acc &&              \
                 ug_aligned16(acc) && ldacc % 4 == 0 && n0 % 4 == 0 && n1 % 4 == 0 && ug_aligned16(zero0) && ug_aligned16(zero1), \
             name ": need 1 <= rows <= 32, K >= 256, K %% 32 == 0, 16-byte aligned operands (rows=%ld K=%ld)", (long)R, (long)K);                        \
  UG_RING_RANGES(name, N, K, ldw, ldacc, 1);                                                                                 \
  UG_REQUIRE(n0 < (1ll << 31) && n1 < (1ll << 31), name ": clears beyond 2^31 floats")

extern "C" int ug_decode_gemv(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* acc, int64_t ldacc,
                              int64_t N, int64_t K, float* zero0, int64_t n0, float* zero1, int64_t n1, float* ss_zero,
                              hipStream_t st) {
  UG_DECODE_COMMON("ug_decode_gemv");
  UG_REQUIRE(x && ldx % 8 == 0 && ug_aligned16(x), "ug_decode_gemv: activations must be 16-byte aligned rows");
  UG_REQUIRE(ldx < (1 << 24), "ug_decode_gemv: ldx beyond 2^24");
  return launch_ring_auto<XIN_BF16>("ug_decode_gemv", st, (const bf16_t*)x, (int)ldx, (int)R, (const bf16_t*)W, (int)ldw, acc, (int)ldacc, 1, (int)N,
                                    (int)K, DecodeIn{}, zero0, n0, zero1, n1, ss_zero);
}

extern "C" int ug_decode_gemv_resid_norm(const float* x_in, const float* pending, int64_t ld_pending, const float* norm_w,
                                         float* x_out, float* ss_out, int64_t R, const void* W, int64_t ldw, float* acc,
                                         int64_t ldacc, int64_t N, int64_t K, float* zero0, int64_t n0, float* zero1, int64_t n1,
                                         float* ss_zero, hipStream_t st) {
  UG_DECODE_COMMON("ug_decode_gemv_resid_norm");
  UG_REQUIRE(x_in && pending && norm_w && x_out && ss_out && x_in != x_out && ld_pending % 4 == 0 && ug_aligned16(x_in) &&
                 ug_aligned16(pending) && ug_aligned16(norm_w) && ug_aligned16(x_out),
             "ug_decode_gemv_resid_norm: bad args (x_in and x_out must be distinct, 16-byte aligned fp32 buffers)");
  DecodeIn f{};
  f.x_in = x_in; f.pend = pending; f.ld_pend = ld_pending; f.norm_w = norm_w; f.x_out = x_out; f.ss_out = ss_out;
  UG_REQUIRE(ld_pending < (1 << 24), "ug_decode_gemv_resid_norm: ld_pending beyond 2^24");
  return launch_ring_auto<XIN_RESID_NORM>("ug_decode_gemv_resid_norm", st, nullptr, 0, (int)R, (const bf16_t*)W, (int)ldw, acc, (int)ldacc, 1, (int)N,
                                          (int)K, f, zero0, n0, zero1, n1, ss_zero);
}

extern "C" int ug_decode_gemv_swiglu(const float* gate_up_acc, int64_t ld_gu, const float* ss_in, float eps, int64_t norm_cols,
                                     int64_t R, const void* W, int64_t ldw, float* acc, int64_t ldacc, int64_t N, int64_t K,
                                     float* zero0, int64_t n0, float* zero1, int64_t n1, float* ss_zero, hipStream_t st) {
  UG_DECODE_COMMON("ug_decode_gemv_swiglu");
  UG_REQUIRE(gate_up_acc && ss_in && norm_cols > 0 && ld_gu % 4 == 0 && K % 4 == 0 && ug_aligned16(gate_up_acc),
             "ug_decode_gemv_swiglu: bad args");
  DecodeIn f{};
  f.gu = gate_up_acc; f.ld_gu = ld_gu; f.ss_in = ss_in; f.eps = eps; f.norm_cols = (int)norm_cols;
  UG_REQUIRE(ld_gu < (1 << 24), "ug_decode_gemv_swiglu: ld_gu beyond 2^24");
  return launch_ring_auto<XIN_SWIGLU>("ug_decode_gemv_swiglu", st, nullptr, 0, (int)R, (const bf16_t*)W, (int)ldw, acc, (int)ldacc, 1, (int)N, (int)K, f,
                                      zero0, n0, zero1, n1, ss_zero);
}

extern "C" int ug_decode_finish_resid_norm(float* acc, int64_t ldacc, float* x, const float* w, void* xn, int64_t rows,
                                           int64_t cols, float eps, int* pos_inc, int* len_inc, hipStream_t st) {
  UG_REQUIRE((pos_inc == nullptr) == (len_inc == nullptr), "ug_decode_finish_resid_norm: pos_inc / len_inc come together");
  UG_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 4096 && ldacc % 4 == 0 && acc && x && w && xn,
             "ug_decode_finish_resid_norm: bad args (cols=%ld, multiple of 4 and <= 4096)", (long)cols);
  UG_REQUIRE(ug_aligned16(x) && ug_aligned16(w) && ug_aligned16(acc) && ((uintptr_t)xn & 7) == 0,
             "ug_decode_finish_resid_norm: alignment");
  return launch_finish_resid_norm("ug_decode_finish_resid_norm", 0, acc, ldacc, x, w, xn, rows, cols, eps, pos_inc, len_inc, st);
}

extern "C" int ug_kv_store(const void* qkv, int64_t ldq, int64_t k_col, int64_t v_col, void* cache_k, void* cache_v,
                           int64_t rows, int64_t L, int HKV, int head_dim, int64_t Tmax, const int* pos_dev, int pos_host,
                           hipStream_t st) {
  UG_REQUIRE(rows > 0 && L > 0 && head_dim == DHD && ldq % 8 == 0 && k_col % 8 == 0 && v_col % 8 == 0, "ug_kv_store: bad args");
  UG_REQUIRE(ug_aligned16(qkv) && ug_aligned16(cache_k) && ug_aligned16(cache_v), "ug_kv_store: alignment");
  const int64_t total = rows * L * HKV * (DHD / 8);
  int64_t g = (total + 255) / 256; if (g > 2048) g = 2048;
  hipLaunchKernelGGL(kv_store_kernel, dim3((unsigned)g), dim3(256), 0, st, (const bf16_t*)qkv, ldq, (int)k_col, (int)v_col,
                     (bf16_t*)cache_k, (bf16_t*)cache_v, (int)rows, (int)L, HKV, (int)Tmax, pos_dev, pos_host);
  UG_CHECK_LAUNCH("ug_kv_store");
  return UG_OK;
}

extern "C" int ug_rope_at(void* qkv, const float* cos_tab, const float* sin_tab, int64_t rows, int64_t ldq, int nheads,
                          int head_dim, const int* pos_dev, int64_t max_pos, hipStream_t st) {
  UG_REQUIRE(rows > 0 && head_dim % 8 == 0 && pos_dev, "ug_rope_at: bad args");
  const int total = (int)(rows * nheads * (head_dim / 8));
  hipLaunchKernelGGL(rope_at_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (bf16_t*)qkv, cos_tab, sin_tab, (int)rows,
                     (int)ldq, nheads, head_dim, pos_dev, (int)max_pos);
  UG_CHECK_LAUNCH("ug_rope_at");
  return UG_OK;
}

extern "C" int ug_attn_decode(const void* q, int64_t ldq, const void* cache_k, const void* cache_v, const uint8_t* key_valid,
                              void* o, int64_t ldo, int64_t rows, int H, int HKV, int head_dim, int64_t Tmax,
                              const int* len_dev, float scale, hipStream_t st) {
  UG_REQUIRE(rows > 0 && head_dim == DHD && H % HKV == 0 && len_dev, "ug_attn_decode: bad args");
  hipLaunchKernelGGL(attn_decode_kernel, dim3(H, (unsigned)rows), dim3(64 * AD_WAVES), 0, st, (const bf16_t*)q, ldq, (const bf16_t*)cache_k,
                     (const bf16_t*)cache_v, key_valid, (bf16_t*)o, ldo, H, HKV, (int)Tmax, len_dev, scale);
  UG_CHECK_LAUNCH("ug_attn_decode");
  return UG_OK;
}

extern "C" int ug_attn_decode_fused(const float* acc_qkv, int64_t ldacc, const float* ss_in, float eps, int64_t norm_cols,
                                    const void* bias, const float* cos_tab, const float* sin_tab, const int* pos_dev,
                                    void* cache_k, void* cache_v, const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows,
                                    int H, int HKV, int head_dim, int64_t Tmax, int64_t max_pos, float scale, hipStream_t st) {
  UG_REQUIRE(rows > 0 && head_dim == DHD && H % HKV == 0 && acc_qkv && ss_in && norm_cols > 0 && pos_dev && cache_k && cache_v && o,
             "ug_attn_decode_fused: bad args");
  UG_REQUIRE(ldacc > 0 && ldacc < (1ll << 31), "ug_attn_decode_fused: ldacc out of range");
  return launch_attn_decode_fused("ug_attn_decode_fused", 0, acc_qkv, ldacc, ss_in, eps, norm_cols, bias, cos_tab, sin_tab, pos_dev, cache_k, cache_v,
                                  key_valid, o, ldo, rows, H, HKV, Tmax, max_pos, scale, st);
}

extern "C" int ug_attn_decode_seq(const float* acc_qkv, int64_t ldacc, const float* ss_in, float eps, int64_t norm_cols,
                                  const void* bias, const float* cos_tab, const float* sin_tab, const int* pos_dev, void* cache_k,
                                  void* cache_v, const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows, int H, int HKV,
                                  int head_dim, int64_t Tmax, int64_t max_pos, float scale, hipStream_t st) {
  UG_REQUIRE(head_dim == DHD && rows >= 1 && rows <= ADS_MAX_ROWS && HKV > 0 && H > 0 && H % HKV == 0 && H <= 1024 && Tmax > 0 &&
                 Tmax < (1ll << 24) && max_pos > 0 && max_pos < (1ll << 24) && norm_cols > 0 && acc_qkv && ss_in && cos_tab && sin_tab &&
                 pos_dev && cache_k && cache_v && o,
             "ug_attn_decode_seq: bad args (head_dim 128, 1 <= rows <= %d consecutive positions of one sequence)", ADS_MAX_ROWS);
  UG_REQUIRE(ldacc >= (int64_t)(H + 2 * HKV) * DHD && ldacc < (1ll << 27) && ldo >= (int64_t)H * DHD && ug_aligned16(cache_k) &&
                 ug_aligned16(cache_v),
             "ug_attn_decode_seq: ldacc / ldo below the q/k/v width or out of range, or a cache that is not 16-byte aligned");
  return ug_launch("ug_attn_decode_seq", attn_decode_seq_kernel, dim3((unsigned)H, (unsigned)rows), dim3(64 * ADS_WAVES), st, acc_qkv, ss_in,
                   pos_dev, (bf16_t*)cache_k, (bf16_t*)cache_v, HKV, H, (int)ldacc, (int)Tmax, (int)max_pos, (const bf16_t*)bias, cos_tab,
                   sin_tab, key_valid, (bf16_t*)o, ldo, eps, (int)norm_cols, scale);
}

extern "C" int ug_skinny_finish(const float* acc, const void* bias, void* out_bf16, float* resid, int64_t M, int64_t N,
                                int mode, hipStream_t st) {
  UG_REQUIRE(M > 0 && N > 0 && (mode == 0 ? out_bf16 != nullptr : resid != nullptr), "ug_skinny_finish: bad args");
  const int64_t total = M * N;
  int64_t g = (total + 255) / 256; if (g > 1024) g = 1024;
  // one slot; the kernel tells the output by the pointer that is given (mode 0: out_bf16, else resid)
  hipLaunchKernelGGL(skinny_finish_kernel, dim3((unsigned)g), dim3(256), 0, st, acc, 1, (int64_t)0, (const bf16_t*)bias,
                     (bf16_t*)(mode == 0 ? out_bf16 : nullptr), (float*)nullptr, mode == 0 ? nullptr : resid, total, (int)N);
  UG_CHECK_LAUNCH("ug_skinny_finish");
  return UG_OK;
}

// ------------------------------------------------------------------ ordered (deterministic) decode forms: include/unigen_hip.h
extern "C" int ug_gemv_bf16_ord(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* part, int64_t ldpart,
                                int64_t part_stride, int64_t N, int64_t K, hipStream_t st) {
  UG_REQUIRE(R > 0 && R <= 32 && N > 0 && K > 0 && K % 32 == 0 && x && W && part, "ug_gemv_bf16_ord: need 1 <= rows <= 32 and K %% 32 == 0 (rows=%ld K=%ld)",
             (long)R, (long)K);
  UG_REQUIRE(ldx % 8 == 0 && ldw % 8 == 0 && ug_aligned16(x) && ug_aligned16(W) && ldpart >= N && part_stride >= R * ldpart,
             "ug_gemv_bf16_ord: 16-byte aligned rows, ldpart >= N and slots of rows x ldpart required");
  UG_REQUIRE(part_stride * ug_plan::dec_slabs(K) < (1ll << 31) && ldx < (1 << 24), "ug_gemv_bf16_ord: partial slots beyond 2^31 floats");
  // one wave per (k-slab, 16 weight rows): slot = k-slab (a contraction shorter than 256 is one slab; the tile loads clamp to K and the
  // steps past K are skipped)
  UG_RING_RANGES("ug_gemv_bf16_ord", N, K, ldw, ldpart, 1);
  DecodeIn f{};
  f.part_slot = (int)part_stride;
  return launch_ring1("ug_gemv_bf16_ord", R <= ug_plan::DEC_RING_MAX_ROWS1 ? 1 : 2, 1, true, to_dim3(ug_plan::gemv_ord_grid(N, K)), st, (const bf16_t*)x,
                      (int)ldx, (int)R, (const bf16_t*)W, (int)ldw, part, (int)ldpart, 1, (int)N, (int)K, f);
}

extern "C" int ug_skinny_finish_ord(const float* parts, int64_t nparts, int64_t part_stride, const void* bias, void* out_bf16, float* out_f32,
                                    float* resid, int64_t M, int64_t N, hipStream_t st) {
  UG_REQUIRE(parts && M > 0 && N > 0 && nparts > 0 && nparts < (1 << 20) && part_stride >= M * N &&
                 (out_bf16 != nullptr) + (out_f32 != nullptr) + (resid != nullptr) == 1 && (bias == nullptr || out_bf16 != nullptr),
             "ug_skinny_finish_ord: bad args (one output of out_bf16 / out_f32 / resid; slots of at least rows x N floats)");
  const int64_t total = M * N;
  int64_t g = (total + 255) / 256; if (g > 1024) g = 1024;
  hipLaunchKernelGGL(skinny_finish_kernel, dim3((unsigned)g), dim3(256), 0, st, parts, (int)nparts, part_stride, (const bf16_t*)bias,
                     (bf16_t*)out_bf16, out_f32, resid, total, (int)N);
  UG_CHECK_LAUNCH("ug_skinny_finish_ord");
  return UG_OK;
}

extern "C" int ug_decode_gemv_resid_norm_ord(const float* x_in, const float* pend_parts, int64_t ld_pending, int64_t npend, const float* norm_w,
                                             float* x_out, float* ss_part, int64_t R, const void* W, int64_t ldw, float* part, int64_t ldpart,
                                             int64_t N, int64_t K, hipStream_t st) {
  UG_REQUIRE(R > 0 && R <= 16 && K >= 256 && K % 32 == 0 && N > 0 && W && ldw % 8 == 0 && ug_aligned16(W) && part && ldpart >= N,
             "ug_decode_gemv_resid_norm_ord: need 1 <= rows <= 16, K >= 256, K %% 32 == 0 (rows=%ld K=%ld)", (long)R, (long)K);
  UG_REQUIRE(npend == 0 || npend == 5, "ug_decode_gemv_resid_norm_ord: built for 0 or 5 pending k-block slots (got %ld)", (long)npend);
  UG_REQUIRE(x_in && norm_w && x_out && ss_part && x_in != x_out && (npend == 0 || pend_parts) && ld_pending % 4 == 0 && ug_aligned16(x_in) &&
                 ug_aligned16(pend_parts) && ug_aligned16(norm_w) && ug_aligned16(x_out),
             "ug_decode_gemv_resid_norm_ord: bad args (x_in and x_out must be distinct, 16-byte aligned fp32 buffers)");
  UG_RING_RANGES("ug_decode_gemv_resid_norm_ord", N, K, ldw, ldpart, 1);
  UG_REQUIRE(npend * R * ld_pending < (1ll << 31) && ug_plan::dec_slabs(K) * R * ldpart < (1ll << 31) && ld_pending < (1 << 24),
             "ug_decode_gemv_resid_norm_ord: partial slots beyond 2^31 floats");
  DecodeIn f{};
  f.x_out = x_out; f.ss_out = ss_part;
  return launch_ring4<XIN_RESID_NORM>("ug_decode_gemv_resid_norm_ord", ug_plan::plan_resid_norm_ord(N, K), (int)npend, st, x_in, pend_parts, norm_w,
                                      (const bf16_t*)W, (int)R, (int)K, (int)ld_pending, (int)ldw, (int)N, part, (int)ldpart, 1, f);
}

extern "C" int ug_attn_decode_fused_ord(const float* qkv_part, int64_t ldpart, int64_t nparts, const float* ss_part, float eps, int64_t norm_cols,
                                        const void* bias, const float* cos_tab, const float* sin_tab, const int* pos_dev,
                                        void* cache_k, void* cache_v, const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows,
                                        int H, int HKV, int head_dim, int64_t Tmax, int64_t max_pos, float scale, hipStream_t st) {
  UG_REQUIRE(rows > 0 && rows <= 32 && head_dim == DHD && HKV > 0 && H % HKV == 0 && qkv_part && ss_part && norm_cols > 0 && pos_dev && cache_k &&
                 cache_v && o, "ug_attn_decode_fused_ord: bad args");
  UG_REQUIRE(nparts == 6, "ug_attn_decode_fused_ord: built for six k-slab slots (a 1536-wide hidden size; got %ld)", (long)nparts);
  UG_REQUIRE(ldpart > 0 && nparts * rows * ldpart < (1ll << 31), "ug_attn_decode_fused_ord: ldpart out of range");
  return launch_attn_decode_fused("ug_attn_decode_fused_ord", nparts, qkv_part, ldpart, ss_part, eps, norm_cols, bias, cos_tab, sin_tab, pos_dev, cache_k,
                                  cache_v, key_valid, o, ldo, rows, H, HKV, Tmax, max_pos, scale, st);
}

extern "C" int ug_decode_finish_resid_norm_ord(const float* parts, int64_t ldp, int64_t nparts, float* x, const float* w, void* xn, int64_t rows,
                                               int64_t cols, float eps, int* pos_inc, int* len_inc, hipStream_t st) {
  UG_REQUIRE((pos_inc == nullptr) == (len_inc == nullptr), "ug_decode_finish_resid_norm_ord: pos_inc / len_inc come together");
  UG_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 4096 && ldp >= cols && ldp % 4 == 0 && nparts > 0 && parts && x && w,
             "ug_decode_finish_resid_norm_ord: bad args (cols=%ld, multiple of 4 and <= 4096)", (long)cols);
  UG_REQUIRE(ug_aligned16(x) && ug_aligned16(w) && ug_aligned16(parts) && ((uintptr_t)xn & 7) == 0 && nparts * rows * ldp < (1ll << 31),
             "ug_decode_finish_resid_norm_ord: alignment / slot range");
  return launch_finish_resid_norm("ug_decode_finish_resid_norm_ord", nparts, parts, ldp, x, w, xn, rows, cols, eps, pos_inc, len_inc, st);
}
