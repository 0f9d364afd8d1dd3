// Scoring given labels against the tied vocabulary without ever holding the logits (include/unigen_hip.h: ug_head_score).
// The only other way to a label's log-probability is ug_gemm_bf16 into a bf16 [R, V] matrix and ug_ce_fwd over it: 320 KB per row
// written and read back for three floats and an index.  Here a workgroup forms a 256-entry slice of the head product for up to 64
// rows in MFMA accumulators, rounds it to bf16 where a Linear output is rounded, and keeps per row only the slice's maximum, the
// first index of it and sum exp(s - maximum); a finishing launch merges a row's slices in slice order.
//
// The product is formed TRANSPOSED (MFMA rows = table entries, MFMA columns = hidden rows), as the attention kernels form their
// scores: in the 32x32 accumulator layout a hidden row is then a LANE and its 16 table entries per tile are that lane's registers,
// so the softmax statistics reduce in registers with one cross-half exchange and one pass through LDS for the four waves.
//
// Bit-reproducible and row-independent by construction: no atomics; every row is reduced on its own in an order fixed by the
// column tile alone (register order in a lane, the two lane halves, waves 0..3, then tiles in order); the row-tile height that
// head_score_plan.h picks from R changes which lane a row sits in and nothing about what is summed for it in which order.
#include "common.h"
#include "head_score_plan.h"
#include "unigen_hip.h"
#include <limits.h>

namespace {

using ug_plan::HS_BK;
using ug_plan::HS_BV;

constexpr int HS_LD = HS_BK + 8;   // bf16 per staged row: 80 bytes, 16-byte aligned, rows spread over the banks

// NT = 32-row tiles of x per workgroup.  Wave w owns table entries [64 w, 64 w + 64) of the column tile (two MFMA row tiles)
// against all 32 NT hidden rows: 2 NT accumulators of 16 registers.
template <int NT>
__global__ __launch_bounds__(256) void head_score_kernel(const bf16_t* __restrict__ x, int64_t ldx, int R,
                                                         const bf16_t* __restrict__ W, int64_t ldw, int V, int K,
                                                         const int64_t* __restrict__ labels, int64_t ignore_index,
                                                         float4* __restrict__ part, float* __restrict__ lab_logit, int row_tiles) {
  constexpr int BR = 32 * NT;
  constexpr int XI = (BR * 4 + 255) / 256;               // 16-byte pieces of the x tile per thread (NT = 1: half the threads load one)
  __shared__ __attribute__((aligned(16))) bf16_t Ws[HS_BV * HS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Xs[BR * HS_LD];
  __shared__ float red_m[4][BR];
  __shared__ int red_i[4][BR];
  __shared__ float red_s[4][BR];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r32 = lane & 31, h = lane >> 5;
  const int rt = (int)ug_plan::head_score_wg_row_tile(blockIdx.x, row_tiles), ct = (int)ug_plan::head_score_wg_col_tile(blockIdx.x, row_tiles);
  const int row0 = rt * BR, v0 = ct * HS_BV;

  // staging: piece p = tid + 256 i is 8 bf16 of row p >> 2 at k = 8 (p & 3).  Rows past the end are clamped to the last real row:
  // nothing behind V or R is ever read, and what the clamped rows produce is masked below.
  const bf16_t* wp[4];
  const bf16_t* xp[XI];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + 256 * i;
    const int e = min(v0 + (p >> 2), V - 1);
    wp[i] = W + (int64_t)e * ldw + (p & 3) * 8;
  }
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int p = min(tid + 256 * i, BR * 4 - 1);
    const int r = min(row0 + (p >> 2), R - 1);
    xp[i] = x + (int64_t)r * ldx + (p & 3) * 8;
  }
  bf16x8_t wr[4], xr[XI];
#pragma unroll
  for (int i = 0; i < 4; ++i) wr[i] = *reinterpret_cast<const bf16x8_t*>(wp[i]);
#pragma unroll
  for (int i = 0; i < XI; ++i) xr[i] = *reinterpret_cast<const bf16x8_t*>(xp[i]);

  f32x16_t acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0.f;

  const int nk = K / HS_BK;
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                      // the previous piece has been read by every wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = tid + 256 * i;
      *reinterpret_cast<bf16x8_t*>(&Ws[(p >> 2) * HS_LD + (p & 3) * 8]) = wr[i];
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int p = tid + 256 * i;
      if (p < BR * 4) *reinterpret_cast<bf16x8_t*>(&Xs[(p >> 2) * HS_LD + (p & 3) * 8]) = xr[i];
    }
    __syncthreads();
    if (kt + 1 < nk) {                                    // the next piece travels under this piece's MFMAs
      const int ko = (kt + 1) * HS_BK;
#pragma unroll
      for (int i = 0; i < 4; ++i) wr[i] = *reinterpret_cast<const bf16x8_t*>(wp[i] + ko);
#pragma unroll
      for (int i = 0; i < XI; ++i) xr[i] = *reinterpret_cast<const bf16x8_t*>(xp[i] + ko);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {                      // k ascending, one accumulator per output: the order does not know R
      bf16x8_t a[2], b[NT];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const bf16x8_t*>(&Ws[(wave * 64 + m * 32 + r32) * HS_LD + kk * 16 + h * 8]);
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = *reinterpret_cast<const bf16x8_t*>(&Xs[(n * 32 + r32) * HS_LD + kk * 16 + h * 8]);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
    }
  }

  // ---- epilogue.  Accumulator (m, n) register j of this lane: table entry v0 + 64 wave + 32 m + (j & 3) + 8 (j >> 2) + 4 h, hidden
  // row row0 + 32 n + r32.  Pass 1: round to bf16, the label's logit, the maximum and its first index.
  const int ebase = v0 + wave * 64 + 4 * h;
  float Mn[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int xl = n * 32 + r32, row = row0 + xl;
    int lab_e = -1;                                       // the label as a table entry, -1: none in this tile for this row
    if (row < R) {
      const int64_t lab = labels[row];
      if (lab != ignore_index && lab >= v0 && lab < (int64_t)V && lab < (int64_t)v0 + HS_BV) lab_e = (int)lab;
    }
    float mx = -INFINITY;
    int mi = INT_MAX;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int e = ebase + m * 32 + (j & 3) + 8 * (j >> 2);
        const float s = bf2f(f2bf(acc[m][n][j]));
        acc[m][n][j] = s;
        if (e < V) {
          if (s > mx) { mx = s; mi = e; }                 // e ascends with (m, j): a tie keeps the lower index
          if (e == lab_e) lab_logit[row] = s;             // the one tile, the one lane that holds the label
        }
      }
    const float om = __shfl_xor(mx, 32, 64);
    const int oi = __shfl_xor(mi, 32, 64);
    if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
    if (h == 0) { red_m[wave][xl] = mx; red_i[wave][xl] = mi; }
  }
  __syncthreads();
  // Pass 2: sum exp(s - tile maximum), registers in order, then the other half, then (below) waves 0..3.
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int xl = n * 32 + r32;
    float M = red_m[0][xl];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, red_m[w][xl]);
    Mn[n] = M;
    float sm = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int e = ebase + m * 32 + (j & 3) + 8 * (j >> 2);
        if (e < V) sm += expf(acc[m][n][j] - M);
      }
    sm += __shfl_xor(sm, 32, 64);
    if (h == 0) red_s[wave][xl] = sm;
  }
  __syncthreads();
  if (tid < BR && row0 + tid < R) {
    float M = red_m[0][tid];
    int I = red_i[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (red_m[w][tid] > M) { M = red_m[w][tid]; I = red_i[w][tid]; }   // waves hold ascending entries: strict keeps the first
    const float S = ((red_s[0][tid] + red_s[1][tid]) + red_s[2][tid]) + red_s[3][tid];
    part[(int64_t)ct * R + row0 + tid] = make_float4(M, S, __int_as_float(I), 0.f);
  }
}

// 4 rows per workgroup, 64 threads per row: thread c walks tiles [c cs, (c + 1) cs) in order, the 64 chunk results are merged in
// chunk order.  Maximum and first index first (exact in any order), then the sum rescaled to the row's maximum in fp64.
__global__ __launch_bounds__(256) void head_score_finish_kernel(const float4* __restrict__ part, const float* __restrict__ lab_logit,
                                                                const int64_t* __restrict__ labels, int64_t ignore_index, int R, int V,
                                                                int T, float* __restrict__ logp, float* __restrict__ lse,
                                                                int64_t* __restrict__ best, float* __restrict__ best_logit) {
  __shared__ float sm[ug_plan::HS_FINISH_ROWS][64];
  __shared__ int si[ug_plan::HS_FINISH_ROWS][64];
  __shared__ double ss[ug_plan::HS_FINISH_ROWS][64];
  const int rl = threadIdx.x & 3, c = threadIdx.x >> 2;
  const int64_t row = (int64_t)blockIdx.x * ug_plan::HS_FINISH_ROWS + rl;
  const bool live = row < R;
  const int cs = (T + 63) / 64, t0 = min(T, c * cs), t1 = min(T, t0 + cs);
  float m = -INFINITY;
  int mi = INT_MAX;
  if (live)
    for (int t = t0; t < t1; ++t) {
      const float4 p = part[(int64_t)t * R + row];
      if (p.x > m) { m = p.x; mi = __float_as_int(p.z); }
    }
  sm[rl][c] = m;
  si[rl][c] = mi;
  __syncthreads();
  float M = sm[rl][0];
  int I = si[rl][0];
  for (int j = 1; j < 64; ++j)
    if (sm[rl][j] > M) { M = sm[rl][j]; I = si[rl][j]; }
  double s = 0.0;
  if (live)
    for (int t = t0; t < t1; ++t) {
      const float4 p = part[(int64_t)t * R + row];
      s += (double)p.y * exp((double)p.x - (double)M);
    }
  ss[rl][c] = s;
  __syncthreads();
  if (c == 0 && live) {
    double S = 0.0;
    for (int j = 0; j < 64; ++j) S += ss[rl][j];
    const float l = (float)((double)M + log(S));
    const int64_t lab = labels[row];
    logp[row] = (lab != ignore_index && lab >= 0 && lab < (int64_t)V) ? lab_logit[row] - l : 0.f;
    if (lse) lse[row] = l;
    if (best) best[row] = I;
    if (best_logit) best_logit[row] = M;
  }
}

int head_score_shape_ok(const char* who, int64_t R, int64_t V) {
  UG_REQUIRE(R >= 1 && V >= 1, "%s: need R >= 1 and V >= 1 (R=%ld V=%ld)", who, (long)R, (long)V);
  UG_REQUIRE(R <= INT_MAX - 128 && V <= INT_MAX - HS_BV, "%s: R and V must fit 32-bit indices (R=%ld V=%ld)", who, (long)R, (long)V);
  const ug_plan::HeadScorePlan pl = ug_plan::plan_head_score(R, V);
  UG_REQUIRE(pl.grid <= INT_MAX && pl.ws_bytes <= INT_MAX, "%s: R x column tiles too large for one call (R=%ld V=%ld): split the rows",
             who, (long)R, (long)V);
  return UG_OK;
}

}  // namespace

extern "C" int ug_head_score_ws_bytes(int64_t R, int64_t V) {
  const int rc = head_score_shape_ok("ug_head_score_ws_bytes", R, V);
  if (rc != UG_OK) return rc;
  return (int)ug_plan::plan_head_score(R, V).ws_bytes;
}

extern "C" int ug_head_score(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, int64_t V, int64_t K,
                             const int64_t* labels, int64_t ignore_index, void* ws, float* logp, float* lse, int64_t* best,
                             float* best_logit, hipStream_t st) {
  const int rc = head_score_shape_ok("ug_head_score", R, V);
  if (rc != UG_OK) return rc;
  UG_REQUIRE(K >= HS_BK && K % HS_BK == 0 && K <= INT_MAX, "ug_head_score: K must be a positive multiple of 32 (K=%ld)", (long)K);
  UG_REQUIRE(ldx >= K && ldx % 8 == 0, "ug_head_score: need ldx >= K and ldx %% 8 == 0 (ldx=%ld K=%ld)", (long)ldx, (long)K);
  UG_REQUIRE(ldw >= K && ldw % 8 == 0, "ug_head_score: need ldw >= K and ldw %% 8 == 0 (ldw=%ld K=%ld)", (long)ldw, (long)K);
  UG_REQUIRE(x && W, "ug_head_score: x and W must not be null");
  UG_REQUIRE(labels, "ug_head_score: labels must not be null");
  UG_REQUIRE(ws, "ug_head_score: ws must not be null (ug_head_score_ws_bytes(R, V) bytes)");
  UG_REQUIRE(logp, "ug_head_score: logp must not be null");
  UG_REQUIRE(ug_aligned16(x) && ug_aligned16(W) && ug_aligned16(ws), "ug_head_score: x, W and ws must be 16B aligned");
  const ug_plan::HeadScorePlan pl = ug_plan::plan_head_score(R, V);
  float4* part = reinterpret_cast<float4*>(ws);
  float* lab_logit = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + pl.label_off);
#define UG_HS_LAUNCH(NT)                                                                                                       \
  hipLaunchKernelGGL(head_score_kernel<NT>, dim3((unsigned)pl.grid), dim3(ug_plan::HS_BLOCK), 0, st, (const bf16_t*)x, ldx, (int)R, \
                     (const bf16_t*)W, ldw, (int)V, (int)K, labels, ignore_index, part, lab_logit, (int)pl.row_tiles)
  if (pl.br == 32) { UG_HS_LAUNCH(1); }
  else { UG_HS_LAUNCH(2); }
#undef UG_HS_LAUNCH
  UG_CHECK_LAUNCH("ug_head_score");
  hipLaunchKernelGGL(head_score_finish_kernel, dim3((unsigned)pl.finish_grid), dim3(256), 0, st, part, lab_logit, labels, ignore_index,
                     (int)R, (int)V, (int)pl.col_tiles, logp, lse, best, best_logit);
  UG_CHECK_LAUNCH("ug_head_score(finish)");
  return UG_OK;
}
