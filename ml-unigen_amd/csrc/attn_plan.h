// Which attention kernels a training / prefill problem runs, as pure functions: plain C++17, no HIP, no globals, no environment, no
// pointer is dereferenced.  attention.hip fills AttnArgs, asks plan_attn_fwd / plan_attn_bwd, and launches what the plan says;
// tests/attn_plan_dump.cpp compiles this header alone for the host and tests/test_attn_plan_cpu.py holds its answers against
// tests/golden/attn_plan.json.  Every threshold below is a measurement (docs/experiments.md records each A/B): an edit that changes a
// row of that table changes which kernel a layer of the training step runs.
#pragma once
#include <cstdint>

namespace ug_plan {

// The settled A/B choices (run-time switches until each was measured and decided, docs/experiments.md; probe builds override them
// with -D, tools/probes/probe_switches.patch).
constexpr bool ATTN_FWD32 = true;           // 32-row forward kernel (attn_fwd32_kernel) where it applies
constexpr bool ATTN_DQ32 = true;            // 32-row dQ kernel (attn_bwd_dq32_kernel) where it applies
constexpr bool ATTN_BWD_FUSE_ROPE = true;   // RoPE / dbias in the 32-row dQ kernel's stores and in the dK/dV finish
constexpr bool ATTN_DKV_DMA = true;         // attn_bwd_dkv_dma_kernel for the split-head dK/dV up to L = 4096
// two query heads per dK/dV workgroup once that still leaves 1 024 workgroups: fused backward 282 -> 271 us per layer causal,
// 404 -> 391 full (three heads per workgroup 273, six 311: too few workgroups)
constexpr int ATTN_DKV_HEADS = 2, ATTN_DKV_MIN_WGS = 1024;
constexpr int ATTN_FINISH_WGS = 128;        // workgroups of dkv_finish_rope_kernel (measurement at its use in plan_attn_bwd)
// AttnArgs::order per launch (wg_coord: 0 pair by pair, 1 tile rank first over all pairs): global for the forward, pair-major for
// dQ and dK/dV.  Measured at 16 x 771 tokens, us per layer: forward 116 vs 128 on the full mask for global vs pair-major; fused
// backward 255 pair-major, 272 global.
constexpr int ATTN_ORDER_FWD = 1, ATTN_ORDER_DQ = 0, ATTN_ORDER_DKV = 0;

// 1-D grid of 8 * ceil(pairs / 8) * nT * G workgroups (wg_coord in attention.hip: every workgroup of one (batch, kv head) pair on
// ONE XCD); surplus ones exit.
inline unsigned wg_grid(int64_t nT, int H, int HKV, int64_t B) {
  const int64_t P = B * HKV;
  return (unsigned)(8 * ((P + 7) / 8) * nT * (H / HKV));
}

// ---------------------------------------------------------------------------------------------- ug_attn_fwd
enum AttnFwdKernel { ATTN_FWD32_4 = 0, ATTN_FWD_8 = 1, ATTN_FWD_4 = 2 };     // attn_fwd32_kernel<4>, attn_fwd_kernel<8>, attn_fwd_kernel<4>

struct AttnFwdPlan {
  AttnFwdKernel kernel = ATTN_FWD_4;
  unsigned grid = 0;
  int block = 256;
  int order = ATTN_ORDER_FWD;          // AttnArgs::order
};

inline AttnFwdPlan plan_attn_fwd(int64_t B, int64_t L, int H, int HKV) {
  AttnFwdPlan pl;
  const int64_t nW = (L + 63) / 64;
  // 128-row query tiles (eight waves share each staged K / V tile) once there are enough of them to fill the chip
  if (ATTN_FWD32 && L >= 256 && L <= 4096 && (int64_t)((L + 127) / 128) * H * B >= 512) {
    pl.kernel = ATTN_FWD32_4; pl.grid = wg_grid((L + 127) / 128, H, HKV, B);
  } else if (L >= 256 && (int64_t)((L + 127) / 128) * H * B >= 512) {
    pl.kernel = ATTN_FWD_8; pl.grid = wg_grid((L + 127) / 128, H, HKV, B); pl.block = 512;
  } else {
    pl.kernel = ATTN_FWD_4; pl.grid = wg_grid(nW, H, HKV, B);
  }
  return pl;
}

// ---------------------------------------------------------------------------------------------- ug_attn_bwd
enum AttnDqKernel { ATTN_DQ32_4 = 0, ATTN_DQ = 1 };                           // attn_bwd_dq32_kernel<4>, attn_bwd_dq_kernel
enum AttnDkvKernel { ATTN_DKV_DMA_SPLIT = 0, ATTN_DKV_SPLIT = 1, ATTN_DKV_WHOLE = 2 };   // attn_bwd_dkv_dma_kernel, attn_bwd_dkv_kernel<true>, <false>
enum AttnFinish { ATTN_FINISH_NONE = 0, ATTN_FINISH_ROPE = 1, ATTN_FINISH_PLAIN = 2 };    // none, dkv_finish_rope_kernel, dkv_finish_kernel

struct AttnBwdPlan {
  AttnDqKernel dq = ATTN_DQ;
  unsigned dq_grid = 0;
  int dq_order = ATTN_ORDER_DQ;
  bool dq_fused = false;               // AttnArgs::rope_cos / rope_sin / dbias are set for the dQ launch: RoPE and dbias ride in its stores
  AttnDkvKernel dkv = ATTN_DKV_WHOLE;
  int dkv_heads = 0;                   // AttnArgs::dkv_heads (the split-head kernels: 1 or 2; 0 = unwritten for the one that does not read it)
  unsigned dkv_grid = 0;
  int dkv_order = ATTN_ORDER_DKV;
  AttnFinish finish = ATTN_FINISH_NONE;
  int rpb = 0;                         // ATTN_FINISH_ROPE: token rows per workgroup
  unsigned finish_grid = 0;
  // what the fused stores do not cover is done by the stand-alone passes (same arithmetic): ug_rope / ug_colsum_bf16
  bool rope_dq = false, colsum_dq = false, rope_dk = false, colsum_dk = false, colsum_dv = false;
};

inline AttnBwdPlan plan_attn_bwd(int64_t B, int64_t L, int H, int HKV, bool has_dkv_ws, bool has_rope, bool has_dbias) {
  AttnBwdPlan pl;
  const int64_t nW = (L + 63) / 64;
  const int64_t tokens = B * L;
  if (ATTN_DQ32 && L >= 256 && L <= 4096 && (int64_t)((L + 127) / 128) * H * B >= 512) {
    pl.dq = ATTN_DQ32_4; pl.dq_grid = wg_grid((L + 127) / 128, H, HKV, B);
    pl.dq_fused = ATTN_BWD_FUSE_ROPE;
  } else {
    pl.dq = ATTN_DQ; pl.dq_grid = wg_grid(nW, H, HKV, B);
  }
  pl.rope_dq = has_rope && !pl.dq_fused; pl.colsum_dq = has_dbias && !pl.dq_fused;
  if (has_dkv_ws) {
    pl.dkv_heads = (ATTN_DKV_HEADS >= 1 && (H / HKV) % ATTN_DKV_HEADS == 0 && (int64_t)nW * (H / ATTN_DKV_HEADS) * B >= ATTN_DKV_MIN_WGS) ? ATTN_DKV_HEADS : 1;
    if (ATTN_DKV_DMA && L <= 4096) { pl.dkv = ATTN_DKV_DMA_SPLIT; pl.dkv_grid = wg_grid(nW, H / pl.dkv_heads, HKV, B); }
    else { pl.dkv = ATTN_DKV_SPLIT; pl.dkv_grid = wg_grid(nW, H, HKV, B); }
    if (ATTN_BWD_FUSE_ROPE && (has_rope || has_dbias) && HKV <= 16 && (HKV & (HKV - 1)) == 0) {
      // ~128 workgroups: every workgroup ends with one atomic per bias column (512 addresses), and 1 000 same-address atomics
      // in a burst cost more (53 us measured) than the whole streaming pass (9 us)
      pl.finish = ATTN_FINISH_ROPE;
      pl.rpb = (int)((tokens + ATTN_FINISH_WGS - 1) / ATTN_FINISH_WGS < 8 ? 8 : (tokens + ATTN_FINISH_WGS - 1) / ATTN_FINISH_WGS);
      pl.finish_grid = (unsigned)((tokens + pl.rpb - 1) / pl.rpb);
      return pl;
    }
    const int64_t total = B * L * (2 * HKV * 128 / 4);
    int64_t gsz = (total + 255) / 256; if (gsz > 4096) gsz = 4096;
    pl.finish = ATTN_FINISH_PLAIN; pl.finish_grid = (unsigned)gsz;
  } else {
    pl.dkv = ATTN_DKV_WHOLE; pl.dkv_grid = wg_grid(nW, HKV, HKV, B);
  }
  pl.rope_dk = has_rope; pl.colsum_dk = pl.colsum_dv = has_dbias;
  return pl;
}

}  // namespace ug_plan
