// Device pieces that decode.hip and decode_sw.hip both use: one definition for the two files.
#pragma once
#include "common.h"

// workgroup barrier for an LDS hand-off: __syncthreads() also drains vmcnt (its fence covers global memory), i.e. waits for the
// weight tiles in flight and the clears' write acknowledgements, which no wave needs at this point
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// bf16(silu(g)) of the decode SwiGLU forms: act = bf16( bf16(silu(bf16 gate)) * bf16 up )  (Qwen2MLP.forward under bf16 autocast)
__device__ __forceinline__ float silu_bf(float g) { return bf2f(f2bf(g / (1.f + __expf(-g)))); }

// The clears a launch carries: up to two accumulators that earlier kernels have fully consumed and one 32-float statistics slot, spread
// over all workgroups (bid = linear workgroup id, nt = threads per workgroup), so the captured graph carries no memset nodes.
// A = DecodeIn (decode.hip) or SwArgs (decode_sw.hip): zero0 / zero1 / ss_zero, their float4 counts n0_4 / n1_4 and every workgroup's
// share per0 / per1.  Everything uniform is 32-bit and comes from the host (ug_plan::clear_shares): dividing int64 counts by the grid
// size in every workgroup cost ~150 dependent scalar instructions per division AHEAD of the kernel's first load
// (profiles/r05_ar_prefetch.md, section 3).
template <class A>
__device__ __forceinline__ void decode_clear(const A& f, int tid, int bid, int nt) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f.zero0) {
    const int lo = bid * f.per0, hi = min(f.n0_4, lo + f.per0);
    for (int i = lo + tid; i < hi; i += nt) reinterpret_cast<float4*>(f.zero0)[i] = z;
  }
  if (f.zero1) {
    const int lo = bid * f.per1, hi = min(f.n1_4, lo + f.per1);
    for (int i = lo + tid; i < hi; i += nt) reinterpret_cast<float4*>(f.zero1)[i] = z;
  }
  if (f.ss_zero && bid == 0 && tid < 32) f.ss_zero[tid] = 0.f;
}
