// Prompt-lookup speculative decoding, the token side (contract: include/unigen_hip.h, ug_spec_verify; the rules: spec_plan.h): behind
// the head of a verify step over S consecutive positions of ONE sequence, two launches --
//   spec_argmax_kernel   one workgroup per row: g[s] = the lowest index attaining the maximum of the bf16-rounded logits (ug_text_pick's
//                        pick), left in the state block; clear != 0 zeroes the row on the way
//   spec_finish_kernel   one workgroup: accept, emit (stop rule, width), the history, the cache position, the next draft by a search of
//                        the history with all threads, the next step's tokens and their embedding rows
// Plain HIP C++: no inline assembly, no atomics.  No host synchronisation, no shape depends on the step: capturable.
#include "common.h"
#include "spec_plan.h"
#include "unigen_hip.h"

namespace {

using namespace ug_plan;
static_assert(SPEC_MAX_ROWS == UG_SPEC_MAX_ROWS, "spec_plan.h and unigen_hip.h state the same row limit");

constexpr int SPA_T = 1024;
constexpr int SPA_W = SPA_T / 64;
constexpr int SPF_T = 256;
constexpr int SPF_W = SPF_T / 64;

template <bool VEC>
__global__ __launch_bounds__(SPA_T) void spec_argmax_kernel(float* __restrict__ logits, int64_t ld, int V, int clear, int* __restrict__ state) {
  __shared__ float red[SPA_W];
  __shared__ int best_i[SPA_W];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* row = logits + (int64_t)r * ld;
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  if (VEC) {
    float4* row4 = reinterpret_cast<float4*>(row);
    const int n4 = (V + 3) >> 2;                                  // (ld is a multiple of 4: the last vector stays inside the row)
    for (int i = t; i < n4; i += SPA_T) {                         // ascending indices per thread: `>` keeps the lowest
      const float4 q = row4[i];
      const float vv[4] = {q.x, q.y, q.z, q.w};
      const int e0 = 4 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = bf2f(f2bf(vv[j]));
        if (e0 + j < V && v > mx) { mx = v; arg = e0 + j; }       // (entries V .. ld-1 are read, never candidates)
      }
      if (clear) {
        if (e0 + 3 < V) row4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else
          for (int j = 0; e0 + j < V; ++j) row[e0 + j] = 0.f;    // nothing is written past the V read entries
      }
    }
  } else {
    for (int e = t; e < V; e += SPA_T) {
      const float v = bf2f(f2bf(row[e]));
      if (v > mx) { mx = v; arg = e; }
      if (clear) row[e] = 0.f;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mx, off, 64);
    const int oi = __shfl_xor(arg, off, 64);
    if (om > mx || (om == mx && oi < arg)) { mx = om; arg = oi; }
  }
  if (lane == 0) { red[wave] = mx; best_i[wave] = arg; }
  __syncthreads();
  if (t == 0) {
    float bmx = red[0];
    int bi = best_i[0];
    for (int w = 1; w < SPA_W; ++w)
      if (red[w] > bmx || (red[w] == bmx && best_i[w] < bi)) { bmx = red[w]; bi = best_i[w]; }
    state[SPEC_PICK + r] = bi >= V ? 0 : bi;                      // (no finite candidate: torch.argmax answers 0 for a row of -inf)
  }
}

struct SpecArgs {
  const int64_t* stop_ids;
  int n_stop;
  const float* embed;
  int64_t lde;
  int embed_rows, H;
  int* state;
  int width, rows, next_rows;
  int64_t* tok;
  int* out_tokens;
  int* lengths;
  int* hist;
  int hist_cap, ngram, num_draft;
  int* pos;
  int* len;
  float* x;
};

__global__ __launch_bounds__(SPF_T) void spec_finish_kernel(SpecArgs o) {
  __shared__ int s_go, s_n, s_last;
  __shared__ int s_first[SPF_W][SPEC_MAX_NGRAM];
  __shared__ int s_tok[SPEC_MAX_ROWS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int* st = o.state;
  if (t == 0) {
    s_go = 0;
    if (!st[SPEC_DONE]) {
      int g[SPEC_MAX_ROWS];
      for (int s = 0; s < o.rows; ++s) g[s] = st[SPEC_PICK + s];
      int nd = st[SPEC_NDRAFT];
      nd = nd < 0 ? 0 : nd > o.rows - 1 ? o.rows - 1 : nd;
      const int a = spec_accept(g, o.tok, nd);
      const int emitted = st[SPEC_EMITTED];
      const SpecEmit e = spec_emit(g, a, o.stop_ids, o.n_stop, emitted, o.width);
      int n = st[SPEC_HIST_LEN];
      for (int i = 0; i < e.n; ++i) {
        o.out_tokens[emitted + i] = g[i];
        if (n < o.hist_cap) o.hist[n++] = g[i];
      }
      st[SPEC_EMITTED] = emitted + e.n;
      st[SPEC_HIST_LEN] = n;
      if (o.pos) {                                                // a decoder step: rows 0 .. a of it now stand in the cache for good
        st[SPEC_STEPS] += 1;
        st[SPEC_DRAFTED] += nd;
        st[SPEC_ACCEPTED] += a;
        const int p = *o.pos + e.n;
        *o.pos = p;
        *o.len = p + 1;
      }
      if (e.done) {
        st[SPEC_DONE] = 1;
        if (o.lengths) o.lengths[0] = emitted + e.n;
      }
      s_go = !e.done && e.n > 0;
      s_n = n;
      s_last = e.n > 0 ? g[e.n - 1] : 0;
    }
  }
  __syncthreads();
  if (!s_go) return;                                              // finished (now or before): tok, x and the draft stay as they are
  const int n = s_n;
  // the earliest earlier occurrence of the last g ids, for every g at once: thread t looks at i = t, t + T, ...
  int first[SPEC_MAX_NGRAM];
#pragma unroll
  for (int g = 0; g < SPEC_MAX_NGRAM; ++g) first[g] = SPEC_NO_MATCH;
  if (o.num_draft > 0) {
    for (int i = t; i + 1 < n; i += SPF_T) {
#pragma unroll
      for (int g = 1; g <= SPEC_MAX_NGRAM; ++g)
        if (g <= o.ngram && first[g - 1] == SPEC_NO_MATCH && spec_match_at(o.hist, n, i, g)) first[g - 1] = i;
    }
  }
#pragma unroll
  for (int g = 0; g < SPEC_MAX_NGRAM; ++g) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first[g] = min(first[g], __shfl_xor(first[g], off, 64));
    if (lane == 0) s_first[wave][g] = first[g];
  }
  __syncthreads();
  if (t == 0) {
    int f[SPEC_MAX_NGRAM];
    for (int g = 0; g < SPEC_MAX_NGRAM; ++g) {
      f[g] = s_first[0][g];
      for (int w = 1; w < SPF_W; ++w) f[g] = min(f[g], s_first[w][g]);
    }
    SpecDraft d = {0, 0, 0};
    if (o.num_draft > 0) d = spec_draft_from(f, n, o.ngram, o.num_draft);
    st[SPEC_NDRAFT] = d.len;
    int last = s_last;
    last = last < 0 ? 0 : last >= o.embed_rows ? o.embed_rows - 1 : last;
    s_tok[0] = last;
    for (int s = 1; s < o.next_rows; ++s) {
      if (s <= d.len) {
        const int id = o.hist[d.start + s - 1];
        last = id < 0 ? 0 : id >= o.embed_rows ? o.embed_rows - 1 : id;      // (the host checked the ids; a table row in any case)
      }
      s_tok[s] = last;                                            // rows behind the draft repeat the last valid one: padding, finite
    }
    for (int s = 0; s < o.next_rows; ++s) o.tok[s] = s_tok[s];
  }
  __syncthreads();
  const int h4 = o.H >> 2;
  for (int i = t; i < o.next_rows * h4; i += SPF_T) {
    const int s = i / h4, c = i - s * h4;
    reinterpret_cast<float4*>(o.x + (int64_t)s * o.H)[c] = reinterpret_cast<const float4*>(o.embed + (int64_t)s_tok[s] * o.lde)[c];
  }
}

}  // namespace

extern "C" int ug_spec_verify(float* logits, int64_t ld, int64_t rows, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop,
                              const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t width, int64_t* tok,
                              int64_t next_rows, int* out_tokens, int* lengths, int* hist, int64_t hist_cap, int64_t ngram,
                              int64_t num_draft, int* pos, int* len, float* x, hipStream_t st) {
  UG_REQUIRE(logits && embed && state && tok && out_tokens && hist && x && (n_stop == 0 || stop_ids), "ug_spec_verify: null argument");
  UG_REQUIRE((pos == nullptr) == (len == nullptr), "ug_spec_verify: pos and len come together (both null: the first token, no advance)");
  UG_REQUIRE(rows >= 1 && rows <= SPEC_MAX_ROWS && next_rows >= 1 && next_rows <= SPEC_MAX_ROWS && V > 0 && ld >= V &&
                 rows * ld < (1ll << 31) && width > 0 && width < (1ll << 31) && n_stop >= 0 && n_stop <= SPEC_MAX_STOP,
             "ug_spec_verify: bad sizes (rows=%ld, next_rows=%ld in 1 .. %d, V=%ld <= ld=%ld, rows*ld < 2^31, width=%ld, n_stop=%ld <= %d)",
             (long)rows, (long)next_rows, SPEC_MAX_ROWS, (long)V, (long)ld, (long)width, (long)n_stop, SPEC_MAX_STOP);
  UG_REQUIRE(num_draft >= 0 && num_draft < next_rows && ngram >= 1 && ngram <= SPEC_MAX_NGRAM && hist_cap > 0 && hist_cap < (1ll << 31),
             "ug_spec_verify: bad draft (num_draft=%ld below next_rows=%ld, ngram=%ld in 1 .. %d, hist_cap=%ld)", (long)num_draft,
             (long)next_rows, (long)ngram, SPEC_MAX_NGRAM, (long)hist_cap);
  UG_REQUIRE(H > 0 && H % 4 == 0 && H < (1 << 24) && ld_embed % 4 == 0 && ld_embed >= H && embed_rows >= V && embed_rows < (1ll << 31) &&
                 ug_aligned16(embed) && ug_aligned16(x),
             "ug_spec_verify: bad table (H=%ld, ld_embed=%ld, rows=%ld >= V; 16-byte aligned table / x)", (long)H, (long)ld_embed,
             (long)embed_rows);
  if (ld % 4 == 0 && ug_aligned16(logits))
    hipLaunchKernelGGL((spec_argmax_kernel<true>), dim3((unsigned)rows), dim3(SPA_T), 0, st, logits, ld, (int)V, clear, state);
  else
    hipLaunchKernelGGL((spec_argmax_kernel<false>), dim3((unsigned)rows), dim3(SPA_T), 0, st, logits, ld, (int)V, clear, state);
  UG_CHECK_LAUNCH("ug_spec_verify");
  const SpecArgs o{stop_ids, (int)n_stop, embed, ld_embed, (int)embed_rows, (int)H, state, (int)width, (int)rows, (int)next_rows, tok,
                   out_tokens, lengths, hist, (int)hist_cap, (int)ngram, (int)num_draft, pos, len, x};
  hipLaunchKernelGGL(spec_finish_kernel, dim3(1), dim3(SPF_T), 0, st, o);
  UG_CHECK_LAUNCH("ug_spec_verify");
  return UG_OK;
}
