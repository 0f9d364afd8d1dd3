/* unigen_hip.h -- C ABI of libunigen_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary underneath the reference's Python model API:
 * the reference itself has no native code, every entry point below replaces a third-party kernel
 * the reference reaches through torch / transformers.  The "replaces" note on each entry cites the
 * reference call site (paths relative to the reference repo) whose arithmetic it implements.
 *
 * Conventions
 *   - plain C types only: device pointers, int64 sizes / strides (in ELEMENTS), float scalars,
 *     a hipStream_t.  No torch types.  bf16 tensors are passed as void* (raw 16-bit storage).
 *   - every function returns 0 on success or a negative error class (UG_ERR_*); the message is
 *     available from ug_last_error() (thread-local).  Nothing throws or aborts across the boundary.
 *   - every tensor is owned by the caller; the library never frees caller memory, allocates only one lazily
 *     created device scratch (k-sliced GEMM partials), never synchronises the device, and launches only on the
 *     stream it is given (so every entry is
 *     legal inside a hipGraph capture).
 *   - shape / alignment requirements are checked at entry and fail loudly (UG_ERR_ARG).
 */
#ifndef UNIGEN_HIP_H
#define UNIGEN_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UG_ABI_VERSION 7

/* ---- library ---------------------------------------------------------------------------- */
const char* ug_last_error(void);
int ug_abi_version(void);

/* ---- handle ----------------------------------------------------------------------------------
 * The library's only allocation: an opaque per-stream workspace (192 MiB of device scratch for k-sliced GEMM partials).
 * ug_create may allocate and must be called outside stream capture; no op entry point allocates, frees, clears or
 * synchronises, so every op is legal inside a hipGraph capture.  One handle per concurrently used stream (SURVEY 8b:
 * "allocates only an opaque workspace/handle created by ug_create() / released by ug_destroy()"). */
typedef struct ug_handle ug_handle;
int ug_create(ug_handle** out);
int ug_destroy(ug_handle* h);

/* ---- dense contraction ------------------------------------------------------------------- */
/* C[M,N] = opA . opB^T, bf16 operands, fp32 accumulate.  Each operand is given either row-major
 * (k contiguous: A[M][K] lda, B[N][K] ldb) or k-major (A[K][M] lda, B[K][N] ldb; a_kmajor/b_kmajor = 1),
 * so forward (0,0), dgrad (0,1: B = W[N_out][K_in]) and wgrad (1,1: contraction over tokens) need no
 * transposed copies.  K is the true contraction length (no padding; see gemm_bf16.hip for the K%8 rule).
 * epilogue: 0 = bf16 out (+ optional bf16 bias[N])
 *           1 = fp32 out, C = (beta ? C : 0) + alpha * acc   (alpha read from device if non-null)
 *           2 = fp32 residual: C = resid + bf16round(acc)
 * replaces: nn.Linear inside transformers Qwen2Attention / Qwen2MLP (q,k,v,o,gate,up,down_proj) and
 *           UniGen's tied lm_head, models/unigen.py:274-287; their autograd dgrad / wgrad. */
#define UG_EPI_BF16 0
#define UG_EPI_F32 1
#define UG_EPI_RESID 2
int ug_gemm_bf16(const ug_handle* h, const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor,
                 void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, const void* bias,
                 const float* resid, int64_t ldr, int beta, const float* alpha_dev, int policy, hipStream_t stream);
/* h: the calling stream's handle (ug_create) or null.  The handle owns the fp32 scratch of the k-sliced launch forms
 * (partial last round of 256x256 tiles, small weight gradients, lm-head dgrad); without one those forms are not chosen.
 * One handle must not be used by two streams at once; any number of handles may run concurrently.
 * policy: (the rules themselves: ml-unigen_amd/csrc/gemm_plan.h, plan_gemm / decode_policy) -1 = automatic kernel selection (the product path); >= 0 pins a kernel for A/B benchmarks and tests:
 * 0 = 128x128 two LDS stages, 2 = 128x128 one LDS stage, 3 = staggered 256x256, 6 = 256x256 with the k-sliced tail forced,
 * 8 = k-sliced small outputs, 10 = 320x256 tiles (A row-major, N % 256 == 0, K % 32 == 0, bf16 / residual epilogue; other
 * launches ignore it), 44 ... 52 except 48 = the same kernel at a tile height of 16 * (policy - 32) = 192 ... 320 rows; UG_GEMM_POLICY_AUTO_BITS = automatic selection when only modifier bits are wanted;
 * | UG_GEMM_NARROW_EPILOGUE = element-wise instead of LDS-transposed 16-byte stores in the 256x256 kernel. */
#define UG_GEMM_NARROW_EPILOGUE 0x100
#define UG_GEMM_ONE_BARRIER 0x200     /* force the 256x256 kernel's one-barrier-per-k-tile main loop (default: weight gradients, both operands k-major) */
#define UG_GEMM_TWO_BARRIERS 0x400    /* force its two-barrier (L | M phase) main loop (default: forward and dgrad) */
#define UG_GEMM_POLICY_AUTO_BITS 0xff

int ug_cast_f32_bf16(const float* in, void* out, int64_t n, hipStream_t stream);

/* The down projection's dgrad with the SwiGLU backward in its epilogue (autograd of Qwen2MLP.forward, modeling_qwen2.py:46-48, under bf16
 * autocast; reference call site models/unigen.py:274-285 through loss.backward(), training/train.py:775): dgu[M, 2I] = d(gate | up) from
 * dy[M, K] (gradient of the down projection's output), W_down stored [K, I] (row stride ldw) and the forward's gu[M, 2I] -- the values of
 * ug_gemm_bf16 (B k-major) followed by ug_swiglu_bwd, bit for bit; d(act) never reaches HBM.  Needs I % 256 == 0, K % 32 == 0 and 16-byte
 * aligned rows; other shapes are refused (UG_ERR_ARG) and run as those two launches.  ABI v5. */
int ug_gemm_bf16_swiglu_bwd(const ug_handle* h, const void* dy, int64_t ld_dy, const void* w_down, int64_t ldw, const void* gu,
                            int64_t ld_gu, void* dgu, int64_t ld_dgu, int64_t M, int64_t I, int64_t K, hipStream_t stream);
/* Tile height of the three fused-epilogue launches above (128 ... 320 rows in steps of 16; 0 = automatic, the default): tests and
 * A/B runs force every instantiated height this way; a height the called entry point does not instantiate is refused (UG_ERR_ARG).
 * Process-wide.  ABI v6. */
int ug_gemm_set_fused_tile_height(int rows);
/* The fused q/k/v projection of a decoder layer (transformers modeling_qwen2.py:200-215 q_proj / k_proj / v_proj + apply_rotary_pos_emb
 * :131-135; reference call site models/unigen.py:274-285): qkv[M, N] = bf16(x[M, K] W[N, K]^T + bias) with rotate-half RoPE (tables
 * [L, head_dim / 2] fp32, row m at position m % L) applied in the GEMM's epilogue to the first rope_cols columns (the q and k heads) --
 * bit-identical to ug_gemm_bf16 followed by ug_rope.  Fused for head_dim 128, N / rope_cols / K multiples of 256 / 256 / 32; any other
 * shape runs as those two launches.  ABI v5. */
int ug_gemm_bf16_qkv_rope(const ug_handle* h, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* qkv,
                          int64_t ldq, int64_t M, int64_t N, int64_t K, const float* cos_tab, const float* sin_tab, int64_t L,
                          int64_t rope_cols, int head_dim, hipStream_t stream);
/* replaces: down_proj's input act_fn(gate_proj(x)) * up_proj(x) in Qwen2MLP.forward (modeling_qwen2.py:46-48) as ONE launch:
 * the gate_up projection of x [M, K] with the fused weight w_gate_up [2I, K] (gate rows, then up rows) whose epilogue also
 * writes act [M, I] = bf16(bf16(silu(gate)) * up).  gu [M, 2I] = [gate | up] is still written (the backward reads it).  A tile
 * of the 256x256 kernel takes 128 gate rows and the same hidden units' 128 up rows of the weight, so both values of a hidden
 * unit meet in one workgroup; values are bit-identical to ug_gemm_bf16 followed by ug_swiglu_fwd, which is also what this
 * entry runs for shapes the 256x256 kernel is not used for (I % 128 != 0 or fewer than 200 tiles). */
int ug_gemm_bf16_swiglu(const ug_handle* h, const void* x, int64_t ldx, const void* w_gate_up, int64_t ldw, void* gu,
                        int64_t ld_gu, void* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, hipStream_t stream);

/* Grouped weight gradients (replaces: the autograd wgrad of the four nn.Linear of a Qwen2DecoderLayer, modeling_qwen2.py:
 * q/k/v_proj fused, o_proj, gate/up_proj fused, down_proj): dw[i][rows_i, cols_i] (= or +=, beta[i]) dy[i]^T x[i] over K[i]
 * tokens, both operands token-major (dy[i]: [K_i][ld_dy_i], x[i]: [K_i][ld_x_i], bf16), fp32 outputs with row stride ld_dw[i].
 * Tiles of one K cost the same, so ONE launch packs the problems into ceil(sum tiles / 256) rounds of the chip (3 for a
 * 1.5B layer at 12 336 tokens; 2 + 1 rounds + two k-sliced launches when issued one by one).  K is per problem (round 4): the
 * host appends a slice of the tied lm_head's weight gradient (models/unigen.py:287, K = the label rows) to every layer's
 * launch, where its short tiles fill the CUs the partial last round leaves idle.  Host arrays of n <= 8 entries. */
int ug_gemm_bf16_wgrad_group(int n, const void* const* dy, const int64_t* ld_dy, const void* const* x, const int64_t* ld_x,
                             float* const* dw, const int64_t* ld_dw, const int64_t* rows, const int64_t* cols,
                             const int* beta, const int64_t* K, hipStream_t stream);

/* ---- Qwen2 decoder-layer row ops ----------------------------------------------------------- */
/* replaces: transformers Qwen2RMSNorm.forward (modeling_qwen2.py:246-252) + the autocast bf16 cast
 * of the following Linear's input.  x fp32 [rows,cols]; y bf16 (or fp32 if out_f32); rstd optional. */
int ug_rmsnorm_fwd(const float* x, const float* w, void* y, float* rstd, int64_t rows, int64_t cols,
                   float eps, int out_f32, hipStream_t stream);
/* dres += d(rmsnorm)/dx . dy ; dw += sum_rows dy * xhat      (dy bf16); dres_bf16 (optional): bf16 copy of the
 * updated dres = the next GEMM's operand, written here instead of by a separate cast pass */
int ug_rmsnorm_bwd(const void* dy, const float* x, const float* rstd, const float* w, float* dres,
                   float* dw, void* dres_bf16, int64_t rows, int64_t cols, hipStream_t stream);
/* replaces: apply_rotary_pos_emb (modeling_qwen2.py:113-135); in place on `nheads` consecutive heads of
 * width head_dim starting at qkv (row stride ldq); position of row t is t % L; cos/sin [L, head_dim/2]. */
int ug_rope(void* qkv, const float* cos_tab, const float* sin_tab, int64_t tokens, int64_t L, int64_t ldq,
            int nheads, int head_dim, int backward, hipStream_t stream);
/* replaces: Qwen2MLP act_fn(gate) * up (modeling_qwen2.py:46-48); gate_up = [tokens, 2I] = [gate | up] */
int ug_swiglu_fwd(const void* gate_up, void* act, int64_t tokens, int64_t I, hipStream_t stream);
int ug_swiglu_bwd(const void* gate_up, const void* dact, void* dgate_up, int64_t tokens, int64_t I,
                  hipStream_t stream);
/* GELU(erf) of UniGen.mm_projector (models/unigen.py:119-128), bf16: out = gelu(x), or dgelu(x)*dy if dy given */
int ug_gelu(const void* x, const void* dy_or_null, void* out, int64_t n, hipStream_t stream);
/* replaces: llm.model.embed_tokens (models/unigen.py:257,370; fp32 gather) and its scatter-add grad */
int ug_embed_fwd(const int64_t* ids, const float* W, float* out, int64_t tokens, int64_t H, int64_t V,
                 int* err_flag, hipStream_t stream);
int ug_embed_bwd(const int64_t* ids, const float* dout, float* dW, int64_t tokens, int64_t H, int64_t V,
                 hipStream_t stream);
/* the same scatter-add, deterministic, for the (id, row) pairs gathered from every data-parallel rank: `ids_sorted` ascending
 * (stable sort: equal ids in rank, then position order; ids outside [0, V) are padding and skipped), `order[p]` = row of `rows`
 * that sorted position p came from; dW[id] += scale * (sum of the run's rows in that order), one writer per table row */
int ug_embed_bwd_sorted(const int64_t* ids_sorted, const int64_t* order, const float* rows, float* dW, int64_t n,
                        int64_t H, int64_t V, float scale, hipStream_t stream);
/* gather (scatter=0): out[i,:] = in[idx[i],:] ; scatter (1): out[idx[i],:] = in[i,:]   (bf16 rows)
 * replaces the logits[..., -(n+1):-1] / [:, :-1] position slicing of models/unigen.py:310-338 */
int ug_gather_rows_bf16(const void* in, int64_t ld_in, const int64_t* idx, void* out, int64_t ld_out,
                        int64_t n, int64_t C, int scatter, hipStream_t stream);
/* out[c] += sum_r in[r,c]  (bias gradients) */
int ug_colsum_bf16(const void* in, int64_t ld, float* out, int64_t R, int64_t C, hipStream_t stream);

/* ---- attention ------------------------------------------------------------------------------ */
/* Mask compression.  replaces the dense additive [B,1,L,L] masks of training/prompting_utils.py:975-1074
 * as consumed by SDPA: bits[B][L][nW] (nW = ceil(L/64); bit j of word w set <=> key w*64+j visible),
 * tileany[B][nW][nW].  err_flag bit 1 is raised if a value is neither 0 nor <= -1e9. */
#define UG_MASK_F32 0
#define UG_MASK_BF16 1
#define UG_MASK_I64 2
#define UG_MASK_BOOL 3
int ug_attn_mask_compress(const void* mask, int mask_dtype, int64_t stride_b, int64_t stride_row,
                          uint64_t* bits, uint8_t* tileany, int64_t B, int64_t L, int* err_flag,
                          hipStream_t stream);
int ug_attn_mask_causal(const uint8_t* key_valid /* [B,L] or null */, uint64_t* bits, uint8_t* tileany,
                        int64_t B, int64_t L, hipStream_t stream);
/* replaces: torch SDPA in Qwen2Attention.forward (modeling_qwen2.py:196-234), GQA H:HKV, head_dim 128.
 * q/k/v: row (b*L+t), head h at column h*128, row stride ldq.
 * o: [tokens, ldo] bf16, lse: [B][H][L] fp32 (natural log of the sum of exp(scale * q.k) over the visible keys).
 * Rows and keys the mask hides completely (left-padded prompts: ug_attn_mask_causal with key_valid):
 *   - a query row that sees no key gets o = 0 (all bits zero) and lse = +INFINITY; ug_attn_bwd gives it dq = 0 and it adds
 *     nothing to dk / dv;
 *   - a key no query sees gets dk = dv = 0;
 *   - every element of o, lse, dq, dk and dv is written, whatever the mask hides (whole hidden query or key tiles included).
 *   - The q / dout rows of such query rows and the k / v rows of such keys are still READ and multiplied by exact-zero
 *     probabilities in the matrix cores: they may hold any finite values (no bit of any other row depends on them), but not
 *     NaN / Inf -- 0 * NaN = NaN would spread to every row that shares the tile.  The callers keep them finite: an empty row
 *     leaves attention as o = 0, so the next layer's projections of that row are finite. */
int ug_attn_fwd(const void* q, const void* k, const void* v, int64_t ldq, void* o,
                int64_t ldo, float* lse, const uint64_t* bits, const uint8_t* tileany, int64_t B, int64_t L,
                int64_t Lp, int H, int HKV, int head_dim, float scale, hipStream_t stream);
/* dq/dk/dv written with row stride ldg (heads laid out like q/k/v); delta: [B][H][L] workspace.
 * dkv_ws: optional fp32 [B*L][2*HKV*128] workspace, ZERO on entry and left zero: dK/dV are then accumulated per query
 * head (6x the workgroups, balanced under causal masks) with fp32 atomics; null -> per-kv-head kernel, no atomics. */
int ug_attn_bwd(const void* q, const void* k, const void* v, int64_t ldq,
                const void* o, const void* dout, int64_t ldo, const float* lse,
                float* delta, void* dq, void* dk, void* dv, int64_t ldg, const uint64_t* bits,
                const uint8_t* tileany, int64_t B, int64_t L, int64_t Lp, int H, int HKV, int head_dim,
                float scale, float* dkv_ws, const float* rope_cos, const float* rope_sin, float* dbias_qkv, hipStream_t stream);
/* rope_cos / rope_sin ([L][64] fp32, or null): dq and dk leave as the gradient w.r.t. the PRE-RoPE projections -- the transposed
 * rotation of apply_rotary_pos_emb (modeling_qwen2.py:131-135) applied where the gradients are stored, same arithmetic as
 * ug_rope(backward = 1) on the stored tensor.  dbias_qkv ([(H + 2 HKV) * 128] fp32, or null): += the column sums of the stored
 * dq | dk | dv (the bias gradient of the fused q / k / v projection, what ug_colsum_bf16 over the three tensors adds). */

/* ---- autoregressive decode (static KV cache, graph-capturable) -------------------------------- */
/* replaces: transformers DynamicCache.update + SDPA on one new token per row inside
 * UniGen.t2i_generate_ar (models/unigen.py:485-519).  Cache layout K,V [rows][HKV][Tmax][128] bf16.
 * Positions / lengths are read from DEVICE ints so a captured graph can be replayed for every step. */
int ug_kv_store(const void* qkv, int64_t ldq, int64_t k_col, int64_t v_col, void* cache_k, void* cache_v,
                int64_t rows, int64_t L, int HKV, int head_dim, int64_t Tmax, const int* pos_dev, int pos_host,
                hipStream_t stream);
/* ug_rope's rotation for `rows` single-token rows, all at table row *pos_dev of cos / sin [max_pos, head_dim/2].  A *pos_dev at or
 * past max_pos is clamped to the last table row, max_pos - 1 (no error is raised; the table is never read past its end). */
int ug_rope_at(void* qkv, const float* cos_tab, const float* sin_tab, int64_t rows, int64_t ldq, int nheads,
               int head_dim, const int* pos_dev, int64_t max_pos, hipStream_t stream);
int ug_attn_decode(const void* q, int64_t ldq, const void* cache_k, const void* cache_v, const uint8_t* key_valid,
                   void* o, int64_t ldo, int64_t rows, int H, int HKV, int head_dim, int64_t Tmax,
                   const int* len_dev, float scale, hipStream_t stream);
/* Prefill onto a filled cache (a shared prompt prefix, chunked prefill, the next turn of a conversation): causal attention of S
 * new query rows per cache row against the keys and values IN the cache.  Query (r, s) is row r*S + s of q (head h at column
 * h*128, row stride ldq) and sits at position P + s; it attends to key t of cache row r iff t <= P + s and (key_valid is null or
 * key_valid[r*Tmax + t] != 0).  The caller has already stored the new keys and values at positions P .. P+S-1 (ug_kv_store with
 * pos_host = P).  P >= 0 is a host int (prefill is not captured), P + S <= Tmax.  o: bf16 [rows*S, ldo], every element written;
 * a query that sees no key gets o = 0.  Forward only, no lse, no atomics: the same bits on every run.
 * Masked keys inside a staged 64-key tile are still multiplied by exact-zero probabilities (as at ug_attn_fwd), so the cache
 * positions [0, round_up(P+S, 64)) clipped to Tmax must hold FINITE values in both caches, whatever the mask hides (a zero-
 * initialised cache does). */
int ug_attn_prefill_cached(const void* q, int64_t ldq, const void* cache_k, const void* cache_v,
                           const uint8_t* key_valid /* [rows][Tmax] or null */, void* o, int64_t ldo,
                           int64_t rows, int64_t S, int64_t P, int H, int HKV, int head_dim, int64_t Tmax,
                           float scale, hipStream_t stream);
/* weight-streaming GEMV for <= 32 activation rows: acc[r*acc_stride_r + n*acc_stride_n] += sum_k x[r][k] W[n][k]
 * (fp32 atomics into a zeroed accumulator; the decode-time form of every nn.Linear of the backbone,
 * models/unigen.py:496-502).  The decode path keeps row-major accumulators (acc_stride_n = 1). */
int ug_gemv_bf16(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* acc, int64_t acc_stride_r,
                 int64_t acc_stride_n, int64_t N, int64_t K, hipStream_t stream);
/* last launch of a decode step (Qwen2Model.norm after the last layer's down_proj, models/unigen.py:496-502): consumes the
 * row-major fp32 accumulator acc[r*ldacc + n] a decode GEMV filled and leaves it zeroed for the next step:
 *   x += bf16round(acc);  xn = bf16(rmsnorm(x) * w) */
int ug_decode_finish_resid_norm(float* acc, int64_t ldacc, float* x, const float* w, void* xn, int64_t rows, int64_t cols,
                                float eps, int* pos_inc, int* len_inc, hipStream_t stream);
/* pos_inc / len_inc (both or neither): the cache's device-side write position and visible length, incremented by one here -- every
 * kernel of the step that reads them has run by then (the `cache_position += 1` of the reference's loop, models/unigen.py:517). */
/* Five-launch decode layer (what UniGen.t2i_generate_ar's per-token forward, models/unigen.py:496-502, runs).  A decode
 * step is bound by the ~4 us floor of every launch, so all finishing work moves to the CONSUMER of each accumulator
 * and kernel boundaries are the only synchronisation:
 *   ug_decode_gemv_resid_norm  q/k/v and gate/up projections.  Operand = bf16(norm_w[k] * xnew[r][k]) with
 *        xnew = x_in + bf16round(pending) (the previous projection's residual add); writes xnew to x_out (!= x_in) and
 *        adds sum_k xnew^2 into ss_out[r].  RMSNorm's per-row rsqrt factor is applied by the accumulator's consumer.
 *   ug_attn_decode_fused       builds the new token's q/k/v from the raw qkv accumulator (rstd, bias, RoPE), appends k/v
 *        to the cache at *pos_dev, attends to cache keys [0, *pos_dev) + the new token.
 *   ug_decode_gemv             o projection (bf16 operand).
 *   ug_decode_gemv_swiglu      down projection.  Operand = bf16(bf16(silu(g)) * u), g, u = bf16(rstd[r] * gate/up acc).
 * Each GEMV also clears up to two fully-consumed accumulators (zero0/zero1, n floats each, multiples of 4) and one
 * 32-float statistics slot, so a captured step has no memset nodes. */
int ug_decode_gemv(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* acc, int64_t ldacc, int64_t N,
                   int64_t K, float* zero0, int64_t n0, float* zero1, int64_t n1, float* ss_zero, hipStream_t stream);
int ug_decode_gemv_resid_norm(const float* x_in, const float* pending, int64_t ld_pending, const float* norm_w, float* x_out,
                              float* ss_out, int64_t R, const void* W, int64_t ldw, float* acc, int64_t ldacc, int64_t N,
                              int64_t K, float* zero0, int64_t n0, float* zero1, int64_t n1, float* ss_zero,
                              hipStream_t stream);
int ug_decode_gemv_swiglu(const float* gate_up_acc, int64_t ld_gu, const float* ss_in, float eps, int64_t norm_cols, int64_t R,
                          const void* W, int64_t ldw, float* acc, int64_t ldacc, int64_t N, int64_t K, float* zero0, int64_t n0,
                          float* zero1, int64_t n1, float* ss_zero, hipStream_t stream);
int ug_attn_decode_fused(const float* acc_qkv, int64_t ldacc, const float* ss_in, float eps, int64_t norm_cols, const void* bias,
                         const float* cos_tab, const float* sin_tab, const int* pos_dev, void* cache_k, void* cache_v,
                         const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows, int H, int HKV, int head_dim,
                         int64_t Tmax, int64_t max_pos, float scale, hipStream_t stream);
/* ug_attn_decode_fused for the VERIFY step of speculative decoding (ug_spec_verify below): the same inputs and the same finishing
 * arithmetic, but the rows are `rows` CONSECUTIVE positions of ONE sequence, 1 <= rows <= UG_SPEC_MAX_ROWS.
 *   acc_qkv fp32 [rows][ldacc], ss_in [rows], eps, norm_cols, bias, cos_tab / sin_tab, max_pos, scale: as above;
 *   cache_k / cache_v: ONE cache row [1][HKV][Tmax][128]; key_valid [1][Tmax] or null; o bf16 [rows][ldo].
 * With p = *pos_dev, row s sits at position p + s: its q / k / v are bf16(rstd * acc + bias), rotate-half RoPE with separately rounded
 * products at table row min(p + s, max_pos - 1) -- the bits a one-row ug_attn_decode_fused launch at p + s builds -- and its k / v are
 * appended at p + s when that is < Tmax.  Row s attends to the cache keys [0, min(p, Tmax)) that key_valid allows and to the new keys
 * of rows 0 .. s of this launch, nothing else: no new key or value is read back from the cache (the workgroups of row s rebuild rows
 * 0 .. s from the accumulator), so what is stored at or past p before the launch reaches no output, and output row s is the same bits
 * whatever `rows` is and whatever rows > s hold.  Plain stores, no atomics.  A default-mode kernel: there is no ordered form. */
#define UG_SPEC_MAX_ROWS 8
int ug_attn_decode_seq(const float* acc_qkv, int64_t ldacc, const float* ss_in, float eps, int64_t norm_cols, const void* bias,
                       const float* cos_tab, const float* sin_tab, const int* pos_dev, void* cache_k, void* cache_v,
                       const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows, int H, int HKV, int head_dim, int64_t Tmax,
                       int64_t max_pos, float scale, hipStream_t stream);
/* Single-writer decode projections (round 6; the same reference call sites: models/unigen.py:496-502 per-token forward, transformers
 * modeling_qwen2.py Qwen2DecoderLayer.forward / Qwen2MLP.forward / Qwen2Model.norm + lm_head).  Every output element has ONE writer -- a
 * workgroup owns a few weight rows for the whole contraction -- so these launches use no fp32 atomics and leave FINISHED values:
 *   ug_decode_sw_resid    h[r][n] += float(bf16(sum_k x[r][k] W[n][k]))  in place (o projection on the attention output; K == 1536)
 *   ug_decode_sw_gate_up  act = bf16(bf16(silu(gate)) * up), gate | up = Linear(RMSNorm(h))   (Qwen2MLP.forward; W = [2 I][H], gate rows first)
 *   ug_decode_sw_head     logits fp32 [R][N] = Linear(RMSNorm(h)) for N rows of the tied embedding; pos_inc / len_inc (both or
 *                         neither) are incremented by one (the step's last reader of them has run)
 * `h` is the fp32 residual stream [R][H]; RMSNorm is applied as the reference applies it: operand = bf16(norm_w * (h * rsqrt(mean(h^2)
 * + eps))).  The norm-fed entry points also sit behind a split-K producer of the form above: with `pend` (raw fp32 accumulator
 * [R][ld_pend]) the residual stream is h + float(bf16(pend)), written to x_out (a buffer other than h, or NULL) by the launch's first
 * eight workgroups; the accumulator is left as it is (a later launch clears it).
 * `h` carries no leading dimension: it is CONTIGUOUS -- [R][N] for ug_decode_sw_resid (its rows are N floats apart), [R][H] = [R][K] for
 * ug_decode_sw_gate_up and ug_decode_sw_head (rows K = 1536 floats apart), and so is x_out.  The entry points cannot check this.
 * R <= 16; ug_decode_sw_supported() says whether a model's sizes fit this build (hidden 1536 = six 256-wide k-slabs, head_dim 128). */
int ug_decode_sw_supported(int64_t hidden, int64_t inter, int64_t q_dim, int head_dim);
/* The down projection's form (its 287 KB operand rules a whole-K workgroup out): split-K in k-blocks of seven 256-wide slabs -- a
 * workgroup owns 32 weight rows x one k-block, its seven partial tiles meet in LDS and join acc[r*ldacc + n] by ONE fp32 atomic per
 * element (K / 1792 atomics per output instead of K / 256).  Same accumulator / clears contract as ug_decode_gemv above. */
int ug_decode_sw_kblock(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* acc, int64_t ldacc, int64_t N, int64_t K,
                        float* zero0, int64_t n0, float* zero1, int64_t n1, float* ss_zero, hipStream_t stream);
int ug_decode_sw_resid(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, int64_t N, int64_t K, float* h,
                       hipStream_t stream);
int ug_decode_sw_gate_up(const float* h, const float* pend, int64_t ld_pend, float* x_out, const float* norm_w, float eps, int64_t R,
                         int64_t H, const void* W, int64_t ldw, int64_t I, void* act, int64_t ld_act, hipStream_t stream);
int ug_decode_sw_head(const float* h, const float* pend, int64_t ld_pend, float* x_out, const float* norm_w, float eps, int64_t R,
                      int64_t H, const void* W, int64_t ldw, int64_t N, float* logits, int64_t ld_logits, int* pos_inc, int* len_inc,
                      hipStream_t stream);
/* finish a split-K fp32 accumulation: mode 0: out_bf16 = bf16(acc + bias); mode 1: resid += bf16round(acc) */
int ug_skinny_finish(const float* acc, const void* bias, void* out_bf16, float* resid, int64_t M, int64_t N,
                     int mode, hipStream_t stream);
/* Ordered (deterministic) decode forms: the split-K launches above sum partial products with fp32 atomics, so their results depend on
 * the order workgroups arrive in.  These entry points write every k-slice's partial tile into a SLOT of its own by plain stores (no
 * atomics, no clears; every slot element has exactly one writer) and the consumer sums the slots in ONE fixed order -- ascending slot
 * index, in fp32 -- before the rounding the default form applies at the same point.  Same step, bit-reproducible run to run and between
 * eager and captured replay.  Slot p of a [slots][rows][ld] buffer starts p * rows * ld floats in, unless a stride is given.
 *   ug_gemv_bf16_ord       part[s * part_stride + r * ldpart + n] = sum_{k in slice s} x[r][k] W[n][k]; slices of 256 k (ceil(K / 256)
 *                          slots; one slot for K < 256).  R <= 32.
 *   ug_skinny_finish_ord   v = sum_{p < nparts} parts[p * part_stride + m * N + n] (ascending p), then exactly one of:
 *                          out_bf16 = bf16(v + bias) | resid += bf16round(v) | out_f32 = v.
 * The single-writer decode layer (R <= 16, ug_decode_sw_supported() sizes; K / 1792 == 5 k-blocks for the down projection):
 *   ug_decode_gemv_resid_norm_ord  q/k/v.  As ug_decode_gemv_resid_norm, with the pending term = bf16round(sum_{p < npend} pend[p][R]
 *                          [ld_pending]) (the previous layer's down k-block slots; npend 0 -- layer 0 -- or 5); the projection lands in
 *                          part[slab][R][ldpart] (ceil(K / 256) slabs) and the row sums of squares of slab s in ss_part[s * 32 + r].
 *   ug_attn_decode_fused_ord   as ug_attn_decode_fused, fed by those slots (nparts == 6: hidden 1536): q/k/v and the statistics are
 *                          the ascending-slab sums, then rstd, bias and RoPE as in the default form.
 *   ug_decode_sw_kblock_ord    down projection: k-block b's partial (its seven slabs pre-reduced in LDS in wave order) is stored into
 *                          part[b][R][ldpart].
 *   ug_decode_finish_resid_norm_ord  x += bf16round(sum_{p < nparts} parts[p][rows][ldp]); xn = bf16(rmsnorm(x) * w) if xn is given. */
int ug_gemv_bf16_ord(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* part, int64_t ldpart, int64_t part_stride,
                     int64_t N, int64_t K, hipStream_t stream);
int ug_skinny_finish_ord(const float* parts, int64_t nparts, int64_t part_stride, const void* bias, void* out_bf16, float* out_f32,
                         float* resid, int64_t M, int64_t N, hipStream_t stream);
int ug_decode_gemv_resid_norm_ord(const float* x_in, const float* pend_parts, int64_t ld_pending, int64_t npend, const float* norm_w,
                                  float* x_out, float* ss_part, int64_t R, const void* W, int64_t ldw, float* part, int64_t ldpart,
                                  int64_t N, int64_t K, hipStream_t stream);
int ug_attn_decode_fused_ord(const float* qkv_part, int64_t ldpart, int64_t nparts, const float* ss_part, float eps, int64_t norm_cols,
                             const void* bias, const float* cos_tab, const float* sin_tab, const int* pos_dev, void* cache_k,
                             void* cache_v, const uint8_t* key_valid, void* o, int64_t ldo, int64_t rows, int H, int HKV, int head_dim,
                             int64_t Tmax, int64_t max_pos, float scale, hipStream_t stream);
int ug_decode_sw_kblock_ord(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, float* part, int64_t ldpart, int64_t N,
                            int64_t K, hipStream_t stream);
int ug_decode_finish_resid_norm_ord(const float* parts, int64_t ldp, int64_t nparts, float* x, const float* w, void* xn, int64_t rows,
                                    int64_t cols, float eps, int* pos_inc, int* len_inc, hipStream_t stream);

/* ---- device-side prompt / mask assembly --------------------------------- */
/* replaces the per-sample Python loops of UniversalPromptingQwen2.t2i_prompt (training/prompting_utils.py:59-111, prompt
 * dropout excluded) and the dense [B,1,L,L] masks of create_attention_mask_predict_next / _for_mmu (:975-1036): the
 * compressed mask is built straight from the token ids.  text_ids: all prompts back to back, text_offsets [B+1].
 * mode: 0 = predict_next with rm_pad_in_image (t2i), 1 = predict_next (lm), 2 = mmu (eoi of the first match in the batch).
 * meta_ws: int32 [4*B], flags_ws: bytes [B*L]. */
int ug_t2i_assemble(const int64_t* text_ids, const int64_t* text_offsets, const int64_t* conv_start, int64_t n_start,
                    const int64_t* conv_end, int64_t n_end, const int64_t* image_in, const int64_t* image_labels, int64_t B,
                    int64_t n_image, int64_t max_seq_len, int64_t pad_id, int64_t soi_id, int64_t eoi_id, int64_t ignore_id,
                    int64_t* input_ids, int64_t* labels, uint8_t* attn01, hipStream_t stream);
int ug_attn_mask_from_ids(const int64_t* ids, int64_t B, int64_t L, int64_t pad_id, int64_t soi_id, int64_t eoi_id, int mode,
                          int* meta_ws, uint8_t* flags_ws, uint64_t* bits, uint8_t* tileany, hipStream_t stream);

/* replaces: mask_or_random_replace_tokens (data/masking.py:13-94, the branch every shipped config takes: noise_type
 * 'mask', no contiguous region, predict_all_tokens off).  scores [B, n] fp32 are the caller's `torch.rand(B, n)`;
 * num_masked [B] fp32 = (n * mask_prob).round().clamp(min=1).  Position j is masked iff argsort(scores)[j] < num_masked
 * (ties broken by index).  input_ids = mask_id on masked positions else the token; labels = token on masked positions
 * else ignore_id.  Bit-equal to the reference for distinct scores. */
int ug_maskgit_train_mask(const int64_t* tokens, const float* scores, const float* num_masked, int64_t B, int64_t n,
                          int64_t mask_id, int64_t ignore_id, int64_t* input_ids, int64_t* labels, hipStream_t stream);

/* ---- MaskGIT parallel decoding step ------------------------------------------------------------ */
/* replaces, per round of UniGen.t2i_generate (models/unigen.py:404-451): the CFG mix of the code-book logits, softmax,
 * torch.multinomial, the gather of the drawn token's probability and models/sampling.py:41-46 mask_by_random_topk.
 * logits: bf16 [(cfg ? 2 : 1) * N * n][ld], row (b*n + i) = image b / position i, the N*n unconditional rows after the
 * conditional ones; V code-book columns.  u_sample / u_conf: uniforms in [0,1) [N*n] from the caller's generator
 * (token = inverse CDF in index order; Gumbel = -log(-log(u))).  cur_ids: code ids or mask_id [N*n].
 * mask_len_sched = floor(n * schedule(ratio)); temperature = the already-compounded Gumbel temperature.
 * Outputs [N*n]: sampled (known tokens kept), next_cur (mask_id where re-masked), next_ids (+ id_offset unless masked),
 * masking_out (optional bytes).  sel_ws: fp32 [N*n] scratch. */
int ug_maskgit_step(const void* logits, int64_t ld, int64_t V, int64_t N, int64_t n, int cfg, float guidance_scale,
                    const float* u_sample, const float* u_conf, const int64_t* cur_ids, int64_t mask_id, int64_t id_offset,
                    int64_t mask_len_sched, float temperature, int64_t* sampled, float* sel_ws, int64_t* next_cur,
                    int64_t* next_ids, uint8_t* masking_out, hipStream_t stream);

/* ug_maskgit_step with a sampling temperature, top-k / top-p / min-p truncation and the drawn tokens' log-probabilities.  Every
 * argument of ug_maskgit_step keeps its meaning (`temperature` stays the Gumbel temperature of the re-masking, which is unchanged);
 * sample_temperature > 0, top_k >= 0 (0 or >= V: off), 0 < top_p <= 1 (1: off), 0 <= min_p <= 1 (0: off).
 * Per masked position bi (cur_ids[bi] == mask_id), with c, u the bf16 logits of rows bi and N*n + bi taken to fp32:
 *   v[e] = (guidance_scale * (c[e] - u[e]) + u[e]) * fp32(1 / sample_temperature)      (cfg == 0: v = c * fp32(1 / sample_temperature))
 *   kept set = ug_ar_sample_filtered's, word for word: {v >= tau}, tau = max(tau_k, tau_p, tau_m); every value tied at the top-k value
 *     is kept, top-p keeps or drops a run of equal values as a whole, the maximum is always kept;
 *   sampled[bi] = inverse CDF in index order on u_sample[bi] over exp(v - max v), dropped entries counted as 0: always a kept token;
 *   sel_ws[bi] = exp(v[tok] - max v) / (sum over the kept): the confidence that decides re-masking is the token's probability under
 *     the distribution it was drawn from.
 * logp (optional, fp32 [N*n][2], natural logs -- the pair ug_ar_sample_*_logp writes):
 *   logp[2*bi]   = v[tok] - max v - log(sum over the kept e of exp(v[e] - max v));
 *   logp[2*bi+1] = c[tok] - max c - log(sum over e < V of exp(c[e] - max c)): the conditional model's own log-softmax (no CFG, no
 *     temperature, no truncation).
 * stats (optional, fp32 [N*n][2]): stats[2*bi] = the smallest kept value, stats[2*bi+1] = the number of kept entries.
 * Known positions behave as in ug_maskgit_step; their logp / stats slots are NOT written (a caller that zeroes logp once and passes it
 * to every round ends with each position's entry from the last round that drew it).
 * Every float sum runs in a fixed order and there are no float atomics: the call is a bit-reproducible function of its inputs.
 * With every filter off and sample_temperature == 1 the draw is ug_maskgit_step's own kernel (instantiated with the two outputs riding
 * along): sampled, sel_ws, next_cur, next_ids and masking_out are bit for bit ug_maskgit_step's, with or without logp / stats.
 * Otherwise one workgroup per masked position reads its two rows once, stages the mixed row in LDS and runs the threshold search it
 * shares with ug_ar_sample_filtered; that path needs V <= 8192 (an argument error beyond).  Any ld >= V and any base alignment
 * work: 16-byte loads are used when ld % 8 == 0 and logits is 16-byte aligned, 2-byte loads otherwise. */
int ug_maskgit_step_ex(const void* logits, int64_t ld, int64_t V, int64_t N, int64_t n, int cfg, float guidance_scale,
                       const float* u_sample, const float* u_conf, const int64_t* cur_ids, int64_t mask_id, int64_t id_offset,
                       int64_t mask_len_sched, float temperature, float sample_temperature, int64_t top_k, float top_p, float min_p,
                       int64_t* sampled, float* sel_ws, int64_t* next_cur, int64_t* next_ids, uint8_t* masking_out, float* logp,
                       float* stats, hipStream_t stream);

/* one autoregressive sampling step (models/unigen.py:503-519) on the raw fp32 lm-head accumulator acc [2*bsz][ldacc]
 * (conditional rows, then unconditional; rounded to bf16 like the head's output; cleared on exit): CFG mix, /temperature,
 * softmax + inverse-CDF draw on uniforms[step*bsz + b] (or argmax if greedy), step = *pos_dev - pos0.  Writes tok[b],
 * out_tokens[b*nsteps + step] and the next input x[b], x[bsz+b] = embed[token + id_offset] (fp32 rows of ld_embed). */
int ug_ar_sample(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                 const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed, int64_t ld_embed,
                 int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, hipStream_t stream);

/* ug_ar_sample with truncated sampling, in the order temperature -> top-k -> top-p -> min-p -> draw (transformers' order).  Per
 * image: v[e] = the mixed logit exactly as ug_ar_sample forms it, mx = max v, ex[e] = exp(v[e] - mx).  Each filter is a value
 * threshold and the kept set is {e : v[e] >= tau}, tau = max(tau_k, tau_p, tau_m):
 *   top_k (0 or >= V: off): tau_k = the k-th largest value, duplicates counted; every value tied at tau_k is kept.
 *   top_p (0 < top_p <= 1; 1: off): over S_k = {v >= tau_k}, Z = sum of ex over S_k: a value t is kept iff the mass of the strictly
 *     greater values of S_k is <= top_p * Z.  A run of equal values is kept or dropped as a whole (a sorted cut through such a run
 *     depends on the sort's order of equal keys); the maximum is always kept.
 *   min_p (0 <= min_p <= 1; 0: off): tau_m = mx + log(min_p).
 * The draw is ug_ar_sample's: inverse CDF in index order on uniforms[step*bsz + b] over ex with dropped entries counted as 0; the
 * drawn token is always a kept one.  No float atomics: a step is a bit-reproducible function of its inputs.  greedy: the filters are
 * ignored (the argmax is always kept) and stats is not written.  stats (optional, [bsz][2]): stats[2b] = the smallest kept value,
 * stats[2b+1] = the number of kept entries. */
int ug_ar_sample_filtered(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                          const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed,
                          int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, int64_t top_k,
                          float top_p, float min_p, float* stats, hipStream_t stream);

/* ---- per-token log-probabilities of the AR samplers --------------------------------------------- */
/* ug_ar_sample / ug_ar_sample_filtered with one more output, logp fp32 [bsz][nsteps][2] (null: an argument error -- callers that want
 * no output use the entry points above); everything else (token, out_tokens, x, the cleared accumulator, stats) is bit for bit what
 * those compute on the same inputs.  All values are natural logs, at most 0.  With c~, u~ the bf16-rounded conditional and unconditional
 * rows, v[e] = (u~[e] + s * (c~[e] - u~[e])) * (1 / temperature) and mx = max v as above, and step = *pos_dev - pos0 (the indexing of
 * out_tokens: the token drawn from the prefill is step 0):
 *   logp[(b * nsteps + step) * 2 + 0] = v[tok] - mx - log(sum over the kept e of exp(v[e] - mx)): the log-probability under the
 *     distribution the token was drawn from, after CFG, temperature and truncation.  Kept = [0, V) for ug_ar_sample_logp, {v >= tau} for
 *     ug_ar_sample_filtered_logp, and [0, V) at the call's temperature with greedy (the filters are ignored, as for the pick).
 *   logp[(b * nsteps + step) * 2 + 1] = c~[tok] - max c~ - log(sum over e < V of exp(c~[e] - max c~)): the conditional model's own
 *     log-softmax -- no CFG, no temperature, no truncation; what a teacher-forced pass would score.
 * Every float sum runs in a fixed order (chunk in index order, tree over the wave, the sixteen wave partials in wave order) and there
 * are no float atomics: logp is a bit-reproducible function of the inputs. */
int ug_ar_sample_logp(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                      const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed, int64_t ld_embed,
                      int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, float* logp, hipStream_t stream);
int ug_ar_sample_filtered_logp(float* acc, int64_t ldacc, int64_t bsz, int64_t V, float guidance_scale, float temperature, int greedy,
                               const float* uniforms, const int* pos_dev, int64_t pos0, int64_t nsteps, const float* embed,
                               int64_t ld_embed, int64_t H, int64_t id_offset, int64_t* tok, int* out_tokens, float* x, int64_t top_k,
                               float top_p, float min_p, float* stats, float* logp, hipStream_t stream);

/* ---- text decode: the pick over the whole vocabulary (csrc/text_sampler.hip) --------------------- */
/* One text decode step behind the head, for R <= 32 rows: the token of every row, the stop rule of the host loop
 * (models/unigen.py: emit_until_stop), the token's slot in the output buffer and the next step's input.
 * logits: fp32 [R][ld], V <= ld (rows on 16-byte boundaries are read four entries at a time); entries V .. ld-1 are never
 * candidates.  clear != 0: the V read entries of every row are zeroed on the way out (what the atomic GEMV head needs, as ug_ar_sample has it); nothing else in the buffer is written.
 * stop_ids: n_stop <= 8 ids in device memory (n_stop == 0: none).  pad_id < 0: none.  embed: fp32 table of embed_rows rows.
 * state (int32, device memory; the HOST resets it to {0, R, 0, 0, 0 ...} at the start of a call, nothing about the prompt is an
 * argument): [0] step -- the kernels' own counter, advanced once per call of this entry point; [1] remaining -- rows not yet done;
 * [2] steps_used; [3] an arrival ticket (0 between calls); [4 + r] done[r].
 * Per row r:
 *   1. value = the logit rounded to bf16 (the rounding of the head output the host loop picks from);
 *   2. token = the LOWEST index attaining the maximum (torch.argmax's documented tie rule);
 *   3. if done[r] and pad_id >= 0: token = pad_id;
 *   4. out_tokens[r * nsteps + step] = tok[r] = token;
 *   5. if token is a stop id and the row was not done: lengths[r] = step + 1 (lengths may be null), done[r] = 1, --remaining, and when
 *      remaining reaches zero steps_used = step + 1;
 *   6. x[r] = embed[token] (H floats).
 * No float atomics; integer atomics only where their order cannot matter: a step is a function of its inputs. */
int ug_text_pick(float* logits, int64_t ld, int64_t R, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                 const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                 int* out_tokens, int* lengths, float* x, hipStream_t stream);

/* number of int32 of the workspace ug_text_sample needs for R rows (a negative status for R outside 1..32).  The workspace must be
 * all zero before the first call; every call leaves it all zero. */
int ug_text_sample_workspace_ints(int64_t R);

/* ug_text_pick with a sampled token: temperature -> top-k -> top-p -> draw.  v[e] = bf16round(logit[e]) * fp32(1 / temperature),
 * ex[e] = exp(v[e] - max v).  The kept set is ug_ar_sample_filtered's: {v >= tau}, tau = max(tau_k, tau_p); top_k 0 or >= V: off, every
 * value tied at tau_k is kept; top_p 1: off, a run of equal values is kept or dropped as a whole.
 * The draw is an inverse CDF on uniforms[step * R + r] over the kept entries ordered by VALUE DESCENDING and, among equal values, by
 * index ascending -- not ug_ar_sample's index order: v is a monotone function of a 16-bit pattern, so the selection runs on a
 * 65 536-bin count histogram of the row (mass of a bin = count x ex) instead of on the 160 000 entries, and the histogram's order is
 * the value's.  With T the kept mass, the drawn key is the first whose running mass exceeds u * T and the rank inside the key is
 * min(count - 1, floor(residual / ex)).  Three launches: histogram (integer atomics), selection (one workgroup per row; every float
 * sum in a fixed order), locate + ug_text_pick's steps 3-6.  A step is a bit-reproducible function of its inputs.
 * V <= 262 144.  stats (optional, [R][2]): the smallest kept value and the number of kept entries.  NaN logits are no candidates. */
int ug_text_sample(float* logits, int64_t ld, int64_t R, int64_t V, int clear, float temperature, int64_t top_k, float top_p,
                   const float* uniforms, int* workspace, float* stats, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                   const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                   int* out_tokens, int* lengths, float* x, hipStream_t stream);

/* ug_text_pick / ug_text_sample with one more output, logp fp32 [R][nsteps] (null: an argument error -- callers that want no output use
 * the entry points above); tokens, records, state, x, the cleared logits and the workspace are bit for bit what those leave.  This is
 * transformers' compute_transition_scores(..., normalize_logits=True): the log-softmax of the PROCESSED scores at the emitted token, a
 * natural log, at most 0.
 *   ug_text_pick_logp:   s[e] = the logit rounded to bf16 (behind ug_text_penalize, if the caller runs it; no temperature);
 *                        logp[r * nsteps + step] = s[tok] - max s - log(sum over e < V of exp(s[e] - max s)).
 *   ug_text_sample_logp: v, the kept set and T (the kept mass relative to max v) as ug_text_sample defines them;
 *                        logp[r * nsteps + step] = v[tok] - max v - log T.
 * A NaN entry contributes nothing (it is no candidate), -inf contributes 0.  A row that was done BEFORE the step records 0.0 (whether it
 * emits pad_id or, without one, goes on emitting tokens); the step that emits the stop id records its real value.  Nothing is written
 * for step >= nsteps.  The greedy sum is formed in the pick's single pass over the row (per thread a running maximum and a sum rescaled
 * to it, then rescaled to the row's maximum, a tree over the wave, the sixteen wave partials in wave order); the sampled form takes T
 * from the selection launch.  Fixed order, no float atomics: a bit-reproducible function of the inputs. */
int ug_text_pick_logp(float* logits, int64_t ld, int64_t R, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                      const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                      int* out_tokens, int* lengths, float* x, float* logp, hipStream_t stream);
int ug_text_sample_logp(float* logits, int64_t ld, int64_t R, int64_t V, int clear, float temperature, int64_t top_k, float top_p,
                        const float* uniforms, int* workspace, float* stats, const int64_t* stop_ids, int64_t n_stop, int64_t pad_id,
                        const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t nsteps, int64_t* tok,
                        int* out_tokens, int* lengths, float* x, float* logp, hipStream_t stream);

/* Logits processor of the on-device text loop: transformers' RepetitionPenaltyLogitsProcessor.  THE RULE: for every token id that
 * occurs in the row's sequence so far, s <- s * p if s < 0 else s / p; once per distinct id, however often the id occurs; ahead of
 * temperature / top-k / top-p.  The row's sequence so far = the prompt ids at positions the key-validity mask marks real + the tokens
 * emitted so far (a prompt given as embeddings has no ids: the emitted tokens only, as transformers has it for inputs_embeds).
 * p is finite and > 0; p = 1 is off (the callers then launch nothing).
 *   host loop:   the rule in fp32 on the fp32 copy of the head's bf16 logits (models/sampling.py: apply_repetition_penalty);
 *   device loop: s = bf16round(logit), the product / quotient in fp32 with round-to-nearest, the fp32 result stored back;
 *                ug_text_pick / ug_text_sample then read it and round it to bf16 as they round every logit.
 * So greedy tokens of the two loops can differ only where two processed values fall within one bf16 step of each other.
 * 0 and -0.0 stay zero, +inf / p = +inf, NaN stays NaN (no candidate downstream).
 * seen: int32 [R][ld_words], ld_words >= W = ceil(V / 32); bit (e & 31) of word (e >> 5) of row r: id e is in row r's sequence. */

/* sets the bit of every prompt id: ids int64 [R][ld_ids >= L]; valid (nullable) uint8 [R][L], 0 = not a real position; ids outside
 * [0, V) are ignored.  Integer atomicOr: the order cannot matter.  Once per call, outside the captured step. */
int ug_text_seen_mark(int* seen, int64_t ld_words, const int64_t* ids, int64_t ld_ids, int64_t R, int64_t L, const uint8_t* valid,
                      int64_t V, hipStream_t stream);

/* One launch per step between the head and the pick, R <= 32; logits / ld as ug_text_pick has them (no alignment needed).  A thread
 * owns whole bitmap words of one row: if tok (nullable, int64 [R]: the token the previous step emitted) falls into its word it ORs the
 * bit in and stores the word (a plain store: nobody else touches the word); for every set bit e < V it then rewrites logits[r][e] by
 * the device rule above.  Bits at or above V in the last word are never acted on; the logits of unseen ids and entries V .. ld-1 are
 * neither read nor written.  No atomics, no float reductions: a bit-reproducible function of its inputs. */
int ug_text_penalize(float* logits, int64_t ld, int64_t R, int64_t V, float penalty, int* seen, int64_t ld_words, const int64_t* tok,
                     hipStream_t stream);

/* Constraints of the text loops: logit_bias, suppress_tokens, min_new_tokens, no_repeat_ngram_size, stop_sequences
 * (UniGen.generate / mmu_generate / mmu_generate_batch; host side models/sampling.py + models/unigen.py: with_constraints).
 * THE ORDER is transformers': sequence bias, repetition penalty, the -inf writers (n-gram block, min-new-tokens, suppress), then
 * temperature / top-k / top-p.  The -inf writers commute with the penalty (-inf * p == -inf / p == -inf for p > 0), so both loops
 * apply all of them in front of the penalty; on the device that is ONE launch ahead of ug_text_penalize.
 *   logit_bias {id: b}: b finite, added to the id's score in every row (SequenceBiasLogitsProcessor with keys of length 1).
 *   suppress_tokens:    the id's score becomes -inf (SuppressTokensLogitsProcessor).  An id in both lists, twice in one, or outside
 *                       [0, V) is refused by the callers before any launch.
 *   min_new_tokens m:   while fewer than m tokens have been emitted every single stop id scores -inf
 *                       (MinNewTokensLengthLogitsProcessor); stop sequences are not held back.
 *   no_repeat_ngram_size n (0: off): NoRepeatNGramLogitsProcessor on the row's HISTORY h = the ids the repetition penalty counts, in
 *                       order: the prompt ids inside [0, V) at mask-valid positions, compacted (a prompt given as embeddings: nothing; a
 *                       prefix + tail prompt: the prefix's ids if it has them, then the tail's), then the tokens emitted (fed back) so
 *                       far.  With T = len h: if T >= n - 1, every t = h[i + n - 1] with h[i .. i + n - 1) == h[T - n + 1 .. T) for
 *                       0 <= i <= T - n scores -inf.  (n = 1: every id of the history.)
 *   stop_sequences:     entries of length 1 join the stop ids (at most 8 in all on the device).  A longer entry finishes a row at the
 *                       step whose emitted token completes it, matched on EMITTED tokens only (a match never reaches into the prompt);
 *                       the completing token is kept, lengths[r] = step + 1, and from the next step on the row is what it is behind a
 *                       stop id: pad fill if there is a pad id, log-probability 0.0, the loop ends once every row is done.
 * The host loop has no size limits.  The device loop: 1024 bias + suppress entries, n <= 16, 8 stop sequences of at most 16 ids. */

/* One launch per step between the head and ug_text_penalize, R <= 32, one workgroup per row; logits / ld as ug_text_pick has them (no
 * alignment needed).
 * bias: n_bias <= 1024 pairs {int32 id, fp32 bias} in device memory, ids DISTINCT; a suppressed id carries bias = -inf.
 * stop_ids / n_stop: the session's single stop ids (ug_text_pick's).  ngram = n <= 16 (0: off).
 * hist int32 [R][ld_hist], hist_len int32 [R]: the prompt part of every row's history, written by the host at the start of a call,
 * outside the captured step (ld_hist == 0: none; a length is clamped to [0, ld_hist]).  out_tokens int32 [R][nsteps]: the pick's
 * records.  state: the pick's state block; step = state[0] is read, nothing of the block is written.
 * Phase 1, thread j -> entry j:  logits[r][id] = bias == -inf ? -inf : fp32(bf16round(logits[r][id]) + bias)   (round to nearest).
 * Workgroup barrier.  Phase 2, the -inf stores: the stop ids while step < min_new; the n-gram bans over the combined history =
 * hist[r][0 .. len) followed by out_tokens[r][0 .. step).  An id outside [0, V) found in a list or a history takes part in the n-gram
 * comparison as the number it is and is never used as an index.  Only the named entries of the logits are read or written; entries
 * V .. ld-1 are never touched.  No atomics, no float reductions: a bit-reproducible function of its inputs. */
int ug_text_constrain(float* logits, int64_t ld, int64_t R, int64_t V, const void* bias, int64_t n_bias, int64_t min_new,
                      const int64_t* stop_ids, int64_t n_stop, int64_t ngram, const int* hist, int64_t ld_hist, const int* hist_len,
                      const int* out_tokens, int64_t nsteps, const int* state, hipStream_t stream);

/* One launch per step BEHIND the pick launch(es), R <= 32: the stop sequences.  seq_ids int32 [n_ids] = the ns <= 8 sequences (2 .. 16
 * ids each) back to back, seq_off int32 [ns + 1] their offsets (seq_off[ns] == n_ids); an entry whose offsets do not fit is skipped.
 * step = state[0] - 1, the step the pick has just recorded.  For every row that is not done and whose last m emitted tokens
 * out_tokens[r][step - m + 1 .. step] equal a sequence of length m <= step + 1 (never a column before 0), exactly step 5 of ug_text_pick:
 * lengths[r] = step + 1 (lengths may be null), done[r] = 1, --remaining, and when remaining reaches zero steps_used = step + 1.  A row
 * that is done -- by a stop id of this very step too -- is left alone: a row never finishes twice, whatever number of sequences match. */
int ug_text_stop_seq(const int* seq_ids, const int* seq_off, int64_t ns, int64_t n_ids, const int* out_tokens, int64_t nsteps, int64_t R,
                     int* state, int* lengths, hipStream_t stream);

/* ---- prompt-lookup speculative decoding of one greedy row (csrc/spec_decode.hip; the rules: csrc/spec_plan.h) ----
 * One verify step runs the decoder stack on S = 1 + K rows: the last emitted token and a draft of up to K tokens copied from an earlier
 * occurrence of the sequence's last ids (transformers' prompt_lookup_num_tokens), at consecutive positions of one cache row
 * (ug_attn_decode_seq).  This entry point runs behind the head and owns everything a step decides; two launches, no host
 * synchronisation, no shape depends on the step.
 *   logits fp32 [rows][ld], V <= ld: the head's output for the step's rows; clear != 0 leaves the V read entries of every row zeroed.
 *   tok int64 [next_rows]: the step's inputs, tok[0] = the last emitted token, tok[1 .. n_draft] the draft; rewritten for the next step.
 *   state int32 [16]: [0] emitted, [1] done, [2] steps, [3] drafted, [4] accepted, [5] n_draft (of tok as it stands), [6] the
 *   history's length, [8 + s] the picks of this call.  The host zeroes it at the start of a call and sets [6].
 *   hist int32 [hist_cap]: the searchable history, state[6] ids of it filled (lookup ids, then the prompt's, then everything emitted).
 *   (a) pick    g[s] = the LOWEST index attaining the maximum of the bf16-rounded logits of row s (ug_text_pick's steps 1 and 2);
 *   (b) accept  a = the number of leading s < n_draft with g[s] == tok[s + 1];
 *   (c) emit    g[0 .. a], cut after the first stop id (inclusive) and at `width`; either cut sets done (and lengths[0] = emitted, if
 *               given).  The tokens go to out_tokens [width] and to the history; with pos / len given (a decoder step; both or neither)
 *               *pos += the number emitted, *len = *pos + 1, ++steps, drafted += n_draft, accepted += a.  Both null: the first token,
 *               picked from the prefill's hidden state, moves no position and counts no step.
 *   (d) draft   on the history h[0, n): for G' = min(ngram, n - 1) down to 1 the smallest i with i + G' < n and
 *               h[i, i + G') == h[n - G', n); the draft is h[i + G', min(i + G' + num_draft, n)); the first G' with a match wins, none
 *               leaves n_draft = 0 (PromptLookupCandidateGenerator.get_candidates' rule);
 *   (e) next    tok[0] = the last emitted token, tok[1 ..] = the draft, rows behind it repeat the last valid one (padding: finite,
 *               their results are ignored); x[s] = embed[tok[s]] (H floats) for all next_rows rows.
 * A call on a done state picks (and clears) and changes nothing else; the call that sets done leaves tok, x and n_draft as they were.
 * rows, next_rows <= UG_SPEC_MAX_ROWS, num_draft < next_rows, 1 <= ngram <= 4, n_stop <= 8.  No atomics: a step is a function of its
 * inputs. */
int ug_spec_verify(float* logits, int64_t ld, int64_t rows, int64_t V, int clear, const int64_t* stop_ids, int64_t n_stop,
                   const float* embed, int64_t ld_embed, int64_t embed_rows, int64_t H, int* state, int64_t width, int64_t* tok,
                   int64_t next_rows, int* out_tokens, int* lengths, int* hist, int64_t hist_cap, int64_t ngram, int64_t num_draft,
                   int* pos, int* len, float* x, hipStream_t stream);

/* ---- loss ------------------------------------------------------------------------------------ */
/* replaces: F.cross_entropy(ignore_index=-100) x3 in UniGen.forward (models/unigen.py:310-338) and
 * get_batch_logps (training/train_dpo.py:51-90).  logits bf16 [R, ld], ld % 8 == 0.
 * loss_and_count (optional): [0] = mean loss over valid rows, [1] = number of valid rows.
 * A row whose label equals ignore_index or lies outside [0, V) is an ignored row everywhere: it gets loss_row = logp = 0.0 (its lse
 * is written as usual), it is not counted in loss_and_count[1], and ug_ce_bwd writes it a zero gradient row, in the mean form and
 * in the row_scale form alike.  With no valid row the mean is 0 / 0 = NaN like F.cross_entropy's, and the gradient is all zeros.
 * Finite logits are a precondition: a lane whose first chunk of a row is all -inf forms -inf - -inf in its running sum. */
int ug_ce_fwd(const void* logits, int64_t ld, int64_t R, int64_t V, const int64_t* labels,
              int64_t ignore_index, float* lse, float* loss_row, float* logp_label, float* loss_and_count,
              hipStream_t stream);
/* in place: logits <- (softmax - onehot) * (*gscale / count) (valid rows), 0 elsewhere incl. pad cols.
 * row_scale (optional, fp32 [R]): per-row factor instead of *gscale / count -- the backward of per-row label
 * log-probabilities (get_batch_logps, training/train_dpo.py:51-90: pass minus the upstream gradient of each row's logp) */
int ug_ce_bwd(void* logits_inout, int64_t ld, int64_t R, int64_t V, const int64_t* labels,
              int64_t ignore_index, const float* lse, const float* loss_and_count, const float* gscale,
              const float* row_scale, hipStream_t stream);

/* ---- scoring given labels without the logits ------------------------------------------------- */
/* The head product and its softmax statistics in one launch pair; no [R, V] buffer exists anywhere (head_score.hip).
 *   x bf16 [R][ldx]: final-norm hidden rows; W bf16 [V][ldw]: the row-major table; K <= ldx, ldw; K % 32 == 0; ldx % 8 == ldw % 8 == 0;
 *   labels int64 [R]; ws: ug_head_score_ws_bytes(R, V) bytes, 16-byte aligned, need not be initialised;
 *   logp, lse, best, best_logit: [R] each; lse / best / best_logit may be null.
 * Per row r, with s[e] = bf16round(fp32 sum over k of x[r][k] * W[e][k]) for e < V (the rounding of the precision contract: a Linear
 * output is rounded where autocast rounds it -- the number the host loop of generate(return_logprobs=True) and ug_text_pick pick from):
 *   lse = max s + log(sum exp(s - max s));  best = the lowest index attaining max s (torch.argmax's tie rule, ug_text_pick's);
 *   best_logit = max s;  logp = s[label] - lse.
 * A row whose label equals ignore_index or lies outside [0, V) gets logp = 0.0; its other outputs are written as usual.  Finite
 * inputs are a precondition.  V needs no alignment; table rows >= V and x rows >= R are never read; nothing past R is written.
 * Workspace: 16 bytes per (row, 256-entry column tile) -- fp32 maximum, fp32 sum rescaled to it, int32 first index of it -- plus one
 * fp32 per row for the label's logit, written once by the single tile that holds it.  A finishing launch merges a row's tiles in
 * tile order.  No atomics, fixed orders: the same bits on every run; and a row's four outputs are the same bits whatever R is and
 * whatever the other rows hold (only the row-tile height follows R, head_score_plan.h).
 * ug_head_score_ws_bytes: > 0, or a negative status and an error string for R < 1 or V < 1 (or a problem too large for one call). */
int ug_head_score_ws_bytes(int64_t R, int64_t V);
int ug_head_score(const void* x, int64_t ldx, int64_t R, const void* W, int64_t ldw, int64_t V, int64_t K,
                  const int64_t* labels, int64_t ignore_index, void* ws, float* logp, float* lse, int64_t* best, float* best_logit,
                  hipStream_t stream);

/* ---- Beam search of the text loop --------------------------------------------------------------
 * The rule (UniGen.beam_search, models/beam.py: BeamSearch) is transformers' GenerationMixin._beam_search with do_sample=False:
 *   - per prompt (a "group") B = num_beams running beams; initial running scores [0, -1e9, ..., -1e9];
 *   - every step takes K = max(2, 1 + number of eos ids) * B candidates per group from the B * V values
 *     log_softmax(logits[b])[e] + running_score[b], in descending order;
 *   - a candidate whose token is an eos id never joins the running set; it enters the group's finished pool only when it ranks among
 *     the first B of the K; the next running beams are the first B non-eos candidates;
 *   - a finished hypothesis scores sum_logprobs / (generated_length ** length_penalty), the eos token counted; the pool keeps the
 *     best B of old and new;
 *   - after every step a group asks whether a running beam can still beat its pool: best running score / (length ** length_penalty)
 *     > the pool's worst score (an incomplete pool counts as -1e9: always), with length = the generated length so far, or
 *     max_new_tokens for early_stopping "never" with length_penalty > 0; once the answer is no it stays no and nothing enters that
 *     pool any more; with early_stopping True a full pool is closed at once, whatever the bound says;
 *   - the call ends when no group can improve, or (early_stopping True) every pool is full, or at max_new_tokens, where every
 *     candidate ends and the first B of each group meet the pool like any finished hypothesis;
 *   - num_beams = 1 is greedy search: a prompt's first hypothesis ends it (early_stopping True, whatever was passed);
 *   - a prompt's output rows are its num_return_sequences <= B best hypotheses, best first, padded behind their eos with pad_token_id
 *     (default: the first eos id).
 * ug_beam_candidates: logits fp32 [G*B][ld], V <= ld (entries V..ld-1 are never read); beam_scores fp32 [G*B];
 *   outputs cand_score fp32 [G][K], cand_beam int32 [G][K] (0..B-1 inside the group), cand_token int32 [G][K]; lse fp32 [G*B] or null.
 *   Per row b: s[e] = bf16round(logit[e]) (the head rounding of the precision contract, what ug_text_pick picks from), m = max s,
 *   lse = m + log(sum exp(s[e] - m)); a NaN entry contributes nothing and is no candidate, a -inf entry contributes 0 and is no
 *   candidate (a +inf entry makes lse +inf and the row supplies no candidates; a row without a finite entry has lse -inf).
 *   Per candidate: total = (s[e] - lse[b]) + beam_scores[b] in fp32, in exactly this order.  A row with beam_scores[b] <= -1e8 is a
 *   dead beam and supplies no candidates.  Output order: total descending, equal totals by flat index b*V + e ascending; slots the
 *   live beams cannot fill hold (-inf, -1, -1).
 *   lse is summed per bf16 pattern (count * exp(value - m), fp64 accumulation, patterns in descending order): bit-reproducible, and a
 *   row's lse bits depend on that row's logits alone -- two rows with equal logits and equal scores tie exactly, the lower beam first.
 *   Limits, refused with a status before anything is touched: 1 <= B <= 8, 1 <= G*B <= 32, 1 <= K <= 64, 1 <= V <= 262144, ld >= V,
 *   null pointers (lse excepted).  ws: ug_beam_candidates_ws_bytes(G, B, V, K) bytes, 16-byte aligned, need not be initialised
 *   (csrc/beam_plan.h: 256 KiB of histogram per row + the rows' lists); > 0, or a negative status outside the limits.
 * ug_beam_kv_reorder: k_ptrs / v_ptrs device arrays of n_layers pointers to bf16 caches [R][HKV][Tmax][hd] (DecodeState's layout,
 *   16-byte aligned); parent int32 [R] in device memory, absolute row indices; len the state's device int; spare bf16
 *   [2*n_layers][R][HKV][span][hd].  For every layer, both caches, every row r, head h and position t in
 *   [first, min(*len, first + span)): cache[r][h][t] = the old cache[parent[r]][h][t]; every other byte of every cache is unchanged.
 *   Two launches: gather into spare for rows with parent[r] != r, then write back; 16 bytes per lane; nothing is read on the host.  A
 *   parent outside [0, R) moves nothing.  Limits: hd == 128, 1 <= R <= 32, first >= 0, span >= 1, first + span <= Tmax,
 *   1 <= n_layers <= 1024, non-null pointers. */
int ug_beam_candidates_ws_bytes(int64_t G, int64_t B, int64_t V, int64_t K);
int ug_beam_candidates(const float* logits, int64_t ld, int64_t G, int64_t B, int64_t V, const float* beam_scores, int64_t K, void* ws,
                       float* cand_score, int* cand_beam, int* cand_token, float* lse, hipStream_t stream);
int ug_beam_kv_reorder(const void* const* k_ptrs, const void* const* v_ptrs, int64_t n_layers, int64_t R, int64_t HKV, int64_t Tmax,
                       int64_t hd, const int* parent, const int* len, int64_t first, void* spare, int64_t span, hipStream_t stream);

/* ---- optimizer ------------------------------------------------------------------------------- */
/* replaces: torch.optim.AdamW.step (training/train.py:324-330,780) over one flat fp32 segment; also
 * refreshes the bf16 compute copy (p_bf16 may be null).  grads are multiplied by grad_scale first. */
int ug_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                  int max_blocks /* 0 = fill the chip; > 0 = grid cap for an update overlapped with other kernels */,
                  hipStream_t stream);
/* ug_adamw_flat with a device-side gradient factor: grads are multiplied by grad_scale * *grad_factor (one fp32 product, formed
 * once per workgroup).  grad_factor: device address of one fp32, 4-byte aligned -- word [1] or [2] of ug_clip_finish's result
 * block -- read when the kernel runs, so no host synchronisation sits between the norm and the update.  Null = ug_adamw_flat
 * exactly (same kernels, same bits). */
int ug_adamw_flat_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                      const float* grad_factor, int max_blocks, hipStream_t stream);

/* ---- gradient-norm clipping ------------------------------------------------------------------ */
/* replaces: torch.nn.utils.clip_grad_norm_ behind accelerator.clip_grad_norm_ (training/train.py:777), norm_type 2.
 * Span table (device, int64, 8-byte aligned): n_spans pairs {byte address of the span's first fp32, element count}.  An address
 * is a multiple of 4 and need NOT be a multiple of 16, a count is any value >= 0 (64-bit: spans beyond 2^31 elements are fine);
 * spans must not overlap.  1 <= n_spans <= 65535.
 *
 * ug_sumsq_spans_f32: partials[b] (device, fp64, `blocks` values, 1 <= blocks <= 4096 = the grid) = the sum of squares of the
 * elements workgroup b read, over all spans.  Plain stores, every slot written on every call, no atomics, fixed summation
 * order: the same bits on every run for the same table, data and `blocks`.  accum 0 = fp64 accumulation (what ships);
 * 1 = fp32 chains of 32 elements flushed into fp64 (kept for measurement, tools/clip_bench.py). */
int ug_sumsq_spans_f32(const int64_t* spans, int64_t n_spans, double* partials, int blocks, int accum, hipStream_t stream);
/* One workgroup: sum = partials[0] + ... + partials[n_partials - 1] in that order in fp64 (1 <= n_partials <= 8192; a caller
 * may append slots of its own, e.g. the squared norm of gradients that took another path), then in fp32, in torch's order:
 *   result[0] total_norm = float(sqrt(sum) * |grad_scale|)          (the norm of grad_scale * g)
 *   result[1] clip_coef  = min(1, max_norm / (total_norm + 1e-6))   (NaN stays NaN, as torch.clamp keeps it)
 *   result[2] grad_scale * clip_coef                                (the factor an optimizer applies to the raw gradients)
 *   result[3] 1.0 if total_norm is inf or NaN, else 0.0
 *   result[4..5] the fp64 sum itself, result[6..7] zero.
 * result: device, 8 fp32 words, 16-byte aligned.  max_norm and grad_scale must not be NaN. */
int ug_clip_finish(const double* partials, int64_t n_partials, float max_norm, float grad_scale, float* result, hipStream_t stream);
/* g *= *coef over the span table (same layout as above), in place.  *coef == 1.0f: the kernel returns without touching the
 * gradients (bit-identical to multiplying by 1.0).  blocks: the grid, 0 = whole chip. */
int ug_scale_spans_f32(const int64_t* spans, int64_t n_spans, const float* coef, int blocks, hipStream_t stream);

/* ---- data-parallel gradient exchange staging ------------------------------------------------ */
/* replaces: the bucket copies + fp32 all-reduce of torch DistributedDataParallel's reducer behind
 * accelerator.backward (training/train.py:492,775).  A bucket of the flat fp32 gradient buffer is packed as
 * bf16(g * scale) (scale = 1 / world size: the mean is formed by the SUM all-reduce), exchanged by RCCL on the side
 * stream, and unpacked back in place.  Buffers 16-byte aligned; tails of any length. */
int ug_grad_pack_bf16(const float* in, void* out_bf16, int64_t n, float scale, hipStream_t stream);
/* Clear n_ranges spans of one fp32 buffer in ONE launch: ranges (device, int64) = {first element, element count} pairs, both
 * multiples of 4; max_len = the longest count (sizes the grid).  Start of a gradient pass: the small accumulating gradients
 * (norm weights, biases) that lie between the big "first write overwrites" matrices of the flat buffer -- 85 fill launches
 * per step otherwise (torch's `zero_grad(set_to_none=False)` semantics for those tensors, reference training/train.py:773). */
int ug_zero_ranges_f32(float* buf, const int64_t* ranges, int64_t n_ranges, int64_t max_len, hipStream_t stream);
int ug_grad_unpack_bf16(const void* in_bf16, float* out, int64_t n, hipStream_t stream);
/* bf16 on the wire, fp32 arithmetic: after an all-to-all of the packed bucket, `shards` holds every rank's bf16 copy of THIS
 * rank's slice (shard r at shards + r * stride elements, stride % 8 == 0).  out[i] = bf16(scale * sum_r float(shards[r][i])),
 * summed in fp32 in rank order (identical on every rank), rounded once; the slices are then all-gathered and unpacked. */
int ug_grad_sum_shards_bf16(const void* shards_bf16, int world, int64_t stride, void* out_bf16, int64_t n, float scale,
                            hipStream_t stream);

/* ---- data-parallel gradient exchange over RCCL ------------------------------------------------ */
/* replaces: the DistributedDataParallel reducer behind accelerator.prepare / accelerator.backward (training/train.py:492,775)
 * for hosts that do not bring torch.distributed (the shipped Python host keeps torch.distributed as its default transport and
 * switches to these entry points with UNIGEN_DDP_TRANSPORT=ug_comm).  One ug_comm per rank = one process per GPU.  RCCL is
 * resolved with dlopen at ug_comm_init time (the copy already mapped into the process, else UNIGEN_RCCL_LIB / librccl.so.1).
 *   ug_comm_unique_id       rank 0 creates the 128-byte rendezvous id; the host hands it to every rank (any side channel)
 *   ug_comm_init            ncclCommInitRank + the communicator's side stream, events and bf16 staging for buckets of up to
 *                           max_bucket_elems elements
 *   ug_comm_allreduce_bucket  MEAN over ranks of grad[0..n) in place.  Ordered after everything queued on `producer` at the
 *                           time of the call (an event is recorded there); pack / collective(s) / unpack run on the
 *                           communicator's side stream, so the producer stream continues with backward.  mode:
 *                             UG_COMM_FP32          ncclAllReduce(fp32, AVG): DDP's arithmetic, 4 bytes per element on the links
 *                             UG_COMM_BF16_FP32ACC  bf16 on the links, fp32 sum in rank order, one final bf16 rounding
 *                             UG_COMM_BF16          bf16(g / world) summed by ncclAllReduce in bf16 (least accurate)
 *                             UG_COMM_FP32_RSAG     fp32 as ncclReduceScatter(AVG) + ncclAllGather in place (+ a short all-reduce
 *                                                   for the tail that does not divide by the world size)
 *   ug_comm_allgather       recv[r * bytes_per_rank ...] = rank r's `send` bytes, on the communicator's side stream, ordered
 *                           after `producer` like a bucket (the per-token embedding-lookup gradient rows and their ids: the
 *                           dense head gradient of the tied table is exchanged right after the head's backward, the lookups'
 *                           few rows at the end, training/train.py:602-609 are the lookups)
 *   ug_comm_wait            `consumer` waits for every bucket issued so far (end of backward, before clipping / the optimizer)
 *   ug_comm_bytes_on_wire   payload handed to the collectives since init (reporting)
 * No call synchronises the host.  Buckets must be 16-byte aligned. */
typedef struct ug_comm ug_comm;
#define UG_COMM_ID_BYTES 128
#define UG_COMM_FP32 0
#define UG_COMM_BF16_FP32ACC 1
#define UG_COMM_BF16 2
#define UG_COMM_FP32_RSAG 3
int ug_comm_unique_id(void* id128);
int ug_comm_init(ug_comm** out, int world, int rank, const void* id128, int64_t max_bucket_elems);
int ug_comm_allreduce_bucket(ug_comm* comm, float* grad, int64_t n, int mode, hipStream_t producer);
int ug_comm_allgather(ug_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, hipStream_t producer);
int ug_comm_wait(ug_comm* comm, hipStream_t consumer);
int ug_comm_destroy(ug_comm* comm);
int64_t ug_comm_bytes_on_wire(const ug_comm* comm);

/* ---- MAGVITv2 tokenizer (fp32, NHWC) ------------------------------------------------------- */
/* replaces: torch.nn.Conv2d in VQGANEncoder/Decoder, ResnetBlock, Downsample (asymmetric pad via
 * pad_top/pad_left = 0, stride 2), Upsample (nearest-2x folded into the load), magvitv2.py:90-178,
 * 319-408; common_modules.py:30-93,301-360.  w_packed: [k*k][Cin][cout_pad] fp32. */
int ug_conv2d_f32(const float* x, const float* w_packed, const float* bias, const float* residual, float* y,
                  int64_t B, int Hin, int Win, int Cin, int Cout, int cout_pad, int ksize, int stride,
                  int pad_top, int pad_left, int Hout, int Wout, int upsample2x, hipStream_t stream);
/* The same convolution at fp32 accuracy on the f16 matrix cores.  Each operand tensor is scaled by the power of two that
 * puts its largest magnitude into [2^14, 2^15), every scaled value split into two fp16 terms (a = a1 + a2, 23 of fp32's 24
 * significand bits) and a.b summed from the three partial products a1b1 + a1b2 + a2b1 in fp32 accumulators; the epilogue
 * undoes the scales.  Error vs fp64 equals a plain fp32 accumulation's (3.5e-7 relative at K = 1152; the reference's own GPU
 * path runs these convs with TF32 operands, 7.7e-4); 3/16 the MFMA cost of ug_conv2d_f32.
 * ug_conv_split_weights turns ug_conv2d_f32's packed weights into the split tile image once per weight version: w_split
 * holds 2 * taps * roundup(Cin, 32) * cout_pad 16-bit elements (a ragged last 32-channel slab is zero-filled) + 8 more
 * whose first four bytes record max|w| (computed here).  x_amax: device fp32, ANY upper bound of max|x| of the activation
 * tensor (ug_amax_f32 computes the exact one; a constant bound is as good -- only its binade is used); null = unscaled
 * (|x| < 65504 assumed, values saturate otherwise).  Needs Cin % 4 == 0, Cout % 4 == 0, cout_pad % 128 == 0; same geometry
 * arguments and the same reference call sites as ug_conv2d_f32. */
int ug_conv_split_weights(const float* w_packed, uint16_t* w_split, int taps, int Cin, int cout_pad, hipStream_t stream);
int ug_amax_f32(const float* x, int64_t rows, int64_t cols, int64_t ld, float* out_amax, hipStream_t stream);
/* the same into a slot the caller keeps zeroed (no memset ahead of the launch; ABI v5) */
int ug_amax_f32_into_zeroed(const float* x, int64_t rows, int64_t cols, int64_t ld, float* out_amax, hipStream_t stream);
int ug_conv2d_split(const float* x, const float* x_amax, const uint16_t* w_split, const float* bias, const float* residual,
                    float* y, int64_t B, int Hin, int Win, int Cin, int Cout, int cout_pad, int ksize, int stride,
                    int pad_top, int pad_left, int Hout, int Wout, int upsample2x, double* out_stats, int out_groups,
                    hipStream_t stream);   /* out_stats: as ug_conv3x3_split (needs Hout * Wout % 128 == 0), or null */
/* 3x3 / stride 1 / pad 1 convolution (every conv1/conv2 of ResnetBlock, conv_in/conv_out of the middle stacks:
 * common_modules.py:301-360, magvitv2.py:90-178) with the split operands of ug_conv2d_split and the 10 x 18 input
 * patch of an 8 x 16 output block resident in LDS for all nine taps.  With gn_mu_rstd (from ug_groupnorm_stats on
 * the same x) the load applies y = swish?(GroupNorm(x)) first -- the `conv(nonlinearity(norm(x)))` pattern of
 * ResnetBlock.forward -- so the normalised tensor never exists in HBM; zero padding applies to the normalised tensor,
 * as in the reference.  x_amax then bounds the NORMALISED tensor. */
int ug_conv3x3_split(const float* x, const float* x_amax, const uint16_t* w_split, const float* bias, const float* residual,
                     float* y, int64_t B, int H, int W, int Cin, int Cout, int cout_pad, const float* gn_mu_rstd,
                     const float* gn_gamma, const float* gn_beta, int gn_groups, int gn_swish, double* out_stats, int out_groups,
                     hipStream_t stream);
/* out_stats (or null): [B][out_groups][2] fp64 + one more 8-byte slot, ZEROED BY THE CALLER -- the sum and the sum of squares of
 * the stored y per (image, group), gathered in the convolution's epilogue with the arithmetic of ug_groupnorm_stats, for the
 * GroupNorm that consumes y (ResnetBlock.forward, common_modules.py:308-335: norm2 reads conv1's output, the next block's norm1
 * reads conv2's output + shortcut); ug_groupnorm_finalize turns them into (mean, rstd) without another pass over y.  The
 * trailing slot receives max|y| as an fp32 in its first four bytes (what ug_amax_f32 computes): the x_amax of a following split
 * convolution that has no GroupNorm on its load path (Downsample, nin_shortcut: common_modules.py:86-93,321-334). */
int ug_groupnorm_finalize(const double* stats, float* mu_rstd, int64_t B, int64_t HW, int C, int groups, float eps,
                          hipStream_t stream);
/* GroupNorm statistics only: stats_ws [B][groups][2] fp64 scratch, mu_rstd [B][groups][2] fp32 = (mean, rstd),
 * rounded as ug_groupnorm_swish rounds them (common_modules.py:19-27). */
int ug_groupnorm_stats(const float* x, double* stats_ws, float* mu_rstd, int64_t B, int64_t HW, int C, int groups,
                       float eps, hipStream_t stream);
/* replaces: SigLipAttention.forward (siglip_encoder.py:196-260): softmax(q k^T * scale) v per (image, head) in one
 * flash-style kernel, fp32 in / out, both contractions on the scaled two-way f16 split (fp32-accurate), scores never leave
 * registers.  qkv: rows (b*T + t), q | k | v blocks of H*head_dim columns, row stride ld; qkv_amax: device fp32 bound of
 * max|qkv| (ug_amax_f32) or null; out [B*T, H*head_dim] at row stride ldo.  head_dim % 4 == 0, <= 80. */
int ug_siglip_attn_f32(const float* qkv, int64_t ld, const float* qkv_amax, float* out, int64_t ldo, int64_t B, int64_t T,
                       int H, int head_dim, float scale, hipStream_t stream);
/* ug_linear_f32 on the same split-f16 contraction (SigLIP q/k/v/out_proj, fc1/fc2: siglip_encoder.py:196-199,
 * 250-259): y = act(x W^T + bias) + residual with W^T packed as ug_conv2d_f32 weights of a 1x1 conv ([1][K][n_pad])
 * and split by ug_conv_split_weights. */
int ug_linear_split(const float* x, int64_t ldx, const float* x_amax, const uint16_t* w_split, const float* bias,
                    const float* residual, int64_t ldres, float* y, int64_t ldy, int64_t M, int64_t N, int64_t K, int n_pad,
                    int act, hipStream_t stream);
/* batched fp32 GEMM on the same kernel (AttnBlock bmm's, common_modules.py:190-214) */
int ug_gemm_f32(const float* A, int64_t lda, int64_t stride_a, const float* B, int64_t ldb, int64_t stride_b,
                int b_is_nk, float* C, int64_t ldc, int64_t stride_c, int64_t M, int64_t N, int64_t K,
                int64_t batch, float alpha, hipStream_t stream);
/* ug_gemm_f32 over a two-level batch z = outer * batch_in + inner (operand z starts inner * s*_in + outer * s*_out
 * elements into its tensor): all heads of all images of SigLipAttention in one launch (siglip_encoder.py:196-230). */
int ug_gemm_f32_nested(const float* A, int64_t lda, int64_t sa_in, int64_t sa_out, const float* B, int64_t ldb,
                       int64_t sb_in, int64_t sb_out, int b_is_nk, float* C, int64_t ldc, int64_t sc_in, int64_t sc_out,
                       int64_t M, int64_t N, int64_t K, int64_t batch_in, int64_t batch_out, float alpha,
                       hipStream_t stream);
/* replaces: Normalize = GroupNorm(32, eps 1e-6) (+ swish), common_modules.py:19-27 */
int ug_groupnorm_swish(const float* x, const float* gamma, const float* beta, float* y, double* stats_ws,
                       int64_t B, int64_t HW, int C, int groups, float eps, int apply_swish, hipStream_t stream);
/* in-place softmax(scale * x) over the first `cols` columns of each row; columns [cols, min(ld, roundup(cols, 4))) are
 * set to zero so the probabilities can be contracted over a 16-byte-aligned width. */
int ug_softmax_rows_f32(float* x, int64_t rows, int64_t cols, int64_t ld, float scale, hipStream_t stream);
/* ---- SigLIP ViT (fp32, frozen; reference models/multimodal_encoder/siglip_encoder.py:152-309) ---- */
/* y = act(x W^T + bias) + residual, W [N][K] as nn.Linear stores it; act 1 = gelu_pytorch_tanh.
 * replaces: q/k/v/out_proj, fc1/fc2 (siglip_encoder.py:196-199,250-259); the 14x14/14 patch embedding is
 * ug_conv2d_f32 with ksize 14, stride 14. */
int ug_linear_f32(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias,
                  const float* residual, int64_t ldres, float* y, int64_t ldy, int64_t M, int64_t N, int64_t K,
                  int act, hipStream_t stream);
/* replaces: nn.LayerNorm(eps 1e-6) (siglip_encoder.py:267-269) */
int ug_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int64_t cols,
                     float eps, hipStream_t stream);
/* Backward pieces of the tower for the UNFROZEN case (reference models/unigen.py:111 freeze=False; training/train_w_clip_vit.py:
 * 282,311-312).  The contractions of the backward run on ug_gemm_f32 / ug_gemm_f32_nested (exact fp32); these are the row-wise /
 * element-wise derivatives:
 *   ug_layernorm_bwd_f32      dx = [dres_in +] LayerNorm'(dy) (statistics recomputed from x); dgamma, dbeta ACCUMULATE
 *   ug_gelu_tanh_f32          dy_or_null == null: out = gelu_pytorch_tanh(pre); else out = dy * gelu'(pre)
 *   ug_softmax_bwd_rows_f32   in place on dP: dS = scale * P * (dP - sum_j dP_j P_j), padding columns [cols, ld) zeroed
 *   ug_colsum_f32             out[c] += sum_r x[r, c]   (bias / position-embedding gradients) */
int ug_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* dres_in, float* dx, float* dgamma,
                         float* dbeta, int64_t rows, int64_t cols, float eps, hipStream_t stream);
int ug_gelu_tanh_f32(const float* pre, const float* dy_or_null, float* out, int64_t n, hipStream_t stream);
int ug_softmax_bwd_rows_f32(const float* P, float* dP, int64_t rows, int64_t cols, int64_t ld, float scale, hipStream_t stream);
int ug_colsum_f32(const float* x, int64_t ld, float* out, int64_t rows, int64_t cols, hipStream_t stream);
/* out[z][c][r] = in[z][r][c] for z < batch (operands z * stride apart); output rows ld_out >= rows long, their tail zero-filled:
 * the transposed activations / probabilities are the row-major A operand of the weight-gradient and dK / dV contractions */
int ug_transpose_f32(const float* in, int64_t ld_in, int64_t stride_in, float* out, int64_t ld_out, int64_t stride_out,
                     int64_t rows, int64_t cols, int64_t batch, hipStream_t stream);
int ug_nchw_to_nhwc(const float* in, float* out, int64_t B, int C, int64_t HW, int c_pad, hipStream_t stream);
int ug_nhwc_to_nchw(const float* in, float* out, int64_t B, int C, int64_t HW, int c_pad, hipStream_t stream);
/* replaces: LFQuantizer.get_indices / get_codebook_entry, magvitv2.py:210-230 */
int ug_lfq_pack(const float* z, int64_t ldz, int64_t* idx, int64_t n, int nbits, hipStream_t stream);
int ug_lfq_unpack(const int64_t* idx, float* z, int64_t n, int nbits, int* err_flag, hipStream_t stream);

/* ---- hardware probes (test-only: dump raw MFMA / LDS-transpose lane layouts) ---------------- */
int ug_probe_layouts(float* out, int64_t n_floats, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIGEN_HIP_H */
