/*
 * moviigen_hip.h — C-ABI of libmoviigen_hip.so, the MI355X (gfx950) kernels behind the
 * MoviiGen1.1 / Wan2.1-14B T2V denoising hot path.
 *
 * The reference (ZulutionAI/MoviiGen1.1) is pure Python + torch and has no FFI of its own;
 * every arithmetic step of its hot path is a call into a third-party native kernel
 * (cuBLAS / flash_attn / ATen elementwise / cuDNN).  Each entry point below names the
 * reference call site (file:line under the reference tree) whose arithmetic it replaces.
 * The Python side that binds these with ctypes is moviigen1.1_amd/wan/backend/lib.py; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 (MG_OK) or a negative error code; nothing throws, nothing
 *     allocates, nothing synchronises: work is enqueued on `stream` (a hipStream_t passed as
 *     void*; NULL = the legacy default stream).
 *   - all pointers are DEVICE pointers owned by the caller.  bf16 travels as uint16_t.
 *   - `ld*` arguments are row strides in ELEMENTS.  Row-major everywhere.
 *   - no torch types, no C++ types in any signature.
 */
#ifndef MOVIIGEN_HIP_H
#define MOVIIGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_ERR_ARG (-1)    /* null pointer / bad enum */
#define MG_ERR_SHAPE (-2)  /* unsupported shape or alignment */
#define MG_ERR_LAUNCH (-3) /* hipGetLastError() != hipSuccess after launch */
#define MG_ERR_UNAVAILABLE (-4) /* librccl could not be bound at run time (collective entry points only) */
#define MG_ERR_COMM (-5) /* an RCCL call returned an error */

/* library identification: returns a static string "moviigen_hip <abi> gfx950" */
const char* mg_version(void);
/* ABI revision, bumped on any signature change */
int mg_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * DiT — token-wise HBM-bound kernels
 * ---------------------------------------------------------------------------------------- */

/* WanLayerNorm (eps, no affine) in fp32 followed by the AdaLN modulation, or by an affine
 * weight/bias (norm3).  Replaces wan/modules/model.py:89-99 + :299,:307 (norm1/norm2 +
 * `*(1+scale)+shift`), :306 (norm3, elementwise_affine) and :340-342 (head norm+modulate).
 *   y = (x-mean)*rsqrt(var+eps);  if round_norm_bf16: y = bf16(y)   [block 0: x is bf16 there,
 *   model.py:99 `.type_as(x)`];  out = add_one ? y*(1+scale)+shift : y*scale+shift
 *   scale/shift: fp32 [dim] or NULL (=> 1 / 0).  out: bf16 (out_f32=0) or fp32 (out_f32=1).
 * dim % 4 == 0, dim <= 8192. */
int mg_ln_modulate(const float* x, int64_t ldx, int64_t rows, int dim, const float* scale,
                   const float* shift, int add_one, float eps, int round_norm_bf16, void* out,
                   int out_f32, int64_t ldo, void* stream);

/* Step cache (not the reference's arithmetic, opt-in).
 *
 * mg_step_resid_capture_f32: r[i] <- x[i] - xin[i], i < n, ONE fp32 subtract per element, behind the last block of a
 * computed step (x the residual stream there, xin the stream as it stood behind the patch embedding).  With stats != NULL
 * the same pass reduces stats[0] = sum |r_new[i] - r_old[i]| and stats[1] = sum |r_old[i]| (r_old = what r held): each
 * difference and absolute value in fp32, widened and accumulated in fp64.  The grid is fixed, the per-workgroup fp64 sums go
 * to `partials` (mg_step_resid_partials_bytes() bytes OWNED BY THE CALLER, 8-byte aligned, no initial value needed) and a
 * second one-lane launch adds them in index order: the same inputs give the same 16 bytes, no atomics.  stats == NULL: no
 * reduction, r is not read, partials is not touched (and may be NULL).
 *   n >= 1, any value (scalar tail).  r, x, xin 16-byte aligned, stats 8-byte aligned: else MG_ERR_SHAPE.
 *
 * mg_resid_ln_modulate_f32: out = LN(x + r) * (1 + scale) + shift in fp32, x + r one fp32 add per element formed in
 * registers: bit for bit mg_ln_modulate(add_one = 1, round_norm_bf16 = 0, out_f32 = 1) of the fp32 sum (the two kernels share
 * one body), without the three passes over the stream (add, write, re-read).  x and r are only read.  The only full-size
 * pass of a skipped step.  dim % 4 == 0, dim <= 8192, ld* % 4 == 0 and >= dim, all pointers 16-byte aligned. */
int64_t mg_step_resid_partials_bytes(void);
int mg_step_resid_capture_f32(float* r, const float* x, const float* xin, int64_t n, double* stats, double* partials,
                              void* stream);
int mg_resid_ln_modulate_f32(const float* x, int64_t ldx, const float* r, int64_t ldr, int64_t rows, int dim,
                             const float* scale, const float* shift, float eps, float* out, int64_t ldo, void* stream);

/* WanRMSNorm over the whole `dim` vector (fp32 math, result rounded to bf16, then * weight in
 * fp32) and optional 3-axis RoPE on adjacent pairs, output bf16.
 * Replaces wan/modules/model.py:70-86 (+:139-140, :168-169) and rope_apply model.py:39-67 /
 * wan/distributed/xdit_context_parallel.py:23-62 (rank slice = pos0).
 *   rope_cs: NULL (no RoPE: cross-attention q/k) or float2 (cos,sin) tables laid out as
 *            [F][c0] ++ [H][c1] ++ [W][c1] with c = head_dim/2, c1 = c/3, c0 = c - 2*c1
 *   token index of row r is pos0 + r, decomposed (f,h,w) row-major over the F*H*W grid;
 *   rows with token index >= F*H*W are passed through un-rotated (padding, model.py:61).
 *   out_scale: the fp32 result is multiplied by it before the (single) rounding to bf16; 1 = the reference value.
 *            WanModel.forward passes softmax_scale*log2(e) for q, so that mg_attn_fwd_bf16_hd128_prescaled needs no
 *            per-score multiply (flash_attn applies softmax_scale to the fp32 scores: same product, one rounding
 *            either way, taken at a different point).
 * dim % 8 == 0, dim <= 8192, head_dim % 2 == 0, dim % head_dim == 0, ldx/ldo % 8 == 0. */
int mg_rmsnorm_rope_bf16(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo,
                         int64_t rows, int dim, const float* weight, float eps, int head_dim,
                         const float* rope_cs, int F, int H, int W, int64_t pos0, float out_scale, void* stream);

/* Pack K and/or V (row-major [L][>=heads*128], row strides ldk/ldv; either may be NULL) into the
 * per-64-key-tile operand layout of mg_attn_fwd_bf16_hd128*, nt = ceil(L/64) tiles per head:
 *     kp[head][tile][c = d/8 (16)][row (64)][8]      key 32u + 8a + 4b + j of the tile sits in row 32u + 16b + 4a + j
 *     vp[head][tile][kc = (key%64)/8 (8)][d (128)][8 keys]
 * each tile = one contiguous 16 KiB block = the LDS image (pure LDS-DMA staging, conflict-free
 * ds_read_b128 with immediate offsets); keys >= L are zero.  The K row order is the one the 16x16x32 attention kernel
 * wants (its scores come out as the B operand of P.V without a shuffle); under the A/B library's mg_attn_set_variant(3) the rows are
 * in natural order (row = key % 64) for the A/B partner kernel.  kp/vp: heads*nt*8192 elements each,
 * 16-byte aligned.  No reference counterpart (flash_attn stages K/V inside its kernel). */
int mg_pack_kv_bf16(const uint16_t* k, int64_t ldk, const uint16_t* v, int64_t ldv, int64_t L,
                    int heads, int head_dim, uint16_t* kp, uint16_t* vp, void* stream);

/* ------------------------------------------------------------------------------------------
 * DiT — MFMA kernels
 * ---------------------------------------------------------------------------------------- */

enum {
    MG_EPI_BIAS_BF16 = 0,      /* out_bf16 = bf16(acc + bias)                         nn.Linear */
    MG_EPI_BIAS_GELU_BF16 = 1, /* out_bf16 = bf16(gelu_tanh(bf16(acc + bias)))        ffn.0+ffn.1 */
    MG_EPI_GATE_RESID_F32 = 2, /* out_f32 += bf16(acc + bias) * gate[n] (gate NULL=>1) x + y*e */
    MG_EPI_BIAS_F32 = 3        /* out_f32 = float(bf16(acc + bias))                   patch embed */
};

/* out[M][N] = A[M][K] . W[N][K]^T (+bias, epilogue) — bf16 operands, fp32 MFMA accumulate
 * (v_mfma_f32_32x32x16_bf16).  Replaces every nn.Linear executed under autocast(bf16) on the
 * path: wan/modules/model.py:139-141,155 (q,k,v,o), :168-170,180 (cross q,k,v,o), :267-269
 * (ffn), :451-453 (text_embedding), :445-450 (patch_embedding as a [L,64]x[64,dim] GEMM), with
 * the residual/gate updates of model.py:301-302,306,308-309 fused as epilogue 2.
 * K % 64 == 0, lda/ldw % 8 == 0, A/W 16-byte aligned; ldo % 4 == 0. */
int mg_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                 const float* bias, int64_t M, int N, int K, int epilogue, void* out,
                 int64_t ldo, const float* gate, void* stream);

/* MXFP8 — the opt-in arithmetic of the six per-block DiT linears (WanModel.set_gemm_precision('mxfp8'); never the default).
 * Format: OCP MXFP8 (E4M3).  Along K every 32 consecutive elements share one E8M0 scale byte s, meaning 2^(s-127); elements
 * are OCP e4m3fn (not the MI300 fnuz encoding).  A block with maximum magnitude amax takes e = floor(log2(amax)) - 8 clamped
 * to [-127, 127] (a block of zeros: e = -127), scale byte e + 127, and each element is x * 2^-e, clamped to +-448 FIRST and
 * then rounded to nearest-even into e4m3: it saturates (500 -> 448) where torch's CPU cast returns NaN.  A dequantised
 * element, e4m3 * 2^e, is exactly a bf16 value.  The input must be finite: the format has no code for infinity, and what a NaN
 * or an infinite element turns into (and what it does to its block's scale) is not defined.
 *
 * mg_quant_mxfp8_rows: x bf16 [rows][K] (row stride ldx elements) -> q e4m3 bytes [rows][K] (row stride ldq) and scale bytes
 * [rows][K/32] (row stride lds).  Serves activations (per call) and weights ([N][K], once).  K % 128 == 0, ldx % 8 == 0,
 * ldq % 16 == 0, lds % 4 == 0, x / q 16-byte and scales 4-byte aligned, else MG_ERR_SHAPE. */
int mg_quant_mxfp8_rows(const uint16_t* x, int64_t ldx, int64_t rows, int K, uint8_t* q, int64_t ldq,
                        uint8_t* scales, int64_t lds, void* stream);

/* out[M][N] = A[M][K] . W[N][K]^T on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 operands, fp32
 * accumulation); Aq / Wq and As / Ws are the element and scale bytes mg_quant_mxfp8_rows writes.  bias, epilogue, out, ldo
 * and gate mean exactly what they mean in mg_gemm_bf16 (MG_EPI_*).  M arbitrary, N % 16 == 0, K % 128 == 0, lda / ldw % 16
 * == 0, ldas / ldws % 4 == 0, ldo % 4 == 0, Aq / Wq / out 16-byte and As / Ws 4-byte aligned, else MG_ERR_SHAPE.  One
 * workgroup per output tile, k ascending, no atomics: the result does not depend on the launch. */
int mg_gemm_mxfp8(const uint8_t* Aq, int64_t lda, const uint8_t* As, int64_t ldas, const uint8_t* Wq, int64_t ldw,
                  const uint8_t* Ws, int64_t ldws, const float* bias, int64_t M, int N, int K, int epilogue,
                  void* out, int64_t ldo, const float* gate, void* stream);

/* MXFP8 where the activation is produced (pure additions to ABI 9): the two producers below write the operand of the next
 * mg_gemm_mxfp8 themselves, so the bf16 activation makes no round trip through memory and mg_quant_mxfp8_rows is not run.  Both
 * emit, byte for byte, what mg_quant_mxfp8_rows makes of the bf16 tensor the bf16 form of the same call stores.
 *
 * mg_ln_modulate_mxfp8: mg_ln_modulate with a bf16 output (same arguments, same arithmetic, same rounding to bf16), the bf16 value
 * then written as e4m3 bytes q [rows][dim] (row stride ldq) and scale bytes scales [rows][dim/32] (row stride lds).  out / ldo:
 * the bf16 row as well, or NULL — then it is never written.  dim % 128 == 0, dim <= 8192, ldx % 4 == 0, ldq % 16 == 0,
 * lds % 4 == 0, x / q 16-byte, scales 4-byte and out 8-byte aligned (ldo % 4 == 0), else MG_ERR_SHAPE. */
int mg_ln_modulate_mxfp8(const float* x, int64_t ldx, int64_t rows, int dim, const float* scale, const float* shift,
                         int add_one, float eps, int round_norm_bf16, uint16_t* out, int64_t ldo, uint8_t* q,
                         int64_t ldq, uint8_t* scales, int64_t lds, void* stream);

/* mg_gemm_mxfp8 with the epilogue MG_EPI_BIAS_GELU_BF16 (same operands, same k order, same bits up to the bf16 value
 * bf16(gelu_tanh(bf16(acc + bias)))), that value stored as e4m3 bytes oq [M][N] (row stride ldoq) and scale bytes oscales
 * [M][N/32] (row stride ldos) in place of bf16: ffn.0 feeding ffn.2.  N % 32 == 0, ldoq % 16 == 0, ldos % 4 == 0, oq 16-byte
 * and oscales 4-byte aligned, the rest as mg_gemm_mxfp8, else MG_ERR_SHAPE.  Bytes of a row past N (N/32) are not touched. */
int mg_gemm_mxfp8_gelu_q(const uint8_t* Aq, int64_t lda, const uint8_t* As, int64_t ldas, const uint8_t* Wq, int64_t ldw,
                         const uint8_t* Ws, int64_t ldws, const float* bias, int64_t M, int N, int K, uint8_t* oq,
                         int64_t ldoq, uint8_t* oscales, int64_t ldos, void* stream);

/* softmax(q k^T * scale) v, non-causal, keys >= Lk masked; bf16 in/out, fp32 accumulate,
 * head_dim 128.  Replaces flash_attn_varlen_func as called from
 * wan/modules/attention.py:96-127 (self-attention model.py:146-151, k_lens=seq_lens;
 * cross-attention model.py:176, Lk = 512 unmasked).
 *   q [Lq][>=heads*128] row stride ldq, head h at column h*128; o likewise (row stride ldo)
 *   kp, vp: K and V of the Lk keys packed by mg_pack_kv_bf16(…, L = Lk, …).
 *   workspace: NULL, or mg_attn_workspace_bytes() device bytes OWNED BY THE CALLER, 8-byte aligned, zeroed once before
 *     their first use.  A persistent launch with >= 32 rounds of work per compute unit hands its (query block, head)
 *     items out by ticket through it (+1.35 % at the metric's launch) and leaves it zeroed when it ends, so launches
 *     that are ordered with respect to one another (one stream, or event-ordered) share one workspace; launches that may
 *     overlap need one each.  With NULL the launch uses the static per-XCD partition (same bits).  The library holds no
 *     device memory of its own and never allocates or synchronises inside a launch; a launch with a
 *     workspace is capturable in a hipGraph from its first call. */
int64_t mg_attn_workspace_bytes(void);
/* Queries per work item (256 or 320) of the launch mg_attn_fwd_bf16_hd128* makes for this shape on a persistent grid of n_cu workgroups
 * (the device's CUs rounded down to a multiple of 8, minus reserve_cus rounded up to one): a pure host function, the one place that
 * knows the item size — a launch has heads * ceil(Lq / item) items and takes tickets from 32 rounds of them per workgroup on. */
int mg_attn_hd128_item_queries(int64_t Lq, int64_t Lk, int heads, int prescaled, int n_cu);
int mg_attn_fwd_bf16_hd128(const uint16_t* q, int64_t ldq, const uint16_t* kp, const uint16_t* vp,
                           uint16_t* o, int64_t ldo, int64_t Lq, int64_t Lk, int heads, float scale,
                           void* workspace, void* stream);

/* Same contract for any head_dim <= 256 (head_dim % 8 == 0): the correctness path for model
 * sizes whose head_dim is not 128 (BASELINE.json configs[0]: head_dim 32).  v is NOT transposed:
 * v [Lk][>=heads*head_dim] row stride ldv. */
/* Same, plus the log-sum-exp of the scaled scores per (head, query): lse[head*Lq + q] fp32 (may be
 * NULL = mg_attn_fwd_bf16_hd128).  Ring attention merges per-block results with it. */
int mg_attn_fwd_bf16_hd128_lse(const uint16_t* q, int64_t ldq, const uint16_t* kp, const uint16_t* vp,
                               uint16_t* o, int64_t ldo, float* lse, int64_t Lq, int64_t Lk, int heads,
                               float scale, void* workspace, void* stream);

/* Same operator for a q that ALREADY carries the factor scale*log2(e) (mg_rmsnorm_rope_bf16 with out_scale: the factor
 * enters before q's one rounding to bf16, so nothing is rounded twice) — the form WanModel.forward uses.  With the
 * default kernel a score then IS its base-2 exponent (no per-score multiply-add).  lse may be NULL; when given it is
 * the natural-log log-sum-exp of the true scaled scores, as above.
 * reserve_cus >= 0: compute units the (persistent, one-workgroup-per-CU) launch leaves free, rounded up to a multiple of
 * 8 = one per XCD — room for a kernel on another stream (RCCL's all-to-all of the next head group under sequence
 * parallelism: a persistent workgroup holds its CU's whole register file until the launch ends).  0 = all CUs. */
int mg_attn_fwd_bf16_hd128_prescaled(const uint16_t* q, int64_t ldq, const uint16_t* kp, const uint16_t* vp,
                                     uint16_t* o, int64_t ldo, float* lse, int64_t Lq, int64_t Lk, int heads,
                                     int reserve_cus, void* workspace, void* stream);

/* x[r][c] += float(y[r][c]) * gate[c]: the gated residual update of wan/modules/model.py:301-302,306,308-309 as a
 * stand-alone kernel (x fp32 [rows][dim] row stride ldx; y bf16 row stride ldy; gate fp32 [dim] or NULL = 1).
 * The fused form is MG_EPI_GATE_RESID_F32; this one serves a caller-replaced attention operator
 * (`types.MethodType(fn, block.self_attn)`, wan/text2video.py:97-100).  dim, ldx, ldy % 4 == 0. */
int mg_gate_residual_f32(float* x, int64_t ldx, const uint16_t* y, int64_t ldy, const float* gate, int64_t rows,
                         int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ulysses sequence-parallel exchange layouts (the transposes xfuser / FastVideo's all_to_all_4D do
 * around their all-to-alls: wan/distributed/xdit_context_parallel.py:185-190,
 * scripts/train/model/model_seq.py:232-234,256).  The collective itself is issued by the host
 * (RCCL all_to_all_single on a communication stream); these two kernels produce / consume its
 * contiguous buffers so that ONE exchange carries q, k and v of a head group.
 * ---------------------------------------------------------------------------------------- */

/* send[p][t][i*w + c] = x_i[t][p*cols_per_dest + col0 + c]   (i = 0,1,2 for q,k,v; p < P; t < Lloc; c < w)
 *   q, k, v: [Lloc][>= P*cols_per_dest] bf16, row strides ldq/ldk/ldv (column slices of a fused buffer are fine)
 *   cols_per_dest = (heads / P) * head_dim; [col0, col0 + w) = the head group inside a destination's slice.
 * After all_to_all_single(recv, send) the receive buffer is the row-major [P*Lloc][3w] matrix of ALL tokens
 * (rank order) x (q | k | v) of this rank's heads of the group.  All widths/strides % 8 == 0, 16-byte aligned. */
int mg_sp_pack_qkv_bf16(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                        int64_t ldv, int64_t Lloc, int P, int cols_per_dest, int col0, int w, uint16_t* send,
                        void* stream);

/* the way back: recv[p][t][c] (attention output of source rank p's heads for MY tokens) ->
 * o[t][p*cols_per_src + col0 + c], o row stride ldo. */
int mg_sp_unpack_o_bf16(const uint16_t* recv, int64_t Lloc, int P, int cols_per_src, int col0, int w, uint16_t* o,
                        int64_t ldo, void* stream);

/* the strided block copy both are built on (one-tensor seq<->head exchanges, all_to_all_4D's reshape):
 * dst[b*d_blk + r*d_row + c] = src[b*s_blk + r*s_row + c], b < blocks, r < rows, c < width; strides in elements,
 * everything % 8 == 0, 16-byte aligned. */
int mg_sp_copy_blocks_bf16(const uint16_t* src, int64_t s_blk, int64_t s_row, uint16_t* dst, int64_t d_blk,
                           int64_t d_row, int blocks, int64_t rows, int width, void* stream);

/* ------------------------------------------------------------------------------------------
 * Collectives on an RCCL communicator.  librccl is bound at run time (dlopen, preferring the
 * copy already loaded in the process); without it these return MG_ERR_UNAVAILABLE and nothing else is affected.
 * `comm` is an ncclComm_t.  Everything is enqueued on `stream`; no host synchronisation.
 * Replaces: xfuser get_sp_group().all_gather / xFuserLongContextAttention's all-to-alls
 * (wan/distributed/xdit_context_parallel.py:148,185-190), FastVideo all_to_all_4D / all_gather
 * (scripts/train/model/model_seq.py:232-234,256,780), torch FSDP's per-block parameter all-gather
 * (wan/distributed/fsdp.py:20-31).
 * ---------------------------------------------------------------------------------------- */

/* communicator bootstrap: rank 0 calls mg_comm_unique_id (128 bytes), hands the bytes to every rank by any side
 * channel (the host code uses torch.distributed's object broadcast), every rank calls mg_comm_create. */
int mg_comm_unique_id(void* id128);
int mg_comm_create(const void* id128, int nranks, int rank, void** comm);
int mg_comm_destroy(void* comm);

/* all-to-all of equal chunks: bytes [p*B, (p+1)*B) of `send` go to rank p, the same range of `recv` comes from rank p
 * (B = bytes_per_peer).  Grouped ncclSend/ncclRecv: on the xGMI mesh every pair uses its own link. */
int mg_sp_all_to_all(void* comm, const void* send, void* recv, int64_t bytes_per_peer, void* stream);

/* FastVideo's all_to_all_4D on one bf16 tensor, layout changes included:
 *   seq_to_head != 0 (scatter_dim=2, gather_dim=1): x [rows = L/P][heads*head_dim] (row stride ldx)
 *        -> out [L][(heads/P)*head_dim] contiguous (ldo must equal (heads/P)*head_dim), tokens in rank order;
 *   seq_to_head == 0 (scatter_dim=1, gather_dim=2): x [rows = L][(heads/P)*head_dim] contiguous
 *        -> out [L/P][heads*head_dim] (row stride ldo).
 * workspace: rows * (heads/P or heads... i.e. as many elements as x) bf16, 16-byte aligned. */
int mg_sp_all_to_all_4d_bf16(void* comm, const uint16_t* x, int64_t ldx, int64_t rows, int heads, int head_dim,
                             int seq_to_head, uint16_t* out, int64_t ldo, uint16_t* workspace, void* stream);

/* rank-order concatenation of `bytes` bytes per rank (ncclAllGather): the head-output gather of the SP forward and the
 * per-block parameter gather of the block-sharded (FSDP-style) weights. */
int mg_sp_all_gather(void* comm, const void* send, void* recv, int64_t bytes, void* stream);
int mg_shard_all_gather(void* comm, const void* shard, void* full, int64_t shard_bytes, void* stream);

/* Ring attention (the reference delegates to yunchang inside xFuserLongContextAttention,
 * generate.py:225-229): fold one block's normalised bf16 result `part` [Lq][heads*128] and its lse into
 * the running fp32 result: lse' = logaddexp(lse, lse_j), acc' = acc*exp(lse-lse') + part*exp(lse_j-lse').
 * first != 0 initialises acc/lse_acc from the block; out (bf16, may be NULL) receives acc'. */
int mg_attn_merge_f32(float* acc, int64_t lda, float* lse_acc, const uint16_t* part, int64_t ldp,
                      const float* lse_part, uint16_t* out, int64_t ldo, int64_t Lq, int heads, int first,
                      void* stream);

int mg_attn_fwd_bf16_generic(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk,
                             const uint16_t* v, int64_t ldv, uint16_t* o, int64_t ldo, int64_t Lq,
                             int64_t Lk, int heads, int head_dim, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * DiT — small fp32 pieces (time embedding, head, patch gather, latent algebra)
 * ---------------------------------------------------------------------------------------- */

/* sinusoidal_embedding_1d, wan/modules/model.py:15-25: out[i][0:half]=cos(t_i*w_j),
 * out[i][half:]=sin(..), w_j = 10000^(-j/half), evaluated in fp64, stored fp32.
 * t_dtype: 0 = int64, 1 = float32, 2 = float64 (device pointer, n entries). */
int mg_sinusoid_embed(const void* t, int t_dtype, int n, int dim, float* out, void* stream);

/* y[N] = W[N][K] . f(x[K]) + bias,  f = SiLU if silu_in else identity; all fp32.
 * Replaces time_embedding / time_projection, wan/modules/model.py:455-457,541-545. */
int mg_gemv_f32(const float* W, const float* bias, const float* x, float* y, int N, int K,
                int silu_in, void* stream);

/* out[r][:] = a[r][:] + b[r % period][:]  (modulation + e0, model.py:292-295; head :340). */
int mg_add_rows_f32(const float* a, const float* b, float* out, int rows, int dim, int period,
                    void* stream);

/* fp32 out[M][N] = x[M][K] . W[N][K]^T + bias (Head.head Linear, model.py:342; N <= 64). */
int mg_head_gemm_f32(const float* x, int64_t ldx, const float* W, const float* bias, float* out,
                     int64_t M, int N, int K, void* stream);

/* latent [C][F][H][W] fp32 -> tokens [F*(H/ph)*(W/pw)][C*ph*pw] bf16 with k = (c,i,j), the
 * im2col of the k=s=(1,ph,pw) Conv3d at model.py:445-450,529-531. */
int mg_patchify_bf16(const float* lat, int C, int F, int H, int W, int ph, int pw,
                     uint16_t* out, int64_t ldo, void* stream);

/* tokens [F*Hg*Wg][ph*pw*C] fp32 (channel fastest) -> latent [C][F][Hg*ph][Wg*pw];
 * WanModel.unpatchify, model.py:581-609. */
int mg_unpatchify_f32(const float* tok, int64_t ldt, int C, int F, int Hg, int Wg, int ph, int pw,
                      float* lat, void* stream);

/* out[i] = c0*x0[i] + c1*x1[i] + c2*x2[i] + c3*x3[i]  (NULL terms skipped).  CFG combine
 * (wan/text2video.py:245-246) and every UniPC / DPM-Solver++ update
 * (wan/utils/fm_solvers_unipc.py:315-332,455-485,600-627; fm_solvers.py:461-470,533-541) are
 * linear combinations with host-side scalar coefficients. */
int mg_lincomb4_f32(float* out, int64_t n, const float* x0, float c0, const float* x1, float c1,
                    const float* x2, float c2, const float* x3, float c3, void* stream);

/* Classifier-free guidance in the reference's operation order: out = uncond + g*(cond - uncond)
 * (wan/text2video.py:245-246). */
int mg_cfg_combine_f32(float* out, const float* uncond, const float* cond, float guide_scale,
                       int64_t n, void* stream);

/* Guidance options (not the reference's arithmetic, opt-in): CFG-Zero* and guidance rescale as three launches
 * behind the pair of predictions of a guided step.  None of them reads on the host, allocates or keeps state: capturable.
 *
 * mg_cfg_stats_f32: stats[5] = (sum u, sum c, sum u^2, sum c^2, sum u c) over the n elements of uncond (u) and cond (c).  Every
 * element is widened to fp64 and multiplied there (the product of two fp32 values is exact in fp64): only the additions round.
 * The grid is fixed, a lane's elements and their order are a function of n alone, the per-workgroup sums go to `partials`
 * (mg_cfg_stats_partials_bytes() bytes OWNED BY THE CALLER, no initial value needed) and a second launch adds them in index
 * order: the same inputs give the same 40 bytes, no atomics.  The inputs are only read.
 *   n >= 1, any value (scalar tail).  uncond, cond 16-byte aligned, stats, partials 8-byte aligned: else MG_ERR_SHAPE.
 *
 * mg_cfg_coef_f32: coef[2] = (a_u, a_c), the coefficients of the guided prediction p = a_u u + a_c c, from stats: one lane,
 * every operation in fp64 without contraction, one rounding to fp32.
 *   s = zero_star ? S_uc / (S_uu + 1e-8) : 1            (CFG-Zero*: the projection of c on u)
 *   a_u = s (1 - g), a_c = g                            (= s u + g (c - s u))
 *   rescale > 0:  mean_p = (a_u S_u + a_c S_c) / n,  E[p^2] = (a_u^2 S_uu + 2 a_u a_c S_uc + a_c^2 S_cc) / n,
 *                 var_p = E[p^2] - mean_p^2,  var_c = S_cc / n - (S_c / n)^2,
 *                 f = rescale sqrt(var_c / var_p) + (1 - rescale), f = 1 when var_p <= 0 or var_c < 0;  a_u, a_c *= f
 *   g finite and rescale in [0, 1]: else MG_ERR_ARG.  n >= 1 (the n of mg_cfg_stats_f32).
 *
 * mg_cfg_combine_coef_f32: out[i] = fma(a_c, cond[i], a_u uncond[i]) with (a_u, a_c) = coef[0..1] read from DEVICE memory:
 * the bits of mg_lincomb4_f32(out, n, uncond, a_u, cond, a_c, ...).  out may be uncond or cond.
 *   n >= 0.  out, uncond, cond 16-byte aligned: else MG_ERR_SHAPE. */
int64_t mg_cfg_stats_partials_bytes(void);
int mg_cfg_stats_f32(const float* uncond, const float* cond, int64_t n, double* stats, double* partials, void* stream);
int mg_cfg_coef_f32(const double* stats, int64_t n, float g, int zero_star, float rescale, float* coef, void* stream);
int mg_cfg_combine_coef_f32(float* out, const float* uncond, const float* cond, int64_t n, const float* coef, void* stream);

/* ------------------------------------------------------------------------------------------
 * umT5 text encoder glue (the GEMMs are mg_gemm_bf16, the T5LayerNorm is
 * mg_rmsnorm_rope_bf16 without RoPE).  Reference wan/modules/t5.py, model in bf16.
 * ---------------------------------------------------------------------------------------- */

/* token_embedding lookup, t5.py:273,289: out[i][:] = table[clamp(ids[i])][:]; dim % 8 == 0. */
int mg_embed_rows_bf16(const uint16_t* table, int64_t vocab, int dim, const int64_t* ids, int n,
                       uint16_t* out, void* stream);

/* bf16 elementwise, n % 8 == 0: mode 0 out = a + b (residual add of bf16 tensors, t5.py:165-166);
 * mode 1 out = a * gelu_tanh(b) (T5FeedForward fc1(x) * gate(x), t5.py:40-44,135). */
int mg_ew_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t n, int mode, void* stream);

/* T5Attention, t5.py:82-113: softmax(q k^T + emb[bucket(j-i)][head]) v, NO 1/sqrt(d) scaling,
 * keys >= Lk masked.  q,k,v [L][heads*head_dim] (row stride ld), rel_emb [num_buckets][heads] bf16,
 * rel_bucket[(j - i) + Lq - 1] (int32, Lq + Lk - 1 entries) = T5RelativeEmbedding bucket of the
 * relative position (t5.py:242-263), tabulated by the host.  head_dim <= 128. */
int mg_t5_attn_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld,
                    const uint16_t* rel_emb, const int* rel_bucket, uint16_t* o, int64_t ldo,
                    int64_t Lq, int64_t Lk, int heads, int head_dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * WanVAE decode (fp32, channels-last activations [T][H][W][C])
 * ---------------------------------------------------------------------------------------- */

/* Generic causal conv as an implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32, exact f32).
 * x: [T][H][W][Cin] channels-last;  w: [Cout][kt][kh][kw][Cin];  out: [T][Ho][Wo][Cout].
 * Temporal taps reach back kt-1 frames: frame index t-(kt-1)+dt; frames < 0 come from
 * `cache` ([tc][H][W][Cin], the last tc <= kt-1 frames of the previous chunk, may be NULL) and
 * are zero before that (CausalConv3d, wan/modules/vae.py:17-36).  Spatial zero padding
 * (kh/2, kw/2).  `up2`: the input is read through a nearest-exact 2x upsample (Ho=2H, Wo=2W;
 * Resample upsample2d/3d, vae.py:66-83,138-141).  residual (same shape as out, may be NULL) is
 * added (ResidualBlock `x + h`, vae.py:220).  kt <= 3, kh and kw in {1, 3} (what WanVAE uses); larger extents return
 * MG_ERR_SHAPE.  So does Cout > 4 that is not a multiple of 4, in every convolution below (rows of out / residual move as float4). */
int mg_vae_conv_f32(const float* x, const float* cache, int tc, int T, int H, int W, int Cin,
                    const float* w, const float* bias, int Cout, int kt, int kh, int kw, int up2,
                    const float* residual, float* out, int mode, void* stream);

/* The 3x3 conv behind a nearest-exact 2x upsample (Resample upsample2d/3d, vae.py:66-83,138-141) as FOUR 2x2 convs of the
 * image itself, one per output parity (py, px): out[t][2y+py][2x+px] reads image rows {y-1, y} (py = 0) or {y, y+1}
 * (py = 1), likewise along x — the 3x3 taps that land on the same image pixel are summed into one weight beforehand.
 * 4/9 of the multiply-adds of mg_vae_conv_f32(up2 = 1) and no per-tap index arithmetic; results agree with it to fp32
 * rounding of the weight sums (not bit for bit).  x [T][H][W][Cin], out [T][2H][2W][Cout], zero padding as the reference's.
 * mg_vae_upconv_fold_weights_f32: w [Cout][1][3][3][Cin] -> wp [4 = 2 py + px][Cout][2][2][Cin] (once per checkpoint). */
int mg_vae_upconv_fold_weights_f32(const float* w, int Cout, int Cin, float* wp, void* stream);
int mg_vae_upconv_phases_f32(const float* x, int T, int H, int W, int Cin, const float* wp, const float* bias, int Cout,
                             float* out, int mode, void* stream);

/* Column-window forms (ABI 9) — one rank's W band of a decode split along W over several GPUs (no reference counterpart: the
 * reference decodes on rank 0 alone, wan/text2video.py:260-261; SURVEY.md 8(e) names the spatial split with one halo pixel per
 * convolution as the natural sharding).  x and cache are the band WITH the neighbours' halo columns: [.][H][W][Cin] where W counts
 * the halos; the launch computes the output columns [col0, col0 + cols) only and writes them compactly — out / residual
 * [T][H][cols][Cout] (phases: out [T][2H][2 cols][Cout]); the zero padding of the reference begins outside [0, W) of x, i.e. at
 * the true image border of an edge rank.  Every output voxel is the same dot product in the same order as in the full launch: the
 * bands of P ranks, side by side, are bit-identical to mg_vae_conv_f32 / mg_vae_upconv_phases_f32 on the whole image. */
int mg_vae_conv_cols_f32(const float* x, const float* cache, int tc, int T, int H, int W, int Cin,
                         const float* w, const float* bias, int Cout, int kt, int kh, int kw,
                         const float* residual, float* out, int col0, int cols, int mode, void* stream);
int mg_vae_upconv_phases_cols_f32(const float* x, int T, int H, int W, int Cin, const float* wp, const float* bias, int Cout,
                                  float* out, int col0, int cols, int mode, void* stream);

/* `mode` of mg_vae_conv_f32 / mg_vae_upconv_phases_f32 — the arithmetic of THAT call (ABI 7: an argument, not a
 * process-global switch; anything else returns MG_ERR_ARG):
 *   MG_VAE_EXACT  = v_mfma_f32_32x32x2_f32, bitwise an fmaf chain — the reference's fp32 arithmetic (vae.py:623,658);
 *   MG_VAE_BF16X3 = split bf16 x 3: every fp32 operand as hi + lo bf16 (16 mantissa bits), W_hi.X_hi + W_hi.X_lo + W_lo.X_hi
 *       on the bf16 MFMA with fp32 accumulation: ~1e-5 relative to the exact mode per convolution, NOT the reference's
 *       arithmetic, opt-in (WanVAE(mode='bf16x3')) and never what bench.py measures.  mg_vae_attn_f32 and convolutions
 *       with Cout <= 4 (the decoder head, on v_mfma_f32_4x4x1_16B_f32) are exact in either mode. */
#define MG_VAE_EXACT 0
#define MG_VAE_BF16X3 1
/* bits 8-9 of `mode` (measurement override, same bits out): the voxel tile of the wide exact convolutions — 0 or
 * MG_VAE_TILE_128 = 128 voxels per workgroup (what the library runs), MG_VAE_TILE_256 = 256 (one workgroup per CU: measured
 * 7 % slower on the 1920x832x81f decode, kept for A/B runs). */
#define MG_VAE_TILE_128 (1 << 8)
#define MG_VAE_TILE_256 (2 << 8)

/* RMS_norm over channels (F.normalize(x, dim=C) * sqrt(C) * gamma, vae.py:39-54), optional SiLU
 * (vae.py:193-197, 466-468).  x,out [rows][C] channels-last; C % 4 == 0, C <= 512, and x, gamma, out 16-byte aligned
 * (they are read and written as float4): anything else returns MG_ERR_SHAPE. */
int mg_vae_rmsnorm_silu_f32(const float* x, const float* gamma, float* out, int64_t rows, int C,
                            int do_silu, void* stream);

/* Single-head attention over one frame's h*w tokens with head dim C (<=512, %32==0), fp32:
 * AttentionBlock, vae.py:247-256 (scaled_dot_product_attention, scale 1/sqrt(C)).
 * qkv [frames][L][3C] (q|k|v), out [frames][L][C]; workspace: caller-owned, mg_vae_attn_workspace_floats(L, C)
 * floats = (min(L, 2048) + C) * roundup(L, 4) — one block of 2048 query rows of the score matrix, which stays
 * inside the Infinity Cache between the three passes, plus V^T — 16-byte aligned (the library never allocates); qkv and
 * out 16-byte aligned too (MG_ERR_SHAPE otherwise: out is written as float4). */
int64_t mg_vae_attn_workspace_floats(int64_t L, int C);
int mg_vae_attn_f32(const float* qkv, float* out, int frames, int64_t L, int C, float* workspace,
                    void* stream);
/* The same attention for Lq <= Lk query rows of a frame against all Lk keys / values held elsewhere (ABI 9; the W-band decode: q =
 * the band's own pixels, k / v = the two halves of the all-gathered k|v tensor): q [frames][Lq][..] row stride ldq, k / v
 * [frames][Lk][..] row stride ldkv, out [frames][Lq][C]; workspace mg_vae_attn_workspace_floats(Lk, C).  A row's bits do not
 * depend on which other rows are computed with it. */
int mg_vae_attn_rows_f32(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, float* out, int frames,
                         int64_t Lq, int64_t Lk, int C, float* workspace, void* stream);

/* z[C][T][H][W] (NCTHW, reference layout) -> channels-last with the latent un-normalisation
 * z/scale1[c] + scale0[c] of vae.py:546-551; and the inverse layout change with clamp(-1,1) for
 * the decoded video (vae.py:661). */
int mg_vae_latent_in_f32(const float* z, const float* mean, const float* inv_std, int C, int T,
                         int H, int W, float* out, void* stream);
int mg_vae_video_out_f32(const float* x, int C, int T, int H, int W, float* out, int t_off,
                         int T_total, void* stream);

/* Decoded video [3][T][H][W] fp32 -> uint8 frames [T][H][W][3] as the reference's cache_video writes
 * them (wan/utils/utils.py:39-47): clamp(lo,hi), (x-lo)/max(hi-lo,1e-5), *255, truncating cast. */
int mg_video_to_u8(const float* video, int T, int H, int W, float lo, float hi, uint8_t* frames,
                   void* stream);

/* One decoded frame [3][H][W] fp32 -> uint8 pixels [H][W][3] as the reference's cache_image writes a t2i result
 * (wan/utils/utils.py:64-91 -> torchvision save_image): clamp(lo,hi), (x-lo)/max(hi-lo,1e-5), *255, +0.5,
 * clamp(0,255), truncating cast. */
int mg_image_to_u8(const float* image, int H, int W, float lo, float hi, uint8_t* pixels, void* stream);

/* The way in (addition to ABI 9; not in the reference, which has no video-to-video start): uint8 RGB frames [T][H0][W0][3] of any size ->
 * the clip [3][T][H][W] fp32 in [-1,1] that mg_vae_video_in_f32 / WanVAE.encode read.  Resize to cover, centre crop, normalise:
 *   s = max(H/H0, W/W0) (fp64);  Hs = max(H, floor(H0 s + 0.5)), Ws = max(W, floor(W0 s + 0.5));  crop origin ((Hs-H)/2, (Ws-W)/2), integer division.
 *   Per axis (in = H0 or W0 samples -> out = Hs or Ws) the antialiased triangle filter with half-pixel centres — what
 *   F.interpolate(mode='bilinear', antialias=True, align_corners=False) computes: scale = in/out, support = max(scale, 1), for output
 *   sample i: c = scale (i + 0.5), taps j in [max(0, int(c - support + 0.5)), min(in, int(c + support + 0.5))) with weight
 *   max(0, 1 - |(j - c + 0.5) / support|), normalised to sum 1.
 *   r = sum over rows (outer) and columns (inner) of (w_row w_col) v in fp32 on the byte values v in [0, 255], one fixed order (one
 *   thread per output pixel, no atomics: run-to-run identical);  video = r / 127.5f - 1.0f (an IEEE fp32 division, then a subtraction).
 * With (H0, W0) == (H, W) every output has the weights {1, 0} per axis and r == v exactly: the result is bitwise (float)v / 127.5f - 1.0f.
 * MG_ERR_SHAPE: a non-positive size, or Hs > 8 H0, Ws > 8 W0, H0 > 8 Hs or W0 > 8 Ws (more than 8x in either direction; 8x down is
 * 17 taps per axis), or H or T above 65535.  frames needs no alignment; video is written once, every element. */
int mg_video_from_u8(const uint8_t* frames, int T, int H0, int W0, int H, int W, float* video, void* stream);

/* Masked video-to-video (additions to ABI 9; not in the reference): WanT2V.inpaint keeps part of an existing clip and regenerates the rest.
 * Masks are hard: a byte is 0 (keep) or non-zero (regenerate).  The four functions use no device memory of their own and no atomics; every
 * output element is written by one thread: run-to-run identical.  A non-positive size is MG_ERR_SHAPE (checked before the pointers), a
 * null pointer MG_ERR_ARG.
 *
 * mg_mask_from_u8: the user's mask [Tm][H0][W0] (Tm == 1: one mask for every frame, else Tm >= T and the first T frames are read) -> the
 * pixel mask pm [T][H][W] through the geometry and the filter of mg_video_from_u8, so that mask and frames stay aligned:
 *   pm[t][y][x] = 0 for t < keep_frames, else (r >= 127.5f) ? 1 : 0, r = the fp32 sum mg_video_from_u8 forms for one channel of frame t
 *   (frame 0 when Tm == 1) holding the mask's bytes: the same taps in the same order, rows outer, columns inner.
 * With (H0, W0) == (H, W) r is the byte itself: pm = (mask >= 128) exactly.  MG_ERR_SHAPE as for mg_video_from_u8, and for Tm outside
 * {1} u [T, inf) or keep_frames outside [0, T].  Every byte of pm is written once. */
int mg_mask_from_u8(const uint8_t* mask, int Tm, int H0, int W0, int T, int H, int W, int keep_frames, uint8_t* pm, void* stream);

/* pm [T][H][W] -> the latent-grid mask lm [(T-1)/st + 1][H/sh][W/sw] of a causal VAE with strides (st, sh, sw): lm[j][y][x] = 1 when any
 * byte of pm is non-zero over rows sh y .. sh y + sh - 1, columns sw x .. sw x + sw - 1 and frames {0} for j = 0, st (j-1) + 1 .. st j for
 * j >= 1, else 0: a latent cell is kept only if every pixel under it is kept.  MG_ERR_SHAPE unless (T-1) % st == 0, H % sh == 0, W % sw == 0. */
int mg_mask_to_latent_u8(const uint8_t* pm, int T, int H, int W, int st, int sh, int sw, uint8_t* lm, void* stream);

/* latent [C][thw] fp32, IN PLACE, lm [thw] shared by the C channels; z0 and noise like latent:
 *   lm == 0: latent = c0 z0 + c1 noise, the bits mg_lincomb4_f32 writes for the two terms (z0, c0), (noise, c1) (fma(c1, noise, c0 z0));
 *   lm != 0: the element keeps its bits.
 * A select: a non-finite value of the side not chosen does not reach the result.  16-byte accesses when latent, z0 and noise are 16-byte
 * aligned, element by element otherwise; any thw. */
int mg_masked_renoise_f32(float* latent, const float* z0, const float* noise, const uint8_t* lm, float c0, float c1, int C, int64_t thw,
                          void* stream);

/* video [3][T][hw] fp32, IN PLACE, src of the same shape, pm [T][hw]: video = src where pm == 0, untouched elsewhere (a select, as above).
 * 16-byte accesses when video and src are 16-byte aligned; any hw. */
int mg_mask_composite_f32(float* video, const float* src, const uint8_t* pm, int T, int64_t hw, void* stream);

/* Context windows (additions to ABI 9; not in the reference): WanT2V.generate(windows=) denoises a latent longer than one DiT
 * pass as a whole and shows it to the DiT through overlapping windows of Fw latent frames.  The two functions move between the whole clip
 * [C][F][hw] and one window [C][Fw][hw] at frames [f0, f0 + Fw); all fp32, dense.  They use no device memory of their own and no atomics;
 * every output element is written by one thread: run-to-run identical, capturable.  A non-positive C, F, hw or Fw, f0 < 0 or
 * f0 + Fw > F is MG_ERR_SHAPE (checked before the pointers), a null pointer MG_ERR_ARG.  All index arithmetic is 64-bit.  A row of hw
 * elements goes as 16-byte accesses when both of its addresses are 16-byte aligned — the row (c, f0 + j) of the whole clip starts
 * (c F + f0 + j) hw elements behind the base, so that depends on F, f0 and hw as well as on the pointers — and element by element
 * otherwise; any hw, no pointer needs more than its type's alignment.
 *
 * mg_window_gather_f32: out[c][j][p] = x[c][f0 + j][p], a copy (the bits are unchanged).  x is only read, out is written once, every element.
 *
 * mg_window_blend_f32: with w[Fw] and first[Fw] in DEVICE memory, for every c, j, p, a = acc[c][f0 + j][p] and v = pred[c][j][p]:
 *   first[j] != 0: acc = w[j] v.  A select: the old content of acc is not read, so it needs no initial value and a NaN in it does not
 *                  reach the result;
 *   first[j] == 0: acc = fma(w[j], v, a).
 * One rounding per element and call; w[j] == 1.0f with first[j] != 0 leaves the bits of v.  Frames of acc outside [f0, f0 + Fw) are not
 * touched.  pred, w and first are only read; acc and pred must not overlap. */
int mg_window_gather_f32(const float* x, int C, int64_t F, int64_t hw, int64_t f0, int Fw, float* out, void* stream);
int mg_window_blend_f32(float* acc, const float* pred, int C, int64_t F, int64_t hw, int64_t f0, int Fw, const float* w, const uint8_t* first,
                        void* stream);

/* time_conv channel halves -> interleaved frames (vae.py:133-137):
 * x [T][H][W][2C] -> out [2T][H][W][C], frame 2t from channels [0,C), 2t+1 from [C,2C). */
int mg_vae_time_interleave_f32(const float* x, int T, int64_t HW, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * WanVAE encode (Encoder3d, WanVAE_.encode): the same fp32 kernels plus the pieces the decoder has no counterpart of.
 * Pure additions to ABI 9.
 * ---------------------------------------------------------------------------------------- */

/* Convolution with a stride and one-sided padding on the same exact-f32 implicit-GEMM tile — the encoder's down-samplers
 * (Resample downsample2d / downsample3d).  x [T][H][W][Cin], w [Cout][kt][kh][kw][Cin], out [To][Ho][Wo][Cout] with
 * n_out = (n + pad0 + pad1 - k) / stride + 1 per axis; output (t, y, x) reads input coordinate stride * out + tap - pad0.
 *   space: ph0 / pw0 zero rows / columns before, ph1 / pw1 behind (downsample: kh = kw = 3, stride 2, pads (0, 1));
 *   time:  the pt0 frames before the chunk come from `cache` ([tc][H][W][Cin], its LAST frames; zeros where it has none) and
 *          nothing is padded behind the chunk (time_conv of downsample3d: kt = 3, st = 2, pt0 = 1, tc = 1: output j reads
 *          frames 2j-1, 2j, 2j+1 of the chunk, frame -1 being the cached one).
 * k <= 3, strides in {1, 2}, pads < k per axis, Cin % 4 == 0; mode must be MG_VAE_EXACT (MG_ERR_ARG otherwise). */
int mg_vae_conv_strided_f32(const float* x, const float* cache, int tc, int T, int H, int W, int Cin, const float* w, const float* bias,
                            int Cout, int kt, int kh, int kw, int st, int sh, int sw, int pt0, int ph0, int ph1, int pw0, int pw1,
                            float* out, int mode, void* stream);

/* The encoder's input convolution, CausalConv3d(3, Cout, 3, padding = 1), on the STAGED video of mg_vae_video_in_f32:
 * xs [T][H][W + 2][4] (channel 3 and the columns 0 and W + 1 are zero), cache [tc <= 2][H][W + 2][4] = the last staged frames of
 * the previous chunk (may be NULL: zeros), w [Cout][3][3][3][4] (channel 3 zero), out [T][H][W][Cout].  The three kw taps of a
 * voxel are one contiguous run of 12 floats, so the contraction is 9 runs = 108 k in 4 chunks of 32 instead of 27 taps of one
 * chunk each; the padding only adds exact zeros.  mode must be MG_VAE_EXACT. */
int mg_vae_conv_in3_f32(const float* xs, const float* cache, int tc, int T, int H, int W, const float* w, const float* bias, int Cout,
                        float* out, int mode, void* stream);

/* video [3][T][H][W] (reference layout), frames [t0, t0 + n) -> the staged layout above, out [n][H][W + 2][4] (16-byte aligned);
 * and x [T][H][W][ldx] channels-last (the encoder's top-level conv1 output, mu | log_var) -> out [C][T][H][W] =
 * (x[..][c] - mean[c]) * inv_std[c] for the first C <= ldx channels (WanVAE.encode's normalised mu). */
int mg_vae_video_in_f32(const float* video, int T, int H, int W, int t0, int n, float* out, void* stream);
int mg_vae_latent_out_f32(const float* x, int ldx, const float* mean, const float* inv_std, int C, int T, int H, int W, float* out,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters (WanModel.load_lora).  A pure addition to ABI 9.
 * ---------------------------------------------------------------------------------------- */

/* Low-rank update of a weight matrix, in place (no reference counterpart):
 *   w[n][k] <- round_w( w[n][k] + sum_{j<R} up[n][j] * down[j][k] )
 * w [N][K] bf16 (w_f32 = 0) or fp32 (w_f32 = 1), row stride ldw elements;
 * up [N][R] fp32 (row stride ldu), down [R][K] fp32 (row stride ldd).
 * The old weight is widened to fp32 and the R products are added to it one after the other, in order of j, each by one fp32 fma (the
 * exact-f32 MFMA); bf16 storage then takes ONE round-to-nearest-even, fp32 storage the sum as it is.  (IEEE addition: a weight of -0
 * whose update is 0 is stored as +0.)  The caller folds an adapter's scale into `up` and passes several adapters as one pair of
 * factors concatenated along R; any R >= 1 is taken, in chunks, with no padding asked of the caller.
 * N >= 1, K >= 8 and K % 8 == 0, ldw >= K.  Elements of a row past K and rows outside [0, N) of a taller buffer are never written: a
 * row slice or a column view of a larger matrix is merged through its own pointer.  Every element of w is read and written by one
 * lane, as part of a 16-byte vector; no atomics.
 * MG_ERR_ARG: a null pointer, w not 16-byte aligned, K % 8 != 0, R, N or K < 1, w_f32 not 0 / 1.
 * MG_ERR_SHAPE: ldw < K or ldw not a multiple of 16 bytes, ldu < R, ldd < K, a factor not 4-byte aligned. */
int mg_lora_merge(void* w, int w_f32, int64_t ldw, int N, int K, const float* up, int64_t ldu, const float* down, int64_t ldd, int R,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Normalized attention guidance (WanModel.forward(nag=); not the reference's arithmetic, opt-in).
 * A pure addition to ABI 9.
 * ---------------------------------------------------------------------------------------- */

/* The row-wise mix of two cross-attention outputs (Chen et al. 2025, NAG): zp [rows][dim] is the output for the positive prompt, zn for
 * the negative one, both bf16 with all heads of a token in one row (row strides ldp / ldn elements).  Per row, every operation in fp32:
 *   g_j  = fma(scale, p_j, -((scale - 1) n_j))
 *   Np   = sum_j |p_j|,  Ng = sum_j |g_j|        (the norm is over the whole row, not per head)
 *   c    = tau Np / (Ng + 1e-7)  if Ng > tau Np,  else 1
 *   out_j = bf16( fma(alpha c, g_j, (1 - alpha) p_j) )                      ONE rounding to bf16
 * The comparison form divides by nothing that can be 0: Np = 0 < Ng gives c = 0, both sums 0 give out = 0.
 * One wave owns a row: a lane adds its elements in index order (chunk lane + 64 i, i ascending, 8 elements each), the 64 partial sums
 * meet in a fixed xor butterfly — the bits of a row depend on the row and the three parameters alone, not on rows, the grid or the
 * rows that share the launch.  No atomics, no device memory besides the operands.
 * scale = 1 gives out == zp bit for bit, and so does zn == zp (finite inputs): the fp32 value lies within ~2 scale 2^-24 relative of
 * the bf16 number p_j, far inside bf16's half ulp for every scale <= 64.
 * out may be zp itself (same pointer, ldo == ldp: a wave reads its whole row before it stores); it may not overlap zn, or zp otherwise.
 * MG_ERR_ARG: a null pointer; scale < 1 or > 64, tau < 1, alpha outside [0, 1], any of them not finite; out overlapping an input other
 *   than as above (the address ranges [ptr, ptr + (rows - 1) ld + dim) are compared).
 * MG_ERR_SHAPE: dim <= 0, dim % 8, dim > 8192, an ld % 8 or < dim, rows < 0, a pointer not 16-byte aligned.
 * rows == 0 with valid arguments: MG_OK, nothing is launched. */
int mg_nag_combine_bf16(const uint16_t* zp, int64_t ldp, const uint16_t* zn, int64_t ldn, uint16_t* out, int64_t ldo, int64_t rows, int dim,
                        float scale, float tau, float alpha, void* stream);

#ifdef MG_AB_BUILD
/* ------------------------------------------------------------------------------------------
 * A/B LIBRARY ONLY (libmoviigen_hip_ab.so, built from the same sources with -DMG_AB_BUILD; the product library
 * libmoviigen_hip.so exports NOTHING of this section).  Measurement partners and s_memtime hooks: used by
 * csrc/tools/selftest.cpp, tools/ and the variant-agreement tests to force a kernel schedule and to take cycle breakdowns
 * of the hot loops.  All are process-global switches, not thread-safe, not part of the drop-in contract; passing 0 / NULL
 * restores the default.  The product path never loads this library (wan/backend/lib.py: load vs load_ab).
 * ---------------------------------------------------------------------------------------- */
/* Tile schedule of mg_gemm_bf16 for M > 256 and N > 128 (same results bit for bit); 0 = the product's rule (12, else 2 / 1).
 * Returns MG_ERR_ARG for a number that names no variant (no silent aliases).
 * 12 = (product) 256x256x64 tile, v_mfma_f32_16x16x32_bf16, persistent, 4 waves = ONE per SIMD; a stage is refilled WHILE it is
 *     consumed — loads two k-tiles ahead, three barriers per k-tile, none behind a drained memory pipe; the k-tile body is a GENERATED
 *     schedule (tools/gen_gemm_v12_schedule.py) in a single self-looping block (200 + flags: 2 raster 0, 4 no stores, 16 direct fp32
 *     epilogue, 32 * (1 + s) generated body s);
 * 11 = the round-4 default: the same tile and epilogues, ONE barrier per k-tile behind vmcnt(0), the last 32 MFMAs of a k-tile behind
 *     the next barrier (tools/gen_gemm_v11_schedule.py; 110 + flags: 1 de-phased waves, 2 raster 0, 4 no stores, 8 skewed start,
 *     16 direct fp32 epilogue, 32 the every-4th-gap schedule);
 * 8 = the round-3 default: EIGHT waves in two ping-pong groups, direct epilogues (the reference the epilogue tests compare with);
 * 7 = one wave per SIMD, compiler-scheduled;   2 = 256x128x64, 8 waves, 3 stages;   1 = 128x128x64, 4 waves, 2 stages. */
int mg_gemm_set_variant(int variant);

/* Kernel behind mg_attn_fwd_bf16_hd128* and the matching K row order of mg_pack_kv_bf16 (pack and attend under the same setting):
 * 0 = "m16" (the product's kernel); 3 = "w64", the round-2 kernel (32x32x16 MFMA, per-row softmax reference; NOT the same bits).
 * Returns MG_ERR_ARG for anything else. */
int mg_attn_set_variant(int variant);

void mg_attn_w64_profile(unsigned long long* dev_buf);     /* both attention kernels: 4 waves x {fence, step A, step B, iterations} at [0, 16); the m16 kernel also stores every workgroup's {start, end} (s_memrealtime) of the last launch at [16 + 2 b]: dev_buf holds 16 + 2 x 512 + 8 entries; m16 also adds wave 0's per-item phases {first loads landed, first tile, refill wait, steady loop, drain, epilogue, items, epilogue up to its last store's issue} at [1040, 1048) */
void mg_attn_w64_debug(int flags);                         /* bit 0: keep the pipelined result of flagged blocks (no exact pass); bits 1-3: filler placement, bit 4: static partition, bits 5-6: MFMA order; bit 7: the pre-scaled entry runs FIVE query blocks per wave (320-query items) at any shape, bit 8: four at any shape */
void mg_attn_w64_flag_counter(unsigned* dev_counter);      /* dev_counter[2]: [0] += query blocks whose pipelined pass flagged (m16: repeated with swept row maxima; w64: redone by the exact loop), [1] += m16 blocks that went on to the exact loop */
void mg_gemm_debug_profile(unsigned long long* dev_buf);   /* GEMM variants 1/2: 8 waves x {wait+barrier, stage issue, MFMA, k-tiles} */
void mg_gemm5_debug_profile(unsigned long long* dev_buf);  /* GEMM variants 7 / 8 / 11 / 12: per-wave s_memtime sums at [0, 64) (csrc/tools/selftest.cpp gemmprof prints each layout); variant 12 also stores every workgroup's {start, end} (s_memrealtime) at [64 + 2 b]: dev_buf holds 64 + 2 x 512 entries */
#endif /* MG_AB_BUILD */

#ifdef __cplusplus
}
#endif
#endif /* MOVIIGEN_HIP_H */
