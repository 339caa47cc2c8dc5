// Low-rank update of a weight matrix in place (mg_lora_merge; WanModel.load_lora):
//     w[n][k] <- round_w( w[n][k] + sum_{j<R} up[n][j] * down[j][k] )
// on the exact-f32 MFMA v_mfma_f32_32x32x2_f32, whose result is bit for bit a j-ordered fmaf chain: the accumulator is
// INITIALISED with the old weight widened to fp32, so a stored element is fma(u_{R-1}, d_{R-1}, ... fma(u_0, d_0, w)) — an fp32 sum of
// R + 1 terms — and, for bf16 storage, ONE round-to-nearest-even behind it (v_cvt_pk_bf16_f32).
//
// A workgroup of 4 waves owns a 64 (n) x 256 (k) tile of w, a wave 32 x 128 of it in four 32 x 32 accumulators.  The MFMA's A operand
// is `down` (MFMA row i = a column k of w), its B operand `up` (MFMA column = a row n of w): a lane then holds ONE row n = lane & 31 and
// 16 MFMA rows, i = (r & 3) + 8 (r >> 2) + 4 h for register r and lane half h = lane >> 5.  MFMA row i is fed column
// kmap(i) = 16 ((i >> 2) & 1) + 4 (i >> 3) + (i & 3) of the 32-column tile — a permutation applied in the LDS read address, nothing
// else — which makes register r of lane half h column 16 h + r: a lane owns 16 CONSECUTIVE k of its row and reads and writes them as
// 16-byte vectors (two per accumulator for bf16 storage, four for fp32).  Every element of w is loaded once and stored once, by the same
// lane; no atomics.
//
// `up` rows and `down` columns of the tile go through LDS in chunks of 32 ranks, zero-filled past R, N and K (an added +0 product changes
// nothing); they are read from global memory element by element, so no alignment or padding is asked of the factors.  The last chunk
// runs only the MFMAs its ranks need.  LDS images: up [64][33] (row stride 33: the 32 rows a wave reads per operand fall into different
// banks), down [32][288] (the two lane halves read neighbouring ranks: 288 = 32 mod 64 keeps them in different banks).
#include "common.h"
#include "../../include/moviigen_hip.h"

#define LM_TN 64        // rows of w per workgroup
#define LM_TK 256       // columns of w per workgroup
#define LM_RC 32        // ranks per LDS chunk
#define LM_UP_LD (LM_RC + 1)
#define LM_DN_LD (LM_TK + 32)

template <bool F32>
__global__ __launch_bounds__(256) void lora_merge_kernel(void* __restrict__ w, int64_t ldw, int N, int K, const float* __restrict__ up,
                                                         int64_t ldu, const float* __restrict__ down, int64_t ldd, int R) {
    __shared__ float up_s[LM_TN * LM_UP_LD];
    __shared__ float dn_s[LM_RC * LM_DN_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * LM_TN, k0 = blockIdx.y * LM_TK;
    const int wn = (wave >> 1) * 32, wk = (wave & 1) * 128;
    const int n = n0 + wn + l31;                        // the row of w this lane owns
    const int kl = k0 + wk + 16 * h;                    // its columns: kl + 32 t + [0, 16), t = 0..3
    char* const wrow = (char*)w + (int64_t)n * ldw * (F32 ? 4 : 2);

    // accumulators = the old weights, widened.  K % 8 == 0: a run of 8 columns is wholly inside the matrix or wholly outside
    f32x16_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = kl + 32 * t + 8 * q;
            if (n < N && k < K) {
                if (F32) {
                    const f32x4_t a = *(const f32x4_t*)(wrow + (int64_t)k * 4), b = *(const f32x4_t*)(wrow + (int64_t)k * 4 + 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { acc[t][8 * q + e] = a[e]; acc[t][8 * q + 4 + e] = b[e]; }
                } else {
                    const u16x8_t v = *(const u16x8_t*)(wrow + (int64_t)k * 2);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[t][8 * q + e] = bf2f(v[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[t][8 * q + e] = 0.f;
            }
        }
    }

    const int kmap = 16 * ((l31 >> 2) & 1) + 4 * (l31 >> 3) + (l31 & 3);
    const float* const up_l = up_s + (wn + l31) * LM_UP_LD + h;
    const float* const dn_l = dn_s + h * LM_DN_LD + wk + kmap;

    for (int j0 = 0; j0 < R; j0 += LM_RC) {
        if (j0) __syncthreads();                        // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < LM_TN * LM_RC / 256; ++i) {
            const int idx = tid + 256 * i, r = idx >> 5, j = idx & 31;
            up_s[r * LM_UP_LD + j] = (n0 + r < N && j0 + j < R) ? up[(int64_t)(n0 + r) * ldu + j0 + j] : 0.f;
        }
#pragma unroll 8
        for (int j = 0; j < LM_RC; ++j)
            dn_s[j * LM_DN_LD + tid] = (j0 + j < R && k0 + tid < K) ? down[(int64_t)(j0 + j) * ldd + k0 + tid] : 0.f;
        __syncthreads();
        const int steps = R - j0 >= LM_RC ? LM_RC / 2 : (R - j0 + 1) >> 1;       // rank pairs of this chunk (uniform)
        for (int s = 0; s < steps; ++s) {
            const float b = up_l[2 * s];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(dn_l[2 * s * LM_DN_LD + 32 * t], b, acc[t], 0, 0, 0);
        }
    }

#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = kl + 32 * t + 8 * q;
            if (n < N && k < K) {
                if (F32) {
                    f32x4_t a, b;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = acc[t][8 * q + e]; b[e] = acc[t][8 * q + 4 + e]; }
                    *(f32x4_t*)(wrow + (int64_t)k * 4) = a;
                    *(f32x4_t*)(wrow + (int64_t)k * 4 + 16) = b;
                } else {
                    u32x4_t v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = pack_bf2(acc[t][8 * q + 2 * e], acc[t][8 * q + 2 * e + 1]);
                    *(u32x4_t*)(wrow + (int64_t)k * 2) = v;
                }
            }
        }
    }
}

extern "C" int mg_lora_merge(void* w, int w_f32, int64_t ldw, int N, int K, const float* up, int64_t ldu, const float* down,
                             int64_t ldd, int R, void* stream) {
    if (!w || !up || !down || ((uintptr_t)w & 15)) return MG_ERR_ARG;
    if (N < 1 || K < 1 || R < 1 || (K & 7) || (w_f32 != 0 && w_f32 != 1)) return MG_ERR_ARG;
    // every row of w starts on a 16-byte boundary; the factors are read as single floats
    if (ldw < K || (ldw & (w_f32 ? 3 : 7)) || ldu < R || ldd < K || (((uintptr_t)up | (uintptr_t)down) & 3)) return MG_ERR_SHAPE;
    const dim3 grid((N + LM_TN - 1) / LM_TN, (K + LM_TK - 1) / LM_TK);
    if (grid.y > 65535) return MG_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (w_f32)
        hipLaunchKernelGGL(lora_merge_kernel<true>, grid, dim3(256), 0, st, w, ldw, N, K, up, ldu, down, ldd, R);
    else
        hipLaunchKernelGGL(lora_merge_kernel<false>, grid, dim3(256), 0, st, w, ldw, N, K, up, ldu, down, ldd, R);
    return mg_check_launch();
}
