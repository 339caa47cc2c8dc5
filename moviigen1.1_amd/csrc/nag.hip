// Normalized attention guidance (WanModel.forward(nag=); definition in the header): mg_nag_combine_bf16 mixes the
// cross-attention output of the positive prompt with that of the negative one, per token row, in front of the `o` projection.
// HBM-bound: two reads and one write of [rows][dim] bf16.
#include <math.h>

#include "common.h"
#include "../../include/moviigen_hip.h"

#define NAG_NT 256
#define NAG_MAX_GRID 2048

// fma(scale, p, -((scale - 1) n)): two roundings, written out so that contraction cannot change them.  scale = 1: sm1 = 0 and g = p exactly.
MG_DEV float nag_g(float p, float n, float s, float sm1) { return fmaf(s, p, -(sm1 * n)); }

// ONE WAVE PER ROW, the shape of rmsnorm_rope_wave_kernel (dit_elementwise.hip): a lane holds chunks lane + 64 i of both rows as packed
// bf16 (2 x MAXN x 4 registers), the two L1 norms are wave reductions, g is formed twice (for its norm, then for the result: the same two
// operations, the same bits) and not kept.  No LDS, no barrier; the row is read whole before the first store, so out may be zp.
// zp and out carry no __restrict__: they may be the same rows.
template <int MAXN>
__global__ __launch_bounds__(NAG_NT) void nag_combine_wave_kernel(const uint16_t* zp, int64_t ldp, const uint16_t* __restrict__ zn, int64_t ldn,
                                                                 uint16_t* out, int64_t ldo, int64_t rows, int dim, float s, float sm1,
                                                                 float tau, float alpha, float oma) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nc = dim >> 3;
    const u16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t row = (int64_t)blockIdx.x * (NAG_NT / 64) + wave; row < rows; row += (int64_t)gridDim.x * (NAG_NT / 64)) {
        const u16x8_t* pr = (const u16x8_t*)(zp + row * ldp);
        const u16x8_t* nr = (const u16x8_t*)(zn + row * ldn);
        u16x8_t up[MAXN], un[MAXN];
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            const int ch = lane + 64 * i;
            up[i] = ch < nc ? pr[ch] : zero;
            un[i] = ch < nc ? nr[ch] : zero;
        }
        float np = 0.f, ng = 0.f;           // chunks past the row are zeros: they add nothing, exactly
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = bf2f(up[i][j]);
                np += fabsf(p);
                ng += fabsf(nag_g(p, bf2f(un[i][j]), s, sm1));
            }
        np = wave_sum(np);
        ng = wave_sum(ng);
        const float lim = tau * np;
        const float c = ng > lim ? lim / (ng + 1e-7f) : 1.f;
        const float w = alpha * c;
        // (both rows are in registers whole by now — the reductions needed every element — so storing chunk by chunk is safe in place)
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = bf2f(up[i][j]);
                y[j] = fmaf(w, nag_g(p, bf2f(un[i][j]), s, sm1), oma * p);
            }
            u32x4_t o;
            o[0] = pack_bf2(y[0], y[1]);
            o[1] = pack_bf2(y[2], y[3]);
            o[2] = pack_bf2(y[4], y[5]);
            o[3] = pack_bf2(y[6], y[7]);
            const int ch = lane + 64 * i;
            if (ch < nc) ((u32x4_t*)(out + row * ldo))[ch] = o;
        }
    }
}

// do the element ranges [a, a + na) and [b, b + nb) of two bf16 buffers meet?
static bool nag_ranges_meet(const uint16_t* a, int64_t na, const uint16_t* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 2 && b0 < a0 + (uintptr_t)na * 2;
}

extern "C" int mg_nag_combine_bf16(const uint16_t* zp, int64_t ldp, const uint16_t* zn, int64_t ldn, uint16_t* out, int64_t ldo, int64_t rows,
                                   int dim, float scale, float tau, float alpha, void* stream) {
    if (!zp || !zn || !out) return MG_ERR_ARG;
    if (dim <= 0 || (dim & 7) || dim > 8192 || (ldp & 7) || (ldn & 7) || (ldo & 7) || ldp < dim || ldn < dim || ldo < dim || rows < 0 ||
        (((uintptr_t)zp | (uintptr_t)zn | (uintptr_t)out) & 15))
        return MG_ERR_SHAPE;
    // (a NaN fails every comparison below: the conditions are written as what must hold)
    if (!(scale >= 1.f && scale <= 64.f) || !(tau >= 1.f) || !isfinite(tau) || !(alpha >= 0.f && alpha <= 1.f)) return MG_ERR_ARG;
    if (rows == 0) return MG_OK;
    const int64_t span_p = (rows - 1) * ldp + dim, span_n = (rows - 1) * ldn + dim, span_o = (rows - 1) * ldo + dim;
    if (nag_ranges_meet(out, span_o, zn, span_n)) return MG_ERR_ARG;
    if (!(out == zp && ldo == ldp) && nag_ranges_meet(out, span_o, zp, span_p)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nc = dim >> 3;
    int64_t grid = (rows + 3) / 4;
    if (grid > NAG_MAX_GRID) grid = NAG_MAX_GRID;      // 8 workgroups per CU, as mg_rmsnorm_rope_bf16's wave kernel; further rows by the row stride
    const float sm1 = scale - 1.f, oma = 1.f - alpha;   // scale - 1 is exact in fp32 for every scale >= 1
#define NAGW(N) hipLaunchKernelGGL((nag_combine_wave_kernel<N>), dim3((unsigned)grid), dim3(NAG_NT), 0, st, zp, ldp, zn, ldn, out, ldo, rows, dim, \
                                   scale, sm1, tau, alpha, oma)
    if (nc <= 64) NAGW(1);
    else if (nc <= 256) NAGW(4);
    else if (nc <= 640) NAGW(10);
    else NAGW(16);
#undef NAGW
    return mg_check_launch();
}
