// Context windows (WanT2V.generate(windows=); definitions in the header): the two passes between the whole-clip latent
// [C][F][hw] and one window [C][Fw][hw] of it — mg_window_gather_f32 cuts the window out, mg_window_blend_f32 adds the window's
// prediction, weighted per frame, into the whole-clip prediction.  Memory-bound, one access per element and operand.
#include "common.h"
#include "../../include/moviigen_hip.h"

#define CW_NT 256
#define CW_MAX_BLOCKS 8192

// row (c, j) of a gather: hw elements of x at frame f0 + j -> hw elements of the dense window
struct GatherRow {
    const float* src;
    float* dst;
    __device__ void put4(int64_t i) const { *reinterpret_cast<f32x4_t*>(dst + i) = *reinterpret_cast<const f32x4_t*>(src + i); }
    __device__ void put1(int64_t i) const { dst[i] = src[i]; }
};
struct GatherOp {
    typedef GatherRow Row;
    const float* x;
    float* out;
    int64_t F, f0;
    int Fw;
    __device__ Row row(int c, int j, int64_t hw) const {
        return Row{x + ((int64_t)c * F + f0 + j) * hw, out + ((int64_t)c * Fw + j) * hw};
    }
};

// row (c, j) of a blend: acc at frame f0 + j <- w[j] pred (first[j] != 0: a select, acc is not loaded) or fma(w[j], pred, acc)
struct BlendRow {
    const float* src;
    float* dst;
    float w;
    bool first;
    __device__ void put4(int64_t i) const {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(src + i);
        f32x4_t r;
        if (first) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = w * v[e];
        } else {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(dst + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(w, v[e], a[e]);
        }
        *reinterpret_cast<f32x4_t*>(dst + i) = r;
    }
    __device__ void put1(int64_t i) const { dst[i] = first ? w * src[i] : __builtin_fmaf(w, src[i], dst[i]); }
};
struct BlendOp {
    typedef BlendRow Row;
    float* acc;
    const float* pred;
    int64_t F, f0;
    int Fw;
    const float* w;
    const uint8_t* first;
    __device__ Row row(int c, int j, int64_t hw) const {
        return Row{pred + ((int64_t)c * Fw + j) * hw, acc + ((int64_t)c * F + f0 + j) * hw, w[j], first[j] != 0};
    }
};

// One workgroup per (channel c, window frame j, run of CW_NT groups of four elements); grid (x = run, y = j, z = c), every axis looped,
// so a row's two pointers, its weight and its alignment are the same in every lane and no index is divided.  A row goes as 16-byte
// accesses when both of its ends of the copy are 16-byte aligned — which depends on the base pointers, F, f0 and hw together — with
// the hw % 4 elements behind the last whole group one by one; a row that is not goes element by element, neighbouring lanes on
// neighbouring elements.  Every element of the window's frames is written by one lane, nothing outside them is touched.
template <class Op>
__global__ __launch_bounds__(CW_NT) void window_rows_kernel(Op op, int C, int Fw, int64_t hw) {
    const int64_t ngrp = (hw + 3) >> 2;
    for (int c = blockIdx.z; c < C; c += gridDim.z)
        for (int j = blockIdx.y; j < Fw; j += gridDim.y) {
            const typename Op::Row r = op.row(c, j, hw);
            const bool vec = ((reinterpret_cast<uintptr_t>(r.src) | reinterpret_cast<uintptr_t>(r.dst)) & 15) == 0;
            for (int64_t g0 = (int64_t)blockIdx.x * CW_NT; g0 < ngrp; g0 += (int64_t)gridDim.x * CW_NT) {
                if (vec) {
                    const int64_t i = 4 * (g0 + threadIdx.x);
                    if (i + 4 <= hw) r.put4(i);
                    else
                        for (int64_t e = i; e < hw; ++e) r.put1(e);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int64_t e = 4 * g0 + k * CW_NT + threadIdx.x;
                        if (e < hw) r.put1(e);
                    }
                }
            }
        }
}

template <class Op>
static int launch_window_rows(const Op& op, int C, int Fw, int64_t hw, void* stream) {
    const int64_t nrun = ((hw + 3) / 4 + CW_NT - 1) / CW_NT;
    const int64_t gx = nrun < CW_MAX_BLOCKS ? nrun : CW_MAX_BLOCKS;
    int64_t gy = CW_MAX_BLOCKS / gx, gz = 1;
    if (gy > Fw) gy = Fw;
    gz = CW_MAX_BLOCKS / (gx * gy);
    if (gz > C) gz = C;
    hipLaunchKernelGGL(window_rows_kernel<Op>, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(CW_NT), 0, (hipStream_t)stream, op, C, Fw, hw);
    return mg_check_launch();
}

// (the last two terms: the byte size of the whole clip fits the 64-bit index arithmetic)
static bool window_shape_ok(int C, int64_t F, int64_t hw, int64_t f0, int Fw) {
    int64_t n;
    return C > 0 && F > 0 && hw > 0 && Fw > 0 && f0 >= 0 && f0 <= F - Fw && !__builtin_mul_overflow(F, hw, &n) &&
           !__builtin_mul_overflow(n, (int64_t)C * 4, &n);
}

extern "C" int mg_window_gather_f32(const float* x, int C, int64_t F, int64_t hw, int64_t f0, int Fw, float* out, void* stream) {
    if (!window_shape_ok(C, F, hw, f0, Fw)) return MG_ERR_SHAPE;
    if (!x || !out) return MG_ERR_ARG;
    return launch_window_rows(GatherOp{x, out, F, f0, Fw}, C, Fw, hw, stream);
}

extern "C" int mg_window_blend_f32(float* acc, const float* pred, int C, int64_t F, int64_t hw, int64_t f0, int Fw, const float* w,
                                   const uint8_t* first, void* stream) {
    if (!window_shape_ok(C, F, hw, f0, Fw)) return MG_ERR_SHAPE;
    if (!acc || !pred || !w || !first) return MG_ERR_ARG;
    return launch_window_rows(BlendOp{acc, pred, F, f0, Fw, w, first}, C, Fw, hw, stream);
}
