// Shared device helpers for the MoviiGen1.1 MI355X (gfx950 / CDNA4) kernels.
// wave = 64 lanes; bf16 travels as uint16_t; all math in fp32 unless stated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MG_OK 0
#define MG_ERR_ARG (-1)
#define MG_ERR_SHAPE (-2)
#define MG_ERR_LAUNCH (-3)
#define MG_ERR_UNAVAILABLE (-4)   // librccl could not be bound at run time
#define MG_ERR_COMM (-5)          // an RCCL call failed

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

#define MG_DEV static __device__ __forceinline__

// fp32 -> bf16 round-to-nearest-even (matches torch .to(bfloat16)); one v_cvt_pk_bf16_f32 per pair
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
MG_DEV unsigned int pack_bf2(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2_t));
}
MG_DEV unsigned short f2bf(float f) { return (unsigned short)(pack_bf2(f, 0.f) & 0xffffu); }
MG_DEV float bf2f(unsigned short h) { return __uint_as_float(((unsigned int)h) << 16); }
MG_DEV float round_bf(float f) { return __uint_as_float(pack_bf2(f, 0.f) << 16); }

MG_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
MG_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide sum for blockDim.x == NT (multiple of 64); `red` is NT/64 floats of LDS.
template <int NT>
MG_DEV float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

// torch.nn.functional.gelu(x, approximate='tanh') = 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3).
// With tanh(u) = 1 - 2 / (e^{2u} + 1):  0.5 x (1 + tanh(u)) = x / (1 + e^{-2u}) — ONE v_exp_f32 and ONE v_rcp_f32 per value (7 VALU instructions; the
// round-1 form went through an IEEE division: ~22, and the GELU epilogue of ffn.0 is VALU-bound behind the tile's last MFMA: 0.72 VALU instructions per
// MFMA over the launch, profiles/r06_pmc_gemm_v12.txt).  -2 log2(e) is folded into the polynomial's constants; x -> +inf: e -> 0, x; x -> -inf: e -> inf, -0.
MG_DEV float gelu_tanh(float x) {
    const float a0 = -2.f * 1.4426950408889634f * 0.7978845608028654f, a1 = a0 * 0.044715f;
    const float e = __builtin_amdgcn_exp2f(x * (a0 + a1 * (x * x)));      // e^{-2u}
    return x * __builtin_amdgcn_rcpf(1.f + e);
}
MG_DEV float silu(float x) { return x / (1.f + __expf(-x)); }

// LDS-DMA (global_load_lds_dwordx4 / _dword): 16 or 4 bytes per lane from g straight to LDS at l + size * lane, no VGPR round trip.
// (mg_lptr_t)p is also how a kernel gets the 32-bit LDS address of p for its inline-assembly ds_read.
typedef const __attribute__((address_space(1))) void* mg_gptr_t;
typedef __attribute__((address_space(3))) void* mg_lptr_t;
MG_DEV void mg_glds16(const void* g, void* l) { __builtin_amdgcn_global_load_lds((mg_gptr_t)g, (mg_lptr_t)l, 16, 0, 0); }
MG_DEV void mg_glds4(const void* g, void* l) { __builtin_amdgcn_global_load_lds((mg_gptr_t)g, (mg_lptr_t)l, 4, 0, 0); }

// CUs of the CURRENT device, asked per call (an attribute lookup; a function-static cache would be wrong in a process
// that drives devices of different sizes and racy on first use from two threads); -1 on error
static inline int mg_cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return -1;
    return n;
}
// CUs a persistent launch may occupy — one workgroup per CU, dealt round-robin over the 8 XCDs: the device's count rounded down to a
// multiple of 8, less `reserve_cus` (rounded up to one: CUs left free for a kernel on another stream), at least 8; -1 on error
static inline int mg_persistent_cus(int reserve_cus = 0) {
    int n_cu = mg_cu_count();
    if (n_cu < 0) return -1;
    n_cu = (n_cu & ~7) - ((reserve_cus + 7) & ~7);
    return n_cu < 8 ? 8 : n_cu;
}

static inline int mg_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MG_OK : MG_ERR_LAUNCH;
}

// In-place masked overwrite of x [C][n] fp32 (total = C n) under a byte mask [n] shared by the C planes: x[i] = f(i) where mask[i % n] == 0,
// the element keeps its bits elsewhere.  A select, not a blend: the side not chosen never enters the arithmetic of the result.
// F has one(i) -> float and vec(i) -> f32x4_t (i % 4 == 0, its sources 16-byte aligned) for the new value of flat element i.
// nvec groups of four elements go as 16-byte accesses (the launcher passes 0 when a pointer is not 16-byte aligned), the elements from
// 4 nvec on one by one.  A group may straddle a plane boundary when n % 4 != 0: its mask bytes are then read one by one with the wrap;
// mask_dword = (n % 4 == 0 and mask 4-byte aligned) reads them as one dword.  A group with nothing to overwrite is neither loaded nor
// stored, one with everything to overwrite does not load x.  (mg_masked_renoise_f32, mg_mask_composite_f32)
template <class F>
__global__ __launch_bounds__(256) void masked_overwrite_kernel(float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t n, int64_t total,
                                                               int64_t nvec, bool mask_dword, F f) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = tid; g < nvec; g += stride) {
        const int64_t i = 4 * g;
        int64_t p = i % n;
        bool keep[4];
        if (mask_dword) {
            const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) keep[e] = ((m >> (8 * e)) & 0xffu) != 0;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                keep[e] = mask[p] != 0;
                if (++p == n) p = 0;
            }
        }
        const bool any_keep = keep[0] | keep[1] | keep[2] | keep[3], all_keep = keep[0] & keep[1] & keep[2] & keep[3];
        if (all_keep) continue;
        f32x4_t v = f.vec(i);
        if (any_keep) {
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = keep[e] ? xv[e] : v[e];
        }
        *reinterpret_cast<f32x4_t*>(x + i) = v;
    }
    for (int64_t i = 4 * nvec + tid; i < total; i += stride)
        if (mask[i % n] == 0) x[i] = f.one(i);
}

// the launch of masked_overwrite_kernel: `aligned16` = x and every source of f are 16-byte aligned
template <class F>
static inline int mg_launch_masked_overwrite(float* x, const uint8_t* mask, int64_t n, int64_t total, bool aligned16, F f, void* stream) {
    const int64_t nvec = aligned16 ? total / 4 : 0, work = nvec + (total - 4 * nvec);
    int64_t grid = (work + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(masked_overwrite_kernel<F>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, mask, n, total, nvec,
                       (n & 3) == 0 && ((uintptr_t)mask & 3) == 0, f);
    return mg_check_launch();
}
