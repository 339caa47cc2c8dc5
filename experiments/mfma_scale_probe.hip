// Probe: operand, scale and result lane maps of the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4 and
// _32x32x64_, e4m3 operands) on gfx950, with EXACT integer data and ASYMMETRIC operands: elements are integers in
// [-8, 8], scale bytes 125..129 differ per row and per 32-block on both sides, so every product and every sum is exact
// in fp32 and a swapped row/column, a permuted k or a misplaced scale changes the result.  For each hypothesis the host
// lays the operands out in registers accordingly, the kernel issues ONE instruction, and the result is compared bit for
// bit with the fp64 sum.
// R = rows of the shape (16 / 32), KK = 2048 / R its depth, lane l = (row l % R, group g = l / R), byte j = 0..31 of its 8 registers.
//   H0: k = 32 g + j; the lane's scale byte (byte `opsel` of its scale register) scales the 32 elements the lane carries
//   H1: k = 16 g + j for j < 16, KK/2 + 16 g + (j - 16) for j >= 16 (registers 0-3 and 4-7 are half the depth apart); scale as H0
//   H2: the k map of H1, but lane (row, g) supplies the scale of the row's k-block g = k in [32 g, 32 g + 32) — elements that
//       OTHER lanes of the row carry
//   result         16x16: lane l, register r = D[4 (l / 16) + r][l % 16];  32x32: D[8 (r / 4) + 4 (l / 32) + r % 4][l % 32]
//                  (D[i][j] = sum_k A[i][k] B[j][k]: A's row index is the result's ROW)
// Then a discovery launch that assumes no map, on row 0 / column 0: a one-hot element against an all-ones operand doubles
// exactly when the lane group whose scale is raised to 2.0 covers that register byte (the scale's reach).
// Last: does v_cvt_pk_fp8_f32 agree with the library's integer e4m3 rounding on every bf16 value of [-448, 448]?
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 experiments/mfma_scale_probe.hip -o mfma_scale_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

template <int OPSEL>
__global__ void one16(const int* a, const int* b, const int* sa, const int* sb, float* d) {
    const int l = threadIdx.x;
    i32x8_t va, vb;
    for (int i = 0; i < 8; ++i) va[i] = a[l * 8 + i], vb[i] = b[l * 8 + i];
    f32x4_t c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, vb, c, 0, 0, OPSEL, sa[l], OPSEL, sb[l]);
    for (int r = 0; r < 4; ++r) d[l * 4 + r] = c[r];
}
template <int OPSEL>
__global__ void one32(const int* a, const int* b, const int* sa, const int* sb, float* d) {
    const int l = threadIdx.x;
    i32x8_t va, vb;
    for (int i = 0; i < 8; ++i) va[i] = a[l * 8 + i], vb[i] = b[l * 8 + i];
    f32x16_t c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, c, 0, 0, OPSEL, sa[l], OPSEL, sb[l]);
    for (int r = 0; r < 16; ++r) d[l * 16 + r] = c[r];
}

__device__ __host__ static unsigned soft_e4m3(float y) {       // csrc/gemm_mxfp8.hip: mx_e4m3
    unsigned b;
    memcpy(&b, &y, 4);
    const unsigned sign = (b >> 24) & 0x80u;
    unsigned a = b & 0x7fffffffu;
    if (a < 0x3c800000u) {
        float f;
        memcpy(&f, &a, 4);
        f += 16384.0f;
        unsigned u;
        memcpy(&u, &f, 4);
        return sign | (u - 0x46800000u);
    }
    a += 0x7ffffu + ((a >> 20) & 1u);
    return sign | ((a >> 20) - (120u << 3));
}
__global__ void cvt_check(unsigned* mismatches, unsigned* first) {
    const unsigned h = blockIdx.x * blockDim.x + threadIdx.x;      // every bf16 bit pattern
    if (h >= 65536) return;
    const float y = __uint_as_float(h << 16);
    if (!(fabsf(y) <= 448.f)) return;
    const unsigned hw = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(y, 0.f, 0, false) & 0xffu;
    if (hw != soft_e4m3(y) && atomicAdd(mismatches, 1u) == 0) first[0] = h, first[1] = hw, first[2] = soft_e4m3(y);
}

static uint8_t e4m3_of_int(int v) {          // integers -8..8 are e4m3 values
    return (uint8_t)soft_e4m3((float)v);
}

template <typename F>
static void launch(int shape, int opsel, F&& fill, std::vector<float>& out) {
    // fill(a, b, sa, sb): host register images, 64 lanes x 8 ints / 64 scale dwords
    std::vector<int> a(512), b(512), sa(64), sb(64);
    fill(a, b, sa, sb);
    int *da, *db, *dsa, *dsb;
    float* dd;
    const int nd = shape == 16 ? 256 : 1024;
    CK(hipMalloc(&da, 2048)); CK(hipMalloc(&db, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dd, nd * 4));
    CK(hipMemcpy(da, a.data(), 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(dsa, sa.data(), 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, sb.data(), 256, hipMemcpyHostToDevice));
#define GO(K, O) hipLaunchKernelGGL((K<O>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd)
    if (shape == 16) { if (opsel == 0) GO(one16, 0); else if (opsel == 1) GO(one16, 1); else if (opsel == 2) GO(one16, 2); else GO(one16, 3); }
    else { if (opsel == 0) GO(one32, 0); else if (opsel == 1) GO(one32, 1); else if (opsel == 2) GO(one32, 2); else GO(one32, 3); }
#undef GO
    CK(hipDeviceSynchronize());
    out.resize(nd);
    CK(hipMemcpy(out.data(), dd, nd * 4, hipMemcpyDeviceToHost));
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dsa)); CK(hipFree(dsb)); CK(hipFree(dd));
}

// the asymmetric problem: R rows on each side, KK = 2048 / R deep
static int Aval(int i, int k) { return (i * 7 + k * 3) % 17 - 8; }
static int Bval(int j, int k) { return (j * 5 + k * 11 + 3) % 17 - 8; }
static int Asc(int i, int kb) { return 125 + (i + 2 * kb) % 5; }
static int Bsc(int j, int kb) { return 125 + (3 * j + kb) % 5; }

static int kmap(int hyp, int R, int l, int j) {
    const int g = l / R;
    if (hyp == 0) return 32 * g + j;
    return j < 16 ? 16 * g + j : 1024 / R + 16 * g + (j - 16);
}

static bool hypothesis(int shape, int hyp, int opsel) {
    const int R = shape, KK = 2048 / R;
    std::vector<float> d;
    launch(shape, opsel, [&](std::vector<int>& a, std::vector<int>& b, std::vector<int>& sa, std::vector<int>& sb) {
        for (int l = 0; l < 64; ++l) {
            uint8_t ab[32], bb[32];
            for (int j = 0; j < 32; ++j) {
                const int k = kmap(hyp, R, l, j);
                ab[j] = e4m3_of_int(Aval(l % R, k));
                bb[j] = e4m3_of_int(Bval(l % R, k));
            }
            memcpy(&a[l * 8], ab, 32);
            memcpy(&b[l * 8], bb, 32);
            const int kb = hyp == 2 ? l / R : kmap(hyp, R, l, 0) / 32;   // H0 / H1: the block of the lane's first element; H2: block g
            // the byte opsel names carries the scale; the other three carry a different one
            unsigned wa = 0x7a7a7a7au, wb = 0x84848484u;
            wa = (wa & ~(0xffu << (8 * opsel))) | ((unsigned)Asc(l % R, kb) << (8 * opsel));
            wb = (wb & ~(0xffu << (8 * opsel))) | ((unsigned)Bsc(l % R, kb) << (8 * opsel));
            sa[l] = (int)wa;
            sb[l] = (int)wb;
        }
    }, d);
    int bad = 0;
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) {
            double ref = 0;
            for (int k = 0; k < KK; ++k)
                ref += ldexp((double)Aval(i, k), Asc(i, k / 32) - 127) * ldexp((double)Bval(j, k), Bsc(j, k / 32) - 127);
            float got;
            if (shape == 16) got = d[(16 * (i / 4) + j) * 4 + i % 4];
            else got = d[(32 * ((i / 4) % 2) + j) * 16 + 4 * (i / 8) + i % 4];
            if ((double)got != ref) ++bad;
        }
    printf("%dx%d  k map H%d  opsel %d: %s (%d of %d entries differ)\n", shape, shape, hyp, opsel, bad ? "no" : "EXACT", bad, R * R);
    return bad == 0;
}

// discovery kernels: one wave, row 0 / column 0 only.  Slot s = (group s / 32, register byte s % 32) of lane R * group.
template <int R>
__device__ float probe_one(int l, int slot_a, int slot_b, int sgrp_a, int sgrp_b) {
    // slot < 0: the operand is all ones (1.0 = 0x38 in e4m3); sgrp >= 0: that lane group's scale is 2.0, every other 1.0
    i32x8_t va, vb;
    for (int i = 0; i < 8; ++i) {
        va[i] = slot_a < 0 ? 0x38383838 : (l == R * (slot_a >> 5) && i == ((slot_a & 31) >> 2) ? 0x38 << (8 * (slot_a & 3)) : 0);
        vb[i] = slot_b < 0 ? 0x38383838 : (l == R * (slot_b >> 5) && i == ((slot_b & 31) >> 2) ? 0x38 << (8 * (slot_b & 3)) : 0);
    }
    const int sa = (sgrp_a >= 0 && l / R == sgrp_a) ? 128 : 127, sb = (sgrp_b >= 0 && l / R == sgrp_b) ? 128 : 127;
    if (R == 16) {
        f32x4_t c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, vb, c, 0, 0, 0, sa, 0, sb);
        return c[0];
    } else {
        f32x16_t c;
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, c, 0, 0, 0, sa, 0, sb);
        return c[0];
    }
}
template <int R>
__global__ void discover_kernel(unsigned char* reach_a, unsigned char* reach_b) {
    const int l = threadIdx.x, NS = 2048 / R;            // slots per operand row; D[0][0] lives in lane 0, register 0
    for (int s = 0; s < NS; ++s)
        for (int g = 0; g < 64 / R; ++g) {
            const float da = probe_one<R>(l, s, -1, g, -1), db = probe_one<R>(l, -1, s, -1, g);
            if (l == 0) reach_a[s * 4 + g] = da == 2.f ? 1 : (da == 1.f ? 0 : 9), reach_b[s * 4 + g] = db == 2.f ? 1 : (db == 1.f ? 0 : 9);
        }
}

template <int R>
static void discover() {
    const int NS = 2048 / R, NG = 64 / R;
    unsigned char *da, *db;
    CK(hipMalloc(&da, NS * 4)); CK(hipMalloc(&db, NS * 4));
    CK(hipMemset(da, 7, NS * 4)); CK(hipMemset(db, 7, NS * 4));
    hipLaunchKernelGGL((discover_kernel<R>), dim3(1), dim3(64), 0, 0, da, db);
    CK(hipDeviceSynchronize());
    std::vector<unsigned char> ra(NS * 4), rb(NS * 4);
    CK(hipMemcpy(ra.data(), da, NS * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rb.data(), db, NS * 4, hipMemcpyDeviceToHost));
    for (int side = 0; side < 2; ++side) {
        const std::vector<unsigned char>& r = side ? rb : ra;
        printf("%dx%d discovery: %c operand, lane group whose scale reaches (group, byte), bytes 0..31 per row:\n", R, R, side ? 'B' : 'A');
        for (int g = 0; g < NG; ++g) {
            printf("    group %d: ", g);
            for (int j = 0; j < 32; ++j) {
                int who = -1, n = 0;
                for (int gs = 0; gs < NG; ++gs)
                    if (r[(g * 32 + j) * 4 + gs] == 1) who = gs, ++n;
                    else if (r[(g * 32 + j) * 4 + gs] != 0) n = 99;
                printf("%c", n == 1 ? '0' + who : '?');
            }
            printf("\n");
        }
    }
    CK(hipFree(da)); CK(hipFree(db));
}

int main() {
    int ok16 = 0, ok32 = 0;
    hypothesis(16, 0, 0);
    hypothesis(16, 1, 0);
    for (int opsel = 0; opsel < 4; ++opsel) ok16 += hypothesis(16, 2, opsel);
    hypothesis(32, 0, 0);
    hypothesis(32, 1, 0);
    for (int opsel = 0; opsel < 4; ++opsel) ok32 += hypothesis(32, 2, opsel);
    discover<16>();
    discover<32>();
    unsigned *dm, hm[4] = {0, 0, 0, 0};
    CK(hipMalloc(&dm, 16));
    CK(hipMemset(dm, 0, 16));
    hipLaunchKernelGGL(cvt_check, dim3(256), dim3(256), 0, 0, dm, dm + 1);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hm, dm, 16, hipMemcpyDeviceToHost));
    printf("v_cvt_pk_fp8_f32 vs integer e4m3 rounding on bf16 values of [-448, 448]: %u mismatches", hm[0]);
    if (hm[0]) printf(" (first: bf16 0x%04x hw 0x%02x soft 0x%02x)", hm[1], hm[2], hm[3]);
    printf("\nSUMMARY 16x16x128 H2 exact for %d of 4 opsel; 32x32x64 H2 exact for %d of 4 opsel\n", ok16, ok32);
    return (ok16 == 4) ? 0 : 2;
}
