// MXFP8 (OCP e4m3fn elements, one E8M0 scale byte per 32 consecutive k) for the DiT linear layers on gfx950 (CDNA4):
//   mg_quant_mxfp8_rows   bf16 [rows][K] -> e4m3 bytes [rows][K] + scale bytes [rows][K/32]        (HBM-bound)
//   mg_gemm_mxfp8         out[M][N] = A[M][K] . W[N][K]^T on v_mfma_scale_f32_16x16x128_f8f6f4, the bf16 GEMM's epilogues
//   mg_gemm_mxfp8_gelu_q  the same product; the GELU epilogue's bf16 value leaves as MXFP8 (the next GEMM's operand), not as bf16
// The format (include/moviigen_hip.h has the full paragraph): block of 32 with maximum magnitude amax takes
// e = clamp(floor(log2 amax) - 8, -127, 127) (a zero block: -127), scale byte e + 127, element = e4m3_rne(clamp(x 2^-e, +-448)).
//
// GEMM structure = gemm_bf16_v7.hip with the k-tile's BYTES unchanged: a 256 x 256 x 128 tile is 256 rows x 128 bytes per
// operand, exactly variant 7's 256 x 64 bf16 image, so the LDS-DMA pieces, the persistent XCD-contiguous raster and the
// 16x16 epilogue (gemm_epilogue.h: mg_gemm_epilogue16) carry over.  Four waves, one per SIMD, 128 tokens x 128 features
// each: 8 x 8 accumulators of 4 registers; ONE k-step per k-tile = 64 MFMAs of 128 deep.
// Operand map of the instruction (experiments/mfma_scale_probe.hip confirms it, DESIGN.md has the table): lane
// (r = lane & 15, G = lane >> 4) carries row r; its registers 0-3 hold k = 16 G .. 16 G + 15 and its registers 4-7 hold
// k = 64 + 16 G .. 64 + 16 G + 15 (the two halves of the depth), byte order = k order.  The scale byte a lane supplies (byte
// `opsel` of its scale register; byte 0 here) is that of the row's k-block G = k in [32 G, 32 G + 32): NOT the elements the
// lane itself carries.
// LDS image: a lane's 32 bytes are the row's 16-byte chunks G and 4 + G = the chunks lane (r, G) of variant 7 reads in its two
// k-steps, so image, swizzle (chunk c at position c ^ ((row >> 1) & 7)) and the two conflict-free ds_read_b128 per fragment
// (positions t3 and t3 ^ 4) are variant 7's, unchanged.
// Scales: the 4 scale bytes of a row's k-tile are ONE dword of the [rows][K/32] array; thread t DMAs the dword of tile row
// t (4-byte LDS-DMA, lane-linear) for A and for W beside each stage, a lane reads the dword of its row and shifts its
// byte G down.  Weights are the MFMA's A operand (feature rows), activations its B operand (token columns), as in every
// bf16 variant: lane (tok, G) owns token tok of block j and features 16 i + 4 G .. + 3.
// Accumulation: k-tiles ascending, fp32, one workgroup per output tile, no atomics: the result does not depend on the launch.
#include "gemm_epilogue.h"
#include "gemm_launch.h"
#include "gemm_raster.h"
#include "mxfp8_quant.h"

#define MX_BM 256
#define MX_BN 256
#define MX_BK 128                       // e4m3 elements = bytes per row of a k-tile
#define MX_THREADS 256
#define MX_A_BYTES (MX_BM * MX_BK)      // 32 KiB
#define MX_W_BYTES (MX_BN * MX_BK)      // 32 KiB
#define MX_SA_OFF (MX_A_BYTES + MX_W_BYTES)          // scale dwords of the A rows, then of the W rows: 1 KiB each
#define MX_SW_OFF (MX_SA_OFF + MX_BM * 4)
#define MX_STAGE (MX_SW_OFF + MX_BN * 4)             // 66 KiB; two stages = 132 KiB of the CU's 160

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

// LDS reads of the k-loop are inline asm with hand-counted lgkmcnt waits, as in gemm_bf16_v7.hip: hipcc puts a vmcnt(0) in front
// of every C++ LDS read that follows an LDS-DMA in program order (it must assume they alias), and with more than 15 reads in
// flight its own lgkmcnt wait degenerates to lgkmcnt(0).  A wait names the registers it releases as "+v" operands, so nothing
// that uses them (the scale byte extraction, a register copy, the MFMA) can be placed above it.
template <int OFF>
MG_DEV void mx_rd128(i32x4_t& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
template <int OFF>
MG_DEV void mx_rd32(int& d, unsigned addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
// block B (rows 16 B .. 16 B + 15 of the wave's 128) of one operand: the lane's two 16-byte chunks (registers 0-3, 4-7) + its row's scale dword
template <int B>
MG_DEV void mx_rd_block(i32x4_t& lo, i32x4_t& hi, int& sc, unsigned b0, unsigned b1, unsigned sb) {
    mx_rd128<B * 2048>(lo, b0);
    mx_rd128<B * 2048>(hi, b1);
    mx_rd32<B * 64>(sc, sb);
}
template <int N>
MG_DEV void mx_wait1(i32x4_t& lo, i32x4_t& hi, int& sc) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(lo), "+v"(hi), "+v"(sc) : "i"(N) : "memory");
}
template <int N>
MG_DEV void mx_wait4(i32x4_t& l0, i32x4_t& h0, int& s0, i32x4_t& l1, i32x4_t& h1, int& s1, i32x4_t& l2, i32x4_t& h2, int& s2,
                     i32x4_t& l3, i32x4_t& h3, int& s3) {
    asm volatile("s_waitcnt lgkmcnt(%12)"
                 : "+v"(l0), "+v"(h0), "+v"(s0), "+v"(l1), "+v"(h1), "+v"(s1), "+v"(l2), "+v"(h2), "+v"(s2), "+v"(l3), "+v"(h3), "+v"(s3)
                 : "i"(N) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------------
// quantiser
// ---------------------------------------------------------------------------------------------------------------------
// element and scale arithmetic: mxfp8_quant.h (mx_e4m3, mx_block_exp, mx_inv_scale, mx_pack4)
// One wave per row; a lane owns 16 consecutive elements (two 16-byte loads, one 16-byte store), a lane PAIR one 32-block,
// eight lanes the 4 scale bytes of 128 elements = one dword store.  K % 128 == 0 keeps every such group whole.
__global__ __launch_bounds__(256) void quant_mxfp8_rows_kernel(const uint16_t* __restrict__ x, int64_t ldx, int64_t rows, int K,
                                                               uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ sc,
                                                               int64_t lds) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                            // wave-uniform
    const uint16_t* xr = x + row * ldx;
    uint8_t* qr = q + row * ldq;
    uint8_t* sr = sc + row * lds;
    for (int k0 = 0; k0 < K; k0 += 1024) {
        const int k = k0 + lane * 16;
        const bool valid = k < K;
        u32x4_t v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
        if (valid) {
            v0 = *(const u32x4_t*)(xr + k);
            v1 = *(const u32x4_t*)(xr + k + 8);
        }
        float f[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(v0[i] << 16);
            f[2 * i + 1] = __uint_as_float(v0[i] & 0xffff0000u);
            f[8 + 2 * i] = __uint_as_float(v1[i] << 16);
            f[8 + 2 * i + 1] = __uint_as_float(v1[i] & 0xffff0000u);
        }
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(f[i]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        const int e = mx_block_exp(amax);
        const unsigned sbyte = (unsigned)(e + 127);
        const float inv = mx_inv_scale(e);
        unsigned o[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned pk = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float y = f[4 * w + b] * inv;
                y = fminf(fmaxf(y, -448.f), 448.f);                     // clamp BEFORE the conversion: 500 -> 448, never NaN
                pk |= mx_e4m3(y) << (8 * b);
            }
            o[w] = pk;
        }
        const int base = lane & ~7;
        const unsigned s0 = __shfl(sbyte, base, 64), s1 = __shfl(sbyte, base + 2, 64), s2 = __shfl(sbyte, base + 4, 64),
                       s3 = __shfl(sbyte, base + 6, 64);
        if (valid) {
            *(u32x4_t*)(qr + k) = (u32x4_t){o[0], o[1], o[2], o[3]};
            if ((lane & 7) == 0) *(unsigned*)(sr + (k >> 5)) = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
        }
    }
}

extern "C" int mg_quant_mxfp8_rows(const uint16_t* x, int64_t ldx, int64_t rows, int K, uint8_t* q, int64_t ldq,
                                   uint8_t* scales, int64_t lds, void* stream) {
    if (!x || !q || !scales) return MG_ERR_ARG;
    if (rows < 0 || K <= 0 || (K % 128) || ldx < K || ldq < K || lds < K / 32) return MG_ERR_SHAPE;
    if ((ldx & 7) || (ldq & 15) || (lds & 3)) return MG_ERR_SHAPE;
    if (((uintptr_t)x & 15) || ((uintptr_t)q & 15) || ((uintptr_t)scales & 3)) return MG_ERR_SHAPE;
    if (rows == 0) return MG_OK;
    const int64_t blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffLL) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(quant_mxfp8_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, rows, K, q,
                       ldq, scales, lds);
    return mg_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------
// EPI of the kernel only (mg_gemm_mxfp8_gelu_q): the GELU epilogue whose bf16 value is stored as e4m3 bytes (out, ldo) + scale bytes
// (qo.s, qo.lds).  The MG_EPI_* instantiations take an empty struct there: ONE kernel text, and their code does not change.
#define MX_EPI_GELU_Q 100
template <bool Q>
struct MxQOut {};
template <>
struct MxQOut<true> {
    uint8_t* s;
    int64_t lds;
};

template <int EPI>
__global__ __launch_bounds__(MX_THREADS, 1) void gemm_mxfp8_kernel(
    const uint8_t* __restrict__ A, int64_t lda, const uint8_t* __restrict__ As, int64_t ldas,
    const uint8_t* __restrict__ Wt, int64_t ldw, const uint8_t* __restrict__ Ws, int64_t ldws,
    const float* __restrict__ bias, int64_t M, int N, int K, void* __restrict__ out, int64_t ldo,
    const float* __restrict__ gate, int tiles_m, int tiles_n, MxQOut<EPI == MX_EPI_GELU_Q> qo) {
    __shared__ __attribute__((aligned(16))) char smem[2 * MX_STAGE];

    const int nwg = gridDim.x, bid = blockIdx.x;
    const int total = tiles_m * tiles_n;
    // variant 7's raster (gemm_raster.h): workgroup b of XCD b & 7 takes, in iteration i, position i * (nwg / 8) + (b >> 3) of its XCD's
    // contiguous range of the tile list; 4 x 256-token bands x all feature panels per group
    int xcd_first, xcd_count;
    mg_xcd_range(total, bid & 7, xcd_first, xcd_count);
    const int per_iter = nwg >> 3;        // host guarantees nwg % 8 == 0
    const int GM = 4;
    const int per_group = GM * tiles_n;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, r16 = lane & 15, G = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;     // 2 (token) x 2 (feature) waves, 128 x 128 each
    const int srow = lane >> 3;
    constexpr int NP = 16;                       // LDS-DMA duty: wave w stages rows [64w, 64w+64) of A (pieces 0-7) and of W (8-15)
    const int prow0 = wave * 64;

    auto tile_of = [&](int pos, int64_t& m0, int& n0) __attribute__((always_inline)) {
        mg_tile_of(xcd_first + pos, GM, per_group, tiles_m, MX_BM, MX_BN, m0, n0);
    };
    const uint8_t* gp[NP];
    const uint8_t *gsa, *gsw;                    // this thread's scale dwords: tile row tid of A and of W
    auto set_pointers = [&](int64_t m0, int n0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int row = prow0 + (i & 7) * 8 + srow;
            const int c = (lane & 7) ^ ((row >> 1) & 7);          // the row's 16-byte chunk stored at this LDS position (variant 7's swizzle)
            if (i < 8) {
                int64_t am = m0 + row;
                if (am > M - 1) am = M - 1;                       // rows past the end re-read the last one; the epilogue drops them
                gp[i] = A + am * lda + (c << 4);
            } else {
                int wr = n0 + row;
                if (wr > N - 1) wr = N - 1;
                gp[i] = Wt + (int64_t)wr * ldw + (c << 4);
            }
        }
        int64_t am = m0 + tid;
        if (am > M - 1) am = M - 1;
        int wr = n0 + tid;
        if (wr > N - 1) wr = N - 1;
        gsa = As + am * ldas;
        gsw = Ws + (int64_t)wr * ldws;
    };
    auto piece_lds = [&](int p) __attribute__((always_inline)) {
        return (p < 8 ? 0 : MX_A_BYTES) + (prow0 + (p & 7) * 8) * 128;
    };

    const int sw = (r16 >> 1) & 7;            // (row >> 1) & 7 of the lane's row in every 16-row block
    const int t3 = G ^ sw;                    // position of chunk G; chunk 4 + G: t3 ^ 4
    const int a_off0 = (wm * 128 + r16) * 128 + (t3 << 4), a_off1 = (wm * 128 + r16) * 128 + ((t3 ^ 4) << 4);
    const int w_off0 = MX_A_BYTES + (wn * 128 + r16) * 128 + (t3 << 4), w_off1 = MX_A_BYTES + (wn * 128 + r16) * 128 + ((t3 ^ 4) << 4);
    const int sa_off = MX_SA_OFF + (wm * 128 + r16) * 4, sw_off = MX_SW_OFF + (wn * 128 + r16) * 4;
    const int sshift = G * 8;
    const unsigned lds0 = (unsigned)(uintptr_t)(mg_lptr_t)smem;
    const int nk = K / MX_BK;

    int pos = bid >> 3;
    if (pos >= xcd_count) return;
    int64_t m0;
    int n0;
    tile_of(pos, m0, n0);
    set_pointers(m0, n0);
    {   // cold start of the FIRST tile only
#pragma unroll
        for (int i = 0; i < NP; ++i) mg_glds16(gp[i], smem + piece_lds(i));
        mg_glds4(gsa, smem + MX_SA_OFF + wave * 256);
        mg_glds4(gsw, smem + MX_SW_OFF + wave * 256);
    }
    int gk = 0;                                   // k-tiles consumed so far by this workgroup: stage = gk & 1
    for (;;) {
        f32x4_t acc[8][8];       // [feature block of 16][token block of 16]
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const int next_pos = pos + per_iter;
        const bool has_next = next_pos < xcd_count;
        int64_t m0n = m0;
        int n0n = n0;
        for (int kt = 0; kt < nk; ++kt, ++gk) {
            // k-tile kt landed (every piece of it), and everyone is past the fragment reads of the previous one
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            int koff2 = (kt + 1) * MX_BK, soff2 = (kt + 1) * 4;
            if (kt == nk - 1) {   // refill slot of the last k-tile: the first k-tile of the NEXT tile (or a redundant re-load)
                koff2 = has_next ? 0 : kt * MX_BK;
                soff2 = has_next ? 0 : kt * 4;
                if (has_next) {
                    tile_of(next_pos, m0n, n0n);
                    set_pointers(m0n, n0n);
                }
            }
            char* lnext = smem + ((gk + 1) & 1) * MX_STAGE;
            // Fragment reads in 16 slots of 3 LDS operations (low half, high half, scale dword), in the order the MFMA groups need them:
            // slot 0 = feature block 0, 1..4 = token blocks 0..3, 5..11 = feature blocks 1..7, 12..15 = token blocks 4..7.  Slots 0..7
            // go out before group 0, two more behind each of groups 0..3.  Group g waits for its newest slot (0: slot 4, 1..7: slot
            // 4 + g, 8: all) = lgkmcnt(3 x (slots issued - slots needed)), capped at the field's 15: 9, 12, 15, 15, 15, 15, 15, 12, 0.
            const unsigned lsb = lds0 + (gk & 1) * MX_STAGE;
            const unsigned wb0 = lsb + w_off0, wb1 = lsb + w_off1, ab0 = lsb + a_off0, ab1 = lsb + a_off1, sab = lsb + sa_off,
                           swb = lsb + sw_off;
            i32x4_t fal[8], fah[8], fwl[8], fwh[8];
            int sa[8], sw8[8];
            auto slot = [&](int s) __attribute__((always_inline)) {
                switch (s) {   // compile-time after unrolling
                    case 0: mx_rd_block<0>(fwl[0], fwh[0], sw8[0], wb0, wb1, swb); break;
                    case 1: mx_rd_block<0>(fal[0], fah[0], sa[0], ab0, ab1, sab); break;
                    case 2: mx_rd_block<1>(fal[1], fah[1], sa[1], ab0, ab1, sab); break;
                    case 3: mx_rd_block<2>(fal[2], fah[2], sa[2], ab0, ab1, sab); break;
                    case 4: mx_rd_block<3>(fal[3], fah[3], sa[3], ab0, ab1, sab); break;
                    case 5: mx_rd_block<1>(fwl[1], fwh[1], sw8[1], wb0, wb1, swb); break;
                    case 6: mx_rd_block<2>(fwl[2], fwh[2], sw8[2], wb0, wb1, swb); break;
                    case 7: mx_rd_block<3>(fwl[3], fwh[3], sw8[3], wb0, wb1, swb); break;
                    case 8: mx_rd_block<4>(fwl[4], fwh[4], sw8[4], wb0, wb1, swb); break;
                    case 9: mx_rd_block<5>(fwl[5], fwh[5], sw8[5], wb0, wb1, swb); break;
                    case 10: mx_rd_block<6>(fwl[6], fwh[6], sw8[6], wb0, wb1, swb); break;
                    case 11: mx_rd_block<7>(fwl[7], fwh[7], sw8[7], wb0, wb1, swb); break;
                    case 12: mx_rd_block<4>(fal[4], fah[4], sa[4], ab0, ab1, sab); break;
                    case 13: mx_rd_block<5>(fal[5], fah[5], sa[5], ab0, ab1, sab); break;
                    case 14: mx_rd_block<6>(fal[6], fah[6], sa[6], ab0, ab1, sab); break;
                    default: mx_rd_block<7>(fal[7], fah[7], sa[7], ab0, ab1, sab); break;
                }
            };
#pragma unroll
            for (int s = 0; s < 8; ++s) slot(s);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int grp = 0; grp < 16; ++grp) {          // group = 4 MFMAs: token half h = grp >> 3, feature block i = grp & 7
                const int h = grp >> 3, i = grp & 7;
                if (grp == 0) {
                    mx_wait1<9>(fwl[0], fwh[0], sw8[0]);
                    mx_wait4<9>(fal[0], fah[0], sa[0], fal[1], fah[1], sa[1], fal[2], fah[2], sa[2], fal[3], fah[3], sa[3]);
                } else if (grp == 1 || grp == 7) {
                    mx_wait1<12>(fwl[i], fwh[i], sw8[i]);
                } else if (grp < 7) {
                    mx_wait1<15>(fwl[i], fwh[i], sw8[i]);
                } else if (grp == 8) {
                    mx_wait4<0>(fal[4], fah[4], sa[4], fal[5], fah[5], sa[5], fal[6], fah[6], sa[6], fal[7], fah[7], sa[7]);
                }
                __builtin_amdgcn_sched_barrier(0);
                const int ws_i = (sw8[i] >> sshift) & 0xff;
                const i32x8_t fw = __builtin_shufflevector(fwl[i], fwh[i], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int j = 4 * h; j < 4 * h + 4; ++j) {
                    const i32x8_t fa = __builtin_shufflevector(fal[j], fah[j], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa, acc[i][j], 0, 0, 0, ws_i, 0,
                                                                                 (sa[j] >> sshift) & 0xff);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (grp < 4) {
                    slot(8 + 2 * grp);
                    slot(9 + 2 * grp);
                }
                mg_glds16(gp[grp] + koff2, lnext + piece_lds(grp));     // one LDS-DMA piece of the next k-tile per group
                if (grp == 14) mg_glds4(gsa + soff2, lnext + MX_SA_OFF + wave * 256);
                if (grp == 15) mg_glds4(gsw + soff2, lnext + MX_SW_OFF + wave * 256);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- epilogue (gemm_epilogue.h) of THIS tile; the next tile's first k-tile is already on its way ----
        if constexpr (EPI == MX_EPI_GELU_Q)
            mg_gemm_epilogue16_gelu_q<8, 8>(acc, m0 + wm * 128, n0 + wn * 128, r16, G, M, N, bias, (uint8_t*)out, ldo, qo.s, qo.lds);
        else
            mg_gemm_epilogue16<EPI, 8, 8>(acc, m0 + wm * 128, n0 + wn * 128, r16, G, M, N, bias, gate, out, ldo);
        if (!has_next) break;
        pos = next_pos;
        m0 = m0n;
        n0 = n0n;
    }
}

// what both entry points ask of the operands: the checks every GEMM shares (gemm_launch.h), then the scale arrays, N and pitch >= extent
static int mx_gemm_check(const uint8_t* Aq, int64_t lda, const uint8_t* As, int64_t ldas, const uint8_t* Wq, int64_t ldw,
                         const uint8_t* Ws, int64_t ldws, const float* bias, const float* gate, int64_t M, int N, int K) {
    if (!As || !Ws) return MG_ERR_ARG;
    const int rc = mg_gemm_check_operands(Aq, lda, Wq, ldw, bias, gate, M, N, K, MX_BK, 16);
    if (rc != MG_OK) return rc;
    if ((N % 16) || lda < K || ldw < K || ldas < K / 32 || ldws < K / 32) return MG_ERR_SHAPE;
    if ((ldas & 3) || (ldws & 3) || ((uintptr_t)As & 3) || ((uintptr_t)Ws & 3)) return MG_ERR_SHAPE;
    return MG_OK;
}

extern "C" int mg_gemm_mxfp8(const uint8_t* Aq, int64_t lda, const uint8_t* As, int64_t ldas, const uint8_t* Wq, int64_t ldw,
                             const uint8_t* Ws, int64_t ldws, const float* bias, int64_t M, int N, int K, int epilogue,
                             void* out, int64_t ldo, const float* gate, void* stream) {
    if (!out) return MG_ERR_ARG;
    int rc = mx_gemm_check(Aq, lda, As, ldas, Wq, ldw, Ws, ldws, bias, gate, M, N, K);
    if (rc == MG_ERR_ARG || epilogue < 0 || epilogue > 3) return MG_ERR_ARG;
    if (rc != MG_OK) return rc;
    if (ldo < N || (ldo & 3) || ((uintptr_t)out & 15)) return MG_ERR_SHAPE;
    if (M == 0) return MG_OK;
    int tiles_m, tiles_n, nwg;      // one workgroup per CU (132 KiB LDS)
    if ((rc = mg_gemm_persistent_grid(M, N, MX_BM, MX_BN, &tiles_m, &tiles_n, &nwg)) != MG_OK) return rc;
    const dim3 grid((unsigned)nwg), block(MX_THREADS);
    MG_GEMM_FOR_EPILOGUE(epilogue, hipLaunchKernelGGL((gemm_mxfp8_kernel<EPI>), grid, block, 0, (hipStream_t)stream, Aq, lda, As, ldas, Wq, ldw, Ws,
                                                      ldws, bias, M, N, K, out, ldo, gate, tiles_m, tiles_n, MxQOut<false>{}));
    return mg_check_launch();
}

extern "C" int mg_gemm_mxfp8_gelu_q(const uint8_t* Aq, int64_t lda, const uint8_t* As, int64_t ldas, const uint8_t* Wq,
                                    int64_t ldw, const uint8_t* Ws, int64_t ldws, const float* bias, int64_t M, int N, int K,
                                    uint8_t* oq, int64_t ldoq, uint8_t* oscales, int64_t ldos, void* stream) {
    if (!oq || !oscales) return MG_ERR_ARG;
    int rc = mx_gemm_check(Aq, lda, As, ldas, Wq, ldw, Ws, ldws, bias, nullptr, M, N, K);
    if (rc != MG_OK) return rc;
    if ((N % 32) || ldoq < N || ldos < N / 32 || (ldoq & 15) || (ldos & 3)) return MG_ERR_SHAPE;
    if (((uintptr_t)oq & 15) || ((uintptr_t)oscales & 3)) return MG_ERR_SHAPE;
    if (M == 0) return MG_OK;
    int tiles_m, tiles_n, nwg;
    if ((rc = mg_gemm_persistent_grid(M, N, MX_BM, MX_BN, &tiles_m, &tiles_n, &nwg)) != MG_OK) return rc;
    const MxQOut<true> qo = {oscales, ldos};
    hipLaunchKernelGGL((gemm_mxfp8_kernel<MX_EPI_GELU_Q>), dim3((unsigned)nwg), dim3(MX_THREADS), 0, (hipStream_t)stream, Aq, lda,
                       As, ldas, Wq, ldw, Ws, ldws, bias, M, N, K, (void*)oq, ldoq, (const float*)nullptr, tiles_m, tiles_n, qo);
    return mg_check_launch();
}
