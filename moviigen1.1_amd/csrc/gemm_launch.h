// Host side of the GEMM family (gemm_bf16*.hip, gemm_mxfp8.hip), once: the launchers' prototypes, the operand checks the entry points
// share, the tile grid, the persistent grid and the run-time epilogue -> template argument dispatch.  Everything here is static /
// inline or a declaration: no symbol of its own.
#pragma once
#include "common.h"
#include "../../include/moviigen_hip.h"

// ---- the tile variants behind mg_gemm_bf16 (gemm_bf16.hip picks one by shape; variant 1 lives there) ---------------------------------
#define MG_GEMM_LAUNCH_ARGS                                                                                                       \
    const uint16_t *A, int64_t lda, const uint16_t *Wt, int64_t ldw, const float *bias, int64_t M, int N, int K, int epilogue, \
        void *out, int64_t ldo, const float *gate, hipStream_t st
int mg_gemm_v2_launch(MG_GEMM_LAUNCH_ARGS);       // gemm_bf16_v2.hip
int mg_gemm_v12_launch(MG_GEMM_LAUNCH_ARGS);      // gemm_bf16_v12.hip
// the measurement partners, switches and s_memtime hook that only the A/B library (-DMG_AB_BUILD) defines
int mg_gemm_v7_launch(MG_GEMM_LAUNCH_ARGS);       // gemm_bf16_v7.hip
int mg_gemm_v8_launch(MG_GEMM_LAUNCH_ARGS);       // gemm_bf16_v8.hip
int mg_gemm_v11_launch(MG_GEMM_LAUNCH_ARGS);      // gemm_bf16_v11.hip
void mg_gemm_v11_set_flags(int f);
void mg_gemm_v12_set_flags(int f);
extern unsigned long long* g_gemm5_prof;          // gemm_bf16.hip (mg_gemm5_debug_profile): the 256x256 kernels (7, 8, 11, 12)

// ---- operand checks common to mg_gemm_bf16, mg_gemm_mxfp8 and mg_gemm_mxfp8_gelu_q ---------------------------------------------------
// A [M][K] and W [N][K], both K-contiguous with pitches in elements; `per16` = elements per 16 bytes, the unit of the LDS-DMA staging.
// A null operand is MG_ERR_ARG and is looked for first; everything else is MG_ERR_SHAPE.  The caller adds what only its family asks
// (outputs, scale arrays, N rules) and treats M == 0 behind all of it.
static inline int mg_gemm_check_operands(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* gate,
                                         int64_t M, int N, int K, int BK, int per16) {
    if (!A || !W) return MG_ERR_ARG;
    if (M < 0 || N <= 0 || K <= 0 || (K % BK) || ((lda | ldw) & (per16 - 1))) return MG_ERR_SHAPE;
    if ((((uintptr_t)A | (uintptr_t)W) & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)gate & 15)) return MG_ERR_SHAPE;      // bias, gate: may be null
    return MG_OK;
}

// ---- grids -----------------------------------------------------------------------------------------------------------------------------
// output tiles of BM x BN; their product must fit the kernels' 31-bit tile index
static inline int mg_gemm_tile_grid(int64_t M, int N, int BM, int BN, int* tiles_m, int* tiles_n) {
    const int64_t tiles_m64 = (M + BM - 1) / BM;
    *tiles_n = (N + BN - 1) / BN;
    if (tiles_m64 * *tiles_n > 0x7fffffffLL) return MG_ERR_SHAPE;
    *tiles_m = (int)tiles_m64;
    return MG_OK;
}
// the persistent kernels' grid: one workgroup per CU walks the tile list (gemm_raster.h), always a multiple of the 8 XCDs; with fewer
// tiles than CUs one iteration, the idle workgroups return at once.  The device is asked first, as the launchers always did:
// MG_ERR_LAUNCH comes before the tile grid's MG_ERR_SHAPE.
static inline int mg_gemm_persistent_grid(int64_t M, int N, int BM, int BN, int* tiles_m, int* tiles_n, int* nwg) {
    const int n_cu = mg_persistent_cus();
    if (n_cu < 0) return MG_ERR_LAUNCH;
    const int rc = mg_gemm_tile_grid(M, N, BM, BN, tiles_m, tiles_n);
    if (rc != MG_OK) return rc;
    const int total = *tiles_m * *tiles_n;
    *nwg = total < n_cu ? (total + 7) & ~7 : n_cu;
    return MG_OK;
}

// ---- epilogue dispatch ---------------------------------------------------------------------------------------------------------------
// runs the statement(s) given once, with the constant EPI = the run-time `epilogue` for a template argument.  The entry points have
// refused numbers outside 0..3 (MG_ERR_ARG) before a launcher gets here.
#define MG_GEMM_FOR_EPILOGUE(epilogue, ...)                                                                  \
    switch (epilogue) {                                                                                      \
        case MG_EPI_BIAS_BF16: { constexpr int EPI = MG_EPI_BIAS_BF16; __VA_ARGS__; } break;                 \
        case MG_EPI_BIAS_GELU_BF16: { constexpr int EPI = MG_EPI_BIAS_GELU_BF16; __VA_ARGS__; } break;       \
        case MG_EPI_GATE_RESID_F32: { constexpr int EPI = MG_EPI_GATE_RESID_F32; __VA_ARGS__; } break;       \
        default: { constexpr int EPI = MG_EPI_BIAS_F32; __VA_ARGS__; } break;                                \
    }
