// The element and scale arithmetic of the project's MXFP8 format (include/moviigen_hip.h has the full paragraph), shared by every
// kernel that WRITES it: the stand-alone quantiser and the GELU-quantising GEMM epilogue (gemm_mxfp8.hip, gemm_epilogue.h) and the
// quantising LayerNorm (dit_elementwise.hip).  One text, so that all producers emit the same bytes for the same bf16 value.
#pragma once
#include "common.h"

// fp32 -> e4m3fn, round to nearest even, |y| <= 448 on entry (the caller clamps first).  Integer arithmetic, so that the
// bytes are defined by this text and not by a conversion instruction's mode bits: normal range rounds the 23-bit mantissa
// to 3 bits with the carry running into the exponent; below 2^-6 the sum y + 2^14 leaves round(y * 2^9) in its low bits.
MG_DEV unsigned mx_e4m3(float y) {
    const unsigned b = __float_as_uint(y), sign = (b >> 24) & 0x80u;
    unsigned a = b & 0x7fffffffu;
    if (a < 0x3c800000u)                                               // < 2^-6: e4m3 subnormal (or zero)
        return sign | (__float_as_uint(__uint_as_float(a) + 16384.0f) - 0x46800000u);
    a += 0x7ffffu + ((a >> 20) & 1u);
    return sign | ((a >> 20) - (120u << 3));
}

// e of a block whose maximum magnitude is amax (finite, >= 0): floor(log2 amax) - 8 = the biased exponent - 127 - 8 (a bf16
// subnormal or zero lands below the lower clamp either way; the upper clamp, 127, cannot be reached from a finite fp32).
// The scale byte is e + 127.
MG_DEV int mx_block_exp(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127 - 8;
    return e < -127 ? -127 : e;
}
// 2^-e, 127 - e in [8, 254]
MG_DEV float mx_inv_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }

// four consecutive elements -> one dword of e4m3 bytes (byte order = element order); clamp BEFORE the conversion: 500 -> 448, never NaN
MG_DEV unsigned mx_pack4(float f0, float f1, float f2, float f3, float inv) {
    const float f[4] = {f0, f1, f2, f3};
    unsigned pk = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float y = f[b] * inv;
        y = fminf(fmaxf(y, -448.f), 448.f);
        pk |= mx_e4m3(y) << (8 * b);
    }
    return pk;
}
