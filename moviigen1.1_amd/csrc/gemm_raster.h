// Workgroup -> output tile for the GEMM kernels (gemm_bf16*.hip, gemm_mxfp8.hip): where in the tile list a workgroup stands, and which
// tile a list position is.  Workgroup ids are dealt round-robin over the 8 XCDs (private 4 MiB L2 each), so XCD x = id & 7.
#pragma once
#include "common.h"

// The XCD split: XCD `xcd` owns the contiguous range [first, first + count) of a list of `total` positions (the first total % 8 XCDs
// one more than the others).  Variants 1 / 2 split their grid (one tile per workgroup: workgroup b stands at first + (b >> 3)); the
// persistent kernels split the tile list, and workgroup b takes position (b >> 3) + i * (grid / 8) of its XCD's range in iteration i.
MG_DEV void mg_xcd_range(int total, int xcd, int& first, int& count) {
    const int q8 = total >> 3, r8 = total & 7;
    first = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    count = q8 + (xcd < r8 ? 1 : 0);
}

// The grouped raster: list position `swz` walks bands of GM row tiles (per_group = GM * tiles_n positions each), column by column inside
// a band (the last band may be shorter), so the tiles that run together share A and W panels in L2.  -> first row / column of the
// BM x BN tile.  (The order of the sum's operands is the one that leaves the kernels' register allocation as it was.)
MG_DEV void mg_tile_of(int swz, int GM, int per_group, int tiles_m, int BM, int BN, int64_t& m0, int& n0) {
    const int group = swz / per_group;
    const int first_m = group * GM;
    const int gsz = (tiles_m - first_m) < GM ? (tiles_m - first_m) : GM;
    const int in_g = swz - group * per_group;
    m0 = (int64_t)(in_g % gsz + first_m) * BM;
    n0 = (in_g / gsz) * BN;
}
