// Tile geometry of the four GEMM / conv kernel families: what the dispatch plan (gemm_plan.cpp, no kernel in it) and the kernels agree on.
#pragma once
#include "common.h"

namespace SDNS {

constexpr int BM = 128;              // tiled kernel (gemm.hip): rows per tile
constexpr int BK = 64;               //   and K elements per step
constexpr int PP_ROWS = 256;         // ping-pong kernel (gemm_pp.hip): rows per tile
constexpr int HALO_SIDE = 16;        // halo conv (conv_halo.hip): a tile is a HALO_SIDE x HALO_SIDE block of output pixels
constexpr int HALO_ROWS = HALO_SIDE * HALO_SIDE;
constexpr int WS_ROWS = 128;         // weight-stationary kernel (gemm_ws.hip): rows per tile
constexpr int WS_PIECES = 100;       //   (n-tile, k-step) pieces of a column group: 10 x 10 at K = 320, 5 x 20 at K = 640
constexpr int ws_group_cols(int K) { return WS_PIECES / (K / 32) * 16; }     // columns per group

}  // namespace SDNS
