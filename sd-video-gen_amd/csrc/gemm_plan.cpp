// Which kernel a GEMM / 3x3-conv problem runs on: family, column-tile width, split-K factor and what its epilogue can emit, decided ONCE
// per launch as a value (GemmPlan).  Pure host code of GemmArgs and the $SVG_* switches: no kernel here, none included, so the whole
// policy is testable without a GPU (tools/host_sanitize/gemm_plan_dump.cpp, tests/test_gemm_plan_cpu.py).  The callers ask gemm_plan(),
// fill gn_part / ln_part from it and hand the same plan to gemm_auto(), which launches it without deciding again.
#include "kernels.h"
#include <algorithm>
#include <cstdlib>

namespace SDNS {

namespace {

// column-tile width of {128, 160}: fewest serial rounds of workgroups (one per CU, 256 CUs) times the width — workgroups beyond one per CU
// share the matrix pipe; ties go to the width with fewer padded columns, then (tie_wider) to the wider tile
int search_bn(int64_t row_tiles, int N, bool tie_wider) {
  int best = 128;
  int64_t best_cost = -1, best_pad = 0;
  for (int bn : {128, 160}) {
    const int64_t tn = cdiv(N, bn);
    const int64_t cost = ((row_tiles * tn + 255) / 256) * bn, pad = tn * bn - N;
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && (pad < best_pad || (tie_wider && pad == best_pad && bn > best)))) {
      best = bn; best_cost = cost; best_pad = pad;
    }
  }
  return best;
}

// ---- halo conv: stride-1 3x3 convs on images whose sides are multiples of 16, with enough 16x16-pixel blocks x channel tiles to give
// every CU a workgroup (below that the 128-row implicit GEMM with its split-K is faster: same-box A/B at 16x16 images)
bool conv_halo_supported(const GemmArgs& g, int* bn) {
  const int off = (int)svg_env_i64("SVG_NO_HALO", 0);
  const int up_on = (int)svg_env_i64("SVG_HALO_UP2", 1);
  const bool s1 = g.amode == A_CONV_S1 && g.Ho == g.H && g.Wo == g.W;
  const bool up = up_on && g.amode == A_CONV_UP2 && g.Ho == 2 * g.H && g.Wo == 2 * g.W && !g.A2;
  if (off || !(s1 || up) || g.Cin % 64 != 0 || g.Ho % HALO_SIDE != 0 || g.Wo % HALO_SIDE != 0 || g.batch != 1 || g.out_f32 == 1 ||
      g.act == ACT_GEGLU || g.N < 128)
    return false;
  const int min_wg = (int)svg_env_i64("SVG_HALO_MIN", 192);      // (cached lookup; svg_env_refresh re-reads it: the parity tests force the kernel at batch 1-2)
  *bn = search_bn(g.M / HALO_ROWS, g.N, false);
  return (int64_t)(g.M / HALO_ROWS) * cdiv(g.N, *bn) >= min_wg;
}

// split-K partitions the 64-channel chunks
int conv_halo_splitk(const GemmArgs& g, int bn) {
  const int64_t blocks = (int64_t)(g.M / HALO_ROWS) * cdiv(g.N, bn);
  const int CC = g.Cin / 64;
  const int tgt = (int)svg_env_i64("SVG_HALO_SPLIT_TGT", 320);
  if (blocks < 192 && CC >= 4) return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((tgt + blocks - 1) / blocks, CC / 2), 8));
  return 1;
}

// ---- weight-stationary: dense, 16-bit output, K = 320, whole column groups, unbatched (one W for all rows), no GEGLU / row bias /
// per-sample bias / swapped LayerNorm / two-source A
bool gemm_ws_supported(const GemmArgs& g) {
  const int on = (int)svg_env_i64("SVG_GEMM_WS", 1);
  if (!on) return false;
  if (g.amode != A_DENSE || g.A2 || g.out_f32 || g.act == ACT_GEGLU || g.bias_row || g.bias_bn || g.ln_swapped || g.batch != 1) return false;
  // K = 640 (80-column groups) builds and is correct but loses: two register sets of 80 A-fragment registers spill, and eight /
  // sixteen column groups re-read A that often (69 vs 53 us at 28672 x 640 x 640): the tiled kernel keeps those shapes
  if (g.K != 320) return false;
  const int gc = ws_group_cols(g.K);
  if (g.N % gc != 0 || g.N > 1280 || (g.n_valid > 0 && g.n_valid < g.N)) return false;
  if (g.residual && (g.ldr & 7)) return false;            // 16-byte residual loads / stores (8 consecutive columns per lane)
  if ((g.lda & 7) || (g.ldc & 7) || (g.ldb & 7)) return false;
  if (g.vt_out && (g.vt_n0 % gc != 0 || g.vt_rows % 16 != 0 || (g.vt_ld & 3) || g.residual || g.gn_part || g.ln_part || g.act != ACT_NONE)) return false;
  if (g.M < 16384) return false;                        // the tiled kernel's territory: too few 128-row tiles per CU to amortise the W load
  return true;
}

// ---- ping-pong: dense, unbatched, K a multiple of 64 and long enough, enough 256-row tiles to give every CU a workgroup
bool gemm_pp_supported(const GemmArgs& g, int* bn) {
  const int on = (int)svg_env_i64("SVG_GEMM_PP", 1);
  const int min_kt = (int)svg_env_i64("SVG_GEMM_PP_MINKT", 16);
  // wide outputs (the GEGLU projection at 32 x 32: N = 5120, K = 640) amortise the tile's unhidden prologue over enough columns at
  // 10 slabs already: 0.248 against 0.258-0.262 ms on the 128-row kernel, same box; N = 1280 at K = 640 loses (0.081 against 0.073)
  const int need_kt = g.N >= 2560 ? std::min(min_kt, 10) : min_kt;
  if (!on || g.amode != A_DENSE || g.batch != 1 || g.out_f32 || (g.K & 63) != 0 || (g.K >> 6) < need_kt || g.A2) return false;
  if (g.lda % 8 != 0 || g.ldb % 8 != 0 || g.bias_row) return false;
  *bn = g.act == ACT_GEGLU ? 128 : search_bn(cdiv(g.M, PP_ROWS), g.N, false);
  return (int64_t)cdiv(g.M, PP_ROWS) * cdiv(g.N, *bn) >= 192;
}

// ---- tiled kernel: takes everything else
int pick_bn(const GemmArgs& g) {
  const int force = (int)svg_env_i64("SVG_GEMM_BN", 0);
  if (force && g.act != ACT_GEGLU && g.N > 64) return force;
  if (g.act == ACT_GEGLU) return 128;
  if (g.out_f32 != 2) {                 // (the f32 stream has 128 / 160-column instantiations only)
    if (g.N <= 32) return 32;
    if (g.N <= 64) return 64;
  }
  const int64_t tm = (int64_t)cdiv(g.M, BM) * g.batch;
  // the 8 x 8 level's convolutions (1792 rows, K = 11520 / 23040): 14 x 8 tiles of 160 columns x split-K 4 = 448 workgroups, two per CU in
  // one wave of the grid: 0.067 / 0.115 ms against 0.073 / 0.121 for 128 columns x split-K 3 (profiles/r04_kbench_8x8_sweep.txt)
  if (g.amode != A_DENSE && g.N % 160 == 0 && tm * (g.N / 160) < 192) return 160;
  return search_bn(tm, g.N, true);      // (wider on a full tie: the A panel is re-read once per column tile)
}

int igemm_splitk(const GemmArgs& g, int bn) {
  const int64_t blocks = (int64_t)cdiv(g.M, BM) * cdiv(g.N, bn) * g.batch;
  const int KT = cdiv(g.K, BK);
  {
    const int force = (int)svg_env_i64("SVG_IGEMM_SK", 0);     // experiments: split-K of the tiled kernel for launches below 192 tiles
    if (force > 0 && blocks < 192 && KT >= 8) return std::min(force, KT / 4);
  }
  if (blocks < 192 && KT >= 8) {
    const int tgt = g.amode != A_DENSE ? 448 : 384;
    const int sk = (int)std::min<int64_t>((tgt + blocks - 1) / blocks, KT / 4);
    return std::max(1, std::min(sk, 16));
  }
  // about one workgroup (4 waves) per CU and a long K: a single wave per SIMD cannot hide its own load phases, so
  // split in two for two co-resident workgroups (same-box A/B at 16 x 16 x 1280 convs: 0.149 -> 0.122 ms)
  if (blocks < 300 && KT >= 64) return 2;
  return 1;
}

}  // namespace

GemmPlan gemm_plan(const GemmArgs& g0) {
  GemmArgs g = g0;
  if (g.n_valid <= 0) g.n_valid = g.N;
  GemmPlan p;
  int rows = 0, col_tiles = 0;      // of the family's tile: rows per GroupNorm partial, LayerNorm partials per row
  if (conv_halo_supported(g, &p.bn)) {
    p.family = GF_HALO; p.splitk = conv_halo_splitk(g, p.bn);
    rows = HALO_ROWS;                // (a conv never feeds a LayerNorm)
  } else if (gemm_ws_supported(g)) {
    p.family = GF_WS; p.bn = ws_group_cols(g.K);
    rows = WS_ROWS; col_tiles = g.N / p.bn;          // one partial per row and column group
  } else if (gemm_pp_supported(g, &p.bn)) {
    p.family = GF_PP;
    rows = PP_ROWS; col_tiles = cdiv(g.N, p.bn);
  } else {
    p.family = GF_IGEMM; p.bn = pick_bn(g); p.splitk = igemm_splitk(g, p.bn);
    rows = p.bn >= 32 ? BM : 0; col_tiles = p.bn >= 128 ? cdiv(g.N, p.bn) : 0;
  }
  // the statistics come from the tile epilogue's stored values: not from split-K slabs, GEGLU pairs, columns the output does not hold,
  // or the fused q | k | V^T form (gemm_ws_supported refuses it with gn_part / ln_part set: the answer must not change once they are)
  const bool emits = p.splitk == 1 && g.act != ACT_GEGLU && g.N <= g.ldc && !g.vt_out;
  if (emits && g.out_f32 != 1 && g.batch == 1) p.gn_rows = rows;
  if (emits && !g.out_f32 && g.amode == A_DENSE && !g.bias_row) p.ln_tiles = col_tiles;
  return p;
}

}  // namespace SDNS
