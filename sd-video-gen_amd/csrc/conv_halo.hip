// Halo 3x3 convolution (stride 1, pad 1) for gfx950: the L2-traffic-lean form of the implicit GEMM.
//
// The plain implicit GEMM (gemm.hip) re-loads its 128-pixel A tile once per tap: 9x the input through L2 -> LDS.
// Measured on MI355X that traffic runs at ~39 % of the L2 rate while the matrix pipe is ~38 % busy — at a 128 x 160
// tile the two limits coincide.  Here a workgroup owns a 16 x 16 PIXEL BLOCK (256 output pixels) x BN channels:
//   * per 64-channel chunk it DMAs the block's 18 x 18 halo patch ONCE (41 KB) and reads all nine taps out of LDS at
//     shifted pixel addresses (the activation fragment of tap (ky,kx), pixel (y,x) is patch pixel (y+ky, x+kx));
//   * only the weights stream per tap (BN x 64, THREE LDS stages, LDS-direct buffer loads, counted vmcnt: the slab of
//     step s+2 is issued while step s is multiplied — one workgroup per CU has no neighbour to hide DMA latency);
//   => (41.5 + 9*20) KB per 47 MFLOP instead of 9*(16+20) KB per 23.6 MFLOP: 2.8x fewer L2 bytes per FLOP.
// 8 waves as 4 (pixel rows) x 2 (channels); wave tile = 4 image rows x 16 px x BN/2 channels; v_mfma_f32_16x16x32_bf16
// with the weight fragment as the A operand (4 consecutive output channels per lane, like gemm.hip).
// Image borders and ragged channel tiles are zero-filled by the buffer range check (voffset 0x80000000).
#include "igemm_epi.h"
#include <cstdlib>

namespace SDNS {

namespace {

constexpr int PW = 18;                 // patch width / height in pixels
static_assert(PW == HALO_SIDE + 2, "the patch is the tile of output pixels the plan counts (gemm_tiles.h) plus its halo");
constexpr int PPIX = PW * PW;          // 324
constexpr int NPD = 6;                 // patch DMA instructions per wave: 8 waves * 64 lanes * 6 = 3072 >= 324 * 8 chunks

// Ping-pong schedule: the 8 waves run as two groups of four (one wave of each group per SIMD) staggered by one barrier, so that while
// one group multiplies (s_setprio 1) the other issues its fragment reads and DMAs — the matrix pipe always has a wave feeding it instead
// of all eight loading, then all eight multiplying.  (A lock-step loop and a two-phase ping-pong loop — one k half per phase — were
// measured against this one and removed: DESIGN.md 4.1.)
// One step (tap) is one phase of the merged loop below.  RF: the f32 residual stream's epilogue (GemmArgs::out_f32 == 2: f32 output and
// residual through the narrow tile epilogue, natural weight rows); otherwise 16-bit output through the wide epilogue.
template <int BN, bool RF>
__global__ void __launch_bounds__(512, 2) conv_halo_kernel(const GemmArgs g) {
  constexpr int NT = BN / 32;            // 16-wide channel tiles per wave
  constexpr int MT = 4;                  // image rows per wave
  constexpr int BIT = BN / 64;           // weight row groups per thread (64 rows per DMA instruction of all 8 waves)
  constexpr int B_BYTES = BN * 128;
  constexpr int PBUF = PPIX * 128;       // one patch buffer: 324 px * 128 B = 41472 B (lanes past it are EXEC-masked)
  constexpr int NWS = 3;                 // weight stages
  constexpr int NW = (BN + 63) / 64;     // weight DMA instructions per wave and slab (BN = 160: waves 4-7 pad with a dummy)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // smem: 2 patch buffers, NWS weight stages, then an 8 KiB sink for the padding DMAs (1 KiB per wave)
  constexpr unsigned INVALID = 0x80000000u;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int wave_u = __builtin_amdgcn_readfirstlane(wid);
  const int l15 = lane & 15, lq = lane >> 4;
  const int ks = blockIdx.z;

  // tile order: the channel tiles of one pixel block are adjacent (they share the patch through L2)
  const int tiles_n = (g.N + BN - 1) / BN;
  // nearest-2x upsample fused in front (A_CONV_UP2: the VAE / UNet upsamplers): the conv runs over the OH x OW upsampled image, patch pixel
  // (yy, xx) of it is source pixel (yy >> 1, xx >> 1) — only the DMA source offsets change, the LDS patch holds the upsampled pixels
  const bool up2 = g.amode == A_CONV_UP2;
  const int OH = up2 ? g.Ho : g.H, OW = up2 ? g.Wo : g.W;
  const int bx_n = OW >> 4, by_n = OH >> 4;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  int tn, pb;
  if (g.tn_major) {   // weight-heavy (small images): the XCD's run of tiles keeps one channel tile's weights in its L2
    const int npb = gridDim.x / tiles_n;
    tn = tile / npb; pb = tile - tn * npb;
  } else {
    tn = tile % tiles_n; pb = tile / tiles_n;
  }
  const int tile_m = pb;                 // linear index of the 16 x 16 pixel block: (b * by_n + by) * bx_n + bx
  const int bx = pb % bx_n; pb /= bx_n;
  const int by = pb % by_n;
  const int b = pb / by_n;
  const int y0 = by << 4, x0 = bx << 4, n0 = tn * BN;

  // channel chunks of this K split
  const int CC = g.Cin >> 6;
  const int cc_per = (CC + g.splitk - 1) / g.splitk;
  const int cc_begin = ks * cc_per;
  const int cc_end = min(CC, cc_begin + cc_per);

  const unsigned a_bytes = (unsigned)((int64_t)(g.M / (OH * OW)) * g.H * g.W * g.Cin * 2);
  const unsigned b_bytes = (unsigned)(((int64_t)(g.n_valid - 1) * g.ldb + g.K) * 2);
  const v4i srdA = buf_srd(g.A, a_bytes), srdB = buf_srd(g.Wt, b_bytes);
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem);   // LDS address of smem[0]

  // ---- patch DMA map: linear LDS image [pixel][8 chunks]; lane id -> (pp, position); the swizzle rides on the source chunk
  auto patch_voff = [&](int i) -> unsigned {
    int ln = lane;
    asm volatile("" : "+v"(ln));                       // keeps LICM from hoisting the six offsets back into registers
    const int id = (i * 8 + wid) * 64 + ln;            // 16-byte slot in the patch buffer
    const int pp = id >> 3, pos = id & 7;
    const int c = pos ^ (pp & 7);
    const int py = pp / PW, px = pp - py * PW;
    const int yy = y0 - 1 + py, xx = x0 - 1 + px;
    const bool ok = pp < PPIX && (unsigned)yy < (unsigned)OH && (unsigned)xx < (unsigned)OW;
    const int sy = up2 ? yy >> 1 : yy, sx = up2 ? xx >> 1 : xx;
    return ok ? (unsigned)(((b * g.H + sy) * g.W + sx) * g.Cin + c * 8) * 2u : INVALID;
  };
  // ---- weight DMA map (as gemm.hip): rows r0 + 64 i, chunk swizzled on the source
  const int r0 = tid >> 3;                                // 0..63
  const int cB = (tid & 7) ^ (r0 & 7);
  unsigned b_voff[5];
  // PERM (BN = 160, NT = 5: round 5): LDS row rb of the weight slab holds the weight row its MFMA operand row stands for in the 16-byte epilogue
  // (igemm_epi.h: epi_perm_col — the quads of a tile pair are 8 consecutive output channels per lane, without lane exchanges or registers)
  constexpr bool PERM = (NT & 1) != 0 && !RF;
  auto w_row = [&](int rb) {
    if (!PERM) return n0 + rb;
    const int run = rb / (BN / 2);
    return n0 + run * (BN / 2) + epi_perm_col<NT>(rb - run * (BN / 2));
  };
#pragma unroll
  for (int i = 0; i < BIT; ++i) {
    const int n = w_row(r0 + 64 * i);
    b_voff[i] = (n < g.n_valid) ? (unsigned)(n * g.ldb + cB * 8) * 2u : INVALID;
  }
  constexpr bool B_TAIL = (BN % 64) != 0;                 // BN = 160: a last half group of 32 rows
  unsigned b_voff_tail = INVALID;
  if (B_TAIL) {
    const int n = w_row(BIT * 64 + (r0 & 31));
    if (r0 < 32 && n < g.n_valid) b_voff_tail = (unsigned)(n * g.ldb + cB * 8) * 2u;
  }

  // Padding DMAs (the 6th patch piece on waves 1-7, the slab's 32-row tail on waves 4-7, out-of-range source, into the sink) give every
  // wave the same number of DMAs per slab and patch piece: the counted vmcnt of the main loop relies on it.  The form without them (each
  // wave counting its own issues) was bit-identical and 3-5 % slower on every BN = 160 shape: profiles/r05_halo_nopad_ab.txt.
  constexpr int OFF_B = 2 * PBUF, OFF_DUMMY = OFF_B + NWS * B_BYTES;
  auto dma_patch_piece = [&](int cc, int buf, int i) {      // one of the NPD pieces (i is a compile-time constant after unrolling)
    const unsigned dst = lds0 + buf * PBUF + wave_u * 1024;
    const int soff = cc * 128;
    const unsigned voff = patch_voff(i);
    if (i < NPD - 1) dma16(srdA, voff, soff, dst + i * 8192);
    else {
      const unsigned d5 = (wave_u == 0) ? (dst + (NPD - 1) * 8192) : (lds0 + OFF_DUMMY + wave_u * 1024);
      if (wid != 0 || lane < 32) dma16(srdA, wid == 0 ? voff : INVALID, soff, d5);
    }
  };
  auto dma_weights = [&](int cc, int tap, int stage) {
    const unsigned dst = lds0 + OFF_B + stage * B_BYTES + wave_u * 1024;
    const int soff = (tap * g.Cin + cc * 64) * 2;
#pragma unroll
    for (int i = 0; i < BIT; ++i) dma16(srdB, b_voff[i], soff, dst + i * 8192);
    if (B_TAIL) {
      // rows BIT*64 .. BIT*64+31 ride on waves 0-3 (r0 < 32); waves 4-7 issue the padding DMA
      const unsigned tdst = (wave_u < 4) ? (dst + BIT * 8192) : (lds0 + OFF_DUMMY + wave_u * 1024);
      dma16(srdB, b_voff_tail, soff, tdst);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- main loop: steps s = (cc, tap), weight slab s lives in stage s % 3, the patch alternates per chunk -------------------------
  // A step (tap) is ONE phase: both k halves, 32 (BN = 128) / 40 (BN = 160) MFMAs between two barriers.  The fragments of a step are
  // read in the step's own load segment (one register set): its latency runs beside the OTHER group's MFMA segment, which is what the
  // stagger is for.  The swizzle key of a patch read is (l15 + d) & 7 with d = (18 i + tap offset) & 7 a compile-time constant, so 8 x 2
  // precomputed lane addresses + an immediate serve all 72 reads of a chunk; the weight reads need 2.
  //   group 0:  [L(s)] P [M(s)] P [L(s+1)] ...      group 1 one barrier behind: its L(s) runs beside group 0's M(s).
  //   L(s): read the 2 (MT + NT) fragments of step s (slab s: own pieces retired by the counted vmcnt of L(s - 1), the others'
  //         published by the barriers since); DMA slab s + 2 -> stage (s + 2) % 3 (slab s - 1: its reads were drained — lgkmcnt(0) —
  //         before the barrier that closed L(s - 1) in BOTH groups); patch piece (taps 0-5) of the next chunk; vmcnt(own issues): slab
  //         s + 1 and the previous patch piece have landed; lgkmcnt(0).
  if (cc_begin < cc_end) {
    const int grp = wave_u >> 2;
    auto dma_w_one = [&](int cc, int tap, int stage, int i) {   // instruction i (compile-time after unrolling) of the slab's NW
      const unsigned dst = lds0 + OFF_B + stage * B_BYTES + wave_u * 1024;
      const int soff = (tap * g.Cin + cc * 64) * 2;
      if (i < BIT) dma16(srdB, b_voff[i], soff, dst + i * 8192);
      else dma16(srdB, b_voff_tail, soff, (wave_u < 4) ? (dst + BIT * 8192) : (lds0 + OFF_DUMMY + wave_u * 1024));
    };
    const int km_cfg = min(__builtin_amdgcn_readfirstlane(g.pp_dma_m), NW + 1);
#pragma unroll
    for (int i = 0; i < NPD; ++i) dma_patch_piece(cc_begin, 0, i);
    dma_weights(cc_begin, 0, 0);
    dma_weights(cc_begin, 1, 1);
    wait_vm(NW);                                          // patch and slab 0 have landed; slab 1 may be in flight

    bar();
    if (grp == 1) bar();

    int xaddr[8][2];
#pragma unroll
    for (int d = 0; d < 8; ++d)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        xaddr[d][kk] = (wm * 4 * PW + l15) * 128 + (((kk * 4 + lq) ^ ((l15 + d) & 7)) << 4);
    int waddr[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) waddr[kk] = OFF_B + (wn * (BN / 2) + l15) * 128 + (((kk * 4 + lq) ^ (l15 & 7)) << 4);
    auto rd_x = [&](int tap, int kk, h16x8 (&xf)[MT]) {
      const int toff = (tap / 3) * PW + (tap % 3);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int rel = i * PW + toff;
        xf[i] = *(const h16x8*)(smem + xaddr[rel & 7][kk] + rel * 128);
      }
    };
    auto rd_w = [&](int stage, int kk, h16x8 (&wf)[NT]) {
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[j] = *(const h16x8*)(smem + waddr[kk] + stage * B_BYTES + j * 2048);
    };

    for (int cc = cc_begin; cc < cc_end; ++cc) {
      const int pbuf = (cc - cc_begin) & 1;
      const int hn = (cc + 1 < cc_end) ? 1 : 0;
      if (cc != cc_begin) {                                // this chunk's patch sits in the other buffer
        const int flip = pbuf ? PBUF : -PBUF;
#pragma unroll
        for (int d = 0; d < 8; ++d) { xaddr[d][0] += flip; xaddr[d][1] += flip; }
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const bool more_w = tap < 7 || hn;                    // slab s + 2 exists
        const int wcc = tap < 7 ? cc : cc + 1, wtap = (tap + 2) % 9;
        const bool pp = tap < NPD && hn;
        h16x8 x0[MT], x1[MT], w0[NT], w1[NT];
        rd_x(tap, 0, x0); rd_w(tap % NWS, 0, w0);
        rd_x(tap, 1, x1); rd_w(tap % NWS, 1, w1);
        // km of the step's DMA instructions (the slab's last ones, then the patch piece) ride among the MFMAs instead (round 6, as in
        // gemm_pp.hip): the load segment — 18 fragment reads + 3-4 DMA issues of ~110 cycles each — is longer than the 40-MFMA segment
        // it hides under and every barrier interval lasts max(load, matrix).  Issued later than before (behind this step's barrier) and
        // ahead of the next load segment's issues, whose counted wait therefore covers them: the RAW / WAR argument above is unchanged.
        const int kw = more_w ? (km_cfg < NW ? km_cfg : NW) : 0;          // weight instructions moved
        const bool p_in_m = pp && km_cfg > NW;                             // the patch piece moved
        if (more_w) {
#pragma unroll
          for (int i = 0; i < NW; ++i)
            if (i < NW - kw) dma_w_one(wcc, wtap, (tap + 2) % NWS, i);
        }
        if (pp && !p_in_m) dma_patch_piece(cc + 1, pbuf ^ 1, tap);
        wait_vm((more_w ? NW - kw : 0) + ((pp && !p_in_m) ? 1 : 0));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bar();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              acc[i][j] = hh == 0 ? MFMA_16x16x32(w0[j], x0[i], acc[i][j]) : MFMA_16x16x32(w1[j], x1[i], acc[i][j]);
              const int idx = (hh * MT + i) * NT + j;
#pragma unroll
              for (int o = 0; o <= NW; ++o)
                if (idx == dma_slot_at(o, MT * NT)) {
                  __builtin_amdgcn_sched_barrier(0);
                  if (o < NW) { if (kw > o) dma_w_one(wcc, wtap, (tap + 2) % NWS, NW - 1 - o); }
                  else if (p_in_m) dma_patch_piece(cc + 1, pbuf ^ 1, tap);
                  __builtin_amdgcn_sched_barrier(0);
                }
            }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        bar();
      }
    }
    if (grp == 0) bar();
  }

  // ---- epilogue -----------------------------------------------------------------------------------------------
  const int mr = (b * OH + y0 + wm * 4) * OW + x0 + l15;        // image row i of the wave adds i * OW
  const int nc = n0 + wn * (BN / 2) + lq * 4;
  if (g.splitk > 1) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        // (PERM: the quads of a tile pair are columns 32 (j >> 1) + 8 lq + 4 (j & 1) .. + 3 of the wave's run, the unpaired tile natural)
        const int n = (PERM && j < (NT & ~1)) ? n0 + wn * (BN / 2) + 32 * (j >> 1) + 8 * lq + 4 * (j & 1) : nc + j * 16;
        if (n < g.N) *(f32x4*)(g.slabs + ((int64_t)ks * g.M + mr + i * OW) * g.N + n) = acc[i][j];
      }
  } else if constexpr (RF) {
    epi_tile<MT, NT, false, 0, true>(g, 0, mr, OW, nc, acc, smem, 4, wm, wn, tile_m, n0);
  } else {
    // 16-bit output, no GEGLU: the wide epilogue — at BN = 128 through lane exchanges; at BN = 160 (NT = 5, the kernel sits at 254 VGPRs, the
    // exchange form spills 38 registers) through the permuted weight rows above (round 5)
    epi_tile<MT, NT, false, (NT % 2 == 0) ? 1 : 2>(g, 0, mr, OW, nc, acc, smem, 4, wm, wn, tile_m, n0);
  }
}

template <int BN, bool RF>
void launch_halo(const GemmArgs& g, dim3 grid, hipStream_t s) {
  constexpr int smem = 2 * PPIX * 128 + 3 * BN * 128 + 8192;
  hipLaunchKernelGGL((conv_halo_kernel<BN, RF>), grid, dim3(512), smem, s, g);
}

constexpr int HALO_DMA_M = 4;          // DMA instructions of a step issued among its MFMAs (the kernel reads GemmArgs::pp_dma_m at run time)

}  // namespace

void conv_halo_init_device() {
  HIP_OK(hipFuncSetAttribute((const void*)conv_halo_kernel<128, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * PPIX * 128 + 3 * 128 * 128 + 8192));
  HIP_OK(hipFuncSetAttribute((const void*)conv_halo_kernel<160, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * PPIX * 128 + 3 * 160 * 128 + 8192));
  HIP_OK(hipFuncSetAttribute((const void*)conv_halo_kernel<128, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * PPIX * 128 + 3 * 128 * 128 + 8192));
  HIP_OK(hipFuncSetAttribute((const void*)conv_halo_kernel<160, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * PPIX * 128 + 3 * 160 * 128 + 8192));
}

// bn: the channel-tile width of the plan (gemm_plan.cpp), 128 or 160
void launch_conv_halo(const GemmArgs& g, int bn, dim3 grid, hipStream_t s) {
  GemmArgs gm = g;
  gm.pp_dma_m = HALO_DMA_M;
  const bool rf = g.out_f32 == 2;        // f32 residual stream
  if (bn == 160) { if (rf) launch_halo<160, true>(gm, grid, s); else launch_halo<160, false>(gm, grid, s); }
  else           { if (rf) launch_halo<128, true>(gm, grid, s); else launch_halo<128, false>(gm, grid, s); }
}

}  // namespace SDNS
