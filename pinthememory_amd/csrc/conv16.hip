// BASELINE configs[2], round 4: the bf16 implicit-GEMM convolution built around LDS-DMA (the core of tools/micro/bf16_glds_lab.hip moved into the library and
// given the convolution gather). Forward and stride-1 data gradient (= forward convolution of dy with the rotated filter) of nn.Conv2d on bf16 activations:
//   C[M][N] = sum_k A[m][k] B[n][k],  M = output pixels, N = output channels, k = (tap, channel), channels padded to a multiple of 64 per tap
//   A = bf16 NHWC activations gathered per (row, tap): one K-step = one tap x 64 channels = 128 bytes of one pixel row
//   B = bf16 weights [N][taps][Cp] (pm_bf16_cast_weights), k-contiguous
// Staging: LDS-DMA (buffer_load_dwordx4 ... lds), 16 bytes per lane, straight from global memory into LDS -- no staging registers, no ds_write pass. The LDS image
// is lane-linear (row = 8 lanes x 16 B), so the XOR swizzle that makes the ds_read_b128 fragment reads conflict-free is applied on the SOURCE chunk a lane fetches
// (and again on the read). Both operands are addressed through buffer descriptors with 32-bit per-lane offsets: padding taps, rows beyond M and columns beyond N
// present an out-of-range offset and the fetch delivers zeros (the first form of the kernel used global_load_lds with 64-bit pointers and a zero page: 2.4 x the
// vector instructions per K-step, 566 vs 684 TF on the ASPP 3x3).
// ONE kernel template, one block per (output tile, K-split), in two families (the pieces it is made of live in conv16_common.h, shared with the persistent form of
// conv16w.hip and with wgrad16.hip):
//   * NARROW, 256 threads = 4 waves x (BM / WM) x (BN / WN) of v_mfma_f32_32x32x16_bf16 tiles, 64 / 128-row and -column tiles, __syncthreads between the K-steps; NST LDS
//     stages (2: the loads of K-step k + 1 fly under the MFMAs of step k; 1 for the single-step reductions of the 64-channel 1x1 convolutions, where four blocks
//     share a CU instead of two);
//   * WIDE (round 5), 512 threads = eight waves, ONE large output tile per CU:
//       256 x 256, two 64 KB LDS stages (128 FLOP per staged byte; wave tile 128 x 64: 0.75 KB of LDS reads per MFMA): the fetches of K-step k + 1 are issued behind the
//       barrier of step k and fly under its 32 MFMAs per wave. THE FORM THE PLANNER USES: the deep reductions (ASPP 3x3 2048 -> 256 on the 48 x 48 maps: 690 TF on the
//       64 x 128 tiles, 764 with skipped filter rows, 834-866 here; the auxiliary head's 3x3 1024 -> 512: 660 -> 780) and very wide outputs of a medium reduction
//       (256 -> 2048: 697 -> 780);
//       256 x 128 / 128 x 256, a three-stage LDS ring filled with COUNTED waits (s_waitcnt vmcnt(N) + a bare s_barrier: the fetches of K-steps k + 1 and k + 2 stay in
//       flight while step k is multiplied; 85 FLOP per staged byte): 733-769 TF on the same shapes, level with the narrow tiles elsewhere -- kept for one-block-per-tile
//       runs (pm_set_conv16(8)) and the tests; the planner's ring plans run in the persistent form (conv16w.hip).
//     Why big tiles: every kernel of this family moves ~20-30 bytes per clock and CU from L2 into LDS whatever its tile (DESIGN section 7 "Round 5"), so TFLOP/s ~ FLOP
//     per staged byte x that; the 64 x 128 / 128 x 128 tiles stage 43 / 64. Why not everywhere: with one block per CU the tile count has to be balanced against the
//     256 CUs (split-K by the planner's cost model, pm_conv16_plan); the 48 x 48 maps give 72 x N / 256 tiles of 256 x 256.
// Epilogue staged through LDS: whole 16-byte row segments of eight bf16 (round to nearest even) with the fused bias / folded BatchNorm / residual / ReLU, or
// fp32 rows for the class logits and the split-K slabs.
// Replaces nn.Conv2d forward / input gradient of Resnet.py:145-150,195,453-457; deepv3plus.py:72-81,398-424; memory.py:75,104 on the bf16 tier.
#include <stdlib.h>
#include <algorithm>

#include "conv16_common.h"

namespace {

constexpr int BKB = C16_BKB;

// NT threads = NT / 64 waves as WM x WN. COUNTED: the wide family's main loop (counted vmcnt waits + bare barriers) instead of __syncthreads.
template <int NT, int BM, int BN, int WM, int WN, int NST, bool COUNTED, bool STATS>
__global__ __launch_bounds__(NT, 2) void conv16_kernel(const pm_conv16 a) {
  static_assert(WM * WN * 64 == NT, "one wave per wave tile");
  typedef c16_a_rows<NT, BM> ARows;      // 16-byte fetches per lane and K-step: a sweep of the block covers NT / 8 rows x 8 chunks
  typedef c16_frags<BM, BN, WM, WN> Frags;
  constexpr int A_IT = ARows::IT, B_IT = BN * 8 / NT;
  constexpr int FETCH = A_IT + B_IT;                         // LDS-DMA instructions one wave issues per stage
  constexpr int A_BYTES = BM * BKB, STAGE = (BM + BN) * BKB;
  constexpr int TM = Frags::TM, TN = Frags::TN;
  static_assert(A_IT >= 1 && B_IT >= 1, "bad tile config");
  extern __shared__ __align__(16) char lds[];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const bool pointwise = c16_pointwise(a);      // block-uniform
  const c16_unit u = c16_open_unit<BM, BN>(a, pointwise, blockIdx.x, blockIdx.z);      // this block's tile and its K-steps
  const long pitchb = a.a_pitch * 2;

  const __amdgpu_buffer_rsrc_t rA =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<pm_bf16*>(a.A), 0, (int)((long)a.N * a.H * a.W * pitchb), 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<pm_bf16*>(a.B), 0, (int)((long)a.Nn * a.K * 2), 0x00020000);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // wave-uniform by construction: the LDS destination of a fetch lives on the scalar unit
  ARows ar;
  ar.direct(a, pointwise, pitchb, u.m0, t);
  int boff[B_IT];
  c16_b_rows<NT, BN>(a, u.n0, t, boff);
  c16_kstate ks;
  ks.open(a, u);

  auto stage = [&](int buf) {
    char* la = lds + buf * STAGE;
    char* lb = la + A_BYTES;
    const int dy = ks.ky * a.dil, dx = ks.kx * a.dil;
    const int toff = (dy * a.W + dx) * (int)pitchb + ks.ch * BKB;
#pragma unroll
    for (int it = 0; it < A_IT; ++it) dma16(rA, la + (it * NT + wave_u * 64) * 16, ar.at(a, it, dy, dx, toff), 0);
#pragma unroll
    for (int it = 0; it < B_IT; ++it) dma16(rB, lb + (it * NT + wave_u * 64) * 16, boff[it], ks.kb);
    ks.advance();
  };

  f32x16 acc[TM][TN];
  c16_zero(acc);
  Frags fr;
  fr.init(wm, wn, lane);
  auto compute = [&](int buf) { fr.step(lds + buf * STAGE, acc); };

  const int nk_eff = u.steps;
  if (nk_eff > 0) {
    if constexpr (!COUNTED) {
      stage(0);
      __syncthreads();
      if constexpr (NST == 1) {
        for (int kt = 0; kt < nk_eff; ++kt) {
          compute(0);
          if (kt + 1 < nk_eff) {
            __syncthreads();      // every wave is done reading the single buffer
            stage(0);
            __syncthreads();
          }
        }
      } else {
        for (int kt = 0; kt < nk_eff; ++kt) {
          if (kt + 1 < nk_eff) stage((kt + 1) & 1);
          compute(kt & 1);
          __syncthreads();
        }
      }
    } else if constexpr (NST == 3) {
      // the ring: stage k + 2 is issued behind the barrier of step k (its buffer was last read in step k - 1, which every wave has left); the wait in front of the
      // barrier leaves the FETCH instructions of stage k + 1 in flight (LDS-DMA fetches of a wave retire in order), so "my part of stage k has landed" + barrier =
      // "stage k has landed".
      stage(0);
      if (nk_eff > 1) stage(1);
      int cur = 0, nxt = 2;
      for (int kt = 0; kt < nk_eff; ++kt) {
        if (kt + 1 < nk_eff) wait_vm<FETCH>();
        else wait_vm<0>();
        ring_barrier();
        if (kt + 2 < nk_eff) stage(nxt);
        compute(cur);
        cur = cur == NST - 1 ? 0 : cur + 1;
        nxt = nxt == NST - 1 ? 0 : nxt + 1;
      }
    } else {
      // 256 x 256 (64 KB per stage): the fetches of K-step k + 1 are issued behind the barrier of step k and fly under its 32 MFMAs per wave; the wait in front of
      // the next barrier is a full one (nothing younger is in flight).
      stage(0);
      for (int kt = 0; kt < nk_eff; ++kt) {
        wait_vm<0>();
        ring_barrier();      // stage kt has landed everywhere, and everybody has left the buffer stage kt + 1 goes into (read in step kt - 1)
        if (kt + 1 < nk_eff) stage((kt + 1) & 1);
        compute(kt & 1);
      }
    }
  }

  // ---- epilogue: a wave parks 32 rows of its tile in LDS (the stages are dead) and stores whole row segments ----------------------------------------
  constexpr int WC = BN / WN;
  if constexpr (!COUNTED) __syncthreads();
  else {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  float* Ws = reinterpret_cast<float*>(lds) + wave * 32 * (WC + 4);
  const int row0 = u.m0 + wm * (BM / WM);
  const int col0 = u.n0 + wn * WC;
  const bool slab = a.ksplit > 1;
  if (a.c_f32 || slab)
    c16_store_f32<TM, TN, WC, false>(Ws, acc, lane, row0, col0, reinterpret_cast<float*>(a.C) + (slab ? (long)u.z * a.c_split : 0), slab ? a.Nn : a.c_pitch, a.M, a.Nn,
                                     a.bias, slab);
  else c16_store_bf16<TM, TN, WC, false, STATS>(Ws, acc, lane, row0, col0, a);
}

template <int NT, int BM, int BN, int WM, int WN, int NST, bool COUNTED, bool STATS>
void launch_tile_s(const pm_conv16& k, hipStream_t st) {
  constexpr size_t stage_bytes = (size_t)NST * (BM + BN) * BKB, ep_bytes = (size_t)(NT / 64) * 32 * (BN / WN + 4) * sizeof(float);
  constexpr size_t smem = stage_bytes > ep_bytes ? stage_bytes : ep_bytes;
  static_assert(smem <= 160 * 1024, "LDS budget");
  static pm_lds_optin optin;
  (void)optin(reinterpret_cast<const void*>(&conv16_kernel<NT, BM, BN, WM, WN, NST, COUNTED, STATS>), 160 * 1024);
  hipLaunchKernelGGL((conv16_kernel<NT, BM, BN, WM, WN, NST, COUNTED, STATS>), dim3(k.tiles_m * k.tiles_n, 1, k.ksplit), dim3(NT), smem, st, k);
}
template <int BM, int BN>
void launch_narrow(const pm_conv16& k, hipStream_t st) {
  const bool one = k.ksteps_per == 1;      // a single K-step per block: one LDS stage, four blocks per CU
  const bool stats = k.stats && k.ksplit == 1 && !k.c_f32;
  if (one) stats ? launch_tile_s<256, BM, BN, 2, 2, 1, false, true>(k, st) : launch_tile_s<256, BM, BN, 2, 2, 1, false, false>(k, st);
  else stats ? launch_tile_s<256, BM, BN, 2, 2, 2, false, true>(k, st) : launch_tile_s<256, BM, BN, 2, 2, 2, false, false>(k, st);
}

}  // namespace

// Tile / split choice. Rows in tiles of 128 (64 when that fills the 256 CUs better on the 48 x 48 maps), columns in tiles of 128 (64 for <= 64 output
// channels); split-K (fp32 slabs, fixed-order reduce by the caller) only where the output tiles alone leave most CUs idle AND the reduction is long.
// Round 5: the WIDE forms (above and conv16w.hip: 256 x 128 / 128 x 256 tile, eight waves, ONE block per CU, three-stage ring) where a cost model of whole rounds of the 256 CUs
// says it wins: its K-step costs ~1.45 x a 64 x 128 step of the narrow kernel for 4 x the tile, but a partly filled last round costs a whole round, so the model picks
// the K-split that balances the tiles against the CUs. PM_C16W: 0 never, 1 by the model (default), 2 wherever the shape allows it (A/B runs, kernel tests).
namespace {
struct WidePick {
  bool ok;
  int bm, bn, ks;
  double cost;      // in units of one wide K-step on a full chip
};
WidePick wide_pick(const pm_conv16* k, int only_cfg = -1) {
  constexpr double OVH = 10.0;      // prologue + epilogue of a block, in K-steps
  WidePick best{false, 0, 0, 0, 1e30};
  const bool forced = pm_route.conv16_wide >= 2;      // kernel tests: every shape the kernel can express, ragged rows / columns and single K-steps included
  if (!forced && (k->Nn < 128 || k->M < 2048 || k->ksteps < 4)) return best;
  // cfg 0: 256 x 128, 1: 128 x 256, 2: 256 x 256 (two LDS stages)
  const int force_cfg = only_cfg >= 0 ? only_cfg : (pm_route.conv16_wide == 3 ? 2 : -1);            // pm_set_conv16(7): the 256 x 256 tile on every shape (kernel tests)
  for (int cfg = 0; cfg < 3; ++cfg) {
    if (force_cfg >= 0 && cfg != force_cfg) continue;
    const int bm = cfg == 1 ? 128 : 256, bn = cfg == 0 ? 128 : 256;
    if (cfg == 2 && force_cfg != 2) continue;      // 256 x 256 only where asked for (the planner's rule below, pm_set_conv16(7))
    const long tiles = (long)pm_cdiv(k->M, bm) * pm_cdiv(k->Nn, bn);
    const double fill = ((double)k->M * k->Nn) / ((double)tiles * bm * bn);      // padded rows / columns are wasted work
    for (int ks = 1; ks <= 16; ++ks) {
      if (ks > 1 && k->ksteps / ks < (forced ? 2 : 8)) break;
      const int per = pm_cdiv(k->ksteps, ks);
      const int kse = pm_cdiv(k->ksteps, per);
      const long blocks = tiles * kse;
      const long rounds = (blocks + 255) / 256;
      // split-K slabs: fp32 partial tiles written and read back by the reduce (bytes / ~4 TB/s, in wide K-steps of ~1.1 us measured on this kernel)
      const double slab = kse > 1 ? (double)kse * k->M * k->Nn * 8.0 / 4e12 / 1.1e-6 : 0.0;
      // a 256 x 256 step covers twice the area of a 256 x 128 one at ~1.3 x its rate (128 vs 85 FLOP per staged byte)
      const double cost = (double)rounds * (per + OVH) / fill * (cfg == 1 ? 1.03 : (cfg == 2 ? 1.5 : 1.0)) + slab;
      if (cost < best.cost) best = WidePick{true, bm, bn, kse, cost};
    }
  }
  return best;
}
}  // namespace
void pm_conv16_plan(pm_conv16* k) {
  k->wide = 0;
  k->bn = k->Nn > 64 ? 128 : 64;
  k->tiles_n = pm_cdiv(k->Nn, k->bn);
  const long t128 = (long)pm_cdiv(k->M, 128) * k->tiles_n, t64 = (long)pm_cdiv(k->M, 64) * k->tiles_n;
  // rounds of the 256 CUs x 2 resident blocks: take 64-row tiles when 128-row tiles would leave the last round under half full or not fill the chip once
  auto waste = [](long tiles) { const long r = (tiles + 511) / 512; return (double)(r * 512) / (double)tiles; };
  k->bm = (t128 < 512 || waste(t128) > 1.25 * waste(t64)) ? 64 : 128;
  k->tiles_m = pm_cdiv(k->M, k->bm);
  const long tiles = (long)k->tiles_m * k->tiles_n;
  int ks = 1;
  if (tiles < 256 && k->ksteps >= 16) ks = (int)std::min<long>(std::min<long>(8, k->ksteps / 8), (512 + tiles - 1) / tiles);
  k->ksteps_per = pm_cdiv(k->ksteps, ks);
  k->ksplit = pm_cdiv(k->ksteps, k->ksteps_per);
  k->c_split = (long)k->M * k->Nn;
  // Round 5, measured and left out: a 64 x 256 "full-N" tile for the HBM-bound 1x1 convolutions with a short reduction and a
  // wide output (64 -> 256 on the 192 x 192 maps, 128 -> 512 on 96 x 96, 256 -> 1024 on 48 x 48), so that the activation rows are fetched once per 256 output channels.
  // tools/conv16_probe.py, same box, alternated: 64 -> 256 253-260 -> 243-252 TF, 128 -> 512 288-297 -> 259-260, 256 -> 1024 360-369 -> 343-347: the second fetch of
  // the rows comes from L2 and was never the bound -- standalone the 64 -> 256 launch already moves its 189 MB in 37 us (5.1 TB/s: the output write), and the wider
  // tile only takes resident blocks away (80 KB of LDS stages per block instead of 48). The in-step figure of that shape (60 us) is not a tiling problem.
  if (pm_route.conv16_wide > 0) {
    // Where the wide tiles win (tools/conv16_probe.py on an MI355X, round 5, profiles/r05_conv16w_probe.txt), all with the 256 x 256 two-stage form (128 FLOP per staged
    // byte, full-N for the 256-channel outputs): the DEEP reductions -- the ASPP 3x3 2048 -> 256 on the 48 x 48 maps (288 K-steps: 690 TF narrow, 764 with skipped filter
    // rows, 733 on 256 x 128, **834-866**), the auxiliary head's 3x3 1024 -> 512 (660 -> 780) -- and the very wide outputs of a medium reduction (3x3 256 -> 2048
    // data-gradient form: 697 narrow, 725-769 on 256 x 128, **778-785**). Not the 72-K-step 3x3 512 -> 512 of layer4 (633 vs 650-700 narrow: 144 tiles), and on the
    // 192 x 192 maps every form sits at 915-958 TF (the decoder's 3x3s stay with the 128 x 128 register-staged kernel).
    const bool wins = k->ksteps >= 128 || (k->Nn >= 2048 && k->ksteps >= 32);
    // Second session: the PERSISTENT ring form (conv16w.hip conv16p_kernel: producer waves fetch ahead across tile boundaries). Same box, default routing -> persistent
    // (profiles/r05_conv16p_probe.txt): decoder 3x3 320 -> 256 @192 0.490 -> 0.423-0.438 ms (1030 TF), 256 -> 256 0.380 -> 0.348-0.355; ASPP 3x3 2048 -> 256 (256 x 256
    // form) 0.205 -> 0.191; its data-gradient form 256 -> 2048 0.225 -> 0.205. Not the 1024 -> 512 3x3 of the auxiliary head (0.222 on 256 x 256 vs 0.229-0.241), the
    // 72-K-step 3x3 512 -> 512 (0.126 narrow vs 0.138-0.145) or the short 1x1 reductions (the epilogue of a tile is not overlapped with anything).
    const bool ring_wins = pm_route.conv16_persistent && ((k->M >= 200000 && k->ksteps >= 32 && k->Nn >= 256) || (k->ksteps >= 128 && k->Nn <= 256) || (k->Nn >= 2048 && k->ksteps >= 32));
    const WidePick w = pm_route.conv16_wide >= 2 ? wide_pick(k) : (ring_wins ? wide_pick(k) : (wins ? wide_pick(k, 2) : WidePick{false, 0, 0, 0, 0}));
    if (w.ok) {
      k->wide = 1, k->bm = w.bm, k->bn = w.bn;
      k->tiles_m = pm_cdiv(k->M, k->bm), k->tiles_n = pm_cdiv(k->Nn, k->bn);
      k->ksteps_per = pm_cdiv(k->ksteps, w.ks);
      k->ksplit = pm_cdiv(k->ksteps, k->ksteps_per);
    }
  }
}
// Fraction of the K-steps the launch really runs: 1 minus the chunks of filter rows no row of a tile can see (the kernels' own rule, c16_visible_rows / c16_ksteps,
// evaluated per row tile on the host). The in-library profile records EXECUTED FLOPs with it, so that a roofline fraction never counts multiplications that were
// skipped (round 5).
double pm_conv16_executed_fraction(const pm_conv16* k) {
  const bool pointwise = c16_pointwise(*k);
  if (pointwise || k->kh <= 1) return 1.0;
  double run = 0.0;
  for (int tm = 0; tm < k->tiles_m; ++tm) {
    unsigned ky_ok;
    c16_visible_rows(*k, pointwise, tm * k->bm, k->bm, ky_ok);
    run += (double)c16_ksteps(*k, ky_ok, 0, k->ksteps) / k->ksteps;
  }
  return k->tiles_m > 0 ? run / k->tiles_m : 1.0;
}

size_t pm_conv16_slab_bytes(const pm_conv16* k) { return k->ksplit > 1 ? pm_align_up((size_t)k->ksplit * k->M * k->Nn * sizeof(float), 256) : 0; }

int pm_conv16_launch(const pm_conv16* k0, hipStream_t st) {
  pm_conv16 k = *k0;
  if (k.wide) {
    PM_REQUIRE(!k.stats, PM_EUNSUPPORTED, "conv16: the wide forms have no statistics epilogue (pm_conv_bn_partials_bytes answers 0 for this plan)");
    if (pm_conv16w_persistent(&k)) return pm_conv16w_launch(&k, st);
    if (k.bm == 256 && k.bn == 128) launch_tile_s<512, 256, 128, 4, 2, 3, true, false>(k, st);
    else if (k.bm == 128 && k.bn == 256) launch_tile_s<512, 128, 256, 2, 4, 3, true, false>(k, st);
    else if (k.bm == 256 && k.bn == 256) launch_tile_s<512, 256, 256, 2, 4, 2, true, false>(k, st);
    else {
      pm_set_error("conv16: no wide %d x %d tile", k.bm, k.bn);
      return PM_EUNSUPPORTED;
    }
    return pm_check_launch("conv16 (wide tile)");
  }
  if (k.bm == 128 && k.bn == 128) launch_narrow<128, 128>(k, st);
  else if (k.bm == 64 && k.bn == 128) launch_narrow<64, 128>(k, st);
  else if (k.bm == 128 && k.bn == 64) launch_narrow<128, 64>(k, st);
  else if (k.bm == 64 && k.bn == 64) launch_narrow<64, 64>(k, st);
  else {
    pm_set_error("conv16: no %d x %d tile", k.bm, k.bn);
    return PM_EUNSUPPORTED;
  }
  return pm_check_launch("conv16");
}
