// BASELINE configs[2], round 5 (second session): the PERSISTENT form of the wide LDS-DMA bf16 implicit-GEMM convolution (conv16.hip; 256 x 128 / 128 x 256 tiles).
// One block per CU walks a sequence of output tiles; four PRODUCER waves do nothing but issue the LDS-DMA fetches of a three-stage ring that runs on across tile
// boundaries (and own the index arithmetic of the A rows); the eight multiplying waves read fragments, issue MFMAs and write the tile out (the protocol:
// conv16_common.h c16_ring_produce / c16_ring_consume, shared with wgrad16.hip).
// Why (profiles/r05_decoder3x3_ta_tcp_sq_counters.txt): with one 144 KB block per CU nothing hides a tile's prologue -- every block asks for its first 96 KB at the
// same moment and waits ~9 k clocks for them, 18 % of the kernel on the decoder's 3x3 -- and a 1 KB fetch instruction holds its wave's issue for 60-185 clocks beside
// the MFMAs of the same wave. Here the first stages of tile i + 1 are in flight while tile i is multiplied and written out, and a stalled fetch blocks nobody else.
// Same operands, addressing, tap skipping and epilogue arithmetic as the tile kernel of conv16.hip (the same functions); split-K slabs and fp32 outputs included.
// Replaces nn.Conv2d forward / input gradient of deepv3plus.py:72-81,419-425 (ASPP, dsn, decoder) on the bf16 tier where the planner picks it.
#include <stdlib.h>
#include <algorithm>

#include "conv16_common.h"

namespace {

constexpr int BKB = C16_BKB;

template <int BM, int BN, int WM, int WN, int NP>
__global__ __launch_bounds__((8 + NP) * 64, (8 + NP) / 4) void conv16p_kernel(const pm_conv16 a) {
  static_assert(WM * WN == 8, "eight multiplying waves");
  constexpr int FT = NP * 64;                                // fetching threads
  typedef c16_a_rows<FT, BM> ARows;
  typedef c16_frags<BM, BN, WM, WN> Frags;
  constexpr int A_IT = ARows::IT, B_IT = BN * 8 / FT;        // 16-byte fetches per producer lane and K-step
  constexpr int FETCH = A_IT + B_IT;
  constexpr int A_BYTES = BM * BKB, STAGE = (BM + BN) * BKB;
  constexpr int TM = Frags::TM, TN = Frags::TN;
  constexpr int LDS_SUB = 36;                                // floats per row of a 32 x 32 epilogue slab
  static_assert(8 * 32 * LDS_SUB * 4 <= STAGE, "the epilogue slabs of the eight waves live in one ring slot");
  extern __shared__ __align__(16) char lds[];

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int ntiles = a.tiles_m * a.tiles_n, total = ntiles * a.ksplit, G = gridDim.x;
  const bool pointwise = c16_pointwise(a);
  auto open = [&](int v) {      // unit v -> its tile, K range and step count: the ONE place producers and consumers learn how many barriers the unit takes
    const int z = v / ntiles;
    return c16_open_unit<BM, BN>(a, pointwise, v - z * ntiles, z);
  };

  if (wave >= 8) {
    // ================================================== producer waves ==================================================
    const int wave_u = wave - 8, t = wave_u * 64 + lane;
    const long pitchb = a.a_pitch * 2;
    const __amdgpu_buffer_rsrc_t rA =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<pm_bf16*>(a.A), 0, (int)((long)a.N * a.H * a.W * pitchb), 0x00020000);
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<pm_bf16*>(a.B), 0, (int)((long)a.Nn * a.K * 2), 0x00020000);
    ARows ar;
    int cur[A_IT], boff[B_IT];
    c16_kstate ks;
    bool fresh = true;
    auto load = [&](const c16_unit& u) {
      ar.stepped(a, pointwise, pitchb, u.m0, t);
      c16_b_rows<FT, BN>(a, u.n0, t, boff);
      ks.open(a, u);
      fresh = true;
    };
    auto fetch = [&](char* la) {
      char* lb = la + A_BYTES;
      if (fresh) {      // border test and pixel offset of the tap: once per tap; the 64-channel chunk rides in the scalar offset of the fetch
        const int dy = ks.ky * a.dil, dx = ks.kx * a.dil;
        const int toff = (dy * a.W + dx) * (int)pitchb;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) cur[it] = ar.at(a, it, dy, dx, toff);
      }
      const int s_cb = ks.ch * BKB;
#pragma unroll
      for (int it = 0; it < A_IT; ++it) dma16(rA, la + (it * FT + wave_u * 64) * 16, cur[it], s_cb);
#pragma unroll
      for (int it = 0; it < B_IT; ++it) dma16(rB, lb + (it * FT + wave_u * 64) * 16, boff[it], ks.kb);
      fresh = ks.advance();
    };
    c16_ring_produce<FETCH, STAGE>(lds, blockIdx.x, total, G, open, load, fetch);
    return;
  }

  // ================================================== multiplying waves ==================================================
  const int wm = wave / WN, wn = wave % WN;
  Frags fr;
  fr.init(wm, wn, lane);
  f32x16 acc[TM][TN];
  c16_ring_consume<STAGE>(
      lds, blockIdx.x, total, G, open, [&](const c16_unit&) { c16_zero(acc); }, [&](const char* ls) { fr.step(ls, acc); },
      [&](const c16_unit& u, char* slot) {
        // ---- epilogue: 32 x 32 slabs of the wave's tile through the ring slot read last ----
        float* Ws = reinterpret_cast<float*>(slot) + wave * 32 * LDS_SUB;
        const int row0 = u.m0 + wm * (BM / WM);
        const int col0 = u.n0 + wn * (BN / WN);
        const bool slab = a.ksplit > 1;
        if (a.c_f32 || slab)      // fp32 rows: split-K slabs (no epilogue arithmetic) or class logits (bias only)
          c16_store_f32<TM, TN, 32, true>(Ws, acc, lane, row0, col0, reinterpret_cast<float*>(a.C) + (slab ? (long)u.z * a.c_split : 0), slab ? a.Nn : a.c_pitch, a.M,
                                          a.Nn, a.bias, slab);
        else c16_store_bf16<TM, TN, 32, true, false>(Ws, acc, lane, row0, col0, a);
      });
}

template <int BM, int BN, int WM, int WN, int NP>
void launch_persistent(const pm_conv16& k, hipStream_t st) {
  constexpr size_t smem = (size_t)3 * (BM + BN) * BKB;
  static_assert(smem <= 160 * 1024, "LDS budget");
  static pm_lds_optin optin;
  const int ncu = optin(reinterpret_cast<const void*>(&conv16p_kernel<BM, BN, WM, WN, NP>), 160 * 1024);
  const int total = k.tiles_m * k.tiles_n * k.ksplit;
  hipLaunchKernelGGL((conv16p_kernel<BM, BN, WM, WN, NP>), dim3(std::min(total, ncu)), dim3((8 + NP) * 64), smem, st, k);
}

}  // namespace

// 1 when pm_conv16_launch runs this plan in the persistent producer / consumer form (the ring tiles with pm_routing.conv16_persistent), 0 for one block per tile
int pm_conv16w_persistent(const pm_conv16* k) { return pm_route.conv16_persistent && k->wide && ((k->bm == 256 && k->bn == 128) || (k->bm == 128 && k->bn == 256)) ? 1 : 0; }

// the persistent plans only (pm_conv16w_persistent); pm_conv16_launch runs every other one
int pm_conv16w_launch(const pm_conv16* k, hipStream_t st) {
  if (k->bm == 256 && k->bn == 128) launch_persistent<256, 128, 4, 2, 4>(*k, st);
  else if (k->bm == 128 && k->bn == 256) launch_persistent<128, 256, 2, 4, 4>(*k, st);
  else {
    pm_set_error("conv16w: no persistent %d x %d tile", k->bm, k->bn);
    return PM_EUNSUPPORTED;
  }
  return pm_check_launch("conv16w");
}
