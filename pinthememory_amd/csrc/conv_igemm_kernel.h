// The implicit-GEMM convolution kernel template of conv_igemm.hip, in a header so that the split-operand instantiations (PREC 5, conv_split.hip) compile as
// their own translation unit beside the fp32 / bf16 ones. See conv_igemm.hip for the description of the modes. The kernel parameter block ConvK and the pieces the
// kernel is put together from (tile map, LDS layouts, epilogues) are in conv_igemm_parts.h; here are the gather, the K-group multiply and the three main-loop schedules.
#pragma once
#include "conv_igemm_parts.h"

// conv_split.hip: launches the PREC 5 instantiation of the tile (bm x bn) / K-state mode of `k`, on one LDS stage of smem bytes
int pm_conv_split_launch(int mode, int bm, int bn, const ConvK& k, unsigned gx, unsigned gy, unsigned gz, size_t smem, hipStream_t st);
size_t pm_conv_split_stage_bytes(int mode, int bm, int bn);

namespace {

// One pixel-window gather, for the A rows of the forward pass (SG = +1: input pixel = window origin + tap displacement) and of the stride-1 data gradient (SG = -1: dy
// pixel = dx pixel + pad - tap displacement): row i reads base[i] + SG * toff where its pixel (y0[i] + SG * dy, x0[i] + SG * dx) lies inside the hh x ww grid and the
// tap exists, zeros elsewhere. Branch-free: every lane always issues its loads, invalid ones at offset OOB.
template <int SG, int N>
__device__ __forceinline__ void igemm_gather_window(__amdgpu_buffer_rsrc_t rs, const int* base, const int* y0, const int* x0, int dy, int dx, int toff, bool tok, int hh, int ww,
                                                    v4f* out) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool ok = ((unsigned)(y0[i] + SG * dy) < (unsigned)hh) & ((unsigned)(x0[i] + SG * dx) < (unsigned)ww) & tok;
    const int off = base[i] + SG * toff;
    out[i] = bload(rs, ok ? off : OOB);
  }
}

// KM selects how the running K-state of the gather advances by one K-step:
//   K_FAST  the channel extent is a multiple of BK (and stride 1 for dgrad): a K-slab never straddles a tap, so
//           (tap, channel) are wave-uniform -> they live in SGPRs and the per-row work is add / compare / select;
//   K_MID   channel extent (or Wo for wgrad) >= BK: at most one wrap per step, per-lane state, compare + select;
//   K_SMALL extent < BK (stem Cin = 4, Cout = 19, tiny test images): per-lane state, looping wrap.
//   K_PW    (round 6, the split path's instantiations) K_FAST on a pointwise problem -- 1x1 / stride 1 / no padding, and every Winograd point product: a row's validity does
//           not depend on the K-step, so it is folded into the row's base offset once and a gather costs ONE add per row (K_FAST: two compares, two adds, a select).
enum { K_FAST = 0, K_MID = 1, K_SMALL = 2, K_PW = 3 };

// ---- gather state, one struct per operand role: init() once per block, load() per K-step (branch-free: every lane always issues its loads, invalid ones at offset
// OOB), advance() per K-step. g = t & 7, r = t >> 3 come from the kernel. xp4 / yp4: bytes between pixels of the convolution's input / output tensor.

// The (tap, channel) decomposition of the running k of a forward pass / data gradient: wave-uniform (K_FAST / K_PW: SGPRs) or per lane (K_MID / K_SMALL: the k-group
// g of this thread). Both operands' gathers read it.
template <int MODE, int KM>
struct IgemmKState {
  static constexpr bool FAST = KM == K_FAST || KM == K_PW;
  int ch = 0, tap = 0, ky = 0, kx = 0;
  __device__ __forceinline__ void init(const ConvK& a, int k_begin, int g) {
    const int cdim = (MODE == MODE_FWD) ? a.Cin : a.Cout;
    if constexpr (FAST) {
      tap = __builtin_amdgcn_readfirstlane(k_begin / cdim);
      ch = k_begin - tap * cdim;
      ky = tap / a.kw;
      kx = tap - ky * a.kw;
    } else {
      const int k = k_begin + g * 4;
      tap = k / cdim;
      ch = k - tap * cdim;
      ky = tap / a.tk_w;
      kx = tap - ky * a.tk_w;
    }
  }
  __device__ __forceinline__ void advance(const ConvK& a) {
    const int cdim = (MODE == MODE_FWD) ? a.Cin : a.Cout;
    ch += BK;
    if constexpr (FAST) {
      if (ch >= cdim) {            // uniform branch on SGPRs (scalar unit), never diverges
        ch = 0;
        ++tap;
        if (++kx == a.kw) kx = 0, ++ky;
      }
    } else if constexpr (KM == K_SMALL) {
      while (ch >= cdim) {
        ch -= cdim;
        ++tap;
        if (++kx == a.tk_w) kx = 0, ++ky;
      }
    } else {
      const bool wrap = ch >= cdim;
      ch -= wrap ? cdim : 0;
      tap += wrap ? 1 : 0;
      const bool roww = wrap & (kx + 1 == a.tk_w);
      kx = roww ? 0 : kx + (wrap ? 1 : 0);
      ky += roww ? 1 : 0;
    }
  }
};

// A rows of the forward pass (pixels of x) and of the data gradient (pixels of dy): row i of the thread is GEMM row m0 + r + 32 * i. The window entry serves the forward
// pass and the stride-1 data gradient (igemm_gather_window); K_PW folds a row's validity into its base offset once; the per-lane data gradient (K_MID / K_SMALL,
// stride 2, parity classes) is the second entry.
template <int MODE, int BM, int KM>
struct IgemmPixelGather {
  static constexpr bool FAST = KM == K_FAST || KM == K_PW, PW = KM == K_PW;
  static constexpr int N = BM / 32;
  int base[N], y0[N], x0[N];      // byte offset of the window origin (per-lane data gradient: pixel offset of the image), window origin
  __device__ __forceinline__ void init(const ConvK& a, int m0, int g, int r, int xp4, int yp4) {
    const int rh = (MODE == MODE_FWD) ? a.Ho : (a.sub ? a.Hc : a.H), rw = (MODE == MODE_FWD) ? a.Wo : (a.sub ? a.Wc : a.W);
    const bool pointwise = FAST && a.kh * a.kw == 1 && a.stride == 1 && a.pad == 0 && !a.sub;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int m = m0 + r + 32 * i;
      int b = 0, y = -(1 << 28), x = -(1 << 28);      // (one store per member and row, behind the branches: stores sunk out of them address the struct dynamically -> scratch)
      if (PW) {          // the launcher vouches for a pointwise problem: rows beyond M carry an out-of-range base, nothing else is checked per K-step
        y = x = 0;
        b = m < a.M ? m * (MODE == MODE_FWD ? xp4 : yp4) + g * 16 : OOB;
      } else if (pointwise) {   // 1x1 / stride 1 / no padding (and every Winograd GEMM): pixel m of the operand, no index decomposition
        y = x = m < a.M ? 0 : -(1 << 28);
        b = m < a.M ? m * (MODE == MODE_FWD ? xp4 : yp4) + (FAST ? g * 16 : 0) : 0;
      } else if (m < a.M) {
        const int img = m / (rh * rw), rem = m - img * (rh * rw);
        const int py = rem / rw, px = rem - py * rw;
        if constexpr (MODE == MODE_FWD) {
          y = py * a.stride - a.pad;
          x = px * a.stride - a.pad;
          b = (img * a.H * a.W + y * a.W + x) * xp4 + (FAST ? g * 16 : 0);
        } else {
          y = (a.sub ? 2 * py + a.sub_cy : py) + a.pad;
          x = (a.sub ? 2 * px + a.sub_cx : px) + a.pad;
          b = FAST ? ((img * a.Ho + y) * a.Wo + x) * yp4 + g * 16 : img * a.Ho * a.Wo;
        }
      }
      base[i] = b, y0[i] = y, x0[i] = x;
    }
  }
  __device__ __forceinline__ void load(const ConvK& a, __amdgpu_buffer_rsrc_t rA, const IgemmKState<MODE, KM>& ks, int xp4, int yp4, v4f* ra) const {
    [[maybe_unused]] const bool tok = ks.tap < a.T_eff;
    if constexpr (PW) {
      // wave-uniform offset; a K-step beyond the reduction (the software pipeline's run-ahead) moves every offset out of the descriptor's range: no traffic
      const unsigned toff = (unsigned)(ks.ch * 4) + (tok ? 0u : 0x80000000u);
#pragma unroll
      for (int i = 0; i < N; ++i) ra[i] = bload(rA, (unsigned)base[i] + toff);
    } else if constexpr (MODE == MODE_FWD) {
      const int dy = ks.ky * a.dil, dx = ks.kx * a.dil;
      igemm_gather_window<1, N>(rA, base, y0, x0, dy, dx, (dy * a.W + dx) * xp4 + ks.ch * 4, tok, a.H, a.W, ra);
    } else if constexpr (FAST) {   // stride 1, Cout % BK == 0: uniform (tap, co0)
      const int dy = ks.ky * a.dil, dx = ks.kx * a.dil;
      igemm_gather_window<-1, N>(rA, base, y0, x0, dy, dx, (dy * a.Wo + dx) * yp4 - ks.ch * 4, tok, a.Ho, a.Wo, ra);
    } else {
      const int dy = (a.ky0 + a.ksy * ks.ky) * a.dil, dx = (a.kx0 + a.ksx * ks.kx) * a.dil, smask = a.stride - 1;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int ty = y0[i] - dy, tx = x0[i] - dx;
        const int oy = ty >> a.sshift, ox = tx >> a.sshift;
        const bool ok = tok & ((ty | tx) >= 0) & (((ty | tx) & smask) == 0) & (oy < a.Ho) & (ox < a.Wo);   // '&': no short-circuit branches
        const int off = (base[i] + oy * a.Wo + ox) * yp4 + ks.ch * 4;   // computed unconditionally: keeps the loop body branch-free
        ra[i] = bload(rA, ok ? off : OOB);
      }
    }
  }
};

// B of the forward pass (weight rows [Cout][K], k contiguous: row n0 + r + 32 * i, k-group g) and of the data gradient (the weights viewed [k][Cin]: k-row r, ci
// group g + 8 * j). The per-lane data gradient keeps the (tap, co) of its own k-row.
template <int MODE, int BN, int KM>
struct IgemmWeightGather {
  static constexpr bool FAST = KM == K_FAST || KM == K_PW, PW = KM == K_PW;
  static constexpr int N = BN / 32;
  int base[N];
  int co = 0, tap = 0;      // per-lane data gradient: (tap, co) of k-row r
  __device__ __forceinline__ void init(const ConvK& a, int n0, int k_begin, int g, int r) {
    if constexpr (MODE == MODE_FWD) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int row = n0 + r + 32 * i;
        base[i] = row < a.Cout ? row * a.K * 4 + g * 16 : OOB;
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int col = n0 + (g + 8 * j) * 4;
        base[j] = col < a.Cin ? col * 4 + (FAST ? r * (a.kh * a.kw) * a.Cin * 4 : 0) : OOB;
      }
      if constexpr (!FAST) {
        const int k = k_begin + r;
        tap = k / a.Cout;
        co = k - tap * a.Cout;
      }
    }
  }
  __device__ __forceinline__ void load(const ConvK& a, __amdgpu_buffer_rsrc_t rB, const IgemmKState<MODE, KM>& ks, int kbase, int k_end, int g, int r, v4f* rb) const {
    const int Treal = a.kh * a.kw;         // tap stride of the KRSC weight layout
    [[maybe_unused]] const bool tok = ks.tap < a.T_eff;
    if constexpr (PW) {
      const unsigned beyond = 0x80000000u;
      const unsigned off = MODE == MODE_FWD ? (kbase < k_end ? (unsigned)(kbase * 4) : beyond) : (tok ? (unsigned)((ks.ch * Treal + ks.tap) * a.Cin * 4) : beyond);
#pragma unroll
      for (int i = 0; i < N; ++i) rb[i] = bload(rB, (unsigned)base[i] + off);
    } else if constexpr (MODE == MODE_FWD) {
      const bool kok = FAST ? (kbase < k_end) : (kbase + g * 4 < k_end);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int off = base[i] + kbase * 4;   // base already carries this thread's k-group (g * 16 bytes)
        rb[i] = bload(rB, (kok & (base[i] != OOB)) ? off : OOB);
      }
    } else {
      bool rok;
      int roff;
      if constexpr (FAST) {
        rok = tok, roff = (ks.ch * Treal + ks.tap) * a.Cin * 4;
      } else {
        rok = (tap < a.T_eff) & (kbase + r < k_end);
        const int tky = tap / a.tk_w, tkx = tap - tky * a.tk_w;
        roff = (co * Treal + (a.ky0 + a.ksy * tky) * a.kw + a.kx0 + a.ksx * tkx) * a.Cin * 4;
      }
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int off = roff + base[j];
        rb[j] = bload(rB, (rok & (base[j] != OOB)) ? off : OOB);
      }
    }
  }
  __device__ __forceinline__ void advance(const ConvK& a) {
    if constexpr (MODE == MODE_DGRAD && !FAST) {
      co += BK;
      if constexpr (KM == K_SMALL) {
        while (co >= a.Cout) co -= a.Cout, ++tap;
      } else {
        const bool wrap = co >= a.Cout;
        co -= wrap ? a.Cout : 0;
        tap += wrap ? 1 : 0;
      }
    }
  }
};

// The weight gradient's pair: A = dy columns (m contiguous: k-row r is output pixel k, channel groups g + 8 * j), B = the x window of that pixel under the tap of
// column group j. KX pixel rows per thread (PREC 4: r and r + 32, eight bf16 channels per 16-byte gather).
template <int BM, int BN, int KM, int PREC>
struct IgemmWgradGather {
  static constexpr bool NAT16 = PREC == 4;
  static constexpr int KX = NAT16 ? 2 : 1, BKW = BK * KX, EPL = NAT16 ? 8 : 4, ESZ = NAT16 ? 2 : 4;      // pixel rows, pixels per K-step, elements per gather, bytes per element
  static constexpr int A_NL = NAT16 ? (BM / 32 + 1) / 2 : BM / 32, B_NL = NAT16 ? (BN / 32 + 1) / 2 : BN / 32;      // 16-byte gathers per thread, tile and pixel row
  int a_col[A_NL];                           // byte offset of dy channel group j (OOB beyond Cout)
  int b_base[B_NL], b_dy[B_NL], b_dx[B_NL];  // tap + channel byte offset of column group j, its tap displacement
  int ox[KX], oy[KX], img[KX];               // output pixel of this thread's k-row(s)
  __device__ __forceinline__ void init(const ConvK& a, int m0, int n0, int k_begin, int g, int r, int xp4) {
#pragma unroll
    for (int j = 0; j < A_NL; ++j) {
      const int col = m0 + (g + 8 * j) * EPL;
      a_col[j] = col < a.Cout ? col * ESZ : OOB;
    }
#pragma unroll
    for (int j = 0; j < B_NL; ++j) {
      const int n = n0 + (g + 8 * j) * EPL;
      const int tap = n < a.Nn ? n / a.Cin : 0;
      const int ky = tap / a.kw, kx = tap - ky * a.kw;
      b_dy[j] = ky * a.dil - a.pad;
      b_dx[j] = kx * a.dil - a.pad;
      b_base[j] = n < a.Nn ? (b_dy[j] * a.W + b_dx[j]) * xp4 + (n - tap * a.Cin) * ESZ : OOB;
    }
#pragma unroll
    for (int kk = 0; kk < KX; ++kk) {
      const int p = k_begin + r + 32 * kk;
      img[kk] = p / (a.Ho * a.Wo);
      const int rem = p - img[kk] * (a.Ho * a.Wo);
      oy[kk] = rem / a.Wo;
      ox[kk] = rem - oy[kk] * a.Wo;
    }
  }
  __device__ __forceinline__ void load(const ConvK& a, __amdgpu_buffer_rsrc_t rA, __amdgpu_buffer_rsrc_t rB, int kbase, int k_end, int r, bool doA, bool doB, int xp4, int yp4,
                                       v4f* ra, v4f* rb) const {
#pragma unroll
    for (int kk = 0; kk < KX; ++kk) {
      const int p = kbase + r + 32 * kk;
      const bool pok = p < k_end;
      const int poff = p * yp4;
      if (doA)
#pragma unroll
      for (int j = 0; j < A_NL; ++j) {
        const int off = poff + a_col[j];
        ra[kk * A_NL + j] = bload(rA, (pok & (a_col[j] != OOB)) ? off : OOB);
      }
      const int by = oy[kk] * a.stride, bx = ox[kk] * a.stride;
      const int rowbase = ((img[kk] * a.H + by) * a.W + bx) * xp4;
      if (doB)
#pragma unroll
      for (int j = 0; j < B_NL; ++j) {
        const bool ok = pok & (b_base[j] != OOB) & ((unsigned)(by + b_dy[j]) < (unsigned)a.H) & ((unsigned)(bx + b_dx[j]) < (unsigned)a.W);
        const int off = rowbase + b_base[j];
        rb[kk * B_NL + j] = bload(rB, ok ? off : OOB);
      }
    }
  }
  __device__ __forceinline__ void advance(const ConvK& a) {
#pragma unroll
    for (int kk = 0; kk < KX; ++kk) {
      ox[kk] += BKW;
      if constexpr (KM == K_SMALL) {
        while (ox[kk] >= a.Wo) {
          ox[kk] -= a.Wo;
          if (++oy[kk] == a.Ho) oy[kk] = 0, ++img[kk];
        }
      } else {      // Wo >= BKW: at most one wrap per step
        const bool wrap = ox[kk] >= a.Wo;
        ox[kk] -= wrap ? a.Wo : 0;
        const bool imgw = wrap & (oy[kk] + 1 == a.Ho);
        oy[kk] = imgw ? 0 : oy[kk] + (wrap ? 1 : 0);
        img[kk] += imgw ? 1 : 0;
      }
    }
  }
};

// Thread -> tile element mapping (256 threads, g = t & 7, r = t >> 3; the LDS layouts of conv_igemm_parts.h):
//   k-contiguous (KC) tiles: thread owns k-group g (4 floats) of rows r + 32*i   -> 1 K-state, static rows
//   m-contiguous (MC) tiles: thread owns k-row r, column groups (g + 8*j) * 4      -> 1 K-state, static cols
// PREC 0: operands stay fp32 -> v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 157 TF). PREC 1: the fp32 tiles staged in LDS are
// rounded to bf16 (RNE, v_cvt_pk_bf16_f32) as the fragments are read -> v_mfma_f32_32x32x16_bf16 with fp32 accumulation (2.5 PF):
// BASELINE configs[2]. Gathers, LDS layout and epilogue are shared; storage stays fp32.
// NST: LDS stages. 1 = single buffer for reductions of <= 64 K-steps (K <= 2048: every 1x1 convolution and Winograd GEMM of the
// flagship), 2 = double-buffered beyond that. A single stage halves the LDS footprint so that three blocks share a CU and cover each other's load / store phases.
// STATS: the staged epilogue also emits the BatchNorm statistics of the tile (a separate instantiation, so that the register budget and the
// occupancy of the kernel without statistics are untouched: 72 vs 74 VGPRs on the 64 x 64 forward tile = 7 vs 6 waves per SIMD).
template <int MODE, int BM, int BN, int WM, int WN, int KM, int PREC, int NST, bool STATS = false>
__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(const ConvK a) {
  constexpr bool A_KC = (MODE != MODE_WGRAD);  // A tile stored [BM][LDK] (k contiguous) else [BK][BM]
  constexpr bool B_KC = (MODE == MODE_FWD);    // B tile stored [BN][LDK] else [BK][BN]
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  // PREC 3 (weight gradient of the bf16 tier): the pixel-major (m-contiguous) tiles are kept in LDS as bf16 [BK][BM + 32] -- rounded once, as the
  // gathered fp32 rows are stored -- and the MFMA fragments (8 consecutive k per lane) come out of them through the hardware transpose read
  // ds_read_b64_tr_b16. The 32-element pad puts the four k-rows one read touches on four disjoint bank quarters (row stride = 64 B mod 256 B).
  // PREC 4: the same with NATIVE bf16 operands (bf16 activations in HBM, BASELINE configs[2] round 4): a lane gathers 16 bytes = eight channels and stores them
  // to LDS as they are -- half the gather instructions, no conversion.
  constexpr bool TR = (PREC == 3 || PREC == 4);
  constexpr bool NAT16 = (PREC == 4);
  // PREC 5 (round 6): the fp32 tier on the bf16 matrix pipe. Every gathered fp32 element is split -- ONCE per block, as the gathered rows are stored to LDS -- into
  // three bf16 pieces by truncation: hi = x & 0xffff0000, r = x - hi (exact), mid = r & 0xffff0000, lo = r - mid (exact: at most eight significant bits are left),
  // so x == hi + mid + lo exactly. LDS holds three bf16 planes per operand tile; a K-step multiplies six cross products (hi hi, hi mid, mid hi, mid mid, hi lo,
  // lo hi; the dropped mid lo + lo mid + lo lo are <= 3 * 2^-24 of |a b|) on v_mfma_f32_32x32x16_bf16 into the same fp32 accumulators: 6 / 16 of the fp32 MFMA's
  // matrix-pipe cycles per K-step. Measured against fp64 (tools/micro/split_gemm.hip): the same error class as the fp32 fma chain of PREC 0.
  constexpr bool SPL = (PREC == 5);
  // K-step of this instantiation. PREC 4 takes 64 pixels per step (a thread gathers two pixel rows, r and r + 32): the bf16 MFMA phase of a 32-pixel step is 256
  // cycles per wave -- too short for one barrier pair and one round of address arithmetic; the forward kernels' steps are 64 deep as well (round 4: 465 -> see DESIGN)
  constexpr int KX = NAT16 ? 2 : 1, BKW = BK * KX;
  static_assert(!TR || MODE == MODE_WGRAD, "PREC 3 / 4 are the weight-gradient forms");
  using LA = LdsTile<PREC, A_KC, BM>;      // the LDS layout of each operand's tile
  using LB = LdsTile<PREC, B_KC, BN>;
  constexpr int A_FLOATS = LA::FLOATS, STAGE = A_FLOATS + LB::FLOATS;
  constexpr int A_N = BM / 32, B_N = BN / 32;  // float4 per thread and tile
  static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && BK == 32, "bad tile config");

  extern __shared__ __align__(16) float smem[];
  if constexpr (PREC == 5) {
    // Two blocks share a CU, i.e. two waves share each SIMD's VALU issue and matrix pipe. Equal waves that start together STAY together: both split (VALU) at the
    // same time, then both multiply (measured: VALU issue 44 % + matrix pipe 57 % of the kernel's cycles ~ 100 %, no overlap at all). A static priority for the wave
    // in the odd hardware slot lets it run ahead by one phase, after which the partner's VALU phase fills the leader's MFMA phase and vice versa.
    if (a.spl_prio && (__builtin_amdgcn_s_getreg(0x1804) & 1)) __builtin_amdgcn_s_setprio(2);      // hwreg(HW_REG_HW_ID, 0, 4): the wave's slot on its SIMD
  }

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int half = lane >> 5, l31 = lane & 31;
  const int g = t & 7, r = t >> 3;

  int tile_m, tile_n, by, z;
  igemm_tile_map(a, a.tiles_m * a.tiles_n, tile_m, tile_n, by, z);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int k_begin = z * a.kper;
  const int k_end = min(a.K, k_begin + a.kper);
  const int nk = (k_end - k_begin + BKW - 1) / BKW;

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A + by * a.a_bs), 0, (int)a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.B + by * a.b_bs), 0, (int)a.b_bytes, 0x00020000);
  const int xp4 = (int)a.x_pitch * (NAT16 ? 2 : 4), yp4 = (int)a.y_pitch * (NAT16 ? 2 : 4);      // bytes between pixels
  constexpr int A_NL = NAT16 ? (A_N + 1) / 2 : A_N, B_NL = NAT16 ? (B_N + 1) / 2 : B_N;            // 16-byte gathers per thread and tile

  // the gathers of this instantiation (the unused role's state is never touched and folds away)
  IgemmKState<MODE, KM> ks;
  IgemmPixelGather<MODE, BM, KM> ga;
  IgemmWeightGather<MODE, BN, KM> gb;
  IgemmWgradGather<BM, BN, KM, PREC> gw;
  if constexpr (MODE != MODE_WGRAD) {
    ga.init(a, m0, g, r, xp4, yp4);
    ks.init(a, k_begin, g);
    gb.init(a, n0, k_begin, g, r);
  } else {
    gw.init(a, m0, n0, k_begin, g, r, xp4);
  }
  v4f ra[A_N], rb[B_N];
  auto load_tiles = [&](int kt, int which = 0) {   // which: 0 both operands, 1 A only, 2 B only
    const int kbase = k_begin + kt * BKW;
    if constexpr (MODE != MODE_WGRAD) {
      if (which != 2) ga.load(a, rA, ks, xp4, yp4, ra);
      if (which != 1) gb.load(a, rB, ks, kbase, k_end, g, r, rb);
    } else {
      gw.load(a, rA, rB, kbase, k_end, r, which != 2, which != 1, xp4, yp4, ra, rb);
    }
  };
  auto advance = [&]() {  // move the K-state one K-step forward
    if constexpr (MODE != MODE_WGRAD) ks.advance(a), gb.advance(a);
    else gw.advance(a);
  };

  // PREC 5: the split pieces of the gathered rows wait in registers (sa / sb) between the split -- interleaved with the MFMAs of the running K-step -- and the
  // LDS write behind the barrier
  uint2 sa[SPL ? A_N : 1][3], sb[SPL ? B_N : 1][3];
  auto split_a = [&]() {
    if constexpr (SPL) {
#pragma unroll
      for (int i = 0; i < A_N; ++i) split4(ra[i], sa[i][0], sa[i][1], sa[i][2]);
    }
  };
  auto split_b = [&]() {
    if constexpr (SPL) {
#pragma unroll
      for (int i = 0; i < B_N; ++i) split4(rb[i], sb[i][0], sb[i][1], sb[i][2]);
    }
  };
  auto write_planes = [&](int buf) {
    if constexpr (SPL) {
      float* As = smem + buf * STAGE;
#pragma unroll
      for (int i = 0; i < A_N; ++i) LA::store(As, r, g, i, sa[i]);
#pragma unroll
      for (int i = 0; i < B_N; ++i) LB::store(As + A_FLOATS, r, g, i, sb[i]);
    }
  };
  auto store_tiles = [&](int buf) {
    float* As = smem + buf * STAGE;
    if constexpr (SPL) {
      split_a();
      split_b();
      write_planes(buf);
    } else {
      lds_store_operand<PREC, A_KC, BM, A_NL>(As, r, g, ra);
      lds_store_operand<PREC, B_KC, BN, B_NL>(As + A_FLOATS, r, g, rb);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  auto compute_kg = [&](int buf, int kg) {   // one 8-k group (fp32) or one 16-k block (bf16: kg = 0, 2 cover the slab)
    const float* As = smem + buf * STAGE;
    const float* Bs = As + A_FLOATS;
    if constexpr (TR) {
      // bf16 [k][m] tiles, fragments through ds_read_b64_tr_b16: within a 16-lane group lane i hands in the address of row (i >> 2), column block
      // (i & 3) * 4 and receives column i of those four rows (tools/micro/tr_probe.hip) -- four consecutive k of its own m. Two reads = the lane's
      // eight k of v_mfma_f32_32x32x16_bf16 (lanes 32..63: the upper eight k of the 16-k block).
      if (kg & 1) return;                                   // two 16-k blocks per slab, issued on the even groups
      const int krow = (kg >> 1) * 16 + half * 8 + ((lane & 15) >> 2);
      const int cofs = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = LA::frag(As, krow, wm * (BM / WM) + i * 32 + cofs);
#pragma unroll
      for (int i = 0; i < TN; ++i) fb[i] = LB::frag(Bs, krow, wn * (BN / WN) + i * 32 + cofs);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int n = 0; n < TN; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[n], acc[i][n], 0, 0, 0);
    } else if constexpr (SPL) {
      if (kg & 1) return;                                   // two 16-k blocks per slab, issued on the even groups
      const int krow = (kg >> 1) * 16 + half * 8 + ((lane & 15) >> 2);
      const int cofs = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
      const int kk = (kg >> 1) * 8 + half * 4;              // float offset of this lane-half's eight bf16 k inside a 64-byte plane row
      bf16x8 fa[3][TM], fb[3][TN];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          fa[p][i] = LA::frag(As, p, wm * (BM / WM) + i * 32 + l31, kk, krow, wm * (BM / WM) + i * 32 + cofs);      // k-contiguous rows take (row, kk), planes (krow, column)
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          fb[p][i] = LB::frag(Bs, p, wn * (BN / WN) + i * 32 + l31, kk, krow, wn * (BN / WN) + i * 32 + cofs);
        }
      }
#define PM_SPL_PROD(PA, PB)                                                                                  \
  _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int n = 0; n < TN; ++n) acc[i][n] = \
      __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA][i], fb[PB][n], acc[i][n], 0, 0, 0);
      PM_SPL_PROD(2, 0) PM_SPL_PROD(0, 2) PM_SPL_PROD(1, 1) PM_SPL_PROD(1, 0) PM_SPL_PROD(0, 1) PM_SPL_PROD(0, 0)
#undef PM_SPL_PROD
    } else if constexpr (PREC == 2) {
      // bf16 operands in HBM and LDS (bf16.hip): the tensors enter as fp32-typed views with half the channels, so one float4 of a
      // k-contiguous LDS row is 8 consecutive bf16 k-values -- exactly this lane-half's operand of v_mfma_f32_32x32x16_bf16. Gather,
      // LDS layout (128-byte rows = 64 k, padded to 144 B) and epilogue are the fp32 code unchanged; 8 x fewer MFMA cycles per slab.
      static_assert(A_KC && B_KC, "bf16 tiles need k-contiguous operands (forward form)");
      const int kk = kg * 8 + half * 4;
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4*>(As + (wm * (BM / WM) + i * 32 + l31) * LDK + kk));
#pragma unroll
      for (int i = 0; i < TN; ++i) fb[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4*>(Bs + (wn * (BN / WN) + i * 32 + l31) * LDK + kk));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int n = 0; n < TN; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[n], acc[i][n], 0, 0, 0);
    } else if constexpr (PREC == 0) {
      const int kk = kg * 8 + half * 4;  // this lane-half's 4 consecutive k of the 8-k group
      float fa[TM][4], fb[TN][4];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * (BM / WM) + i * 32 + l31;
        if constexpr (A_KC) {
          const float4 v = *reinterpret_cast<const float4*>(As + row * LDK + kk);
          fa[i][0] = v.x, fa[i][1] = v.y, fa[i][2] = v.z, fa[i][3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) fa[i][j] = As[(kk + j) * BM + row];
        }
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int col = wn * (BN / WN) + i * 32 + l31;
        if constexpr (B_KC) {
          const float4 v = *reinterpret_cast<const float4*>(Bs + col * LDK + kk);
          fb[i][0] = v.x, fb[i][1] = v.y, fb[i][2] = v.z, fb[i][3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) fb[i][j] = Bs[(kk + j) * BN + col];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int n = 0; n < TN; ++n)
            acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][j], fb[n][j], acc[i][n], 0, 0, 0);
    } else {
      if (kg & 1) return;                       // bf16: two 16-k blocks per slab, issued on the even groups
      const int kk = (kg >> 1) * 16 + half * 8;  // this lane-half's 8 consecutive k of the 16-k block
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * (BM / WM) + i * 32 + l31;
        float v[8];
        if constexpr (A_KC) {
          const float4 p = *reinterpret_cast<const float4*>(As + row * LDK + kk), q = *reinterpret_cast<const float4*>(As + row * LDK + kk + 4);
          v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w, v[4] = q.x, v[5] = q.y, v[6] = q.z, v[7] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = As[(kk + j) * BM + row];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) fa[i][j] = (__bf16)v[j];
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int col = wn * (BN / WN) + i * 32 + l31;
        float v[8];
        if constexpr (B_KC) {
          const float4 p = *reinterpret_cast<const float4*>(Bs + col * LDK + kk), q = *reinterpret_cast<const float4*>(Bs + col * LDK + kk + 4);
          v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w, v[4] = q.x, v[5] = q.y, v[6] = q.z, v[7] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = Bs[(kk + j) * BN + col];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) fb[i][j] = (__bf16)v[j];
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int n = 0; n < TN; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[n], acc[i][n], 0, 0, 0);
    }
  };
  auto compute = [&](int buf) {
#pragma unroll
    for (int kg = 0; kg < BKW / 8; ++kg) compute_kg(buf, kg);
  };

  // ---- main loop: the gathers of slab kt+1 are issued (branch-free) ahead of the MFMAs of slab kt, whose 4096 matrix-pipe
  // cycles cover the load latency; LDS is double-buffered, one barrier per K-step ----------------------------------------
  if constexpr (SPL && NST == 1) {
    // PREC 5, one LDS stage, two blocks per CU. A wave's split (VALU) runs in the shadow of its OWN MFMAs -- measured: two equal waves on a SIMD do not fill each
    // other's phases (VALU issue 44 % + matrix pipe 57 % of the cycles, no overlap) -- so the K-step is software-pipelined inside the wave:
    //   first 16-k group's MFMAs  | split of the A rows of step kt + 1 (registers -> registers) | A gathers of step kt + 2 issued
    //   second 16-k group's MFMAs | split of the B rows of step kt + 1                          | B gathers of step kt + 2 issued
    //   barrier | write the planes of step kt + 1 | barrier
    // A gather has one K-step (~1.5 k cycles) to land before its split; a gather beyond the last K-step presents out-of-range offsets (no traffic).
    if (nk > 0) {
      load_tiles(0);
      advance();
      split_a(), split_b();
      write_planes(0);
      __syncthreads();
      load_tiles(1);
      advance();
      constexpr int NDS = 3 * (TM * (A_KC ? 1 : 2) + TN * (B_KC ? 1 : 2));      // fragment reads of one 16-k group
      constexpr int NMF = 6 * TM * TN;                                           // MFMAs of one 16-k group
      for (int kt = 0; kt < nk; ++kt) {
        compute_kg(0, 0);
        split_a();
        load_tiles(kt + 2, 1);
        __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
#pragma unroll
        for (int q = 0; q < NMF; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x006, 5, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        compute_kg(0, 2);
        split_b();
        load_tiles(kt + 2, 2);
        __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
#pragma unroll
        for (int q = 0; q < NMF; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x006, 5, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();          // every wave is done reading the single buffer
        write_planes(0);          // unconditional (behind the last K-step: zeros nobody reads) and in the same basic block as the splits: a conditional write lets
        __syncthreads();          // the compiler sink the split arithmetic behind the barrier, out of the MFMAs' shadow
        advance();                // (its wave-uniform branches end the block: behind the write for the same reason)
      }
    }
  } else if constexpr (NST == 1) {
    if (nk > 0) {
      load_tiles(0);
      advance();
      store_tiles(0);
      __syncthreads();
      for (int kt = 0; kt < nk - 1; ++kt) {
        load_tiles(kt + 1);
        __builtin_amdgcn_sched_barrier(0);
        advance();
        compute(0);
        __syncthreads();          // every wave is done reading the single buffer
        store_tiles(0);
        __syncthreads();
      }
      compute(0);
    }
  } else if (nk > 0) {
    load_tiles(0);
    advance();
    store_tiles(0);
    __syncthreads();
    for (int kt = 0; kt < nk - 1; ++kt) {
      // Region 1: first k-group (fragment reads + TM*TN*4 MFMAs) with the whole gather of slab kt+1 (address VALU + the
      // buffer loads) interleaved into the 64-cycle MFMA shadows, so the matrix pipe restarts right after the barrier.
      compute_kg(kt & 1, 0);
      load_tiles(kt + 1);
      advance();
      __builtin_amdgcn_sched_group_barrier(0x100, TM + TN + (A_KC ? 0 : 3 * TM) + (B_KC ? 0 : 3 * TN), 0);  // fragment DS reads
#define PM_SG(I)                                                                   \
      if constexpr ((A_NL + B_NL) * KX > I) {                                                \
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  /* 2 MFMA            */ \
        __builtin_amdgcn_sched_group_barrier(0x006, 8, 0);  /* <= 8 VALU / SALU  */ \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  /* 1 buffer load     */ \
      }
      PM_SG(0) PM_SG(1) PM_SG(2) PM_SG(3) PM_SG(4) PM_SG(5) PM_SG(6) PM_SG(7)
#undef PM_SG
      __builtin_amdgcn_sched_barrier(0);
      // Region 2: the remaining three k-groups cover the load latency; then the LDS write of slab kt+1 and the barrier
#pragma unroll
      for (int kg = 1; kg < BKW / 8; ++kg) compute_kg(kt & 1, kg);
      store_tiles((kt + 1) & 1);
      __syncthreads();
    }
    compute((nk - 1) & 1);
  }

  // ---- epilogue -------------------------------------------------------------------------------------------------
  // Split-K slabs are plain fp32 whatever the tier. Otherwise: the staged form for every output of 16-byte row segments (bf16: eight columns per lane, fp32: four),
  // the per-element form for the rest -- batched launches (stage_ep == 0), the 19 class logits, a bf16 residual that is a channel slice off a 16-byte boundary
  // (pm_conv_fwd does not constrain the residual's pitch or alignment, so the C ABI admits that call).
  float* Cb = a.C + by * a.c_bs + (a.ksplit > 1 ? (long)z * a.c_split : 0);
  const bool plain = a.ksplit > 1 || !(a.bias || a.scale || a.residual || a.relu);
  const bool aff = !plain && (a.bias || a.scale), res = !plain && a.residual, relu = !plain && a.relu;
  const int rbase = m0 + wm * (BM / WM) + 4 * half, cbase = n0 + wn * (BN / WN) + l31;
  if (a.io16 && a.ksplit == 1) {
    pm_bf16* C16 = reinterpret_cast<pm_bf16*>(a.C) + by * a.c_bs;
    const pm_bf16* R16 = reinterpret_cast<const pm_bf16*>(a.residual);
    if (((a.c_pitch | a.Nn | (a.residual ? a.res_pitch : 0)) & 7) == 0 && ((reinterpret_cast<uintptr_t>(a.C) | reinterpret_cast<uintptr_t>(a.residual)) & 15) == 0)
      igemm_epilogue_staged<pm_bf16, false, STATS, BM, BN, WM, WN>(a, C16, R16, smem, acc, m0, n0, wm, wn, wave, lane, l31, half, aff, res, relu);
    else
      igemm_epilogue_elems<pm_bf16, true>(a, C16, R16, acc, rbase, cbase, true, R16 != nullptr, a.relu != 0);
    return;
  }
  const bool vec = a.stage_ep && ((a.c_pitch | a.Nn | (a.residual ? a.res_pitch : 0)) & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(Cb) | reinterpret_cast<uintptr_t>(a.residual)) & 15) == 0;
  if (vec) {
    igemm_epilogue_staged<float, MODE == MODE_DGRAD, STATS, BM, BN, WM, WN>(a, Cb, a.residual, smem, acc, m0, n0, wm, wn, wave, lane, l31, half, aff, res, relu);
  } else if (m0 + BM <= a.M && n0 + BN <= a.Nn) {
    // interior tile: straight-line code specialised on the (wave-uniform) fused operations, no per-element predicate
#define PM_EP(AFF, RES, RELU) igemm_epilogue_elems<float, false>(a, Cb, a.residual, acc, rbase, cbase, AFF, RES, RELU)
    if (!aff && !res && !relu) PM_EP(false, false, false);
    else if (!aff && res && !relu) PM_EP(false, true, false);       // dgrad + fused skip gradient
    else if (aff && !res && !relu) PM_EP(true, false, false);       // conv + bias
    else if (aff && !res && relu) PM_EP(true, false, true);         // eval: conv + folded BN + ReLU
    else if (aff && res && relu) PM_EP(true, true, true);           // eval: bottleneck tail
    else if (aff && res && !relu) PM_EP(true, true, false);
    else if (!aff && res && relu) PM_EP(false, true, true);
    else PM_EP(false, false, true);
#undef PM_EP
  } else {
    // fp32 edge tile (the 19 class logits): written out. Through igemm_epilogue_elems<float, true> the per-element branches became selects and the forward pass of the
    // class head (1x1 256 -> 19 at 192 x 192) measured 0.076 -> 0.082 ms (profiles/igemm_refactor_ab.txt).
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = cbase + n * 32;
        const bool cok = col < a.Nn;
        float bi = 0.f, sc = 1.f, sh = 0.f;
        if (!plain && cok) {
          if (a.bias) bi = a.bias[col];
          if (a.scale) sc = a.scale[col], sh = a.shift[col];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = rbase + i * 32 + (q & 3) + 8 * (q >> 2);
          if (row < a.M && cok) {
            float v = acc[i][n][q];
            if (!plain) {
              v = (v + bi) * sc + sh;
              if (a.residual) v += a.residual[(long)row * a.res_pitch + col];
              if (a.relu) v = fmaxf(v, 0.f);
            }
            Cb[(long)row * a.c_pitch + col] = v;
          }
        }
      }
  }
}

// One instantiation's launch: the > 64 KB dynamic-LDS opt-in, made once per device and kernel (pm_lds_optin), then the launch on `smem` bytes of LDS.
template <auto KERNEL>
void igemm_launch(const ConvK& k, dim3 grid, size_t smem, hipStream_t st) {
  static pm_lds_optin optin;
  (void)optin(reinterpret_cast<const void*>(KERNEL), 160 * 1024);
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), smem, st, k);
}

}  // namespace
