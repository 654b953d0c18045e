// The pieces conv_igemm_kernel (conv_igemm_kernel.h) is put together from, each written once: the kernel parameter block, the 16-byte buffer load and the operand
// conversions (shared with pwstream.hip), the tile map, one LDS layout trait per layout (A and B call the same code with their own extents; the transpose read),
// the staged and the per-element epilogue over pm_elem<float> / pm_elem<pm_bf16>. The kernel keeps its constants, the gather, the K-group multiply and the three
// main-loop schedules.
// Helpers take lane / l31 / half from the kernel instead of recomputing them (profiles/conv16_resource_usage.txt: recomputing cost registers there).
#pragma once
#include <stdint.h>
#include <type_traits>

#include "pm_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// kernel parameter block (global namespace: conv_igemm.hip hands it to the PREC 5 launcher of conv_split.hip)
struct ConvK {
  const float* A;
  const float* B;
  float* C;
  int N, H, W, Cin;       // conv input tensor (x / dx)
  int Ho, Wo, Cout;       // conv output tensor (y / dy)
  long x_pitch, y_pitch;  // floats between pixels
  int kh, kw, stride, pad, dil, sshift;
  int M, Nn, K;           // GEMM extents
  int ksplit;             // gridDim.z
  int kper;               // K range per split (multiple of BK)
  long c_pitch;           // row pitch of C
  long c_split;           // floats between split-K slabs (ksplit > 1 -> C is the workspace)
  long a_bs, b_bs, c_bs;  // batched launch (gridDim.y > 1, the 16 / 36 Winograd points): floats between consecutive A / B / C operands
  int tiles_m, tiles_n;
  unsigned a_bytes, b_bytes;  // extents of the A / B buffers (buffer-descriptor range)
  int kmode;                  // K_FAST / K_MID / K_SMALL: how the gather's K-state advances (see the kernel; the launchers derive K_PW from it)
  int prec;                   // the kernel's PREC: 0 fp32 MFMA; 1 fp32 tiles rounded to bf16 per fragment; 2 bf16 operands in HBM and LDS (fp32-typed views); 3 / 4 the weight
                              // gradient's transpose-read tiles from fp32 / bf16 rows; 5 fp32 operands split into three bf16 pieces (set by launch(), conv_split.hip)
  // tap list actually iterated: rows ky0 + ksy*i (i < nky), cols kx0 + ksx*j (j < tk_w); T_eff = nky * tk_w. The full kernel
  // window for fwd / wgrad / stride-1 dgrad; the parity-matching subset for one input-pixel class of a stride-2 dgrad.
  int T_eff, tk_w, ky0, kx0, ksy, ksx;
  int sub, sub_cy, sub_cx, Hc, Wc;  // stride-2 dgrad: this launch covers input pixels (2*py + sub_cy, 2*px + sub_cx) only
  const float* bias;
  const float* scale;
  const float* shift;
  const float* residual;
  long res_pitch;
  const unsigned char* res_mask;   // data gradient, fp32 staged epilogue only, or null: `residual` enters masked -- one byte per float4 group of C, dense [M][Nn / 4] (pm_bn_apply_mask's
                                   // layout), bit e set = element e of the group is added, clear = it counts as 0 (the skip gradient behind a ReLU, never stored masked)
  int relu;
  float* stats;               // train-mode BN statistics of the output: (mean, M2) per 32-row slab and channel, or null
  int io16;                   // the bf16 tier: C and `residual` are bf16 tensors (pitches in elements); accumulation and the epilogue arithmetic stay fp32
  int stage_ep;               // 1: epilogue staged through LDS (16-byte row stores); 0: per-element stores (batched launches)
  int n_group;                // > 0: N tiles are walked in groups of n_group columns (tile order inside a group: M outer, N inner), so that one XCD's co-resident
                              // blocks cover a squarer patch of the output and the weight columns of the group stay in that XCD's L2 over the whole sweep of M
  int batch_xcd;              // 1: gridDim.y >= 8 batches are dealt to the XCDs whole (igemm_tile_map); set by the launcher when the counts divide
  int spl_prio;               // PREC 5: 1 = waves in odd hardware wave slots run at s_setprio 2 (see the kernel), 0 = all equal
};

namespace {

enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };
constexpr int BK = 32;
constexpr int LDK = 36;  // k-contiguous LDS row stride (floats): 144 B rows -> conflict-free ds_read_b128
constexpr int LD5 = 52;  // PREC 5, floats per k-contiguous row: [hi | mid | lo] x 32 k x 2 B + 16 B -> 13 sixteen-byte granules per row: conflict-free ds_read_b128

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int OOB = 0x7fffffff;  // any byte offset beyond num_records makes a raw buffer load return zeros

// 16-byte load through a buffer descriptor: out-of-range lanes read 0 without a branch (padding taps, tile edges),
// and the address is a 32-bit byte offset (half the VALU work of 64-bit pointer arithmetic).
__device__ __forceinline__ v4f bload(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

// four fp32 -> four bf16 (RNE), 8 bytes
__device__ __forceinline__ uint2 pack4(const v4f& v) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  bf16x4 o;
  o[0] = (__bf16)v.x, o[1] = (__bf16)v.y, o[2] = (__bf16)v.z, o[3] = (__bf16)v.w;
  return __builtin_bit_cast(uint2, o);
}
// four fp32 -> 3 x four bf16 by truncation: hi = x & 0xffff0000, r = x - hi (exact), mid = r & 0xffff0000, lo = r - mid (exact: at most eight significant bits are
// left), so x == hi + mid + lo exactly. 16 VALU + 6 v_perm_b32.
__device__ __forceinline__ void split4(const v4f& v, uint2& hi, uint2& mid, uint2& lo) {
  const unsigned u0 = __float_as_uint(v.x), u1 = __float_as_uint(v.y), u2 = __float_as_uint(v.z), u3 = __float_as_uint(v.w);
  hi.x = __builtin_amdgcn_perm(u1, u0, 0x07060302), hi.y = __builtin_amdgcn_perm(u3, u2, 0x07060302);
  const float r0 = v.x - __uint_as_float(u0 & 0xffff0000u), r1 = v.y - __uint_as_float(u1 & 0xffff0000u);
  const float r2 = v.z - __uint_as_float(u2 & 0xffff0000u), r3 = v.w - __uint_as_float(u3 & 0xffff0000u);
  const unsigned q0 = __float_as_uint(r0), q1 = __float_as_uint(r1), q2 = __float_as_uint(r2), q3 = __float_as_uint(r3);
  mid.x = __builtin_amdgcn_perm(q1, q0, 0x07060302), mid.y = __builtin_amdgcn_perm(q3, q2, 0x07060302);
  const float s0 = r0 - __uint_as_float(q0 & 0xffff0000u), s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
  const float s2 = r2 - __uint_as_float(q2 & 0xffff0000u), s3 = r3 - __uint_as_float(q3 & 0xffff0000u);
  lo.x = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302);
  lo.y = __builtin_amdgcn_perm(__float_as_uint(s3), __float_as_uint(s2), 0x07060302);
}

// ---- tile map -------------------------------------------------------------------------------------------------------------------------------------------------
// Linear workgroup id -> (tile_m, tile_n) of batch `by`, K slice `z`.
// Batched / split-K launches (the 36 / 16 point GEMMs of a Winograd layer; the K slices of a weight gradient) with a.batch_xcd: whole (batch, K-slice) units go to one
// XCD (unit u -> XCD u mod 8; a remainder of 1 / 2 / 4 units is cut into 8 / 4 / 2 runs of tiles), so that both operands of a unit pass through ONE L2 instead of the
// weight tile of a point (the activation rows of a K slice) being fetched by every XCD that holds a few of its tiles. The linear workgroup id is dealt round-robin to
// the XCDs (MI355X_MICROARCH.md "Workgroup dispatch"); a wrong guess costs locality only. a.n_group: see ConvK.
__device__ __forceinline__ void igemm_tile_map(const ConvK& a, int ntile, int& tile_m, int& tile_n, int& by, int& z) {
  int lid;
  if (a.batch_xcd) {
    const int L = blockIdx.x + ntile * (blockIdx.y + gridDim.y * blockIdx.z), xcd = L & 7, idx = L >> 3;
    const int units = (int)(gridDim.y * gridDim.z), whole = units >> 3, rem = units & 7;
    int u;
    if (idx < whole * ntile) {
      u = xcd + 8 * (idx / ntile), lid = idx % ntile;
    } else {
      const int share = 8 / rem, per = ntile / share;
      u = whole * 8 + xcd / share, lid = (xcd % share) * per + (idx - whole * ntile);
    }
    by = u % (int)gridDim.y, z = u / (int)gridDim.y;
  } else {
    lid = pm_xcd_remap(blockIdx.x, ntile), by = blockIdx.y, z = blockIdx.z;
  }
  if (a.n_group > 0 && a.tiles_n > a.n_group) {
    const int gsz = a.tiles_m * a.n_group, grp = lid / gsz, rem = lid - grp * gsz;
    const int gw = min(a.n_group, a.tiles_n - grp * a.n_group);      // the last group may be narrower
    tile_m = rem / gw, tile_n = grp * a.n_group + rem % gw;
  } else {
    tile_m = lid / a.tiles_n, tile_n = lid % a.tiles_n;
  }
}

// ---- LDS layouts ----------------------------------------------------------------------------------------------------------------------------------------------
// One operand tile of EXT rows (m: BM for A, BN for B) x one K-step, as one thread stores it and one lane reads its MFMA fragments back. Thread -> tile element mapping
// (256 threads, g = t & 7, r = t >> 3):
//   k-contiguous tiles [rows][LDK / LD5]: the thread owns k-group g (4 floats) of rows r + 32 * i
//   m-contiguous tiles [BK][cols]       : the thread owns k-row r, column groups (g + 8 * i) * 4 (eight columns with native bf16 rows)
// Every layout gives FLOATS (LDS floats of the tile) and store(T, r, g, i, value); the bf16 layouts give their fragment read (the fp32 ones are read in the kernel's K-group multiply).

// fp32 rows, k contiguous: [EXT][LDK]
template <int EXT>
struct LdsRows {
  static constexpr int FLOATS = EXT * LDK;
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const v4f& v) { *reinterpret_cast<v4f*>(T + (r + 32 * i) * LDK + g * 4) = v; }
};
// fp32, m contiguous: [BK][EXT]
template <int EXT>
struct LdsCols {
  static constexpr int FLOATS = BK * EXT;
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const v4f& v) { *reinterpret_cast<v4f*>(T + r * EXT + (g + 8 * i) * 4) = v; }
};
// bf16, m contiguous, behind the hardware transpose read: [KROWS][EXT + 32]. The 32-element pad puts the four k-rows one read touches on four disjoint bank quarters
// (row stride = 64 B mod 256 B). The weight gradient's tiles of PREC 3 (fp32 rows rounded once, as they are stored) and PREC 4 (native bf16 rows, stored as they are,
// KROWS = 64), and each of the three planes of a PREC 5 m-contiguous operand.
template <int EXT, int KROWS = BK>
struct LdsT16 {
  static constexpr int LD = EXT + 32;      // bf16 elements per k-row
  static constexpr int FLOATS = KROWS * LD / 2;
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const uint2& v) { *reinterpret_cast<uint2*>(reinterpret_cast<char*>(T) + (r * LD + (g + 8 * i) * 4) * 2) = v; }
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const v4f& v) { *reinterpret_cast<v4f*>(reinterpret_cast<char*>(T) + (r * LD + (g + 8 * i) * 8) * 2) = v; }
  // Fragment through ds_read_b64_tr_b16: within a 16-lane group lane i hands in the address of row (i >> 2), column block (i & 3) * 4 and receives column i of those
  // four rows (tools/micro/tr_probe.hip) -- four consecutive k of its own m. Two reads = the lane's eight k of v_mfma_f32_32x32x16_bf16 (lanes 32..63: the upper
  // eight k of the 16-k block). krow = 16-k block * 16 + half * 8 + ((lane & 15) >> 2); col = the 32-column MFMA tile + ((lane >> 4) & 1) * 16 + (lane & 3) * 4.
  static __device__ __forceinline__ bf16x8 frag(const float* T, int krow, int col) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const short* base = reinterpret_cast<const short*>(T) + krow * LD + col;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * LD));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
};
// PREC 5, k contiguous: rows of three 64-byte bf16 planes [hi | mid | lo] + 16 B: [EXT][LD5]
template <int EXT>
struct LdsRows5 {
  static constexpr int FLOATS = EXT * LD5;
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const uint2* s) {
    float* d = T + (r + 32 * i) * LD5 + g * 2;
    *reinterpret_cast<uint2*>(d) = s[0], *reinterpret_cast<uint2*>(d + 16) = s[1], *reinterpret_cast<uint2*>(d + 32) = s[2];
  }
  // plane p, this lane-half's eight k at float offset kk of the 64-byte plane row
  static __device__ __forceinline__ bf16x8 frag(const float* T, int p, int row, int kk, int, int) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const v4f*>(T + row * LD5 + p * 16 + kk)); }
};
// PREC 5, m contiguous: three LdsT16 planes
template <int EXT>
struct LdsPlanes5 {
  static constexpr int PLANE = LdsT16<EXT>::FLOATS;
  static constexpr int FLOATS = 3 * PLANE;
  static __device__ __forceinline__ void store(float* T, int r, int g, int i, const uint2* s) {
    LdsT16<EXT>::store(T, r, g, i, s[0]), LdsT16<EXT>::store(T + PLANE, r, g, i, s[1]), LdsT16<EXT>::store(T + 2 * PLANE, r, g, i, s[2]);
  }
  static __device__ __forceinline__ bf16x8 frag(const float* T, int p, int, int, int krow, int col) { return LdsT16<EXT>::frag(T + p * PLANE, krow, col); }
};
// the layout of one operand: KC = k contiguous (A of forward / data gradient, B of forward)
template <int PREC, bool KC, int EXT>
using LdsTile = std::conditional_t<PREC == 5, std::conditional_t<KC, LdsRows5<EXT>, LdsPlanes5<EXT>>,
                                   std::conditional_t<KC, LdsRows<EXT>, std::conditional_t<PREC == 3, LdsT16<EXT>, std::conditional_t<PREC == 4, LdsT16<EXT, 2 * BK>, LdsCols<EXT>>>>>;

// One operand's gathered registers -> its LDS tile (PREC 0 - 4; PREC 5 stores its split pieces through LdsTile::store directly). N16: 16-byte gathers per thread and
// pixel row; PREC 4 holds two pixel rows (r, r + 32) per thread, 16 bytes = eight channels per gather, stored as they are.
template <int PREC, bool KC, int EXT, int N16>
__device__ __forceinline__ void lds_store_operand(float* T, int r, int g, const v4f* regs) {
  using Lay = LdsTile<PREC, KC, EXT>;
#pragma unroll
  for (int kk = 0; kk < (PREC == 4 ? 2 : 1); ++kk)
#pragma unroll
    for (int i = 0; i < N16; ++i) {
      if constexpr (PREC == 3 && !KC) Lay::store(T, r, g, i, pack4(regs[i]));
      else Lay::store(T, r + 32 * kk, g, i, regs[kk * N16 + i]);
    }
}

// ---- epilogues ------------------------------------------------------------------------------------------------------------------------------------------------
// v = (acc + bias) * scale + shift (+ residual) (ReLU), in fp32; T = float or pm_bf16: the element type of C and the residual (pitches in elements).
// The MFMA's native C layout: register q of lane (l31, half) of a 32 x 32 tile is column l31, row (q & 3) + 8 * (q >> 2) + 4 * half.

// Staged form (every 16-byte-aligned output): each wave parks 32 rows of its tile in LDS (the A / B stages are dead by now) and stores WHOLE row segments --
// (BN / WN) / V lanes per row, 16 bytes = V elements per lane, full 128-byte lines -- instead of 16 element stores per MFMA tile and lane. A finished tile is bound by
// the ISSUE of its stores, not by bandwidth: 64 -> 16 store instructions per lane and 128 x 128 fp32 tile (tools/micro/gemm_lab.hip: +4 ... +18 % on the store-heavy
// shapes, never slower). The fused epilogue operands are read as 16-byte vectors of the same row segments; values and their evaluation order are those of the
// per-element form. MASKED (fp32 data gradients): a.res_mask, if set, gates the residual per element. STATS: the BatchNorm statistics of each 32-row slab, taken
// while it is parked (bf16: pm_slab_stats16 of pm_common.h; fp32: written out below) -- the epilogue is then the convolution plus at most a bias.
template <typename T, bool MASKED, bool STATS, int BM, int BN, int WM, int WN, int TM, int TN>
__device__ __forceinline__ void igemm_epilogue_staged(const ConvK& a, T* C, const T* R, float* smem, const f32x16 (&acc)[TM][TN], int m0, int n0, int wm, int wn, int wave, int lane,
                                                      int l31, int half, bool aff, bool res, bool relu) {
  constexpr int V = pm_elem<T>::V;
  constexpr int WC = BN / WN, LDC = WC + 4, LPR = WC / V, RPI = 64 / LPR;   // columns per wave, padded pitch, lanes per row, rows per instruction
  static_assert(32 % RPI == 0, "row segments must tile the 32-row slab");
  __syncthreads();                                  // every wave is done reading the last K-slab
  float* Ws = smem + wave * 32 * LDC;
  const int rr0 = lane / LPR, cc = (lane % LPR) * V;
  const int col = n0 + wn * WC + cc;
  const bool cok = col < a.Nn;                      // Nn % V == 0: the group is all in or all out
  float bi[V], sc[V], sh[V];
#pragma unroll
  for (int e = 0; e < V; ++e) bi[e] = 0.f, sc[e] = 1.f, sh[e] = 0.f;
  if (aff && cok) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (a.bias) bi[e] = a.bias[col + e];
      if (a.scale) sc[e] = a.scale[col + e], sh[e] = a.shift[col + e];
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int q = 0; q < 16; ++q) Ws[((q & 3) + 8 * (q >> 2) + 4 * half) * LDC + n * 32 + l31] = acc[i][n][q];
#pragma unroll
    for (int r0 = 0; r0 < 32; r0 += RPI) {
      const int rr = r0 + rr0;
      const long row = m0 + wm * (BM / WM) + i * 32 + rr;
      float v[V];
      pm_ldp<V>(Ws + rr * LDC + cc, v);
      if (row < a.M && cok) {
        if (aff) {
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] = (v[e] + bi[e]) * sc[e] + sh[e];
        }
        if (res) {
          float q[V];
          pm_elem<T>::ld(R + row * a.res_pitch + col, q);
          if constexpr (MASKED) if (a.res_mask) {      // (data gradients only: the forward instantiations keep their register allocation)
            const unsigned mb = a.res_mask[row * (a.Nn >> 2) + (col >> 2)];
#pragma unroll
            for (int e = 0; e < V; ++e) q[e] = (mb & (1u << e)) ? q[e] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] += q[e];
        }
        if (relu) {
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        pm_elem<T>::st(C + row * a.c_pitch + col, v);
      }
    }
    if constexpr (STATS && V == 8) {
      if (a.stats) pm_slab_stats16<LDC, LPR, RPI>(Ws, rr0, cc, (long)m0 + wm * (BM / WM) + i * 32, a.M, a.Nn, col, cok, bi, sc, sh, a.stats);
    } else if constexpr (STATS) {      // (the fp32 form never tested a.stats: launch_nst / launch_split pick a STATS instantiation only where k.stats is set)
      // pm_slab_stats16's fp32 sibling: four columns per lane, nothing rounded; the same two passes over the parked slab, exchange order and output layout. Written
      // out here on float4 components: behind a function of pm_slab_stats16's shape (and as one template over the lane width) it cost the 64 x 128 split-operand
      // forward kernel two VGPRs and with them the step from 4 to 3 waves per SIMD (profiles/igemm_resource_usage.txt).
      const long slab_row0 = m0 + wm * (BM / WM) + i * 32;
      const float cnt = (float)max(0l, min(32l, (long)a.M - slab_row0));
      auto slab_row = [&](int r0, bool& rok) {
        float4 v = *reinterpret_cast<const float4*>(Ws + (r0 + rr0) * LDC + cc);
        v.x = (v.x + bi[0]) * sc[0] + sh[0], v.y = (v.y + bi[1]) * sc[1] + sh[1], v.z = (v.z + bi[2]) * sc[2] + sh[2], v.w = (v.w + bi[3]) * sc[3] + sh[3];
        rok = slab_row0 + r0 + rr0 < a.M;
        return v;
      };
      float s1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += RPI) {
        bool rok;
        const float4 v = slab_row(r0, rok);
        s1[0] += rok ? v.x : 0.f, s1[1] += rok ? v.y : 0.f, s1[2] += rok ? v.z : 0.f, s1[3] += rok ? v.w : 0.f;
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[e] += __shfl_xor(s1[e], o, 64);
      float mu[4], m2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) mu[e] = cnt > 0.f ? s1[e] / cnt : 0.f;
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += RPI) {
        bool rok;
        const float4 v = slab_row(r0, rok);
        const float d0 = v.x - mu[0], d1 = v.y - mu[1], d2 = v.z - mu[2], d3 = v.w - mu[3];
        m2[0] += rok ? d0 * d0 : 0.f, m2[1] += rok ? d1 * d1 : 0.f, m2[2] += rok ? d2 * d2 : 0.f, m2[3] += rok ? d3 * d3 : 0.f;
      }
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) m2[e] += __shfl_xor(m2[e], o, 64);
      if (rr0 == 0 && cok && cnt > 0.f) {
        float* dst = a.stats + ((slab_row0 >> 5) * (long)a.Nn + col) * 2;
        PM_ST4(dst, make_float4(mu[0], m2[0], mu[1], m2[1]));
        PM_ST4(dst + 4, make_float4(mu[2], m2[2], mu[3], m2[3]));
      }
    }
  }
}

// Per-element form: batched launches (the Winograd products stay in L2 for the output transform), outputs that are not 16-byte aligned row segments (the 19 class
// logits; a bf16 residual that is a channel slice off a 16-byte boundary). A lane holds one output column and 16 rows of it. EDGE: the tile crosses M or Nn, every
// element is predicated. The callers pass aff / res / relu as constants where the (wave-uniform) operations are known: the interior form is straight-line code.
template <typename T, bool EDGE, int TM, int TN>
__device__ __forceinline__ void igemm_epilogue_elems(const ConvK& a, T* C, const T* R, const f32x16 (&acc)[TM][TN], int rbase, int cbase, bool aff, bool res, bool relu) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      const int col = cbase + n * 32;
      const bool cok = !EDGE || col < a.Nn;
      float bi = 0.f, sc = 1.f, sh = 0.f;
      if (aff && cok) {
        if (a.bias) bi = a.bias[col];
        if (a.scale) sc = a.scale[col], sh = a.shift[col];
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const long row = rbase + i * 32 + (q & 3) + 8 * (q >> 2);
        if (!EDGE || (row < a.M && cok)) {
          float v = acc[i][n][q];
          if (aff) v = (v + bi) * sc + sh;
          if (res) v += pm_elem<T>::widen(R[row * a.res_pitch + col]);
          if (relu) v = fmaxf(v, 0.f);
          C[row * a.c_pitch + col] = pm_elem<T>::narrow(v);
        }
      }
    }
}

}  // namespace
