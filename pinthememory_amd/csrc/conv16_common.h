// What the bf16 LDS-DMA convolution kernels share (conv16.hip: the tile kernel in its narrow and wide forms; conv16w.hip: the persistent producer / consumer form;
// wgrad16.hip: the weight gradient on the same ring), each once: the LDS-DMA primitives, the rule for filter rows no row of a tile can see, the tap / channel
// K-state, the A / B row fetch offsets, the fragment reads + MFMA K-step, the two staged epilogues and the persistent ring protocol.
#pragma once
#include "pm_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int C16_BKB = 128;             // bytes per row and K-step (64 bf16)
constexpr int C16_OOB = 0x7fffffff;      // a fetch offset beyond every descriptor's range: the fetch delivers zeros

// ---- primitives -------------------------------------------------------------------------------------------------------------------------------------------------
// one 16-byte LDS-DMA fetch through a buffer descriptor: lane l of the wave lands at dst + 16 l (dst wave-uniform -> m0), out-of-range offsets deliver zeros.
// (A __device__ function of its own: with the builtin written into the kernel template the host pass silently drops the kernel's stub -- ROCm 7.2.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// s_waitcnt vmcnt(n) only (expcnt / lgkmcnt untouched): gfx9 encoding vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[15:14]
template <int N>
__device__ __forceinline__ void wait_vm() {
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// a bare s_barrier the compiler moves nothing across. No __syncthreads(): its fence would drain the DMA queue (vmcnt(0)) at every K-step.
__device__ __forceinline__ void ring_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Stores the compiler's wait bookkeeping does not see. Beside LDS-DMA hipcc puts s_waitcnt vmcnt(0) in front of an LDS read while ANY vector-memory operation of
// the wave is pending: with ordinary stores the first fragment read of the NEXT tile waits until this tile's output has been acknowledged by L2 (1-2 us per tile).
// Nothing reads these addresses again inside the kernel, and a wave's stores complete whatever it does next.
__device__ __forceinline__ void st16_untracked(void* p, u32x4 q) { asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(q) : "memory"); }
__device__ __forceinline__ void st4_untracked(float* p, float v) { asm volatile("global_store_dword %0, %1, off" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st8_bf16_untracked(pm_bf16* p, const float* v) {
  u32x4 q;
  q.x = pm_pack_bf16(v[0], v[1]), q.y = pm_pack_bf16(v[2], v[3]), q.z = pm_pack_bf16(v[4], v[5]), q.w = pm_pack_bf16(v[6], v[7]);
  st16_untracked(p, q);
}

// ---- visible filter rows ----------------------------------------------------------------------------------------------------------------------------------------
// 1x1 / stride 1 / no padding: output pixel m reads input pixel m
__host__ __device__ inline bool c16_pointwise(const pm_conv16& a) { return a.kh * a.kw == 1 && a.stride == 1 && a.pad == 0 && a.Ho == a.H && a.Wo == a.W; }

// Taps no row of a tile can see (round 5): a tile of bm output pixels from m0 on covers image rows oy_a ... oy_b of ONE image (else: no skipping); a filter row ky whose
// input rows oy * stride - pad + ky * dil lie outside the image for all of them contributes zeros only -- its K-steps are neither staged nor multiplied. On the
// 48 x 48 maps the dilated ASPP branches (rates 6 / 12 / 18, deepv3plus.py:58-81) lose 8 / 17 / 25 % of their K-steps this way, nothing else is affected.
// -> ky_ok, bit ky set: filter row ky is visible; ~0u: every filter row is (all interior tiles): no skipping, none of its per-tap bookkeeping, no K-step recount.
// (The mask is written through the reference, into the caller's own variable, and the function has one exit: returned by value from early exits it cost the
//  persistent kernel, which sits at the scalar-register limit, 75 instead of 8 SGPRs spilled to VGPR lanes per instantiation and 2 - 4 % of its speed.)
__host__ __device__ inline void c16_visible_rows(const pm_conv16& a, bool pointwise, int m0, int bm, unsigned& ky_ok) {
  ky_ok = ~0u;
  if (!pointwise && a.kh > 1) {
    const int hw = a.Ho * a.Wo, ml = (m0 + bm < a.M ? m0 + bm : a.M) - 1;
    const int ia = m0 / hw, ib = ml / hw;
    if (ia == ib) {
      const int oy_a = (m0 - ia * hw) / a.Wo, oy_b = (ml - ib * hw) / a.Wo;
      ky_ok = 0;
      for (int ky = 0; ky < a.kh; ++ky)
        if (oy_b * a.stride - a.pad + ky * a.dil >= 0 && oy_a * a.stride - a.pad + ky * a.dil < a.H) ky_ok |= 1u << ky;
    }
  }
  if (ky_ok == (1u << a.kh) - 1u) ky_ok = ~0u;
}
// K-steps of the range [kt0, kt0 + nk) that are really run under a mask: the range minus the chunks of invisible taps
__host__ __device__ inline int c16_ksteps(const pm_conv16& a, unsigned ky_ok, int kt0, int nk) {
  if (ky_ok == ~0u) return nk;
  const int cpc = a.Cp >> 6;
  int n = 0;
  for (int kt = kt0; kt < kt0 + nk;) {
    const int tap = kt / cpc, end = (tap + 1) * cpc, run = (kt0 + nk < end ? kt0 + nk : end) - kt;
    if ((ky_ok >> (tap / a.kw)) & 1u) n += run;
    kt += run;
  }
  return n;
}

// One unit of work: output tile (m0, n0) x K-split z = K-steps [kt0, kt0 + nk), of which `steps` are run under ky_ok. A block of the tile kernel has one; a block of
// the persistent kernel walks units v = blockIdx.x, + gridDim.x, ..., and its producer and consumer waves BOTH take a unit's step count from this one function.
struct c16_unit {
  int m0, n0, z, kt0, nk, steps;
  unsigned ky_ok;
};
template <int BM, int BN>
__device__ __forceinline__ c16_unit c16_open_unit(const pm_conv16& a, bool pointwise, int bid, int z) {
  c16_unit u;
  const int lid = pm_xcd_remap(bid, a.tiles_m * a.tiles_n);
  u.m0 = (lid / a.tiles_n) * BM, u.n0 = (lid % a.tiles_n) * BN;
  u.z = z, u.kt0 = z * a.ksteps_per, u.nk = min(a.ksteps - u.kt0, a.ksteps_per);
  c16_visible_rows(a, pointwise, u.m0, BM, u.ky_ok);
  u.ky_ok = __builtin_amdgcn_readfirstlane(u.ky_ok);
  u.steps = __builtin_amdgcn_readfirstlane(c16_ksteps(a, u.ky_ok, u.kt0, u.nk));
  return u;
}

// ---- the wave-uniform K-state: (filter row, filter column, 64-channel chunk) of the next K-step to stage, on the scalar unit -----------------------------------
struct c16_kstate {
  int ch, ky, kx, kb;      // kb: byte offset of the K-step inside a weight row (scalar offset of the B fetches)
  int cpc, kh, kw;         // 64-channel chunks per tap, filter extent
  unsigned ky_ok;
  // move past invisible taps (whole taps: the state sits at a tap start, or at the unit's first K-step)
  __device__ __forceinline__ void skip() {
    while (ky < kh && !((ky_ok >> ky) & 1u)) {
      kb += (cpc - ch) * C16_BKB;
      ch = 0;
      if (++kx == kw) kx = 0, ++ky;
    }
  }
  __device__ __forceinline__ void open(const pm_conv16& a, const c16_unit& u) {
    cpc = a.Cp >> 6, kh = a.kh, kw = a.kw, ky_ok = u.ky_ok;
    const int tap = u.kt0 / cpc;
    ch = __builtin_amdgcn_readfirstlane(u.kt0 - tap * cpc);
    ky = __builtin_amdgcn_readfirstlane(tap / kw);
    kx = __builtin_amdgcn_readfirstlane(tap - ky * kw);
    kb = u.kt0 * C16_BKB;
    if (ky_ok != ~0u) skip();
  }
  // one K-step on; true when the state entered a new tap (what a caller keeps per tap -- border tests, pixel offsets -- is stale)
  __device__ __forceinline__ bool advance() {
    kb += C16_BKB;
    if (++ch != cpc) return false;
    ch = 0;
    if (++kx == kw) kx = 0, ++ky;
    if (ky_ok != ~0u) skip();
    return true;
  }
};

// ---- per-lane fetch offsets: this lane's rows of the A and B tiles and the (swizzled) 16-byte chunk it fetches of each ------------------------------------------
// Addressing (round 4, second form): both operands are fetched through BUFFER descriptors -- a 32-bit byte offset per lane, and a lane that must read zeros
// (padding tap, row beyond M, column beyond N) simply presents an offset beyond the descriptor's range: the fetch returns 0 into LDS. The first form built a
// 64-bit source pointer per fetch and selected a zero page for such lanes: 59 VALU + 56 SALU instructions per wave and K-step around 8 MFMAs.
// FT fetching threads sweep FT / 8 rows x 8 chunks; piece `it` of thread t is row it * FT / 8 + (t >> 3) of the tile.
template <int FT, int BM>
struct c16_a_rows {
  static constexpr int IT = BM * 8 / FT, RSTEP = FT / 8;
  int off[IT], y0[IT], x0[IT];      // byte offset and input coordinates of the row's pixel at tap (0, 0)

  __device__ __forceinline__ void row(const pm_conv16& a, bool pointwise, long pitchb, int it, int m, int ch, int img, int oy, int ox) {
    if (m < a.M && pointwise) {      // output pixel m reads input pixel m -- no index decomposition
      y0[it] = x0[it] = 0;
      off[it] = (int)((long)m * pitchb) + ch * 16;
    } else if (m < a.M) {
      y0[it] = oy * a.stride - a.pad, x0[it] = ox * a.stride - a.pad;
      off[it] = (int)(((long)(img * a.H + y0[it]) * a.W + x0[it]) * pitchb) + ch * 16;      // may be negative at the image border: only used with an in-range tap added
    } else {
      y0[it] = x0[it] = -(1 << 28);      // never inside the image: the row reads zeros
      off[it] = 0;
    }
  }
  // every piece decomposes its own row index (two integer divisions per row): the tile kernel, once per block
  __device__ __forceinline__ void direct(const pm_conv16& a, bool pointwise, long pitchb, int m0, int t) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = it * RSTEP + (t >> 3), ch = (t & 7) ^ ((r >> 1) & 7), m = m0 + r;
      int img = 0, oy = 0, ox = 0;
      if (!pointwise && m < a.M) {
        img = m / (a.Ho * a.Wo);
        const int rem = m - img * (a.Ho * a.Wo);
        oy = rem / a.Wo, ox = rem - oy * a.Wo;
      }
      row(a, pointwise, pitchb, it, m, ch, img, oy, ox);
    }
  }
  // ONE index decomposition, the other pieces step on from it by RSTEP pixels: the persistent producer, once per unit beside the fetches in flight
  __device__ __forceinline__ void stepped(const pm_conv16& a, bool pointwise, long pitchb, int m0, int t) {
    int m = m0 + (t >> 3), img = 0, oy = 0, ox = 0;
    if (!pointwise) {
      img = m / (a.Ho * a.Wo);
      const int rem = m - img * (a.Ho * a.Wo);
      oy = rem / a.Wo, ox = rem - oy * a.Wo;
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = it * RSTEP + (t >> 3), ch = (t & 7) ^ ((r >> 1) & 7);
      row(a, pointwise, pitchb, it, m, ch, img, oy, ox);
      m += RSTEP;
      if (!pointwise) {
        ox += RSTEP;
        while (ox >= a.Wo) {
          ox -= a.Wo;
          if (++oy == a.Ho) oy = 0, ++img;
        }
      }
    }
  }
  // the fetch offset of piece `it` at the tap displaced by (dy, dx) pixels = toff bytes, or out of range where the tap falls into the padding
  __device__ __forceinline__ int at(const pm_conv16& a, int it, int dy, int dx, int toff) const {
    const bool ok = ((unsigned)(y0[it] + dy) < (unsigned)a.H) & ((unsigned)(x0[it] + dx) < (unsigned)a.W);
    return ok ? off[it] + toff : C16_OOB;
  }
};
template <int FT, int BN>
__device__ __forceinline__ void c16_b_rows(const pm_conv16& a, int n0, int t, int (&boff)[BN * 8 / FT]) {
#pragma unroll
  for (int it = 0; it < BN * 8 / FT; ++it) {
    const int u = it * FT + t, row = u >> 3, ch = (u & 7) ^ ((row >> 1) & 7);
    const int n = n0 + row;
    boff[it] = n < a.Nn ? n * a.K * 2 + ch * 16 : C16_OOB;
  }
}

// ---- fragment reads + MFMAs of one 64-k stage ---------------------------------------------------------------------------------------------------------------------
// A lane's fragment rows and their swizzle keys are K-step invariant: byte offsets inside a stage ([BM rows][128 B] of A, then [BN rows][128 B] of B), one per
// 16-k group through the XOR. Wave (wm, wn) of WM x WN owns TM x TN blocks of v_mfma_f32_32x32x16_bf16.
template <int BM, int BN, int WM, int WN>
struct c16_frags {
  static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  static_assert(TM >= 1 && TN >= 1, "bad tile config");
  int ra_off[TM], ra_key[TM], rb_off[TN], rb_key[TN], half;

  __device__ __forceinline__ void init(int wm, int wn, int lane) {
    const int l31 = lane & 31;
    half = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int ra = wm * (BM / WM) + i * 32 + l31;
      ra_off[i] = ra * C16_BKB, ra_key[i] = (ra >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int rb = wn * (BN / WN) + j * 32 + l31;
      rb_off[j] = BM * C16_BKB + rb * C16_BKB, rb_key[j] = (rb >> 1) & 7;
    }
  }
  __device__ __forceinline__ void step(const char* ls, f32x16 (&acc)[TM][TN]) const {
    // (Measured and removed: all 16 fragment reads of the K-step issued ahead of the 16 MFMAs behind a sched_barrier -- 194 instead of 126 VGPRs, 9 % slower on
    //  every shape, two alternated runs: 828-833 -> 743-764 TF on the decoder's 3x3s. The compiler's read / MFMA pairing with two waves per SIMD is the better schedule.)
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) {
      const int c = kg * 2 + half;      // this lane-half's eight k of the 16-k block
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(ls + ra_off[i] + ((c ^ ra_key[i]) << 4));
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(ls + rb_off[j] + ((c ^ rb_key[j]) << 4));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
};

template <int TM, int TN>
__device__ __forceinline__ void c16_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// ---- epilogues: a wave parks 32-row slabs of its TM x TN accumulator blocks in LDS (Ws: the wave's own 32 x (SW + 4) floats) and stores whole row segments ------
// Slab geometry: SW = the wave's whole width (one slab per 32 rows: the tile kernel, whose stages are dead by then) or 32 (one slab per accumulator block, column
// block outermost: the persistent kernels, whose eight slabs fit the ring slot read last). UT: untracked stores (the persistent kernels).
// The MFMA layout: element q of lane (l31, half) of a block is row (q & 3) + 8 (q >> 2) + 4 half, column l31.
template <int TN, int SW, int LDC>
__device__ __forceinline__ void c16_park(float* Ws, const f32x16 (&acc)[TN], int s, int l31, int half) {
#pragma unroll
  for (int n = 0; n < SW / 32; ++n)
#pragma unroll
    for (int q = 0; q < 16; ++q) Ws[((q & 3) + 8 * (q >> 2) + 4 * half) * LDC + n * 32 + l31] = acc[s * (SW / 32) + n][q];
}

// fp32 rows: split-K slabs (no epilogue arithmetic) or the class logits (bias only; 19 columns at pitch 20: per-element stores). Rows from row0 on below M, columns
// from col0 on below `lim`, at Cf[row * cp + col].
template <int TM, int TN, int SW, bool UT>
__device__ __forceinline__ void c16_store_f32(float* Ws, const f32x16 (&acc)[TM][TN], int lane, int row0, int col0, float* Cf, long cp, int M, int lim,
                                              const float* bias, bool slab) {
  constexpr int LDC = SW + 4, LPR = SW / 4, RPI = 64 / LPR;
  const int l31 = lane & 31, half = lane >> 5, rr0 = lane / LPR, cc = (lane % LPR) * 4;
#pragma unroll
  for (int s = 0; s < TN * 32 / SW; ++s) {
    const int col = col0 + s * SW + cc;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      c16_park<TN, SW, LDC>(Ws, acc[i], s, l31, half);
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += RPI) {
        const int rr = r0 + rr0;
        const long row = row0 + i * 32 + rr;
        const float4 v = *reinterpret_cast<const float4*>(Ws + rr * LDC + cc);
        if (row >= M) continue;
        const float e[4] = {v.x, v.y, v.z, v.w};
        if (((cp | lim) & 3) == 0 && col + 4 <= lim && !bias) {
          if constexpr (UT) st16_untracked(Cf + row * cp + col, u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)});
          else PM_ST4(Cf + row * cp + col, v);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (col + k < lim) {
              const float o = e[k] + ((bias && !slab) ? bias[col + k] : 0.f);
              if constexpr (UT) st4_untracked(Cf + row * cp + col + k, o);
              else Cf[row * cp + col + k] = o;
            }
        }
      }
    }
  }
}

// bf16 rows, eight channels = 16 bytes per lane: (v + bias) * scale + shift, + residual, ReLU, round to nearest even. STATS (whole-width slabs only): the BatchNorm
// statistics of each 32-row slab (pm_slab_stats16) -- a separate instantiation: the kernels without statistics keep their register budget.
template <int TM, int TN, int SW, bool UT, bool STATS>
__device__ __forceinline__ void c16_store_bf16(float* Ws, const f32x16 (&acc)[TM][TN], int lane, int row0, int col0, const pm_conv16& a) {
  constexpr int LDC = SW + 4, NS = TN * 32 / SW, LPR = SW / 8, RPI = 64 / LPR;
  static_assert(32 % RPI == 0, "row segments must tile the 32-row slab");
  static_assert(!STATS || NS == 1, "statistics are taken over whole-width slabs");
  const int l31 = lane & 31, half = lane >> 5, rr0 = lane / LPR, cc = (lane % LPR) * 8;
  const bool aff = a.bias || a.scale, res = a.residual != nullptr, relu = a.relu != 0;
  pm_bf16* C16 = reinterpret_cast<pm_bf16*>(a.C);
  const pm_bf16* R16 = reinterpret_cast<const pm_bf16*>(a.residual);
  // the per-channel constants of ALL column groups are fetched before the first store of the tile: a register load issued behind a store would wait for it
  float bi[NS][8], sc[NS][8], sh[NS][8];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int col = col0 + s * SW + cc;
#pragma unroll
    for (int e = 0; e < 8; ++e) bi[s][e] = 0.f, sc[s][e] = 1.f, sh[s][e] = 0.f;
    if (aff && col < a.Nn) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (a.bias) bi[s][e] = a.bias[col + e];
        if (a.scale) sc[s][e] = a.scale[col + e], sh[s][e] = a.shift[col + e];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int col = col0 + s * SW + cc;
    const bool cok = col < a.Nn;      // Nn % 8 == 0: the group is all in or all out
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      c16_park<TN, SW, LDC>(Ws, acc[i], s, l31, half);
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += RPI) {
        const int rr = r0 + rr0;
        const long row = row0 + i * 32 + rr;
        const float4 v0 = *reinterpret_cast<const float4*>(Ws + rr * LDC + cc), v1 = *reinterpret_cast<const float4*>(Ws + rr * LDC + cc + 4);
        float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        if (row < a.M && cok) {
          if (aff) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (v[e] + bi[s][e]) * sc[s][e] + sh[s][e];
          }
          if (res) {
            float q[8];
            pm_ld8(R16 + row * a.res_pitch + col, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += q[e];
          }
          if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
          }
          if constexpr (UT) st8_bf16_untracked(C16 + row * a.c_pitch + col, v);
          else pm_st8(C16 + row * a.c_pitch + col, v);
        }
      }
      if constexpr (STATS) pm_slab_stats16<LDC, LPR, RPI>(Ws, rr0, cc, (long)row0 + i * 32, a.M, a.Nn, col, cok, bi[s], sc[s], sh[s], a.stats);
    }
  }
}

// ---- the persistent ring protocol (round 5, second session) -----------------------------------------------------------------------------------------------------
// One block per CU walks units v = first, first + G, ... < total; PRODUCER waves do nothing but issue the LDS-DMA fetches of a three-stage ring that runs on across
// unit boundaries, CONSUMER waves multiply the stages and write each unit out. Synchronisation is ONE s_barrier per K-step for all waves, plus one per unit in front
// of the epilogue (which parks accumulators in the ring slot that was read last -- the producers refill it only behind the NEXT step's barrier):
//   step g:  producers wait until their part of stage g has landed (counted vmcnt: the FETCH instructions of stage g + 1 stay in flight; LDS-DMA fetches of a wave
//            retire in order, so "my part has landed" + barrier = "stage g has landed") | barrier | producers issue stage g + 2 into the slot of stage g - 1,
//            consumers multiply stage g.
// Both sides take a unit's step count from the SAME call, open(v).steps, and walk the same units: steps + 1 barriers per unit on either side, a unit of zero steps
// (every tap invisible) included -- the producer's fetch sequence skips it, its barrier mirror does not.
//   open(v)   -> the unit (anything with .steps), pure;          load(unit): set the fetch state up for a unit with steps > 0;
//   fetch(ls) :  issue the fetches of the unit's next step into the stage at ls and move the fetch state one step on.
template <int FETCH, int STAGE, class Open, class Load, class Fetch>
__device__ __forceinline__ void c16_ring_produce(char* lds, int first, int total, int G, Open open, Load load, Fetch fetch) {
  int vf = first, left = 0, slot = 0;      // the unit being fetched (runs ahead of the unit being multiplied), its steps left, ring slot of the next stage
  auto open_next = [&]() {                 // fetch state of unit vf, or of the next one with something to fetch; left == 0 afterwards: no unit is left
    for (; vf < total; vf += G) {
      const auto u = open(vf);
      if (u.steps <= 0) continue;
      left = u.steps;
      load(u);
      return;
    }
    left = 0;
  };
  auto issue = [&]() -> int {      // one more stage of the flat (unit, K-step) sequence; 0 when the sequence is over
    if (left == 0) {
      if (vf >= total) return 0;
      vf += G;
      open_next();
      if (left == 0) return 0;
    }
    fetch(lds + slot * STAGE);
    --left;
    slot = slot == 2 ? 0 : slot + 1;
    return 1;
  };
  open_next();
  int ahead = issue();      // stages issued and not yet handed over
  ahead += issue();
  for (int vc = first; vc < total; vc += G) {      // mirror of the consumers' barrier sequence
    const int steps = open(vc).steps;
    for (int kt = 0; kt < steps; ++kt) {
      if (ahead >= 2) wait_vm<FETCH>();      // the oldest stage in flight has landed, the younger one may still fly
      else wait_vm<0>();
      ring_barrier();
      ahead += issue() - 1;
    }
    ring_barrier();      // the unit's epilogue barrier
  }
}
//   begin(unit): clear the accumulators;   multiply(ls): one stage;   finish(unit, slot): the epilogue through the ring slot read last.
template <int STAGE, class Open, class Begin, class Multiply, class Finish>
__device__ __forceinline__ void c16_ring_consume(char* lds, int first, int total, int G, Open open, Begin begin, Multiply multiply, Finish finish) {
  int rd = 0;      // ring slot of the next stage to multiply
  for (int vc = first; vc < total; vc += G) {
    const auto u = open(vc);
    begin(u);
    for (int kt = 0; kt < u.steps; ++kt) {
      ring_barrier();
      multiply(lds + rd * STAGE);
      rd = rd == 2 ? 0 : rd + 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ring_barrier();
    finish(u, lds + (rd == 0 ? 2 : rd - 1) * STAGE);      // free until the producers pass the next step's barrier
  }
}
