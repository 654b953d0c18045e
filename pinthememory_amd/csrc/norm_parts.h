// The parts BatchNorm (bn.hip) and InstanceNorm (instnorm.hip) are both put together from, each written once. BatchNorm is InstanceNorm with one image:
// the two reductions take the image index from the grid (BATCH) or fix it at zero, and index mean / invstd as [img][c].
//   * the mask helpers and the dx expression;
//   * the two-stage reduction: per-thread shifted sums over a pixel chunk -> block_reduce_store -> part[img][chunk][c][2] -> final_sums in double, in a fixed
//     order (no floating-point atomics: bit-identical from run to run and under graph replay), with the forward and the backward partial kernel;
//   * the elementwise driver: a thread owns one 16-byte channel group, keeps that group's per-(image, channel) constants in registers and strides over pixels
//     (FIXED), or walks (pixel, group) items and re-loads them; what a pass computes is a small functor.
// One body for fp32 and bf16 tensors: a lane moves 16 bytes (pm_elem<T>::V channels), values are widened to fp32 in registers and travel as float[V]; every
// statistic / accumulator is fp32 (second stages in double); bf16 results are rounded (nearest even) once, on the way out.
// Each module keeps its plan (block shape, chunking), its finish (what becomes of the sums) and its entry points.
#pragma once
#include <type_traits>

#include "pm_common.h"

namespace {

// ---- elementwise expressions ----------------------------------------------------------------------------------------------------------
// y = (x - mean) * invstd * gamma + beta, evaluated the same way in the forward pass and wherever the backward pass rebuilds the
// ReLU mask from x (two explicit FMAs: bit-identical in both places whatever the compiler would contract).
template <int V>
__device__ __forceinline__ void bn_affine(const float* v, const float* mu, const float* is, const float* ga, const float* be, float* o) {
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = pm_bn_affine(v[j], mu[j], is[j], ga[j], be[j]);
}
// the ReLU passes g where the activation o was positive (o: the forward output, or bn_affine of x)
template <int V>
__device__ __forceinline__ void relu_mask(const float* o, float* g) {
#pragma unroll
  for (int j = 0; j < V; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
}
// ... or where bit j of the byte bn_apply left for the group is set (positive_bits)
template <int V>
__device__ __forceinline__ void relu_mask_bits(unsigned mb, float* g) {
#pragma unroll
  for (int j = 0; j < V; ++j) g[j] = ((mb >> j) & 1u) ? g[j] : 0.f;
}
template <int V>
__device__ __forceinline__ unsigned positive_bits(const float* o) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < V; ++j) m |= o[j] > 0.f ? (1u << j) : 0u;
  return m;
}
template <int V>
__device__ __forceinline__ void relu(float* o) {
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = fmaxf(o[j], 0.f);
}
// dx = (g - sum(g) / n - xhat * sum(g xhat) / n) * invstd * gamma, with k1 = s1 * inv_n, k2 = s2 * inv_n, sg = is * ga -- hoisted by the caller or written in place.
// A macro: as a function the three products are evaluated before the rest, and that order alone costs the bf16 generic pass two VGPRs (64 against 62).
#define BN_DX(g, v, mu, is, k1, k2, sg) (((g) - (k1) - ((v) - (mu)) * (is) * (k2)) * (sg))

// ---- reductions -------------------------------------------------------------------------------------------------------------------------
// A block is GPR lane groups (of V channels) per pixel row x RL row lanes: lane r sums pixels p0 + r, p0 + r + RL, ... of the block's chunk; CB = GPR * V channels.
struct Plan {
  int gpr, rows, nb, colblocks;      // rows: pixels per chunk, nb: chunks per image
};
// launch(integral_constant<int, GPR>) for the plan's GPR; MIN_GPR 16: the plan never asks for 8 and no kernel is built for it
template <int MIN_GPR, typename L>
void with_gpr(int gpr, L launch) {
  if constexpr (MIN_GPR == 8) {
    if (gpr == 8) return launch(std::integral_constant<int, 8>{});
  }
  launch(std::integral_constant<int, 16>{});
}
// launch(true_type / false_type) for a run-time flag
template <typename L>
void with_flag(bool on, L launch) {
  if (on) return launch(std::true_type{});
  launch(std::false_type{});
}

// block-level reduce of per-thread (s1[V], s2[V]) over the row lanes, in row-lane order -> part[c][2] of this block's (image, chunk)
template <int V, int GPR, int RL>
__device__ __forceinline__ void block_reduce_store(const float* s1, const float* s2, int g, int r, int C, float* __restrict__ part) {
  constexpr int CB = GPR * V;
  __shared__ float sm[RL][CB][2];
#pragma unroll
  for (int j = 0; j < V; ++j) sm[r][g * V + j][0] = s1[j], sm[r][g * V + j][1] = s2[j];
  __syncthreads();
  if (threadIdx.x < CB * 2) {
    const int cc = threadIdx.x >> 1, w = threadIdx.x & 1;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RL; ++i) s += sm[i][cc][w];
    const int ch = blockIdx.y * CB + cc;
    if (ch < C) part[(long)ch * 2 + w] = s;
  }
}

// forward partials: part[img][chunk][c][2] = sum(x - K), sum((x - K)^2) over the chunk, K = the image's first pixel (shifted sums: no cancellation).
// BATCH: blockIdx.x = img * nb + chunk; else one image of HW pixels, blockIdx.x = chunk (no division in the kernel).
template <typename T, int GPR, int RL, bool BATCH>
__global__ __launch_bounds__(GPR* RL) void norm_stats_partial(const T* __restrict__ x, long pitch, long HW, int C, int rows, int nb, float* __restrict__ part) {
  constexpr int V = pm_elem<T>::V;
  const int g = threadIdx.x % GPR, r = threadIdx.x / GPR;
  const int c = blockIdx.y * GPR * V + g * V;
  const long img = BATCH ? blockIdx.x / nb : 0, chunk = BATCH ? blockIdx.x % nb : blockIdx.x;
  const long p0 = chunk * rows, p1 = min(HW, p0 + rows);
  const T* xi = x + img * HW * pitch;
  float s1[V], s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
  if (c < C) {
    float k[V];
    pm_elem<T>::ld(xi + c, k);
    for (long p = p0 + r; p < p1; p += RL) {
      float v[V];
      pm_elem<T>::ld(xi + p * pitch + c, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = v[j] - k[j];
        s1[j] += d, s2[j] = fmaf(d, d, s2[j]);
      }
    }
  }
  block_reduce_store<V, GPR, RL>(s1, s2, g, r, C, part + (long)blockIdx.x * C * 2);
}

// Second stage over the nb partials of one image: 4 channels x 64 lanes per block; each lane sums a strided subset in double, the 64
// lane sums are combined in lane order by lane 0 (deterministic; a 512-long serial chain per channel would cost ~100 us of pure latency).
constexpr int FC = 4, FL = 64;
__device__ __forceinline__ void final_sums(const float* __restrict__ part, int nb, int C, int c, int lane, double& s1, double& s2) {
  __shared__ double red[FL][FC][2];
  double a = 0.0, b = 0.0;
  if (c < C)
#pragma unroll 8   // eight independent partial loads in flight per lane (the additions keep their order)
    for (int i = lane; i < nb; i += FL) {
      const float2 v = *reinterpret_cast<const float2*>(part + ((long)i * C + c) * 2);
      a += (double)v.x, b += (double)v.y;
    }
  red[lane][threadIdx.x & (FC - 1)][0] = a, red[lane][threadIdx.x & (FC - 1)][1] = b;
  __syncthreads();
  s1 = s2 = 0.0;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < FL; ++i) s1 += red[i][threadIdx.x & (FC - 1)][0], s2 += red[i][threadIdx.x & (FC - 1)][1];
  }
}

// The incoming gradient of a backward reduction: load(q, c, d) hands over V channels of pixel q (counted over the whole batch). A tensor, or what bn.hip gathers
// from a pooled gradient (PoolGrad).
template <typename T>
struct TensorGrad {
  const T* dy;
  long pitch;
  __device__ __forceinline__ void load(long q, int c, float* d) const { pm_elem<T>::ld(dy + q * pitch + c, d); }
};

// backward partials: part[img][chunk][c][2] = sum(dyz), sum(dyz * xhat), dyz = dy masked by the ReLU of the forward pass; mean / invstd are [img][c].
// RELU 0: no activation. 1: mask = y > 0 read from the forward output (needed when a residual was added before the ReLU).
// 2: mask rebuilt from x (y = relu(bn(x)), no residual) -- one tensor less to read.
// 3: mask from the byte per 16-byte group bn_apply left behind (bit e = output e of the group was positive): 1 / 16 of the bytes of reading y.
// GOUT: also store dyz (the gradient of the residual branch), so that the apply pass reads one tensor (dyz) instead of two (dy, y).
template <typename T, int GPR, int RL, bool BATCH, int RELU, bool GOUT, typename SRC>
__global__ __launch_bounds__(GPR* RL) void norm_bwd_partial(SRC dy, const T* __restrict__ y, long ypitch, const uint8_t* __restrict__ mask, const T* __restrict__ x, long xpitch,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ gout, long gpitch, long HW, int C, int rows, int nb,
                                                            float* __restrict__ part) {
  constexpr int V = pm_elem<T>::V;
  const int g = threadIdx.x % GPR, r = threadIdx.x / GPR;
  const int c = blockIdx.y * GPR * V + g * V;
  const long img = BATCH ? blockIdx.x / nb : 0, chunk = BATCH ? blockIdx.x % nb : blockIdx.x;
  const long p0 = chunk * rows, p1 = min(HW, p0 + rows), q0 = img * HW;
  float s1[V], s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
  if (c < C) {
    float mu[V], is[V], ga[V], be[V];
    pm_ldp<V>(mean + img * C + c, mu), pm_ldp<V>(invstd + img * C + c, is);
    if (RELU == 2) pm_ldp<V>(gamma + c, ga), pm_ldp<V>(beta + c, be);
    for (long p = p0 + r; p < p1; p += RL) {
      float d[V], v[V], o[V];
      dy.load(q0 + p, c, d);
      pm_elem<T>::ld(x + (q0 + p) * xpitch + c, v);
      if (RELU == 1) {
        pm_elem<T>::ld(y + (q0 + p) * ypitch + c, o);
        relu_mask<V>(o, d);
      } else if (RELU == 3) {
        relu_mask_bits<V>(mask[(q0 + p) * (C / V) + c / V], d);
      } else if (RELU == 2) {
        bn_affine<V>(v, mu, is, ga, be, o);
        relu_mask<V>(o, d);
      }
      if (GOUT) pm_elem<T>::st(gout + (q0 + p) * gpitch + c, d);
#pragma unroll
      for (int j = 0; j < V; ++j) s1[j] += d[j], s2[j] = fmaf(d[j], (v[j] - mu[j]) * is[j], s2[j]);
    }
  }
  block_reduce_store<V, GPR, RL>(s1, s2, g, r, C, part + (long)blockIdx.x * C * 2);
}

// ---- elementwise passes: block = (image, pixel chunk), 256 threads ------------------------------------------------------------------------------------------
// FIXED: the channel groups divide the block (cg = C / V a divisor of 256) -- a thread keeps one group and its per-(image, channel) constants in registers and
// strides over pixels. Otherwise a thread walks (pixel, group) items and re-loads the constants: 128-192 bytes of L1 traffic for every 16-byte group of activations
// it moves, which held the bf16 BatchNorm passes at 4.0-4.4 TB/s where their fp32 twins reach 5.6 (twice the tensor bytes per parameter load).
// F, the pass: F::V channels per group; F::BATCH (false: one image, blockIdx.x is the block within it); struct F::K, the constants of one group;
// f.load(img, ch, k) fills them, f.pixel(q, ch, k) evaluates group ch of pixel q (counted over the whole batch).
inline bool fixed_ok(int cg) { return cg >= 1 && cg <= 256 && 256 % cg == 0; }
// blocks per image of an elementwise pass: up to 4096 blocks over the batch
inline int ew_bpi(int n, long HW, int cg, bool fixed) {
  const long work = fixed ? (HW + 256 / cg - 1) / (256 / cg) : (HW * cg + 255) / 256;
  return (int)std::max<long>(1, std::min<long>(work, std::max<long>(1, 4096 / n)));
}
template <bool FIXED, typename F>
__device__ __forceinline__ void norm_ew_drive(const F& f, long HW, int cg, int bpi) {
  const long img = F::BATCH ? blockIdx.x / bpi : 0;
  const int blk = F::BATCH ? blockIdx.x % bpi : blockIdx.x;
  if constexpr (FIXED) {
    const int ppb = 256 / cg, ch = (threadIdx.x % cg) * F::V;
    typename F::K k;
    f.load(img, ch, k);
    for (long p = (long)blk * ppb + threadIdx.x / cg; p < HW; p += (long)bpi * ppb) f.pixel(img * HW + p, ch, k);
  } else {
    const long total = HW * cg;
    for (long i = (long)blk * 256 + threadIdx.x; i < total; i += (long)bpi * 256) {
      const long p = i / cg;
      const int ch = (int)(i - p * cg) * F::V;
      typename F::K k;
      f.load(img, ch, k);
      f.pixel(img * HW + p, ch, k);
    }
  }
}
template <bool FIXED, typename F>
__global__ __launch_bounds__(256) void norm_ew_kernel(F f, long HW, int cg, int bpi) {
  norm_ew_drive<FIXED>(f, HW, cg, bpi);
}

}  // namespace
