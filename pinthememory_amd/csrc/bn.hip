// K4: BatchNorm2d over NHWC activations of both tiers (train statistics, apply + ReLU + residual, backward), HBM-bound.
// Replaces mynn.Norm2d (the reference's network/mynn.py:8-14) == nn.BatchNorm2d / SyncBatchNorm everywhere it is
// used (Resnet.py:146-151,429,456; deepv3plus.py:73,79,88,399,405,410,413,421; memory.py:76,105).
// Statistics are shifted sums (shift = first pixel of each channel) -> (mean, M2, count), combined in double in a
// fixed order: one pass over the activation, no catastrophic cancellation, deterministic, mergeable across ranks.
// The reductions, the mask helpers, the dx expression and the fixed-group elementwise driver are norm_parts.h's, shared with instnorm.hip: BatchNorm runs them
// with one image of P pixels. Its own: the plan, the finishes (float, running moments, the moments exchange format, slab partials, the rank merge), the folds and
// the functors of its bf16 elementwise passes.
#include "norm_parts.h"

namespace {

// count <= 0 on the host: the element count lives on the device at sums[2 * C] -- SyncBatchNorm all-reduces it with the two sums, so ranks with
// different batch sizes normalise by the true global count (torch.nn.SyncBatchNorm gathers the counts the same way)
__device__ __forceinline__ float bn_inv_n(bool dev_count, const float* sums, int C, float host_inv_n) { return dev_count ? 1.f / sums[2 * C] : host_inv_n; }
// ---- reductions -------------------------------------------------------------------------------------------------------------------------
// 256-thread blocks: RL = 256 / GPR row lanes, GPR from the element type (pm_elem<T>::gpr) -- the bf16 maps of <= 64 channels would idle half-waves at 16.
// rows: pixels per block: >= 2048 blocks over (pixel chunks x channel groups), >= 64 rows each
template <typename T>
Plan bn_plan(long P, int C) {
  Plan p;
  p.gpr = pm_elem<T>::gpr(C);
  const int RL = 256 / p.gpr, CB = p.gpr * pm_elem<T>::V;
  p.colblocks = pm_cdiv(C, CB);
  const long want = std::max<long>(512, 2048 / std::max<long>(1, p.colblocks));   // narrow tensors (64 channels) need more pixel chunks to fill the GPU
  const long r = std::max<long>((P + want - 1) / want, 64);
  p.rows = (int)((r + RL - 1) / RL * RL);
  p.nb = pm_cdiv(P, p.rows);
  return p;
}
template <typename T>
constexpr int MIN_GPR = pm_elem<T>::V == 8 ? 8 : 16;      // pm_elem<float>::gpr is always 16
template <typename T>
size_t bn_workspace(const pm_tensor* x) {
  return pm_align_up((size_t)bn_plan<T>(pm_pixels(x), x->c).nb * x->c * 2 * sizeof(float), 256);
}
// The tail of every statistics kernel: channel c's (mean m, M2 m2, count n) leave as moments (mean | M2 | count, the SyncBatchNorm exchange format), or (FIN) as
// mean / invstd plus the running-moment update, on the same float values the moments would hand over (bit-identical), one launch less per BN layer.
template <bool FIN>
__device__ __forceinline__ void bn_finish(int c, int C, float m, float m2, float n, float* __restrict__ moments, float eps, float* __restrict__ mean,
                                          float* __restrict__ invstd, float* running_mean, float* running_var, float momentum) {
  if constexpr (!FIN) {
    moments[c] = m, moments[C + c] = m2, moments[2 * C + c] = n;
  } else {
    const float var = m2 / n;
    mean[c] = m;
    invstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    if (running_var && n > 1.f) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2 / (n - 1.f));   // n == 1: no unbiased estimate (0 / 0)
  }
}

template <typename T, bool FIN>
__global__ __launch_bounds__(256) void bn_stats_final(const float* __restrict__ part, int nb, const T* __restrict__ x, long P, int C, float* __restrict__ moments,
                                                      float eps, float* __restrict__ mean, float* __restrict__ invstd, float* running_mean, float* running_var,
                                                      float momentum) {
  const int c = blockIdx.x * FC + (threadIdx.x & (FC - 1)), lane = threadIdx.x / FC;
  double s1, s2;
  final_sums(part, nb, C, c, lane, s1, s2);
  if (lane != 0 || c >= C) return;
  const double n = (double)P;
  const float m = (float)((double)pm_elem<T>::widen(x[c]) + s1 / n), m2 = (float)fmax(s2 - s1 * s1 / n, 0.0);
  bn_finish<FIN>(c, C, m, m2, (float)n, moments, eps, mean, invstd, running_mean, running_var, momentum);
}

__global__ void bn_finalize_kernel(const float* __restrict__ moments, int C, float eps, float* __restrict__ mean, float* __restrict__ invstd,
                                   float* running_mean, float* running_var, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_finish<true>(c, C, moments[c], moments[C + c], moments[2 * C + c], nullptr, eps, mean, invstd, running_mean, running_var, momentum);
}

// Merge of the (mean, M2) slab partials a convolution epilogue emitted for its own output (conv_igemm.hip, staged epilogue): rows in slabs
// of 32, part[slab][c][2]. Block = 4 channels x 64 lanes; lane l accumulates, in double, A = sum n_b mean_b and B = sum (M2_b + n_b mean_b^2)
// over slabs l, l + 64, ... (two FMAs per slab, no division); the 64 lane pairs are added in lane order (fixed -> deterministic);
// mean = A / N, M2 = B - N mean^2 (the within-slab part is exact two-pass fp32; the between-slab part is a sum of squares in double:
// relative error 1e-16 (mean^2 / var), harmless below 1e8). MOM: write mean | M2 | count for the SyncBatchNorm exchange instead of finalising.
template <bool MOM>
__global__ __launch_bounds__(256) void bn_partials_final(const float* __restrict__ part, long rows, int C, float eps, float* __restrict__ mean,
                                                         float* __restrict__ invstd, float* running_mean, float* running_var, float momentum,
                                                         float* __restrict__ moments) {
  __shared__ double red[FL][FC][2];
  const int ci = threadIdx.x & (FC - 1), lane = threadIdx.x / FC;
  const int c = blockIdx.x * FC + ci;
  const long nslab = (rows + 31) / 32;
  double A = 0.0, B = 0.0;
  if (c < C)
#pragma unroll 8
    for (long sidx = lane; sidx < nslab; sidx += FL) {
      const float2 v = *reinterpret_cast<const float2*>(part + (sidx * C + c) * 2);
      const double nb = (double)min(32l, rows - sidx * 32), mb = (double)v.x;
      A = fma(nb, mb, A);
      B += fma(nb * mb, mb, (double)v.y);
    }
  red[lane][ci][0] = A, red[lane][ci][1] = B;
  __syncthreads();
  if (lane != 0 || c >= C) return;
  A = B = 0.0;
#pragma unroll 1
  for (int i = 0; i < FL; ++i) A += red[i][ci][0], B += red[i][ci][1];
  const double n = (double)rows, gm = A / n;
  bn_finish<!MOM>(c, C, (float)gm, (float)fmax(B - n * gm * gm, 0.0), (float)n, moments, eps, mean, invstd, running_mean, running_var, momentum);
}

// The incoming gradient of a backward pass: a tensor, or (the stem) what pm_maxpool3x3s2_bwd would have written, gathered per pixel from the gradient of the
// 3x3 / s2 max pool that followed the activation and its argmax bytes (pm_maxpool_gather: the same values in the same order), so that the full-resolution
// gradient is never written.
struct PoolGrad {
  const float* dyp;
  long pitch;
  int Ho, Wo;
  const uint8_t* arg;
  int H, W, C;
  __device__ __forceinline__ void load(long p, int c, float* d) const {
    pm_maxpool_gather<float, 4>(dyp, pitch, Ho, Wo, arg, H, W, C, p, c, d);
  }
};

__global__ __launch_bounds__(256) void bn_bwd_final(const float* __restrict__ part, int nb, int C, float* __restrict__ sums) {
  const int c = blockIdx.x * FC + (threadIdx.x & (FC - 1)), lane = threadIdx.x / FC;
  double s1, s2;
  final_sums(part, nb, C, c, lane, s1, s2);
  if (lane != 0 || c >= C) return;
  sums[c] = (float)s1;
  sums[C + c] = (float)s2;
}

// Chan et al. merge of per-rank (mean | M2 | count) rows gathered over the process group: [W][3C] -> [3C], in double.
// FIN: SyncBatchNorm costs one launch less per layer (bn_finish).
template <bool FIN>
__global__ void bn_merge_kernel(const float* __restrict__ parts, int W, int C, float* __restrict__ out, float eps, float* __restrict__ mean,
                                float* __restrict__ invstd, float* running_mean, float* running_var, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, s = 0.0;
  for (int r = 0; r < W; ++r) {
    const double cnt = parts[(long)r * 3 * C + 2 * C + c];
    n += cnt, s += cnt * (double)parts[(long)r * 3 * C + c];
  }
  const double gmean = s / n;
  double m2d = 0.0;
  for (int r = 0; r < W; ++r) {
    const double cnt = parts[(long)r * 3 * C + 2 * C + c], d = (double)parts[(long)r * 3 * C + c] - gmean;
    m2d += (double)parts[(long)r * 3 * C + C + c] + cnt * d * d;
  }
  bn_finish<FIN>(c, C, (float)gmean, (float)m2d, (float)n, out, eps, mean, invstd, running_mean, running_var, momentum);
}

// every BatchNorm of a network folded in one launch (eval-mode forward): table[i] = {gamma, beta, running_mean, running_var} device
// pointers of layer i, cs[i] its channel count, offs[i] its offset in the arena (scale at arena + offs[i], shift at arena + total + offs[i])
__global__ void bn_fold_multi_kernel(const unsigned long long* __restrict__ table, const int* __restrict__ cs, const int* __restrict__ offs, int total,
                                     float eps, float* __restrict__ arena) {
  const int i = blockIdx.x, C = cs[i];
  const float *g = (const float*)table[4 * i], *b = (const float*)table[4 * i + 1], *rm = (const float*)table[4 * i + 2], *rv = (const float*)table[4 * i + 3];
  float* scale = arena + offs[i];
  float* shift = arena + total + offs[i];
  for (int c = blockIdx.y * blockDim.x + threadIdx.x; c < C; c += gridDim.y * blockDim.x) {
    const float s = g[c] / sqrtf(rv[c] + eps);      // the same expressions as bn_fold_kernel: identical values
    scale[c] = s;
    shift[c] = b[c] - rm[c] * s;
  }
}

__global__ void bn_fold_kernel(const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ rm, const float* __restrict__ rv,
                               const float* __restrict__ cb, int C, float eps, float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = g[c] / sqrtf(rv[c] + eps);
  scale[c] = s;
  shift[c] = b[c] - rm[c] * s + (cb ? cb[c] * s : 0.f);
}

// ---- the bf16 elementwise passes on the fixed-group driver (norm_parts.h), one image ------------------------------------------------------------------------
// Only the bf16 tier: the fp32 passes stay on pm_ew_launch_as, where they reach 5.6 TB/s. Taken when the channel groups divide the block (C = 64 ... 2048).
constexpr int V8 = 8;
template <bool RES, bool MASK, bool RELU>
struct Bn16Apply {
  static constexpr int V = V8;
  static constexpr bool BATCH = false;
  const pm_bf16* __restrict__ x;
  long xp;
  const float *__restrict__ mean, *__restrict__ invstd, *__restrict__ gamma, *__restrict__ beta;
  const pm_bf16* __restrict__ res;
  long rp;
  pm_bf16* __restrict__ y;
  long yp;
  uint8_t* __restrict__ mask;
  int cg;
  struct K {
    float sc[V8], sh[V8];
  };
  __device__ __forceinline__ void load(long, int ch, K& k) const {
    float mu[V8], is[V8], ga[V8], be[V8];
    pm_ld8f(mean + ch, mu), pm_ld8f(invstd + ch, is), pm_ld8f(gamma + ch, ga), pm_ld8f(beta + ch, be);
#pragma unroll
    for (int e = 0; e < V8; ++e) k.sc[e] = is[e] * ga[e], k.sh[e] = fmaf(-mu[e], k.sc[e], be[e]);      // pm_bn_affine(v) == fmaf(v, sc, sh): the same two FMAs
  }
  __device__ __forceinline__ void pixel(long p, int ch, const K& k) const {
    float v[V8], o[V8];
    pm_ld8(x + p * xp + ch, v);
#pragma unroll
    for (int e = 0; e < V8; ++e) o[e] = fmaf(v[e], k.sc[e], k.sh[e]);
    if constexpr (RES) {
      float q[V8];
      pm_ld8(res + p * rp + ch, q);
#pragma unroll
      for (int e = 0; e < V8; ++e) o[e] += q[e];
    }
    if constexpr (MASK) mask[p * cg + ch / V8] = (unsigned char)positive_bits<V8>(o);
    if constexpr (RELU) relu<V8>(o);
    pm_st8(y + p * yp + ch, o);
  }
};

// MODE 0: no ReLU (dy is already the masked gradient); 1: mask = forward output > 0; 2: mask rebuilt from x
template <int MODE, bool DRES>
struct Bn16BwdApply {
  static constexpr int V = V8;
  static constexpr bool BATCH = false;
  const pm_bf16* __restrict__ dy;
  long dp;
  const pm_bf16* __restrict__ yo;
  long op;
  const pm_bf16* __restrict__ x;
  long xp;
  const float *__restrict__ mean, *__restrict__ invstd, *__restrict__ gamma, *__restrict__ beta, *__restrict__ sums;
  float host_inv_n;
  int dev_count, C;
  pm_bf16* __restrict__ dx;
  long dxp;
  pm_bf16* __restrict__ dres;
  long drp;
  struct K {
    float mu[V8], is[V8], k1[V8], k2[V8], sg[V8], sh[V8];
  };
  __device__ __forceinline__ void load(long, int ch, K& k) const {
    const float inv_n = bn_inv_n(dev_count, sums, C, host_inv_n);
    float ga[V8], s1[V8], s2[V8];
    pm_ld8f(mean + ch, k.mu), pm_ld8f(invstd + ch, k.is), pm_ld8f(gamma + ch, ga), pm_ld8f(sums + ch, s1), pm_ld8f(sums + C + ch, s2);
#pragma unroll
    for (int e = 0; e < V8; ++e) k.k1[e] = s1[e] * inv_n, k.k2[e] = s2[e] * inv_n, k.sg[e] = k.is[e] * ga[e];
    if constexpr (MODE == 2) {
      float be[V8];
      pm_ld8f(beta + ch, be);
#pragma unroll
      for (int e = 0; e < V8; ++e) k.sh[e] = fmaf(-k.mu[e], k.sg[e], be[e]);      // the forward pass's scale is sg
    }
  }
  __device__ __forceinline__ void pixel(long p, int ch, const K& k) const {
    float g[V8], v[V8], o[V8], r[V8];
    pm_ld8(dy + p * dp + ch, g);
    pm_ld8(x + p * xp + ch, v);
    if constexpr (MODE == 1) {
      pm_ld8(yo + p * op + ch, o);
      relu_mask<V8>(o, g);
    }
    if constexpr (MODE == 2) {
#pragma unroll
      for (int e = 0; e < V8; ++e) o[e] = fmaf(v[e], k.sg[e], k.sh[e]);
      relu_mask<V8>(o, g);
    }
    if constexpr (DRES) pm_st8(dres + p * drp + ch, g);
#pragma unroll
    for (int e = 0; e < V8; ++e) r[e] = BN_DX(g[e], v[e], k.mu[e], k.is[e], k.k1[e], k.k2[e], k.sg[e]);      // the generic kernel's expression, constants hoisted
    pm_st8(dx + p * dxp + ch, r);
  }
};
// one image of P pixels on the fixed driver: ew_bpi(1, ...) blocks
template <typename F>
void bn16_launch_fixed(const F& f, long P, int cg, hipStream_t st) {
  const int bpi = ew_bpi(1, P, cg, true);
  hipLaunchKernelGGL((norm_ew_kernel<true, F>), dim3(bpi), dim3(256), 0, st, f, P, cg, bpi);
}

// ---- host side: one function per pass, both element types ------------------------------------------------------------------------------------
#define BN_BY_DTYPE(x, f, ...) (pm_is_bf16(x) ? f<pm_bf16>(__VA_ARGS__) : f<float>(__VA_ARGS__))

// moments != NULL: mean | M2 | count; else finalise
template <typename T>
int bn_stats(const char* who, const pm_tensor* x, float* moments, float eps, float* mean, float* invstd, float* running_mean, float* running_var, float momentum,
             void* ws, size_t ws_bytes, hipStream_t st) {
  if (int e = pm_elem<T>::check(x, who)) return e;
  PM_REQUIRE(ws && ws_bytes >= bn_workspace<T>(x), PM_EWORKSPACE, "%s: workspace too small", who);
  const long P = pm_pixels(x);
  const int C = x->c;
  PM_REQUIRE(P > 0, PM_EINVAL, "%s: empty tensor", who);
  // torch.nn.BatchNorm2d in training mode: "Expected more than 1 value per channel when training" (B = 1 through ASPP's image-pooling branch)
  PM_REQUIRE(moments || P > 1, PM_EINVAL, "%s: expected more than 1 value per channel when training, got %ld", who, P);
  const Plan pl = bn_plan<T>(P, C);
  const T* px = (const T*)x->ptr;
  with_gpr<MIN_GPR<T>>(pl.gpr, [&](auto G) {
    constexpr int GPR = decltype(G)::value;
    hipLaunchKernelGGL((norm_stats_partial<T, GPR, 256 / GPR, false>), dim3(pl.nb, pl.colblocks), dim3(256), 0, st, px, (long)x->pitch, P, C, pl.rows, pl.nb, (float*)ws);
  });
  if (moments)
    hipLaunchKernelGGL((bn_stats_final<T, false>), dim3(pm_cdiv(C, FC)), dim3(256), 0, st, (const float*)ws, pl.nb, px, P, C, moments, 0.f, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f);
  else
    hipLaunchKernelGGL((bn_stats_final<T, true>), dim3(pm_cdiv(C, FC)), dim3(256), 0, st, (const float*)ws, pl.nb, px, P, C, (float*)nullptr, eps, mean, invstd,
                       running_mean, running_var, momentum);
  return pm_check_launch(who);
}

// RAFF: the residual is itself a BatchNorm output that was never stored -- bn_affine(r, ...) of the raw tensor r with its own (mean, invstd, gamma, beta),
// the two FMAs pm_bn_apply would have evaluated before storing it (an fp32 store and reload is lossless: same bits), added exactly where a stored residual is.
// mask: one byte per 16-byte channel group.
template <typename T, bool RAFF = false>
int bn_apply(const char* who, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* res, const float* rmean,
             const float* rinvstd, const float* rgamma, const float* rbeta, int relu_on, const pm_tensor* y, uint8_t* mask, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  if (int e = pm_elem<T>::check(x, who)) return e;
  if (int e = pm_elem<T>::check(y, who)) return e;
  PM_REQUIRE(pm_same_shape(x, y) && mean && invstd && gamma && beta, PM_EINVAL, "%s: bad args", who);
  if (res) {
    if (int e = pm_elem<T>::check(res, who)) return e;
    PM_REQUIRE(pm_same_shape(x, res), PM_EINVAL, "%s: residual shape mismatch", who);
  }
  PM_REQUIRE(!RAFF || (res && rmean && rinvstd && rgamma && rbeta), PM_EINVAL, "%s: bad args", who);
  const T *px = (const T*)x->ptr, *pr = res ? (const T*)res->ptr : nullptr;
  T* py = (T*)y->ptr;
  const long a = x->pitch, b = res ? res->pitch : 0, c = y->pitch, P = pm_pixels(x);
  const int cg = x->c / V;
  if constexpr (V == V8) {
    if (x->c % V8 == 0 && fixed_ok(cg) && P > 0) {
      with_flag(pr != nullptr, [&](auto R) {
        with_flag(mask != nullptr, [&](auto M) {
          with_flag(relu_on != 0, [&](auto L) {
            bn16_launch_fixed(Bn16Apply<decltype(R)::value, decltype(M)::value, decltype(L)::value>{px, a, mean, invstd, gamma, beta, pr, b, py, c, mask, cg}, P, cg, st);
          });
        });
      });
      return pm_check_launch(who);
    }
  }
  return pm_ew_launch_as<T>(P, x->c, st, who, [=] __device__(long p, int ch) {
    float v[V], mu[V], is[V], ga[V], be[V], o[V];
    pm_elem<T>::ld(px + p * a + ch, v);
    pm_ldp<V>(mean + ch, mu), pm_ldp<V>(invstd + ch, is), pm_ldp<V>(gamma + ch, ga), pm_ldp<V>(beta + ch, be);
    bn_affine<V>(v, mu, is, ga, be, o);
    if (pr) {
      float q[V];
      pm_elem<T>::ld(pr + p * b + ch, q);
      if constexpr (RAFF) {
        float rm[V], ri[V], rg[V], rb[V];
        pm_ldp<V>(rmean + ch, rm), pm_ldp<V>(rinvstd + ch, ri), pm_ldp<V>(rgamma + ch, rg), pm_ldp<V>(rbeta + ch, rb);
        bn_affine<V>(q, rm, ri, rg, rb, q);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] += q[j];
    }
    if (mask) mask[p * cg + ch / V] = (unsigned char)positive_bits<V>(o);
    if (relu_on) relu<V>(o);
    pm_elem<T>::st(py + p * c + ch, o);
  });
}

// dy: the incoming gradient (its own checks are the caller's). relu 0 ... 3 as norm_bwd_partial; the pooled gradient always takes mode 2 without gmask.
template <typename T, typename SRC>
int bn_bwd_reduce(const char* who, SRC dy, const pm_tensor* y, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, int relu_mode, const pm_tensor* gmask, float* sums, void* ws, size_t ws_bytes, hipStream_t st) {
  if (int e = pm_elem<T>::check(x, who)) return e;
  PM_REQUIRE(mean && invstd && sums, PM_EINVAL, "%s: bad args", who);
  PM_REQUIRE(relu_mode >= 0 && relu_mode <= 3, PM_EINVAL, "%s: relu mode %d (0 none, 1 mask from y, 2 mask rebuilt from x, 3 mask bytes)", who, relu_mode);
  PM_REQUIRE(relu_mode != 1 || (y && pm_elem<T>::check(y, who) == PM_OK && pm_same_shape(y, x)), PM_EINVAL, "%s: relu mode 1 needs the forward output", who);
  PM_REQUIRE(relu_mode != 2 || (gamma && beta), PM_EINVAL, "%s: relu mode 2 needs gamma and beta", who);
  PM_REQUIRE(relu_mode != 3 || mask, PM_EINVAL, "%s: relu mode 3 needs the mask bytes", who);
  PM_REQUIRE(!gmask || (relu_mode != 0 && pm_elem<T>::check(gmask, who) == PM_OK && pm_same_shape(gmask, x)), PM_EINVAL, "%s: gmask needs a ReLU mode and the shape of x", who);
  PM_REQUIRE(ws && ws_bytes >= bn_workspace<T>(x), PM_EWORKSPACE, "%s: workspace too small", who);
  const long P = pm_pixels(x);
  const int C = x->c;
  const Plan pl = bn_plan<T>(P, C);
  const T *py = relu_mode == 1 ? (const T*)y->ptr : nullptr, *px = (const T*)x->ptr;
  const long yp = relu_mode == 1 ? y->pitch : 0, gp = gmask ? gmask->pitch : 0;
  T* pg = gmask ? (T*)gmask->ptr : nullptr;
  with_gpr<MIN_GPR<T>>(pl.gpr, [&](auto G) {
    constexpr int GPR = decltype(G)::value;
    auto go = [&](auto R, auto O) {
      hipLaunchKernelGGL((norm_bwd_partial<T, GPR, 256 / GPR, false, decltype(R)::value, decltype(O)::value, SRC>), dim3(pl.nb, pl.colblocks), dim3(256), 0, st, dy, py, yp,
                         mask, px, (long)x->pitch, mean, invstd, gamma, beta, pg, gp, P, C, pl.rows, pl.nb, (float*)ws);
    };
    using std::false_type;
    using std::true_type;
    if constexpr (std::is_same<SRC, PoolGrad>::value) go(std::integral_constant<int, 2>{}, false_type{});
    else if (relu_mode == 0) go(std::integral_constant<int, 0>{}, false_type{});
    else if (relu_mode == 1 && gmask) go(std::integral_constant<int, 1>{}, true_type{});
    else if (relu_mode == 1) go(std::integral_constant<int, 1>{}, false_type{});
    else if (relu_mode == 2 && gmask) go(std::integral_constant<int, 2>{}, true_type{});
    else if (relu_mode == 2) go(std::integral_constant<int, 2>{}, false_type{});
    else if (gmask) go(std::integral_constant<int, 3>{}, true_type{});
    else go(std::integral_constant<int, 3>{}, false_type{});
  });
  hipLaunchKernelGGL(bn_bwd_final, dim3(pm_cdiv(C, FC)), dim3(256), 0, st, (const float*)ws, pl.nb, C, sums);
  return pm_check_launch(who);
}

// MODE < 0: the ReLU mode (0, 1, 2) is the run-time `relu_mode`; MODE 2 / 3: fixed at compile time (the pooled gradient / the mask bytes), no other branch is compiled.
template <typename T, int MODE, typename SRC>
int bn_bwd_apply(const char* who, SRC dy, const pm_tensor* y, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                 const float* beta, const float* sums, float count, int relu_mode, const pm_tensor* dx, const pm_tensor* dres, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  if (int e = pm_elem<T>::check(x, who)) return e;
  if (int e = pm_elem<T>::check(dx, who)) return e;
  PM_REQUIRE(pm_same_shape(dx, x) && mean && invstd && gamma && sums, PM_EINVAL, "%s: bad args", who);
  PM_REQUIRE(pm_aligned16(sums), PM_EINVAL, "%s: sums must be 16-byte aligned (sections of a shared exchange start at multiples of 4 floats)", who);
  if (MODE >= 0) relu_mode = MODE;
  PM_REQUIRE(MODE >= 0 || (relu_mode >= 0 && relu_mode <= 2), PM_EINVAL, "%s: relu mode %d (0 none, 1 mask from y, 2 mask rebuilt from x)", who, relu_mode);
  PM_REQUIRE(relu_mode != 1 || (y && pm_elem<T>::check(y, who) == PM_OK && pm_same_shape(y, x)), PM_EINVAL, "%s: relu mode 1 needs the forward output", who);
  PM_REQUIRE(relu_mode != 2 || beta, PM_EINVAL, "%s: relu mode 2 needs beta", who);
  PM_REQUIRE(relu_mode != 3 || mask, PM_EINVAL, "%s: relu mode 3 needs the mask bytes", who);
  PM_REQUIRE(!dres || (pm_elem<T>::check(dres, who) == PM_OK && pm_same_shape(dres, x)), PM_EINVAL, "%s: dres shape mismatch", who);
  const T *po = relu_mode == 1 ? (const T*)y->ptr : nullptr, *px = (const T*)x->ptr;
  T *pdx = (T*)dx->ptr, *pdr = dres ? (T*)dres->ptr : nullptr;
  const long b = relu_mode == 1 ? y->pitch : 0, c = x->pitch, d = dx->pitch, e2 = dres ? dres->pitch : 0, P = pm_pixels(x);
  const int C = x->c, cg = C / V;
  const bool dev_count = !(count > 0.f), from_x = relu_mode == 2;
  const float host_inv_n = dev_count ? 0.f : 1.f / count;
  if constexpr (V == V8 && MODE < 0) {
    if (C % V8 == 0 && fixed_ok(cg) && P > 0) {
      auto go = [&](auto M) {
        with_flag(pdr != nullptr, [&](auto D) {
          bn16_launch_fixed(Bn16BwdApply<decltype(M)::value, decltype(D)::value>{dy.dy, dy.pitch, po, b, px, c, mean, invstd, gamma, beta, sums, host_inv_n, dev_count ? 1 : 0, C,
                                                                                 pdx, d, pdr, e2},
                            P, cg, st);
        });
      };
      if (relu_mode == 0) go(std::integral_constant<int, 0>{});
      else if (relu_mode == 1) go(std::integral_constant<int, 1>{});
      else go(std::integral_constant<int, 2>{});
      return pm_check_launch(who);
    }
  }
  return pm_ew_launch_as<T>(P, C, st, who, [=] __device__(long p, int ch) {
    const float inv_n = bn_inv_n(dev_count, sums, C, host_inv_n);
    float g[V], v[V], mu[V], is[V], ga[V], s1[V], s2[V], r[V];
    dy.load(p, ch, g);
    if (MODE < 0 && po) {
      float o[V];
      pm_elem<T>::ld(po + p * b + ch, o);
      relu_mask<V>(o, g);
    }
    if constexpr (MODE == 3) relu_mask_bits<V>(mask[p * cg + ch / V], g);
    pm_elem<T>::ld(px + p * c + ch, v);
    pm_ldp<V>(mean + ch, mu), pm_ldp<V>(invstd + ch, is), pm_ldp<V>(gamma + ch, ga);
    if (MODE == 2 || (MODE < 0 && from_x)) {
      float be[V], o[V];
      pm_ldp<V>(beta + ch, be);
      bn_affine<V>(v, mu, is, ga, be, o);
      relu_mask<V>(o, g);
    }
    if (MODE < 0 && pdr) pm_elem<T>::st(pdr + p * e2 + ch, g);
    pm_ldp<V>(sums + ch, s1), pm_ldp<V>(sums + C + ch, s2);
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = BN_DX(g[j], v[j], mu[j], is[j], s1[j] * inv_n, s2[j] * inv_n, is[j] * ga[j]);
    pm_elem<T>::st(pdx + p * d + ch, r);
  });
}

// the incoming gradient as a tensor of x's type and shape
template <typename T>
int tensor_grad(const char* who, const pm_tensor* dy, const pm_tensor* x, TensorGrad<T>* g) {
  if (int e = pm_elem<T>::check(dy, who)) return e;
  PM_REQUIRE(pm_same_shape(dy, x), PM_EINVAL, "%s: dy must have the shape of x", who);
  g->dy = (const T*)dy->ptr, g->pitch = dy->pitch;
  return PM_OK;
}
template <typename T>
int bn_bwd_reduce_tensor(const char* who, const pm_tensor* dy, const pm_tensor* y, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int relu_mode, const pm_tensor* gmask, float* sums, void* ws, size_t ws_bytes, hipStream_t st) {
  TensorGrad<T> g;
  if (int e = tensor_grad<T>(who, dy, x, &g)) return e;
  return bn_bwd_reduce<T>(who, g, y, mask, x, mean, invstd, gamma, beta, relu_mode, gmask, sums, ws, ws_bytes, st);
}
template <typename T>
int bn_bwd_apply_tensor(const char* who, const pm_tensor* dy, const pm_tensor* y, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, const float* sums, float count, int relu_mode, const pm_tensor* dx, const pm_tensor* dres, hipStream_t st) {
  TensorGrad<T> g;
  if (int e = tensor_grad<T>(who, dy, x, &g)) return e;
  return bn_bwd_apply<T, -1>(who, g, y, nullptr, x, mean, invstd, gamma, beta, sums, count, relu_mode, dx, dres, st);
}
// the stem: dy is the gradient of the 3x3 / s2 / p1 max pool of a tensor shaped like x (fp32)
int pool_grad(const char* who, const pm_tensor* dyp, const uint8_t* argmax, const pm_tensor* x, PoolGrad* g) {
  PM_REQUIRE(dyp && argmax && x, PM_EINVAL, "%s: null", who);
  if (int e = pm_elem<float>::check(dyp, who)) return e;
  if (int e = pm_elem<float>::check(x, who)) return e;
  PM_REQUIRE(dyp->n == x->n && dyp->c == x->c && dyp->h == (x->h + 2 - 3) / 2 + 1 && dyp->w == (x->w + 2 - 3) / 2 + 1, PM_EINVAL,
             "%s: dy is the gradient of the 3x3 / s2 / p1 max pool of a tensor shaped like x", who);
  *g = PoolGrad{(const float*)dyp->ptr, (long)dyp->pitch, dyp->h, dyp->w, argmax, x->h, x->w, x->c};
  return PM_OK;
}

}  // namespace

extern "C" size_t pm_bn_workspace(const pm_tensor* x) { return BN_BY_DTYPE(x, bn_workspace, x); }

extern "C" int pm_bn_stats(const pm_tensor* x, float* moments, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(x && moments, PM_EINVAL, "bn_stats: null");
  return BN_BY_DTYPE(x, bn_stats, "bn_stats", x, moments, 0.f, nullptr, nullptr, nullptr, nullptr, 0.f, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pm_bn_stats_finalize(const pm_tensor* x, float eps, float* mean, float* invstd, float* running_mean, float* running_var, float momentum,
                                    void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(x && mean && invstd, PM_EINVAL, "bn_stats_finalize: bad args");
  return BN_BY_DTYPE(x, bn_stats, "bn_stats_finalize", x, nullptr, eps, mean, invstd, running_mean, running_var, momentum, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pm_bn_finalize(const float* moments, int c, float eps, float* mean, float* invstd, float* running_mean, float* running_var,
                              float momentum, void* stream) {
  PM_REQUIRE(moments && mean && invstd && c > 0, PM_EINVAL, "bn_finalize: bad args");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(pm_cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, moments, c, eps, mean, invstd, running_mean, running_var,
                     momentum);
  return pm_check_launch("bn_finalize");
}

extern "C" int pm_bn_merge(const float* parts, int world, int c, float* moments, void* stream) {
  PM_REQUIRE(parts && moments && world >= 1 && c > 0, PM_EINVAL, "bn_merge: bad args");
  hipLaunchKernelGGL(bn_merge_kernel<false>, dim3(pm_cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, parts, world, c, moments, 0.f, (float*)nullptr,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f);
  return pm_check_launch("bn_merge");
}

extern "C" int pm_bn_merge_finalize(const float* parts, int world, int c, float eps, float* mean, float* invstd, float* running_mean, float* running_var,
                                    float momentum, void* stream) {
  PM_REQUIRE(parts && mean && invstd && world >= 1 && c > 0, PM_EINVAL, "bn_merge_finalize: bad args");
  hipLaunchKernelGGL(bn_merge_kernel<true>, dim3(pm_cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, parts, world, c, (float*)nullptr, eps, mean, invstd,
                     running_mean, running_var, momentum);
  return pm_check_launch("bn_merge_finalize");
}

extern "C" int pm_bn_partials_finalize(const float* partials, int64_t pixels, int c, float eps, float* mean, float* invstd, float* running_mean,
                                       float* running_var, float momentum, float* moments, void* stream) {
  PM_REQUIRE(partials && pixels > 0 && c > 0 && (moments || (mean && invstd)), PM_EINVAL, "bn_partials_finalize: bad args");
  PM_REQUIRE(moments || pixels > 1, PM_EINVAL, "bn_partials_finalize: expected more than 1 value per channel when training, got %ld", (long)pixels);
  hipStream_t st = (hipStream_t)stream;
  if (moments)
    hipLaunchKernelGGL(bn_partials_final<true>, dim3(pm_cdiv(c, FC)), dim3(256), 0, st, partials, (long)pixels, c, eps, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, 0.f, moments);
  else
    hipLaunchKernelGGL(bn_partials_final<false>, dim3(pm_cdiv(c, FC)), dim3(256), 0, st, partials, (long)pixels, c, eps, mean, invstd, running_mean, running_var,
                       momentum, (float*)nullptr);
  return pm_check_launch("bn_partials_finalize");
}

extern "C" int pm_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, const float* conv_bias, int c, float eps, float* scale,
                          float* shift, void* stream) {
  PM_REQUIRE(gamma && beta && rm && rv && scale && shift && c > 0, PM_EINVAL, "bn_fold: bad args");
  hipLaunchKernelGGL(bn_fold_kernel, dim3(pm_cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, gamma, beta, rm, rv, conv_bias, c, eps, scale, shift);
  return pm_check_launch("bn_fold");
}

extern "C" int pm_bn_fold_multi(const void* table, const int* cs, const int* offs, int n, int max_c, int total, float eps, float* arena, void* stream) {
  PM_REQUIRE(table && cs && offs && arena && n > 0 && max_c > 0 && total > 0, PM_EINVAL, "bn_fold_multi: bad args");
  hipLaunchKernelGGL(bn_fold_multi_kernel, dim3(n, pm_cdiv(max_c, 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)table, cs, offs, total, eps,
                     arena);
  return pm_check_launch("bn_fold_multi");
}

extern "C" int pm_bn_apply(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* res,
                           int relu, const pm_tensor* y, void* stream) {
  return pm_bn_apply_mask(x, mean, invstd, gamma, beta, res, relu, y, nullptr, stream);
}

extern "C" int pm_bn_apply_mask(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* res,
                                int relu, const pm_tensor* y, uint8_t* mask, void* stream) {
  PM_REQUIRE(x && y, PM_EINVAL, "bn_apply: null");
  return BN_BY_DTYPE(x, bn_apply, "bn_apply", x, mean, invstd, gamma, beta, res, nullptr, nullptr, nullptr, nullptr, relu, y, mask, (hipStream_t)stream);
}

// pm_bn_apply_mask whose residual is bn(r) of a second raw tensor (the downsample branch of a stage's first Bottleneck): the normalised residual is never stored.
extern "C" int pm_bn_apply_mask_affine(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* r,
                                       const float* r_mean, const float* r_invstd, const float* r_gamma, const float* r_beta, int relu, const pm_tensor* y,
                                       uint8_t* mask, void* stream) {
  PM_REQUIRE(x && y && r, PM_EINVAL, "bn_apply_mask_affine: null");      // fp32 only: the bf16 tier stores its normalised residual
  return bn_apply<float, true>("bn_apply_mask_affine", x, mean, invstd, gamma, beta, r, r_mean, r_invstd, r_gamma, r_beta, relu, y, mask, (hipStream_t)stream);
}

extern "C" int pm_bn_bwd_reduce(const pm_tensor* dy, const pm_tensor* y, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, int relu, const pm_tensor* gmask, float* sums, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(dy && x, PM_EINVAL, "bn_bwd_reduce: null");
  PM_REQUIRE(relu >= 0 && relu <= 2, PM_EINVAL, "bn_bwd_reduce: relu mode %d (0 none, 1 mask from y, 2 mask rebuilt from x)", relu);
  return BN_BY_DTYPE(x, bn_bwd_reduce_tensor, "bn_bwd_reduce", dy, y, nullptr, x, mean, invstd, gamma, beta, relu, gmask, sums, ws, ws_bytes, (hipStream_t)stream);
}

// BN + residual + ReLU backward reduce with the ReLU mask taken from pm_bn_apply_mask's bytes instead of the forward output: sums and the masked
// gradient gmask (= the gradient of the residual branch), as pm_bn_bwd_reduce(relu = 1) gives them -- same values, 1 / 16 of the mask bytes.
extern "C" int pm_bn_bwd_reduce_mask(const pm_tensor* dy, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd,
                                     const pm_tensor* gmask, float* sums, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(dy && x && mask, PM_EINVAL, "bn_bwd_reduce_mask: null");
  return BN_BY_DTYPE(x, bn_bwd_reduce_tensor, "bn_bwd_reduce_mask", dy, nullptr, mask, x, mean, invstd, nullptr, nullptr, 3, gmask, sums, ws, ws_bytes,
                     (hipStream_t)stream);
}

extern "C" int pm_bn_bwd_apply(const pm_tensor* dy, const pm_tensor* y, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, const float* sums, float count, int relu, const pm_tensor* dx, const pm_tensor* dres, void* stream) {
  PM_REQUIRE(dy && x && dx, PM_EINVAL, "bn_bwd_apply: null");
  PM_REQUIRE(relu >= 0 && relu <= 2, PM_EINVAL, "bn_bwd_apply: relu mode %d (0 none, 1 mask from y, 2 mask rebuilt from x)", relu);
  return BN_BY_DTYPE(x, bn_bwd_apply_tensor, "bn_bwd_apply", dy, y, x, mean, invstd, gamma, beta, sums, count, relu, dx, dres, (hipStream_t)stream);
}

// pm_bn_bwd_apply on dyz = dy masked by pm_bn_apply_mask's bytes (bit e of byte [pixel][ch / 4]: the ReLU passed element e), for ANY x of that shape: the BatchNorm the
// mask came from, or the downsample BatchNorm whose output was that activation's residual. Same arithmetic as pm_bn_bwd_apply(relu = 0) on the stored masked
// gradient, which therefore need not exist.
extern "C" int pm_bn_bwd_apply_mask(const pm_tensor* dy, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                                    const float* sums, float count, const pm_tensor* dx, void* stream) {
  PM_REQUIRE(dy && x && dx && mask, PM_EINVAL, "bn_bwd_apply_mask: null");
  TensorGrad<float> g;
  if (int e = tensor_grad<float>("bn_bwd_apply_mask", dy, x, &g)) return e;
  return bn_bwd_apply<float, 3>("bn_bwd_apply_mask", g, nullptr, mask, x, mean, invstd, gamma, nullptr, sums, count, 3, dx, nullptr, (hipStream_t)stream);
}

// ---- the stem's BN + ReLU backward behind a 3x3 / s2 max pool, straight from the pooled gradient ------------------------------------------------------------------
// pm_bn_bwd_reduce / pm_bn_bwd_apply with relu = 2 (mask rebuilt from x) where dy is what pm_maxpool3x3s2_bwd(dyp, argmax) would have written: each pass gathers
// it per pixel from the pooled gradient and the argmax bytes (a quarter of the pixels), so neither the full-resolution activation nor its gradient exists.
extern "C" int pm_bn_bwd_reduce_pool(const pm_tensor* dyp, const uint8_t* argmax, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                                     const float* beta, float* sums, void* ws, size_t ws_bytes, void* stream) {
  PoolGrad g;
  if (int e = pool_grad("bn_bwd_reduce_pool", dyp, argmax, x, &g)) return e;
  return bn_bwd_reduce<float>("bn_bwd_reduce_pool", g, nullptr, nullptr, x, mean, invstd, gamma, beta, 2, nullptr, sums, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pm_bn_bwd_apply_pool(const pm_tensor* dyp, const uint8_t* argmax, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                                    const float* beta, const float* sums, float count, const pm_tensor* dx, void* stream) {
  PoolGrad g;
  if (int e = pool_grad("bn_bwd_apply_pool", dyp, argmax, x, &g)) return e;
  PM_REQUIRE(dx, PM_EINVAL, "bn_bwd_apply_pool: null");
  return bn_bwd_apply<float, 2>("bn_bwd_apply_pool", g, nullptr, nullptr, x, mean, invstd, gamma, beta, sums, count, 2, dx, nullptr, (hipStream_t)stream);
}
