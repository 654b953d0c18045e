// K4b: InstanceNorm2d over NHWC activations of both tiers (per-image, per-channel statistics; apply + ReLU; backward), HBM-bound.
// nn.InstanceNorm2d(C, affine = False / True) of the IBN trunks: the stem's bn1 and the tail of the last Bottleneck of a stage.
// Biased variance, no running statistics: the same per-image statistics in train and eval mode, nothing folds.
// The reductions (shifted sums -> block partials -> a second stage in double, in a fixed order), the mask helpers, the dx expression and the elementwise driver are
// norm_parts.h's, shared with bn.hip: InstanceNorm runs them with the image index in the grid (blockIdx.x = img * nb + chunk), three launches per direction
// whatever the batch size. Its own: the plan, the two finishes (variance and invstd in double; the dgamma / dbeta sums over the images), the two functors of its
// elementwise passes and the entry points.
#include "norm_parts.h"

namespace {

// The plan differs from BatchNorm's on purpose: RL = 16 row lanes and blocks of GPR x 16 threads, and a chunking that does not depend on the element type -- the
// order in which a channel's values are summed (row lane, chunk, second stage) is then the same for both, and the bf16 instantiation yields the statistics the fp32
// one yields on the widened tensor, bit for bit.
constexpr int RL = 16;
// chunks per image: >= 2048 blocks over (image x chunk x 64-channel group), >= 64 pixels each
inline void in_chunks(int n, long HW, int C, int* rows, int* nb) {
  const long want = std::max<long>(1, 2048 / ((long)n * pm_cdiv(C, 64)));
  const long r = std::max<long>((HW + want - 1) / want, 64);
  *rows = (int)std::min<long>((r + RL - 1) / RL * RL, 1 << 30);
  *nb = pm_cdiv(HW, *rows);
}
template <typename T>
Plan in_plan(int n, long HW, int C) {
  Plan p;
  const int groups = C / pm_elem<T>::V;
  p.gpr = groups <= 8 ? 8 : 16;
  p.colblocks = pm_cdiv(groups, p.gpr);
  in_chunks(n, HW, C, &p.rows, &p.nb);
  return p;
}
// part[n][nb][C][2] | sums[n][2][C] (backward: sum g | sum g xhat per image)
inline size_t in_workspace(int n, long HW, int C) {
  int rows, nb;
  in_chunks(n, HW, C, &rows, &nb);
  return pm_align_up(((size_t)n * nb * C * 2 + (size_t)n * C * 2) * sizeof(float), 256);
}

// ---- the finishes: in double, unlike BatchNorm's float ones -- n x C values per call, the double divide and root cost nothing, and there is no exchange format
// whose float values a second path would have to reproduce. Block = (image, 4 channels).
// mean = K + s1 / HW, var = max(s2 - s1^2 / HW, 0) / HW (biased), invstd = 1 / sqrt(var + eps), one rounding each
template <typename T>
__global__ __launch_bounds__(FC* FL) void in_stats_final(const float* __restrict__ part, int nb, const T* __restrict__ x, long pitch, long HW, int C, float eps,
                                                         float* __restrict__ mean, float* __restrict__ invstd) {
  const int cblocks = (C + FC - 1) / FC;
  const long img = blockIdx.x / cblocks;
  const int c = (int)(blockIdx.x % cblocks) * FC + (threadIdx.x & (FC - 1)), lane = threadIdx.x / FC;
  double s1, s2;
  final_sums(part + img * nb * C * 2, nb, C, c, lane, s1, s2);
  if (lane != 0 || c >= C) return;
  const double n = (double)HW;
  const double var = fmax(s2 - s1 * s1 / n, 0.0) / n;
  mean[img * C + c] = (float)((double)pm_elem<T>::widen(x[img * HW * pitch + c]) + s1 / n);
  invstd[img * C + c] = (float)(1.0 / sqrt(var + (double)eps));
}
// sums[img][0][c] = sum g, sums[img][1][c] = sum g xhat
__global__ __launch_bounds__(FC* FL) void in_bwd_final(const float* __restrict__ part, int nb, int C, float* __restrict__ sums) {
  const int cblocks = (C + FC - 1) / FC;
  const long img = blockIdx.x / cblocks;
  const int c = (int)(blockIdx.x % cblocks) * FC + (threadIdx.x & (FC - 1)), lane = threadIdx.x / FC;
  double s1, s2;
  final_sums(part + img * nb * C * 2, nb, C, c, lane, s1, s2);
  if (lane != 0 || c >= C) return;
  sums[img * 2 * C + c] = (float)s1, sums[img * 2 * C + C + c] = (float)s2;
}

// ---- the functors of the elementwise passes (norm_ew_drive), both element types on the fixed driver --------------------------------------------------------------
// y = ((x - mean) * invstd) * gamma + beta, the centred form, not BatchNorm's folded x * scale + shift: with a mean far from zero (1e3 against a deviation of 1e-2)
// the fold would round the shift at the size of mean * scale. x and y may be the same tensor (a thread reads a group before it writes it).
template <typename T, bool RELU>
struct InApply {
  static constexpr int V = pm_elem<T>::V;
  static constexpr bool BATCH = true;
  const T* x;
  long xp;
  T* y;
  long yp;
  int C;
  const float *__restrict__ mean, *__restrict__ invstd, *__restrict__ gamma, *__restrict__ beta;
  struct K {
    float mu[V], is[V], ga[V], be[V];
  };
  __device__ __forceinline__ void load(long img, int ch, K& k) const {
    pm_ldp<V>(mean + img * C + ch, k.mu), pm_ldp<V>(invstd + img * C + ch, k.is);
    if (gamma) pm_ldp<V>(gamma + ch, k.ga), pm_ldp<V>(beta + ch, k.be);
#pragma unroll
    for (int j = 0; j < V; ++j) k.ga[j] = gamma ? k.ga[j] : 1.f, k.be[j] = gamma ? k.be[j] : 0.f;
  }
  __device__ __forceinline__ void pixel(long q, int ch, const K& k) const {
    float v[V], o[V];
    pm_elem<T>::ld(x + q * xp + ch, v);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = fmaf((v[j] - k.mu[j]) * k.is[j], k.ga[j], k.be[j]);
    if constexpr (RELU) relu<V>(o);
    pm_elem<T>::st(y + q * yp + ch, o);
  }
};

// dx = gamma * invstd * (g - s1 / HW - xhat * s2 / HW), g = dy masked by the ReLU of the forward pass (RELU: y > 0 read from the forward output)
template <typename T, bool RELU>
struct InBwdApply {
  static constexpr int V = pm_elem<T>::V;
  static constexpr bool BATCH = true;
  const T* __restrict__ dy;
  long dp;
  const T* __restrict__ x;
  long xp;
  const T* __restrict__ y;
  long yp;
  T* __restrict__ dx;
  long dxp;
  int C;
  float inv_hw;
  const float *__restrict__ mean, *__restrict__ invstd, *__restrict__ gamma, *__restrict__ sums;
  struct K {
    float mu[V], is[V], k1[V], k2[V], sg[V];
  };
  __device__ __forceinline__ void load(long img, int ch, K& k) const {
    float s1[V], s2[V];
    pm_ldp<V>(mean + img * C + ch, k.mu), pm_ldp<V>(invstd + img * C + ch, k.is), pm_ldp<V>(sums + img * 2 * C + ch, s1), pm_ldp<V>(sums + img * 2 * C + C + ch, s2);
    float ga[V] = {};      // zeroed: left undefined it is carried around the (pixel, group) loop, which costs the bf16 ReLU pass an occupancy step (66 VGPRs)
    if (gamma) pm_ldp<V>(gamma + ch, ga);
#pragma unroll
    for (int j = 0; j < V; ++j) k.k1[j] = s1[j] * inv_hw, k.k2[j] = s2[j] * inv_hw, k.sg[j] = gamma ? k.is[j] * ga[j] : k.is[j];
  }
  __device__ __forceinline__ void pixel(long q, int ch, const K& k) const {
    float d[V], v[V], o[V];
    pm_elem<T>::ld(dy + q * dp + ch, d);
    pm_elem<T>::ld(x + q * xp + ch, v);
    if constexpr (RELU) {
      float f[V];
      pm_elem<T>::ld(y + q * yp + ch, f);
      relu_mask<V>(f, d);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = BN_DX(d[j], v[j], k.mu[j], k.is[j], k.k1[j], k.k2[j], k.sg[j]);
    pm_elem<T>::st(dx + q * dxp + ch, o);
  }
};
// The backward apply pass with the affine finish folded in: the first block adds the per-image sums up, in double and in image order: dbeta[c] = sum_n s1,
// dgamma[c] = sum_n s2 (n x C values: no launch of its own, and the second stage above keeps one block per image).
template <bool FIXED, typename F>
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(F f, long HW, int cg, int bpi, int n, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  if (blockIdx.x == 0 && (dgamma || dbeta))
    for (int c = threadIdx.x; c < f.C; c += 256) {
      double t1 = 0.0, t2 = 0.0;
      for (long i = 0; i < n; ++i) t1 += (double)f.sums[i * 2 * f.C + c], t2 += (double)f.sums[i * 2 * f.C + f.C + c];
      if (dbeta) dbeta[c] = (float)t1;
      if (dgamma) dgamma[c] = (float)t2;
    }
  norm_ew_drive<FIXED>(f, HW, cg, bpi);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------------------------
struct View {
  const char* name;
  const void* ptr;
  int64_t pitch;
};
// the checks every entry point shares, in the order the header documents; vec: channels per 16-byte access of the dtype
int check_geometry(const char* who, int n, int h, int w, int c, int dtype, const View* views, int nviews) {
  for (int i = 0; i < nviews; ++i) PM_REQUIRE(views[i].ptr, PM_EINVAL, "%s: %s is null", who, views[i].name);
  PM_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, PM_EINVAL, "%s: sizes must be positive (n %d h %d w %d c %d)", who, n, h, w, c);
  PM_REQUIRE(dtype == PM_F32 || dtype == PM_BF16, PM_EUNSUPPORTED, "%s: unknown dtype %d", who, dtype);
  PM_REQUIRE(c % 8 == 0, PM_EUNSUPPORTED, "%s: c %% 8 != 0 (c %d)", who, c);
  const int vec = dtype == PM_BF16 ? 8 : 4;
  for (int i = 0; i < nviews; ++i) {
    PM_REQUIRE(views[i].pitch >= c && views[i].pitch % vec == 0, PM_EINVAL, "%s: the pitch of %s (%ld) must be >= c and a multiple of %d", who, views[i].name,
               (long)views[i].pitch, vec);
    PM_REQUIRE(pm_aligned16(views[i].ptr), PM_EINVAL, "%s: %s must be 16-byte aligned", who, views[i].name);
  }
  // the image index travels in gridDim.x: n x chunks (<= HW / 64 + 1 each) and n x C / 4 blocks
  PM_REQUIRE((long)n * std::max<long>(((long)h * w + 63) / 64, (c + FC - 1) / FC) < (1l << 31), PM_EUNSUPPORTED, "%s: batch too large for one grid", who);
  return PM_OK;
}

template <typename T>
int in_fwd(const char* who, const T* x, T* y, int n, long HW, int C, long xp, long yp, const float* gamma, const float* beta, float eps, int relu, float* mean,
           float* invstd, float* ws, hipStream_t st) {
  const Plan pl = in_plan<T>(n, HW, C);
  with_gpr<8>(pl.gpr, [&](auto G) {
    constexpr int GPR = decltype(G)::value;
    hipLaunchKernelGGL((norm_stats_partial<T, GPR, RL, true>), dim3(n * pl.nb, pl.colblocks), dim3(GPR * RL), 0, st, x, xp, HW, C, pl.rows, pl.nb, ws);
  });
  hipLaunchKernelGGL((in_stats_final<T>), dim3(n * pm_cdiv(C, FC)), dim3(FC * FL), 0, st, (const float*)ws, pl.nb, x, xp, HW, C, eps, mean, invstd);
  const int cg = C / pm_elem<T>::V;
  const bool fixed = fixed_ok(cg);
  const int bpi = ew_bpi(n, HW, cg, fixed);
  with_flag(fixed, [&](auto F) {
    with_flag(relu != 0, [&](auto R) {
      using Pass = InApply<T, decltype(R)::value>;
      hipLaunchKernelGGL((norm_ew_kernel<decltype(F)::value, Pass>), dim3(n * bpi), dim3(256), 0, st, Pass{x, xp, y, yp, C, mean, invstd, gamma, beta}, HW, cg, bpi);
    });
  });
  return pm_check_launch(who);
}

template <typename T>
int in_bwd(const char* who, const T* dy, const T* x, const T* y, T* dx, int n, long HW, int C, long dp, long xp, long yp, long dxp, const float* gamma,
           const float* mean, const float* invstd, int relu, float* dgamma, float* dbeta, float* ws, hipStream_t st) {
  const Plan pl = in_plan<T>(n, HW, C);
  float* sums = ws + (size_t)n * pl.nb * C * 2;
  const TensorGrad<T> g{dy, dp};
  with_gpr<8>(pl.gpr, [&](auto G) {
    with_flag(relu != 0, [&](auto R) {
      constexpr int GPR = decltype(G)::value;
      hipLaunchKernelGGL((norm_bwd_partial<T, GPR, RL, true, decltype(R)::value ? 1 : 0, false, TensorGrad<T>>), dim3(n * pl.nb, pl.colblocks), dim3(GPR * RL), 0, st, g, y, yp,
                         (const uint8_t*)nullptr, x, xp, mean, invstd, (const float*)nullptr, (const float*)nullptr, (T*)nullptr, 0l, HW, C, pl.rows, pl.nb, ws);
    });
  });
  hipLaunchKernelGGL(in_bwd_final, dim3(n * pm_cdiv(C, FC)), dim3(FC * FL), 0, st, (const float*)ws, pl.nb, C, sums);
  const int cg = C / pm_elem<T>::V;
  const bool fixed = fixed_ok(cg);
  const int bpi = ew_bpi(n, HW, cg, fixed);
  with_flag(fixed, [&](auto F) {
    with_flag(relu != 0, [&](auto R) {
      using Pass = InBwdApply<T, decltype(R)::value>;
      hipLaunchKernelGGL((in_bwd_apply_kernel<decltype(F)::value, Pass>), dim3(n * bpi), dim3(256), 0, st,
                         Pass{dy, dp, x, xp, y, yp, dx, dxp, C, 1.f / (float)HW, mean, invstd, gamma, (const float*)sums}, HW, cg, bpi, n, dgamma, dbeta);
    });
  });
  return pm_check_launch(who);
}

}  // namespace

extern "C" size_t pm_instnorm_workspace(int n, int h, int w, int c) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return in_workspace(n, (long)h * w, c);
}

extern "C" int pm_instnorm_fwd(const void* x, void* y, int n, int h, int w, int c, int64_t x_pitch, int64_t y_pitch, int dtype, const float* gamma, const float* beta,
                               float eps, int relu, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "instnorm_fwd";
  const View views[] = {{"x", x, x_pitch}, {"y", y, y_pitch}};
  PM_REQUIRE(mean && invstd, PM_EINVAL, "%s: mean / invstd is null", who);
  if (int e = check_geometry(who, n, h, w, c, dtype, views, 2)) return e;
  PM_REQUIRE((gamma != nullptr) == (beta != nullptr), PM_EINVAL, "%s: gamma and beta are both null (no affine) or both set", who);
  PM_REQUIRE(pm_aligned16(mean) && pm_aligned16(invstd) && pm_aligned16(gamma) && pm_aligned16(beta), PM_EINVAL, "%s: mean, invstd, gamma, beta must be 16-byte aligned",
             who);
  PM_REQUIRE(x == y ? x_pitch == y_pitch : true, PM_EINVAL, "%s: y aliases x with another pitch", who);
  PM_REQUIRE(ws && pm_aligned16(ws), PM_EINVAL, "%s: the workspace is null or not 16-byte aligned", who);
  PM_REQUIRE(ws_bytes >= in_workspace(n, (long)h * w, c), PM_EWORKSPACE, "%s: workspace too small", who);
  const long HW = (long)h * w;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == PM_BF16)
    return in_fwd<pm_bf16>(who, (const pm_bf16*)x, (pm_bf16*)y, n, HW, c, (long)x_pitch, (long)y_pitch, gamma, beta, eps, relu, mean, invstd, (float*)ws, st);
  return in_fwd<float>(who, (const float*)x, (float*)y, n, HW, c, (long)x_pitch, (long)y_pitch, gamma, beta, eps, relu, mean, invstd, (float*)ws, st);
}

extern "C" int pm_instnorm_bwd(const void* dy, const void* x, const void* y, void* dx, int n, int h, int w, int c, int64_t dy_pitch, int64_t x_pitch, int64_t y_pitch,
                               int64_t dx_pitch, int dtype, const float* gamma, const float* mean, const float* invstd, int relu, float* dgamma, float* dbeta, void* ws,
                               size_t ws_bytes, void* stream) {
  const char* who = "instnorm_bwd";
  const View views[] = {{"dy", dy, dy_pitch}, {"x", x, x_pitch}, {"dx", dx, dx_pitch}, {"y", y, y_pitch}};
  PM_REQUIRE(mean && invstd, PM_EINVAL, "%s: mean / invstd is null", who);
  if (int e = check_geometry(who, n, h, w, c, dtype, views, relu ? 4 : 3)) return e;      // y is read only behind a fused ReLU
  PM_REQUIRE(pm_aligned16(mean) && pm_aligned16(invstd) && pm_aligned16(gamma), PM_EINVAL, "%s: mean, invstd, gamma must be 16-byte aligned", who);
  PM_REQUIRE(ws && pm_aligned16(ws), PM_EINVAL, "%s: the workspace is null or not 16-byte aligned", who);
  PM_REQUIRE(ws_bytes >= in_workspace(n, (long)h * w, c), PM_EWORKSPACE, "%s: workspace too small", who);
  const long HW = (long)h * w;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == PM_BF16)
    return in_bwd<pm_bf16>(who, (const pm_bf16*)dy, (const pm_bf16*)x, (const pm_bf16*)y, (pm_bf16*)dx, n, HW, c, (long)dy_pitch, (long)x_pitch, (long)y_pitch,
                           (long)dx_pitch, gamma, mean, invstd, relu, dgamma, dbeta, (float*)ws, st);
  return in_bwd<float>(who, (const float*)dy, (const float*)x, (const float*)y, (float*)dx, n, HW, c, (long)dy_pitch, (long)x_pitch, (long)y_pitch, (long)dx_pitch, gamma,
                       mean, invstd, relu, dgamma, dbeta, (float*)ws, st);
}
