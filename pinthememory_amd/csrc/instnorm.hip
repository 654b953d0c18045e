// K4b: InstanceNorm2d over NHWC activations of both tiers (per-image, per-channel statistics; apply + ReLU; backward), HBM-bound.
// nn.InstanceNorm2d(C, affine = False / True) of the IBN trunks: the stem's bn1 and the tail of the last Bottleneck of a stage.
// Biased variance, no running statistics: the same per-image statistics in train and eval mode, nothing folds.
// Built as bn.hip is: shifted sums (shift = the first pixel of each image and channel) -> block partials in a workspace -> a second stage in double, in a fixed
// order (no floating-point atomics: bit-identical from run to run and under graph replay). One body for fp32 and bf16 tensors: a lane moves 16 bytes
// (pm_elem<T>::V channels), values are widened to fp32 in registers; every statistic / accumulator is fp32 (second stages in double); bf16 results are rounded once.
// Three launches per direction whatever the batch size: the image index is part of the grid.
// The order in which a channel's values are summed (row lane, chunk, second stage) does not depend on the element type: the bf16 instantiation yields the statistics
// the fp32 one yields on the widened tensor, bit for bit.
#include <type_traits>

#include "pm_common.h"

namespace {

constexpr int RL = 16;               // row lanes of a reduction block: lane r sums pixels p0 + r, p0 + r + RL, ... of the block's chunk
constexpr int FC = 4, FL = 64;       // second stage: 4 channels x 64 lanes per block

// gpr lane groups (of V channels) per pixel row: block = gpr x RL threads, CB = gpr * V channels
struct Plan {
  int gpr, colblocks, rows, nb;      // rows: pixels per chunk, nb: chunks per image
};
// chunks per image: >= 2048 blocks over (image x chunk x 64-channel group), >= 64 pixels each. Independent of the element type (see the header comment).
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
template <typename L>
void with_gpr(int gpr, L launch) {
  if (gpr == 8) return launch(std::integral_constant<int, 8>{});
  launch(std::integral_constant<int, 16>{});
}

// block-level reduce of per-thread (s1[V], s2[V]) over the row lanes, in row-lane order -> part[c][2] of this block's (image, chunk)
template <int V, int GPR>
__device__ __forceinline__ void block_reduce_store(const float* s1, const float* s2, int g, int r, int cb, int C, float* __restrict__ part) {
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
    const int ch = cb * CB + cc;
    if (ch < C) part[(long)ch * 2 + w] = s;
  }
}

// forward partials: sum(x - K), sum((x - K)^2) over the chunk, K = the image's first pixel
template <typename T, int GPR>
__global__ __launch_bounds__(GPR* RL) void in_stats_partial(const T* __restrict__ x, long pitch, long HW, int C, int rows, int nb, float* __restrict__ part) {
  constexpr int V = pm_elem<T>::V;
  const int g = threadIdx.x % GPR, r = threadIdx.x / GPR;
  const int c = blockIdx.y * GPR * V + g * V;
  const long img = blockIdx.x / nb, chunk = blockIdx.x % nb;
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
  block_reduce_store<V, GPR>(s1, s2, g, r, blockIdx.y, C, part + (long)blockIdx.x * C * 2);
}

// Second stage over the nb partials of one image: each lane sums a strided subset in double, the 64 lane sums are combined in lane order by lane 0.
__device__ __forceinline__ void final_sums(const float* __restrict__ part, int nb, int C, int c, int lane, double& s1, double& s2) {
  __shared__ double red[FL][FC][2];
  double a = 0.0, b = 0.0;
  if (c < C)
#pragma unroll 8
    for (int i = lane; i < nb; i += FL) {
      const float2 v = *reinterpret_cast<const float2*>(part + ((long)i * C + c) * 2);
      a += (double)v.x, b += (double)v.y;
    }
  red[lane][threadIdx.x & (FC - 1)][0] = a, red[lane][threadIdx.x & (FC - 1)][1] = b;
  __syncthreads();
  s1 = s2 = 0.0;
  if (lane == 0) {
#pragma unroll 1
    for (int i = 0; i < FL; ++i) s1 += red[i][threadIdx.x & (FC - 1)][0], s2 += red[i][threadIdx.x & (FC - 1)][1];
  }
}

// block = (image, 4 channels): mean = K + s1 / HW, var = max(s2 - s1^2 / HW, 0) / HW (biased), invstd = 1 / sqrt(var + eps), in double
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
  invstd[img * C + c] = (float)(1.0 / sqrt(var + (double)eps));      // one rounding: 64 x C values per call, the double divide and root cost nothing
}

// ---- elementwise passes: block = (image, pixel chunk) ----------------------------------------------------------------------------------------------------------
// FIXED: the channel groups divide the block (C / V a power of two <= 256: 64 ... 2048 channels) -- a thread keeps one group and its per-(image, channel) constants
// in registers and strides over pixels. Otherwise a thread walks (pixel, group) items and re-loads the constants (L1).
template <int V>
__device__ __forceinline__ void ld_affine(const float* gamma, const float* beta, int ch, float* ga, float* be) {
  if (gamma) {
    pm_ldp<V>(gamma + ch, ga), pm_ldp<V>(beta + ch, be);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) ga[j] = 1.f, be[j] = 0.f;
  }
}

// y = ((x - mean) * invstd) * gamma + beta, the centred form: with a mean far from zero (1e3 against a deviation of 1e-2) the folded x * scale + shift would round the
// shift at the size of mean * scale. x and y may be the same tensor (a thread reads a group before it writes it).
template <typename T, bool FIXED, bool RELU>
__global__ __launch_bounds__(256) void in_apply_kernel(const T* x, long xp, T* y, long yp, long HW, int C, int bpi, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta) {
  constexpr int V = pm_elem<T>::V;
  const int cg = C / V;
  const long img = blockIdx.x / bpi;
  const int blk = blockIdx.x % bpi;
  const T* xi = x + img * HW * xp;
  T* yi = y + img * HW * yp;
  const float *mi = mean + img * C, *ii = invstd + img * C;
  auto consts = [&](int ch, float* mu, float* is, float* ga, float* be) {
    pm_ldp<V>(mi + ch, mu), pm_ldp<V>(ii + ch, is);
    ld_affine<V>(gamma, beta, ch, ga, be);
  };
  auto pixel = [&](long p, int ch, const float* mu, const float* is, const float* ga, const float* be) {
    float v[V], o[V];
    pm_elem<T>::ld(xi + p * xp + ch, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = fmaf((v[j] - mu[j]) * is[j], ga[j], be[j]);
      if (RELU) o[j] = fmaxf(o[j], 0.f);
    }
    pm_elem<T>::st(yi + p * yp + ch, o);
  };
  float mu[V], is[V], ga[V], be[V];
  if constexpr (FIXED) {
    const int ppb = 256 / cg, ch = (threadIdx.x % cg) * V;
    consts(ch, mu, is, ga, be);
    for (long p = (long)blk * ppb + threadIdx.x / cg; p < HW; p += (long)bpi * ppb) pixel(p, ch, mu, is, ga, be);
  } else {
    const long total = HW * cg;
    for (long i = (long)blk * 256 + threadIdx.x; i < total; i += (long)bpi * 256) {
      const long p = i / cg;
      const int ch = (int)(i - p * cg) * V;
      consts(ch, mu, is, ga, be);
      pixel(p, ch, mu, is, ga, be);
    }
  }
}

// backward partials: sum(g), sum(g * xhat) over the chunk, g = dy masked by the ReLU of the forward pass (RELU: y > 0 read from the forward output)
template <typename T, int GPR, bool RELU>
__global__ __launch_bounds__(GPR* RL) void in_bwd_partial(const T* __restrict__ dy, long dp, const T* __restrict__ x, long xp, const T* __restrict__ y, long yp,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd, long HW, int C, int rows, int nb,
                                                          float* __restrict__ part) {
  constexpr int V = pm_elem<T>::V;
  const int g = threadIdx.x % GPR, r = threadIdx.x / GPR;
  const int c = blockIdx.y * GPR * V + g * V;
  const long img = blockIdx.x / nb, chunk = blockIdx.x % nb;
  const long p0 = chunk * rows, p1 = min(HW, p0 + rows), q0 = img * HW;
  float s1[V], s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
  if (c < C) {
    float mu[V], is[V];
    pm_ldp<V>(mean + img * C + c, mu), pm_ldp<V>(invstd + img * C + c, is);
    for (long p = p0 + r; p < p1; p += RL) {
      float d[V], v[V];
      pm_elem<T>::ld(dy + (q0 + p) * dp + c, d);
      pm_elem<T>::ld(x + (q0 + p) * xp + c, v);
      if constexpr (RELU) {
        float o[V];
        pm_elem<T>::ld(y + (q0 + p) * yp + c, o);
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = o[j] > 0.f ? d[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) s1[j] += d[j], s2[j] = fmaf(d[j], (v[j] - mu[j]) * is[j], s2[j]);
    }
  }
  block_reduce_store<V, GPR>(s1, s2, g, r, blockIdx.y, C, part + (long)blockIdx.x * C * 2);
}

// block = (image, 4 channels): sums[img][0][c] = sum g, sums[img][1][c] = sum g xhat
__global__ __launch_bounds__(FC* FL) void in_bwd_final(const float* __restrict__ part, int nb, int C, float* __restrict__ sums) {
  const int cblocks = (C + FC - 1) / FC;
  const long img = blockIdx.x / cblocks;
  const int c = (int)(blockIdx.x % cblocks) * FC + (threadIdx.x & (FC - 1)), lane = threadIdx.x / FC;
  double s1, s2;
  final_sums(part + img * nb * C * 2, nb, C, c, lane, s1, s2);
  if (lane != 0 || c >= C) return;
  sums[img * 2 * C + c] = (float)s1, sums[img * 2 * C + C + c] = (float)s2;
}

// dx = gamma * invstd * (g - s1 / HW - xhat * s2 / HW). The first block also adds the per-image sums up, in double and in image order: dbeta[c] = sum_n s1,
// dgamma[c] = sum_n s2 (n x C values: no launch of its own, and the second stage above keeps one block per image).
template <typename T, bool FIXED, bool RELU>
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const T* __restrict__ dy, long dp, const T* __restrict__ x, long xp, const T* __restrict__ y, long yp,
                                                           T* __restrict__ dx, long dxp, long HW, int C, int bpi, float inv_hw, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ sums, int n,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  constexpr int V = pm_elem<T>::V;
  const int cg = C / V;
  if (blockIdx.x == 0 && (dgamma || dbeta))
    for (int c = threadIdx.x; c < C; c += 256) {
      double t1 = 0.0, t2 = 0.0;
      for (long i = 0; i < n; ++i) t1 += (double)sums[i * 2 * C + c], t2 += (double)sums[i * 2 * C + C + c];
      if (dbeta) dbeta[c] = (float)t1;
      if (dgamma) dgamma[c] = (float)t2;
    }
  const long img = blockIdx.x / bpi, q0 = img * HW;
  const int blk = blockIdx.x % bpi;
  const float *mi = mean + img * C, *ii = invstd + img * C, *si = sums + img * 2 * C;
  auto consts = [&](int ch, float* mu, float* is, float* k1, float* k2, float* sg) {
    float s1[V], s2[V];
    pm_ldp<V>(mi + ch, mu), pm_ldp<V>(ii + ch, is), pm_ldp<V>(si + ch, s1), pm_ldp<V>(si + C + ch, s2);
    if (gamma) pm_ldp<V>(gamma + ch, sg);
#pragma unroll
    for (int j = 0; j < V; ++j) k1[j] = s1[j] * inv_hw, k2[j] = s2[j] * inv_hw, sg[j] = gamma ? is[j] * sg[j] : is[j];
  };
  auto pixel = [&](long p, int ch, const float* mu, const float* is, const float* k1, const float* k2, const float* sg) {
    float d[V], v[V], o[V];
    pm_elem<T>::ld(dy + (q0 + p) * dp + ch, d);
    pm_elem<T>::ld(x + (q0 + p) * xp + ch, v);
    if constexpr (RELU) {
      float f[V];
      pm_elem<T>::ld(y + (q0 + p) * yp + ch, f);
#pragma unroll
      for (int j = 0; j < V; ++j) d[j] = f[j] > 0.f ? d[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (d[j] - k1[j] - (v[j] - mu[j]) * is[j] * k2[j]) * sg[j];
    pm_elem<T>::st(dx + (q0 + p) * dxp + ch, o);
  };
  float mu[V], is[V], k1[V], k2[V], sg[V];
  if constexpr (FIXED) {
    const int ppb = 256 / cg, ch = (threadIdx.x % cg) * V;
    consts(ch, mu, is, k1, k2, sg);
    for (long p = (long)blk * ppb + threadIdx.x / cg; p < HW; p += (long)bpi * ppb) pixel(p, ch, mu, is, k1, k2, sg);
  } else {
    const long total = HW * cg;
    for (long i = (long)blk * 256 + threadIdx.x; i < total; i += (long)bpi * 256) {
      const long p = i / cg;
      const int ch = (int)(i - p * cg) * V;
      consts(ch, mu, is, k1, k2, sg);
      pixel(p, ch, mu, is, k1, k2, sg);
    }
  }
}

inline bool fixed_ok(int cg) { return cg >= 1 && cg <= 256 && 256 % cg == 0; }
// blocks per image of an elementwise pass: up to 4096 blocks over the batch
inline int apply_bpi(int n, long HW, int cg, bool fixed) {
  const long work = fixed ? (HW + 256 / cg - 1) / (256 / cg) : (HW * cg + 255) / 256;
  return (int)std::max<long>(1, std::min<long>(work, std::max<long>(1, 4096 / n)));
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
  constexpr int V = pm_elem<T>::V;
  const Plan pl = in_plan<T>(n, HW, C);
  with_gpr(pl.gpr, [&](auto G) {
    constexpr int GPR = decltype(G)::value;
    hipLaunchKernelGGL((in_stats_partial<T, GPR>), dim3(n * pl.nb, pl.colblocks), dim3(GPR * RL), 0, st, x, xp, HW, C, pl.rows, pl.nb, ws);
  });
  hipLaunchKernelGGL((in_stats_final<T>), dim3(n * pm_cdiv(C, FC)), dim3(FC * FL), 0, st, (const float*)ws, pl.nb, x, xp, HW, C, eps, mean, invstd);
  const int cg = C / V;
  const bool fixed = fixed_ok(cg);
  const int bpi = apply_bpi(n, HW, cg, fixed);
#define IN_APPLY(F, R) hipLaunchKernelGGL((in_apply_kernel<T, F, R>), dim3(n * bpi), dim3(256), 0, st, x, xp, y, yp, HW, C, bpi, mean, invstd, gamma, beta)
  if (fixed && relu) IN_APPLY(true, true);
  else if (fixed) IN_APPLY(true, false);
  else if (relu) IN_APPLY(false, true);
  else IN_APPLY(false, false);
#undef IN_APPLY
  return pm_check_launch(who);
}

template <typename T>
int in_bwd(const char* who, const T* dy, const T* x, const T* y, T* dx, int n, long HW, int C, long dp, long xp, long yp, long dxp, const float* gamma,
           const float* mean, const float* invstd, int relu, float* dgamma, float* dbeta, float* ws, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  const Plan pl = in_plan<T>(n, HW, C);
  float* sums = ws + (size_t)n * pl.nb * C * 2;
  with_gpr(pl.gpr, [&](auto G) {
    constexpr int GPR = decltype(G)::value;
    if (relu)
      hipLaunchKernelGGL((in_bwd_partial<T, GPR, true>), dim3(n * pl.nb, pl.colblocks), dim3(GPR * RL), 0, st, dy, dp, x, xp, y, yp, mean, invstd, HW, C, pl.rows,
                         pl.nb, ws);
    else
      hipLaunchKernelGGL((in_bwd_partial<T, GPR, false>), dim3(n * pl.nb, pl.colblocks), dim3(GPR * RL), 0, st, dy, dp, x, xp, y, yp, mean, invstd, HW, C, pl.rows,
                         pl.nb, ws);
  });
  hipLaunchKernelGGL(in_bwd_final, dim3(n * pm_cdiv(C, FC)), dim3(FC * FL), 0, st, (const float*)ws, pl.nb, C, sums);
  const int cg = C / V;
  const bool fixed = fixed_ok(cg);
  const int bpi = apply_bpi(n, HW, cg, fixed);
  const float inv_hw = 1.f / (float)HW;
#define IN_BAPPLY(F, R) \
  hipLaunchKernelGGL((in_bwd_apply_kernel<T, F, R>), dim3(n * bpi), dim3(256), 0, st, dy, dp, x, xp, y, yp, dx, dxp, HW, C, bpi, inv_hw, mean, invstd, gamma, (const float*)sums, n, dgamma, dbeta)
  if (fixed && relu) IN_BAPPLY(true, true);
  else if (fixed) IN_BAPPLY(true, false);
  else if (relu) IN_BAPPLY(false, true);
  else IN_BAPPLY(false, false);
#undef IN_BAPPLY
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
