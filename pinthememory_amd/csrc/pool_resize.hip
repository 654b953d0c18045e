// K3/K5: max-pool 3x3 s2 p1, global average pool, bilinear resize (align_corners=True) over NHWC activations of both tiers, HBM-bound.
// Replaces nn.MaxPool2d(3,2,1) (/root/reference/network/Resnet.py:432), nn.AdaptiveAvgPool2d(1) (deepv3plus.py:85)
// and mynn.Upsample (mynn.py:57-62). Backward passes are gathers (no atomics): deterministic.
// One kernel template per pass for fp32 and bf16 tensors (pm_elem<T>, pm_common.h): a lane moves 16 bytes = V channels (4 floats / 8 bf16), values travel as float[V],
// every accumulator is fp32, bf16 results are rounded once on the way out. V = 1 instantiates the same bodies for fp32 views that are no 16-byte vectors (the 19 class
// logits on a dense pitch); the bf16 tier has no scalar form. One host function per entry point does the view checks and launches; the extern "C" function keeps the
// null / shape checks and selects T once (BY_DTYPE). The eval-only kernels at the bottom (half-pixel resize, softmax mean, stitch, argmax) are fp32.
#include <type_traits>

#include "pm_common.h"

namespace {

// ---- max pool ------------------------------------------------------------------------------------------------------------------------------------
// thread = (output pixel, V channels). The argmax bytes leave as one 8-byte store on the bf16 tier and byte by byte on fp32, which takes any argmax alignment.
// BN (fp32 vectors only): x is a raw convolution output and every tap is relu(bn(x)) -- normalised and clamped BEFORE the comparison, so values, argmax bytes and
// the ties among clamped zeros are those of pooling the stored activation, which is never written (the stem, Resnet.py:471-478).
template <typename T, bool BN = false, int V = pm_elem<T>::V>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, long xp, int H, int W, T* __restrict__ y, long yp, int Ho, int Wo, int C, long total,
                                                          uint8_t* __restrict__ arg, const float* __restrict__ mean = nullptr, const float* __restrict__ invstd = nullptr,
                                                          const float* __restrict__ gamma = nullptr, const float* __restrict__ beta = nullptr) {
  static_assert(!BN || (V == 4 && sizeof(T) == 4), "the normalising form is fp32 and vectorised");
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long op = i / cg;
    const int ch = (int)(i - op * cg) * V;
    const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), n = (int)(op / ((long)Wo * Ho));
    float best[V];
    std::conditional_t<V == 8, unsigned, uint8_t> bi[V];      // the parent forms' types: as unsigned the fp32 vector form takes 36 VGPRs instead of 34, as bytes the bf16 form 180 instructions more
#pragma unroll
    for (int e = 0; e < V; ++e) best[e] = -INFINITY, bi[e] = 0;
    float4 mu, is, ga, be;      // float4 members, not float[V]: as arrays the normalising form takes 54 VGPRs instead of 46
    if constexpr (BN) mu = PM_LD4(mean + ch), is = PM_LD4(invstd + ch), ga = PM_LD4(gamma + ch), be = PM_LD4(beta + ch);
    bool first = true;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        if ((unsigned)ix >= (unsigned)W) continue;
        float v[V];
        pm_ldv<T, V>(x + ((long)(n * H + iy) * W + ix) * xp + ch, v);
        if constexpr (BN) {
          v[0] = fmaxf(pm_bn_affine(v[0], mu.x, is.x, ga.x, be.x), 0.f), v[1] = fmaxf(pm_bn_affine(v[1], mu.y, is.y, ga.y, be.y), 0.f);
          v[2] = fmaxf(pm_bn_affine(v[2], mu.z, is.z, ga.z, be.z), 0.f), v[3] = fmaxf(pm_bn_affine(v[3], mu.w, is.w, ga.w, be.w), 0.f);
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (first || v[e] > best[e] || v[e] != v[e]) best[e] = v[e], bi[e] = (uint8_t)(ky * 3 + kx);
        first = false;
      }
    }
    pm_stv<T, V>(y + op * yp + ch, best);      // exact on bf16: the maximum is one of the inputs
    uint8_t* a = arg + op * C + ch;
    if constexpr (V == 8) {
      *reinterpret_cast<uint2*>(a) = make_uint2(bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24), bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24));
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) a[e] = bi[e];
    }
  }
}

// thread = (input pixel, V channels): pm_maxpool_gather
template <typename T, int V = pm_elem<T>::V>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dy, long dp, int Ho, int Wo, const uint8_t* __restrict__ arg, T* __restrict__ dx, long xp,
                                                          int H, int W, int C, long total) {
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long ip = i / cg;
    const int ch = (int)(i - ip * cg) * V;
    float g[V];
    pm_maxpool_gather<T, V>(dy, dp, Ho, Wo, arg, H, W, C, ip, ch, g);
    pm_stv<T, V>(dx + ip * xp + ch, g);
  }
}

// ---- global average pool (and the column sum of the 1x1-source resize backward) ------------------------------------------------------------------
// block = one image x 16 V channels: 16 lane groups x 16 row lanes, four independent partial sums per lane -- four 16 B loads in flight per thread (one block per CU
// has little else to hide latency with); the 16 row lanes are folded through LDS in row-lane order
template <typename T>
__global__ __launch_bounds__(256) void gap_fwd_kernel(const T* __restrict__ x, long xp, long HW, int C, T* __restrict__ y, long yp, float scale, int accumulate) {
  constexpr int V = pm_elem<T>::V, CB = 16 * V;
  __shared__ float sm[16][CB];
  const int g = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.y * CB + g * V, n = blockIdx.x;
  float s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  if (c < C) {
    float a[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) a[u][j] = 0.f;
    const T* base = x + (long)n * HW * xp + c;
    long p = r;
    for (; p + 48 < HW; p += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[V];
        pm_elem<T>::ld(base + (p + 16 * u) * xp, v);
#pragma unroll
        for (int j = 0; j < V; ++j) a[u][j] += v[j];
      }
    }
    for (; p < HW; p += 16) {
      float v[V];
      pm_elem<T>::ld(base + p * xp, v);
#pragma unroll
      for (int j = 0; j < V; ++j) a[0][j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = (a[0][j] + a[1][j]) + (a[2][j] + a[3][j]);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) sm[r][g * V + j] = s[j];
  __syncthreads();
  if (threadIdx.x < CB) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sm[i][threadIdx.x];
    const int ch = blockIdx.y * CB + threadIdx.x;
    if (ch < C) {
      T* o = y + (long)n * yp + ch;
      *o = pm_elem<T>::narrow((accumulate ? pm_elem<T>::widen(*o) : 0.f) + t * scale);
    }
  }
}

// ---- bilinear, align_corners=True ------------------------------------------------------------------------------------------------------------------
template <typename T, int V = pm_elem<T>::V>
__global__ __launch_bounds__(256) void resize_fwd_kernel(const T* __restrict__ x, long xp, int h, int w, T* __restrict__ y, long yp, int H, int W, int C, long total,
                                                         float sy, float sx) {
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long op = i / cg;
    const int ch = (int)(i - op * cg) * V;
    const int X = (int)(op % W), Y = (int)((op / W) % H), n = (int)(op / ((long)W * H));
    const pm_lerp ly = pm_ac_lerp(sy, Y, h), lx = pm_ac_lerp(sx, X, w);
    const T* r0 = x + ((long)(n * h + ly.i0) * w) * xp + ch;
    const T* r1 = x + ((long)(n * h + ly.i1) * w) * xp + ch;
#define LERP(a, b, c, d) (ly.w0 * (lx.w0 * (a) + lx.w1 * (b)) + ly.w1 * (lx.w0 * (c) + lx.w1 * (d)))
    if constexpr (V == 4) {      // float4 members, not float[4]: over the array the compiler contracts the upper row's two products the other way round (other bits)
      const float4 a = PM_LD4(r0 + lx.i0 * xp), b = PM_LD4(r0 + lx.i1 * xp), c = PM_LD4(r1 + lx.i0 * xp), d = PM_LD4(r1 + lx.i1 * xp);
      float4 o;
      o.x = LERP(a.x, b.x, c.x, d.x), o.y = LERP(a.y, b.y, c.y, d.y), o.z = LERP(a.z, b.z, c.z, d.z), o.w = LERP(a.w, b.w, c.w, d.w);
      PM_ST4(y + op * yp + ch, o);
    } else {
      float a[V], b[V], c[V], d[V], o[V];
      pm_ldv<T, V>(r0 + lx.i0 * xp, a), pm_ldv<T, V>(r0 + lx.i1 * xp, b), pm_ldv<T, V>(r1 + lx.i0 * xp, c), pm_ldv<T, V>(r1 + lx.i1 * xp, d);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = LERP(a[e], b[e], c[e], d[e]);
      pm_stv<T, V>(y + op * yp + ch, o);
    }
#undef LERP
  }
}

// g[e] += w * q[e]: the one accumulation statement of every backward pass below
template <int V>
__device__ __forceinline__ void axpy(float w, const float* q, float* g) {
#pragma unroll
  for (int e = 0; e < V; ++e) g[e] += w * q[e];
}
// dx (+)= g, rounded once
template <typename T, int V>
__device__ __forceinline__ void store_grad(T* o, float* g, int accumulate) {
  if (accumulate) {
    float q[V];
    pm_ldv<T, V>(o, q);
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] += q[e];
  }
  pm_stv<T, V>(o, g);
}

// Gather formulation of the backward (any ratio): each input pixel sums the output pixels whose bilinear taps touch it, in ascending order. CACHED: the per-row /
// per-column tap weights of a support window of at most MAXT x MAXT are computed once into registers, so the inner loops are pure load + FMA; larger windows (the
// 1x1 -> HxW broadcast of the ASPP image feature) and CACHED = false take the generic loop. Both add the same products in the same order.
template <typename T, int V, bool CACHED>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const T* __restrict__ dy, long dp, int H, int W, T* __restrict__ dx, long xp, int h, int w, int C, long total,
                                                         float sy, float sx, int accumulate) {
  constexpr int MAXT = 14;
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long ip = i / cg;
    const int ch = (int)(i - ip * cg) * V;
    const int x = (int)(ip % w), y = (int)((ip / w) % h), n = (int)(ip / ((long)w * h));
    int ylo, yhi, xlo, xhi;
    pm_support(sy, y, H, ylo, yhi);
    pm_support(sx, x, W, xlo, xhi);
    float g[V];
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    if (CACHED && yhi - ylo < MAXT && xhi - xlo < MAXT) {
      if constexpr (CACHED) {
        float wyv[MAXT], wxv[MAXT];
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
          wyv[k] = ylo + k <= yhi ? pm_tap_weight(pm_ac_lerp(sy, ylo + k, h), y) : 0.f;
          wxv[k] = xlo + k <= xhi ? pm_tap_weight(pm_ac_lerp(sx, xlo + k, w), x) : 0.f;
        }
        const T* base = dy + ((long)(n * H + ylo) * W + xlo) * dp + ch;
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
          if (wyv[k] == 0.f) continue;
#pragma unroll
          for (int l = 0; l < MAXT; ++l) {
            if (wxv[l] == 0.f) continue;
            float q[V];
            pm_ldv<T, V>(base + ((long)k * W + l) * dp, q);
            axpy<V>(wyv[k] * wxv[l], q, g);
          }
        }
      }
    } else {
      for (int Y = ylo; Y <= yhi; ++Y) {
        const float wy = pm_tap_weight(pm_ac_lerp(sy, Y, h), y);
        if (wy == 0.f) continue;
        for (int X = xlo; X <= xhi; ++X) {
          const float wx = pm_tap_weight(pm_ac_lerp(sx, X, w), x);
          if (wx == 0.f) continue;
          float q[V];
          pm_ldv<T, V>(dy + ((long)(n * H + Y) * W + X) * dp + ch, q);
          axpy<V>(wy * wx, q, g);
        }
      }
    }
    store_grad<T, V>(dx + ip * xp + ch, g, accumulate);
  }
}

// Separable backward for up-sampling ratios >= 2: the transposed operator factorises into a column pass and a row pass, so the large gradient dy is read ONCE (the
// gather above re-reads every hi-res pixel from the ~4 low-res pixels whose support covers it: 873 MB of traffic for the 302 MB fp32 decoder gradient).
//   pass 1  T[n, Y, x, c] = sum_X wx(X, x) * dy[n, Y, X, c]        (thread = (n, Y, x, V channels), <= 14 taps; T is an fp32 workspace on both tiers)
//   pass 2  dx[n, y, x, c] (+)= sum_Y wy(Y, y) * T[n, Y, x, c]
// Both sums run in ascending index order: deterministic.
template <typename T>
__global__ __launch_bounds__(256) void resize_bwd_cols_kernel(const T* __restrict__ dy, long dp, int H, int W, float* __restrict__ ws, int w, int C, long total, float sx) {
  constexpr int V = pm_elem<T>::V;
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long ip = i / cg;
    const int ch = (int)(i - ip * cg) * V;
    const int x = (int)(ip % w);
    const long row = ip / w;   // n * H + Y
    int xlo, xhi;
    pm_support(sx, x, W, xlo, xhi);
    float g[V];
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    const T* base = dy + (row * W) * dp + ch;
    for (int X = xlo; X <= xhi; ++X) {
      const float wx = pm_tap_weight(pm_ac_lerp(sx, X, w), x);
      if (wx == 0.f) continue;
      float q[V];
      pm_elem<T>::ld(base + (long)X * dp, q);
      axpy<V>(wx, q, g);
    }
    pm_stp<V>(ws + ip * C + ch, g);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void resize_bwd_rows_kernel(const float* __restrict__ ws, int H, T* __restrict__ dx, long xp, int h, int w, int C, long total, float sy,
                                                              int accumulate) {
  constexpr int V = pm_elem<T>::V;
  const int cg = C / V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long ip = i / cg;
    const int ch = (int)(i - ip * cg) * V;
    const int x = (int)(ip % w), y = (int)((ip / w) % h), n = (int)(ip / ((long)w * h));
    int ylo, yhi;
    pm_support(sy, y, H, ylo, yhi);
    float g[V];
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    for (int Y = ylo; Y <= yhi; ++Y) {
      const float wy = pm_tap_weight(pm_ac_lerp(sy, Y, h), y);
      if (wy == 0.f) continue;
      float q[V];
      pm_ldp<V>(ws + (((long)n * H + Y) * w + x) * C + ch, q);
      axpy<V>(wy, q, g);
    }
    store_grad<T, V>(dx + ip * xp + ch, g, accumulate);
  }
}

// F.interpolate(..., mode='bilinear') with align_corners=False as ATen computes it: scale = in/out (float),
// src = scale * (dst + 0.5) - 0.5 clamped at 0, i0 = floor(src), i1 = i0 + (i0 < in-1), lambda = src - i0.
__device__ __forceinline__ pm_lerp hp_lerp(float scale, int dst, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  pm_lerp r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  float l1 = src - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  r.w1 = l1;
  r.w0 = 1.f - l1;
  return r;
}
__global__ __launch_bounds__(256) void resize_hp_fwd_kernel(const float* __restrict__ x, long xp, int h, int w, float* __restrict__ y, long yp, int H, int W,
                                                            int C, long total, float sy, float sx, int flip_w) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long op = i / C;
    const int ch = (int)(i - op * C);
    const int X = (int)(op % W), Y = (int)((op / W) % H), n = (int)(op / ((long)W * H));
    const pm_lerp ly = hp_lerp(sy, Y, h), lx = hp_lerp(sx, X, w);
    const float* r0 = x + ((long)(n * h + ly.i0) * w) * xp + ch;
    const float* r1 = x + ((long)(n * h + ly.i1) * w) * xp + ch;
    const float v = ly.w0 * (lx.w0 * r0[lx.i0 * xp] + lx.w1 * r0[lx.i1 * xp]) + ly.w1 * (lx.w0 * r1[lx.i0 * xp] + lx.w1 * r1[lx.i1 * xp]);
    const int Xo = flip_w ? W - 1 - X : X;   // un-flip on the way out (eval.py:330 flip_tensor2(y, -1))
    y[((long)(n * H + Y) * W + Xo) * yp + ch] = v;
  }
}
// one thread per pixel: softmax over C <= 32 classes in fp32 (as torch.softmax on fp32 logits), running mean in fp64
__global__ __launch_bounds__(256) void softmax_mean_kernel(const float* __restrict__ lg, long lp, long pixels, int C, double* __restrict__ buf, double inv_cnt) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long)gridDim.x * 256) {
    float v[32];
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) v[c] = lg[p * lp + c], mx = fmaxf(mx, v[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) v[c] = expf(v[c] - mx), se += v[c];
    for (int c = 0; c < C; ++c) {
      const double pr = (double)(v[c] / se), b = buf[p * C + c];
      buf[p * C + c] = b + (pr - b) * inv_cnt;
    }
  }
}
__global__ __launch_bounds__(256) void argmax_f64_kernel(const double* __restrict__ buf, long pixels, int C, int64_t* __restrict__ cls, double* __restrict__ prob) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long)gridDim.x * 256) {
    double best = buf[p * C];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const double v = buf[p * C + c];
      if (v > best) best = v, bi = c;             // first maximum wins, as torch.max
    }
    cls[p] = bi;
    if (prob) prob[p] = best;
  }
}

// ---- host side: one function per entry point, both element types --------------------------------------------------------------------------------------
// both tensors bf16 -> f<pm_bf16>; otherwise both have to be fp32 (a mixed-type call ends here with PM_EUNSUPPORTED) -> f<float>
#define BY_DTYPE(a, b, who, f, ...)                                 \
  do {                                                              \
    if (pm_is_bf16(a) && pm_is_bf16(b)) return f<pm_bf16>(__VA_ARGS__); \
    PM_REQUIRE_F32(a, who);                                         \
    PM_REQUIRE_F32(b, who);                                         \
    return f<float>(__VA_ARGS__);                                   \
  } while (0)
#define LAUNCH(kernel, work, st, ...) hipLaunchKernelGGL((kernel), dim3(pm_grid_for(work)), dim3(256), 0, st, __VA_ARGS__)

template <typename T>
constexpr bool has_scalar_form = pm_elem<T>::V == 4;      // fp32 views that are no 16-byte vectors run the V = 1 instantiations; a bf16 view has to be a vector view

template <typename T>
int maxpool_fwd(const pm_tensor* x, const pm_tensor* y, uint8_t* argmax, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  const bool vec = pm_elem<T>::vec(x) && pm_elem<T>::vec(y);
  const T* px = (const T*)x->ptr;
  T* py = (T*)y->ptr;
  if constexpr (has_scalar_form<T>) {      // any argmax alignment: the bytes are stored one by one
    if (!vec) {
      const long total = pm_pixels(y) * y->c;
      LAUNCH((maxpool_fwd_kernel<T, false, 1>), total, st, px, (long)x->pitch, x->h, x->w, py, (long)y->pitch, y->h, y->w, y->c, total, argmax);
      return pm_check_launch("maxpool_fwd");
    }
  } else {
    PM_REQUIRE(vec && (reinterpret_cast<uintptr_t>(argmax) & 7u) == 0, PM_EINVAL, "maxpool_fwd: bf16 tensors need 16-byte views and an 8-byte aligned argmax");
  }
  const long total = pm_pixels(y) * (y->c / V);
  LAUNCH((maxpool_fwd_kernel<T>), total, st, px, (long)x->pitch, x->h, x->w, py, (long)y->pitch, y->h, y->w, y->c, total, argmax);
  return pm_check_launch("maxpool_fwd");
}

template <typename T>
int maxpool_bwd(const pm_tensor* dy, const uint8_t* argmax, const pm_tensor* dx, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;      // the V argmax bytes of a lane come as one load: V-byte aligned argmax
  const bool vec = pm_elem<T>::vec(dy) && pm_elem<T>::vec(dx) && (reinterpret_cast<uintptr_t>(argmax) & (V - 1)) == 0;
  const T* pd = (const T*)dy->ptr;
  T* px = (T*)dx->ptr;
  if constexpr (has_scalar_form<T>) {
    if (!vec) {
      const long total = pm_pixels(dx) * dx->c;
      LAUNCH((maxpool_bwd_kernel<T, 1>), total, st, pd, (long)dy->pitch, dy->h, dy->w, argmax, px, (long)dx->pitch, dx->h, dx->w, dx->c, total);
      return pm_check_launch("maxpool_bwd");
    }
  } else {
    PM_REQUIRE(vec, PM_EINVAL, "maxpool_bwd: bf16 tensors need 16-byte views and an 8-byte aligned argmax");
  }
  const long total = pm_pixels(dx) * (dx->c / V);
  LAUNCH((maxpool_bwd_kernel<T>), total, st, pd, (long)dy->pitch, dy->h, dy->w, argmax, px, (long)dx->pitch, dx->h, dx->w, dx->c, total);
  return pm_check_launch("maxpool_bwd");
}

// y[n, c] (+)= scale * sum over the pixels of x[n, :, :, c]
template <typename T>
int column_sum(const char* who, const pm_tensor* x, const pm_tensor* y, float scale, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(gap_fwd_kernel<T>, dim3(x->n, pm_cdiv(x->c, 16 * pm_elem<T>::V)), dim3(256), 0, st, (const T*)x->ptr, (long)x->pitch, (long)x->h * x->w, x->c,
                     (T*)y->ptr, (long)y->pitch, scale, accumulate);
  return pm_check_launch(who);
}
template <typename T>
int gap_fwd(const pm_tensor* x, const pm_tensor* y, hipStream_t st) {
  PM_REQUIRE(pm_elem<T>::vec(x), PM_EINVAL, "global_avgpool_fwd: bad args");
  return column_sum<T>("global_avgpool_fwd", x, y, 1.f / (float)((long)x->h * x->w), 0, st);
}

template <typename T>
int gap_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  // the fp32 pass reads dy channel by channel and takes any dy row; the bf16 pass reads it as 16-byte vectors
  PM_REQUIRE(pm_elem<T>::vec(dx) && (has_scalar_form<T> || (pm_aligned16(dy->ptr) && dy->pitch % V == 0)), PM_EINVAL, "global_avgpool_bwd: bad args");
  const T* pd = (const T*)dy->ptr;
  T* px = (T*)dx->ptr;
  const long dp = dy->pitch, xp = dx->pitch, HW = (long)dx->h * dx->w;
  const float inv = 1.f / (float)HW;
  return pm_ew_launch_as<T>(pm_pixels(dx), dx->c, st, "global_avgpool_bwd", [=] __device__(long p, int ch) {
    const long n = p / HW;
    float o[V], d[V];
    if (accumulate) pm_elem<T>::ld(px + p * xp + ch, o);
    else {
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = 0.f;
    }
    if constexpr (has_scalar_form<T>) {
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = pd[n * dp + ch + e];
    } else {
      pm_elem<T>::ld(pd + n * dp + ch, d);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] += d[e] * inv;
    pm_elem<T>::st(px + p * xp + ch, o);
  });
}

template <typename T>
int resize_fwd(const pm_tensor* x, const pm_tensor* y, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  const float sy = pm_ac_scale(x->h, y->h), sx = pm_ac_scale(x->w, y->w);
  const T* px = (const T*)x->ptr;
  T* py = (T*)y->ptr;
  int c = y->c;
  if constexpr (has_scalar_form<T>) {
    // channel counts that are not a multiple of 4 (the 19 class logits) on pitch-padded views: run the float4 path over the padded width -- the pad lanes of
    // the input are zero (kernels.new), so the pad lanes of the output are written as zero. Padded lanes only when they are the views' own.
    const int cv = (x->c + 3) & ~3;
    if (!(pm_vec_ok(x) && pm_vec_ok(y) && (x->c % 4 == 0 || (x->pitch == cv && y->pitch == cv)))) {
      const long total = pm_pixels(y) * c;
      LAUNCH((resize_fwd_kernel<T, 1>), total, st, px, (long)x->pitch, x->h, x->w, py, (long)y->pitch, y->h, y->w, c, total, sy, sx);
      return pm_check_launch("resize_fwd");
    }
    c = cv;
  } else {
    PM_REQUIRE(pm_elem<T>::vec(x) && pm_elem<T>::vec(y), PM_EINVAL, "resize_fwd: bf16 tensors need 16-byte views");
  }
  const long total = pm_pixels(y) * (c / V);
  LAUNCH((resize_fwd_kernel<T>), total, st, px, (long)x->pitch, x->h, x->w, py, (long)y->pitch, y->h, y->w, c, total, sy, sx);
  return pm_check_launch("resize_fwd");
}

// The register-cached tap window of the gather: fp32 has it on both of its forms. bf16 instantiates the generic loop alone (profiles/pool_resource_usage.txt).
template <typename T>
constexpr bool cached_window = has_scalar_form<T>;

template <typename T>
int resize_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  const bool vec = pm_elem<T>::vec(dy) && pm_elem<T>::vec(dx);
  const float sy = pm_ac_scale(dx->h, dy->h), sx = pm_ac_scale(dx->w, dy->w);
  const T* pd = (const T*)dy->ptr;
  T* px = (T*)dx->ptr;
  if constexpr (has_scalar_form<T>) {
    if (!vec) {
      const long total = pm_pixels(dx) * dx->c;
      LAUNCH((resize_bwd_kernel<T, 1, cached_window<T>>), total, st, pd, (long)dy->pitch, dy->h, dy->w, px, (long)dx->pitch, dx->h, dx->w, dx->c, total, sy, sx, accumulate);
      return pm_check_launch("resize_bwd");
    }
  } else {
    PM_REQUIRE(vec, PM_EINVAL, "resize_bwd: bf16 tensors need 16-byte views");
  }
  if (dx->h == 1 && dx->w == 1)      // 1x1 source (ASPP image feature): every output pixel has weight 1 -> a plain column sum
    return column_sum<T>("resize_bwd(1x1)", dy, dx, 1.f, accumulate, st);
  const long total = pm_pixels(dx) * (dx->c / V);
  LAUNCH((resize_bwd_kernel<T, V, cached_window<T>>), total, st, pd, (long)dy->pitch, dy->h, dy->w, px, (long)dx->pitch, dx->h, dx->w, dx->c, total, sy, sx, accumulate);
  return pm_check_launch("resize_bwd");
}

// workspace of the separable backward (0: shape not eligible -> use pm_resize_bilinear_bwd)
template <typename T>
size_t resize_bwd_workspace(const pm_tensor* dy, const pm_tensor* dx) {
  if (!pm_elem<T>::vec(dy) || !pm_elem<T>::vec(dx) || dx->h < 2 || dx->w < 2 || dy->h < 2 * dx->h || dy->w < 2 * dx->w) return 0;
  return pm_align_up((size_t)dy->n * dy->h * dx->w * dy->c * sizeof(float), 256);
}
template <typename T>
int resize_bwd_separable(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* ws, size_t ws_bytes, hipStream_t st) {
  constexpr int V = pm_elem<T>::V;
  const size_t need = resize_bwd_workspace<T>(dy, dx);
  PM_REQUIRE(need > 0, PM_EUNSUPPORTED, "resize_bwd_separable: needs 16-byte channel vectors and an up-sampling ratio >= 2 in both directions");
  PM_REQUIRE(ws && ws_bytes >= need, PM_EWORKSPACE, "resize_bwd_separable: workspace %zu < %zu", ws_bytes, need);
  const float sy = pm_ac_scale(dx->h, dy->h), sx = pm_ac_scale(dx->w, dy->w);
  const long t1 = (long)dy->n * dy->h * dx->w * (dy->c / V), t2 = pm_pixels(dx) * (dx->c / V);
  LAUNCH(resize_bwd_cols_kernel<T>, t1, st, (const T*)dy->ptr, (long)dy->pitch, dy->h, dy->w, (float*)ws, dx->w, dy->c, t1, sx);
  LAUNCH(resize_bwd_rows_kernel<T>, t2, st, (const float*)ws, dy->h, (T*)dx->ptr, (long)dx->pitch, dx->h, dx->w, dx->c, t2, sy, accumulate);
  return pm_check_launch("resize_bwd_separable");
}

}  // namespace

extern "C" int pm_maxpool3x3s2_fwd(const pm_tensor* x, const pm_tensor* y, uint8_t* argmax, void* stream) {
  PM_REQUIRE(x && y && argmax && x->ptr && y->ptr, PM_EINVAL, "maxpool_fwd: null");
  PM_REQUIRE(y->h == (x->h + 2 - 3) / 2 + 1 && y->w == (x->w + 2 - 3) / 2 + 1 && x->n == y->n && x->c == y->c, PM_EINVAL, "maxpool_fwd: shape mismatch");
  BY_DTYPE(x, y, "maxpool_fwd", maxpool_fwd, x, y, argmax, (hipStream_t)stream);
}

// pm_maxpool3x3s2_fwd of relu(bn(x)) for a raw convolution output x: the normalised activation is evaluated per tap and never stored. fp32, c % 4 == 0.
extern "C" int pm_maxpool3x3s2_bn_relu_fwd(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* y,
                                           uint8_t* argmax, void* stream) {
  PM_REQUIRE(x && y && argmax && x->ptr && y->ptr && mean && invstd && gamma && beta, PM_EINVAL, "maxpool_bn_relu_fwd: null");
  PM_REQUIRE(y->h == (x->h + 2 - 3) / 2 + 1 && y->w == (x->w + 2 - 3) / 2 + 1 && x->n == y->n && x->c == y->c, PM_EINVAL, "maxpool_bn_relu_fwd: shape mismatch");
  PM_REQUIRE_F32(x, "maxpool_bn_relu_fwd"); PM_REQUIRE_F32(y, "maxpool_bn_relu_fwd");
  PM_REQUIRE(pm_vec4(x) && pm_vec4(y), PM_EINVAL, "maxpool_bn_relu_fwd: tensors must be 16B aligned with pitch %% 4 == 0 and c %% 4 == 0");
  const long total = pm_pixels(y) * y->c / 4;
  if (total == 0) return PM_OK;
  LAUNCH((maxpool_fwd_kernel<float, true>), total, (hipStream_t)stream, (const float*)x->ptr, (long)x->pitch, x->h, x->w, (float*)y->ptr, (long)y->pitch, y->h, y->w, x->c,
         total, argmax, mean, invstd, gamma, beta);
  return pm_check_launch("maxpool_bn_relu_fwd");
}

extern "C" int pm_maxpool3x3s2_bwd(const pm_tensor* dy, const uint8_t* argmax, const pm_tensor* dx, void* stream) {
  PM_REQUIRE(dy && dx && argmax && dy->ptr && dx->ptr && dy->n == dx->n && dy->c == dx->c, PM_EINVAL, "maxpool_bwd: bad args");
  BY_DTYPE(dy, dx, "maxpool_bwd", maxpool_bwd, dy, argmax, dx, (hipStream_t)stream);
}

extern "C" int pm_global_avgpool_fwd(const pm_tensor* x, const pm_tensor* y, void* stream) {
  PM_REQUIRE(x && y && y->ptr && y->h == 1 && y->w == 1 && y->n == x->n && y->c == x->c, PM_EINVAL, "global_avgpool_fwd: bad args");
  BY_DTYPE(x, y, "global_avgpool_fwd", gap_fwd, x, y, (hipStream_t)stream);
}

extern "C" int pm_global_avgpool_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* stream) {
  PM_REQUIRE(dy && dx && dy->ptr && dy->h == 1 && dy->w == 1 && dy->n == dx->n && dy->c == dx->c, PM_EINVAL, "global_avgpool_bwd: bad args");
  BY_DTYPE(dy, dx, "global_avgpool_bwd", gap_bwd, dy, dx, accumulate, (hipStream_t)stream);
}

extern "C" int pm_resize_bilinear_fwd(const pm_tensor* x, const pm_tensor* y, void* stream) {
  PM_REQUIRE(x && y && x->ptr && y->ptr && x->n == y->n && x->c == y->c, PM_EINVAL, "resize_fwd: bad args");
  BY_DTYPE(x, y, "resize_fwd", resize_fwd, x, y, (hipStream_t)stream);
}

extern "C" int pm_resize_bilinear_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* stream) {
  PM_REQUIRE(dy && dx && dy->ptr && dx->ptr && dy->n == dx->n && dy->c == dx->c, PM_EINVAL, "resize_bwd: bad args");
  BY_DTYPE(dy, dx, "resize_bwd", resize_bwd, dy, dx, accumulate, (hipStream_t)stream);
}

extern "C" size_t pm_resize_bilinear_bwd_workspace(const pm_tensor* dy, const pm_tensor* dx) {
  if (!dy || !dx) return 0;
  if (pm_is_bf16(dy) && pm_is_bf16(dx)) return resize_bwd_workspace<pm_bf16>(dy, dx);
  return pm_is_f32(dy) && pm_is_f32(dx) ? resize_bwd_workspace<float>(dy, dx) : 0;
}
extern "C" int pm_resize_bilinear_bwd_separable(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(dy && dx && dy->ptr && dx->ptr && dy->n == dx->n && dy->c == dx->c, PM_EINVAL, "resize_bwd_separable: bad args");
  BY_DTYPE(dy, dx, "resize_bwd_separable", resize_bwd_separable, dy, dx, accumulate, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pm_resize_bilinear_hp_fwd(const pm_tensor* x, const pm_tensor* y, int flip_w, void* stream) {
  PM_REQUIRE(x && y && x->ptr && y->ptr && x->n == y->n && x->c == y->c, PM_EINVAL, "resize_hp_fwd: bad args");
  PM_REQUIRE_F32(x, "resize_hp_fwd"); PM_REQUIRE_F32(y, "resize_hp_fwd");
  const long total = pm_pixels(y) * y->c;
  hipLaunchKernelGGL(resize_hp_fwd_kernel, dim3(pm_grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x->ptr, (long)x->pitch, x->h, x->w,
                     (float*)y->ptr, (long)y->pitch, y->h, y->w, y->c, total, (float)x->h / (float)y->h, (float)x->w / (float)y->w, flip_w);
  return pm_check_launch("resize_hp_fwd");
}
extern "C" int pm_softmax_mean_update(const pm_tensor* logits, double* buffer, int counter, void* stream) {
  PM_REQUIRE(logits && logits->ptr && buffer && counter >= 1 && logits->c >= 1 && logits->c <= 32, PM_EINVAL, "softmax_mean_update: bad args");
  PM_REQUIRE_F32(logits, "softmax_mean_update");
  const long pixels = pm_pixels(logits);
  hipLaunchKernelGGL(softmax_mean_kernel, dim3(pm_grid_for(pixels)), dim3(256), 0, (hipStream_t)stream, (const float*)logits->ptr, (long)logits->pitch, pixels,
                     logits->c, buffer, 1.0 / (double)counter);
  return pm_check_launch("softmax_mean_update");
}
namespace {
// Sliding-window stitching (eval.py:210-274: add the tiles' logits, divide by the per-pixel tile count, un-flip; the reference does it per
// class in numpy threads on the host). One thread per output pixel: float64 sum over the covering tiles in tile order, / count, written to
// the class-major float64 accumulator at the (un-flipped) column; `accumulate` adds to what an earlier flip / scale left there.
constexpr int STITCH_MAX_TILES = 64;
struct StitchTiles {
  int n;
  int x1[STITCH_MAX_TILES], y1[STITCH_MAX_TILES], x2[STITCH_MAX_TILES], y2[STITCH_MAX_TILES];
};
__global__ __launch_bounds__(256) void sliding_stitch_kernel(const float* __restrict__ lg, long pitch, int th, int tw, int C, const StitchTiles tiles, int H, int W,
                                                             int flip, double* __restrict__ acc, int accumulate) {
  const long total = (long)H * W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const int xo = flip ? W - 1 - x : x;
    double cnt = 0.0;
    for (int t = 0; t < tiles.n; ++t)
      if (x >= tiles.x1[t] && x < tiles.x2[t] && y >= tiles.y1[t] && y < tiles.y2[t]) cnt += 1.0;
    for (int c = 0; c < C; ++c) {
      double s = 0.0;
      for (int t = 0; t < tiles.n; ++t)
        if (x >= tiles.x1[t] && x < tiles.x2[t] && y >= tiles.y1[t] && y < tiles.y2[t])
          s += (double)lg[(((long)t * th + (y - tiles.y1[t])) * tw + (x - tiles.x1[t])) * pitch + c];
      const double v = s / cnt;          // uncovered pixels: 0 / 0 = NaN, as the host formulation gives
      double* dst = acc + ((long)c * H + y) * W + xo;
      *dst = accumulate ? *dst + v : v;
    }
  }
}

}  // namespace
extern "C" int pm_sliding_stitch(const pm_tensor* logits, const int32_t* tiles_xyxy, int ntiles, int H, int W, int flip_w, double* acc, int accumulate,
                                 void* stream) {
  PM_REQUIRE(logits && logits->ptr && tiles_xyxy && acc && ntiles >= 1 && ntiles <= STITCH_MAX_TILES && logits->n == ntiles, PM_EINVAL,
             "sliding_stitch: bad args (1..%d tiles, logits->n == ntiles)", STITCH_MAX_TILES);
  PM_REQUIRE_F32(logits, "sliding_stitch");
  StitchTiles t;
  t.n = ntiles;
  for (int i = 0; i < ntiles; ++i) {
    t.x1[i] = tiles_xyxy[4 * i], t.y1[i] = tiles_xyxy[4 * i + 1], t.x2[i] = tiles_xyxy[4 * i + 2], t.y2[i] = tiles_xyxy[4 * i + 3];
    PM_REQUIRE(t.x2[i] - t.x1[i] == logits->w && t.y2[i] - t.y1[i] == logits->h && t.x1[i] >= 0 && t.y1[i] >= 0 && t.x2[i] <= W && t.y2[i] <= H, PM_EINVAL,
               "sliding_stitch: tile %d does not match the logits' %dx%d", i, logits->h, logits->w);
  }
  hipLaunchKernelGGL(sliding_stitch_kernel, dim3(pm_grid_for((long)H * W)), dim3(256), 0, (hipStream_t)stream, (const float*)logits->ptr, (long)logits->pitch, logits->h,
                     logits->w, logits->c, t, H, W, flip_w, acc, accumulate);
  return pm_check_launch("sliding_stitch");
}
extern "C" int pm_argmax_f64(const double* buffer, int n, int h, int w, int c, int64_t* out_cls, double* out_prob, void* stream) {
  PM_REQUIRE(buffer && out_cls && c >= 1, PM_EINVAL, "argmax_f64: bad args");
  const long pixels = (long)n * h * w;
  hipLaunchKernelGGL(argmax_f64_kernel, dim3(pm_grid_for(pixels)), dim3(256), 0, (hipStream_t)stream, buffer, pixels, c, out_cls, out_prob);
  return pm_check_launch("argmax_f64");
}
