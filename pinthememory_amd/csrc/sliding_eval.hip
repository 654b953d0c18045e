// Sliding-window evaluation (eval.py:158-274 reverse_mapping / reverse_sliding_window, :340-405 inference_sliding, :647 the mean over scales), consumed from the
// heads' LOW-RES logits: per pixel of the scaled image and flip, the covering tiles are up-sampled (bilinear, align_corners=True: pm_ac_lerp and the expression of
// resize_fwd_kernel), widened to double, summed in tile order and divided by the true cover count; the flipped stack is read at column Ws - 1 - x. Neither the
// up-sampled tiles nor a stitched C x Hs x Ws map is ever written:
//   one scale   (sliding_eval_kernel):     (flip0 + flip1) / F, argmax (lowest class among the maxima), hist[label][pred] in per-block LDS counters folded by
//                                          integer adds (pm_hist_fold_kernel), the float64 mean logits only on request;
//   more scales (sliding_resample_kernel): each flip's stitched map resampled to H x W as cv2.resize(INTER_LINEAR) does for float64 (eval.py:197-207), from at
//                                          most four scaled-image pixels stitched on the fly; the mean over flips goes into the float64 accumulator [C][H][W];
//   sliding_finish_kernel:                 accumulator / scales -> argmax, hist (and the mean logits on request).
// The tile table lives in the workspace: uploaded 64 tiles per launch through the kernel arguments, so any number of tiles is served and nothing has to outlive the call.
#include "pm_common.h"

#include <vector>

namespace {
constexpr int SE_MAX_BLOCKS = 2048;      // blocks of the pixel kernels: 8 per CU of the largest part; one row of C x C counters per block
constexpr int SE_CHUNK = 4;              // classes per thread of the resampling kernel
constexpr int SE_UPLOAD = 64;            // tiles per upload launch (1 KB of kernel arguments)

struct SlideGeom {
  const float* lg;        // [F * T][hl][wl] pixels of `pitch` floats
  const int4* tiles;      // (x1, y1, x2, y2) of the T tiles, in the workspace
  long pitch, tile_stride;
  int hl, wl, C, T, F, th, tw, Hs, Ws, H, W;
  float sy, sx;           // pm_ac_scale(hl, th), pm_ac_scale(wl, tw)
};

struct TileChunk {
  int4 t[SE_UPLOAD];
};
__global__ __launch_bounds__(SE_UPLOAD) void tiles_upload_kernel(const TileChunk c, int n, int4* __restrict__ dst) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.t[threadIdx.x];
}

// resize_fwd_kernel's ly.w0 * (lx.w0 * a + lx.w1 * b) + ly.w1 * (lx.w0 * c + lx.w1 * d) with its contractions spelled out: every instantiation, and so the
// one-scale launch and the accumulator route, round alike
__device__ __forceinline__ float tile_lerp(const pm_lerp& ly, const pm_lerp& lx, float a, float b, float c, float d) {
  return fmaf(ly.w0, fmaf(lx.w0, a, lx.w1 * b), ly.w1 * fmaf(lx.w0, c, lx.w1 * d));
}

// classes c0 ... c0 + NC - 1 of flip f's stitched map at pixel (y, x) of the scaled image: float64 sum of the covering tiles in tile order / cover count.
// VEC: 16-byte loads (base 16B-aligned, pitch % 4 == 0, c0 % 4 == 0); the pad lanes behind class C - 1 land in entries nobody reads.
template <int NC, bool VEC>
__device__ __forceinline__ void stitch_point(const SlideGeom& g, int f, int y, int x, int c0, double* s) {
  const int xs = f ? g.Ws - 1 - x : x;      // the un-flip of np.fliplr
  const float* base = g.lg + (long)f * g.T * g.tile_stride;
#pragma unroll
  for (int e = 0; e < NC; ++e) s[e] = 0.0;
  int cnt = 0;
  for (int t = 0; t < g.T; ++t) {
    const int4 r = g.tiles[t];
    const int tx = xs - r.x, ty = y - r.y;
    if ((unsigned)tx >= (unsigned)g.tw || (unsigned)ty >= (unsigned)g.th) continue;
    const pm_lerp ly = pm_ac_lerp(g.sy, ty, g.hl), lx = pm_ac_lerp(g.sx, tx, g.wl);
    const float* r0 = base + (long)t * g.tile_stride + (long)ly.i0 * g.wl * g.pitch + c0;
    const float* r1 = base + (long)t * g.tile_stride + (long)ly.i1 * g.wl * g.pitch + c0;
    const float *p00 = r0 + lx.i0 * g.pitch, *p01 = r0 + lx.i1 * g.pitch, *p10 = r1 + lx.i0 * g.pitch, *p11 = r1 + lx.i1 * g.pitch;
    if constexpr (VEC) {
#pragma unroll
      for (int k = 0; k < (NC + 3) / 4; ++k)
        if (c0 + 4 * k < g.C) {
          const float4 a = PM_LD4(p00 + 4 * k), b = PM_LD4(p01 + 4 * k), c = PM_LD4(p10 + 4 * k), d = PM_LD4(p11 + 4 * k);
          s[4 * k] += (double)tile_lerp(ly, lx, a.x, b.x, c.x, d.x);
          if (4 * k + 1 < NC) s[4 * k + 1] += (double)tile_lerp(ly, lx, a.y, b.y, c.y, d.y);
          if (4 * k + 2 < NC) s[4 * k + 2] += (double)tile_lerp(ly, lx, a.z, b.z, c.z, d.z);
          if (4 * k + 3 < NC) s[4 * k + 3] += (double)tile_lerp(ly, lx, a.w, b.w, c.w, d.w);
        }
    } else {
#pragma unroll
      for (int e = 0; e < NC; ++e)
        if (c0 + e < g.C) s[e] += (double)tile_lerp(ly, lx, p00[e], p01[e], p10[e], p11[e]);
    }
    ++cnt;
  }
  const double n = (double)cnt;      // >= 1: the entry point refuses a table that leaves a pixel uncovered
#pragma unroll
  for (int e = 0; e < NC; ++e) s[e] /= n;
}

template <int C_, bool VEC>
__global__ __launch_bounds__(256) void sliding_eval_kernel(const SlideGeom g, const int64_t* __restrict__ labels, unsigned* __restrict__ counts,
                                                           uint8_t* __restrict__ pred, double* __restrict__ out) {
  constexpr int NC = C_ > 0 ? C_ : PM_MAX_CLASSES;
  __shared__ unsigned cnt[NC * NC];
  const int C = g.C;
  if (labels) {
    for (int i = threadIdx.x; i < C * C; i += 256) cnt[i] = 0u;
    __syncthreads();
  }
  const long total = (long)g.H * g.W;
  const double flips = (double)g.F;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int y = (int)(p / g.W), x = (int)(p - (long)y * g.W);
    double tot[NC];
    stitch_point<NC, VEC>(g, 0, y, x, 0, tot);
    if (g.F == 2) {
      double s[NC];
      stitch_point<NC, VEC>(g, 1, y, x, 0, s);
#pragma unroll
      for (int e = 0; e < NC; ++e) tot[e] += s[e];
    }
    double best = 0.0;
    int arg = 0;
#pragma unroll
    for (int e = 0; e < NC; ++e)
      if (e < C) {
        const double v = tot[e] / flips;      // np.mean(batch_return, axis=0)
        if (out) out[(long)e * total + p] = v;
        if (e == 0 || v > best) best = v, arg = e;      // the lowest class among the maxima
      }
    if (pred) pred[p] = (uint8_t)arg;
    if (labels) {
      const int64_t lab = labels[p];
      if (lab >= 0 && lab < C) atomicAdd(&cnt[(int)lab * C + arg], 1u);      // fast_hist's mask (utils/misc.py:65-70)
    }
  }
  if (labels) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) counts[(long)blockIdx.x * C * C + i] = cnt[i];
  }
}

// One axis of cv2.resize(INTER_LINEAR) for float64 data: taps i0 / i1 with float weights w0 / w1 (w1 == 0: one tap, at a border or where the grids coincide).
struct Cv2Tap {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ Cv2Tap cv2_tap(int d, int S, double scale) {
  float f = (float)__dadd_rn(__dmul_rn((double)d + 0.5, scale), -0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) s = 0, f = 0.f;
  if (s >= S - 1) s = S - 1, f = 0.f;
  Cv2Tap t;
  t.i0 = s, t.i1 = min(s + 1, S - 1);
  t.w0 = 1.f - f, t.w1 = f;
  return t;
}

// acc[c][Y][X] (+)= mean over flips of the stitched map resampled to H x W: horizontal pass a * w0 + b * w1 in double, then the vertical one the same way, every
// product and sum rounded on its own (no fma). A tap of weight 0 is not evaluated: a * w0 + b * 0 == a * w0 for finite b.
template <bool VEC>
__global__ __launch_bounds__(256) void sliding_resample_kernel(const SlideGeom g, double scale_y, double scale_x, double* __restrict__ acc, int add) {
  const long total = (long)g.H * g.W;
  const int c0 = blockIdx.y * SE_CHUNK;
  const double flips = (double)g.F;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int Y = (int)(p / g.W), X = (int)(p - (long)Y * g.W);
    const Cv2Tap ty = cv2_tap(Y, g.Hs, scale_y), tx = cv2_tap(X, g.Ws, scale_x);
    double tot[SE_CHUNK];
    for (int f = 0; f < g.F; ++f) {
      double r[SE_CHUNK];
      for (int k = 0; k < 2; ++k) {
        const float wy = k ? ty.w1 : ty.w0;
        if (k && wy == 0.f) break;
        const int ys = k ? ty.i1 : ty.i0;
        double h[SE_CHUNK], b[SE_CHUNK];
        stitch_point<SE_CHUNK, VEC>(g, f, ys, tx.i0, c0, h);
#pragma unroll
        for (int e = 0; e < SE_CHUNK; ++e) h[e] = __dmul_rn(h[e], (double)tx.w0);
        if (tx.w1 != 0.f) {
          stitch_point<SE_CHUNK, VEC>(g, f, ys, tx.i1, c0, b);
#pragma unroll
          for (int e = 0; e < SE_CHUNK; ++e) h[e] = __dadd_rn(h[e], __dmul_rn(b[e], (double)tx.w1));
        }
#pragma unroll
        for (int e = 0; e < SE_CHUNK; ++e) r[e] = k ? __dadd_rn(r[e], __dmul_rn(h[e], (double)wy)) : __dmul_rn(h[e], (double)wy);
      }
#pragma unroll
      for (int e = 0; e < SE_CHUNK; ++e) tot[e] = f ? tot[e] + r[e] : r[e];
    }
#pragma unroll
    for (int e = 0; e < SE_CHUNK; ++e)
      if (c0 + e < g.C) {
        const double v = tot[e] / flips;
        double* dst = acc + (long)(c0 + e) * total + p;
        *dst = add ? *dst + v : v;
      }
  }
}

// `out` may be the accumulator itself: every element is read and written by the one thread that owns its pixel
__global__ __launch_bounds__(256) void sliding_finish_kernel(const double* acc, int C, long total, double scales, const int64_t* __restrict__ labels,
                                                             unsigned* __restrict__ counts, uint8_t* __restrict__ pred, double* out) {
  __shared__ unsigned cnt[PM_MAX_CLASSES * PM_MAX_CLASSES];
  if (labels) {
    for (int i = threadIdx.x; i < C * C; i += 256) cnt[i] = 0u;
    __syncthreads();
  }
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    double best = 0.0;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const double v = acc[(long)c * total + p] / scales;      // np.mean over the scales (eval.py:647)
      if (out) out[(long)c * total + p] = v;
      if (c == 0 || v > best) best = v, arg = c;
    }
    if (pred) pred[p] = (uint8_t)arg;
    if (labels) {
      const int64_t lab = labels[p];
      if (lab >= 0 && lab < C) atomicAdd(&cnt[(int)lab * C + arg], 1u);
    }
  }
  if (labels) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) counts[(long)blockIdx.x * C * C + i] = cnt[i];
  }
}

inline int se_blocks(int H, int W) { return (int)std::min<long>(((long)H * W + 255) / 256, SE_MAX_BLOCKS); }
inline size_t se_tile_bytes(int ntiles) { return pm_align_up((size_t)std::max(ntiles, 0) * sizeof(int4), 256); }
inline size_t se_count_bytes(int C, int H, int W) { return pm_align_up((size_t)se_blocks(H, W) * C * C * sizeof(unsigned), 256); }
inline bool se_sizes_ok(int C, int H, int W) { return C >= 1 && C <= PM_MAX_CLASSES && H >= 1 && W >= 1; }

// Does every pixel of Hs x Ws lie in a tile? Checked on the cells between the tiles' distinct edges: a cell [xs[i], xs[i + 1]) x [ys[j], ys[j + 1]) is inside or
// outside every tile as a whole. Every tile adds 1 to its rectangle of cells through four corner marks; a prefix sum over the cells gives the cover counts.
// Host work of O(n log n + cells), cells <= (2 n + 1)^2 for n tiles with no edge in common and (columns + 1) x (rows + 1) for a grid of sliding_tiles -- the
// tiles were checked to lie inside the image before, so every edge is found among the cell borders.
bool se_covered(const int32_t* t, int n, int Hs, int Ws) {
  std::vector<int> xs{0, Ws}, ys{0, Hs};
  xs.reserve(2 * (size_t)n + 2), ys.reserve(2 * (size_t)n + 2);
  for (int i = 0; i < n; ++i) xs.push_back(t[4 * i]), ys.push_back(t[4 * i + 1]), xs.push_back(t[4 * i + 2]), ys.push_back(t[4 * i + 3]);
  std::sort(xs.begin(), xs.end()), std::sort(ys.begin(), ys.end());
  xs.erase(std::unique(xs.begin(), xs.end()), xs.end()), ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
  const size_t nx = xs.size(), ny = ys.size();      // borders: nx - 1 columns and ny - 1 rows of cells, marks one past them
  std::vector<int> cover(nx * ny, 0);
  for (int i = 0; i < n; ++i) {
    const size_t x1 = std::lower_bound(xs.begin(), xs.end(), t[4 * i]) - xs.begin(), x2 = std::lower_bound(xs.begin(), xs.end(), t[4 * i + 2]) - xs.begin();
    const size_t y1 = std::lower_bound(ys.begin(), ys.end(), t[4 * i + 1]) - ys.begin(), y2 = std::lower_bound(ys.begin(), ys.end(), t[4 * i + 3]) - ys.begin();
    ++cover[y1 * nx + x1], --cover[y1 * nx + x2], --cover[y2 * nx + x1], ++cover[y2 * nx + x2];
  }
  for (size_t j = 0; j + 1 < ny; ++j)
    for (size_t i = 0; i + 1 < nx; ++i) {
      int& c = cover[j * nx + i];
      c += (i ? cover[j * nx + i - 1] : 0) + (j ? cover[(j - 1) * nx + i] : 0) - (i && j ? cover[(j - 1) * nx + i - 1] : 0);
      if (c <= 0) return false;
    }
  return true;
}

void se_fold(const unsigned* counts, int nblk, int C, int accumulate, int64_t* hist, hipStream_t st) {
  hipLaunchKernelGGL(pm_hist_fold_kernel, dim3((C * C + 31) / 32), dim3(PM_HIST_FOLD_T), 0, st, counts, nblk, C * C, accumulate, hist);
}
}  // namespace

extern "C" size_t pm_sliding_eval_workspace(int ntiles, int C, int H, int W) {
  if (ntiles < 0 || !se_sizes_ok(C, H, W)) return 0;
  return se_tile_bytes(ntiles) + se_count_bytes(C, H, W);
}

extern "C" int pm_sliding_eval(const float* logits, int n, int h, int w, int C, int64_t pitch, int flips, const int32_t* tiles_xyxy, int ntiles, int Hs, int Ws,
                               int H, int W, const int64_t* labels, int64_t* hist, int accumulate, uint8_t* pred, double* logits_out, double* acc, int acc_add,
                               void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(logits && tiles_xyxy, PM_EINVAL, "sliding_eval: null logits / tiles");
  PM_REQUIRE(flips == 1 || flips == 2, PM_EINVAL, "sliding_eval: %d flips (1: the image, 2: the image and its mirror)", flips);
  PM_REQUIRE(C >= 1 && C <= PM_MAX_CLASSES, PM_EUNSUPPORTED, "sliding_eval: classes %d not in 1..%d", C, PM_MAX_CLASSES);
  PM_REQUIRE(ntiles >= 1 && h >= 1 && w >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && pitch >= C && (long)n == (long)flips * ntiles, PM_EINVAL,
             "sliding_eval: bad sizes (logits n = flips x tiles = %d x %d, pitch >= C, every extent >= 1)", flips, ntiles);
  PM_REQUIRE((accumulate == 0 || accumulate == 1) && (acc_add == 0 || acc_add == 1), PM_EINVAL, "sliding_eval: accumulate / acc_add is neither 0 nor 1");
  if (acc) {
    PM_REQUIRE(!labels && !hist && !pred && !logits_out, PM_EINVAL, "sliding_eval: with an accumulator, class map and histogram come from pm_sliding_eval_finish");
  } else {
    PM_REQUIRE(Hs == H && Ws == W, PM_EINVAL, "sliding_eval: a %d x %d scaled image for a %d x %d output needs the accumulator", Hs, Ws, H, W);
    PM_REQUIRE(!labels || hist, PM_EINVAL, "sliding_eval: labels without a histogram");
    PM_REQUIRE(labels || pred || logits_out, PM_EINVAL, "sliding_eval: nothing to write");
  }
  const int th = tiles_xyxy[3] - tiles_xyxy[1], tw = tiles_xyxy[2] - tiles_xyxy[0];
  PM_REQUIRE(th >= 1 && tw >= 1, PM_EINVAL, "sliding_eval: tile 0 is empty");
  for (int i = 0; i < ntiles; ++i) {
    const int32_t* t = tiles_xyxy + 4 * i;
    PM_REQUIRE(t[0] >= 0 && t[1] >= 0 && t[2] <= Ws && t[3] <= Hs && t[2] - t[0] == tw && t[3] - t[1] == th, PM_EINVAL,
               "sliding_eval: tile %d (%d, %d, %d, %d) leaves the %d x %d image or is not %d x %d as tile 0", i, t[0], t[1], t[2], t[3], Hs, Ws, th, tw);
  }
  PM_REQUIRE(se_covered(tiles_xyxy, ntiles, Hs, Ws), PM_EINVAL, "sliding_eval: the tiles leave pixels of the %d x %d image uncovered", Hs, Ws);
  const size_t tile_bytes = se_tile_bytes(ntiles);
  PM_REQUIRE(ws && ws_bytes >= tile_bytes + se_count_bytes(C, H, W), PM_EWORKSPACE, "sliding_eval: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  int4* dtiles = (int4*)ws;
  unsigned* counts = (unsigned*)((char*)ws + tile_bytes);
  for (int i0 = 0; i0 < ntiles; i0 += SE_UPLOAD) {
    TileChunk c;
    const int m = std::min(SE_UPLOAD, ntiles - i0);
    for (int i = 0; i < SE_UPLOAD; ++i) {
      const int32_t* t = tiles_xyxy + 4 * (i0 + std::min(i, m - 1));
      c.t[i] = make_int4(t[0], t[1], t[2], t[3]);
    }
    hipLaunchKernelGGL(tiles_upload_kernel, dim3(1), dim3(SE_UPLOAD), 0, st, c, m, dtiles + i0);
  }
  SlideGeom g;
  g.lg = logits, g.tiles = dtiles, g.pitch = pitch, g.tile_stride = (long)h * w * pitch;
  g.hl = h, g.wl = w, g.C = C, g.T = ntiles, g.F = flips, g.th = th, g.tw = tw, g.Hs = Hs, g.Ws = Ws, g.H = H, g.W = W;
  g.sy = pm_ac_scale(h, th), g.sx = pm_ac_scale(w, tw);
  const int nblk = se_blocks(H, W);
  const bool vec = pm_aligned16(logits) && pitch % 4 == 0;      // the pitch-padded rows the heads write
  if (acc) {
    const dim3 grid(nblk, (C + SE_CHUNK - 1) / SE_CHUNK);
    const double scy = (double)Hs / (double)H, scx = (double)Ws / (double)W;
    if (vec) hipLaunchKernelGGL(sliding_resample_kernel<true>, grid, dim3(256), 0, st, g, scy, scx, acc, acc_add);
    else hipLaunchKernelGGL(sliding_resample_kernel<false>, grid, dim3(256), 0, st, g, scy, scx, acc, acc_add);
    return pm_check_launch("sliding_eval");
  }
#define SE_LAUNCH(CC, V) hipLaunchKernelGGL((sliding_eval_kernel<CC, V>), dim3(nblk), dim3(256), 0, st, g, labels, counts, pred, logits_out)
  if (C == 19 && vec) SE_LAUNCH(19, true);
  else if (C == 19) SE_LAUNCH(19, false);
  else if (vec) SE_LAUNCH(0, true);
  else SE_LAUNCH(0, false);
#undef SE_LAUNCH
  if (labels) se_fold(counts, nblk, C, accumulate, hist, st);
  return pm_check_launch("sliding_eval");
}

extern "C" int pm_sliding_eval_finish(const double* acc, int C, int H, int W, int nscales, const int64_t* labels, int64_t* hist, int accumulate, uint8_t* pred,
                                      double* logits_out, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(acc, PM_EINVAL, "sliding_eval_finish: null accumulator");
  PM_REQUIRE(C >= 1 && C <= PM_MAX_CLASSES, PM_EUNSUPPORTED, "sliding_eval_finish: classes %d not in 1..%d", C, PM_MAX_CLASSES);
  PM_REQUIRE(H >= 1 && W >= 1 && nscales >= 1 && (accumulate == 0 || accumulate == 1), PM_EINVAL, "sliding_eval_finish: bad sizes / accumulate");
  PM_REQUIRE(!labels || hist, PM_EINVAL, "sliding_eval_finish: labels without a histogram");
  PM_REQUIRE(labels || pred || logits_out, PM_EINVAL, "sliding_eval_finish: nothing to write");
  PM_REQUIRE(ws && ws_bytes >= se_count_bytes(C, H, W), PM_EWORKSPACE, "sliding_eval_finish: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = se_blocks(H, W);
  hipLaunchKernelGGL(sliding_finish_kernel, dim3(nblk), dim3(256), 0, st, acc, C, (long)H * W, (double)nscales, labels, (unsigned*)ws, pred, logits_out);
  if (labels) se_fold((const unsigned*)ws, nblk, C, accumulate, hist, st);
  return pm_check_launch("sliding_eval_finish");
}
