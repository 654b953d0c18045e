// The ablation sweep (ablation.py RunAbla.tsne_memact with tsnelib.py RunTsne): the per-class feature sums behind the t-SNE prototypes and the memory activation maps.
// The reference up-samples the 256-channel feature map to the label size and multiplies it with a one-hot of the labels (tsnelib.py:48-74). The up-sampling is linear,
// so the labels are instead splatted ONCE through the transpose of the bilinear operator into a low-res [h][w][classes + 1] weight map (label_splat_kernel, a gather:
// every low-res cell walks its own support), and the sums are a [classes + 1] x [h w] . [h w] x [C] product over the normalised low-res features
// (class_sums_partial + class_sums_merge). The activation map (ablation.py:309-315,371-399) is one pass over the output pixels from the low-res scores.
// No floating-point atomics anywhere: every sum has one fixed order that does not depend on the grid.
#include "pm_common.h"

#include "augment_math.h"
#pragma clang fp contract(fast)      // augment_math.h switches contraction off for what follows it; the interpolation below is pool_resize.hip's, under its setting

namespace {

// label -> row of the splat / the counts: 255 is the reference's extra class (gt[gt == 255] = num_class), any other value outside [0, classes) is skipped
__device__ __forceinline__ int label_row(int64_t l, int classes) { return l == 255 ? classes : (l >= 0 && l < classes ? (int)l : -1); }

// ---- splat: one wave per low-res cell --------------------------------------------------------------------------------------------------------------------------
// Lane t takes the support pixels t, t + 64, ... (row-major over the cell's support window) and keeps one accumulator per class in LDS, laid out [class][lane]: a
// register array indexed by the label would live in scratch. The lanes are then summed per class in lane order.
constexpr int SPLAT_LD = 65;      // floats between class rows: the final column walk of lane k hits 64 different banks
__global__ __launch_bounds__(64) void label_splat_kernel(const int64_t* __restrict__ labels, long cells, int H, int W, int h, int w, int classes, float sy, float sx,
                                                         float* __restrict__ splat) {
  __shared__ float acc[PM_MAX_CLASSES * SPLAT_LD];
  const int lane = threadIdx.x, K1 = classes + 1;
  for (long cell = blockIdx.x; cell < cells; cell += gridDim.x) {
    const int j = (int)(cell % w), i = (int)((cell / w) % h);
    const long img = cell / ((long)w * h);
    for (int k = 0; k < K1; ++k) acc[k * SPLAT_LD + lane] = 0.f;
    int ylo, yhi, xlo, xhi;
    pm_support(sy, i, H, ylo, yhi);
    pm_support(sx, j, W, xlo, xhi);
    const int ww = xhi - xlo + 1, cnt = (yhi - ylo + 1) * ww;
    const int64_t* lab = labels + img * H * W;
    for (int t = lane; t < cnt; t += 64) {
      const int Y = ylo + t / ww, X = xlo + t % ww;
      const float wgt = pm_tap_weight(pm_ac_lerp(sy, Y, h), i) * pm_tap_weight(pm_ac_lerp(sx, X, w), j);
      const int k = label_row(lab[(long)Y * W + X], classes);
      if (k >= 0 && wgt != 0.f) acc[k * SPLAT_LD + lane] += wgt;
    }
    __syncthreads();
    if (lane < K1) {
      float s = 0.f;
      for (int t = 0; t < 64; ++t) s += acc[lane * SPLAT_LD + t];
      splat[cell * K1 + lane] = s;
    }
    __syncthreads();
  }
}

// exact pixel counts: an integer histogram per block, then one integer add per class and block (order-free)
__global__ __launch_bounds__(256) void label_count_kernel(const int64_t* __restrict__ labels, long HW, int classes, int bpi, unsigned long long* __restrict__ counts) {
  __shared__ unsigned hist[PM_MAX_CLASSES];
  const long img = blockIdx.x / bpi;
  const int b = blockIdx.x % bpi;
  if (threadIdx.x < PM_MAX_CLASSES) hist[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t* lab = labels + img * HW;
  for (long p = (long)b * 256 + threadIdx.x; p < HW; p += (long)bpi * 256) {
    const int k = label_row(lab[p], classes);
    if (k >= 0) atomicAdd(&hist[k], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x <= classes && hist[threadIdx.x]) atomicAdd(&counts[img * (classes + 1) + threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// ---- class sums: block = (image, chunk of CS_CHUNK low-res pixels), thread = channel ---------------------------------------------------------------------------------
constexpr int CS_CHUNK = 32;
inline int cs_chunks(long HW) { return pm_cdiv(HW, CS_CHUNK); }
inline size_t cs_workspace(int n, long HW, int C, int classes) { return pm_align_up((size_t)n * cs_chunks(HW) * (classes + 1) * C * sizeof(float), 256); }

// part[img][chunk][k][ch] = sum over the chunk's pixels q, in pixel order, of splat[q][k] * feat[q][ch] / max(|feat[q]|, 1e-12)
template <typename T>
__global__ __launch_bounds__(256) void class_sums_partial(const T* __restrict__ feat, long pitch, long HW, int C, const float* __restrict__ splat, int K1, int nchunks,
                                                          float* __restrict__ part) {
  __shared__ float sp[CS_CHUNK * PM_MAX_CLASSES];      // [pixel][K1]
  __shared__ float den[CS_CHUNK];
  const long img = blockIdx.x / nchunks;
  const int ck = blockIdx.x % nchunks, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long q0 = (long)ck * CS_CHUNK;
  const int np = (int)min((long)CS_CHUNK, HW - q0);
  const T* f = feat + (img * HW + q0) * pitch;
  const float* s = splat + (img * HW + q0) * K1;
  for (int t = tid; t < np * K1; t += 256) sp[t] = s[t];
  for (int p = wv; p < np; p += 4) {      // F.normalize(dim=1): the norm in fp32 over the widened channels, one wave per pixel
    float ss = 0.f;
    for (int ch = lane; ch < C; ch += 64) {
      const float v = pm_elem<T>::widen(f[p * pitch + ch]);
      ss += v * v;
    }
    ss = pm_wave_sum(ss);
    if (lane == 0) den[p] = fmaxf(sqrtf(ss), 1e-12f);
  }
  __syncthreads();
  for (int ch = tid; ch < C; ch += 256) {
    float acc[PM_MAX_CLASSES];
#pragma unroll
    for (int k = 0; k < PM_MAX_CLASSES; ++k) acc[k] = 0.f;
    for (int p = 0; p < np; ++p) {
      const float v = pm_elem<T>::widen(f[p * pitch + ch]) / den[p];
#pragma unroll
      for (int k = 0; k < PM_MAX_CLASSES; ++k)      // fully unrolled: acc stays in registers
        if (k < K1) acc[k] += sp[p * K1 + k] * v;
    }
    float* o = part + ((img * nchunks + ck) * K1) * C + ch;
#pragma unroll
    for (int k = 0; k < PM_MAX_CLASSES; ++k)
      if (k < K1) o[(long)k * C] = acc[k];
  }
}
// the chunks of one image in chunk order, in double, rounded once
__global__ __launch_bounds__(256) void class_sums_merge(const float* __restrict__ part, int nchunks, long KC, long total, float* __restrict__ sums) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long img = i / KC, r = i - img * KC;
    double s = 0.0;
    for (int ck = 0; ck < nchunks; ++ck) s += (double)part[(img * nchunks + ck) * KC + r];
    sums[i] = (float)s;
  }
}

// ---- memory activation map: thread = full-res pixel ------------------------------------------------------------------------------------------------------------------
// The m interpolated scores of a pixel are parked in LDS ([slot][thread]: a register array indexed by the slot list would live in scratch), so that a listed slot's
// value is the very float that entered the pixel's min / max: the arg-min slot gives exactly 0, the arg-max slot exactly 1.
struct ActSlots {
  int32_t s[PM_MAX_CLASSES];
};
__global__ __launch_bounds__(256) void mem_actmap_kernel(const float* __restrict__ pm, int h, int w, int m, long pitch, int H, int W, float sy, float sx, ActSlots sl,
                                                         int ns, float* __restrict__ act, uint8_t* __restrict__ bytes, const uint8_t* __restrict__ pal,
                                                         const uint8_t* __restrict__ image, float alpha, uint8_t* __restrict__ rgb, uint8_t* __restrict__ blend,
                                                         long total) {
  extern __shared__ float vals[];      // [m][256]
  const int tid = threadIdx.x;
  const long HW = (long)H * W;
  for (long op = (long)blockIdx.x * 256 + tid; op < total; op += (long)gridDim.x * 256) {
    const int X = (int)(op % W), Y = (int)((op / W) % H);
    const long img = op / HW, pix = op - img * HW;
    const pm_lerp ly = pm_ac_lerp(sy, Y, h), lx = pm_ac_lerp(sx, X, w);
    const float* r0 = pm + ((img * h + ly.i0) * w) * pitch;
    const float* r1 = pm + ((img * h + ly.i1) * w) * pitch;
    const float *a = r0 + lx.i0 * pitch, *b = r0 + lx.i1 * pitch, *c = r1 + lx.i0 * pitch, *d = r1 + lx.i1 * pitch;
    float lo = INFINITY, hi = -INFINITY;
    for (int s = 0; s < m; ++s) {
      const float v = ly.w0 * (lx.w0 * a[s] + lx.w1 * b[s]) + ly.w1 * (lx.w0 * c[s] + lx.w1 * d[s]);      // resize_fwd_kernel's expression
      vals[s * 256 + tid] = v;
      lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    const float range = hi - lo;
    for (int e = 0; e < ns; ++e) {
      const float v = vals[sl.s[e] * 256 + tid];
      const float an = range > 0.f ? (v - lo) / range : 0.f;      // hi == lo: the reference divides 0 by 0; defined as 0 here
      const int by = (int)(fminf(fmaxf(an, 0.f), 1.f) * 255.f);   // np.uint8(np.clip(., 0, 1) * 255) on float32
      const long o = (img * ns + e) * HW + pix;
      if (act) act[o] = an;
      if (bytes) bytes[o] = (uint8_t)by;
      if (rgb || blend) {
        const uint8_t* q = pal + by * 3;
        if (rgb) rgb[o * 3] = q[0], rgb[o * 3 + 1] = q[1], rgb[o * 3 + 2] = q[2];
        if (blend) {
          const uint8_t* im = image + (img * HW + pix) * 3;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) blend[o * 3 + ch] = (uint8_t)pm_aug_blend((int)im[ch], (int)q[ch], alpha);
        }
      }
    }
  }
}

}  // namespace

extern "C" int pm_label_splat(const int64_t* labels, int n, int H, int W, int h, int w, int classes, float* splat, int64_t* counts, void* stream) {
  const char* who = "label_splat";
  PM_REQUIRE(labels && splat && counts, PM_EINVAL, "%s: labels / splat / counts is null", who);
  PM_REQUIRE(n > 0 && H > 0 && W > 0 && h > 0 && w > 0 && classes > 0, PM_EINVAL, "%s: sizes must be positive (n %d H %d W %d h %d w %d classes %d)", who, n, H, W, h, w,
             classes);
  PM_REQUIRE(classes < PM_MAX_CLASSES, PM_EUNSUPPORTED, "%s: at most %d classes (got %d)", who, PM_MAX_CLASSES - 1, classes);
  PM_REQUIRE((long)H * W < (1l << 31) && (long)n * h * w < (1l << 40), PM_EUNSUPPORTED, "%s: image too large", who);
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W, cells = (long)n * h * w;
  if (hipMemsetAsync(counts, 0, (size_t)n * (classes + 1) * sizeof(int64_t), st) != hipSuccess) {
    (void)hipGetLastError();
    pm_set_error("%s: clearing the counts failed", who);
    return PM_ELAUNCH;
  }
  const int bpi = (int)std::min<long>(pm_cdiv(HW, 256 * 8), std::max<long>(1, 65536 / n));
  hipLaunchKernelGGL(label_count_kernel, dim3(n * bpi), dim3(256), 0, st, labels, HW, classes, bpi, reinterpret_cast<unsigned long long*>(counts));
  hipLaunchKernelGGL(label_splat_kernel, dim3((unsigned)std::min<long>(cells, 1l << 20)), dim3(64), 0, st, labels, cells, H, W, h, w, classes, pm_ac_scale(h, H),
                     pm_ac_scale(w, W), splat);
  return pm_check_launch(who);
}

extern "C" size_t pm_class_sums_workspace(int n, int h, int w, int c, int classes) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || classes <= 0) return 0;
  return cs_workspace(n, (long)h * w, c, classes);
}

extern "C" int pm_class_sums(const void* feat, int n, int h, int w, int c, int64_t feat_pitch, int dtype, const float* splat, int classes, float* sums, void* ws,
                             size_t ws_bytes, void* stream) {
  const char* who = "class_sums";
  PM_REQUIRE(feat && splat && sums, PM_EINVAL, "%s: feat / splat / sums is null", who);
  PM_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && classes > 0, PM_EINVAL, "%s: sizes must be positive (n %d h %d w %d c %d classes %d)", who, n, h, w, c, classes);
  PM_REQUIRE(dtype == PM_F32 || dtype == PM_BF16, PM_EUNSUPPORTED, "%s: unknown dtype %d", who, dtype);
  PM_REQUIRE(c % 8 == 0, PM_EUNSUPPORTED, "%s: c %% 8 != 0 (c %d)", who, c);
  PM_REQUIRE(classes < PM_MAX_CLASSES, PM_EUNSUPPORTED, "%s: at most %d classes (got %d)", who, PM_MAX_CLASSES - 1, classes);
  const int vec = dtype == PM_BF16 ? 8 : 4;
  PM_REQUIRE(feat_pitch >= c && feat_pitch % vec == 0, PM_EINVAL, "%s: the pitch of feat (%ld) must be >= c and a multiple of %d", who, (long)feat_pitch, vec);
  PM_REQUIRE(pm_aligned16(feat), PM_EINVAL, "%s: feat must be 16-byte aligned", who);
  const long HW = (long)h * w;
  const int nchunks = cs_chunks(HW);
  PM_REQUIRE((long)n * nchunks < (1l << 31), PM_EUNSUPPORTED, "%s: batch too large for one grid", who);
  PM_REQUIRE(ws && pm_aligned16(ws), PM_EINVAL, "%s: the workspace is null or not 16-byte aligned", who);
  PM_REQUIRE(ws_bytes >= cs_workspace(n, HW, c, classes), PM_EWORKSPACE, "%s: workspace too small", who);
  hipStream_t st = (hipStream_t)stream;
  const int K1 = classes + 1;
  if (dtype == PM_BF16)
    hipLaunchKernelGGL((class_sums_partial<pm_bf16>), dim3(n * nchunks), dim3(256), 0, st, (const pm_bf16*)feat, (long)feat_pitch, HW, c, splat, K1, nchunks, (float*)ws);
  else
    hipLaunchKernelGGL((class_sums_partial<float>), dim3(n * nchunks), dim3(256), 0, st, (const float*)feat, (long)feat_pitch, HW, c, splat, K1, nchunks, (float*)ws);
  const long total = (long)n * K1 * c;
  hipLaunchKernelGGL(class_sums_merge, dim3(pm_grid_for(total)), dim3(256), 0, st, (const float*)ws, nchunks, (long)K1 * c, total, sums);
  return pm_check_launch(who);
}

extern "C" int pm_mem_actmap(const float* p_mem, int n, int h, int w, int m, int64_t pitch, int H, int W, const int32_t* slots, int nslots, float* act, uint8_t* bytes,
                             const uint8_t* palette, const uint8_t* image, float alpha, uint8_t* rgb, uint8_t* blend, void* stream) {
  const char* who = "mem_actmap";
  PM_REQUIRE(p_mem && slots, PM_EINVAL, "%s: p_mem / slots is null", who);
  PM_REQUIRE(n > 0 && h > 0 && w > 0 && m > 0 && H > 0 && W > 0, PM_EINVAL, "%s: sizes must be positive (n %d h %d w %d m %d H %d W %d)", who, n, h, w, m, H, W);
  PM_REQUIRE(m <= PM_MAX_CLASSES, PM_EUNSUPPORTED, "%s: at most %d slots (got %d)", who, PM_MAX_CLASSES, m);
  PM_REQUIRE(nslots >= 1 && nslots <= m, PM_EINVAL, "%s: nslots must lie in 1 .. m (got %d, m %d)", who, nslots, m);
  PM_REQUIRE(pitch >= m, PM_EINVAL, "%s: the pitch of p_mem (%ld) must be >= m", who, (long)pitch);
  ActSlots sl = {};
  for (int e = 0; e < nslots; ++e) {
    PM_REQUIRE(slots[e] >= 0 && slots[e] < m, PM_EINVAL, "%s: slot %d (entry %d) outside 0 .. m - 1", who, slots[e], e);
    sl.s[e] = slots[e];
  }
  PM_REQUIRE(act || bytes || rgb || blend, PM_EINVAL, "%s: no output requested", who);
  PM_REQUIRE(!rgb || palette, PM_EINVAL, "%s: rgb needs the palette", who);
  PM_REQUIRE(!blend || (palette && image), PM_EINVAL, "%s: blend needs the palette and the image", who);
  const long total = (long)n * H * W;
  hipLaunchKernelGGL(mem_actmap_kernel, dim3(pm_grid_for(total)), dim3(256), (size_t)m * 256 * sizeof(float), (hipStream_t)stream, p_mem, h, w, m, (long)pitch, H, W,
                     pm_ac_scale(h, H), pm_ac_scale(w, W), sl, nslots, act, bytes, palette, image, alpha, rgb, blend, total);
  return pm_check_launch(who);
}
