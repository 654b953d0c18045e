// Augmenting input edge: colour jitter, Gaussian blur and horizontal flip of uint8 batches in HBM, then ToTensor + Normalize (include/pinmem_hip.h, pm_augment_u8).
// Two launches per batch: an exact integer grey sum per image whose contrast op is on, and one pass that recomputes the colour ops for a tile plus its blur halo into LDS,
// blurs there in float64 (H, then W) and writes NHWC4 floats. Per-image parameters come from a device array: order and flags are uniform over a block.
#include "pm_common.h"

#include "augment_math.h"      // sets fp contract(off) for the rest of this file: no product below may be fused with its sum

namespace {
constexpr int TH = 32, TW = 64, RMAX = PM_AUG_MAX_RADIUS;
constexpr int LW = TW + 2 * RMAX, LH = TH + 2 * RMAX;             // 74 x 42 pixels with the halo
constexpr int ROWB = LW * 3;                                      // bytes (and doubles) per tile row
constexpr int U8_BYTES = (LH * ROWB + 15) / 16 * 16;              // 9 328: the colour stage
constexpr int COL_BYTES = TH * ROWB * 8;                          // 56 832: the column-filtered tile, float64
constexpr int LUT_BYTES = 256 * 8;                                // v / 255.0 per byte value (one float64 division per value instead of one per tap)
constexpr int LDS_BYTES = U8_BYTES + COL_BYTES + LUT_BYTES;       // 68 208

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// sums[n] += grey of every pixel of image n after the ops in front of its contrast op. Blocks of an image without contrast leave at once.
__global__ __launch_bounds__(256) void aug_grey_sum_kernel(const uint8_t* __restrict__ img, long hw, const pm_aug_image* __restrict__ params,
                                                           unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long part[4];
  const int n = blockIdx.y;
  const pm_aug_image P = params[n];
  if (!((P.enabled >> PM_AUG_CONTRAST) & 1)) return;
  const uint8_t* src = img + (long)n * hw * 3;
  unsigned long long acc = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
    int r = src[p * 3], g = src[p * 3 + 1], b = src[p * 3 + 2];
    pm_aug_colour(&r, &g, &b, P, 0, PM_AUG_CONTRAST);
    acc += (unsigned)pm_aug_grey(r, g, b);
  }
  acc = wave_sum_u64(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sums + n, part[0] + part[1] + part[2] + part[3]);
}

// Gaussian blur of the TH x TW centre of a tile with a halo of R: along H from the bytes (through lut: v / 255.0) into `col`, along W from there, (uint8)(y * 255)
// written back over the tile at (ly, lx) without the halo offset. scipy's correlate1d for a symmetric kernel: the centre first, then the pairs from the far one in.
template <int R>
__device__ __forceinline__ void aug_blur_tile(uint8_t* tile, double* col, const double* lut, const double* __restrict__ wg, int tid) {
  double w[R + 1];
#pragma unroll
  for (int j = 0; j <= R; ++j) w[j] = wg[j];
  constexpr int rowe = (TW + 2 * R) * 3;      // interleaved channel bytes per row, halo included
  for (int i = tid; i < TH * rowe; i += 256) {
    const int ly = i / rowe, e = i - ly * rowe;
    const uint8_t* c = tile + (ly + R) * ROWB + e;
    double acc = lut[c[0]] * w[0];
#pragma unroll
    for (int j = R; j >= 1; --j) acc += (lut[c[-j * ROWB]] + lut[c[j * ROWB]]) * w[j];
    col[ly * ROWB + e] = acc;
  }
  __syncthreads();      // every read of the colour stage is done: its place takes the result
  for (int i = tid; i < TH * TW * 3; i += 256) {
    const int ly = i / (TW * 3), e = i - ly * (TW * 3);
    const double* c = col + ly * ROWB + R * 3 + e;
    double acc = c[0] * w[0];
#pragma unroll
    for (int j = R; j >= 1; --j) acc += (c[-3 * j] + c[3 * j]) * w[j];
    tile[ly * ROWB + e] = (uint8_t)(int)(acc * 255.0);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void aug_apply_kernel(const uint8_t* __restrict__ img, int H, int W, const pm_aug_image* __restrict__ params,
                                                        const unsigned long long* __restrict__ sums, float m0, float m1, float m2, float s0, float s1, float s2,
                                                        float* __restrict__ out4, uint8_t* __restrict__ out8) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint8_t* tile = smem;
  double* col = reinterpret_cast<double*>(smem + U8_BYTES);
  double* lut = reinterpret_cast<double*>(smem + U8_BYTES + COL_BYTES);
  const int n = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, tid = threadIdx.x;
  const pm_aug_image P = params[n];
  const int r = min(max(P.radius, 0), RMAX);
  const long hw = (long)H * W;
  const int mean = ((P.enabled >> PM_AUG_CONTRAST) & 1) ? pm_aug_mean(sums[n], hw) : 0;
  const uint8_t* src = img + (long)n * hw * 3;
  const int lh = TH + 2 * r, lw = TW + 2 * r;

  // colour stage of the tile and its halo, coordinates clamped to the image (mode 'nearest'); the flip is taken on the way in, it commutes with all that follows
  for (int i = tid; i < lh * lw; i += 256) {
    const int ly = i / lw, lx = i - ly * lw;
    const int gy = min(max(y0 - r + ly, 0), H - 1), gx = min(max(x0 - r + lx, 0), W - 1);
    const uint8_t* q = src + ((long)gy * W + (P.flip ? W - 1 - gx : gx)) * 3;
    int cr = q[0], cg = q[1], cb = q[2];
    pm_aug_colour(&cr, &cg, &cb, P, mean, 4);
    uint8_t* t = tile + ly * ROWB + lx * 3;
    t[0] = (uint8_t)cr, t[1] = (uint8_t)cg, t[2] = (uint8_t)cb;
  }
  if (r > 0) lut[tid] = (double)tid / 255.0;
  __syncthreads();

  switch (r) {      // block-uniform: the taps unroll and the weights sit in registers
    case 1: aug_blur_tile<1>(tile, col, lut, params[n].w, tid); break;
    case 2: aug_blur_tile<2>(tile, col, lut, params[n].w, tid); break;
    case 3: aug_blur_tile<3>(tile, col, lut, params[n].w, tid); break;
    case 4: aug_blur_tile<4>(tile, col, lut, params[n].w, tid); break;
    case 5: aug_blur_tile<5>(tile, col, lut, params[n].w, tid); break;
    default: break;
  }

  for (int i = tid; i < TH * TW; i += 256) {
    const int ly = i / TW, lx = i - ly * TW;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const uint8_t* t = tile + ly * ROWB + lx * 3;      // r == 0: the tile has no halo; else aug_blur_tile left its result here
    const int v[3] = {t[0], t[1], t[2]};
    const long p = (long)n * hw + (long)gy * W + gx;
    if (out8) out8[p * 3] = (uint8_t)v[0], out8[p * 3 + 1] = (uint8_t)v[1], out8[p * 3 + 2] = (uint8_t)v[2];
    // ToTensor: /255 ; Normalize: (x - mean) / std -- the expression of image_u8_kernel (misc.hip), the same bits
    if (out4) PM_ST4(out4 + p * 4, make_float4(((float)v[0] / 255.f - m0) / s0, ((float)v[1] / 255.f - m1) / s1, ((float)v[2] / 255.f - m2) / s2, 0.f));
  }
}

__global__ __launch_bounds__(256) void labels_u8_flip_kernel(const uint8_t* __restrict__ lab, long total, int H, int W, const pm_aug_image* __restrict__ params,
                                                             int64_t* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / W;
    const int x = (int)(i - row * W);
    out[i] = (int64_t)lab[row * W + (params[row / H].flip ? W - 1 - x : x)];
  }
}
}  // namespace

extern "C" int pm_aug_blur_weights(double sigma, int32_t* radius, double* w6) {
  PM_REQUIRE(radius && w6, PM_EINVAL, "aug_blur_weights: null output");
  PM_REQUIRE(sigma > 0.0 && sigma < 1.375, PM_EUNSUPPORTED, "aug_blur_weights: sigma %g outside (0, 1.375): the radius would exceed %d", sigma, RMAX);
  const int r = (int)(4.0 * sigma + 0.5), cnt = 2 * r + 1;
  double phi[2 * RMAX + 1];
  const double s = -0.5 / (sigma * sigma);
  for (int k = -r; k <= r; ++k) phi[k + r] = exp(s * (double)(k * k));
  // numpy's add.reduce over a contiguous float64 array: the first element + the pairwise sum of the rest (eight accumulators from eight elements on)
  const double* a = phi + 1;
  const int m = cnt - 1;
  double rest;
  if (m < 8) {
    rest = 0.;
    for (int i = 0; i < m; ++i) rest += a[i];
  } else {
    rest = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (int i = 8; i < m; ++i) rest += a[i];
  }
  const double sum = phi[0] + rest;
  for (int k = 0; k <= RMAX; ++k) w6[k] = k <= r ? phi[r + k] / sum : 0.0;
  *radius = r;
  return PM_OK;
}

extern "C" size_t pm_augment_workspace(int n) { return n > 0 ? (size_t)n * sizeof(unsigned long long) : 0; }

extern "C" int pm_augment_u8(const uint8_t* img, int n, int H, int W, const pm_aug_image* params, int32_t struct_size, const float* mean3, const float* std3,
                             float* out4, uint8_t* out8, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_aug_image), PM_EINVAL, "augment_u8: pm_aug_image struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)",
             struct_size, sizeof(pm_aug_image), PM_ABI_VERSION);
  PM_REQUIRE(img && params && mean3 && std3 && n >= 0 && H > 0 && W > 0, PM_EINVAL, "augment_u8: bad args");
  PM_REQUIRE(out4 || out8, PM_EINVAL, "augment_u8: no output (out_nhwc4 and out_u8 are both null)");
  PM_REQUIRE(pm_aligned16(out4) && (const void*)out4 != (const void*)img && out8 != img, PM_EINVAL, "augment_u8: out_nhwc4 must be 16-byte aligned, no output may alias img");
  PM_REQUIRE(n <= 65535 && pm_cdiv(H, TH) <= 65535, PM_EUNSUPPORTED, "augment_u8: n %d / H %d beyond the launch grid", n, H);
  if (n == 0) return PM_OK;
  PM_REQUIRE(ws && ws_bytes >= pm_augment_workspace(n) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, PM_EWORKSPACE,
             "augment_u8: workspace %zu < %zu bytes (or null / not 8-byte aligned)", ws_bytes, pm_augment_workspace(n));
  static pm_lds_optin optin;
  optin(reinterpret_cast<const void*>(aug_apply_kernel), LDS_BYTES);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* sums = (unsigned long long*)ws;
  if (hipMemsetAsync(sums, 0, pm_augment_workspace(n), st) != hipSuccess) {
    pm_set_error("augment_u8: clearing the grey sums failed: %s", hipGetErrorString(hipGetLastError()));
    return PM_ELAUNCH;
  }
  const long hw = (long)H * W;
  hipLaunchKernelGGL(aug_grey_sum_kernel, dim3((int)std::min<long>((hw + 2047) / 2048, 256), n), dim3(256), 0, st, img, hw, params, sums);
  int rc = pm_check_launch("augment_u8 (grey sum)");
  if (rc != PM_OK) return rc;
  hipLaunchKernelGGL(aug_apply_kernel, dim3(pm_cdiv(W, TW), pm_cdiv(H, TH), n), dim3(256), LDS_BYTES, st, img, H, W, params, sums, mean3[0], mean3[1], mean3[2], std3[0],
                     std3[1], std3[2], out4, out8);
  return pm_check_launch("augment_u8");
}

extern "C" int pm_labels_u8_flip_to_i64(const uint8_t* lab, int n, int H, int W, const pm_aug_image* params, int32_t struct_size, int64_t* out, void* stream) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_aug_image), PM_EINVAL,
             "labels_u8_flip_to_i64: pm_aug_image struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)", struct_size, sizeof(pm_aug_image), PM_ABI_VERSION);
  PM_REQUIRE(lab && params && out && n >= 0 && H > 0 && W > 0, PM_EINVAL, "labels_u8_flip_to_i64: bad args");
  const long total = (long)n * H * W;
  if (total == 0) return PM_OK;
  hipLaunchKernelGGL(labels_u8_flip_kernel, dim3((int)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, lab, total, H, W, params, out);
  return pm_check_launch("labels_u8_flip_to_i64");
}
