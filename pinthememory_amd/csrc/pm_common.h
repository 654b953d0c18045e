// Shared helpers for libpinmem_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pinmem_hip.h"

void pm_set_error(const char* fmt, ...);

#define PM_REQUIRE(cond, code, ...)      \
  do {                                   \
    if (!(cond)) {                       \
      pm_set_error(__VA_ARGS__);         \
      return (code);                     \
    }                                    \
  } while (0)

static inline int pm_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    pm_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return PM_ELAUNCH;
  }
  return PM_OK;
}

static inline bool pm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int64_t pm_pixels(const pm_tensor* t) { return (int64_t)t->n * t->h * t->w; }
static inline int pm_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline size_t pm_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Vectorisable NHWC view: base 16B-aligned, pitch % 4 == 0.
static inline bool pm_vec_ok(const pm_tensor* t) { return pm_aligned16(t->ptr) && (t->pitch % 4) == 0; }
static inline bool pm_is_f32(const pm_tensor* t) { return t->dtype == PM_F32; }
static inline bool pm_is_bf16(const pm_tensor* t) { return t->dtype == PM_BF16; }
// every fp32-only entry point starts with this: a bf16 tensor handed to a kernel that would read it as floats must fail loudly
#define PM_REQUIRE_F32(t, who) PM_REQUIRE(!(t) || pm_is_f32(t), PM_EUNSUPPORTED, "%s: fp32 tensors only (got dtype %d)", who, (t)->dtype)
// bf16 views move 16 bytes = 8 channels per lane: base 16B-aligned, pitch % 8 == 0, c % 8 == 0
static inline bool pm_vec8(const pm_tensor* t) { return pm_is_bf16(t) && pm_aligned16(t->ptr) && (t->pitch % 8) == 0 && (t->c % 8) == 0; }

// ---- Winograd F(m x m, 3x3) transforms, m = 2 / 4 (winograd.hip), driven by the conv entry points in conv_igemm.hip ------------
struct pm_wino_geom {
  int N, H, W, d, m, TY, TX;   // tiles per image = d*d sub-lattices x TY x TX tiles of m x m outputs
  long tiles;
};
pm_wino_geom pm_wino_make_geom(int n, int h, int w, int d, int m);
int pm_wino_input_xf(const float* x, long pitch, int C, int Kp, const pm_wino_geom& g, float* V, hipStream_t st);
int pm_wino_filter_xf(const float* w, int Cout, int Cin, int Kp, bool dgrad, int m, float* U, hipStream_t st);
int pm_wino_filter_xf_multi(const float* const* w, float* const* U, const int* cout, const int* cin, const int* kp, const int* m, int n, hipStream_t st);
int pm_wino_output_xf(const float* M, int Cout, const pm_wino_geom& g, float* y, long ypitch, const float* bias, const float* scale, const float* shift,
                      const float* residual, long res_pitch, int relu, hipStream_t st);
int pm_wino_fused_f4(const float* V, const float* U, int Cout, int Kp, const pm_wino_geom& g, float* y, long ypitch, const float* bias, const float* scale,
                     const float* shift, const float* residual, long res_pitch, int relu, hipStream_t st);
int pm_wino_dy_xf(const float* dy, long pitch, int Cout, const pm_wino_geom& g, float* Z, hipStream_t st);
int pm_wino_dw_xf(const float* slab, int ks, int Cout, int Cin, int Kp, int m, float* dw, hipStream_t st);

// ---- bf16 operand preparation of the convolution kernels (bf16.hip; prec = 2) ----------------------------------------------------------
int pm_bf16_cast_rows(const float* x, long pitch, int C, int Cp, long P, void* out, hipStream_t st);
int pm_bf16_cast_weights(const float* w, int Cout, int T, int Cin, int Cp, bool rotate, void* out, hipStream_t st);
struct PmS2Classes {      // the four input-pixel parity classes of a stride-2 data gradient: tap subset (ky0 + 2 i, kx0 + 2 j) and the class' bf16 sub-filter buffer
  int ky0[4], nky[4], kx0[4], nkx[4];
  void* out[4];
};
int pm_bf16_cast_weights_s2(const float* w, int Cout, int kh, int kw, int Cin, int Cp, const PmS2Classes* cl, hipStream_t st);
int pm_bf16_transpose_taps(const float* x, long pitch, int C, int N, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int pad, int dil, void* out,
                           hipStream_t st);

// ---- bf16 activations (NHWC, pm_tensor.dtype == PM_BF16) ---------------------------------------------------------------------------------------------------------
typedef unsigned short pm_bf16;
// dense conversions (bf16.hip) used by the convolution entry points for the few mixed-type call sites of the tier (fp32 logits / image next to bf16 activations)
int pm16_to_f32(const pm_bf16* x, long pitch, int C, long P, float* out, long out_pitch, hipStream_t st);
int pm16_pad_rows(const pm_bf16* x, long pitch, int C, int Cp, long P, pm_bf16* out, hipStream_t st);

// ---- the LDS-DMA bf16 implicit-GEMM convolution (conv16.hip), driven by the conv entry points in conv_igemm.hip ----------------------------------------
struct pm_conv16 {
  const pm_bf16* A;          // bf16 NHWC activations (x, or dy for the data gradient), gathered in place
  const pm_bf16* B;          // bf16 weights [Nn][taps][Cp] (pm_bf16_cast_weights; rotated / transposed for the data gradient)
  void* C;                   // bf16 [M][c_pitch] (c_f32 == 0), fp32 [M][c_pitch] (c_f32 != 0), or the fp32 split-K slabs [ksplit][M][Nn] (ksplit > 1)
  int N, H, W, Ho, Wo;       // input and output pixel grids
  long a_pitch;              // bf16 elements between input pixels
  int Cp;                    // channels per tap, a multiple of 64 (zero pad channels inside the pitch)
  int kh, kw, stride, pad, dil;
  int M, Nn, K, ksteps;      // GEMM extents; K = taps * Cp, ksteps = K / 64
  long c_pitch;
  int c_f32;
  const float *bias, *scale, *shift;
  const void* residual;      // bf16, same shape as C
  long res_pitch;
  int relu;
  float* stats;              // train-mode BatchNorm statistics of the bf16 output: (mean, M2) per 32-row slab and channel (pm_conv_epilogue.bn_partials), or null
  int bm, bn, tiles_m, tiles_n, ksplit, ksteps_per;      // pm_conv16_plan
  long c_split;
  int wide;                  // pm_conv16_plan: 1 = a wide form takes the call (one block per CU): 256 x 256 two-stage, or the 256 x 128 / 128 x 256 ring (persistent: conv16w.hip)
};
void pm_conv16_plan(pm_conv16* k);
int pm_conv16w_launch(const pm_conv16* k, hipStream_t st);      // the persistent plans only; pm_conv16_launch takes every plan and hands these on
int pm_conv16w_persistent(const pm_conv16* k);      // 1: the plan runs in the persistent producer / consumer form of conv16w.hip
size_t pm_conv16_slab_bytes(const pm_conv16* k);
double pm_conv16_executed_fraction(const pm_conv16* k);
int pm_conv16_launch(const pm_conv16* k, hipStream_t st);

// ---- the weight gradient of the bf16 tier on LDS-DMA (wgrad16.hip): persistent producer / consumer ring over (tile, pixel-range) units ---------------------------------
struct pm_wgrad16 {
  const pm_bf16* X;          // bf16 NHWC input of the convolution
  const pm_bf16* DY;         // bf16 NHWC output gradient
  float* C;                  // fp32 dw [Cout][taps * Cin] (ksplit == 1) or the split-K slabs [ksplit][Cout][taps * Cin]
  int N, H, W, Ho, Wo;
  long x_pitch, dy_pitch;    // bf16 elements between pixels
  int Cin, Cout, kh, kw, stride, pad, dil;
  int M, Nn, P;              // GEMM extents: Cout, taps * Cin, output pixels (the reduction)
  int kper, ksplit;          // pixels per split (a multiple of 64) and number of splits
  long c_split;              // floats between slabs
  int bm, bn, tiles_m, tiles_n;      // pm_wgrad16_plan
};
bool pm_wgrad16_plan(pm_wgrad16* k);      // false: the shape stays with the register-staged kernel
int pm_wgrad16_launch(const pm_wgrad16* k, hipStream_t st);

// pwstream.hip: a pointwise fp32 GEMM C[M x Nn] = A[M x K] . B^T with a short reduction (K = 64 / 128), streamed wave by wave (split-operand bf16 MFMA arithmetic)
struct pm_gemm_pw {
  const float* A;            // rows of K floats, a_pitch floats apart
  const float* B;            // element (n, k) at B[n * b_sn + k * b_sk]
  float* C;                  // rows of Nn floats, c_pitch floats apart
  const float *bias, *scale, *shift, *residual;      // v = (acc + bias) * scale + shift (+ residual) (relu): the tile kernels' epilogue
  const unsigned char* res_mask;                     // null, or residual enters masked: byte [row][col / 4] of a dense [M][Nn / 4] array, bit e = element e is added
  long a_pitch, c_pitch, res_pitch;
  int b_sn, b_sk;
  long M;
  int Nn, K, relu;
};
bool pm_pwstream_ok(const pm_gemm_pw* g);
int pm_pwstream_launch(const pm_gemm_pw* g, hipStream_t st);

// The > 64 KB dynamic-LDS opt-in of ONE kernel, made once per device, and the CU count of the current device (persistent kernels size their grid by it). Declare it
// `static` inside the kernel's (per-instantiation) launch template, one object per kernel: many kernels share one function-pointer type, so nothing keyed on that type
// would do. ADVICE r5: a per-process flag served the device that happened to be current at the first call. Safe from several threads: a device is marked done only
// after hipFuncSetAttribute succeeded; a failed call is cleared and retried at the next launch, which meanwhile reports its own error for a plan beyond 64 KB.
constexpr int PM_MAX_DEVICES = 64;
inline int pm_device_cus(int dev) {
  static std::atomic<int> cached[PM_MAX_DEVICES];
  const bool keep = dev >= 0 && dev < PM_MAX_DEVICES;
  int n = keep ? cached[dev].load(std::memory_order_relaxed) : 0;
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (keep) cached[dev].store(n, std::memory_order_relaxed);
  return n;
}
struct pm_lds_optin {
  std::atomic<bool> done[PM_MAX_DEVICES] = {};
  int operator()(const void* kernel, int lds_bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const bool keep = dev >= 0 && dev < PM_MAX_DEVICES;
    if (!keep || !done[dev].load(std::memory_order_acquire)) {
      if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) (void)hipGetLastError();
      else if (keep) done[dev].store(true, std::memory_order_release);
    }
    return pm_device_cus(dev);
  }
};

// the library's routing state (conv_igemm.hip): one struct, see include/pinmem_hip.h pm_routing
extern pm_routing pm_route;


// ---- device helpers -------------------------------------------------------------------------------------------
// XCD-aware bijective remap of a block id: workgroups are dealt round-robin to the 8 XCDs, each with its own 4 MB L2; consecutive LOGICAL ids (which share an operand
// panel: the A rows of a GEMM tile row, the low-res logit rows of the fused upsample + CE, the V rows of the fused Winograd) land on one XCD and re-use its L2.
__device__ __forceinline__ int pm_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}
// eight bf16 channels (16 bytes) <-> eight floats. Round to nearest even on the way out (v_cvt_pk_bf16_f32).
__device__ __forceinline__ void pm_ld8(const pm_bf16* p, float* v) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(q.x << 16), v[1] = __uint_as_float(q.x & 0xffff0000u), v[2] = __uint_as_float(q.y << 16), v[3] = __uint_as_float(q.y & 0xffff0000u);
  v[4] = __uint_as_float(q.z << 16), v[5] = __uint_as_float(q.z & 0xffff0000u), v[6] = __uint_as_float(q.w << 16), v[7] = __uint_as_float(q.w & 0xffff0000u);
}
__device__ __forceinline__ unsigned pm_pack_bf16(float a, float b) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  bf16x2_t o;
  o[0] = (__bf16)a, o[1] = (__bf16)b;
  return __builtin_bit_cast(unsigned, o);
}
__device__ __forceinline__ void pm_st8(pm_bf16* p, const float* v) {
  uint4 q;
  q.x = pm_pack_bf16(v[0], v[1]), q.y = pm_pack_bf16(v[2], v[3]), q.z = pm_pack_bf16(v[4], v[5]), q.w = pm_pack_bf16(v[6], v[7]);
  *reinterpret_cast<uint4*>(p) = q;
}
__device__ __forceinline__ float pm_bf16_to_f32(pm_bf16 h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ pm_bf16 pm_f32_to_bf16(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }

// BatchNorm statistics of one 32-row slab of a bf16 convolution output, taken where the slab is still parked in LDS as fp32 (the staged epilogues of conv16.hip
// and conv_igemm.hip): the values are first rounded to bf16 exactly as they are stored -- the statistics are those of the tensor the BatchNorm will read -- then,
// per column, the mean over the valid rows and M2 around it (two passes over LDS, as the fp32 statistics epilogue). A lane owns eight columns (cc ... cc + 7) of rows
// rr0 + k * RPI; the RPI... 64 / LPR lanes sharing a column group are combined by lane exchanges in a fixed order. Output layout = pm_bn_partials_finalize's:
// stats[(slab * Nn + col) * 2 + {0: mean, 1: M2}]. bi / sc / sh: the fused affine of the epilogue (identity in train mode unless the convolution has a bias).
template <int LDC, int LPR, int RPI>
__device__ __forceinline__ void pm_slab_stats16(const float* Ws, int rr0, int cc, long slab_row0, long M, long Nn, int col, bool cok, const float* bi, const float* sc,
                                                const float* sh, float* stats) {
  const float cnt = (float)max(0l, min(32l, M - slab_row0));
  float s1[8], mu[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1[e] = 0.f, m2[e] = 0.f;
  auto slab_row = [&](int r0, float* v) {
    const float4 v0 = *reinterpret_cast<const float4*>(Ws + (r0 + rr0) * LDC + cc), v1 = *reinterpret_cast<const float4*>(Ws + (r0 + rr0) * LDC + cc + 4);
    const float t[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = pm_bf16_to_f32(pm_f32_to_bf16((t[e] + bi[e]) * sc[e] + sh[e]));
    return slab_row0 + r0 + rr0 < M;
  };
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += RPI) {
    float v[8];
    const bool rok = slab_row(r0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] += rok ? v[e] : 0.f;
  }
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] += __shfl_xor(s1[e], o, 64);
#pragma unroll
  for (int e = 0; e < 8; ++e) mu[e] = cnt > 0.f ? s1[e] / cnt : 0.f;
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += RPI) {
    float v[8];
    const bool rok = slab_row(r0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = v[e] - mu[e];
      m2[e] += rok ? d * d : 0.f;
    }
  }
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) m2[e] += __shfl_xor(m2[e], o, 64);
  if (rr0 == 0 && cok && cnt > 0.f) {
    float* dst = stats + ((slab_row0 >> 5) * Nn + col) * 2;
#pragma unroll
    for (int e = 0; e < 8; e += 2) *reinterpret_cast<float4*>(dst + 2 * e) = make_float4(mu[e], m2[e], mu[e + 1], m2[e + 1]);
  }
}

// BatchNorm's y = (x - mean) * invstd * gamma + beta, evaluated the same way wherever it appears -- the apply pass, every backward pass that rebuilds the ReLU mask
// from x, the max pool that normalises its taps itself (two explicit FMAs: bit-identical in all of them whatever the compiler would contract).
__device__ __forceinline__ float pm_bn_affine(float v, float mu, float is, float ga, float be) {
  const float s = is * ga;
  return fmaf(v, s, fmaf(-mu, s, be));
}

// ToTensor + Normalize of one pixel (torchvision's order: / 255, - mean, / std; zero 4th channel), evaluated the same way wherever it appears -- pm_image_u8_to_nhwc4
// and pm_eval_tiles_u8 -- whatever the translation unit's contraction setting.
__device__ __forceinline__ float4 pm_normalise_u8(const uint8_t* q, float m0, float m1, float m2, float s0, float s1, float s2) {
#pragma clang fp contract(off)
  return make_float4(((float)q[0] / 255.f - m0) / s0, ((float)q[1] / 255.f - m1) / s1, ((float)q[2] / 255.f - m2) / s2, 0.f);
}

__device__ __forceinline__ float pm_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float pm_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// the class limit of the loss and evaluation kernels (per-class registers, C x C LDS counters)
constexpr int PM_MAX_CLASSES = 32;

// Confusion-matrix fold of the evaluation kernels (loss.hip, sliding_eval.hip): hist[e] (+)= sum over the blocks' count rows: 32 entries x 32 slices of the rows per
// block, integer adds only -- order-free, so deterministic. `static`: each of the two translation units that launch it compiles its own copy, and one that
// never names it emits no code for it, so the other sources' code objects are what they were.
constexpr int PM_HIST_FOLD_T = 1024;
static __global__ __launch_bounds__(PM_HIST_FOLD_T) void pm_hist_fold_kernel(const unsigned* __restrict__ counts, int nblk, int entries, int accumulate,
                                                                             int64_t* __restrict__ hist) {
  __shared__ unsigned long long tot[32];
  const int e = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
  if (threadIdx.x < 32) tot[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long a = 0ull;
  if (e < entries)
    for (int r = sl; r < nblk; r += PM_HIST_FOLD_T / 32) a += counts[(long)r * entries + e];
  if (a) atomicAdd(&tot[threadIdx.x & 31], a);
  __syncthreads();
  if (threadIdx.x < 32 && e < entries) hist[e] = (accumulate ? hist[e] : 0) + (int64_t)tot[threadIdx.x];
}

// ATen's align_corners=True source-index math, in fp32 exactly as area_pixel_compute_scale /
// area_pixel_compute_source_index do it (scale = (in-1)/(out-1) in float, src = scale*dst).
struct pm_lerp {
  int i0, i1;
  float w0, w1;
};
__host__ __device__ __forceinline__ float pm_ac_scale(int in, int out) {
  return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
}
__device__ __forceinline__ pm_lerp pm_ac_lerp(float scale, int dst, int in) {
  float src = scale * (float)dst;
  int i0 = (int)src;                       // src >= 0 -> truncation == floor
  if (i0 > in - 1) i0 = in - 1;
  int i1 = i0 + (i0 < in - 1 ? 1 : 0);
  float l1 = src - (float)i0;
  if (l1 < 0.f) l1 = 0.f;
  if (l1 > 1.f) l1 = 1.f;
  pm_lerp r;
  r.i0 = i0;
  r.i1 = i1;
  r.w1 = l1;
  r.w0 = 1.f - l1;
  return r;
}

// The transposed operator (every resize backward pass, and the fused up-sample + loss backward): output indices whose taps may touch input index `i`, a
// conservative [lo, hi] from the inverse map -- each is verified exactly by pm_tap_weight, the weight output index (lerp l) puts on input index i.
__device__ __forceinline__ void pm_support(float scale, int i, int out, int& lo, int& hi) {
  if (scale <= 0.f) {
    lo = 0, hi = out - 1;
    return;
  }
  const float inv = 1.f / scale;
  lo = max(0, (int)floorf(((float)i - 1.f) * inv) - 1);
  hi = min(out - 1, (int)ceilf(((float)i + 1.f) * inv) + 1);
}
__device__ __forceinline__ float pm_tap_weight(const pm_lerp& l, int i) { return (l.i0 == i ? l.w0 : 0.f) + (l.i1 == i ? l.w1 : 0.f); }

// ---- generic NHWC elementwise driver: thread -> (pixel, 4 channels) ----------------------------------------------
// VEC=true needs 16B-aligned views with c % 4 == 0 (pm_vec4). f(pixel, channel) is a __device__ lambda.
template <bool VEC, typename F>
__global__ __launch_bounds__(256) void pm_ew_kernel(long pixels, int c, F f) {
  const int cg = VEC ? c / 4 : c;
  const long total = pixels * cg;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i / cg;
    const int ch = (int)(i - p * cg) * (VEC ? 4 : 1);
    f(p, ch);
  }
}
static inline int pm_ew_grid(long work) { return (int)std::min<long>((work + 255) / 256, 256 * 16); }
template <typename F>
static inline int pm_ew_launch(bool vec, long pixels, int c, hipStream_t st, const char* name, F f) {
  if (pixels * c == 0) return PM_OK;
  if (vec) hipLaunchKernelGGL((pm_ew_kernel<true, F>), dim3(pm_ew_grid(pixels * c / 4)), dim3(256), 0, st, pixels, c, f);
  else hipLaunchKernelGGL((pm_ew_kernel<false, F>), dim3(pm_ew_grid(pixels * c)), dim3(256), 0, st, pixels, c, f);
  return pm_check_launch(name);
}
static inline bool pm_same_shape(const pm_tensor* a, const pm_tensor* b) { return a->n == b->n && a->h == b->h && a->w == b->w && a->c == b->c; }
static inline bool pm_vec4(const pm_tensor* t) { return pm_vec_ok(t) && t->c % 4 == 0; }
#define PM_LD4(ptr) (*reinterpret_cast<const float4*>(ptr))
#define PM_ST4(ptr, v) (*reinterpret_cast<float4*>(ptr) = (v))

// eight fp32 values (two 16-byte loads): per-channel parameters next to an eight-channel bf16 access
__device__ __forceinline__ void pm_ld8f(const float* p, float* v) {
  const float4 a = PM_LD4(p), b = PM_LD4(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
// the elementwise driver of the bf16 tier: thread -> (pixel, 8 channels)
template <typename F>
__global__ __launch_bounds__(256) void pm_ew16_kernel(long pixels, int cg, F f) {
  const long total = pixels * cg;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i / cg;
    f(p, (int)(i - p * cg) * 8);
  }
}
template <typename F>
static inline int pm_ew16_launch(long pixels, int c, hipStream_t st, const char* name, F f) {
  if (pixels * c == 0) return PM_OK;
  const long work = pixels * (c / 8);
  hipLaunchKernelGGL((pm_ew16_kernel<F>), dim3((int)std::min<long>((work + 255) / 256, 256 * 16)), dim3(256), 0, st, pixels, c / 8, f);
  return pm_check_launch(name);
}

// ---- the element trait: what differs between the fp32 and the bf16 activation tier ---------------------------------------------------------------------------------
// A lane moves 16 bytes = V channels; values are widened to fp32 in registers and travel as float[V] (every loop over V fully unrolled); bf16 results are rounded
// (nearest even) once, on the way out. One kernel template over T serves both tiers (bn.hip, pool_resize.hip, misc.hip).
template <typename T>
struct pm_elem;
template <>
struct pm_elem<float> {
  static constexpr int V = 4;      // channels per 16-byte lane access
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 a = PM_LD4(p);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { PM_ST4(p, make_float4(v[0], v[1], v[2], v[3])); }
  static __device__ __forceinline__ float widen(float v) { return v; }
  static __device__ __forceinline__ float narrow(float v) { return v; }
  static int gpr(int) { return 16; }      // BatchNorm reductions, lane groups per pixel row: 16 float4 groups x 16 row lanes
  static bool vec(const pm_tensor* t) { return pm_vec4(t); }
  static int check(const pm_tensor* t, const char* who) {
    PM_REQUIRE_F32(t, who);      // a mixed-type call ends here
    PM_REQUIRE(t && t->ptr && pm_vec4(t), PM_EINVAL, "%s: tensor must be 16B aligned, pitch %% 4 == 0 and C %% 4 == 0", who);
    return PM_OK;
  }
};
template <>
struct pm_elem<pm_bf16> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void ld(const pm_bf16* p, float* v) { pm_ld8(p, v); }
  static __device__ __forceinline__ void st(pm_bf16* p, const float* v) { pm_st8(p, v); }
  static __device__ __forceinline__ float widen(pm_bf16 v) { return pm_bf16_to_f32(v); }
  static __device__ __forceinline__ pm_bf16 narrow(float v) { return pm_f32_to_bf16(v); }
  static int gpr(int C) { return C <= 64 ? 8 : 16; }      // 8 for tensors of <= 64 channels: no idle half-waves on the 64-channel maps of layer1
  static bool vec(const pm_tensor* t) { return pm_vec8(t); }
  static int check(const pm_tensor* t, const char* who) {
    PM_REQUIRE(t && t->ptr && pm_vec8(t), PM_EINVAL, "%s: bf16 tensors must be 16B aligned with pitch %% 8 == 0 and C %% 8 == 0", who);
    return PM_OK;
  }
};
// V channels of a T tensor <-> float[V]: V = pm_elem<T>::V (one 16-byte access) or 1 (the scalar fallbacks of odd fp32 views)
template <typename T, int V>
__device__ __forceinline__ void pm_ldv(const T* p, float* v) {
  if constexpr (V == 1) v[0] = pm_elem<T>::widen(*p);
  else pm_elem<T>::ld(p, v);
}
template <typename T, int V>
__device__ __forceinline__ void pm_stv(T* p, const float* v) {
  if constexpr (V == 1) *p = pm_elem<T>::narrow(v[0]);
  else pm_elem<T>::st(p, v);
}
// V per-channel fp32 values (mean, invstd, gamma, beta, sums; the fp32 workspace of the separable resize backward)
template <int V>
__device__ __forceinline__ void pm_ldp(const float* p, float* v) {
  if constexpr (V == 4) pm_elem<float>::ld(p, v);
  else pm_ld8f(p, v);
}
template <int V>
__device__ __forceinline__ void pm_stp(float* p, const float* v) {
  pm_elem<float>::st(p, v);
  if constexpr (V == 8) pm_elem<float>::st(p + 4, v + 4);
}
// thread -> (pixel, V channels), f(pixel, channel) a __device__ lambda
template <typename T, typename F>
int pm_ew_launch_as(long pixels, int c, hipStream_t st, const char* name, F f) {
  if constexpr (pm_elem<T>::V == 8) {
    return pm_ew16_launch(pixels, c, st, name, f);
  } else {      // pm_ew_launch(true, ...) without its scalar twin
    if (pixels * c == 0) return PM_OK;
    hipLaunchKernelGGL((pm_ew_kernel<true, F>), dim3(pm_ew_grid(pixels * c / 4)), dim3(256), 0, st, pixels, c, f);
    return pm_check_launch(name);
  }
}
// grid of the grid-stride pooling / resize / conversion kernels (256 threads, one work item each per trip)
static inline int pm_grid_for(long work) { return (int)std::min<long>((work + 255) / 256, 256 * 32); }

// Gradient of input pixel ip (channels ch ... ch + V - 1) of a 3x3 / stride 2 / pad 1 max pool: the sum, in window order, of dy over the (at most four) windows that
// cover the pixel and whose argmax byte names this tap; the V argmax bytes come as one load. A gather: no atomics, deterministic. The only copy of the window walk:
// the pool's own backward on both tiers (V = 1: the scalar fallback) and the BatchNorm backward passes that read a pooled gradient (the stem) produce the same bits.
template <typename T, int V>
__device__ __forceinline__ void pm_maxpool_gather(const T* __restrict__ dy, long dp, int Ho, int Wo, const uint8_t* __restrict__ arg, int H, int W, int C, long ip, int ch,
                                                  float* g) {
  const int ix = (int)(ip % W), iy = (int)((ip / W) % H), n = (int)(ip / ((long)W * H));
#pragma unroll
  for (int e = 0; e < V; ++e) g[e] = 0.f;
  const int oy_hi = min((iy + 1) >> 1, Ho - 1), ox_hi = min((ix + 1) >> 1, Wo - 1);
  for (int oy = iy >> 1; oy <= oy_hi; ++oy) {
    const int ky = iy + 1 - 2 * oy;
    if (ky < 0 || ky > 2) continue;
    for (int ox = ix >> 1; ox <= ox_hi; ++ox) {
      const int kx = ix + 1 - 2 * ox;
      if (kx < 0 || kx > 2) continue;
      const long op = (long)(n * Ho + oy) * Wo + ox;
      const uint8_t* ap = arg + op * C + ch;
      uint2 a = make_uint2(0u, 0u);
      if constexpr (V == 1) a.x = *ap;
      else if constexpr (V == 4) a.x = *reinterpret_cast<const unsigned*>(ap);
      else a = *reinterpret_cast<const uint2*>(ap);
      const unsigned want = (unsigned)(ky * 3 + kx);
      float d[V];
      pm_ldv<T, V>(dy + op * dp + ch, d);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const unsigned b = ((e < 4 ? a.x : a.y) >> (8 * (e & 3))) & 255u;
        g[e] += b == want ? d[e] : 0.f;
      }
    }
  }
}
