// The image dumps of evaluation (eval.py:664-693 RunEval.inf under --dump_images): the colourised class map, its blend with the source image, the difference image and
// the label-id map, from the uint8 class map the evaluation kernels left on the device. One streaming pass over the pixels: at most 12 bytes read and 10 written per
// pixel, no atomics, no workspace. A thread takes 4 consecutive pixels, so that every 3-byte-pixel array moves as 12 aligned bytes and the class map and the id map as
// one dword; the pixels behind the last whole group take the same per-pixel body one at a time.
#include "pm_common.h"

#include "augment_math.h"      // pm_aug_blend: PIL's Blend.c, not contracted into an FMA

namespace {

struct DumpArgs {
  const uint8_t* pred;
  const uint8_t* image;
  const int64_t* labels;
  uint8_t *color, *compose, *diff, *ids;
  float alpha;
};
struct DumpPixel {
  uint32_t color, compose, diff, id;      // the colours as r | g << 8 | b << 16
};
struct Bytes12 {      // 4 RGB pixels
  uint32_t d[3];
};

// The only copy of the per-pixel rules. pal / tab: the block's LDS copies (palette rows packed as above). An output nobody asked for is not computed.
__device__ __forceinline__ DumpPixel dump_pixel(const DumpArgs& a, const uint32_t* pal, const uint8_t* tab, uint32_t cls, uint32_t im, int64_t label) {
  DumpPixel o = {0u, 0u, 0xffffffu, 0u};
  if (a.color || a.compose || a.diff) o.color = pal[cls];
  if (a.compose || a.diff) {
#pragma unroll
    for (int sh = 0; sh < 24; sh += 8) o.compose |= (uint32_t)(uint8_t)pm_aug_blend((int)((im >> sh) & 255u), (int)((o.color >> sh) & 255u), a.alpha) << sh;
  }
  if (a.diff && label != 255 && label != (int64_t)cls) o.diff = o.compose;      // lighter(blend, invert(diff)): the blend where diff is set, white elsewhere
  if (a.ids) o.id = tab[cls];
  return o;
}

__device__ __forceinline__ void unpack4(const Bytes12& b, uint32_t* px) {
  px[0] = b.d[0] & 0xffffffu;
  px[1] = (b.d[0] >> 24) | ((b.d[1] & 0xffffu) << 8);
  px[2] = (b.d[1] >> 16) | ((b.d[2] & 0xffu) << 16);
  px[3] = b.d[2] >> 8;
}
__device__ __forceinline__ Bytes12 pack4(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) { return {{p0 | (p1 << 24), (p1 >> 8) | (p2 << 16), (p2 >> 16) | (p3 << 8)}}; }
__device__ __forceinline__ void store3(uint8_t* q, uint32_t v) { q[0] = (uint8_t)v, q[1] = (uint8_t)(v >> 8), q[2] = (uint8_t)(v >> 16); }

// groups: the number of 4-pixel groups moved as dwords (pixels / 4, or 0 where pred / ids are not dword aligned); the pixels from 4 * groups on go one by one.
__global__ __launch_bounds__(256) void eval_dump_kernel(DumpArgs a, const uint8_t* __restrict__ palette, const uint8_t* __restrict__ id_table, long groups, long pixels) {
  __shared__ uint32_t pal[256];
  __shared__ uint8_t tab[256];
  const int tid = threadIdx.x;
  pal[tid] = palette ? (uint32_t)palette[3 * tid] | ((uint32_t)palette[3 * tid + 1] << 8) | ((uint32_t)palette[3 * tid + 2] << 16) : 0u;
  tab[tid] = id_table ? id_table[tid] : (uint8_t)0;
  __syncthreads();
  const bool blend = a.compose || a.diff;
  const long first = (long)blockIdx.x * 256 + tid, stride = (long)gridDim.x * 256;
  for (long g = first; g < groups; g += stride) {
    const uint32_t cls = *reinterpret_cast<const uint32_t*>(a.pred + 4 * g);
    uint32_t im[4] = {0u, 0u, 0u, 0u};
    if (blend) unpack4(*reinterpret_cast<const Bytes12*>(a.image + 12 * g), im);
    int64_t lab[4] = {255, 255, 255, 255};
    if (a.diff) {
#pragma unroll
      for (int k = 0; k < 4; ++k) lab[k] = a.labels[4 * g + k];
    }
    DumpPixel o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = dump_pixel(a, pal, tab, (cls >> (8 * k)) & 255u, im[k], lab[k]);
    if (a.color) *reinterpret_cast<Bytes12*>(a.color + 12 * g) = pack4(o[0].color, o[1].color, o[2].color, o[3].color);
    if (a.compose) *reinterpret_cast<Bytes12*>(a.compose + 12 * g) = pack4(o[0].compose, o[1].compose, o[2].compose, o[3].compose);
    if (a.diff) *reinterpret_cast<Bytes12*>(a.diff + 12 * g) = pack4(o[0].diff, o[1].diff, o[2].diff, o[3].diff);
    if (a.ids) *reinterpret_cast<uint32_t*>(a.ids + 4 * g) = o[0].id | (o[1].id << 8) | (o[2].id << 16) | (o[3].id << 24);
  }
  for (long p = 4 * groups + first; p < pixels; p += stride) {
    uint32_t im = 0u;
    if (blend) im = (uint32_t)a.image[3 * p] | ((uint32_t)a.image[3 * p + 1] << 8) | ((uint32_t)a.image[3 * p + 2] << 16);
    const DumpPixel o = dump_pixel(a, pal, tab, a.pred[p], im, a.diff ? a.labels[p] : 255);
    if (a.color) store3(a.color + 3 * p, o.color);
    if (a.compose) store3(a.compose + 3 * p, o.compose);
    if (a.diff) store3(a.diff + 3 * p, o.diff);
    if (a.ids) a.ids[p] = (uint8_t)o.id;
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int pm_eval_dump(const uint8_t* pred, int64_t pixels, const uint8_t* palette, const uint8_t* image, const int64_t* labels, const uint8_t* id_table, float alpha,
                            uint8_t* color, uint8_t* compose, uint8_t* diff, uint8_t* ids, void* stream) {
  const char* who = "eval_dump";
  PM_REQUIRE(pred, PM_EINVAL, "%s: pred is null", who);
  PM_REQUIRE(pixels > 0, PM_EINVAL, "%s: pixels must be positive (got %ld)", who, (long)pixels);
  PM_REQUIRE(color || compose || diff || ids, PM_EINVAL, "%s: no output requested", who);
  PM_REQUIRE(!(color || compose || diff) || palette, PM_EINVAL, "%s: color / compose / diff need the palette", who);
  PM_REQUIRE(!(compose || diff) || image, PM_EINVAL, "%s: compose / diff need the image", who);
  PM_REQUIRE(!diff || labels, PM_EINVAL, "%s: diff needs the labels", who);
  PM_REQUIRE(!ids || id_table, PM_EINVAL, "%s: ids need the id table", who);
  PM_REQUIRE(std::isfinite(alpha), PM_EINVAL, "%s: alpha must be finite", who);
  PM_REQUIRE(aligned_to(image, 4) && aligned_to(color, 4) && aligned_to(compose, 4) && aligned_to(diff, 4), PM_EINVAL,
             "%s: image / color / compose / diff must be 4-byte aligned", who);
  PM_REQUIRE(aligned_to(labels, 8), PM_EINVAL, "%s: labels must be 8-byte aligned", who);
  const long groups = aligned_to(pred, 4) && aligned_to(ids, 4) ? (long)(pixels / 4) : 0;
  const DumpArgs a = {pred, image, labels, color, compose, diff, ids, alpha};
  hipLaunchKernelGGL(eval_dump_kernel, dim3(pm_grid_for(std::max<long>(groups, pixels - 4 * groups))), dim3(256), 0, (hipStream_t)stream, a, palette, id_table, groups,
                     (long)pixels);
  return pm_check_launch(who);
}
