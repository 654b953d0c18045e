// Resampling input edge: RandomSizeAndCrop's antialiased bicubic resize (image) and nearest resize (mask), pad and crop, for the crop window alone, with PIL's
// bytes (include/pinmem_hip.h, pm_resample_crop_u8). The host writes PIL's coefficient tables for the window (pm_resample_tables: double arithmetic, fixed point
// 2^22); one kernel stages a tile's source footprint in LDS, filters it along W into bytes in a second LDS buffer, filters those along H and gathers the labels.
#include "pm_common.h"

#include <math.h>

#pragma clang fp contract(off)      // the library is built with -ffp-contract=fast: a fused multiply-add below would change a weight's last bit and a truncated coefficient

namespace {
constexpr int TH = 32, TW = 64, REC = PM_RESAMPLE_REC, MAXT = PM_RESAMPLE_MAX_TAPS, PREC = 22;
constexpr int NT = 512, NW = NT / 64;               // eight waves per block, two blocks per CU: the passes are chains of LDS reads, waves hide them
constexpr int ROWB = TW * 3;                       // bytes per row of the horizontally filtered tile
constexpr int MID_ROWS = 80;                       // source rows one pass holds: 32 output rows at in / out = 2 reach over 74
constexpr int SRC_BYTES = 32768;                   // the staged footprint, rows padded to dwords: 74 x 138 pixels at in / out = 2; and MAXT rows of the widest footprint (64 columns at 5.75)
constexpr int STAGE_U = MID_ROWS / NW / 2;         // rows a wave has in flight while staging
constexpr int TAB_BYTES = (TH + TW) * REC * 4;     // 9 984: the tile's row and column records
constexpr int LDS_BYTES = TAB_BYTES + MID_ROWS * ROWB + SRC_BYTES;      // 58 112: two blocks per CU

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// Records of `cnt` positions from `pos0` on into LDS, positions past `lim` as pad; first index and tap count clamped so that no table content leads outside [0, in).
__device__ __forceinline__ void load_records(int* dst, const int32_t* __restrict__ tab, int pos0, int cnt, int lim, int in, int tid) {
  for (int i = tid; i < cnt * REC; i += NT) {
    const int p = i / REC;
    dst[i] = pos0 + p < lim ? tab[(long)(pos0 + p) * REC + (i - p * REC)] : 0;
  }
  __syncthreads();
  if (tid < cnt) {
    int* r = dst + tid * REC;
    const int x0 = min(max(r[0], 0), in - 1), c = min(min(max(r[1], 0), MAXT), in - x0);
    r[0] = x0, r[1] = c;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void resample_crop_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab, int Hs, int Ws,
                                                            const pm_geo_image* __restrict__ geo, const int32_t* __restrict__ bic_rows,
                                                            const int32_t* __restrict__ bic_cols, const int32_t* __restrict__ near_rows,
                                                            const int32_t* __restrict__ near_cols, int th, int tw, int ignore, uint8_t* __restrict__ out_img,
                                                            uint8_t* __restrict__ out_lab) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* rtab = reinterpret_cast<int*>(smem);                  // [TH][REC]
  int* ctab = rtab + TH * REC;                               // [TW][REC]
  uint8_t* mid = smem + TAB_BYTES;                           // [MID_ROWS][ROWB]: source rows filtered along W
  uint8_t* stage = mid + MID_ROWS * ROWB;                    // the source footprint of the rows in `mid`
  const int n = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, tid = threadIdx.x;
  const pm_geo_image G = geo[n];
  const int h_in = min(max(G.h_in, 1), Hs), w_in = min(max(G.w_in, 1), Ws);
  const int nr = min(TH, th - y0), nc = min(TW, tw - x0);
  const long slab = (long)Hs * Ws;

  // labels: a gather through the two nearest tables
  {
    const uint8_t* src = lab + (long)n * slab;
    const int32_t *ry = near_rows + (long)n * th + y0, *rx = near_cols + (long)n * tw + x0;
    uint8_t* dst = out_lab + ((long)n * th + y0) * tw + x0;
    for (int i = tid; i < nr * TW; i += NT) {
      const int ly = i / TW, lx = i - ly * TW;
      if (lx >= nc) continue;
      const int sy = ry[ly], sx = rx[lx];
      dst[(long)ly * tw + lx] = (sy < 0 || sx < 0) ? (uint8_t)ignore : src[(long)min(sy, h_in - 1) * Ws + min(sx, w_in - 1)];
    }
  }

  load_records(rtab, bic_rows + (long)n * th * REC, y0, TH, th, h_in, tid);
  load_records(ctab, bic_cols + (long)n * tw * REC, x0, TW, tw, w_in, tid);

  // source columns the tile reads: [fx0, fx1) over the columns with taps (every lane computes the same: broadcast reads)
  int fx0 = w_in, fx1 = 0;
  for (int x = 0; x < TW; ++x) {
    const int a = ctab[x * REC], c = ctab[x * REC + 1];
    if (c > 0) fx0 = min(fx0, a), fx1 = max(fx1, a + c);
  }
  const int fw = max(fx1 - fx0, 0), fwb = fw * 3, spb = (fwb + 3) & ~3;      // staged rows start on a dword
  const uint8_t* src = img + (long)n * slab * 3;
  uint8_t* dst = out_img + (((long)n * th + y0) * tw + x0) * 3;
  const bool vec = (((long)tw * 3) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_img) & 3) == 0;      // every tile row starts on a dword and ends on one
  const int wave = tid >> 6, lane = tid & 63;

  // the tile's rows in passes of as many as fit: the source rows of a pass go through `stage` into `mid`
  for (int ya = 0; ya < nr;) {
    int fy0 = h_in, fy1 = 0, yb = ya;
    for (; yb < nr; ++yb) {
      const int a = rtab[yb * REC], c = rtab[yb * REC + 1];
      const int lo = c > 0 ? min(fy0, a) : fy0, hi = c > 0 ? max(fy1, a + c) : fy1;
      if (yb > ya && (hi - lo > MID_ROWS || (hi - lo) * spb > SRC_BYTES)) break;
      fy0 = lo, fy1 = hi;
    }
    int fh = max(fy1 - fy0, 0);
    if (fh > MID_ROWS || fh * spb > SRC_BYTES) fh = 0;      // one row alone does not fit: not a table of pm_resample_tables; its pixels come out as the rounding constant, 0

    // staging: a wave takes rows wave, wave + NW, ...; its lanes the dwords of a row (loaded from any byte address), STAGE_U rows in flight; the last 0 .. 3 bytes of a
    // row go one by one, so no byte outside the footprint is read
    for (int q = lane; q < (fwb >> 2); q += 64) {
      for (int r0 = wave; r0 < fh; r0 += NW * STAGE_U) {
        unsigned v[STAGE_U];
#pragma unroll
        for (int u = 0; u < STAGE_U; ++u)
          if (r0 + u * NW < fh) __builtin_memcpy(&v[u], src + ((long)(fy0 + r0 + u * NW) * Ws + fx0) * 3 + 4 * q, 4);
#pragma unroll
        for (int u = 0; u < STAGE_U; ++u)
          if (r0 + u * NW < fh) reinterpret_cast<unsigned*>(stage + (r0 + u * NW) * spb)[q] = v[u];
      }
    }
    if (lane < (fwb & 3))
      for (int r = wave; r < fh; r += NW) stage[r * spb + (fwb & ~3) + lane] = src[((long)(fy0 + r) * Ws + fx0) * 3 + (fwb & ~3) + lane];
    __syncthreads();
    for (int i = tid; i < fh * TW; i += NT) {               // along W: one pixel of one staged row per lane
      const int r = i / TW, x = i - r * TW;
      const int* rec = ctab + x * REC;
      const int c = rec[1];
      const uint8_t* p = stage + r * spb + (rec[0] - fx0) * 3;
      int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
      for (int j = 0; j < c; ++j) {
        const int k = rec[2 + j];
        s0 += p[3 * j] * k, s1 += p[3 * j + 1] * k, s2 += p[3 * j + 2] * k;
      }
      uint8_t* m = mid + r * ROWB + x * 3;                   // a pad column (no taps) holds 0, and stays 0 along H
      m[0] = (uint8_t)clip8(s0 >> PREC), m[1] = (uint8_t)clip8(s1 >> PREC), m[2] = (uint8_t)clip8(s2 >> PREC);
    }
    __syncthreads();
    for (int i = tid; i < (yb - ya) * (ROWB / 4); i += NT) {      // along H: four bytes of one output row per lane
      const int ly = ya + i / (ROWB / 4), e = (i % (ROWB / 4)) * 4;
      const int* rec = rtab + ly * REC;
      const int c = fh > 0 ? rec[1] : 0;
      const uint8_t* p = mid + (rec[0] - fy0) * ROWB + e;
      int s[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
      for (int j = 0; j < c; ++j) {
        const unsigned v = *reinterpret_cast<const unsigned*>(p + j * ROWB);
        const int k = rec[2 + j];
        s[0] += (int)(v & 255u) * k, s[1] += (int)((v >> 8) & 255u) * k, s[2] += (int)((v >> 16) & 255u) * k, s[3] += (int)(v >> 24) * k;
      }
      uint8_t* o = dst + (long)ly * tw * 3 + e;
      if (vec) {
        if (e < nc * 3)
          *reinterpret_cast<unsigned*>(o) = (unsigned)clip8(s[0] >> PREC) | (unsigned)clip8(s[1] >> PREC) << 8 | (unsigned)clip8(s[2] >> PREC) << 16 |
                                            (unsigned)clip8(s[3] >> PREC) << 24;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (e + b < nc * 3) o[b] = (uint8_t)clip8(s[b] >> PREC);
      }
    }
    __syncthreads();      // `stage` and `mid` are free for the next pass
    ya = yb;
  }
}

// PIL's bicubic (Resample.c bicubic_filter, a = -0.5)
double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc of Resample.c for output positions [p0 - pad, p0 - pad + cnt) of an axis resized from `in` to `out`; false: over the tap cap
bool bicubic_axis(int in, int out, int pad, int p0, int cnt, int32_t* rec, int* taps_needed) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, ss = 1.0 / fs;
  for (int i = 0; i < cnt; ++i) {
    int32_t* r = rec + (long)i * REC;
    for (int j = 0; j < REC; ++j) r[j] = 0;
    const int xx = p0 - pad + i;
    if (xx < 0 || xx >= out) continue;      // pad: no taps
    if (in == out) {                        // PIL skips the pass: a copy
      r[0] = xx, r[1] = 1, r[2] = 1 << PREC;
      continue;
    }
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > MAXT) {
      *taps_needed = xmax;
      return false;
    }
    double w[MAXT], ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = bicubic((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    r[0] = xmin, r[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) w[x] /= ww;
      r[2 + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PREC)) : (int)(0.5 + w[x] * (1 << PREC));
    }
  }
  return true;
}

// ImagingScaleAffine of Geometry.c (what Image.resize(NEAREST) runs): the source coordinate is accumulated from output position 0
void nearest_axis(int in, int out, int pad, int p0, int cnt, int32_t* idx) {
  const double a = (double)in / (double)out;
  double xo = a * 0.5;
  for (int i = 0; i < cnt; ++i) idx[i] = -1;
  const int end = std::min(out, p0 - pad + cnt);
  for (int x = 0; x < end; ++x, xo += a) {
    const int i = x - (p0 - pad);
    if (i >= 0) idx[i] = std::min((int)xo, in - 1);
  }
}
}  // namespace

extern "C" int pm_resample_tables(const pm_geo_image* g, int32_t struct_size, int Hs, int Ws, int th, int tw, int32_t* bic_rows, int32_t* bic_cols, int32_t* near_rows,
                                  int32_t* near_cols) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_geo_image), PM_EINVAL, "resample_tables: pm_geo_image struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)",
             struct_size, sizeof(pm_geo_image), PM_ABI_VERSION);
  PM_REQUIRE(g && bic_rows && bic_cols && near_rows && near_cols, PM_EINVAL, "resample_tables: null pointer");
  PM_REQUIRE(g->h_in > 0 && g->w_in > 0 && g->h > 0 && g->w > 0 && th > 0 && tw > 0 && g->pad_h >= 0 && g->pad_w >= 0, PM_EINVAL,
             "resample_tables: empty size or negative pad (source %d x %d, resized %d x %d, crop %d x %d, pad %d, %d)", g->h_in, g->w_in, g->h, g->w, th, tw, g->pad_h, g->pad_w);
  PM_REQUIRE(g->h_in <= Hs && g->w_in <= Ws, PM_EINVAL, "resample_tables: image %d x %d larger than its slab %d x %d", g->h_in, g->w_in, Hs, Ws);
  PM_REQUIRE(g->y1 >= 0 && g->x1 >= 0 && (long)g->y1 + th <= (long)g->h + 2l * g->pad_h && (long)g->x1 + tw <= (long)g->w + 2l * g->pad_w, PM_EINVAL,
             "resample_tables: crop %d x %d at (%d, %d) outside the padded image %ld x %ld", th, tw, g->y1, g->x1, (long)g->h + 2l * g->pad_h, (long)g->w + 2l * g->pad_w);
  int need = 0;
  const bool ok = bicubic_axis(g->h_in, g->h, g->pad_h, g->y1, th, bic_rows, &need) && bicubic_axis(g->w_in, g->w, g->pad_w, g->x1, tw, bic_cols, &need);
  PM_REQUIRE(ok, PM_EUNSUPPORTED, "resample_tables: %d x %d -> %d x %d needs %d taps per output position, more than PM_RESAMPLE_MAX_TAPS = %d", g->h_in, g->w_in, g->h,
             g->w, need, MAXT);
  nearest_axis(g->h_in, g->h, g->pad_h, g->y1, th, near_rows);
  nearest_axis(g->w_in, g->w, g->pad_w, g->x1, tw, near_cols);
  return PM_OK;
}

extern "C" int pm_resample_crop_u8(const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo, int32_t struct_size, const int32_t* bic_rows,
                                   const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw, int ignore_index, uint8_t* out_img,
                                   uint8_t* out_lab, void* stream) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_geo_image), PM_EINVAL, "resample_crop_u8: pm_geo_image struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)",
             struct_size, sizeof(pm_geo_image), PM_ABI_VERSION);
  PM_REQUIRE(img && lab && geo && bic_rows && bic_cols && near_rows && near_cols && out_img && out_lab, PM_EINVAL, "resample_crop_u8: null pointer");
  PM_REQUIRE(n >= 0 && Hs > 0 && Ws > 0 && th > 0 && tw > 0 && ignore_index >= 0 && ignore_index <= 255, PM_EINVAL,
             "resample_crop_u8: bad args (n %d, slab %d x %d, crop %d x %d, ignore_index %d)", n, Hs, Ws, th, tw, ignore_index);
  PM_REQUIRE(n <= 65535 && pm_cdiv(th, TH) <= 65535, PM_EUNSUPPORTED, "resample_crop_u8: n %d / crop height %d beyond the launch grid", n, th);
  const size_t in_px = (size_t)n * Hs * Ws, out_px = (size_t)n * th * tw;
  auto overlap = [](const uint8_t* a, size_t na, const uint8_t* b, size_t nb) { return a < b + nb && b < a + na; };
  PM_REQUIRE(n == 0 || !(overlap(out_img, out_px * 3, img, in_px * 3) || overlap(out_img, out_px * 3, lab, in_px) || overlap(out_lab, out_px, img, in_px * 3) ||
                         overlap(out_lab, out_px, lab, in_px) || overlap(out_img, out_px * 3, out_lab, out_px)),
             PM_EINVAL, "resample_crop_u8: an output overlaps an input (or the other output): a tile would read resampled pixels");
  if (n == 0) return PM_OK;
  hipLaunchKernelGGL(resample_crop_kernel, dim3(pm_cdiv(tw, TW), pm_cdiv(th, TH), n), dim3(NT), LDS_BYTES, (hipStream_t)stream, img, lab, Hs, Ws, geo, bic_rows, bic_cols,
                     near_rows, near_cols, th, tw, ignore_index, out_img, out_lab);
  return pm_check_launch("resample_crop_u8");
}
