// Resampling input edge: RandomSizeAndCrop's antialiased bicubic resize (image) and nearest resize (mask), pad and crop, for the crop window alone, with PIL's
// bytes (include/pinmem_hip.h, pm_resample_crop_u8). The host writes PIL's coefficient tables for the window (pm_resample_tables: double arithmetic, fixed point
// 2^22); one kernel stages a tile's source footprint in LDS, filters it along W into bytes in a second LDS buffer, filters those along H and gathers the labels.
// The evaluation edge (pm_eval_tiles_u8) runs the same passes with the tables of Image.resize(BILINEAR) over the whole scaled image (pm_resize_axis_tables) and
// stores a piece of a sliding window, mirrored or not, as normalised float4 pixels: neither the scaled image nor its mirror exists in memory.
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
constexpr int EVAL_LDS_BYTES = LDS_BYTES + TH * ROWB;                   // 64 256 with the tile's bytes in front of their conversion: still two blocks per CU

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

// Source columns [fx0, fx0 + fw) the tile's columns with taps read (every lane computes the same: broadcast reads); staged rows start on a dword.
struct Footprint {
  int fx0, fwb, spb;      // first column, bytes of a footprint row, bytes between staged rows
};
__device__ __forceinline__ Footprint column_footprint(const int* ctab, int w_in) {
  int fx0 = w_in, fx1 = 0;
  for (int x = 0; x < TW; ++x) {
    const int a = ctab[x * REC], c = ctab[x * REC + 1];
    if (c > 0) fx0 = min(fx0, a), fx1 = max(fx1, a + c);
  }
  const int fwb = max(fx1 - fx0, 0) * 3;
  return {fx0, fwb, (fwb + 3) & ~3};
}

// One pass takes as many of the tile's rows as fit: -> yb, rows [ya, yb) read source rows [fy0, fy0 + fh), which `mid` and `stage` hold. fh == 0 where one row alone
// does not fit: not a table of this library (the hosts refuse such a geometry); its pixels come out as the rounding constant, 0.
__device__ __forceinline__ int pass_rows(const int* rtab, int ya, int nr, int h_in, int spb, int& fy0, int& fh) {
  int lo0 = h_in, hi0 = 0, yb = ya;
  for (; yb < nr; ++yb) {
    const int a = rtab[yb * REC], c = rtab[yb * REC + 1];
    const int lo = c > 0 ? min(lo0, a) : lo0, hi = c > 0 ? max(hi0, a + c) : hi0;
    if (yb > ya && (hi - lo > MID_ROWS || (hi - lo) * spb > SRC_BYTES)) break;
    lo0 = lo, hi0 = hi;
  }
  fy0 = lo0, fh = max(hi0 - lo0, 0);
  if (fh > MID_ROWS || fh * spb > SRC_BYTES) fh = 0;
  return yb;
}

// Staging of rows [fy0, fy0 + fh) of the footprint from the image `src` with `pitch` pixels per row: a wave takes rows wave, wave + NW, ...; its lanes the dwords of a
// row (loaded from any byte address), STAGE_U rows in flight; the last 0 .. 3 bytes of a row go one by one, so no byte outside the footprint is read.
__device__ __forceinline__ void stage_rows(uint8_t* stage, const uint8_t* __restrict__ src, int pitch, int fy0, int fh, Footprint f, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  for (int q = lane; q < (f.fwb >> 2); q += 64) {
    for (int r0 = wave; r0 < fh; r0 += NW * STAGE_U) {
      unsigned v[STAGE_U];
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u)
        if (r0 + u * NW < fh) __builtin_memcpy(&v[u], src + ((long)(fy0 + r0 + u * NW) * pitch + f.fx0) * 3 + 4 * q, 4);
#pragma unroll
      for (int u = 0; u < STAGE_U; ++u)
        if (r0 + u * NW < fh) reinterpret_cast<unsigned*>(stage + (r0 + u * NW) * f.spb)[q] = v[u];
    }
  }
  if (lane < (f.fwb & 3))
    for (int r = wave; r < fh; r += NW) stage[r * f.spb + (f.fwb & ~3) + lane] = src[((long)(fy0 + r) * pitch + f.fx0) * 3 + (f.fwb & ~3) + lane];
  __syncthreads();
}

// Along W: one pixel of one staged row per lane, rounded to bytes in `mid`; a pad column (no taps) holds 0, and stays 0 along H.
__device__ __forceinline__ void filter_w(uint8_t* mid, const uint8_t* stage, const int* ctab, int fh, Footprint f, int tid) {
  for (int i = tid; i < fh * TW; i += NT) {
    const int r = i / TW, x = i - r * TW;
    const int* rec = ctab + x * REC;
    const int c = rec[1];
    const uint8_t* p = stage + r * f.spb + (rec[0] - f.fx0) * 3;
    int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < c; ++j) {
      const int k = rec[2 + j];
      s0 += p[3 * j] * k, s1 += p[3 * j + 1] * k, s2 += p[3 * j + 2] * k;
    }
    uint8_t* m = mid + r * ROWB + x * 3;
    m[0] = (uint8_t)clip8(s0 >> PREC), m[1] = (uint8_t)clip8(s1 >> PREC), m[2] = (uint8_t)clip8(s2 >> PREC);
  }
  __syncthreads();
}

// clip8(s >> PREC) with the clamp in front of the shift: the same byte, the shift being monotone. Packing clip8(a >> PREC) | clip8(b >> PREC) << 8 directly makes hipcc
// (ROCm 7.2) select v_ashr_pk_u8_i32 and OR the other bytes over its result; on gfx950 that instruction keeps bits 16 .. 31 of its destination register, which held
// one of the sums (seen as bytes 2 and 3 of every packed dword ORed with bits 16 .. 31 of the second sum).
__device__ __forceinline__ unsigned round8(int s) { return (unsigned)min(max(s, 0), (256 << PREC) - 1) >> PREC; }

// Along H: bytes e .. e + 3 of the output row of record `rec` (`c` of its taps), from the rows of `mid` that start at source row fy0, packed low byte first.
__device__ __forceinline__ unsigned filter_h4(const uint8_t* mid, const int* rec, int c, int fy0, int e) {
  const uint8_t* p = mid + (rec[0] - fy0) * ROWB + e;
  int s[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
  for (int j = 0; j < c; ++j) {
    const unsigned v = *reinterpret_cast<const unsigned*>(p + j * ROWB);
    const int k = rec[2 + j];
    s[0] += (int)(v & 255u) * k, s[1] += (int)((v >> 8) & 255u) * k, s[2] += (int)((v >> 16) & 255u) * k, s[3] += (int)(v >> 24) * k;
  }
  return round8(s[0]) | round8(s[1]) << 8 | round8(s[2]) << 16 | round8(s[3]) << 24;
}

// The decode step of the label-decoding edge (include/pinmem_hip.h, pm_label_table): one label pixel through its image's table, which the block holds in LDS; a null
// table is the pass-through. The probe walk ends at the key, at an empty slot or after PM_LABEL_SLOTS steps, and every index is a byte or masked to the slot count.
constexpr unsigned LABEL_EMPTY = 0xFFFFFFFFu, LABEL_HASH = 0x9E3779B1u;
__host__ __device__ __forceinline__ unsigned label_slot(unsigned key) { return (key * LABEL_HASH) >> 24; }
static_assert(PM_LABEL_SLOTS == 256, "label_slot keeps the top 8 bits of the product");
constexpr int TABLE_WORDS = (int)(sizeof(pm_label_table) / 4);
static_assert(sizeof(pm_label_table) % 4 == 0, "the table is copied to LDS as dwords");

__device__ __forceinline__ uint8_t decode_label(const pm_label_table* T, const uint8_t* p, int lab_c) {
  if (!T) return p[0];
  if (T->mode != PM_LABEL_COLORS) return T->lut[p[0]];
  if (lab_c != 3) return (uint8_t)T->fill;
  const unsigned key = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
  unsigned s = label_slot(key);
  for (int i = 0; i < PM_LABEL_SLOTS; ++i, s = (s + 1) & (PM_LABEL_SLOTS - 1)) {
    const unsigned k = T->keys[s];
    if (k == key) return T->vals[s];
    if (k == LABEL_EMPTY) break;
  }
  return (uint8_t)T->fill;
}

// The table of image n into `dst` (LDS; every thread of the block calls this): null for the pass-through (a negative entry, or no tables at all); the index is clamped.
template <int THREADS>
__device__ __forceinline__ const pm_label_table* load_label_table(unsigned* dst, const pm_label_table* __restrict__ tables, int ntables,
                                                                  const int32_t* __restrict__ image_table, int n, int tid) {
  const int t = image_table[n];
  if (t < 0 || ntables <= 0) return nullptr;      // uniform over the block
  const unsigned* src = reinterpret_cast<const unsigned*>(tables + min(t, ntables - 1));
  for (int i = tid; i < TABLE_WORDS; i += THREADS) dst[i] = src[i];
  __syncthreads();
  return reinterpret_cast<const pm_label_table*>(dst);
}

// DECODE: the mask is [n][Hs][Ws][lab_c] and every gathered pixel goes through its image's pm_label_table; without it the plain gather of pm_resample_crop_u8.
template <bool DECODE>
__global__ __launch_bounds__(NT) void resample_crop_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab, int Hs, int Ws,
                                                            const pm_geo_image* __restrict__ geo, const int32_t* __restrict__ bic_rows,
                                                            const int32_t* __restrict__ bic_cols, const int32_t* __restrict__ near_rows,
                                                            const int32_t* __restrict__ near_cols, int th, int tw, int ignore, int lab_c,
                                                            const pm_label_table* __restrict__ tables, int ntables, const int32_t* __restrict__ image_table,
                                                            uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_lab) {
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

  // labels: a gather through the two nearest tables, with DECODE each pixel through the image's label table (parked in `stage`, which the image passes claim only
  // behind the barriers of load_records)
  {
    const int lc = DECODE ? lab_c : 1;
    const pm_label_table* T = nullptr;
    if constexpr (DECODE) T = load_label_table<NT>(reinterpret_cast<unsigned*>(stage), tables, ntables, image_table, n, tid);
    const uint8_t* src = lab + (long)n * slab * lc;
    const int32_t *ry = near_rows + (long)n * th + y0, *rx = near_cols + (long)n * tw + x0;
    uint8_t* dst = out_lab + ((long)n * th + y0) * tw + x0;
    for (int i = tid; i < nr * TW; i += NT) {
      const int ly = i / TW, lx = i - ly * TW;
      if (lx >= nc) continue;
      const int sy = ry[ly], sx = rx[lx];
      if (sy < 0 || sx < 0) {
        dst[(long)ly * tw + lx] = (uint8_t)ignore;
        continue;
      }
      const uint8_t* p = src + ((long)min(sy, h_in - 1) * Ws + min(sx, w_in - 1)) * lc;
      dst[(long)ly * tw + lx] = DECODE ? decode_label(T, p, lc) : p[0];
    }
  }

  load_records(rtab, bic_rows + (long)n * th * REC, y0, TH, th, h_in, tid);
  load_records(ctab, bic_cols + (long)n * tw * REC, x0, TW, tw, w_in, tid);

  const Footprint f = column_footprint(ctab, w_in);
  const uint8_t* src = img + (long)n * slab * 3;
  uint8_t* dst = out_img + (((long)n * th + y0) * tw + x0) * 3;
  const bool vec = (((long)tw * 3) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_img) & 3) == 0;      // every tile row starts on a dword and ends on one

  // the tile's rows in passes of as many as fit: the source rows of a pass go through `stage` into `mid`
  for (int ya = 0; ya < nr;) {
    int fy0, fh;
    const int yb = pass_rows(rtab, ya, nr, h_in, f.spb, fy0, fh);
    stage_rows(stage, src, Ws, fy0, fh, f, tid);
    filter_w(mid, stage, ctab, fh, f, tid);
    for (int i = tid; i < (yb - ya) * (ROWB / 4); i += NT) {      // along H: four bytes of one output row per lane
      const int ly = ya + i / (ROWB / 4), e = (i % (ROWB / 4)) * 4;
      const int* rec = rtab + ly * REC;
      const unsigned v = filter_h4(mid, rec, fh > 0 ? rec[1] : 0, fy0, e);
      uint8_t* o = dst + (long)ly * tw * 3 + e;
      if (vec) {
        if (e < nc * 3) *reinterpret_cast<unsigned*>(o) = v;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (e + b < nc * 3) o[b] = (uint8_t)(v >> (8 * b));
      }
    }
    __syncthreads();      // `stage` and `mid` are free for the next pass
    ya = yb;
  }
}

// pm_eval_tiles_u8: blocks (x piece, y piece, flip * T + tile). The piece's rows and columns of the SCALED image go through the passes above; a mirrored window
// computes the un-mirrored columns [Ws - x2, Ws - x1) and stores them reversed. The tile's origin is clamped so that the window lies inside the scaled image whatever the
// table holds (the host has checked th <= Hs, tw <= Ws), the records are clamped by load_records, and every store address comes from the block index alone.
__global__ __launch_bounds__(NT) void eval_tiles_kernel(const uint8_t* __restrict__ img, int H, int W, const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                         int Hs, int Ws, const int32_t* __restrict__ tiles, int T, int th, int tw, float m0, float m1, float m2, float s0,
                                                         float s1, float s2, float* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* rtab = reinterpret_cast<int*>(smem);                  // [TH][REC]
  int* ctab = rtab + TH * REC;                               // [TW][REC]
  uint8_t* mid = smem + TAB_BYTES;                           // [MID_ROWS][ROWB]
  uint8_t* stage = mid + MID_ROWS * ROWB;
  uint8_t* px = stage + SRC_BYTES;                           // [TH][ROWB]: the piece's scaled bytes, un-mirrored
  const int t = blockIdx.z % T, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, tid = threadIdx.x;
  const bool mirror = (int)blockIdx.z >= T;
  const int nr = min(TH, th - y0), nc = min(TW, tw - x0);
  const int y1 = min(max(tiles[4 * t + 1], 0), Hs - th) + y0, x1 = min(max(tiles[4 * t], 0), Ws - tw) + x0;      // the piece's origin in the window's own direction
  const int c0 = mirror ? Ws - x1 - nc : x1;                 // first un-mirrored column: x1 + nc <= Ws
  load_records(rtab, rows, y1, TH, y1 + nr, H, tid);
  load_records(ctab, cols, c0, TW, c0 + nc, W, tid);
  const Footprint f = column_footprint(ctab, W);
  for (int ya = 0; ya < nr;) {
    int fy0, fh;
    const int yb = pass_rows(rtab, ya, nr, H, f.spb, fy0, fh);
    stage_rows(stage, img, W, fy0, fh, f, tid);
    filter_w(mid, stage, ctab, fh, f, tid);
    for (int i = tid; i < (yb - ya) * (ROWB / 4); i += NT) {
      const int ly = ya + i / (ROWB / 4), e = (i % (ROWB / 4)) * 4;
      const int* rec = rtab + ly * REC;
      *reinterpret_cast<unsigned*>(px + ly * ROWB + e) = filter_h4(mid, rec, fh > 0 ? rec[1] : 0, fy0, e);
    }
    __syncthreads();
    ya = yb;
  }
  float* dst = out + (((long)blockIdx.z * th + y0) * tw + x0) * 4;
  for (int i = tid; i < nr * TW; i += NT) {                  // one pixel per lane: a wave stores 1 KiB of a row
    const int ly = i / TW, lx = i - ly * TW;
    if (lx < nc) PM_ST4(dst + ((long)ly * tw + lx) * 4, pm_normalise_u8(px + ly * ROWB + (mirror ? nc - 1 - lx : lx) * 3, m0, m1, m2, s0, s1, s2));
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

// PIL's triangle (Resample.c bilinear_filter)
double bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

struct Filter {
  double (*weight)(double);
  double support;
};
// the struct imagingfilter of Resample.c behind a PM_FILTER_* value; null: not one of them
const Filter* filter_of(int filter) {
  static const Filter BILINEAR = {bilinear, 1.0}, BICUBIC = {bicubic, 2.0};
  return filter == PM_FILTER_BILINEAR ? &BILINEAR : filter == PM_FILTER_BICUBIC ? &BICUBIC : nullptr;
}

// precompute_coeffs + normalize_coeffs_8bpc of Resample.c for output positions [p0 - pad, p0 - pad + cnt) of an axis resized from `in` to `out`; false: over the tap cap
bool filter_axis(const Filter& f, int in, int out, int pad, int p0, int cnt, int32_t* rec, int* taps_needed) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale, support = f.support * fs, ss = 1.0 / fs;
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
      w[x] = f.weight((x + xmin - center + 0.5) * ss);
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
  const Filter& f = *filter_of(PM_FILTER_BICUBIC);
  const bool ok = filter_axis(f, g->h_in, g->h, g->pad_h, g->y1, th, bic_rows, &need) && filter_axis(f, g->w_in, g->w, g->pad_w, g->x1, tw, bic_cols, &need);
  PM_REQUIRE(ok, PM_EUNSUPPORTED, "resample_tables: %d x %d -> %d x %d needs %d taps per output position, more than PM_RESAMPLE_MAX_TAPS = %d", g->h_in, g->w_in, g->h,
             g->w, need, MAXT);
  nearest_axis(g->h_in, g->h, g->pad_h, g->y1, th, near_rows);
  nearest_axis(g->w_in, g->w, g->pad_w, g->x1, tw, near_cols);
  return PM_OK;
}

extern "C" int pm_resize_axis_tables(int in, int out, int filter, int32_t* rec) {
  const Filter* f = filter_of(filter);
  PM_REQUIRE(rec && f, PM_EINVAL, "resize_axis_tables: null pointer or unknown filter %d", filter);
  PM_REQUIRE(in > 0 && out > 0, PM_EINVAL, "resize_axis_tables: empty size (%d -> %d)", in, out);
  int need = 0;
  PM_REQUIRE(filter_axis(*f, in, out, 0, 0, out, rec, &need), PM_EUNSUPPORTED,
             "resize_axis_tables: %d -> %d needs %d taps per output position, more than PM_RESAMPLE_MAX_TAPS = %d", in, out, need, MAXT);
  return PM_OK;
}

namespace {
bool overlap(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) { return a < b + nb && b < a + na; }

// the checks and the launch both resampling entry points share; DECODE: lab holds lab_c channels per pixel and goes through the label tables
template <bool DECODE>
int resample_crop(const char* who, const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo, int32_t struct_size, const int32_t* bic_rows,
                  const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw, int ignore_index, int lab_c, const pm_label_table* tables,
                  int ntables, const int32_t* image_table, uint8_t* out_img, uint8_t* out_lab, void* stream) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_geo_image), PM_EINVAL, "%s: pm_geo_image struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)", who,
             struct_size, sizeof(pm_geo_image), PM_ABI_VERSION);
  PM_REQUIRE(img && lab && geo && bic_rows && bic_cols && near_rows && near_cols && out_img && out_lab, PM_EINVAL, "%s: null pointer", who);
  PM_REQUIRE(n >= 0 && Hs > 0 && Ws > 0 && th > 0 && tw > 0 && ignore_index >= 0 && ignore_index <= 255, PM_EINVAL,
             "%s: bad args (n %d, slab %d x %d, crop %d x %d, ignore_index %d)", who, n, Hs, Ws, th, tw, ignore_index);
  PM_REQUIRE(n <= 65535 && pm_cdiv(th, TH) <= 65535, PM_EUNSUPPORTED, "%s: n %d / crop height %d beyond the launch grid", who, n, th);
  const size_t in_px = (size_t)n * Hs * Ws, out_px = (size_t)n * th * tw, lab_b = in_px * lab_c;
  PM_REQUIRE(n == 0 || !(overlap(out_img, out_px * 3, img, in_px * 3) || overlap(out_img, out_px * 3, lab, lab_b) || overlap(out_lab, out_px, img, in_px * 3) ||
                         overlap(out_lab, out_px, lab, lab_b) || overlap(out_img, out_px * 3, out_lab, out_px)),
             PM_EINVAL, "%s: an output overlaps an input (or the other output): a tile would read resampled pixels", who);
  if (n == 0) return PM_OK;
  hipLaunchKernelGGL(resample_crop_kernel<DECODE>, dim3(pm_cdiv(tw, TW), pm_cdiv(th, TH), n), dim3(NT), LDS_BYTES, (hipStream_t)stream, img, lab, Hs, Ws, geo, bic_rows,
                     bic_cols, near_rows, near_cols, th, tw, ignore_index, lab_c, tables, ntables, image_table, out_img, out_lab);
  return pm_check_launch(who);
}

// what both decoding entry points ask of their table arguments
int check_label_tables(const char* who, int lab_c, const pm_label_table* tables, int ntables, int32_t struct_size, const int32_t* image_table) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_label_table), PM_EINVAL, "%s: pm_label_table struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)", who,
             struct_size, sizeof(pm_label_table), PM_ABI_VERSION);
  PM_REQUIRE(lab_c == 1 || lab_c == 3, PM_EINVAL, "%s: label slabs of 1 or 3 channels (got %d)", who, lab_c);
  PM_REQUIRE(ntables >= 0 && (ntables == 0 || tables) && image_table, PM_EINVAL, "%s: %d tables at %p, image_table %p", who, ntables, (const void*)tables,
             (const void*)image_table);
  PM_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 3) == 0 && (reinterpret_cast<uintptr_t>(image_table) & 3) == 0, PM_EINVAL, "%s: tables and image_table must be 4-byte aligned",
             who);
  return PM_OK;
}

// Whole-slab decode: blocks (x, image); a block parks its image's table in LDS and strides over the image's pixels, four to a thread (VEC: dword loads and one dword
// store; else pixel by pixel).
constexpr int DT = 256;
template <bool VEC>
__global__ __launch_bounds__(DT) void labels_decode_kernel(const uint8_t* __restrict__ lab, long hw, int lab_c, const pm_label_table* __restrict__ tables, int ntables,
                                                           const int32_t* __restrict__ image_table, uint8_t* __restrict__ out) {
  __shared__ unsigned tab[TABLE_WORDS];
  const int n = blockIdx.y, tid = threadIdx.x;
  const pm_label_table* T = load_label_table<DT>(tab, tables, ntables, image_table, n, tid);
  const uint8_t* src = lab + (long)n * hw * lab_c;
  uint8_t* dst = out + (long)n * hw;
  const long step = (long)gridDim.x * DT, first = (long)blockIdx.x * DT + tid;
  if constexpr (VEC) {      // hw % 4 == 0 and both bases on a dword: every group of four pixels is whole dwords
    for (long q = first; q < (hw >> 2); q += step) {
      unsigned w[3] = {0u, 0u, 0u};
      for (int j = 0; j < lab_c; ++j) w[j] = reinterpret_cast<const unsigned*>(src)[q * lab_c + j];
      uint8_t px[12];
      __builtin_memcpy(px, w, 12);
      unsigned o = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) o |= (unsigned)decode_label(T, px + e * lab_c, lab_c) << (8 * e);
      reinterpret_cast<unsigned*>(dst)[q] = o;
    }
  } else {
    for (long i = first; i < hw; i += step) dst[i] = decode_label(T, src + i * lab_c, lab_c);
  }
}

// one kept entry into the hash; false: the table is full of other keys
bool label_insert(pm_label_table* t, unsigned key, uint8_t val) {
  unsigned s = label_slot(key);
  for (int i = 0; i < PM_LABEL_SLOTS; ++i, s = (s + 1) & (PM_LABEL_SLOTS - 1)) {
    if (t->keys[s] == LABEL_EMPTY || t->keys[s] == key) {
      t->keys[s] = key, t->vals[s] = val;
      return true;
    }
  }
  return false;
}

void label_table_clear(pm_label_table* t, int mode, int fill) {
  t->mode = mode, t->fill = fill;
  for (int i = 0; i < 256; ++i) t->lut[i] = (uint8_t)i;
  for (int i = 0; i < PM_LABEL_SLOTS; ++i) t->keys[i] = LABEL_EMPTY, t->vals[i] = (uint8_t)fill;
}
}  // namespace

extern "C" int pm_resample_crop_u8(const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo, int32_t struct_size, const int32_t* bic_rows,
                                   const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw, int ignore_index, uint8_t* out_img,
                                   uint8_t* out_lab, void* stream) {
  return resample_crop<false>("resample_crop_u8", img, lab, n, Hs, Ws, geo, struct_size, bic_rows, bic_cols, near_rows, near_cols, th, tw, ignore_index, 1, nullptr, 0,
                              nullptr, out_img, out_lab, stream);
}

extern "C" int pm_resample_crop_decode_u8(const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo, int32_t struct_size,
                                          const int32_t* bic_rows, const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw,
                                          int ignore_index, int lab_c, const pm_label_table* tables, int ntables, int32_t struct_size_table, const int32_t* image_table,
                                          uint8_t* out_img, uint8_t* out_lab, void* stream) {
  if (int rc = check_label_tables("resample_crop_decode_u8", lab_c, tables, ntables, struct_size_table, image_table)) return rc;
  return resample_crop<true>("resample_crop_decode_u8", img, lab, n, Hs, Ws, geo, struct_size, bic_rows, bic_cols, near_rows, near_cols, th, tw, ignore_index, lab_c, tables,
                             ntables, image_table, out_img, out_lab, stream);
}

extern "C" int pm_eval_tiles_u8(const uint8_t* img, int H, int W, const int32_t* rows, const int32_t* cols, int Hs, int Ws, const int32_t* tiles, int ntiles, int th, int tw,
                                int flips, const float* mean3, const float* std3, float* out, void* stream) {
  PM_REQUIRE(img && rows && cols && tiles && mean3 && std3 && out, PM_EINVAL, "eval_tiles_u8: null pointer");
  PM_REQUIRE(H > 0 && W > 0 && Hs > 0 && Ws > 0 && th > 0 && tw > 0 && ntiles >= 0, PM_EINVAL, "eval_tiles_u8: empty size (image %d x %d, scaled %d x %d, %d tiles of %d x %d)", H,
             W, Hs, Ws, ntiles, th, tw);
  PM_REQUIRE(th <= Hs && tw <= Ws, PM_EINVAL, "eval_tiles_u8: tiles of %d x %d in a scaled image of %d x %d", th, tw, Hs, Ws);
  PM_REQUIRE(flips == 1 || flips == 2, PM_EINVAL, "eval_tiles_u8: flips %d (1: the image, 2: and its mirror)", flips);
  PM_REQUIRE(pm_aligned16(out), PM_EINVAL, "eval_tiles_u8: out must be 16-byte aligned");
  PM_REQUIRE(((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(cols) | reinterpret_cast<uintptr_t>(tiles)) & 3) == 0, PM_EINVAL,
             "eval_tiles_u8: the tables must be 4-byte aligned");
  const size_t out_b = (size_t)flips * ntiles * th * tw * 16;
  const uint8_t* o = reinterpret_cast<const uint8_t*>(out);
  PM_REQUIRE(!(overlap(o, out_b, img, (size_t)H * W * 3) || overlap(o, out_b, reinterpret_cast<const uint8_t*>(rows), (size_t)Hs * REC * 4) ||
               overlap(o, out_b, reinterpret_cast<const uint8_t*>(cols), (size_t)Ws * REC * 4) || overlap(o, out_b, reinterpret_cast<const uint8_t*>(tiles), (size_t)ntiles * 16)),
             PM_EINVAL, "eval_tiles_u8: out overlaps the image or a table");
  PM_REQUIRE((long)flips * ntiles <= 65535 && pm_cdiv(th, TH) <= 65535, PM_EUNSUPPORTED, "eval_tiles_u8: %d tiles x %d flips / tile height %d beyond the launch grid", ntiles,
             flips, th);
  // one output row alone must fit the staging buffers: at most MAXT source rows of a piece's columns, which reach over (TW - 1) * W / Ws + MAXT + 2 source pixels at the most
  const long reach = std::min<long>(W, (long)((TW - 1) * ((double)W / Ws)) + MAXT + 2), rows_most = std::min(H, MAXT);
  PM_REQUIRE(rows_most * ((reach * 3 + 3) & ~3l) <= SRC_BYTES, PM_EUNSUPPORTED,
             "eval_tiles_u8: %d -> %d columns: %d source rows of %ld pixels do not fit the %d staged bytes of a %d-column piece", W, Ws, (int)rows_most, reach, SRC_BYTES, TW);
  if (ntiles == 0) return PM_OK;
  hipLaunchKernelGGL(eval_tiles_kernel, dim3(pm_cdiv(tw, TW), pm_cdiv(th, TH), flips * ntiles), dim3(NT), EVAL_LDS_BYTES, (hipStream_t)stream, img, H, W, rows, cols, Hs, Ws,
                     tiles, ntiles, th, tw, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out);
  return pm_check_launch("eval_tiles_u8");
}

extern "C" int pm_labels_decode_u8(const uint8_t* lab, int n, int H, int W, int lab_c, const pm_label_table* tables, int ntables, int32_t struct_size,
                                   const int32_t* image_table, uint8_t* out, void* stream) {
  if (int rc = check_label_tables("labels_decode_u8", lab_c, tables, ntables, struct_size, image_table)) return rc;
  PM_REQUIRE(lab && out, PM_EINVAL, "labels_decode_u8: null pointer");
  PM_REQUIRE(n >= 0 && H > 0 && W > 0, PM_EINVAL, "labels_decode_u8: bad args (n %d, %d x %d)", n, H, W);
  PM_REQUIRE(n <= 65535, PM_EUNSUPPORTED, "labels_decode_u8: n %d beyond the launch grid", n);
  const long hw = (long)H * W;
  PM_REQUIRE(n == 0 || !overlap(out, (size_t)n * hw, lab, (size_t)n * hw * lab_c), PM_EINVAL, "labels_decode_u8: out overlaps lab");
  if (n == 0) return PM_OK;
  const bool vec = (hw & 3) == 0 && ((reinterpret_cast<uintptr_t>(lab) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
  // about 2048 blocks in all (eight per CU), each image's share striding over its pixels: a block's copy of the table is paid once per several thousand pixels
  const dim3 grid((unsigned)std::min<long>(pm_cdiv(vec ? hw >> 2 : hw, DT), pm_cdiv(2048, n)), n);
  if (vec) hipLaunchKernelGGL(labels_decode_kernel<true>, grid, dim3(DT), 0, (hipStream_t)stream, lab, hw, lab_c, tables, ntables, image_table, out);
  else hipLaunchKernelGGL(labels_decode_kernel<false>, grid, dim3(DT), 0, (hipStream_t)stream, lab, hw, lab_c, tables, ntables, image_table, out);
  return pm_check_launch("labels_decode_u8");
}

extern "C" int pm_label_table_ids(const int32_t* keys, const int32_t* vals, int count, pm_label_table* table, int32_t struct_size) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_label_table), PM_EINVAL, "label_table_ids: pm_label_table struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)",
             struct_size, sizeof(pm_label_table), PM_ABI_VERSION);
  PM_REQUIRE(table && count >= 0 && (count == 0 || (keys && vals)), PM_EINVAL, "label_table_ids: null pointer or negative count (%d)", count);
  label_table_clear(table, PM_LABEL_IDS, 255);
  for (int i = 0; i < count; ++i)
    if (keys[i] >= 0 && keys[i] <= 255) table->lut[keys[i]] = (uint8_t)vals[i];      // -1 wraps to 255, as the assignment into a uint8 array does
  return PM_OK;
}

extern "C" int pm_label_table_colors(const int32_t* rgb, const int32_t* vals, int count, int fill, pm_label_table* table, int32_t struct_size) {
  PM_REQUIRE(struct_size == (int32_t)sizeof(pm_label_table), PM_EINVAL,
             "label_table_colors: pm_label_table struct_size %d != %zu (caller built against another pinmem_hip.h; ABI %d)", struct_size, sizeof(pm_label_table), PM_ABI_VERSION);
  PM_REQUIRE(table && count >= 0 && (count == 0 || (rgb && vals)), PM_EINVAL, "label_table_colors: null pointer or negative count (%d)", count);
  PM_REQUIRE(fill >= 0 && fill <= 255, PM_EINVAL, "label_table_colors: fill %d outside 0..255", fill);
  label_table_clear(table, PM_LABEL_COLORS, fill);
  int kept = 0;
  for (int i = 0; i < count; ++i) {
    const int32_t* c = rgb + 3l * i;
    if (vals[i] == 255 || vals[i] == -1) continue;                                                            // gtav.py:444
    if (c[0] < 0 || c[0] > 255 || c[1] < 0 || c[1] > 255 || c[2] < 0 || c[2] > 255) continue;                 // no uint8 pixel equals it
    const unsigned key = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
    bool known = false;
    for (int s = 0; s < PM_LABEL_SLOTS; ++s) known |= table->keys[s] == key;
    PM_REQUIRE(known || kept < PM_LABEL_MAX_COLORS, PM_EUNSUPPORTED, "label_table_colors: more than PM_LABEL_MAX_COLORS = %d colours", PM_LABEL_MAX_COLORS);
    kept += known ? 0 : 1;
    label_insert(table, key, (uint8_t)vals[i]);
  }
  return PM_OK;
}
