// Winograd F(m x m, 3x3) transforms, m = 2 or 4, for the stride-1 "same" 3x3 convolutions (pad == dilation) of the trunk / ASPP /
// decoder.
//
//   Y = At [ (G g Gt) .* (Bt d B) ] A          (Lavin & Gray; correlation form, fp32 throughout; points 0, +-1 (, +-2), inf)
//
// The element-wise product over channels is P = (m+2)^2 independent GEMMs [tiles x Cin] x [Cin x Cout], which run on the
// implicit-GEMM kernel of conv_igemm.hip as a batched 1x1 convolution (blockIdx.y = transform point): 16 multiplies per 2x2 output
// tile (2.25x fewer MFMA FLOPs than the direct algorithm) or 36 per 4x4 tile (4x fewer).  The transforms here are HBM streaming
// kernels:
//   input   x  [N,H,W,C]        -> V [P][tiles][Kp]   (Kp = C rounded up to 32 so that the GEMM's K-state stays wave-uniform)
//   filter  w  [Cout,3,3,Cin]   -> U [P][Cout][Kp]    (or the 180-degree-rotated, channel-transposed filter for the data gradient;
//                                                      staged through LDS; wino_filter_multi_kernel: every kept forward filter in one launch)
//   output  M  [P][tiles][Cout] -> y [N,H,W,Cout]     (+ the fused epilogue: bias / affine / residual / ReLU)
//   weight gradient: Z = A dY At [P][tiles][Cout];  dU[p] = Z[p]^T V[p] (batched wgrad GEMM, split-K slabs);  dw = Gt (sum dU) G
// and, as an opt-in for F(4x4), wino_fused_f4_kernel: the 36 point GEMMs and the output transform in one kernel.
// A dilated convolution (d > 1) is d*d independent undilated convolutions on the sub-lattices (y % d, x % d); the tile index
// enumerates (image, sub-lattice, tile row, tile column) and the transforms address pixels as  r + d * (m t + a + off)  (wino_pixel).
//
// Every transform is the same two passes, written once (wino_sandwich); a kernel is its load and its store. The (tile, channel
// group) walk (wino_walk), the output tile with its epilogue (wino_output_tile, WinoEpilogue: the two-pass output kernel and the fused
// kernel's tail) and the host's dispatch on m (wino_for_m) are written once as well.
#include "pm_common.h"

#include <type_traits>

namespace {

// ---- transform matrices as compile-time functions (every use is fully unrolled, so zero coefficients vanish) ---------------------
enum { W_BT = 0, W_AT = 1, W_G = 2, W_A = 3, W_GT = 4 };   // W_A = At^T, W_GT = G^T

template <int MT>
__host__ __device__ constexpr float wino_bt(int i, int j) {
  if (MT == 2) {
    constexpr float t[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
    return t[i & 3][j & 3];
  }
  constexpr float t[6][6] = {{4, 0, -5, 0, 1, 0}, {0, -4, -4, 1, 1, 0}, {0, 4, -4, -1, 1, 0}, {0, -2, -1, 2, 1, 0}, {0, 2, -1, -2, 1, 0}, {0, 4, 0, -5, 0, 1}};
  return t[i][j];
}
template <int MT>
__host__ __device__ constexpr float wino_at(int i, int j) {
  if (MT == 2) {
    constexpr float t[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
    return t[i & 1][j & 3];
  }
  constexpr float t[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};
  return t[i][j];
}
template <int MT>
__host__ __device__ constexpr float wino_g(int i, int j) {
  if (MT == 2) {
    constexpr float t[4][3] = {{1, 0, 0}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0, 0, 1}};
    return t[i & 3][j];
  }
  constexpr float t[6][3] = {{1.f / 4, 0, 0},          {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                             {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6},  {0, 0, 1}};
  return t[i][j];
}
template <int MT, int WHICH>
__host__ __device__ constexpr float wino_coef(int r, int c) {
  return WHICH == W_BT ? wino_bt<MT>(r, c) : WHICH == W_AT ? wino_at<MT>(r, c) : WHICH == W_G ? wino_g<MT>(r, c) : WHICH == W_A ? wino_at<MT>(c, r) : wino_g<MT>(c, r);
}

template <int W>
struct Vec {
  float v[W];
};
template <int W>
__device__ __forceinline__ Vec<W> vzero() {
  Vec<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.v[i] = 0.f;
  return r;
}
template <int W>
__device__ __forceinline__ Vec<W> vload(const float* p) {
  Vec<W> r;
  if constexpr (W == 4) {
    const float4 q = PM_LD4(p);
    r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
  } else if constexpr (W == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    r.v[0] = q.x, r.v[1] = q.y;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int W>
__device__ __forceinline__ void vstore(float* p, const Vec<W>& r) {
  if constexpr (W == 4) PM_ST4(p, make_float4(r.v[0], r.v[1], r.v[2], r.v[3]));
  else if constexpr (W == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  else *p = r.v[0];
}

// out[r] = sum_c coef(r, c) * in[c], r < R, c < C: constants folded, +-1 become adds, zeros disappear
template <int MT, int WHICH, int R, int C, int W>
__device__ __forceinline__ void mat_apply(const Vec<W> (&in)[C], Vec<W> (&out)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    Vec<W> acc = vzero<W>();
    bool first = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float k = wino_coef<MT, WHICH>(r, c);
      if (k == 0.f) continue;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        if (first) acc.v[i] = k == 1.f ? in[c].v[i] : (k == -1.f ? -in[c].v[i] : k * in[c].v[i]);
        else if (k == 1.f) acc.v[i] += in[c].v[i];
        else if (k == -1.f) acc.v[i] -= in[c].v[i];
        else acc.v[i] = fmaf(k, in[c].v[i], acc.v[i]);
      }
      first = false;
    }
    out[r] = acc;
  }
}

// The two-pass body of every transform, out = T in T^t for an RI x RI patch and the RO x RI matrix T = WHICH: the column pass over load(a, b) into a
// temporary, then the row pass into store(a, b, v). What a transform reads and writes is its load and its store, each in one place.
template <int MT, int WHICH, int RI, int RO, int W, class Load, class Store>
__device__ __forceinline__ void wino_sandwich(Load load, Store store) {
  Vec<W> t[RO][RI];
#pragma unroll
  for (int b = 0; b < RI; ++b) {   // T in, one patch column at a time
    Vec<W> col[RI], o[RO];
#pragma unroll
    for (int a = 0; a < RI; ++a) col[a] = load(a, b);
    mat_apply<MT, WHICH>(col, o);
#pragma unroll
    for (int a = 0; a < RO; ++a) t[a][b] = o[a];
  }
#pragma unroll
  for (int a = 0; a < RO; ++a) {   // (T in) T^t
    Vec<W> o[RO];
    mat_apply<MT, WHICH>(t[a], o);
#pragma unroll
    for (int b = 0; b < RO; ++b) store(a, b, o[b]);
  }
}

struct TileId {
  int n, ry, rx, ty, tx;
};
__device__ __forceinline__ TileId decode_tile(unsigned tile, const pm_wino_geom& g) {
  TileId t;
  t.tx = (int)(tile % (unsigned)g.TX);
  unsigned q = tile / (unsigned)g.TX;
  t.ty = (int)(q % (unsigned)g.TY);
  q /= (unsigned)g.TY;
  t.rx = (int)(q % (unsigned)g.d);
  q /= (unsigned)g.d;
  t.ry = (int)(q % (unsigned)g.d);
  t.n = (int)(q / (unsigned)g.d);
  return t;
}
// element (a, b) of tile t's patch on its sub-lattice: the pixel index r + d * (m t + a + off) per axis (off = -1: the input patch with its halo, 0: the
// m x m output tile) and whether it lies in the image
template <int MT>
__device__ __forceinline__ bool wino_pixel(const pm_wino_geom& g, const TileId& t, int a, int b, int off, long& pix) {
  const int yy = t.ry + g.d * (MT * t.ty + a + off), xx = t.rx + g.d * (MT * t.tx + b + off);
  pix = (long)(t.n * g.H + yy) * g.W + xx;
  return (unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
}
// grid-stride walk, thread -> (tile, W of `ch` channels); W = 4 floats for m = 2, 2 floats for m = 4 (36 live values per lane): body(tile, c)
template <int W, class Body>
__device__ __forceinline__ void wino_walk(const pm_wino_geom& g, int ch, Body body) {
  const unsigned cg = ch / W;
  const unsigned total = (unsigned)g.tiles * cg;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned tile = i / cg;
    body(tile, (int)(i - tile * cg) * W);
  }
}

template <int MT, int W>
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, long xp, int C, int Kp, const pm_wino_geom g, float* __restrict__ V) {
  constexpr int A = MT + 2;
  const long plane = g.tiles * (long)Kp;
  wino_walk<W>(g, Kp, [&](unsigned tile, int c) {
    const TileId t = decode_tile(tile, g);
    float* out = V + (long)tile * Kp + c;
    wino_sandwich<MT, W_BT, A, A, W>(   // Bt d B; the K padding and the halo outside the image read as 0
        [&](int a, int b) {
          long pix;
          return (wino_pixel<MT>(g, t, a, b, -1, pix) && c < C) ? vload<W>(x + pix * xp + c) : vzero<W>();
        },
        [&](int a, int b, const Vec<W>& v) { vstore<W>(out + (a * A + b) * plane, v); });
  });
}

// The fused epilogue of the output transform: y = relu((v + bias) * scale + shift + residual), every part optional. The per-channel vectors are loaded once per
// (tile, channel group); residual and ReLU are applied per pixel.
struct WinoEpilogueArgs {
  const float* bias;
  const float* scale;
  const float* shift;
  const float* residual;
  long rp;
  int relu;
};
template <int W>
struct WinoEpilogue {
  const WinoEpilogueArgs& e;
  const int c;
  Vec<W> bi = vzero<W>(), sc = vzero<W>(), sh = vzero<W>();
  __device__ __forceinline__ WinoEpilogue(const WinoEpilogueArgs& e_, int c_) : e(e_), c(c_) {
    if (e.bias) bi = vload<W>(e.bias + c);
    if (e.scale) sc = vload<W>(e.scale + c), sh = vload<W>(e.shift + c);
  }
  __device__ __forceinline__ Vec<W> operator()(Vec<W> v, long pix) const {
    if (e.bias) {
#pragma unroll
      for (int q = 0; q < W; ++q) v.v[q] += bi.v[q];
    }
    if (e.scale) {
#pragma unroll
      for (int q = 0; q < W; ++q) v.v[q] = v.v[q] * sc.v[q] + sh.v[q];
    }
    if (e.residual) {
      const Vec<W> rr = vload<W>(e.residual + pix * e.rp + c);
#pragma unroll
      for (int q = 0; q < W; ++q) v.v[q] += rr.v[q];
    }
    if (e.relu) {
#pragma unroll
      for (int q = 0; q < W; ++q) v.v[q] = fmaxf(v.v[q], 0.f);
    }
    return v;
  }
};
// y = At m A + the epilogue for W channels (from c) of one tile, m read through load(a, b); output pixels beyond H / W are skipped
template <int MT, int W, class Load>
__device__ __forceinline__ void wino_output_tile(Load load, const pm_wino_geom& g, const TileId& t, int c, float* __restrict__ y, long yp, const WinoEpilogueArgs& e) {
  const WinoEpilogue<W> ep(e, c);
  wino_sandwich<MT, W_AT, MT + 2, MT, W>(load, [&](int a, int b, const Vec<W>& v) {
    long pix;
    if (wino_pixel<MT>(g, t, a, b, 0, pix)) vstore<W>(y + pix * yp + c, ep(v, pix));
  });
}

template <int MT, int W>
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ M, int Cout, const pm_wino_geom g, float* __restrict__ y, long yp, const WinoEpilogueArgs e) {
  constexpr int A = MT + 2;
  const long plane = g.tiles * (long)Cout;
  wino_walk<W>(g, Cout, [&](unsigned tile, int c) {
    const float* in = M + (long)tile * Cout + c;
    wino_output_tile<MT, W>([&](int a, int b) { return vload<W>(in + (a * A + b) * plane); }, g, decode_tile(tile, g), c, y, yp, e);
  });
}

// U = G g Gt for a 32 (rows of the GEMM's B) x 32 (its K) block of filters, staged through LDS so that both the KRSC read and the
// [P][rows][Kp] write are coalesced for either orientation:
//   forward   rows = Cout, k = Cin,  g(ky,kx) = w[row][ky][kx][k]
//   data grad rows = Cin,  k = Cout, g(ky,kx) = w[k][2-ky][2-kx][row]      (180-degree rotation, channels transposed)
template <int MT, bool DGRAD>
__device__ __forceinline__ void wino_filter_block(const float* __restrict__ w, int Cout, int Cin, int Kp, float* __restrict__ U, int bx, int by,
                                                  float (*sg)[32][33]) {   // sg: [tap][co_local][ci_local]
  constexpr int A = MT + 2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int R = DGRAD ? Cin : Cout;      // GEMM rows
  const int Kr = DGRAD ? Cout : Cin;     // real K extent (zero-filled up to Kp)
  const int r0 = by * 32, k0 = bx * 32;
  const int co0 = DGRAD ? k0 : r0, ci0 = DGRAD ? r0 : k0;
  for (int j = ty; j < 32; j += 8) {   // coalesced over ci
    const int co = co0 + j, ci = ci0 + tx;
    const bool ok = co < Cout && ci < Cin;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) sg[tap][j][tx] = ok ? w[((long)co * 9 + tap) * Cin + ci] : 0.f;
  }
  __syncthreads();
  const long plane = (long)R * Kp;
  // thread -> (row r0 + j, four consecutive k = k0 + 4 q): one float4 store per transform point (36 x 16 B instead of 144 x 4 B per thread)
  const int j = threadIdx.x >> 3, q = threadIdx.x & 7;
  const int row = r0 + j, k = k0 + 4 * q;
  if (row >= R || k >= Kp) return;
  float* out = U + (long)row * Kp + k;
  wino_sandwich<MT, W_G, 3, A, 4>(   // G g Gt
      [&](int ky, int kx) {
        Vec<4> v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = DGRAD ? sg[(2 - ky) * 3 + (2 - kx)][4 * q + e][j] : sg[ky * 3 + kx][j][4 * q + e];
        return v;
      },
      [&](int a, int b, Vec<4> v) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e >= Kr) v.v[e] = 0.f;   // zero fill of the K padding
        vstore<4>(out + (a * A + b) * plane, v);
      });
}
template <int MT, bool DGRAD>
__global__ __launch_bounds__(256) void wino_filter_kernel(const float* __restrict__ w, int Cout, int Cin, int Kp, float* __restrict__ U) {
  __shared__ float sg[9][32][33];
  wino_filter_block<MT, DGRAD>(w, Cout, Cin, Kp, U, blockIdx.x, blockIdx.y, sg);
}

// Every kept forward transform of a model rewritten in ONE launch (pm_conv_wxf_refresh_f32, called behind the optimizer step): the 17-21 per-layer launches of
// wino_filter_kernel in front of the next forward pass are 4 ... 512 blocks each and mostly pure launch latency (17 us on average, 0.36 ms per step).
// Same block body, same values; block -> (job, tile) through a start table carried in the kernel arguments.
constexpr int WR_BATCH = 48;
struct WinoRefreshJobs {
  const float* w[WR_BATCH];
  float* U[WR_BATCH];
  int cout[WR_BATCH], cin[WR_BATCH], kp[WR_BATCH], m[WR_BATCH];
  int start[WR_BATCH + 1];
  int n;
};
__global__ __launch_bounds__(256) void wino_filter_multi_kernel(const WinoRefreshJobs t) {
  __shared__ float sg[9][32][33];
  int j = 0;
  while (j + 1 < t.n && (int)blockIdx.x >= t.start[j + 1]) ++j;      // <= 48 jobs: a scalar walk
  const int local = (int)blockIdx.x - t.start[j];
  const int nbx = t.kp[j] / 32;
  const int bx = local % nbx, by = local / nbx;
  if (t.m[j] == 4) wino_filter_block<4, false>(t.w[j], t.cout[j], t.cin[j], t.kp[j], t.U[j], bx, by, sg);
  else wino_filter_block<2, false>(t.w[j], t.cout[j], t.cin[j], t.kp[j], t.U[j], bx, by, sg);
}

// Weight gradient, step 1: Z = A dY At -- the m x m output-gradient tile scattered to the P transform points (pixels outside the
// image contribute 0).  dU[p][co][ci] = sum_tiles Z[p][tile][co] * V[p][tile][ci] is then a batched wgrad GEMM.
template <int MT, int W>
__global__ __launch_bounds__(256) void wino_dy_kernel(const float* __restrict__ dy, long yp, int Cout, const pm_wino_geom g, float* __restrict__ Z) {
  constexpr int A = MT + 2;
  const long plane = g.tiles * (long)Cout;
  wino_walk<W>(g, Cout, [&](unsigned tile, int c) {
    const TileId t = decode_tile(tile, g);
    float* out = Z + (long)tile * Cout + c;
    wino_sandwich<MT, W_A, MT, A, W>(   // A dY At
        [&](int a, int b) {
          long pix;
          return wino_pixel<MT>(g, t, a, b, 0, pix) ? vload<W>(dy + pix * yp + c) : vzero<W>();
        },
        [&](int a, int b, const Vec<W>& v) { vstore<W>(out + (a * A + b) * plane, v); });
  });
}

// Weight gradient, step 3: fixed-order sum of the split-K slabs [ks][P][Cout][Kp] and dw = Gt dU G -> KRSC [Cout][3][3][Cin].
template <int MT>
__global__ __launch_bounds__(256) void wino_dw_kernel(const float* __restrict__ slab, int ks, int Cout, int Cin, int Kp, float* __restrict__ dw) {
  constexpr int A = MT + 2, P = A * A;
  const long total = (long)Cout * Cin, plane = (long)Cout * Kp;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int co = (int)(i / Cin), ci = (int)(i - (long)co * Cin);
    const float* in = slab + (long)co * Kp + ci;
    // slab sum with z outermost: the P loads of one slab are independent and all in flight together (the per-element order of the
    // additions over z is unchanged, so the result is bit-identical to a z-innermost loop)
    float du[P];
#pragma unroll
    for (int q = 0; q < P; ++q) du[q] = 0.f;
    for (int z = 0; z < ks; ++z) {
      float ld[P];
#pragma unroll
      for (int q = 0; q < P; ++q) ld[q] = in[((long)z * P + q) * plane];
#pragma unroll
      for (int q = 0; q < P; ++q) du[q] += ld[q];
    }
    float* out = dw + (long)co * 9 * Cin + ci;
    wino_sandwich<MT, W_GT, A, 3, 1>(   // Gt dU G
        [&](int a, int b) { return Vec<1>{{du[a * A + b]}}; }, [&](int k, int l, const Vec<1>& v) { out[(k * 3 + l) * (long)Cin] = v.v[0]; });
  }
}

// ---- F(4x4,3x3): the 36 point GEMMs AND the output transform in one kernel -- M = V U^T never reaches HBM ------------------------------
// One block = 32 transform tiles x 32 output channels x ALL 36 points: 12 waves, wave w owns points 3w .. 3w + 2, one 32 x 32 MFMA tile
// (v_mfma_f32_32x32x2_f32, exact fp32 chain) per point = 48 accumulator registers per lane. K (input channels) runs outermost in slabs of 16:
// per slab the block stages 36 x (32 tile rows of V + 32 channel rows of U) x 64 B = 144 KB in LDS (16-byte chunks XOR-swizzled by (row >> 2) & 3:
// conflict-free ds_read_b128 without padding), next slab's rows prefetched to registers under the MFMAs. After the K loop the accumulators are
// parked in the same LDS as M[36][32][32 (+1)] and every (tile, channel) pair applies y = At M A + the fused epilogue (wino_output_tile, the body
// of wino_output_kernel at one channel per thread), stores leave as 128-byte channel runs. Against GEMM + wino_output_kernel this removes the write
// and the read of M (2.25 x the output each) and one launch; the price is U / V re-read from L2 (Cout / 32 and tiles / 32 times).
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WinoFusedArgs {
  const float* V;      // [36][tiles][Kp]
  const float* U;      // [36][Cout][Kp]
  float* y;
  long yp;
  int Cout, Kp;
  pm_wino_geom g;
  WinoEpilogueArgs ep;
  int ncb;            // channel blocks (Cout / 32, rounded up); gridDim.x = tile blocks * ncb
};

constexpr int WF_THREADS = 768, WF_TB = 32, WF_CB = 32, WF_BK = 16, WF_P = 36;
constexpr size_t WF_LDS = (size_t)WF_P * WF_TB * (WF_CB + 1) * sizeof(float);   // the parked accumulators (152 064 B) >= the operand stage (147 456 B)

__global__ __launch_bounds__(WF_THREADS) void wino_fused_f4_kernel(const WinoFusedArgs a) {
  extern __shared__ __align__(16) float4 lds4[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lid = pm_xcd_remap(blockIdx.x, gridDim.x);
  const int tb = lid / a.ncb, cb = lid - tb * a.ncb;
  const long tile0 = (long)tb * WF_TB;
  const int co0 = cb * WF_CB;

  // ---- loader: thread -> one 16-byte chunk of one row, the same (row, chunk) for the points pgrp, pgrp + 3, ... (12 per thread) ----------------
  const int rem = tid & 255, row = rem >> 2, chunk = rem & 3, pgrp = tid >> 8;
  const bool is_a = row < WF_TB;
  bool valid;
  const float* gp;
  long plane;
  if (is_a) {
    const long tile = tile0 + row;
    valid = tile < a.g.tiles;
    gp = a.V + (valid ? tile : 0) * a.Kp + chunk * 4;
    plane = a.g.tiles * (long)a.Kp;
  } else {
    const int co = co0 + row - WF_TB;
    valid = co < a.Cout;
    gp = a.U + (long)(valid ? co : 0) * a.Kp + chunk * 4;
    plane = (long)a.Cout * a.Kp;
  }
  gp += (long)pgrp * plane;
  const long pstep = 3 * plane;
  const int ldsw = pgrp * 256 + row * 4 + (chunk ^ ((row >> 2) & 3));
  float4 r[12];
  auto gload = [&](int k0) {
#pragma unroll
    for (int it = 0; it < 12; ++it) r[it] = valid ? PM_LD4(gp + it * pstep + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto lstore = [&]() {
#pragma unroll
    for (int it = 0; it < 12; ++it) lds4[it * 768 + ldsw] = r[it];
  };

  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
  const int l31 = lane & 31, half = lane >> 5;
  // fragment rows: A row l31, B row 32 + l31; this lane-half's 8 k are chunks 2 half, 2 half + 1 of the row (swizzled)
  const int sa = (l31 >> 2) & 3, sb = ((32 + l31) >> 2) & 3;
  const int ia0 = l31 * 4 + ((2 * half) ^ sa), ia1 = l31 * 4 + ((2 * half + 1) ^ sa);
  const int ib0 = (32 + l31) * 4 + ((2 * half) ^ sb), ib1 = (32 + l31) * 4 + ((2 * half + 1) ^ sb);
  auto compute = [&]() {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4* T = lds4 + (wave * 3 + j) * 256;
      const float4 a0 = T[ia0], a1 = T[ia1], b0 = T[ib0], b1 = T[ib1];
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc[j], 0, 0, 0);
    }
  };

  const int nk = a.Kp / WF_BK;
  gload(0);
  lstore();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) gload((kt + 1) * WF_BK);      // in flight under the 24 MFMAs of this slab
    compute();
    __syncthreads();                                // every wave is done reading the stage
    if (kt + 1 < nk) {
      lstore();
      __syncthreads();
    }
  }

  // ---- epilogue: park the 36 products of every (tile, channel) pair in LDS, then y = At M A per pair -----------------------------------------
  float* Ms = reinterpret_cast<float*>(lds4);       // [36][32 tiles][33]
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int pnt = wave * 3 + j;
#pragma unroll
    for (int q = 0; q < 16; ++q) Ms[(pnt * WF_TB + (q & 3) + 8 * (q >> 2) + 4 * half) * (WF_CB + 1) + l31] = acc[j][q];
  }
  __syncthreads();
  for (int idx = tid; idx < WF_TB * WF_CB; idx += WF_THREADS) {
    const int t = idx >> 5, c = idx & 31;
    const long tile = tile0 + t;
    const int co = co0 + c;
    if (tile >= a.g.tiles || co >= a.Cout) continue;
    wino_output_tile<4, 1>([&](int aa, int b) { return vload<1>(Ms + ((aa * 6 + b) * WF_TB + t) * (WF_CB + 1) + c); }, a.g, decode_tile((unsigned)tile, a.g), co, a.y,
                           a.yp, a.ep);
  }
}

inline unsigned nblocks(long total) { return (unsigned)std::min<long>((total + 255) / 256, 1 << 20); }

// f(MT, W) as compile-time constants for a run-time m: F(4x4) with 2 channels per thread, F(2x2) with 4
template <class F>
inline void wino_for_m(int m, F f) {
  if (m == 4) f(std::integral_constant<int, 4>(), std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 2>(), std::integral_constant<int, 4>());
}

}  // namespace

pm_wino_geom pm_wino_make_geom(int n, int h, int w, int d, int m) {
  pm_wino_geom g;
  g.N = n, g.H = h, g.W = w, g.d = d, g.m = m;
  g.TY = (pm_cdiv(h, d) + m - 1) / m, g.TX = (pm_cdiv(w, d) + m - 1) / m;
  g.tiles = (long)n * d * d * g.TY * g.TX;
  return g;
}

int pm_wino_input_xf(const float* x, long pitch, int C, int Kp, const pm_wino_geom& g, float* V, hipStream_t st) {
  wino_for_m(g.m, [&](auto mt, auto cw) {
    constexpr int MT = mt, W = cw;
    hipLaunchKernelGGL((wino_input_kernel<MT, W>), dim3(nblocks(g.tiles * (Kp / W))), dim3(256), 0, st, x, pitch, C, Kp, g, V);
  });
  return pm_check_launch("wino_input");
}

int pm_wino_filter_xf(const float* w, int Cout, int Cin, int Kp, bool dgrad, int m, float* U, hipStream_t st) {
  const int R = dgrad ? Cin : Cout;
  dim3 grid(Kp / 32, pm_cdiv(R, 32));
  wino_for_m(m, [&](auto mt, auto) {
    constexpr int MT = mt;
    if (dgrad) hipLaunchKernelGGL((wino_filter_kernel<MT, true>), grid, dim3(256), 0, st, w, Cout, Cin, Kp, U);
    else hipLaunchKernelGGL((wino_filter_kernel<MT, false>), grid, dim3(256), 0, st, w, Cout, Cin, Kp, U);
  });
  return pm_check_launch("wino_filter");
}

// jobs: forward transforms only (w [Cout][3][3][Cin], U [P][Cout][Kp], m in {2, 4}); batches of WR_BATCH per launch
int pm_wino_filter_xf_multi(const float* const* w, float* const* U, const int* cout, const int* cin, const int* kp, const int* m, int n, hipStream_t st) {
  for (int i0 = 0; i0 < n; i0 += WR_BATCH) {
    WinoRefreshJobs t;
    t.n = std::min(WR_BATCH, n - i0);
    long blocks = 0;
    for (int i = 0; i < t.n; ++i) {
      t.w[i] = w[i0 + i], t.U[i] = U[i0 + i], t.cout[i] = cout[i0 + i], t.cin[i] = cin[i0 + i], t.kp[i] = kp[i0 + i], t.m[i] = m[i0 + i];
      t.start[i] = (int)blocks;
      blocks += (long)(kp[i0 + i] / 32) * pm_cdiv(cout[i0 + i], 32);
    }
    t.start[t.n] = (int)blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(wino_filter_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, t);
    if (int e = pm_check_launch("wino_filter_multi")) return e;
  }
  return PM_OK;
}

int pm_wino_output_xf(const float* M, int Cout, const pm_wino_geom& g, float* y, long ypitch, const float* bias, const float* scale, const float* shift,
                      const float* residual, long res_pitch, int relu, hipStream_t st) {
  const WinoEpilogueArgs e = {bias, scale, shift, residual, res_pitch, relu};
  wino_for_m(g.m, [&](auto mt, auto cw) {
    constexpr int MT = mt, W = cw;
    hipLaunchKernelGGL((wino_output_kernel<MT, W>), dim3(nblocks(g.tiles * (Cout / W))), dim3(256), 0, st, M, Cout, g, y, ypitch, e);
  });
  return pm_check_launch("wino_output");
}

int pm_wino_dy_xf(const float* dy, long pitch, int Cout, const pm_wino_geom& g, float* Z, hipStream_t st) {
  wino_for_m(g.m, [&](auto mt, auto cw) {
    constexpr int MT = mt, W = cw;
    hipLaunchKernelGGL((wino_dy_kernel<MT, W>), dim3(nblocks(g.tiles * (Cout / W))), dim3(256), 0, st, dy, pitch, Cout, g, Z);
  });
  return pm_check_launch("wino_dy");
}

int pm_wino_dw_xf(const float* slab, int ks, int Cout, int Cin, int Kp, int m, float* dw, hipStream_t st) {
  const unsigned nb = (unsigned)std::min<long>(((long)Cout * Cin + 255) / 256, 1 << 16);
  wino_for_m(m, [&](auto mt, auto) {
    constexpr int MT = mt;
    hipLaunchKernelGGL(wino_dw_kernel<MT>, dim3(nb), dim3(256), 0, st, slab, ks, Cout, Cin, Kp, dw);
  });
  return pm_check_launch("wino_dw");
}

// GEMMs + output transform in one kernel (F(4x4) only): V [36][tiles][Kp] x U [36][Cout][Kp] -> y with the fused epilogue.
int pm_wino_fused_f4(const float* V, const float* U, int Cout, int Kp, const pm_wino_geom& g, float* y, long ypitch, const float* bias, const float* scale,
                     const float* shift, const float* residual, long res_pitch, int relu, hipStream_t st) {
  static pm_lds_optin optin;
  (void)optin(reinterpret_cast<const void*>(&wino_fused_f4_kernel), (int)WF_LDS);
  WinoFusedArgs a;
  a.V = V, a.U = U, a.y = y, a.yp = ypitch, a.Cout = Cout, a.Kp = Kp, a.g = g;
  a.ep = {bias, scale, shift, residual, res_pitch, relu};
  a.ncb = (Cout + WF_CB - 1) / WF_CB;
  const long ntb = (g.tiles + WF_TB - 1) / WF_TB;
  hipLaunchKernelGGL(wino_fused_f4_kernel, dim3((unsigned)(ntb * a.ncb)), dim3(WF_THREADS), WF_LDS, st, a);
  return pm_check_launch("wino_fused_f4");
}

