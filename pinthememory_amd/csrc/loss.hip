// K6: fused bilinear-upsample(align_corners=True) + CrossEntropy(ignore_index=255, reduction='mean').
// Replaces  Upsample(dec2, x_size) -> criterion  (/root/reference/network/deepv3plus.py:575-578), the aux loss
// (:589-595, same-size case) and the read loss  F.interpolate(score/T) -> celoss  (/root/reference/network/memory.py:173-176)
// WITHOUT materialising the [B,19,H,W] upsampled logits (358 MB at bs=8, 768^2): the low-res logits stay L2-resident
// and each hi-res pixel interpolates its 19 classes in registers. HBM-bound on the int64 labels (37.7 MB).
// Forward: block partial (sum, count) -> fixed-order final reduce (deterministic).
// Backward: the transposed bilinear operator is separable, so the gradient is gathered in two passes without atomics
// (deterministic): (1) per hi-res row, softmax - onehot of every hi-res pixel once (staged in LDS) reduced over its columns to the
// low-res columns -> T[n][H][w][C]; (2) per low-res pixel, T reduced over the supporting hi-res rows.
// Label forms (class template parameter Form, below: hard labels unweighted / weighted, class sets). Weighted: CrossEntropyLoss(weight=...), CrossEntropyLoss2d and
// ImageBasedCrossEntropyLoss2d (/root/reference/loss.py:20-43,71-88,120-180). Every pixel's terms are multiplied by w[image][label] and the divisor is a weight sum
// (of the batch, or of each image with the per-image losses added in image order); pm_label_class_weights builds the image-based weight rows from the labels on
// the device (loss.py:136-146), so the criterion needs neither the materialised logits nor a host round trip.
#include <type_traits>

#include "pm_common.h"

namespace {

constexpr int MAXC = PM_MAX_CLASSES;
constexpr int RX_MAXC = 31;            // class sets: bit C is the ignore class

struct CEGeom {
  const float* logits;
  long lp;           // pitch
  int n, h, w, C;
  const void* labels;      // [n][H][W] words of the label form (Form::word): int64 labels or uint32 class sets
  int H, W;
  float sy, sx, inv_temp;
  // weighted forms only: w = wts[b * wstride + class]; per_image: every image is divided by its own weight sum
  const float* wts;
  long wstride;
  int per_image;
};

// The interpolation expression, written once: every kernel's per-pixel logits carry the same bits because they all come from here.
__device__ __forceinline__ float ce_lerp(const pm_lerp& ly, const pm_lerp& lx, float a, float b, float c, float d) {
  return ly.w0 * (lx.w0 * a + lx.w1 * b) + ly.w1 * (lx.w0 * c + lx.w1 * d);
}

// interpolated logits of hi-res pixel (b, Y, X) into v[0..C), taps from global memory
template <int C_>
__device__ __forceinline__ void interp_logits(const CEGeom& g, int b, const pm_lerp& ly, const pm_lerp& lx, float* v) {
  const float* r0 = g.logits + ((long)(b * g.h + ly.i0) * g.w) * g.lp;
  const float* r1 = g.logits + ((long)(b * g.h + ly.i1) * g.w) * g.lp;
  const float* p00 = r0 + (long)lx.i0 * g.lp;
  const float* p01 = r0 + (long)lx.i1 * g.lp;
  const float* p10 = r1 + (long)lx.i0 * g.lp;
  const float* p11 = r1 + (long)lx.i1 * g.lp;
  const int C = C_ > 0 ? C_ : g.C;
#pragma unroll
  for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c) {
    if (c < C) {
      const float a = p00[c] * g.inv_temp, bq = p01[c] * g.inv_temp, cq = p10[c] * g.inv_temp, d = p11[c] * g.inv_temp;
      v[c] = ce_lerp(ly, lx, a, bq, cq, d);
    }
  }
}

// Workgroups are dealt round-robin to the 8 XCDs, each with its own 4 MB L2. With block id = hi-res row, every XCD would walk ALL low-res logit rows (the four
// hi-res rows between two low-res rows sit on four different XCDs): the 22 MB of main-loss logits were fetched 8 x per sweep (counters, round 4: 226 MB read for
// 60 MB of inputs). Bijective remap (pm_xcd_remap): consecutive hi-res rows -> one XCD, so a low-res row pair is fetched into one L2 and re-used there.

// Block partial: wave sums, then thread 0 adds the waves' sums in wave order: true for that thread alone, with the block's (loss sum, count or weight sum) in lsum and
// lcnt -- the caller stores them. NW = 4: a block of four waves, one expression; NW = 0: blockDim.x / 64 waves, a loop.
template <int N>
__device__ __forceinline__ void ce_wave_partials(float lsum, float lcnt, float (&sm)[2][N]) {
  lsum = pm_wave_sum(lsum);
  lcnt = pm_wave_sum(lcnt);
  if ((threadIdx.x & 63) == 0) sm[0][threadIdx.x >> 6] = lsum, sm[1][threadIdx.x >> 6] = lcnt;
}
template <int NW, int N>
__device__ __forceinline__ bool ce_block_partial(float& lsum, float& lcnt, float (&sm)[2][N]) {
  ce_wave_partials(lsum, lcnt, sm);
  __syncthreads();
  if (threadIdx.x != 0) return false;
  if constexpr (NW == 4) {
    lsum = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3];
    lcnt = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
  } else {
    lsum = lcnt = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) lsum += sm[0][k], lcnt += sm[1][k];
  }
  return true;
}

// Weighted forms, kernels whose block belongs to one image: that image's C weights, staged once per block (visible after the block's next barrier)
__device__ __forceinline__ void ce_stage_weights(const CEGeom& g, int b, float* wsm) {
  if ((int)threadIdx.x < g.C) wsm[threadIdx.x] = g.wts[(long)b * g.wstride + threadIdx.x];
}

// ---- the pieces the row kernels below share, each written once: their outputs agree bit for bit because they run these expressions -----------------------------
// Low-res rows y0 and y1 of image b, columns [x0, x0 + ncol), pre-scaled by 1/T, into L0 / L1 as [x][C | 1]; nt = block size. Both rows in one loop.
__device__ __forceinline__ void ce_stage_rows(const CEGeom& g, int C, int CP, int b, int y0, int y1, int x0, int ncol, int nt, float* L0, float* L1) {
  for (int i = threadIdx.x; i < ncol * C; i += nt) {
    const int xl = i / C, c = i - xl * C;
    L0[xl * CP + c] = g.logits[((long)(b * g.h + y0) * g.w + x0 + xl) * g.lp + c] * g.inv_temp;
    L1[xl * CP + c] = g.logits[((long)(b * g.h + y1) * g.w + x0 + xl) * g.lp + c] * g.inv_temp;
  }
}

// int64 label -> byte: a class below 254 as itself, 255 (ignored) as 255, everything else 254: a label no class matches (as the kernels reading int64 treat it)
__device__ __forceinline__ unsigned char ce_label_byte(int64_t l) { return (l >= 0 && l < 254) ? (unsigned char)l : (l == 255 ? 255 : 254); }

// Class c of a pixel, its logit vc just interpolated: the running maximum mx and the label's logit vl. ARGMAX: the maximum by a strict > scan (not fmaxf), returning
// the lowest index among the maxima as output.max(1)[1].
template <bool ARGMAX, typename Lab>
__device__ __forceinline__ void ce_class_step(float vc, int c, Lab lab, float& mx, float& vl, int& arg) {
  if constexpr (ARGMAX) {
    if (vc > mx) mx = vc, arg = c;
  } else {
    mx = fmaxf(mx, vc);
  }
  if (c == (int)lab) vl = vc;
}
// Sum of exp(v[c] - mx); KEEP: the terms replace v[c] (the field kernels go on to softmax - onehot). v_exp_f32 (~1 ulp per term): the libm expf was 2/3 of the
// row-staged forward's ALU work
template <int C_, bool KEEP>
__device__ __forceinline__ float ce_exp_sum(float* v, float mx, int C) {
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c)
    if (c < C) {
      if constexpr (KEEP) v[c] = __expf(v[c] - mx), se += v[c];
      else se += __expf(v[c] - mx);
    }
  return se;
}

// The field kernels: w (softmax - hot) of one pixel (v from ce_exp_sum; hot = the one-hot entry, or the relaxed form's p / P_S on the classes of the set) into A (left-tap weight: stays in the pixel's low-res column) and B (right-tap weight: owed
// to the next column). w multiplies the difference alone: every other expression stays the unweighted one, so w = 1 leaves its bits.
template <bool WT>
__device__ __forceinline__ void ce_grad_tap(float p, float hot, float wl, float wa, float wb, float& A, float& B) {
  float gq = p - hot;
  if constexpr (WT) gq *= wl;
  A += wa * gq, B += wb * gq;
}

// One pixel whose set holds the real classes S (not empty), v[0..C) its logits and mx their maximum: v becomes exp(v - mx), se their sum, ps the sum over S, wbar the
// mean weight over S; returns the pixel's loss term - wbar log P_S.
template <int C_>
__device__ __forceinline__ float rx_term(float* v, float mx, unsigned S, const float* wsm, int C, float& se, float& ps, float& wbar) {
  se = ce_exp_sum<C_, true>(v, mx, C);
  float ws = 0.f;
  ps = 0.f;
#pragma unroll
  for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c)
    if (c < C && ((S >> c) & 1u)) ps += v[c], ws += wsm[c];
  wbar = ws / (float)__popc(S);
  return wbar * (logf(se) - logf(ps));
}

// ---- the label forms: everything the three losses differ in, as a compile-time parameter (Form) of the kernels below -------------------------------------------------
// HardForm<false>: int64 labels, CE(ignore 255); HardForm<true>: the same with w[image][label]; SetForm: uint32 class sets, the relaxed-border loss (see the relaxed
// section below for its terms). A form names its label word in global memory (word) and in LDS (staged), how a word is held in a register (ld) and staged (stage), when
// a pixel is skipped, whether the image's weight row is staged (weighted) and what a pixel contributes: its loss term and count (term), its one-hot entry (hot) and
// weight (CEPix::wl) for ce_grad_tap, and how an image's folded partials become loss_out (fold_image / fold_batch).
enum CEWhere { CE_FLAT, CE_ROWS, CE_FIELD };      // the kernel a pixel is evaluated in: flat forward; row-staged forward and validation; a field kernel (v is kept as
                                                  // exp(v - mx) for the taps)
struct CEPix {      // what a pixel's term leaves for its taps
  float se, wl, invs;      // sum of exp(v - mx); the weight on (p - hot); sets: 1 / P_S
};

template <bool WT>
struct HardForm {
  using word = int64_t;
  using staged = unsigned char;
  using held = int;      // a staged label in a register
  static constexpr bool weighted = WT, sets = false;
  static constexpr bool prefetch = true;      // the row-staged forward loads a lane's first three words before it stages the logit rows
  static constexpr word none = 255;      // a word that skips its pixel
  // Weighted field kernel of a generic class count: a label that is no class weighs 0 by a select, not by a skip -- the skip's branch tells the compiler that C > 0, it
  // then lays out the class loop differently and contracts the interpolation of class 0 into another fma than the unweighted kernel does (1 ulp)
  template <int C_, CEWhere K>
  static constexpr bool select = WT && C_ == 0 && K == CE_FIELD;
  // The row-staged forward of that class count meets the same through its skip once the lerp loop is a function of its own (the flat forward does not): there the
  // class count enters the comparison through a readfirstlane, which the compiler's value tracking does not see through
  template <int C_, CEWhere K>
  static constexpr bool opaque = WT && C_ == 0 && K == CE_ROWS;
  static __device__ __forceinline__ word ld(word l, int) { return l; }
  static __device__ __forceinline__ staged stage(word l, int) { return ce_label_byte(l); }
  template <int C_, CEWhere K, typename Lab>
  static __device__ __forceinline__ bool skip(Lab lab, int C) {
    if (lab == 255) return true;
    if constexpr (WT && !select<C_, K>) return lab < 0 || lab >= (opaque<C_, K> ? __builtin_amdgcn_readfirstlane(C) : C);      // only labels of a class carry a weight
    else return false;
  }
  template <typename Lab>
  static __device__ __forceinline__ Lab pick(Lab lab) { return lab; }      // the class whose logit ce_class_step picks out of the lerp loop
  // v: the pixel's logits, mx their maximum, vl the label's; own: the pixel counts for this block's partial
  template <int C_, CEWhere K, typename Lab>
  static __device__ __forceinline__ CEPix term(float* v, float mx, float vl, Lab lab, const float* wsm, int C, bool own, float& lsum, float& lcnt) {
    CEPix q{0.f, 1.f, 0.f};
    if constexpr (K == CE_FLAT) {      // libm's expf, as this kernel always had it (ce_exp_sum came with the row-staged forward)
#pragma unroll
      for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c)
        if (c < C) q.se += expf(v[c] - mx);
    } else {
      q.se = ce_exp_sum<C_, K == CE_FIELD>(v, mx, C);
    }
    if constexpr (WT) {
      if constexpr (select<C_, K>) q.wl = lab < C ? wsm[min((int)lab, MAXC - 1)] : 0.f;
      else q.wl = wsm[lab];
      if (own) lsum += q.wl * ((mx + logf(q.se)) - vl), lcnt += q.wl;
    } else {
      if (own) lsum += (mx + logf(q.se)) - vl, lcnt += 1.f;
    }
    return q;
  }
  template <typename Lab>
  static __device__ __forceinline__ float hot(const CEPix&, float, int c, Lab lab) { return c == lab ? 1.f : 0.f; }
  // (sum w nll, sum w) = (s, d) of image b: out[2 + b] = its weight sum; per_image: out[0] = sum over b, in index order, of s_b / d_b -- 0 / 0 = NaN for an image without
  // a weighted pixel, as nll_loss -- and out[1] = total weight sum. Without per_image, out[0] and out[1] are ce_final_kernel's (same order as the unweighted loss).
  static __device__ __forceinline__ void fold_image(double s, double d, int b, int, float* out, double& loss, double& den) {
    out[2 + b] = (float)d;
    loss += s / d;
    den += d;
  }
  static __device__ __forceinline__ void fold_batch(double loss, double den, int, int per_image, float* out) {
    if (per_image) {
      out[0] = (float)loss;
      out[1] = (float)den;
    }
  }
};

struct SetForm {
  using word = uint32_t;
  using staged = uint32_t;      // four bytes a pixel
  using held = uint32_t;
  static constexpr bool weighted = true, sets = true;
  static constexpr bool prefetch = false;
  static constexpr word none = 0u;
  static __device__ __forceinline__ word ld(word s, int C) { return s & ((1u << C) - 1u); }      // the real classes of the set
  static __device__ __forceinline__ staged stage(word s, int C) { return ld(s, C); }
  template <int C_, CEWhere K>
  static __device__ __forceinline__ bool skip(unsigned S, int) { return !S; }
  static __device__ __forceinline__ int pick(unsigned) { return -1; }      // no label logit
  template <int C_, CEWhere K>
  static __device__ __forceinline__ CEPix term(float* v, float mx, float, unsigned S, const float* wsm, int C, bool own, float& lsum, float& lcnt) {
    CEPix q;
    float ps;
    const float t = rx_term<C_>(v, mx, S, wsm, C, q.se, ps, q.wl);
    if (own) lsum += t, lcnt += 1.f;
    q.invs = 1.f / ps;
    return q;
  }
  static __device__ __forceinline__ float hot(const CEPix& q, float e, int c, unsigned S) { return (S >> c) & 1u ? e * q.invs : 0.f; }
  // (sum of terms, valid pixels) = (s, d) of image i: out[2 + i] = loss_i = s / (d + 1), out[2 + n + i] = (d + 1) n: what the row pass divides image i by;
  // out[0] = sum_i loss_i / n, out[1] = valid pixels of the batch
  static __device__ __forceinline__ void fold_image(double s, double d, int b, int n, float* out, double& loss, double& den) {
    const double li = s / (d + 1.0);
    out[2 + b] = (float)li;
    out[2 + n + b] = (float)((d + 1.0) * (double)n);
    loss += li;
    den += d;
  }
  static __device__ __forceinline__ void fold_batch(double loss, double den, int n, int, float* out) {
    out[0] = (float)(loss / (double)n);
    out[1] = (float)den;
  }
};
template <class Form>
__device__ __forceinline__ const typename Form::word* ce_words(const CEGeom& g) { return static_cast<const typename Form::word*>(g.labels); }

// One hi-res pixel from the staged rows (L0 / L1 hold the low-res columns from x0 on): its interpolated logits v[0..C) -- the expression of interp_logits --, their
// maximum mx (ARGMAX: and its index) and the logit vl of class `lab`
template <int C_, bool ARGMAX, typename Lab>
__device__ __forceinline__ void ce_pixel_logits(const pm_lerp& ly, const pm_lerp& lx, const float* L0, const float* L1, int x0, int CP, int C, Lab lab, float* v, float& mx,
                                                float& vl, int& arg) {
  const float *p00 = L0 + (lx.i0 - x0) * CP, *p01 = L0 + (lx.i1 - x0) * CP, *p10 = L1 + (lx.i0 - x0) * CP, *p11 = L1 + (lx.i1 - x0) * CP;
  mx = -INFINITY, vl = 0.f, arg = 0;
#pragma unroll
  for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c)
    if (c < C) ce_class_step<ARGMAX>(v[c] = ce_lerp(ly, lx, p00[c], p01[c], p10[c], p11[c]), c, lab, mx, vl, arg);
}
// ... and, in the field kernels after the form's term<.., CE_FIELD>, what its taps share: 1 / se and the pixel's weight on its left and right low-res column. Class c
// then adds ce_grad_tap<Form::weighted>(v[c] * inv, Form::hot(q, v[c], c, lab), q.wl, wa, wb, A[c], B[c]); that class loop stays in the kernels: as a function of
// its own the compiler lays the generic class count's loops out differently and packs the adds of the loss partial instead of fusing them (other bits).
struct CETaps {
  float inv, wa, wb;
};
__device__ __forceinline__ CETaps ce_taps(const CEPix& q, const pm_lerp& lx) {
  const float inv = 1.f / q.se;
  const float wa = lx.i1 == lx.i0 ? lx.w0 + lx.w1 : lx.w0, wb = lx.i1 == lx.i0 ? 0.f : lx.w1;
  return {inv, wa, wb};
}

// Flat forward (any shape), taps from global memory. Unweighted: one grid over the batch. Weighted forms: blockIdx.y = image (the final fold needs every image's
// partials apart), the x blocks stride over that image's pixels. (loss sum, count or weight sum) per block.
template <int C_, class Form>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const CEGeom g, float* __restrict__ part) {
  constexpr bool IMG = Form::weighted;
  const int C = C_ > 0 ? C_ : g.C;
  const long total = IMG ? (long)g.H * g.W : (long)g.n * g.H * g.W;
  const typename Form::word* labels = ce_words<Form>(g) + (IMG ? (long)blockIdx.y * total : 0);
  const float* wsm = nullptr;
  if constexpr (Form::sets) {      // a weight per class of the set: the image's row, staged
    __shared__ float wrow[MAXC];
    ce_stage_weights(g, blockIdx.y, wrow);
    __syncthreads();
    wsm = wrow;
  } else if constexpr (Form::weighted) {      // one weight per pixel: from global memory
    wsm = g.wts + (long)blockIdx.y * g.wstride;
  }
  float lsum = 0.f, lcnt = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const auto lab = Form::ld(labels[i], C);
    if (Form::template skip<C_, CE_FLAT>(lab, C)) continue;
    const int X = (int)(i % g.W), Y = IMG ? (int)(i / g.W) : (int)((i / g.W) % g.H), b = IMG ? (int)blockIdx.y : (int)(i / ((long)g.W * g.H));
    const pm_lerp ly = pm_ac_lerp(g.sy, Y, g.h), lx = pm_ac_lerp(g.sx, X, g.w);
    float v[C_ > 0 ? C_ : MAXC];
    interp_logits<C_>(g, b, ly, lx, v);
    float mx = -INFINITY, vl = 0.f;
    [[maybe_unused]] int arg = 0;
#pragma unroll
    for (int c = 0; c < (C_ > 0 ? C_ : MAXC); ++c)
      if (c < C) ce_class_step<false>(v[c], c, Form::pick(lab), mx, vl, arg);
    Form::template term<C_, CE_FLAT>(v, mx, vl, lab, wsm, C, true, lsum, lcnt);
  }
  __shared__ float sm[2][4];
  if (ce_block_partial<4>(lsum, lcnt, sm)) {
    const long pb = IMG ? (long)blockIdx.y * gridDim.x + blockIdx.x : blockIdx.x;
    part[pb * 2] = lsum, part[pb * 2 + 1] = lcnt;
  }
}

// Row-staged forward: block = one hi-res row (Y, image b). The two low-res logit rows that row interpolates between are staged in LDS
// once (coalesced, pre-scaled by 1/T); every hi-res pixel then gathers its 4 x C taps from LDS instead of issuing 4 x C scattered global
// loads. The interpolation expression is the one of interp_logits, so the per-pixel logits carry the same bits.
template <int C_, class Form>
__global__ __launch_bounds__(256) void ce_fwd_rows_kernel(const CEGeom g, float* __restrict__ part) {
  extern __shared__ float L[];
  const int C = C_ > 0 ? C_ : g.C;
  const int CP = C | 1;
  const int bid = pm_xcd_remap(blockIdx.x, gridDim.x);
  const int Y = bid % g.H, b = bid / g.H;
  float* wsm = nullptr;
  if constexpr (Form::weighted) {
    __shared__ float wrow[MAXC];
    wsm = wrow;
    ce_stage_weights(g, b, wsm);
  }
  const pm_lerp ly = pm_ac_lerp(g.sy, Y, g.h);
  float* L0 = L;
  float* L1 = L + (size_t)g.w * CP;
  const typename Form::word* lrow = ce_words<Form>(g) + ((long)b * g.H + Y) * g.W;
  typename Form::word labs[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) labs[u] = Form::prefetch && (int)threadIdx.x + 256 * u < g.W ? lrow[threadIdx.x + 256 * u] : Form::none;   // in flight while the rows are staged
  ce_stage_rows(g, C, CP, b, ly.i0, ly.i1, 0, g.w, 256, L0, L1);
  __syncthreads();
  float lsum = 0.f, lcnt = 0.f;
  for (int X = threadIdx.x, u = 0; X < g.W; X += 256, ++u) {
    const auto lab = Form::ld(Form::prefetch && u < 3 ? (u == 0 ? labs[0] : (u == 1 ? labs[1] : labs[2])) : lrow[X], C);
    if (Form::template skip<C_, CE_ROWS>(lab, C)) continue;
    float v[C_ > 0 ? C_ : MAXC], mx, vl;
    [[maybe_unused]] int arg;
    ce_pixel_logits<C_, false>(ly, pm_ac_lerp(g.sx, X, g.w), L0, L1, 0, CP, C, Form::pick(lab), v, mx, vl, arg);
    Form::template term<C_, CE_ROWS>(v, mx, vl, lab, wsm, C, true, lsum, lcnt);
  }
  __shared__ float sm[2][4];
  if (ce_block_partial<4>(lsum, lcnt, sm)) part[bid * 2] = lsum, part[bid * 2 + 1] = lcnt;
}

// One block folds the per-block (loss sum, pixel count) partials in double: 1024 threads keep the chain of dependent loads short (the
// 64-thread version walked 96 L2 round trips per thread: 26 us for 50 KB), then a fixed binary tree in LDS.
constexpr int CE_FINAL_T = 1024;
// nb (sum, count) pairs from pair index `first` on -> s[0][0], s[1][0] (valid after the call's last barrier)
__device__ __forceinline__ void ce_fold_pairs(const float* __restrict__ part, long first, int nb, double (&s)[2][CE_FINAL_T]) {
  double a = 0.0, c = 0.0;
  for (int b = threadIdx.x; b < nb; b += CE_FINAL_T) {
    const float2 v = *reinterpret_cast<const float2*>(part + (first + b) * 2);
    a += (double)v.x, c += (double)v.y;
  }
  s[0][threadIdx.x] = a, s[1][threadIdx.x] = c;
  __syncthreads();
  for (int w = CE_FINAL_T / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s[0][threadIdx.x] += s[0][threadIdx.x + w], s[1][threadIdx.x] += s[1][threadIdx.x + w];
    __syncthreads();
  }
}
__global__ __launch_bounds__(CE_FINAL_T) void ce_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
  __shared__ double s[2][CE_FINAL_T];
  ce_fold_pairs(part, 0, nb, s);
  if (threadIdx.x == 0) {
    out[0] = (float)(s[0][0] / s[1][0]);  // 0/0 -> NaN like torch when every pixel is ignored
    out[1] = (float)s[1][0];
  }
}

// Weighted forms: the block partials are image-major, `per` consecutive ones per image. One block folds image after image (the tree of ce_final_kernel per image, in
// double); what an image's pair and the batch leave in out is the form's (fold_image / fold_batch).
template <class Form>
__global__ __launch_bounds__(CE_FINAL_T) void ce_final_img_kernel(const float* __restrict__ part, int per, int n, int per_image, float* __restrict__ out) {
  __shared__ double s[2][CE_FINAL_T];
  double loss = 0.0, den = 0.0;
  for (int b = 0; b < n; ++b) {
    ce_fold_pairs(part, (long)b * per, per, s);
    if (threadIdx.x == 0) Form::fold_image(s[0][0], s[1][0], b, n, out, loss, den);
    __syncthreads();      // s is rewritten for the next image
  }
  if (threadIdx.x == 0) Form::fold_batch(loss, den, n, per_image, out);
}

// pass 2: thread per (low-res pixel, class): supporting hi-res rows in ascending order, then the loss scale (WT, per_image: the image's own weight sum divides)
template <bool WT = false>
__global__ __launch_bounds__(256) void ce_bwd_cols_kernel(const CEGeom g, const float* __restrict__ T, const float* __restrict__ loss_out,
                                                          const float* __restrict__ gscale, float* __restrict__ dl, long dlp) {
  const int C = g.C;
  const long total = (long)g.n * g.h * g.w * C;
  const float gs = (gscale ? gscale[0] : 1.f) * g.inv_temp / loss_out[1];
  // consecutive logical blocks (neighbouring low-res rows, which share most of their supporting field rows) on one XCD's L2
  for (long i = (long)pm_xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long q = i / C;
    const int x = (int)(q % g.w);
    q /= g.w;
    const int y = (int)(q % g.h), b = (int)(q / g.h);
    int lo, hi;
    pm_support(g.sy, y, g.H, lo, hi);
    float acc = 0.f;
    for (int Y = lo; Y <= hi; ++Y) acc += pm_tap_weight(pm_ac_lerp(g.sy, Y, g.h), y) * T[(((long)b * g.H + Y) * g.w + x) * C + c];
    if constexpr (WT) {
      const float gsb = g.per_image ? (gscale ? gscale[0] : 1.f) * g.inv_temp / loss_out[2 + b] : gs;
      dl[((long)(b * g.h + y) * g.w + x) * dlp + c] = acc * gsb;
    } else {
      dl[((long)(b * g.h + y) * g.w + x) * dlp + c] = acc * gs;
    }
  }
}

// ---- forward and the first backward pass in ONE sweep over the labels ------------------------------------------------------------
// The forward already evaluates the softmax of every hi-res pixel; softmax - onehot is all the backward needs from the labels and the
// up-sampled logits, and the upstream scale is a scalar that can be applied last. So the training forward leaves the column-reduced field
//   T[b][Y][x][c] = sum over hi-res columns X of (softmax - onehot)(b, Y, X)[c] * (bilinear weight of X on low-res column x)
// behind, and the backward is the row pass (ce_bwd_cols_kernel) alone: the labels and the logits are read once per step instead of twice.
// Block = one hi-res row (Y, image b): the label row (as bytes) and the two low-res logit rows it interpolates between are staged in LDS.
// Lane group (low-res column x, part p of PARTS) walks its share of the hi-res pixels whose left tap is x -- every pixel is evaluated exactly
// once -- and keeps two weighted sums per class: A (left-tap weight, stays in column x) and B (right-tap weight, goes to column x + 1).
// The PARTS lanes of a column are combined by a fixed butterfly, columns exchange B through LDS, and T leaves as one contiguous row.
// Fixed association order everywhere: run-to-run deterministic.
__device__ __forceinline__ int ce_first_ge(float sx, int k, int w, int W) {   // first hi-res column whose left tap i0 is >= k (i0 is non-decreasing)
  if (k <= 0) return 0;
  if (k > w - 1 || sx <= 0.f) return W;
  int X = (int)ceilf((float)k / sx);
  X = max(0, min(W, X));
  while (X > 0 && pm_ac_lerp(sx, X - 1, w).i0 >= k) --X;
  while (X < W && pm_ac_lerp(sx, X, w).i0 < k) ++X;
  return X;
}

template <int C_, int PARTS, class Form>
__global__ __launch_bounds__(256) void ce_fused_rows_kernel(const CEGeom g, float* __restrict__ part, float* __restrict__ T) {
  extern __shared__ float L[];
  __shared__ float carry[MAXC];   // B of the last column of a round, owed to the first column of the next (rows wider than one round only)
  const int C = C_ > 0 ? C_ : g.C;
  const int CP = C | 1;
  const int nt = (int)blockDim.x, tid = (int)threadIdx.x;
  const int bid = pm_xcd_remap(blockIdx.x, gridDim.x);
  const int Y = bid % g.H, b = bid / g.H;
  float* wsm = nullptr;
  if constexpr (Form::weighted) {
    __shared__ float wrow[MAXC];
    wsm = wrow;
    ce_stage_weights(g, b, wsm);
  }
  const pm_lerp ly = pm_ac_lerp(g.sy, Y, g.h);
  float* L0 = L;
  float* L1 = L + (size_t)g.w * CP;                                   // (+ C floats of slack behind it: bufB holds one column more than a round)
  typename Form::staged* labs = reinterpret_cast<typename Form::staged*>(L1 + (size_t)g.w * CP + C);
  const typename Form::word* lrow = ce_words<Form>(g) + ((long)b * g.H + Y) * g.W;
  for (int X = tid; X < g.W; X += nt) labs[X] = Form::stage(lrow[X], C);
  auto stage_rows = [&]() { ce_stage_rows(g, C, CP, b, ly.i0, ly.i1, 0, g.w, nt, L0, L1); };
  stage_rows();
  __syncthreads();
  constexpr int CR = C_ > 0 ? C_ : MAXC;
  float lsum = 0.f, lcnt = 0.f;
  const int R = nt / PARTS;                       // low-res columns per round
  const int rounds = (g.w + R - 1) / R;
  for (int rd = 0; rd < rounds; ++rd) {
    if (rd > 0) {                                 // the previous round recycled the staged rows as its exchange buffers
      __syncthreads();
      stage_rows();
      __syncthreads();
    }
    const int xr0 = rd * R, xr1 = min(g.w, xr0 + R);
    const int x = xr0 + tid / PARTS, p = tid % PARTS;
    const bool live = x < xr1;
    float A[CR], B[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) A[c] = B[c] = 0.f;
    if (live) {
      const int j0 = ce_first_ge(g.sx, x, g.w, g.W), j1 = ce_first_ge(g.sx, x + 1, g.w, g.W);
      const int per = (j1 - j0 + PARTS - 1) / PARTS;
      const int ja = j0 + p * per, jb = min(j1, ja + per);
      for (int X = ja; X < jb; ++X) {
        const typename Form::held lab = labs[X];
        if (Form::template skip<C_, CE_FIELD>(lab, C)) continue;
        const pm_lerp lx = pm_ac_lerp(g.sx, X, g.w);
        float v[CR], mx, vl;
        [[maybe_unused]] int arg;
        ce_pixel_logits<C_, false>(ly, lx, L0, L1, 0, CP, C, Form::pick(lab), v, mx, vl, arg);
        const CEPix q = Form::template term<C_, CE_FIELD>(v, mx, vl, lab, wsm, C, true, lsum, lcnt);
        const CETaps t = ce_taps(q, lx);
#pragma unroll
        for (int c = 0; c < CR; ++c)
          if (c < C) ce_grad_tap<Form::weighted>(v[c] * t.inv, Form::hot(q, v[c], c, lab), q.wl, t.wa, t.wb, A[c], B[c]);
      }
    }
    if constexpr (PARTS > 1) {
#pragma unroll
      for (int o = 1; o < PARTS; o <<= 1)
#pragma unroll
        for (int c = 0; c < CR; ++c)
          if (c < C) A[c] += __shfl_xor(A[c], o, 64), B[c] += __shfl_xor(B[c], o, 64);
    }
    __syncthreads();                            // every lane is done with the staged rows: they become the exchange buffers
    float* bufA = L0;                           // A of column x         -> bufA[x - xr0]
    float* bufB = L1;                           // B of column x (owed to column x + 1) -> bufB[x - xr0 + 1]; bufB[0] = carry of the previous round
    if (live && p == 0) {
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          bufA[(x - xr0) * C + c] = A[c];
          bufB[(x - xr0 + 1) * C + c] = B[c];
        }
    }
    if (tid < C) bufB[tid] = rd == 0 ? 0.f : carry[tid];
    __syncthreads();
    float* Trow = T + (((long)b * g.H + Y) * g.w + xr0) * C;
    for (int i = tid; i < (xr1 - xr0) * C; i += nt) Trow[i] = bufB[i] + bufA[i];
    if (tid < C) carry[tid] = bufB[(xr1 - xr0) * C + tid];
  }
  __shared__ float sm[2][4];
  if (ce_block_partial<0>(lsum, lcnt, sm)) part[bid * 2] = lsum, part[bid * 2 + 1] = lcnt;
}

// ---- the same sweep with the ROW half of the transposed bilinear operator folded in (round 4, second session) ------------------------------------------------
// ce_fused_rows_kernel leaves one column-reduced row per HI-RES row (T[n][H][w][C]: 89.7 MB for the main loss) and the backward gathers ~8 of them per low-res
// pixel. Here a block owns a low-res row INTERVAL y -- every hi-res row whose upper tap is y (four of them at 192 -> 768) -- and folds their column-reduced rows with
// the two row weights straight away: FA[b][y] = sum_Y w0(Y) T_Y (stays in low-res row y), FB[b][y] = sum_Y w1(Y) T_Y (owed to row y + 1). The field is two
// low-res-sized rows per interval (2 x 22.4 MB) and the backward is dl[y] = (FA[y] + FB[y - 1]) x scale, elementwise.
//   * block = RG row groups x TPR threads; group gi takes rows Ya + gi, Ya + gi + RG, ...; lane x of a group = low-res column x (the form for modest up-sampling
//     ratios: one lane per column, PARTS == 1), walking the hi-res pixels whose left tap is x exactly as the kernel above (same expressions, same order);
//   * the right-tap sums B go to the neighbouring lane by a one-lane shuffle (wave edges through LDS) instead of an LDS round trip of the whole row;
//   * every round the groups fold their row into the block's LDS accumulators accA / accB in group order (one barrier per group: per-lane register accumulators
//     for all rounds put the 1 024-thread block 27 registers over its 128-register budget and the spills into the pixel loop: 190 instead of 120 us), loss
//     partials per block: all fixed-order, deterministic.
__host__ __device__ __forceinline__ int ce2_rows_per_interval(int h, int H) { return (H + h - 1) / h + 1; }
template <int C_, class Form>      // hard-label forms only
__global__ __launch_bounds__(1024) void ce_fused_rows2_kernel(const CEGeom g, float* __restrict__ part, float* __restrict__ FA, float* __restrict__ FB, int tpr, int rg, int nseg, int ws) {
  extern __shared__ float L[];
  __shared__ float sm2[2][16];
  constexpr int CR = C_ > 0 ? C_ : MAXC;
  const int C = C_ > 0 ? C_ : g.C;
  const int CP = C | 1;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int gi = tid / tpr, x = tid - gi * tpr, lane = tid & 63, wv = x >> 6;       // group, low-res column (lane of the group), wave of the group
  const int nwv = tpr >> 6;
  // block = (image b, interval y, column segment seg): the segment owns the low-res columns [c0, c0 + ncol); lane x of a group is column c0 - 1 + x, i.e. lane 0 is
  // the column LEFT of the segment -- it evaluates its hi-res pixels only for the right-tap sums B they owe to column c0 (4 % of redundant work at 96 columns per
  // segment; its loss terms and its own row entries belong to the neighbouring segment and are dropped here). Half the columns per block = half the LDS: four
  // resident blocks per CU instead of two.
  const int bid = pm_xcd_remap(blockIdx.x, gridDim.x);
  const int seg = bid % nseg, y = (bid / nseg) % g.h, b = bid / (nseg * g.h);
  const int y1 = min(y + 1, g.h - 1);
  float* wsm = nullptr;
  if constexpr (Form::weighted) {
    __shared__ float wrow[MAXC];
    wsm = wrow;
    ce_stage_weights(g, b, wsm);
  }
  const int c0 = seg * ws, ncol = min(ws, g.w - c0);
  const int cb = max(c0 - 1, 0), ce = min(c0 + ncol, g.w - 1), nst = ce - cb + 1;   // staged low-res columns [cb, ce]: the taps of the lanes' pixels
  const int Wp = (g.W + 15) & ~15;
  float* L0 = L;
  float* L1 = L + (size_t)(ws + 2) * CP;
  float* accA = L1 + (size_t)(ws + 2) * CP;                                         // [ws][C] x 2: the block's pieces of the FA / FB rows
  float* accB = accA + (size_t)ws * C;
  float* edge = accB + (size_t)ws * C;                                              // [rg][nwv][CR]: B of a wave's last lane, owed to the next wave's lane 0
  unsigned char* lab8 = reinterpret_cast<unsigned char*>(edge + (size_t)rg * nwv * CR);   // [rg][Wp]
  ce_stage_rows(g, C, CP, b, y, y1, cb, nst, nt, L0, L1);
  for (int i = tid; i < ws * C; i += nt) accA[i] = 0.f, accB[i] = 0.f;
  const int Ya = ce_first_ge(g.sy, y, g.h, g.H), Yb = ce_first_ge(g.sy, y + 1, g.h, g.H);
  const int Xlo = ce_first_ge(g.sx, cb, g.w, g.W), Xhi = ce_first_ge(g.sx, c0 + ncol, g.w, g.W);   // hi-res columns whose left tap is one of the lanes' columns
  const int ov = nseg > 1 ? 1 : 0;                                                  // a single segment needs no neighbour lane
  const int xc = c0 - ov + x;                                                       // this lane's low-res column
  const bool own = x >= ov && x < ov + ncol;                                        // a column of the segment (with segments, lane 0: the left neighbour, B only)
  const bool colive = own || (ov && x == 0 && c0 > 0);
  int j0 = 0, j1 = 0;
  if (colive) j0 = ce_first_ge(g.sx, xc, g.w, g.W), j1 = ce_first_ge(g.sx, xc + 1, g.w, g.W);
  float lsum = 0.f, lcnt = 0.f;
  const int rounds = (Yb - Ya + rg - 1) / rg;
  for (int rd = 0; rd < rounds; ++rd) {
    const int Y = Ya + rd * rg + gi;
    const bool rowlive = Y < Yb;
    unsigned char* mylab = lab8 + (size_t)gi * Wp;
    if (rowlive) {
      const typename Form::word* lrow = ce_words<Form>(g) + ((long)b * g.H + Y) * g.W;
      for (int X = Xlo + x; X < Xhi; X += tpr) mylab[X - Xlo] = Form::stage(lrow[X], C);
    }
    __syncthreads();                                 // labels (and, in the first round, the logit rows) are staged
    float A[CR], B[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) A[c] = B[c] = 0.f;
    pm_lerp ly = pm_ac_lerp(g.sy, rowlive ? Y : Ya, g.h);
    if (rowlive && colive) {
      for (int X = j0; X < j1; ++X) {
        const typename Form::held lab = mylab[X - Xlo];
        if (Form::template skip<C_, CE_FIELD>(lab, C)) continue;
        const pm_lerp lx = pm_ac_lerp(g.sx, X, g.w);
        float v[CR], mx, vl;
        [[maybe_unused]] int arg;
        ce_pixel_logits<C_, false>(ly, lx, L0, L1, cb, CP, C, Form::pick(lab), v, mx, vl, arg);
        const CEPix q = Form::template term<C_, CE_FIELD>(v, mx, vl, lab, wsm, C, own, lsum, lcnt);      // own: the left-neighbour lane's pixels are counted by their segment
        const CETaps t = ce_taps(q, lx);
#pragma unroll
        for (int c = 0; c < CR; ++c)
          if (c < C) ce_grad_tap<Form::weighted>(v[c] * t.inv, Form::hot(q, v[c], c, lab), q.wl, t.wa, t.wb, A[c], B[c]);
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) edge[((size_t)gi * nwv + wv) * CR + c] = B[c];
    }
    __syncthreads();                                 // wave-edge values are in LDS; every lane is done with this round's labels
    {
      const float wA = ly.i1 == ly.i0 ? ly.w0 + ly.w1 : ly.w0, wB = ly.i1 == ly.i0 ? 0.f : ly.w1;
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          float bs = __shfl_up(B[c], 1, 64);
          if (lane == 0) bs = wv > 0 ? edge[((size_t)gi * nwv + wv - 1) * CR + c] : 0.f;
          A[c] = bs + A[c];                           // the column-reduced row entry T[Y][x][c] of the kernel above (same two terms)
        }
      for (int k = 0; k < rg; ++k) {                  // fold into the block's rows, group after group
        if (gi == k && rowlive && own) {
#pragma unroll
          for (int c = 0; c < CR; ++c)
            if (c < C) accA[(x - ov) * C + c] += wA * A[c], accB[(x - ov) * C + c] += wB * A[c];
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();                                    // (also the barrier between staging / zeroing and the stores when an interval has no row)
  float* outA = FA + (((long)b * g.h + y) * g.w + c0) * C;
  float* outB = FB + (((long)b * g.h + y) * g.w + c0) * C;
  for (int i = tid; i < ncol * C; i += nt) outA[i] = accA[i], outB[i] = accB[i];
  if (ce_block_partial<0>(lsum, lcnt, sm2)) part[bid * 2] = lsum, part[bid * 2 + 1] = lcnt;
}
// backward of the interval form: dl[b][y][x][c] = (FA[b][y][x][c] + FB[b][y - 1][x][c]) x upstream scale / valid pixels / T
template <bool WT = false>
__global__ __launch_bounds__(256) void ce_bwd_rows2_kernel(const CEGeom g, const float* __restrict__ FA, const float* __restrict__ FB, const float* __restrict__ loss_out,
                                                           const float* __restrict__ gscale, float* __restrict__ dl, long dlp) {
  const int C = g.C;
  const long rowsz = (long)g.w * C, total = (long)g.n * g.h * rowsz;
  const float gs = (gscale ? gscale[0] : 1.f) * g.inv_temp / loss_out[1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long pix = i / C;
    const int c = (int)(i - pix * C);
    const int y = (int)((pix / g.w) % g.h);
    const float v = FA[i] + (y > 0 ? FB[i - rowsz] : 0.f);
    if constexpr (WT) {
      const float gsb = g.per_image ? (gscale ? gscale[0] : 1.f) * g.inv_temp / loss_out[2 + pix / ((long)g.w * g.h)] : gs;
      dl[pix * dlp + c] = v * gsb;
    } else {
      dl[pix * dlp + c] = v * gs;
    }
  }
}
constexpr size_t ROWS2_MAX_LDS = 120 * 1024;      // dynamic LDS of the interval form (opt-in beyond 64 KB, set per device at the first launch)
struct Rows2Plan {
  bool ok;
  int tpr, rg, nseg, ws;
  size_t lds;
};
inline Rows2Plan rows2_plan(const CEGeom& g) {
  constexpr int SEG_COLS = 96;
  constexpr int MAX_THREADS = 256;      // measured best (gpu_r6_ce.sh)
  Rows2Plan p{};
  const int ratio = std::max(1, g.W / std::max(1, g.w));
  p.nseg = std::max(1, (g.w + SEG_COLS - 1) / SEG_COLS);      // column segments per interval (<= 96 columns each: 31 KB of LDS at 19 classes)
  p.ws = (g.w + p.nseg - 1) / p.nseg;
  p.nseg = (g.w + p.ws - 1) / p.ws;
  p.tpr = std::min(320, (p.ws + (p.nseg > 1 ? 1 : 0) + 63) / 64 * 64);      // + the left-neighbour lane when there are segments
  p.rg = std::max(1, std::min(ce2_rows_per_interval(g.h, g.H), MAX_THREADS / std::max(64, p.tpr)));
  p.lds = ((size_t)2 * (p.ws + 2) * (g.C | 1) + (size_t)2 * p.ws * g.C + (size_t)p.rg * (p.tpr / 64) * MAXC) * sizeof(float) + (size_t)p.rg * ((g.W + 15) & ~15);
  // one lane per low-res column (modest up-sampling ratios; the 16-fold read loss keeps the PARTS form: its field is small), up-sampling only (block count <= hi-res rows:
  // the partial workspace is sized for those), everything in 64 KB of dynamic LDS
  p.ok = g.C == 19 && g.w <= 256 && ratio < 8 && g.H >= g.h && g.h >= 1 && p.lds <= ROWS2_MAX_LDS && (long)g.n * g.h * p.nseg <= (1l << 30) && p.nseg <= 2 * std::max(1, g.H / std::max(1, g.h)) ;      // 19 classes: the
  // specialised instantiation (2 x 19 accumulators + 3 x 19 working registers sit at the 128-register budget of a 1 024-thread block; 32 classes would not)
  return p;
}

template <class Form>
inline void rows2_launch(const CEGeom& g, const Rows2Plan& r, float* part, float* field, hipStream_t st) {
  static pm_lds_optin optin;      // > 64 KB of dynamic LDS needs the opt-in, once per device
  (void)optin(reinterpret_cast<const void*>(&ce_fused_rows2_kernel<19, Form>), (int)ROWS2_MAX_LDS);
  const long half = (long)g.n * g.h * g.w * g.C;
  hipLaunchKernelGGL((ce_fused_rows2_kernel<19, Form>), dim3(g.n * g.h * r.nseg), dim3(r.tpr * r.rg), r.lds, st, g, part, field, field + half, r.tpr, r.rg, r.nseg, r.ws);
}

inline int fwd_blocks(long total) { return (int)std::min<long>((total + 255) / 256, 4096); }
inline int wfwd_blocks(long hw) { return (int)std::min<long>((hw + 255) / 256, 512); }      // x blocks per image of the flat forward of the weighted forms

enum CEForm { CE_HARD, CE_WEIGHTED, CE_SETS };      // the run-time names of HardForm<false>, HardForm<true>, SetForm
// one pair of block partials per block of any forward or field kernel of the form
inline size_t ce_workspace(CEForm form, int n, int H, int W) {
  const long flat = form == CE_HARD ? fwd_blocks((long)n * H * W) : (long)n * wfwd_blocks((long)H * W);
  const long rows = (long)n * H * (form == CE_SETS ? 1 : 2);      // hard labels: the interval form has <= 2 n H blocks (rows2_plan)
  return pm_align_up((size_t)std::max<long>(flat, rows) * 2 * sizeof(float), 256);
}

// The geometry of a call of any form (the relaxed entry points hand their flat logit arguments over as a pm_tensor of their own); each form keeps its checks.
int fill(CEGeom& g, const char* who, CEForm form, const pm_tensor* logits, float inv_temp, const void* labels, int H, int W) {
  if (form == CE_SETS) {
    PM_REQUIRE(logits->ptr && logits->n > 0 && logits->h > 0 && logits->w > 0 && H > 0 && W > 0, PM_EINVAL, "%s: null/empty", who);
    PM_REQUIRE(logits->c >= 1 && logits->c <= RX_MAXC, PM_EUNSUPPORTED, "%s: classes %d not in 1..%d", who, logits->c, RX_MAXC);
    PM_REQUIRE(logits->pitch >= logits->c, PM_EINVAL, "%s: pitch %lld < %d classes", who, (long long)logits->pitch, logits->c);
  } else {
    PM_REQUIRE(logits && logits->ptr && labels && H > 0 && W > 0, PM_EINVAL, "%s: null/empty", who);
    PM_REQUIRE(logits->c >= 1 && logits->c <= MAXC, PM_EUNSUPPORTED, "%s: classes %d > %d", who, logits->c, MAXC);
  }
  g.logits = (const float*)logits->ptr, g.lp = logits->pitch, g.n = logits->n, g.h = logits->h, g.w = logits->w, g.C = logits->c;
  g.labels = labels, g.H = H, g.W = W;
  g.sy = pm_ac_scale(logits->h, H), g.sx = pm_ac_scale(logits->w, W), g.inv_temp = inv_temp;
  g.wts = nullptr, g.wstride = 0, g.per_image = form == CE_SETS;      // sets: the row pass divides every image by its own divisor
  return PM_OK;
}

// The weighted entry points' extra arguments; a null CEWeights* is the unweighted loss.
struct CEWeights {
  const float* w;
  int64_t stride;
  int per_image;
};
int fill_w(CEGeom& g, const CEWeights& wt, const char* who) {
  PM_REQUIRE(wt.w, PM_EINVAL, "%s: null weights", who);
  PM_REQUIRE(wt.stride == 0 || wt.stride >= g.C, PM_EINVAL, "%s: weight_stride %lld is neither 0 nor >= %d classes", who, (long long)wt.stride, g.C);
  PM_REQUIRE(wt.per_image == 0 || wt.per_image == 1, PM_EINVAL, "%s: per_image %d is neither 0 nor 1", who, wt.per_image);
  g.wts = wt.w, g.wstride = (long)wt.stride, g.per_image = wt.per_image;
  return PM_OK;
}

// f(class count as a constant: 19 or 0 = generic, the form as an object): the one place where the run-time (C == 19, form) pair picks a kernel instantiation
template <class F>
inline void ce_dispatch(int C, CEForm form, F&& f) {
  auto with = [&](auto cc) {
    if (form == CE_HARD) f(cc, HardForm<false>{});
    else if (form == CE_WEIGHTED) f(cc, HardForm<true>{});
    else f(cc, SetForm{});
  };
  if (C == 19) with(std::integral_constant<int, 19>{});
  else with(std::integral_constant<int, 0>{});
}

struct FusedPlan {
  int parts, threads;
  size_t lds;
};
inline FusedPlan fused_plan(const CEGeom& g, size_t label_bytes) {      // label_bytes: of a staged label, sizeof(Form::staged)
  FusedPlan p;
  // ~4 hi-res pixels per lane: PARTS lanes share a low-res column when the up-sampling ratio is large (the read loss: 768 / 48 = 16)
  const int ratio = std::max(1, g.W / std::max(1, g.w));
  p.parts = 1;
  while (p.parts < 16 && p.parts * 8 <= ratio && g.w * p.parts * 2 <= 256) p.parts *= 2;
  p.threads = std::min(256, std::max(64, (g.w * p.parts + 63) / 64 * 64));
  p.lds = ((size_t)2 * g.w * (g.C | 1) + g.C) * sizeof(float) + label_bytes * ((size_t)(g.W + 15) / 16 * 16);
  return p;
}
constexpr size_t FUSED_MAX_LDS = 159 * 1024;   // dynamic part; the kernel also declares up to 288 B of static LDS
inline size_t ce_label_bytes(CEForm form) { return form == CE_SETS ? sizeof(SetForm::staged) : sizeof(HardForm<false>::staged); }
template <int CC, int PP, class Form>
void fused_launch_one(const CEGeom& g, const FusedPlan& p, float* part, float* T, hipStream_t st) {
  // > 64 KB of dynamic LDS (logit rows wider than ~420 pixels x 19 classes) needs an explicit opt-in, once per kernel AND device
  static pm_lds_optin optin;
  (void)optin(reinterpret_cast<const void*>(&ce_fused_rows_kernel<CC, PP, Form>), (int)FUSED_MAX_LDS);
  hipLaunchKernelGGL((ce_fused_rows_kernel<CC, PP, Form>), dim3(g.n * g.H), dim3(p.threads), p.lds, st, g, part, T);
}

// ---- the one host route: every forward and field entry point ends here --------------------------------------------------------------------------------------------
// Chooses the kernel -- field: interval form (hard labels) or PARTS form; forward: row-staged or flat --, launches it with block partials into `part` and, given a
// loss_out, folds them. `who` is the entry point's name (it leads every message); the caller has filled g and checked its own arguments.
enum CERoute { CE_INTERVAL, CE_PARTS, CE_ROW_STAGED, CE_FLAT_GRID };
int ce_run(const char* who, const CEGeom& g, CEForm form, bool want_field, float* loss_out, float* field, float* part, hipStream_t st) {
  Rows2Plan r{};
  FusedPlan p{};
  const size_t row_lds = 2 * (size_t)g.w * (g.C | 1) * sizeof(float);     // the two staged low-res rows
  CERoute route;
  if (want_field) route = form != CE_SETS && (r = rows2_plan(g)).ok ? CE_INTERVAL : CE_PARTS;
  else route = row_lds <= 48 * 1024 && (long)g.n * g.H <= (1 << 20) && g.W >= 32 ? CE_ROW_STAGED : CE_FLAT_GRID;      // row-staged: one block per hi-res row
  // image-major grids (blockIdx.y = image): the flat forward of the weighted forms; the relaxed entry points refuse such a batch on every route
  PM_REQUIRE(g.n <= 65535 || form == CE_HARD || (form == CE_WEIGHTED && route != CE_FLAT_GRID), PM_EUNSUPPORTED, "%s: %d images > 65535", who, g.n);
  if (route == CE_PARTS) {
    p = fused_plan(g, ce_label_bytes(form));
    PM_REQUIRE(p.lds <= FUSED_MAX_LDS && (long)g.n * g.H <= (1l << 30), PM_EUNSUPPORTED, "%s: logit rows of %d x %d classes do not fit LDS", who, g.w, g.C);
  }
  int per = g.H, n = g.n;      // block partials per image, images
  ce_dispatch(g.C, form, [&](auto cc, auto fm) {
    constexpr int CC = decltype(cc)::value;
    using Form = decltype(fm);
    switch (route) {
      case CE_INTERVAL:
        per = g.h * r.nseg;
        if constexpr (CC == 19 && !Form::sets) rows2_launch<Form>(g, r, part, field, st);
        break;
      case CE_PARTS:
        switch (p.parts) {
          case 1: fused_launch_one<CC, 1, Form>(g, p, part, field, st); break;
          case 2: fused_launch_one<CC, 2, Form>(g, p, part, field, st); break;
          case 4: fused_launch_one<CC, 4, Form>(g, p, part, field, st); break;
          case 8: fused_launch_one<CC, 8, Form>(g, p, part, field, st); break;
          default: fused_launch_one<CC, 16, Form>(g, p, part, field, st); break;
        }
        break;
      case CE_ROW_STAGED: hipLaunchKernelGGL((ce_fwd_rows_kernel<CC, Form>), dim3(g.n * g.H), dim3(256), row_lds, st, g, part); break;
      case CE_FLAT_GRID:
        if (Form::weighted) {      // image-major grid: the final fold needs every image's partials apart
          per = wfwd_blocks((long)g.H * g.W);
          hipLaunchKernelGGL((ce_fwd_kernel<CC, Form>), dim3(per, g.n), dim3(256), 0, st, g, part);
        } else {                   // one grid over the batch
          per = fwd_blocks((long)g.n * g.H * g.W), n = 1;
          hipLaunchKernelGGL((ce_fwd_kernel<CC, Form>), dim3(per), dim3(256), 0, st, g, part);
        }
        break;
    }
  });
  // Final fold of n x per block partials (image-major for the weighted forms). Hard labels, unweighted or weighted over the batch: loss and divisor in the order of
  // ce_final_kernel; the weighted forms then add what they keep per image (and, per_image, the sum of the images' own means).
  if (loss_out) {
    if (form == CE_HARD || (form == CE_WEIGHTED && !g.per_image)) hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(CE_FINAL_T), 0, st, (const float*)part, n * per, loss_out);
    if (form == CE_WEIGHTED) hipLaunchKernelGGL(ce_final_img_kernel<HardForm<true>>, dim3(1), dim3(CE_FINAL_T), 0, st, (const float*)part, per, n, g.per_image, loss_out);
    if (form == CE_SETS) hipLaunchKernelGGL(ce_final_img_kernel<SetForm>, dim3(1), dim3(CE_FINAL_T), 0, st, (const float*)part, per, n, 1, loss_out);
  }
  return pm_check_launch(who);
}

// Every forward and training-forward entry point: its argument checks, then the route. wt: the weights, or null (CE_HARD).
int ce_fwd(const char* who, CEForm form, const pm_tensor* logits, float inv_temp, const void* labels, int H, int W, const CEWeights* wt, bool want_field, float* loss_out,
           float* field, void* ws, size_t ws_bytes, hipStream_t st) {
  PM_REQUIRE_F32(logits, who);
  CEGeom g;
  if (int e = fill(g, who, form, logits, inv_temp, labels, H, W)) return e;
  PM_REQUIRE(labels, PM_EINVAL, "%s: null bits", who);      // (null int64 labels: refused by fill)
  if (wt)
    if (int e = fill_w(g, *wt, who)) return e;
  PM_REQUIRE(loss_out && (field || !want_field) && ws && ws_bytes >= ce_workspace(form, g.n, H, W), PM_EWORKSPACE,
             want_field || form == CE_SETS ? "%s: workspace too small / null field" : "%s: workspace too small", who);
  return ce_run(who, g, form, want_field, loss_out, field, (float*)ws, st);
}

// The row pass over a field (the backward proper): reads neither labels, logits nor weights. loss_out: where the divisors sit ([1]; per image from [2] on).
void ce_row_pass(const CEGeom& g, CEForm form, const float* field, const float* loss_out, const float* gscale, float* dl, long dlp, hipStream_t st) {
  const long total = (long)g.n * g.h * g.w * g.C;
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1 << 20));
  const bool rows2 = form != CE_SETS && rows2_plan(g).ok;
  ce_dispatch(0, form, [&](auto, auto fm) {
    constexpr bool WT = decltype(fm)::weighted;
    if (rows2) hipLaunchKernelGGL(ce_bwd_rows2_kernel<WT>, grid, dim3(256), 0, st, g, field, field + total, loss_out, gscale, dl, dlp);
    else hipLaunchKernelGGL(ce_bwd_cols_kernel<WT>, grid, dim3(256), 0, st, g, field, loss_out, gscale, dl, dlp);
  });
}

// wt: only per_image is read
int ce_bwd_field(const char* who, const pm_tensor* logits, float inv_temp, int H, int W, const CEWeights* wt, const float* loss_out, const float* gscale,
                 const float* field, const pm_tensor* dlogits, hipStream_t st) {
  PM_REQUIRE_F32(logits, who);
  PM_REQUIRE_F32(dlogits, who);
  CEGeom g;
  static const int64_t dummy = 0;
  if (int e = fill(g, who, wt ? CE_WEIGHTED : CE_HARD, logits, inv_temp, &dummy, H, W)) return e;
  if (wt) {
    PM_REQUIRE(wt->per_image == 0 || wt->per_image == 1, PM_EINVAL, "%s: per_image %d is neither 0 nor 1", who, wt->per_image);
  }
  PM_REQUIRE(loss_out && field && dlogits && dlogits->ptr && pm_same_shape(logits, dlogits), PM_EINVAL, "%s: bad args", who);
  if (wt) g.per_image = wt->per_image;
  ce_row_pass(g, wt ? CE_WEIGHTED : CE_HARD, field, loss_out, gscale, (float*)dlogits->ptr, (long)dlogits->pitch, st);
  return pm_check_launch(who);
}

}  // namespace

extern "C" size_t pm_upsample_ce_workspace(int n, int H, int W) { return ce_workspace(CE_HARD, n, H, W); }
extern "C" size_t pm_upsample_wce_workspace(int n, int H, int W) { return ce_workspace(CE_WEIGHTED, n, H, W); }
extern "C" size_t pm_upsample_wce_loss_floats(int n) { return (size_t)2 + (size_t)std::max(n, 0); }

extern "C" size_t pm_upsample_ce_field_bytes(const pm_tensor* logits, int H, int W) {
  if (!logits || !pm_is_f32(logits)) return 0;      // fp32 tensors only
  // 0 also when the fused row kernel cannot take the shape -- two low-res logit rows + the label row of one hi-res row must fit LDS (159 KB: w <= ~1000 low-res
  // columns at 19 classes) -- so that a caller routes such shapes elsewhere instead of meeting PM_EUNSUPPORTED (ops.upsample_ce composes resize + CE then)
  CEGeom g{};
  g.n = logits->n, g.h = logits->h, g.w = logits->w, g.H = H, g.W = W, g.C = logits->c;
  if (rows2_plan(g).ok) return (size_t)2 * logits->n * logits->h * logits->w * logits->c * sizeof(float);      // interval form: FA | FB
  if (fused_plan(g, ce_label_bytes(CE_HARD)).lds > FUSED_MAX_LDS) return 0;
  return (size_t)logits->n * H * logits->w * logits->c * sizeof(float);
}

// The unweighted and the weighted entry points (CrossEntropyLoss(weight) / ImageBasedCrossEntropyLoss2d, loss.py:20-43,71-88,120-180): same kernels, same routing
// between them, same field layout. Weighted block partials are (sum w nll, sum w), image-major.
extern "C" int pm_upsample_ce_fwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out, void* ws, size_t ws_bytes,
                                  void* stream) {
  return ce_fwd("upsample_ce_fwd", CE_HARD, logits, inv_temp, labels, H, W, nullptr, false, loss_out, nullptr, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pm_upsample_wce_fwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* weights, int64_t weight_stride,
                                   int per_image, float* loss_out, void* ws, size_t ws_bytes, void* stream) {
  const CEWeights wt{weights, weight_stride, per_image};
  return ce_fwd("upsample_wce_fwd", CE_WEIGHTED, logits, inv_temp, labels, H, W, &wt, false, loss_out, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

// Training forward (the logits carry a graph): the loss and the field the row pass needs, in one sweep over the labels.
extern "C" int pm_upsample_ce_fwd_field(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out, float* field,
                                        void* ws, size_t ws_bytes, void* stream) {
  return ce_fwd("upsample_ce_fwd_field", CE_HARD, logits, inv_temp, labels, H, W, nullptr, true, loss_out, field, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pm_upsample_wce_fwd_field(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* weights, int64_t weight_stride,
                                         int per_image, float* loss_out, float* field, void* ws, size_t ws_bytes, void* stream) {
  const CEWeights wt{weights, weight_stride, per_image};
  return ce_fwd("upsample_wce_fwd_field", CE_WEIGHTED, logits, inv_temp, labels, H, W, &wt, true, loss_out, field, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pm_upsample_ce_bwd_field(const pm_tensor* logits, float inv_temp, int H, int W, const float* loss_out, const float* gscale, const float* field,
                                        const pm_tensor* dlogits, void* stream) {
  return ce_bwd_field("upsample_ce_bwd_field", logits, inv_temp, H, W, nullptr, loss_out, gscale, field, dlogits, (hipStream_t)stream);
}
extern "C" int pm_upsample_wce_bwd_field(const pm_tensor* logits, float inv_temp, int H, int W, int per_image, const float* loss_out, const float* gscale,
                                         const float* field, const pm_tensor* dlogits, void* stream) {
  const CEWeights wt{nullptr, 0, per_image};
  return ce_bwd_field("upsample_wce_bwd_field", logits, inv_temp, H, W, &wt, loss_out, gscale, field, dlogits, (hipStream_t)stream);
}

// Backward without a field from the forward (the caller ran pm_upsample_ce_fwd): the field is rebuilt into the workspace by the same fused sweep
// (its loss partials are discarded), then the row pass. Same results as pm_upsample_ce_fwd_field + pm_upsample_ce_bwd_field.
extern "C" size_t pm_upsample_ce_bwd_workspace(const pm_tensor* logits, int H, int W) {
  if ((logits && !pm_is_f32(logits))) return 0;      // fp32 tensors only
  return pm_align_up(pm_upsample_ce_field_bytes(logits, H, W), 256) + pm_upsample_ce_workspace(logits->n, H, W);
}

extern "C" int pm_upsample_ce_bwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* loss_out, const float* gscale,
                                  const pm_tensor* dlogits, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE_F32(logits, "upsample_ce_bwd");
  PM_REQUIRE_F32(dlogits, "upsample_ce_bwd");
  CEGeom g;
  if (int e = fill(g, "upsample_ce_bwd", CE_HARD, logits, inv_temp, labels, H, W)) return e;
  PM_REQUIRE(loss_out && dlogits && dlogits->ptr && pm_same_shape(logits, dlogits), PM_EINVAL, "upsample_ce_bwd: bad args");
  PM_REQUIRE(ws && ws_bytes >= pm_upsample_ce_bwd_workspace(logits, H, W), PM_EWORKSPACE, "upsample_ce_bwd: workspace too small");
  float* field = (float*)ws;
  float* part = (float*)((char*)ws + pm_align_up(pm_upsample_ce_field_bytes(logits, H, W), 256));
  if (int e = ce_run("upsample_ce_bwd", g, CE_HARD, true, nullptr, field, part, (hipStream_t)stream)) return e;      // no loss_out: the partials are not folded
  return pm_upsample_ce_bwd_field(logits, inv_temp, H, W, loss_out, gscale, field, dlogits, stream);
}


// ---- validation sweep: loss + predicted class + confusion matrix of the up-sampled logits (train.py:847-939 per batch: Upsample -> criterion -> max(1)[1] -> fast_hist) ---
// The row-staged forward with two more products per pixel. Block = EVAL rows-per-block consecutive hi-res rows of one image: rows that share a low-res row pair stage it
// once, and when the walk moves one low-res row down the lower staged row becomes the upper one (pointer swap) and only one row is staged. Nothing in the result depends
// on how rows are dealt to blocks: the interpolation is per pixel, the loss partial is per HI-RES ROW (reduced over its columns in the fixed order of
// ce_fwd_rows_kernel: lane X, X + 256, ..., wave sum, four waves), and the counts are integers. Counts: C x C unsigned LDS counters per block through LDS integer adds,
// one count row per block in the workspace, folded by integer adds into the int64 histogram (the label_count_kernel / label_weights_kernel pattern).
namespace {
constexpr int EVAL_MAX_ROWS = 8;                   // hi-res rows per block, at most
constexpr size_t EVAL_MAX_LDS = 159 * 1024;        // dynamic part (two staged rows + the counters); the kernel also declares 256 B of static LDS

struct EvalPlan {
  bool ok;
  int rows, chunks;      // hi-res rows per block, blocks per image
  size_t lds, part_bytes, bytes;
};
inline EvalPlan eval_plan(int n, int h, int w, int C, int H, int W) {
  EvalPlan p{};
  if (n < 1 || h < 1 || w < 1 || C < 1 || C > MAXC || H < 1 || W < 1) return p;
  p.lds = ((size_t)2 * w * (C | 1) + (size_t)C * C) * sizeof(float);
  if (p.lds > EVAL_MAX_LDS || (long)n * H > (1l << 22)) return p;
  // about as many rows as share one low-res pair, fewer while that leaves under two blocks per CU of the largest part (256 CUs)
  p.rows = std::max(1, std::min(EVAL_MAX_ROWS, (H + h - 1) / h));
  while (p.rows > 1 && (long)n * ((H + p.rows - 1) / p.rows) < 512) --p.rows;
  p.chunks = (H + p.rows - 1) / p.rows;
  p.part_bytes = pm_align_up((size_t)n * H * 2 * sizeof(float), 256);
  p.bytes = p.part_bytes + pm_align_up((size_t)n * p.chunks * C * C * sizeof(unsigned), 256);
  p.ok = true;
  return p;
}

__device__ __forceinline__ void eval_stage_row(const CEGeom& g, int C, int CP, int b, int y, float* dst) {
  const float* src = g.logits + ((long)(b * g.h + y) * g.w) * g.lp;
  for (int i = threadIdx.x; i < g.w * C; i += 256) {
    const int xl = i / C, c = i - xl * C;
    dst[xl * CP + c] = src[(long)xl * g.lp + c] * g.inv_temp;
  }
}

template <int C_>
__global__ __launch_bounds__(256) void ce_eval_rows_kernel(const CEGeom g, int rows, int chunks, float* __restrict__ part, unsigned* __restrict__ counts,
                                                           uint8_t* __restrict__ pred) {
  extern __shared__ float L[];
  __shared__ float sm[EVAL_MAX_ROWS][2][4];
  const int C = C_ > 0 ? C_ : g.C;
  const int CP = C | 1;
  const int bid = pm_xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / chunks, Y0 = (bid - b * chunks) * rows, Y1 = min(g.H, Y0 + rows);
  float* L0 = L;
  float* L1 = L + (size_t)g.w * CP;
  unsigned* cnt = reinterpret_cast<unsigned*>(L + (size_t)2 * g.w * CP);
  for (int i = threadIdx.x; i < C * C; i += 256) cnt[i] = 0u;      // visible after the first row's staging barrier
  int s0 = -1, s1 = -1;      // the low-res rows in L0, L1
  for (int Y = Y0; Y < Y1; ++Y) {
    const pm_lerp ly = pm_ac_lerp(g.sy, Y, g.h);
    const int64_t* lrow = ce_words<HardForm<false>>(g) + ((long)b * g.H + Y) * g.W;
    int64_t labs[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) labs[u] = (int)threadIdx.x + 256 * u < g.W ? lrow[threadIdx.x + 256 * u] : 255;   // in flight while the rows are staged
    if (ly.i0 != s0 || ly.i1 != s1) {      // uniform over the block
      __syncthreads();                     // every lane has finished the previous row's reads
      if (ly.i0 == s1) {                   // one low-res row down: the lower row becomes the upper one
        float* t = L0;
        L0 = L1, L1 = t;
        s0 = s1, s1 = -1;
      }
      if (ly.i0 != s0) eval_stage_row(g, C, CP, b, ly.i0, L0), s0 = ly.i0;
      if (ly.i1 != s1) eval_stage_row(g, C, CP, b, ly.i1, L1), s1 = ly.i1;
      __syncthreads();
    }
    uint8_t* prow = pred ? pred + ((long)b * g.H + Y) * g.W : nullptr;
    float lsum = 0.f, lcnt = 0.f;
    for (int X = threadIdx.x, u = 0; X < g.W; X += 256, ++u) {
      const int64_t lab = u < 3 ? (u == 0 ? labs[0] : (u == 1 ? labs[1] : labs[2])) : lrow[X];
      if (lab == 255 && !prow) continue;
      float v[C_ > 0 ? C_ : MAXC], mx, vl;
      int arg;
      ce_pixel_logits<C_, true>(ly, pm_ac_lerp(g.sx, X, g.w), L0, L1, 0, CP, C, lab, v, mx, vl, arg);
      if (prow) prow[X] = (uint8_t)arg;           // every pixel, ignored ones included
      if (lab == 255) continue;
      HardForm<false>::term<C_, CE_ROWS>(v, mx, vl, lab, nullptr, C, true, lsum, lcnt);
      if (lab >= 0 && lab < C) atomicAdd(&cnt[(int)lab * C + arg], 1u);      // fast_hist's mask (utils/misc.py:65-70)
    }
    ce_wave_partials(lsum, lcnt, sm[Y - Y0]);
  }
  __syncthreads();
  if ((int)threadIdx.x < Y1 - Y0) {
    const float* s = &sm[threadIdx.x][0][0];
    const long r = (long)b * g.H + Y0 + threadIdx.x;
    part[r * 2] = s[0] + s[1] + s[2] + s[3];
    part[r * 2 + 1] = s[4] + s[5] + s[6] + s[7];
  }
  for (int i = threadIdx.x; i < C * C; i += 256) counts[(long)bid * C * C + i] = cnt[i];
}

template <int CC>
void eval_launch(const CEGeom& g, const EvalPlan& p, float* part, unsigned* counts, uint8_t* pred, hipStream_t st) {
  static pm_lds_optin optin;      // > 64 KB of dynamic LDS (rows wider than ~420 pixels x 19 classes: one Cityscapes image has 512) needs the opt-in
  (void)optin(reinterpret_cast<const void*>(&ce_eval_rows_kernel<CC>), (int)EVAL_MAX_LDS);
  hipLaunchKernelGGL(ce_eval_rows_kernel<CC>, dim3(g.n * p.chunks), dim3(256), p.lds, st, g, p.rows, p.chunks, part, counts, pred);
}
}  // namespace

extern "C" size_t pm_upsample_eval_workspace(const pm_tensor* logits, int H, int W) {
  if (!logits || !pm_is_f32(logits)) return 0;      // fp32 tensors only
  return eval_plan(logits->n, logits->h, logits->w, logits->c, H, W).bytes;      // 0: the two low-res rows + the counters do not fit LDS
}

extern "C" int pm_upsample_eval(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out, int64_t* hist, int accumulate,
                                uint8_t* pred, void* ws, size_t ws_bytes, void* stream) {
  PM_REQUIRE_F32(logits, "upsample_eval");
  CEGeom g;
  if (int e = fill(g, "upsample_eval", CE_HARD, logits, inv_temp, labels, H, W)) return e;
  PM_REQUIRE(loss_out && hist, PM_EINVAL, "upsample_eval: null loss_out / hist");
  PM_REQUIRE(accumulate == 0 || accumulate == 1, PM_EINVAL, "upsample_eval: accumulate %d is neither 0 nor 1", accumulate);
  const EvalPlan p = eval_plan(g.n, g.h, g.w, g.C, H, W);
  PM_REQUIRE(p.ok, PM_EUNSUPPORTED, "upsample_eval: logit rows of %d x %d classes do not fit LDS (or n x H = %d x %d rows > 2^22)", g.w, g.C, g.n, H);
  PM_REQUIRE(ws && ws_bytes >= p.bytes, PM_EWORKSPACE, "upsample_eval: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  unsigned* counts = (unsigned*)((char*)ws + p.part_bytes);
  ce_dispatch(g.C, CE_HARD, [&](auto cc, auto) { eval_launch<decltype(cc)::value>(g, p, part, counts, pred, st); });
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(CE_FINAL_T), 0, st, (const float*)part, g.n * H, loss_out);
  hipLaunchKernelGGL(pm_hist_fold_kernel, dim3((g.C * g.C + 31) / 32), dim3(PM_HIST_FOLD_T), 0, st, (const unsigned*)counts, g.n * p.chunks, g.C * g.C, accumulate, hist);
  return pm_check_launch("upsample_eval");
}


// ---- per-image class weights from the labels: ImageBasedCrossEntropyLoss2d.calculate_weights (loss.py:136-146) without the trip through the host ---------------------
// counts: LDS integer counters per block, one row of block counts per (image, block), folded by integer adds -- order-free, so deterministic. The weight expression is
// numpy's ((hist != 0) * ub * (1 - hist)) + 1 in double, product and sum rounded separately (no fma), then rounded to float.
namespace {
constexpr int LCW_BLOCKS = 64;      // count blocks per image, at most
constexpr int LCW_PIX = 4096;       // pixels per count block, at least
inline int lcw_blocks(long hw) { return (int)std::max<long>(1, std::min<long>(LCW_BLOCKS, (hw + LCW_PIX - 1) / LCW_PIX)); }

__global__ __launch_bounds__(256) void label_count_kernel(const int64_t* __restrict__ labels, long hw, int classes, unsigned* __restrict__ counts) {
  __shared__ unsigned cnt[MAXC];
  if (threadIdx.x < MAXC) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t* lab = labels + (long)blockIdx.y * hw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    const int64_t l = lab[i];
    if (l >= 0 && l < classes) atomicAdd(&cnt[(int)l], 1u);
  }
  __syncthreads();
  if (threadIdx.x < MAXC) counts[((long)blockIdx.y * gridDim.x + blockIdx.x) * MAXC + threadIdx.x] = cnt[threadIdx.x];
}

__device__ __forceinline__ double lcw_weight(double hist, double ub, int norm) {
#pragma clang fp contract(off)
  const double m = hist != 0.0 ? ub : 0.0;
  const double t = norm ? 1.0 / hist : 1.0 - hist;
  const double p = m * t;
  return p + 1.0;
}

// block = one output row b: 32 classes x 8 slices of the count blocks of image b (per_batch: of every image)
// bins: the counted entries the divisor sums over (classes; classes + 1 for border sets, whose ignore bit is counted and gets no weight); empty_one: a row without
// any count is all ones instead of NaN
__global__ __launch_bounds__(256) void label_weights_kernel(const unsigned* __restrict__ counts, int nblk, int n, int classes, int bins, int empty_one, double ub, int norm,
                                                            int per_batch, float* __restrict__ weights) {
  __shared__ unsigned long long tot[MAXC];
  const int b = blockIdx.x, c = threadIdx.x & (MAXC - 1), sl = threadIdx.x / MAXC;
  if (threadIdx.x < MAXC) tot[threadIdx.x] = 0ull;
  __syncthreads();
  const long r0 = per_batch ? 0 : (long)b * nblk, r1 = per_batch ? (long)n * nblk : (long)(b + 1) * nblk;
  unsigned long long a = 0ull;
  for (long r = r0 + sl; r < r1; r += 256 / MAXC) a += counts[r * MAXC + c];
  if (a) atomicAdd(&tot[c], a);
  __syncthreads();
  if ((int)threadIdx.x < classes) {
    unsigned long long all = 0ull;
    for (int k = 0; k < bins; ++k) all += tot[k];
    const double hist = (double)tot[threadIdx.x] / (double)all;      // 0 / 0 = NaN for an image without a countable pixel, as numpy
    weights[(long)b * classes + threadIdx.x] = empty_one && all == 0ull ? 1.f : (float)lcw_weight(hist, ub, norm);
  }
}
}  // namespace

extern "C" size_t pm_label_class_weights_workspace(int n) { return pm_align_up((size_t)std::max(n, 1) * LCW_BLOCKS * MAXC * sizeof(unsigned), 256); }

extern "C" int pm_label_class_weights(const int64_t* labels, int n, int H, int W, int classes, double upper_bound, int norm, int per_batch, float* weights, void* ws,
                                      size_t ws_bytes, void* stream) {
  PM_REQUIRE(labels && weights && n > 0 && H > 0 && W > 0, PM_EINVAL, "label_class_weights: null/empty");
  PM_REQUIRE(classes >= 1 && classes <= MAXC, PM_EUNSUPPORTED, "label_class_weights: classes %d not in 1..%d", classes, MAXC);
  PM_REQUIRE(n <= 65535, PM_EUNSUPPORTED, "label_class_weights: %d images > 65535", n);
  PM_REQUIRE(ws && ws_bytes >= pm_label_class_weights_workspace(n), PM_EWORKSPACE, "label_class_weights: workspace too small");
  const long hw = (long)H * W;
  const int nblk = lcw_blocks(hw);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(label_count_kernel, dim3(nblk, n), dim3(256), 0, st, labels, hw, classes, (unsigned*)ws);
  hipLaunchKernelGGL(label_weights_kernel, dim3(n), dim3(256), 0, st, (const unsigned*)ws, nblk, n, classes, classes, 0, upper_bound, norm != 0, per_batch != 0, weights);
  return pm_check_launch("label_class_weights");
}


// ---- relaxed-border training: RelaxedBoundaryLossToTensor (transforms/transforms.py:99-148) + ImgWtLossSoftNLL (loss.py:182-263) ---------------------------------
// The third label form of the pixel body. A pixel's target is a SET of classes -- one uint32, bit c = class c, bit C = the ignore class --: the classes of the
// (2 border + 1)^2 window around it, built on the device from the int64 labels (rx_border_kernel) or packed from the reference's uint8 multi-hot (rx_pack_kernel).
// With S the real classes of the set, k = |S|, p = softmax(z) and P_S = sum of p over S, the reference's max(p_c, P_S) is P_S for every c in S, so the pixel's term is
//   - W_S log P_S,  W_S = (sum of w_c over S) / k,        gradient  W_S (p_j - [j in S] p_j / P_S);
// k = 0 ignores the pixel. Image i: sum of terms / (valid_i + 1); batch: sum over images / n. Classes outside S contribute exactly nothing (the reference multiplies
// 0 by log p_c there: NaN once p_c underflows). The kernels are the CE ones with Form = SetForm (rx_term is the pixel's term; the set words are staged in LDS, four
// bytes a pixel, in the place of the label bytes): flat and row-staged forward, the PARTS field kernel, the per-image final fold and the row pass ce_bwd_cols_kernel.
namespace {
constexpr int RX_MAX_BORDER = 3;
constexpr int RX_COLS = 1024;          // label columns per block of the border kernel

// block = (hi-res row Y of image b, column chunk): the 2 border + 1 label rows around Y as class bytes in LDS (outside the image and every label that is no class: the
// ignore class), then the OR over the window. strict: a pixel whose own class is in the mask keeps its one-hot (cfg.STRICTBORDERCLASS).
__global__ __launch_bounds__(256) void rx_border_kernel(const int64_t* __restrict__ labels, int H, int W, int classes, int border, unsigned strict,
                                                        uint32_t* __restrict__ bits) {
  __shared__ unsigned char rows[2 * RX_MAX_BORDER + 1][RX_COLS + 2 * RX_MAX_BORDER];
  const int bid = pm_xcd_remap(blockIdx.x, gridDim.x);      // neighbouring rows (which share 2 border of their label rows) on one XCD's L2
  const int Y = bid % H, b = bid / H;
  const int X0 = (int)blockIdx.y * RX_COLS, ncol = min(RX_COLS, W - X0), span = ncol + 2 * border;
  for (int r = 0; r <= 2 * border; ++r) {
    const int yy = Y + r - border;
    for (int i = threadIdx.x; i < span; i += 256) {
      const int xx = X0 + i - border;
      int cls = classes;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const int l = ce_label_byte(labels[((long)b * H + yy) * W + xx]);
        if (l < classes) cls = l;
      }
      rows[r][i] = (unsigned char)cls;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncol; i += 256) {
    const unsigned own = rows[border][i + border];
    unsigned s = 0u;
    if ((strict >> own) & 1u) {
      s = 1u << own;
    } else {
      for (int r = 0; r <= 2 * border; ++r)
        for (int d = 0; d <= 2 * border; ++d) s |= 1u << rows[r][i + d];
    }
    bits[((long)b * H + Y) * W + X0 + i] = s;
  }
}

// uint8 multi-hot [n][planes][hw] (non-zero = set) -> the same words; blockIdx.y = image
__global__ __launch_bounds__(256) void rx_pack_kernel(const uint8_t* __restrict__ mh, long hw, int planes, uint32_t* __restrict__ bits) {
  const uint8_t* src = mh + (long)blockIdx.y * planes * hw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    unsigned s = 0u;
    for (int c = 0; c < planes; ++c) s |= src[(long)c * hw + i] ? 1u << c : 0u;
    bits[(long)blockIdx.y * hw + i] = s;
  }
}

// Pixels whose set holds class c, c = 0..31, in the count-row layout of label_count_kernel (label_weights_kernel folds them). A wave counts one class per ballot and
// keeps class c's count in lane c; integer adds only.
__global__ __launch_bounds__(256) void rx_count_kernel(const uint32_t* __restrict__ bits, long hw, unsigned* __restrict__ counts) {
  __shared__ unsigned cnt[MAXC];
  if (threadIdx.x < MAXC) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* src = bits + (long)blockIdx.y * hw;
  const int lane = threadIdx.x & 63;
  unsigned mine = 0u;
  for (long i0 = (long)blockIdx.x * 256; i0 < hw; i0 += (long)gridDim.x * 256) {      // uniform trip count: every lane votes in every ballot
    const long i = i0 + threadIdx.x;
    const unsigned s = i < hw ? src[i] : 0u;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const unsigned v = (unsigned)__popcll(__ballot((s >> c) & 1u));
      if (lane == c) mine += v;
    }
  }
  if (lane < MAXC && mine) atomicAdd(&cnt[lane], mine);
  __syncthreads();
  if (threadIdx.x < MAXC) counts[((long)blockIdx.y * gridDim.x + blockIdx.x) * MAXC + threadIdx.x] = cnt[threadIdx.x];
}

// The relaxed entry points take their logits as flat arguments: the same view as a pm_tensor
inline pm_tensor rx_view(const float* p, int n, int h, int w, int C, int64_t pitch) { return pm_tensor{const_cast<float*>(p), n, h, w, C, pitch, PM_F32, 0}; }
}  // namespace

extern "C" int pm_relax_border_bits(const int64_t* labels, int n, int H, int W, int classes, int border, uint32_t strict_mask, uint32_t* bits, void* stream) {
  PM_REQUIRE(labels && bits && n > 0 && H > 0 && W > 0, PM_EINVAL, "relax_border_bits: null/empty");
  PM_REQUIRE(classes >= 1 && classes <= RX_MAXC, PM_EUNSUPPORTED, "relax_border_bits: classes %d not in 1..%d", classes, RX_MAXC);
  PM_REQUIRE(border >= 0 && border <= RX_MAX_BORDER, PM_EUNSUPPORTED, "relax_border_bits: border %d not in 0..%d", border, RX_MAX_BORDER);
  const long chunks = ((long)W + RX_COLS - 1) / RX_COLS;
  PM_REQUIRE((long)n * H <= (1l << 30) && chunks <= 65535, PM_EUNSUPPORTED, "relax_border_bits: %d x %d rows of %d columns", n, H, W);
  hipLaunchKernelGGL(rx_border_kernel, dim3(n * H, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, labels, H, W, classes, border, strict_mask, bits);
  return pm_check_launch("relax_border_bits");
}

extern "C" int pm_multihot_to_bits(const uint8_t* multihot, int n, int planes, int H, int W, uint32_t* bits, void* stream) {
  PM_REQUIRE(multihot && bits && n > 0 && H > 0 && W > 0, PM_EINVAL, "multihot_to_bits: null/empty");
  PM_REQUIRE(planes >= 1 && planes <= 32, PM_EUNSUPPORTED, "multihot_to_bits: %d planes not in 1..32", planes);
  PM_REQUIRE(n <= 65535, PM_EUNSUPPORTED, "multihot_to_bits: %d images > 65535", n);
  const long hw = (long)H * W;
  hipLaunchKernelGGL(rx_pack_kernel, dim3(pm_grid_for(hw), n), dim3(256), 0, (hipStream_t)stream, multihot, hw, planes, bits);
  return pm_check_launch("multihot_to_bits");
}

extern "C" size_t pm_relax_class_weights_workspace(int n) { return pm_label_class_weights_workspace(n); }

extern "C" int pm_relax_class_weights(const uint32_t* bits, int n, int H, int W, int classes, double upper_bound, int norm, int per_batch, float* weights, void* ws,
                                      size_t ws_bytes, void* stream) {
  PM_REQUIRE(bits && weights && n > 0 && H > 0 && W > 0, PM_EINVAL, "relax_class_weights: null/empty");
  PM_REQUIRE(classes >= 1 && classes <= RX_MAXC, PM_EUNSUPPORTED, "relax_class_weights: classes %d not in 1..%d", classes, RX_MAXC);
  PM_REQUIRE(n <= 65535, PM_EUNSUPPORTED, "relax_class_weights: %d images > 65535", n);
  PM_REQUIRE(ws && ws_bytes >= pm_relax_class_weights_workspace(n), PM_EWORKSPACE, "relax_class_weights: workspace too small");
  const long hw = (long)H * W;
  const int nblk = lcw_blocks(hw);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rx_count_kernel, dim3(nblk, n), dim3(256), 0, st, bits, hw, (unsigned*)ws);
  hipLaunchKernelGGL(label_weights_kernel, dim3(n), dim3(256), 0, st, (const unsigned*)ws, nblk, n, classes, classes + 1, 1, upper_bound, norm != 0, per_batch != 0, weights);
  return pm_check_launch("relax_class_weights");
}

extern "C" size_t pm_upsample_relax_workspace(int n, int H, int W) { return ce_workspace(CE_SETS, n, H, W); }
extern "C" size_t pm_upsample_relax_loss_floats(int n) { return (size_t)2 + (size_t)2 * std::max(n, 0); }
extern "C" size_t pm_upsample_relax_field_bytes(int n, int h, int w, int C, int H, int W) {
  if (n < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 1 || C > RX_MAXC) return 0;
  CEGeom g{};
  g.n = n, g.h = h, g.w = w, g.H = H, g.W = W, g.C = C;
  if (fused_plan(g, ce_label_bytes(CE_SETS)).lds > FUSED_MAX_LDS || (long)n * H > (1l << 30)) return 0;
  return (size_t)n * H * w * C * sizeof(float);
}

extern "C" int pm_upsample_relax_fwd(const float* logits, int n, int h, int w, int C, int64_t pitch, float inv_temp, const uint32_t* bits, int H, int W,
                                     const float* weights, int64_t weight_stride, float* loss_out, void* ws, size_t ws_bytes, void* stream) {
  const pm_tensor lg = rx_view(logits, n, h, w, C, pitch);
  const CEWeights wt{weights, weight_stride, 1};
  return ce_fwd("upsample_relax_fwd", CE_SETS, &lg, inv_temp, bits, H, W, &wt, false, loss_out, nullptr, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pm_upsample_relax_fwd_field(const float* logits, int n, int h, int w, int C, int64_t pitch, float inv_temp, const uint32_t* bits, int H, int W,
                                           const float* weights, int64_t weight_stride, float* loss_out, float* field, void* ws, size_t ws_bytes, void* stream) {
  const pm_tensor lg = rx_view(logits, n, h, w, C, pitch);
  const CEWeights wt{weights, weight_stride, 1};
  return ce_fwd("upsample_relax_fwd_field", CE_SETS, &lg, inv_temp, bits, H, W, &wt, true, loss_out, field, ws, ws_bytes, (hipStream_t)stream);
}
// The row pass of ce_bwd_cols_kernel, every image divided by its own out[2 + n + i] (its weighted form reads the divisor of image i at [2 + i] of what it is given).
extern "C" int pm_upsample_relax_bwd_field(int n, int h, int w, int C, float inv_temp, int H, int W, const float* loss_out, const float* gscale, const float* field,
                                           float* dlogits, int64_t dpitch, void* stream) {
  CEGeom g;
  PM_REQUIRE(dlogits, PM_EINVAL, "upsample_relax_bwd_field: null dlogits");
  const pm_tensor dl = rx_view(dlogits, n, h, w, C, dpitch);
  if (int e = fill(g, "upsample_relax_bwd_field", CE_SETS, &dl, inv_temp, nullptr, H, W)) return e;
  PM_REQUIRE(loss_out && field, PM_EINVAL, "upsample_relax_bwd_field: null loss_out / field");
  PM_REQUIRE(pm_upsample_relax_field_bytes(n, h, w, C, H, W) != 0, PM_EUNSUPPORTED, "upsample_relax_bwd_field: no field for this shape");
  ce_row_pass(g, CE_SETS, field, loss_out + n, gscale, dlogits, (long)dpitch, (hipStream_t)stream);
  return pm_check_launch("upsample_relax_bwd_field");
}
