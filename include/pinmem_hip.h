/* pinmem_hip.h -- C ABI of libpinmem_hip.so: hand-written gfx950 (MI355X) kernels for the dense hot path of
 * Genie-Kim/PintheMemory (DeepLabV3+/V2 over ResNet, plus the categorical memory read/update).
 *
 * The reference is pure Python on stock torch ops: no FFI exists there. Each entry point below therefore names
 * the reference op sequence (file:line under /root/reference) it replaces; INTEGRATION.md shows the ctypes stub
 * that binds it. Conventions:
 *   - every pointer is a BORROWED device pointer (torch owns the memory); the library never allocates or frees
 *     tensor memory; scratch comes from the caller through (ws, ws_bytes);
 *   - activations are NHWC fp32: pixel-major rows of `c` channels, `pitch` floats between pixels
 *     (pitch >= c lets a kernel write into a channel slice of a wider concat buffer);
 *   - a call reads and writes channels [0, c) of each of the n*h*w pixels of a pm_tensor and NOTHING ELSE: not the other `pitch - c` lanes of a pixel, not
 *     the memory before the first pixel or behind the last one (a ragged last tile is masked, never rounded up). Two exceptions, both the caller's choice:
 *     an fp32 view with c % 4 != 0 and pitch == roundup4(c) owns its pad lanes -- the caller hands them over as zeros, a call may read them and may write
 *     zeros there; and PM_TF_ZERO_PAD64 (below) lets a bf16 convolution READ the zero lanes c .. roundup(c, 64) - 1. An input tensor or array is never written.
 *     A view an entry point cannot serve (no 16-byte rows where it has no element-wise form) is refused with a negative status before anything is launched;
 *     tests/test_tensor_views.py holds every entry point to this on views inside poisoned memory and lists the refusals;
 *   - conv weights are KRSC fp32 ([Cout][kh][kw][Cin] == a torch channels_last [Cout,Cin,kh,kw] tensor);
 *   - labels are int64 as the reference's callers provide them (transforms/transforms.py:95-97), 255 = ignore;
 *   - all work is enqueued on `stream` (a hipStream_t), no host synchronisation inside;
 *   - return value: 0 = PM_OK, negative = pm_status; pm_last_error() gives the message (thread-local). */
#ifndef PINMEM_HIP_H
#define PINMEM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pm_status { PM_OK = 0, PM_EINVAL = -1, PM_EWORKSPACE = -2, PM_ELAUNCH = -3, PM_EUNSUPPORTED = -4 } pm_status;

/* Element type of an activation tensor. PM_F32: BASELINE configs[1], the parity path (every entry point). PM_BF16: BASELINE configs[2], the bf16 tier --
 * activations and their gradients are STORED as bf16 between layers (round to nearest even), every reduction / statistic / accumulator stays fp32.
 * Entry points say which they take; all tensor arguments of one call share the type unless stated otherwise; anything else returns PM_EUNSUPPORTED. */
typedef enum pm_dtype { PM_F32 = 0, PM_BF16 = 1 } pm_dtype;
/* pm_tensor.flags */
#define PM_TF_ZERO_PAD64 1      /* caller's promise: channels c .. roundup(c, 64) - 1 of every pixel lie inside `pitch` and hold zeros (a bf16 convolution
                                   input whose channel count is not a multiple of 64 is then gathered in place instead of being copied to a padded buffer) */

typedef struct pm_tensor {      /* NHWC activation view */
  void* ptr;
  int32_t n, h, w, c;
  int64_t pitch;                /* ELEMENTS between consecutive pixels (>= c) */
  int32_t dtype;                /* pm_dtype */
  int32_t flags;                /* PM_TF_* */
} pm_tensor;

/* ABI version of this header (pm_version() returns the library's). The two structs below carry their own size as first member: an entry point that
 * receives a struct built against another header returns PM_EINVAL instead of reading past the caller's object (they grew in rounds 2 and 3).
 * 400 (round 4): pm_tensor carries dtype + flags (bf16 activation tier).
 * 410: pm_aug_image and the augmenting input edge (pm_augment_u8, pm_labels_u8_flip_to_i64); the size of that struct is an ARGUMENT of the calls that read it,
 * because the array lives in device memory where the library cannot look at a first member.
 * 420: pm_geo_image and the resampling input edge (pm_resample_tables, pm_resample_crop_u8), PM_RESAMPLE_MAX_TAPS.
 * 430: pm_label_table and the label-decoding input edge (pm_label_table_ids, pm_label_table_colors, pm_labels_decode_u8, pm_resample_crop_decode_u8).
 * 440: sliding-window evaluation (pm_sliding_eval, pm_sliding_eval_finish, pm_sliding_eval_workspace).
 * 450: the evaluation input edge (pm_resize_axis_tables, pm_eval_tiles_u8), PM_FILTER_*.
 * 460: per-image normalisation of the IBN trunks (pm_instnorm_workspace, pm_instnorm_fwd, pm_instnorm_bwd).
 * The ablation sweep (pm_label_splat, pm_class_sums_workspace, pm_class_sums, pm_mem_actmap) and the evaluation image dumps (pm_eval_dump) arrived WITHOUT a version step: the number tracks the layouts of the
 * structs above, those entry points take raw pointers and sizes only and no struct changed; a caller finds out whether a library has them by looking the symbols up. */
#define PM_ABI_VERSION 460

typedef struct pm_conv_params { /* nn.Conv2d geometry (square kernels/strides as used by the reference) */
  int32_t struct_size;          /* = sizeof(pm_conv_params) */
  int32_t kh, kw, stride, pad, dil;
  int32_t prec;                 /* 0: fp32 MFMA (exact fp32 chain, parity path, BASELINE configs[1]);
                                   1: fp32 tiles staged in LDS, rounded to bf16 per fragment for v_mfma_f32_32x32x16_bf16, fp32 accumulate and storage;
                                   2: BASELINE configs[2] -- operands converted to bf16 in HBM (one streaming pass) and bf16 tiles in LDS, fp32
                                      accumulate and storage; call sites the form does not cover (3-channel stem, 19-class heads, stride-2 data
                                      gradients, weight gradients) run as prec 1 */
  void* wino_v;                 /* optional caller-owned buffer for the Winograd-transformed input of this convolution (NULL: none).
                                   pm_conv_fwd writes it there instead of its workspace; pm_conv_bwd_weight then reads it instead of
                                   transforming x again. Size from pm_conv_winograd_v_bytes (0 = the layer does not take the route). */
  int64_t wino_v_bytes;
  void* wxf;                    /* optional caller-owned buffer for the TRANSFORMED FILTER pm_conv_fwd derives from w (NULL: none), size from
                                   pm_conv_wxf_bytes: the Winograd U = G w G^T of a layer on that route, or the bf16 copy of the weights with
                                   prec == 2. wxf_valid == 0: the call writes it there instead of its workspace; != 0: the call trusts the
                                   content and skips the transform -- for a caller that knows the weights are unchanged since the call that
                                   filled it (eval-mode forward of step t and training forward of step t + 1). */
  int64_t wxf_bytes;
  int32_t wxf_valid;
} pm_conv_params;

typedef struct pm_conv_epilogue { /* optional fused epilogue of pm_conv_fwd; all pointers may be NULL */
  int64_t struct_size;          /* = sizeof(pm_conv_epilogue) */
  const float* bias;            /* [Cout]  conv bias (deepv3plus.py:417,420,424) */
  const float* scale;           /* [Cout]  folded eval-mode BN: y = conv*scale + shift (mynn.py:8-14 in .eval()) */
  const float* shift;           /* [Cout] */
  const float* residual;        /* NHWC, same n,h,w,c AND dtype as y (a bf16 y takes a bf16 residual: cast the pointer); += (Resnet.py:207) */
  int64_t residual_pitch;       /* elements */
  int32_t relu;                 /* max(.,0) last (Resnet.py:216) */
  float* bn_partials;           /* optional (NULL: none): train-mode BatchNorm statistics of y produced by the epilogue itself -- per 32-row slab of the
                                   GEMM and per channel (mean, M2), float[ceil(pixels / 32)][Cout][2], two-pass inside the slab -- so that no
                                   separate pass re-reads y; merged by pm_bn_partials_finalize. Size from pm_conv_bn_partials_bytes
                                   (0 = this call does not take the route: Winograd, split-K, unaligned / narrow outputs). Needs relu == 0, no residual. */
  int64_t bn_partials_bytes;
} pm_conv_epilogue;

const char* pm_last_error(void);
int pm_version(void);

/* ---- K1/K2/K3 convolution, implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------------------------------
 * Replaces nn.Conv2d forward/backward at Resnet.py:145-150,195,404,453-457; deepv3plus.py:72-81,87,398-424;
 * deepv2.py:44-51,138-151; memory.py:75,104.  y: [n,ho,wo,cout], x: [n,h,w,cin], cin % 4 == 0.
 * dtypes: all PM_F32 = the parity path. The bf16 tier (BASELINE configs[2]) is entered by prec = 2 or by any PM_BF16 tensor: x / y / dy / dx / add may each be
 * bf16 (c % 8 == 0, pitch % 8 == 0) or fp32 (the image in, the class logits and their gradient out); weights, dw, dbias, bias / scale / shift stay fp32,
 * every product is accumulated in fp32 and rounded once on the way out. A bf16 input whose channel count is not a multiple of 64 is gathered in place
 * only with PM_TF_ZERO_PAD64, else it is copied to a zero-padded workspace buffer first.
 * Size queries: a query and the call it sizes resolve ONE plan (same tensors, parameters and routing state -> same route, same buffer layout), so an entry point
 * requires exactly the bytes pm_conv_workspace answers for it -- PM_EWORKSPACE with one byte less -- and writes nothing behind them. The other queries read the
 * same plan: what a caller may keep between calls (Winograd V, transformed filter) and whether the forward call can emit bn_partials. */
size_t pm_conv_workspace(const pm_tensor* x, const pm_tensor* y, const pm_conv_params* p, int which /*0 fwd,1 dgrad,2 wgrad*/);
size_t pm_conv_winograd_v_bytes(const pm_tensor* x, const pm_tensor* y, const pm_conv_params* p);
size_t pm_conv_wxf_bytes(const pm_tensor* x, const pm_tensor* y, const pm_conv_params* p);   /* 0: pm_conv_fwd keeps no transformed filter for this call */
/* the same for pm_conv_bwd_data on the bf16 tier: bytes of the rotated / transposed bf16 filter a stride-1 data gradient derives from w (0: none). The caller
 * passes the buffer in pm_conv_params.wxf / wxf_bytes / wxf_valid exactly as for pm_conv_fwd. */
size_t pm_conv_wxf_bytes_dgrad(const pm_tensor* dy, const pm_tensor* dx, const pm_conv_params* p);
/* bf16 tier: rewrite MANY kept bf16 filters (the buffers of pm_conv_wxf_bytes / _dgrad with prec == 2) from their fp32 weights in one or two launches, e.g.
 * right after the optimizer moved the weights -- the next pm_conv_fwd / pm_conv_bwd_data calls then arrive with wxf_valid = 1 and derive nothing (142 small
 * casts per training step otherwise). Layout written = the one those calls read: forward [cout][kh*kw][round64(cin)], dgrad (rotated / transposed)
 * [cin][kh*kw][round64(cout)] with tap t <- kh*kw-1-t; pad channels zero. wxf_bytes is checked against that size. */
typedef struct pm_wxf_job {
  const float* w;      /* KRSC fp32 weights [cout][kh][kw][cin] */
  void* wxf;           /* the kept buffer */
  int64_t wxf_bytes;
  int32_t cout, kh, kw, cin;
  int32_t dgrad;       /* 0: forward copy, 1: rotated / transposed copy of the data gradient */
  int32_t reserved;
} pm_wxf_job;
int pm_conv_wxf_refresh_bf16(const pm_wxf_job* jobs, int n, void* stream);
/* fp32 tier: the kept Winograd forward transforms (U = G g Gt, what pm_conv_fwd writes into wxf for the wide stride-1 3x3 layers) of all jobs in one launch per
 * 48 filters; kh = kw = 3, dgrad = 0, wxf_bytes = pm_conv_wxf_bytes of the call that owns the buffer (it tells F(4x4) from F(2x2)). Same values as the per-call
 * transform; replaces ~20 latency-bound launches per training step (network/deepv3plus.py:72-81,398-404; Resnet.py:195). */
int pm_conv_wxf_refresh_f32(const pm_wxf_job* jobs, int n, void* stream);
/* bytes of pm_conv_epilogue.bn_partials for this forward call, 0 if the call cannot emit them (then run pm_bn_stats* on y as before) */
size_t pm_conv_bn_partials_bytes(const pm_tensor* x, const pm_tensor* y, const pm_conv_params* p);
int pm_conv_fwd(const pm_tensor* x, const float* w_krsc, const pm_tensor* y, const pm_conv_params* p,
                const pm_conv_epilogue* ep, void* ws, size_t ws_bytes, void* stream);
/* dx = dgrad(dy) [+ add]: `add` (nullable, same shape as dx) fuses the sum with a second gradient path, e.g. the
 * identity/downsample branch of a Bottleneck (Resnet.py:207). */
int pm_conv_bwd_data(const pm_tensor* dy, const float* w_krsc, const pm_tensor* dx, const pm_conv_params* p,
                     const pm_tensor* add, void* ws, size_t ws_bytes, void* stream);
/* The same with a MASKED add: dx = dgrad(dy) + (bit ? add : 0). add_mask (NULL: exactly the call above) holds one byte per float4 channel group of dx, dense
 * [pixels][c / 4], bit e = element e of the group is added -- the bytes pm_bn_apply_mask leaves behind, so the skip gradient of a Bottleneck tail is passed on as
 * (incoming gradient, ReLU bytes) and its masked copy is never stored. fp32 tensors; same plan and workspace as the unmasked call (pm_conv_workspace(.., 1)).
 * Served where the call routes to the fp32 implicit-GEMM kernels (every stride-1 1x1 data gradient: streaming pointwise kernel, tile epilogue, split-K reduce);
 * a call that routes to Winograd, the stride-2 class kernels or the bf16 tier returns PM_EUNSUPPORTED -- the mask is never dropped. */
int pm_conv_bwd_data_masked(const pm_tensor* dy, const float* w_krsc, const pm_tensor* dx, const pm_conv_params* p,
                            const pm_tensor* add, const uint8_t* add_mask, void* ws, size_t ws_bytes, void* stream);
/* dw_krsc [Cout][kh][kw][Cin]; dbias [Cout] or NULL. Deterministic (split-K partials reduced in fixed order). */
int pm_conv_bwd_weight(const pm_tensor* x, const pm_tensor* dy, float* dw_krsc, float* dbias, const pm_conv_params* p,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- ROUTING (round 6): the library's ONLY mutable global state is one pm_routing value -- which kernel takes a call; never WHAT is computed (every route is parity-tested
 * against the same oracle). It is initialised when the library is loaded from exactly six environment variables (PM_WINO_FUSED, PM_CONV16, PM_C16W, PM_C16P, PM_WGRAD16,
 * PM_SPLIT: the defaults below), and the library reads no other environment, then or later. pm_routing_set replaces it as a whole: a
 * production caller sets it once before the first pm_conv_* call, or never, and the library is then re-entrant with an immutable kernel table. The pm_set_*
 * entry points further down are thin wrappers that change ONE field -- for kernel tests that must reach a specific kernel and same-box A/B runs. Contract for both: call from
 * one thread while no other thread is inside a pm_conv_* entry point; repeat size queries (pm_conv_workspace, pm_conv_wxf_bytes, ...) after a change. */
typedef struct pm_routing {
  int32_t struct_size;        /* = sizeof(pm_routing): guards against a caller built with another header */
  int32_t winograd;           /* fp32 tier, wide stride-1 3x3s: 4 prefer F(4x4,3x3) (default), 2 F(2x2,3x3) only, 0 direct */
  int32_t winograd_fused;     /* F(4x4) point products + output transform in one kernel: 0 (default; PM_WINO_FUSED), 1 */
  int32_t conv16;             /* bf16 tier, forward / stride-1 data gradient: 1 per shape (default; PM_CONV16), 2 LDS-DMA kernels everywhere, 0 register-staged everywhere */
  int32_t conv16_wide;        /* the wide LDS-DMA forms (conv16w.hip): 1 by the planner's cost model (default; PM_C16W), 0 never, 2 wherever the shape allows, 3 = 2 with the 256 x 256 tile */
  int32_t conv16_persistent;  /* the ring tiles run as the persistent producer / consumer kernel: 1 (default; PM_C16P), 0 one block per tile */
  int32_t wgrad16;            /* bf16 tier, weight gradient on the LDS-DMA persistent ring (wgrad16.hip): 1 (default; PM_WGRAD16), 0 register-staged */
  int32_t bf16_wgrad;         /* prec = 2 weight gradients on pixel-contiguous bf16 copies: 0 (default), 1 */
  int32_t split;              /* fp32 tier on the bf16 matrix pipe (conv_split.hip: fp32 operands, 3-way exact bf16 split, 6 products, fp32 accumulate): 1 (default; PM_SPLIT), 0 */
} pm_routing;
int pm_routing_get(pm_routing* out);            /* out->struct_size must be set by the caller */
int pm_routing_set(const pm_routing* r);

/* ---- single-field wrappers over pm_routing (kernel tests, A/B runs) -------------------------------------------------------------------------------------------------------
 * pm_set_winograd, pm_set_winograd_fused, pm_set_conv16, pm_set_wgrad16, pm_set_split, pm_set_bf16_wgrad and pm_profile_enable flip process-wide ROUTING / MEASUREMENT switches. They exist for
 * same-box A/B runs, kernel tests that must reach a specific kernel, and bench.py's roofline leg; they never change WHAT is computed (every route is parity-tested
 * against the same oracle), only which kernel computes it or whether launches are timed. Contract: call them from ONE thread while no other thread is inside a
 * pm_conv_* entry point (the switches are plain ints read at plan time: a concurrent flip is a benign race between two valid routes for an in-flight PLAN, but the
 * workspace size a caller asked for with the old setting may not fit the new route -> PM_EWORKSPACE, never a wrong result); size queries (pm_conv_workspace,
 * pm_conv_wxf_bytes, ...) must be repeated after a flip (pinthememory_amd/hip/kernels.py keys its size cache on a generation counter for that).
 * A production caller leaves all of them at their defaults and the library is then re-entrant with an immutable kernel table, as the boundary contract says. ------- */

/* Wide stride-1 3x3 convolutions with pad == dilation (Resnet.py:195 conv2 of layer2/3/4, deepv3plus.py:72-81 ASPP branches,
 * :398-404 final1, :455 dsn) run as Winograd convolutions in fp32: F(4x4,3x3) (4x fewer MFMA FLOPs) where the image tiles by
 * 4*dilation, else F(2x2,3x3) (2.25x fewer), else direct. Results stay within fp32 rounding of an fp64 convolution (max error
 * ~3e-6 of the output scale for F(4x4), ~4e-7 for F(2x2); the direct MFMA chain: ~5e-7).
 * mode: 0 = direct implicit GEMM everywhere, 2 = F(2x2) only, 4 = prefer F(4x4) (default). */
int pm_set_winograd(int mode);
/* F(4x4) layers: the 36 point GEMMs and the output transform in ONE kernel, so that the products M = V U^T never reach HBM (one block = 32 tiles x
 * 32 channels x all 36 points). Same results to fp32 round-off; measured slower than GEMM + output-transform pass on every flagship layer
 * (DESIGN.md section 7), hence off by default: 0 off, 1 on. Process-wide like pm_set_winograd. */
int pm_set_winograd_fused(int on);
/* bf16 tier, forward and stride-1 data gradient: which kernel takes a call. 1 (default) = per shape: the LDS-DMA kernel (csrc/conv16.hip: global_load_lds
 * staging, swizzled LDS image) on 64-row tiles and single-K-step reductions, the register-staged kernel of rounds 2-3 on 128 x 128 tiles; 2 = LDS-DMA everywhere;
 * 0 = register-staged everywhere (A/B runs and tests). Round 5: the wide form of the LDS-DMA kernel (csrc/conv16w.hip: 256 x 128 / 128 x 256 tile, eight waves, one block
 * per CU, three-stage LDS ring with counted waits) is part of "per shape" (the planner's cost model decides); 2 = LDS-DMA everywhere on the NARROW tiles only,
 * 3 = LDS-DMA everywhere with the wide tile wherever the shape allows it (kernel tests: the PERSISTENT ring -- one block per CU walks the tiles, four producer waves
 * fetch ahead across tile boundaries, eight waves multiply; 7 = the same with the 256 x 256 two-stage form, 8 = the ring with one block per tile), 4 = per shape
 * without the wide kernel (A/B). PM_C16P=0 in the environment keeps the ring out of "per shape" and runs it one block per tile. The HBM-bound 1x1 convolutions
 * with K = 64 / 128 / 256 had a streaming kernel of their own in round 5 (measured level with the tile kernel, never the default): it left the library in round 6
 * (tools/experiments/pw16/); modes 5 and 6 are accepted and mean 1.
 * Process-wide like pm_set_winograd. */
int pm_set_conv16(int on);
/* prec = 2 weight gradients on pixel-contiguous bf16 copies of x (one per tap) and dy instead of the staged-fp32 form: 0 off (default: the
 * copies cost more HBM time than the GEMM saves), 1 on. Process-wide like pm_set_winograd. */
int pm_set_bf16_wgrad(int on);
/* bf16 tier, weight gradient with both operands bf16 (nn.Conv2d backward of Resnet.py / deepv3plus.py on bf16 rows): 1 (default) = the LDS-DMA persistent ring of
 * csrc/wgrad16.hip wherever Cin is a multiple of 128 and Cout >= 128 (one block per CU walks (256 x 128 tile, pixel range) units, producer waves fetch ahead, fragments
 * through the transpose read), 0 = the register-staged implicit-GEMM kernel everywhere (A/B runs, kernel tests). Same split-K slabs, same fixed-order reduce.
 * Process-wide like pm_set_winograd; PM_WGRAD16=0 in the environment sets the default. */
int pm_set_wgrad16(int on);
/* fp32 tier (round 6): which fp32 convolution / Winograd-GEMM launches run on the bf16 matrix pipe -- fp32 operands, every element split exactly into three bf16
 * pieces inside the kernel (hi + mid + lo == x), six cross products on v_mfma_f32_32x32x16_bf16, fp32 accumulation, fp32 results (csrc/conv_split.hip; replaces the
 * nn.Conv2d of Resnet.py:145-150 / deepv3plus.py:72-81,397-414 like the fp32-MFMA kernel it stands in for). 1 (default; PM_SPLIT in the environment) = every eligible
 * launch (output tiles >= 64 columns wide; forward / data-gradient reductions of >= 129, batched Winograd products of any length), 0 = v_mfma_f32_32x32x2_f32 everywhere
 * (A/B runs, accuracy tests). Same results to fp32 round-off (tests/test_hip_kernels.py::test_split_path_accuracy_vs_fp64). Process-wide like pm_set_winograd. */
int pm_set_split(int on);

/* In-library HIP-event timing of the implicit-GEMM kernel (bench.py's roofline leg). While enabled every conv launch is
 * bracketed by two events on its stream; pm_profile_read sums duration and algorithmic FLOPs (2*M*N*K) of one
 * instantiation conv_igemm_kernel<mode, bm, bn, .., km> (mode 0 fwd / 1 dgrad / 2 wgrad, block tile bm x bn, K-state variant
 * km 0 fast / 1 mid / 2 small, nst LDS stages 1 / 2; negative = any) and optionally clears the records. */
int pm_profile_enable(int on);
int pm_profile_dump(const char* csv_path);   /* one line per recorded launch: mode,bm,bn,km,nst,prec,M,N,K,batch,ksplit,ms,gflop */
int pm_profile_read(int mode, int bm, int bn, int km, int nst, double* total_ms, double* total_flops, int64_t* launches, int clear);
/* the same, additionally keyed by the operand form of the instantiation (prec 0 / 1 / 2 of pm_conv_params; negative = any) */
int pm_profile_read_prec(int mode, int bm, int bn, int km, int nst, int prec, double* total_ms, double* total_flops, int64_t* launches, int clear);
/* Sum of the ALGORITHMIC HBM bytes of the recorded launches of one implicit-GEMM instantiation (same keys, negative = any): both operands once + the output (every slab of a
 * split-K launch) -- the figure bench.py's roofline.traffic (PMC counters) is held against. Call before the pm_profile_read* that clears the records. */
int pm_profile_read_bytes(int mode, int bm, int bn, int km, int nst, int prec, double* total_bytes);

/* ---- K4 BatchNorm2d (mynn.py:8-14 -> nn.BatchNorm2d / SyncBatchNorm, eps 1e-5, momentum 0.1) -------------------
 * stats: per-channel shifted sums -> (count, mean, M2) so that ranks can be merged exactly (SyncBN, train.py:95).
 * moments layout: float[3*C] = mean[C] | m2[C] | count (replicated [C]). */
size_t pm_bn_workspace(const pm_tensor* x);
int pm_bn_stats(const pm_tensor* x, float* moments, void* ws, size_t ws_bytes, void* stream);
/* pm_bn_stats + pm_bn_finalize in one call for local (non-synchronised) statistics: same values, one launch less per BN layer.
 * PM_EINVAL for a single value per channel (torch: "Expected more than 1 value per channel when training"). */
int pm_bn_stats_finalize(const pm_tensor* x, float eps, float* mean, float* invstd, float* running_mean /*nullable*/, float* running_var /*nullable*/,
                         float momentum, void* ws, size_t ws_bytes, void* stream);
/* SyncBatchNorm (train.py:95): exact merge of the per-rank moments gathered over the process group, parts = float[world][3*C] */
int pm_bn_merge(const float* parts, int world, int c, float* moments, void* stream);
/* pm_bn_merge + pm_bn_finalize in one launch (the same values): SyncBatchNorm forward = stats, all-gather, this, apply */
int pm_bn_merge_finalize(const float* parts, int world, int c, float eps, float* mean, float* invstd, float* running_mean /*nullable*/,
                         float* running_var /*nullable*/, float momentum, void* stream);
/* mean/var(biased) -> invstd; optionally updates running stats (unbiased var), momentum as torch. */
int pm_bn_finalize(const float* moments, int c, float eps, float* mean, float* invstd,
                   float* running_mean, float* running_var, float momentum, void* stream);
/* y = relu?( (x-mean)*invstd*gamma + beta + residual? ) */
int pm_bn_apply(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                const pm_tensor* residual /*nullable*/, int relu, const pm_tensor* y, void* stream);
/* the same, and (mask != NULL) one byte per float4 channel group of y: bit e set <=> element e of the group is positive BEFORE the ReLU clamp, i.e. the
 * ReLU passes its gradient. Dense [pixels][c / 4] bytes whatever the pitches. pm_bn_bwd_reduce_mask then masks the incoming gradient from these bytes
 * instead of re-reading the forward output (BN + residual + ReLU, Resnet.py:207-216): 1 / 16 of the bytes. */
int pm_bn_apply_mask(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const pm_tensor* residual /*nullable*/, int relu, const pm_tensor* y, uint8_t* mask /*nullable*/, void* stream);
int pm_bn_bwd_reduce_mask(const pm_tensor* dy, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd,
                          const pm_tensor* gmask /*nullable*/, float* sums, void* ws, size_t ws_bytes, void* stream);
/* pm_bn_apply_mask whose residual is the BatchNorm output of a second raw tensor r (same shape), (r-r_mean)*r_invstd*r_gamma + r_beta, evaluated in the launch
 * with the arithmetic pm_bn_apply would have stored -- bit-identical to the two-launch form, and the normalised residual (the downsample branch of a stage's
 * first Bottleneck, Resnet.py:207-216) is never written. fp32 tensors only. */
int pm_bn_apply_mask_affine(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                            const pm_tensor* r, const float* r_mean, const float* r_invstd, const float* r_gamma, const float* r_beta,
                            int relu, const pm_tensor* y, uint8_t* mask /*nullable*/, void* stream);
/* pm_bn_bwd_apply (below) on dyz = dy masked by those bytes, for ANY x of the mask's shape with its own statistics: together with
 * pm_bn_bwd_reduce_mask(gmask = NULL) the backward of BN + residual + ReLU -- and of the downsample BatchNorm behind it -- without a stored masked gradient.
 * Bit-identical to pm_bn_bwd_apply(dy = gmask, relu = 0). fp32 tensors only. PM_EINVAL, before any launch, for a `sums` that is not 16-byte aligned. */
int pm_bn_bwd_apply_mask(const pm_tensor* dy, const uint8_t* mask, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                         const float* sums, float count, const pm_tensor* dx, void* stream);
/* backward: dyz = dy * mask, sums[2*C] = sum(dyz) | sum(dyz * xhat).  relu: 0 no activation (mask = 1); 1 mask = y > 0 read from the
 * forward output (BN + residual + ReLU, Resnet.py:207-216); 2 mask rebuilt from x with gamma / beta (BN + ReLU without a residual:
 * one tensor less to read).  gmask (nullable, relu != 0): dyz is also stored there -- it is the gradient of the residual branch, and
 * pm_bn_bwd_apply can then take it as `dy` with relu = 0 instead of re-reading dy and y. */
int pm_bn_bwd_reduce(const pm_tensor* dy, const pm_tensor* y /*relu == 1 only*/, const pm_tensor* x, const float* mean, const float* invstd,
                     const float* gamma /*relu == 2 only*/, const float* beta /*relu == 2 only*/, int relu, const pm_tensor* gmask /*nullable*/,
                     float* sums, void* ws, size_t ws_bytes, void* stream);
/* dx = gamma*invstd*(dyz - sum_dy/count - xhat*sum_dy_xhat/count); dres = dyz (nullable); count = global element count.
 * count <= 0: the count is read from the device at sums[2*C] (SyncBatchNorm all-reduces [sums | local count] in one exchange, so ranks
 * with uneven batches normalise by the true global count, as torch.nn.SyncBatchNorm does).
 * PM_EINVAL, before any launch, for a `sums` that is not 16-byte aligned (both dtypes): the pass reads it 16 bytes at a time. */
int pm_bn_bwd_apply(const pm_tensor* dy, const pm_tensor* y /*relu == 1 only*/, const pm_tensor* x, const float* mean, const float* invstd,
                    const float* gamma, const float* beta /*relu == 2 only*/, const float* sums, float count, int relu, const pm_tensor* dx,
                    const pm_tensor* dres /*nullable*/, void* stream);
/* eval-mode fold: scale = gamma/sqrt(running_var+eps); shift = beta - running_mean*scale + (conv_bias ? conv_bias*scale : 0) */
/* Chan merge (double, fixed order) of the (mean, M2) slab partials a convolution epilogue emitted for its own output (pm_conv_epilogue.bn_partials,
 * `pixels` rows in slabs of 32). moments == NULL: finalise like pm_bn_stats_finalize (mean, invstd, running moments); moments != NULL: write
 * mean[C] | M2[C] | count[C] for the SyncBatchNorm exchange instead (mean / invstd / running_* are ignored). */
int pm_bn_partials_finalize(const float* partials, int64_t pixels, int c, float eps, float* mean, float* invstd, float* running_mean /*nullable*/,
                            float* running_var /*nullable*/, float momentum, float* moments /*nullable*/, void* stream);
int pm_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, const float* conv_bias,
               int c, float eps, float* scale, float* shift, void* stream);
/* the same fold for n BatchNorm layers in one launch (eval-mode forward of a whole network): table = n x {gamma, beta, running_mean,
 * running_var} device pointers (uint64), cs[n] channel counts, offs[n] offsets into arena; scale_i = arena + offs[i], shift_i = arena + total + offs[i] */
int pm_bn_fold_multi(const void* table, const int* cs, const int* offs, int n, int max_c, int total, float eps, float* arena, void* stream);
/* eval-mode / frozen-stat backward helper and plain elementwise ops */
int pm_relu_bwd(const pm_tensor* dy, const pm_tensor* y, const pm_tensor* dx, void* stream);
int pm_add(const pm_tensor* a, const pm_tensor* b, const pm_tensor* y, void* stream);
/* y = xs[0] + ... + xs[n-1], 2 <= n <= 8, one pass (gradient accumulation of a multi-consumer tensor, e.g. the ASPP input,
 * deepv3plus.py:72-95: autograd would chain n-1 two-operand adds) */
int pm_add_n(const pm_tensor* const* xs, int n, const pm_tensor* y, void* stream);
int pm_copy(const pm_tensor* src, const pm_tensor* dst, void* stream);
int pm_scale_shift_act(const pm_tensor* x, const float* scale, const float* shift, const pm_tensor* residual, int relu,
                       const pm_tensor* y, void* stream);

/* ---- K4b InstanceNorm2d (Resnet.py:162-167,412-417: nn.InstanceNorm2d(C, affine = False / True), eps 1e-5) of the IBN trunks -------------------------------------
 * Per-(image, channel) statistics of an NHWC activation -- biased variance, no running moments, the same in train and eval mode -- as raw pointers plus
 * pitches (ELEMENTS between consecutive pixels; images are h * w pixels apart), dtype PM_F32 or PM_BF16 for every tensor of a call. Statistics are shifted sums
 * (shift = the first pixel of each image) in fp32 block partials, merged in double in a fixed order: no floating-point atomics, bit-identical from run to run. The
 * bf16 instantiation yields the mean / invstd the fp32 one yields on the widened tensor, bit for bit. Three launches per call whatever n is.
 *   fwd: y = (x - mean[n,c]) * invstd[n,c] * gamma[c] + beta[c], then max(., 0) if relu; mean / invstd: float[n][c] outputs. gamma and beta are both NULL
 *        (affine = False) or both set. y may be x itself (same pitch); any other overlap of y's elements with x's is undefined (not checked: channel slices of one
 *        slab interleave without overlapping).
 *   bwd: g = dy * [y > 0] if relu (y is read only then, and may be NULL otherwise); per (n, c) s1 = sum g, s2 = sum g * xhat;
 *        dx = gamma * invstd * (g - s1 / hw - xhat * s2 / hw); dgamma[c] = sum_n s2, dbeta[c] = sum_n s1 (fp32 [c], each nullable). gamma NULL: 1.
 *   ws:  pm_instnorm_workspace(n, h, w, c) bytes (the same for both passes and dtypes; 0 for a non-positive size).
 * Before anything touches the device -- PM_EINVAL: a null required pointer, a non-positive size, a pitch below c or not a multiple of the 16-byte vector width (4 fp32 /
 * 8 bf16 elements), a tensor or parameter pointer that is not 16-byte aligned, exactly one of gamma / beta, y aliasing x with another pitch.
 * PM_EUNSUPPORTED: an unknown dtype, c % 8 != 0. PM_EWORKSPACE: a workspace shorter than the query answers. */
size_t pm_instnorm_workspace(int n, int h, int w, int c);
int pm_instnorm_fwd(const void* x, void* y, int n, int h, int w, int c, int64_t x_pitch, int64_t y_pitch, int dtype, const float* gamma /*nullable*/,
                    const float* beta /*nullable*/, float eps, int relu, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream);
int pm_instnorm_bwd(const void* dy, const void* x, const void* y /*relu only*/, void* dx, int n, int h, int w, int c, int64_t dy_pitch, int64_t x_pitch, int64_t y_pitch,
                    int64_t dx_pitch, int dtype, const float* gamma /*nullable*/, const float* mean, const float* invstd, int relu, float* dgamma /*nullable*/,
                    float* dbeta /*nullable*/, void* ws, size_t ws_bytes, void* stream);

/* dtype conversion between two views of the same shape (PM_F32 <-> PM_BF16, round to nearest even): the edges of the bf16 tier -- the memory module
 * (memory.py:167-239) and the losses stay fp32. Only the c channels of a pixel are written (pad lanes of a wider pitch are left alone). */
int pm_cast(const pm_tensor* x, const pm_tensor* y, void* stream);

/* ---- K3 pooling (Resnet.py:432 MaxPool2d(3,2,1); deepv3plus.py:85 AdaptiveAvgPool2d(1)) ------------------------- */
int pm_maxpool3x3s2_fwd(const pm_tensor* x, const pm_tensor* y, uint8_t* argmax, void* stream);
int pm_maxpool3x3s2_bwd(const pm_tensor* dy, const uint8_t* argmax, const pm_tensor* dx, void* stream);
/* The stem tail (Resnet.py:471-478: conv -> BN -> ReLU -> max pool) without its full-resolution activation and gradient; fp32, c % 4 == 0.
 * Forward: pm_maxpool3x3s2_fwd of relu(bn(x)), x the raw convolution output -- each tap is normalised and clamped before the comparison, so y and argmax (ties
 * among clamped zeros included) are those of pooling the stored activation.
 * Backward: pm_bn_bwd_reduce / pm_bn_bwd_apply with relu = 2 whose incoming gradient is pm_maxpool3x3s2_bwd(dy_pooled, argmax), gathered per pixel inside the
 * pass instead of read from a tensor. Bit-identical to the separate kernels; workspace of pm_bn_workspace(x); count as pm_bn_bwd_apply.
 * pm_bn_bwd_apply_pool: PM_EINVAL, before any launch, for a `sums` that is not 16-byte aligned. */
int pm_maxpool3x3s2_bn_relu_fwd(const pm_tensor* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const pm_tensor* y,
                                uint8_t* argmax, void* stream);
int pm_bn_bwd_reduce_pool(const pm_tensor* dy_pooled, const uint8_t* argmax, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, float* sums, void* ws, size_t ws_bytes, void* stream);
int pm_bn_bwd_apply_pool(const pm_tensor* dy_pooled, const uint8_t* argmax, const pm_tensor* x, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, const float* sums, float count, const pm_tensor* dx, void* stream);
int pm_global_avgpool_fwd(const pm_tensor* x, const pm_tensor* y /*n,1,1,c*/, void* stream);
int pm_global_avgpool_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* stream);

/* ---- K5 bilinear resize, align_corners=True (mynn.py:57-62), fp32 index math as ATen ---------------------------- */
int pm_resize_bilinear_fwd(const pm_tensor* x, const pm_tensor* y, void* stream);
int pm_resize_bilinear_bwd(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* stream);
/* the same gradient as a column pass + a row pass through a [n, H, w, c] workspace: dy is read once (up-sampling ratio >= 2 both ways,
 * c % 4 == 0; pm_resize_bilinear_bwd_workspace returns 0 for shapes that must take the gather above) */
size_t pm_resize_bilinear_bwd_workspace(const pm_tensor* dy, const pm_tensor* dx);
int pm_resize_bilinear_bwd_separable(const pm_tensor* dy, const pm_tensor* dx, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- pooled multi-scale / flip evaluation (eval.py:133-145,277-337) -------------------------------------------------
 * half-pixel bilinear (F.interpolate(mode='bilinear') default, align_corners=False) of the logits to the original size;
 * MeanFusion: buffer += (softmax(logits) - buffer) / counter in float64 (buffer NHWC double); argmax over channels. */
int pm_resize_bilinear_hp_fwd(const pm_tensor* x, const pm_tensor* y, int flip_w, void* stream);
int pm_softmax_mean_update(const pm_tensor* logits, double* buffer, int counter, void* stream);
/* Sliding-window stitching (eval.py:210-274,340-405): logits [ntiles, th, tw, C] of the tiles (x1,y1,x2,y2)[ntiles] (HOST array) -> float64 sum over
 * the covering tiles (tile order) / tile count, written to acc[C][H][W] at the un-flipped column (flip_w); accumulate != 0 adds to acc. */
int pm_sliding_stitch(const pm_tensor* logits, const int32_t* tiles_xyxy, int ntiles, int H, int W, int flip_w, double* acc, int accumulate, void* stream);
int pm_argmax_f64(const double* buffer, int n, int h, int w, int c, int64_t* out_cls, double* out_prob /*nullable*/, void* stream);
/* Sliding-window evaluation of one (image, scale) from the heads' LOW-RES logits (eval.py:340-405 inference_sliding, :158-194 the tiles, :210-274 reverse_mapping /
 * reverse_sliding_window, :197-207 resize_thread). logits: [flips * ntiles][h][w] pixels of `pitch` >= C floats, the un-flipped tiles first, then those of the mirrored
 * image, both in table order. tiles_xyxy: HOST array of ntiles x (x1, y1, x2, y2) in the scaled image Hs x Ws, all of one size th x tw (th != tw allowed), together
 * covering every pixel; the library copies it into the workspace, so any number of tiles is taken and the array need not outlive the call. Per scaled-image pixel and
 * flip: the covering tiles, in table order, are up-sampled to th x tw (bilinear, align_corners=True, fp32: the arithmetic of pm_resize_bilinear_fwd), widened to double,
 * summed and divided by the cover count; the mirrored stack is read at column Ws - 1 - x (np.fliplr). Neither the up-sampled tiles nor the stitched map is written.
 *   acc == NULL (one scale; Hs == H, Ws == W): the pixel's value is (flip0 + flip1) / flips (np.mean(batch_return, axis=0)). pred (nullable, uint8 [H][W]): the LOWEST
 *     class among the maxima, as pm_upsample_eval. labels (nullable, int64 [H][W]): hist[label][pred] += 1 for 0 <= label < C (fast_hist, utils/misc.py:65-70),
 *     int64 [C][C], accumulate 0: overwritten, 1: added to; integer counts, deterministic; without labels hist is not touched. logits_out (nullable, float64
 *     [C][H][W]): the mean logits.
 *   acc != NULL (float64 [C][H][W]; labels, hist, pred and logits_out must be NULL): each flip's stitched map is resampled to H x W as cv2.resize(INTER_LINEAR) does
 *     for float64 -- per axis f = float((d + 0.5) * (double(S) / D) - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= S - 1: s = S - 1, one tap; float weights
 *     1.f - f and f; horizontal a * w0 + b * w1 in double, then vertical -- from at most four scaled-image pixels stitched on the fly. The mean over the flips is
 *     written to acc (acc_add 0, the first scale) or added to it (1). pm_sliding_eval_finish then takes acc / nscales (np.mean over the scales, eval.py:647) to
 *     pred / hist / logits_out as above; logits_out may be acc itself.
 * ws: pm_sliding_eval_workspace(ntiles, C, H, W) bytes (the finish call: ntiles = 0). PM_EINVAL: null pointers, flips not 1 or 2, a tile outside Hs x Ws or of another
 * size than the first, an uncovered pixel; PM_EUNSUPPORTED: C > 32; PM_EWORKSPACE: too few bytes -- each before any launch. The cover check is host work of
 * O(ntiles log ntiles + cells) per call, cells between the tiles' distinct edges: (columns + 1) x (rows + 1) for a regular grid, at most (2 ntiles + 1)^2.
 * A 16-byte aligned `logits` with pitch % 4 == 0 (the heads' padded rows) is read with 16-byte loads; any other with 4-byte loads, about 2.6 times slower, same bits. */
size_t pm_sliding_eval_workspace(int ntiles, int C, int H, int W);
int pm_sliding_eval(const float* logits, int n, int h, int w, int C, int64_t pitch, int flips, const int32_t* tiles_xyxy, int ntiles, int Hs, int Ws, int H, int W,
                    const int64_t* labels /*nullable*/, int64_t* hist, int accumulate, uint8_t* pred /*nullable*/, double* logits_out /*nullable*/,
                    double* acc /*nullable*/, int acc_add, void* ws, size_t ws_bytes, void* stream);
int pm_sliding_eval_finish(const double* acc, int C, int H, int W, int nscales, const int64_t* labels /*nullable*/, int64_t* hist, int accumulate,
                           uint8_t* pred /*nullable*/, double* logits_out /*nullable*/, void* ws, size_t ws_bytes, void* stream);

/* ---- evaluation image dumps (eval.py:664-693 RunEval.inf under --dump_images; csrc/eval_dump.hip) -----------------------------------------------------------------
 * The four images the reference writes per evaluated image, from the uint8 class map the evaluation kernels leave on the device (pm_sliding_eval's pred), in one
 * streaming pass over pixels = n * H * W dense pixels; no geometry, no workspace, no atomics: the same bytes from run to run. All pointers are device memory.
 *   color   uint8 [pixels][3] = palette[pred] (colorize_mask; palette: uint8 [256][3] RGB, all 256 rows are read -- the library ships no colour table).
 *   compose uint8 [pixels][3] = Image.blend(image, color, alpha) per colour channel with PIL's bytes, (uint8)((float)i + alpha * (float)(c - i)) in fp32, truncated
 *           (pm_mem_actmap's blend); image: uint8 [pixels][3]. The reference's alpha is 0.5; an alpha outside [0, 1] clips as PIL does.
 *   diff    uint8 [pixels][3] = ImageChops.lighter(compose, invert(diff mask)): the compose pixel where labels != 255 and labels != pred, else (255, 255, 255).
 *           labels: int64 [pixels] train ids; a value that is neither a class nor 255 counts as a difference, as in the reference.
 *   ids     uint8 [pixels] = id_table[pred] (the reference's loop over id_to_trainid; id_table: uint8 [256]).
 * The alpha channel of the reference's RGBA images is constantly 255 and is not written. Each output is nullable, any non-empty subset; an input is read only where a
 * requested output needs it. A thread moves 4 pixels as aligned dwords; a pred or ids pointer that is not 4-byte aligned sends the call to the one-pixel path
 * (same bytes, slower).
 * Before any launch -- PM_EINVAL: null pred, pixels <= 0, no output, color / compose / diff without palette, compose / diff without image, diff without labels, ids
 * without id_table, a non-finite alpha, image / color / compose / diff not 4-byte aligned, labels not 8-byte aligned. */
int pm_eval_dump(const uint8_t* pred, int64_t pixels, const uint8_t* palette /*[256][3], nullable*/, const uint8_t* image /*[pixels][3], nullable*/,
                 const int64_t* labels /*nullable*/, const uint8_t* id_table /*[256], nullable*/, float alpha, uint8_t* color /*nullable*/, uint8_t* compose /*nullable*/,
                 uint8_t* diff /*nullable*/, uint8_t* ids /*nullable*/, void* stream);

/* ---- ablation sweep (ablation.py:292-399 RunAbla.tsne_memact, tsnelib.py:48-74 RunTsne.input2basket; csrc/ablation.hip) ------------------------------------------
 * The per-class feature sums behind the t-SNE prototypes and the memory activation maps, from LOW-RES tensors: neither the up-sampled feature map ([256][H][W]) nor the
 * one-hot of the labels ([H W][20]) nor the up-sampled scores are written. Raw pointers, sizes, pitches in ELEMENTS; bilinear arithmetic = align_corners=True with the
 * coordinates and weights of pm_resize_bilinear_fwd. No floating-point atomics: bit-identical from run to run, independent of the grid.
 *   pm_label_splat: labels int64 [n][H][W] -> splat float [n][h][w][classes + 1] and counts int64 [n][classes + 1]. Label 255 goes to row `classes` (tsnelib.py:54
 *     gt[gt == 255] = num_class), a value in 0 .. classes - 1 to its own row, ANY OTHER value is skipped as pm_upsample_eval skips it (the reference's F.one_hot raises
 *     there). splat[n][i][j][k] = sum over the full-res pixels of row k of the weight with which low-res pixel (i, j) enters that pixel's interpolation (the labels
 *     pushed through the transpose of the up-sampling; a gather per low-res cell over its support, in a fixed order); counts = exact pixel counts. classes <= 31.
 *   pm_class_sums: feat NHWC [n][h][w] pixels of c channels (PM_F32 / PM_BF16, feat_pitch elements between pixels), splat as above -> sums float [n][classes + 1][c],
 *     sums[n][k][:] = sum over low-res pixels q of splat[n][q][k] * feat[n][q][:] / max(|feat[n][q][:]|_2, 1e-12) (F.normalize(dim=1); the norm in fp32 after widening)
 *     -- what tsnelib.py:51-65 computes as matmul(upsample(normalize(feat)), one_hot), because the up-sampling is linear. sums[k] / counts[k] is the class mean vector.
 *     Chunks of 32 pixels -> partials in ws (pm_class_sums_workspace bytes; 0 for a non-positive size) -> merged in chunk order in double. c % 8 == 0; pitch and
 *     alignment rules of pm_instnorm_fwd. One splat serves any number of feature maps of the same size (the sweep has two).
 *   pm_mem_actmap: p_mem float [n][h][w] rows of `pitch` >= m floats, the soft-max over the m memory slots (pm_mem_read_fwd's p_mem); slots: HOST array of nslots slot
 *     indices (copied into the launch). Per full-res pixel: all m slots interpolated, lo / hi = min / max over the m slots (ablation.py:309-315 channelwise_minmax, which
 *     is per PIXEL over the slots despite its name), and per listed slot e, a = (v - lo) / (hi - lo), byte = (uint8)(min(max(a, 0), 1) * 255.f) truncated in fp32
 *     (np.uint8(np.clip(., 0, 1) * 255), :386-389). hi == lo: the reference divides 0 by 0 and converts NaN to an undefined byte; HERE a = 0 and the byte is 0.
 *     Outputs, each nullable, any subset (at least one): act float [n][nslots][H][W] = a; bytes uint8 [n][nslots][H][W]; rgb uint8 [n][nslots][H][W][3] =
 *     palette[byte] (palette: uint8 [256][3] RGB in device memory -- the library ships no colour table); blend uint8 [n][nslots][H][W][3] = Image.blend(image, rgb, alpha)
 *     per colour channel with PIL's bytes (image: uint8 [n][H][W][3]; the alpha channel of the reference's RGBA blend is constantly 255 and is not written). Slot order
 *     is the list's. m <= 32, 1 <= nslots <= m.
 * Before any launch -- PM_EINVAL: a null required pointer, a non-positive size, a bad pitch or alignment, a slot outside 0 .. m - 1, nslots outside 1 .. m, no output, rgb
 * without palette, blend without palette or image. PM_EUNSUPPORTED: an unknown dtype, c % 8 != 0, classes > 31, m > 32. PM_EWORKSPACE: a workspace shorter than the query
 * answers. */
int pm_label_splat(const int64_t* labels, int n, int H, int W, int h, int w, int classes, float* splat, int64_t* counts, void* stream);
size_t pm_class_sums_workspace(int n, int h, int w, int c, int classes);
int pm_class_sums(const void* feat, int n, int h, int w, int c, int64_t feat_pitch, int dtype, const float* splat, int classes, float* sums, void* ws, size_t ws_bytes,
                  void* stream);
int pm_mem_actmap(const float* p_mem, int n, int h, int w, int m, int64_t pitch, int H, int W, const int32_t* slots, int nslots, float* act /*nullable*/,
                  uint8_t* bytes /*nullable*/, const uint8_t* palette /*nullable*/, const uint8_t* image /*nullable*/, float alpha, uint8_t* rgb /*nullable*/,
                  uint8_t* blend /*nullable*/, void* stream);

/* ---- input edge: ToTensor + Normalize(ImageNet) (datasets/gtav.py:284-289) and MaskToTensor
 * (transforms/transforms.py:95-97) on the GPU: uint8 HWC images -> normalised NHWC4 fp32 (zero 4th channel, the stem's layout),
 * uint8 label maps -> int64. Cuts the host->device traffic of a batch 4x (images) / 8x (labels). */
int pm_image_u8_to_nhwc4(const uint8_t* img_nhw3, int64_t pixels, const float* mean3, const float* std3, float* out_nhwc4, void* stream);
int pm_labels_u8_to_i64(const uint8_t* lab, int64_t n, int64_t* out, void* stream);

/* ---- augmenting input edge: what the training scripts run per image on the host before ToTensor (datasets/__init__.py:63-95 `--color_aug 0.5 --gblur`, :128-144 the
 * hard augmentation of the meta-test domains; transforms/transforms.py:179-187 RandomGaussianBlur; transforms/joint_transforms.py RandomHorizontallyFlip), on uint8
 * pixels in HBM, quantised to uint8 after every step as PIL / skimage do:
 *   colour: torchvision 0.10 ColorJitter on PIL -- ImageEnhance.Brightness / Contrast / Color = Image.blend(degenerate, image, factor) in float32 (truncating inside
 *     [0, 1], clipping outside) with degenerate = black / the rounded mean of convert("L") over the whole image in its state before the op / convert("L"); hue = PIL's
 *     RGB -> HSV, H += hue_shift mod 256, HSV -> RGB. The ops run in the image's own order; an op whose bit in `enabled` is clear is skipped.
 *   blur (radius > 0): skimage 0.16 gaussian(multichannel=True) = scipy correlate1d along H then W in float64 on x / 255.0, edges clamped, each output
 *     centre * w[0] + sum over j = radius .. 1 of (x[-j] + x[+j]) * w[j] (scipy's order, unfused), then (uint8)(y * 255).
 *   flip: image and label columns mirrored.
 * The colour bytes are PIL's; the blurred bytes are scipy's. Then ToTensor + Normalize with the arithmetic of pm_image_u8_to_nhwc4: an image with no op, radius 0 and
 * no flip gives that entry point's bytes. */
typedef struct pm_aug_image {   /* one per image, in DEVICE memory */
  uint8_t order[4];             /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue (torchvision's fn_idx); NOT checked on the device */
  uint8_t enabled;              /* bit i: op i runs */
  uint8_t flip;                 /* != 0: mirror the columns */
  uint8_t hue_shift;            /* (int)(hue_factor * 255) & 255 */
  uint8_t reserved;
  float brightness, contrast, saturation;      /* blend factors */
  int32_t radius;               /* 0: no blur; else 1 .. 5 (values outside are clamped on the device) */
  double w[6];                  /* blur weights: centre, then one side (pm_aug_blur_weights) */
} pm_aug_image;
/* host only: scipy.ndimage's Gaussian kernel for truncate = 4.0 -- radius = (int)(4 sigma + 0.5), w[k] = exp(-0.5 / sigma^2 * k^2) / sum over -radius .. radius, summed as
 * numpy's add.reduce does; w6[radius + 1 ..] = 0. sigma outside (0, 1.375) needs a radius beyond 5: PM_EUNSUPPORTED. */
int pm_aug_blur_weights(double sigma, int32_t* radius, double* w6);
size_t pm_augment_workspace(int n);      /* one exact integer grey sum per image */
/* img_nhw3 uint8 [n][H][W][3]; params_dev: n structs of struct_size = sizeof(pm_aug_image) bytes in device memory; out_nhwc4 float [n][H][W][4] (16-byte aligned, pad lane 0)
 * and / or out_u8 uint8 [n][H][W][3] (the augmented pixels before ToTensor): either may be NULL, not both; neither may alias img. Deterministic (integer atomics). */
int pm_augment_u8(const uint8_t* img_nhw3, int n, int H, int W, const pm_aug_image* params_dev, int32_t struct_size, const float* mean3, const float* std3,
                  float* out_nhwc4, uint8_t* out_u8, void* ws, size_t ws_bytes, void* stream);
/* pm_labels_u8_to_i64 with the columns of image i mirrored where params_dev[i].flip != 0 */
int pm_labels_u8_flip_to_i64(const uint8_t* lab, int n, int H, int W, const pm_aug_image* params_dev, int32_t struct_size, int64_t* out, void* stream);

/* ---- resampling input edge: joint_transforms.RandomSizeAndCrop (transforms/joint_transforms.py:414-444) with its RandomCrop (:61-141) on uint8 pixels in HBM, in
 * front of everything above: the whole image resized with PIL's antialiased bicubic (Image.resize(BICUBIC)) and the mask with Image.NEAREST, both padded where the result
 * is smaller than the crop (image 0, mask ignore_index), then one crop window taken. Only the window is computed: its pixels and their filter footprints.
 * The bytes are PIL's. Its 8-bit resampling is integer arithmetic (Resample.c): per axis and output position a first source index, a tap count and int32 coefficients
 * round(w * 2^22); one output byte of a pass = clip8(((1 << 21) + sum of pixel * k) >> 22), arithmetic shift; the horizontal pass runs first and is ROUNDED TO BYTES before
 * the vertical one. An axis whose size does not change is a copy (PIL skips the pass). NEAREST reads source index (int)xo with xo = a / 2 + a + a + ... accumulated in
 * double from output position 0 (Geometry.c), a = in / out: the closed form (int)(a * (x + 0.5)) is NOT the same pixels. */
#define PM_RESAMPLE_MAX_TAPS 24 /* taps per output position and axis the tables hold: enough for every in / out <= 5.75, which covers every scale in [0.25, 4] of every
                                   image (int() of the resized size makes in / out exceed 1 / scale; with >= 24 source pixels it stays below 4.8, with fewer the taps
                                   cannot outnumber the pixels) */
#define PM_RESAMPLE_REC (PM_RESAMPLE_MAX_TAPS + 2)      /* int32 per bicubic table record: first source index, tap count, coefficients (unused ones 0) */
typedef struct pm_geo_image {   /* the geometry of one image, in DEVICE memory for the kernel and in host memory for pm_resample_tables */
  int32_t h_in, w_in;           /* the image occupies the top-left h_in x w_in corner of its [Hs][Ws] slab: domains of different sizes share one batch */
  int32_t h, w;                 /* size after the resize: int(H * scale), int(W * scale) */
  int32_t pad_h, pad_w;         /* border added on BOTH sides of an axis shorter than the crop: (t - size) / 2 + 1 */
  int32_t y1, x1;               /* crop origin in padded coordinates: 0 <= y1 <= h + 2 pad_h - th */
} pm_geo_image;
/* host only, no device involved: the four tables pm_resample_crop_u8 reads for ONE image, for the th x tw crop window alone. bic_rows [th][PM_RESAMPLE_REC] and
 * bic_cols [tw][PM_RESAMPLE_REC]: per crop row / column the record above; a pad position has tap count 0, an axis with out == in one tap of 2^22. near_rows [th],
 * near_cols [tw]: the mask's source index, -1 on the pad. Evaluated in double without fused multiply-adds, as PIL's C is compiled. Hs, Ws: the slab the image lives in.
 * PM_EINVAL: a null pointer, another struct_size, an empty size, h_in > Hs or w_in > Ws, a crop that does not lie inside the padded image.
 * PM_EUNSUPPORTED: an output position needs more than PM_RESAMPLE_MAX_TAPS taps (what the tables hold then is unspecified). */
int pm_resample_tables(const pm_geo_image* geo_host, int32_t struct_size, int Hs, int Ws, int th, int tw, int32_t* bic_rows, int32_t* bic_cols, int32_t* near_rows,
                       int32_t* near_cols);
/* img uint8 [n][Hs][Ws][3], lab uint8 [n][Hs][Ws]; geo_dev: n structs of struct_size = sizeof(pm_geo_image) bytes in device memory; the four tables of every image in
 * device memory, image-major ([n][th][PM_RESAMPLE_REC], [n][tw][PM_RESAMPLE_REC], [n][th], [n][tw]), as pm_resample_tables wrote them. out_img uint8 [n][th][tw][3],
 * out_lab uint8 [n][th][tw] -- the layouts pm_augment_u8 / pm_labels_u8_flip_to_i64 take. No output may overlap an input. Slab bytes outside h_in x w_in and source
 * pixels outside the window's footprint are never read. Integer arithmetic, no atomics: the same bytes for every tiling and on every run. A table that did not come from
 * pm_resample_tables gives undefined bytes, but its indices are clamped to the image: no access outside the slabs. */
int pm_resample_crop_u8(const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo_dev, int32_t struct_size, const int32_t* bic_rows,
                        const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw, int ignore_index, uint8_t* out_img, uint8_t* out_lab,
                        void* stream);

/* ---- evaluation input edge: the scaled, mirrored, normalised crops of sliding-window evaluation, from the uint8 image on the device (csrc/resample.hip) ----------
 * host only, no device involved: PIL's coefficient records (above) of a WHOLE axis resized from `in` to `out`, rec [out][PM_RESAMPLE_REC]: what
 * img.resize((target_w, target_h), Image.BILINEAR) of eval.py:357-358 computes per axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc). PM_FILTER_BILINEAR:
 * bilinear_filter, support 1.0; PM_FILTER_BICUBIC: bicubic_filter, support 2.0 -- the un-padded records of pm_resample_tables; either support is stretched by
 * max(in / out, 1). in == out: one tap of 2^22 per position. PM_EINVAL: an empty size, a null pointer, an unknown filter. PM_EUNSUPPORTED: a position needs more than
 * PM_RESAMPLE_MAX_TAPS taps (bilinear: in / out > 11.5; what rec holds then is unspecified). */
#define PM_FILTER_BILINEAR 2      /* the values of PIL's Image.BILINEAR / Image.BICUBIC */
#define PM_FILTER_BICUBIC 3
int pm_resize_axis_tables(int in, int out, int filter, int32_t* rec);
/* One launch per (image, scale) for everything eval.py runs between the decoded image and the network: the resize of eval.py:357-358, the mirror image of :362-364
 * (transpose(FLIP_LEFT_RIGHT)), ToTensor + Normalize of :366-368 and the crops of sliding_window_cropping, :148-194. img uint8 [H][W][3]; rows_dev [Hs][PM_RESAMPLE_REC],
 * cols_dev [Ws][PM_RESAMPLE_REC]: the two axis tables of pm_resize_axis_tables (H -> Hs, W -> Ws) in device memory; tiles_xyxy_dev: ntiles x (x1, y1, x2, y2) int32 in
 * DEVICE memory, windows of the scaled image, all th x tw, which the CALLER has checked to lie inside [0, Ws] x [0, Hs] (the kernel reads x1, y1 alone and clamps them
 * into [0, Ws - tw] x [0, Hs - th]); mean3 / std3: host floats. out fp32 [flips * ntiles][th][tw][4], 16-byte aligned: pixel (y, x) of tile t holds the scaled image's
 * bytes at (y1 + y, x1 + x) -- PIL's: the pass along W rounded and clipped to bytes, then the pass along H -- normalised with the arithmetic of pm_image_u8_to_nhwc4
 * (channel 3 = 0); tile ntiles + t holds the mirrored image's window, the bytes at (y1 + y, Ws - 1 - (x1 + x)). Equal to pm_image_u8_to_nhwc4 of the scaled image (of its
 * mirror) sliced per tile, bit for bit; neither image is written to memory. Integer arithmetic up to the bytes, no atomics: the same bits on every run. A table that did
 * not come from pm_resize_axis_tables gives undefined pixels, but its indices are clamped to the image: no access outside img, and nothing is written outside out.
 * PM_EINVAL (each before any launch): a null pointer, an empty size, th > Hs or tw > Ws, flips not 1 or 2, out not 16-byte aligned or overlapping img or a table, a
 * table not 4-byte aligned. PM_EUNSUPPORTED: flips * ntiles > 65535; W / Ws so large (beyond about 6.8) that PM_RESAMPLE_MAX_TAPS source rows of a 64-column piece's
 * footprint do not fit the kernel's staging buffer. ntiles == 0: PM_OK, nothing launched. */
int pm_eval_tiles_u8(const uint8_t* img_hw3, int H, int W, const int32_t* rows_dev, const int32_t* cols_dev, int Hs, int Ws, const int32_t* tiles_xyxy_dev, int ntiles,
                     int th, int tw, int flips, const float* mean3, const float* std3, float* out, void* stream);

/* ---- label-decoding input edge: colour- and id-coded masks -> train ids on the device (csrc/resample.hip) ----------------------------------------------------------
 * The per-image host loops of the reference's datasets over their label dicts, as one table lookup per pixel; uint8 in, uint8 out, exact.
 *   PM_LABEL_COLORS {(r, g, b): v} (datasets/gtav.py:440-445): the output starts as `fill`; entries with v == 255 or v == -1 are dropped; a pixel equal to an entry's
 *     colour on all three channels gets (uint8) v; every other pixel keeps `fill`. A colour listed twice keeps its last kept value (a dict cannot hold one twice).
 *   PM_LABEL_IDS {k: v} (datasets/synthia.py:254-257, cityscapes.py): the output starts as the input id (channel 0); pixels whose ORIGINAL id equals k get (uint8) v
 *     (-1 becomes 255); assignments do not chain; keys outside 0..255 never match; a key listed twice keeps its last value.
 * The table is plain data: built on the host (no device involved, as pm_resample_tables), copied to device memory by the caller, read there. Colours sit in an
 * open-addressed hash of PM_LABEL_SLOTS slots, linear probing from slot ((r | g << 8 | b << 16) * 0x9E3779B1 mod 2^32) >> 24, an empty slot's key 0xFFFFFFFF; at most
 * PM_LABEL_MAX_COLORS kept entries, so a miss meets an empty slot after a short walk. */
#define PM_LABEL_SLOTS 256
#define PM_LABEL_MAX_COLORS 128
#define PM_LABEL_IDS 0
#define PM_LABEL_COLORS 1
typedef struct pm_label_table {       /* 1 544 bytes; an array of these lives in DEVICE memory, its struct size is an argument of the calls that read it */
  int32_t mode;                       /* PM_LABEL_IDS / PM_LABEL_COLORS */
  int32_t fill;                       /* colours: the value of a pixel whose colour the table does not hold (0..255) */
  uint8_t lut[256];                   /* ids: lut[id]; the identity for a colour table */
  uint32_t keys[PM_LABEL_SLOTS];      /* colours: r | g << 8 | b << 16, 0xFFFFFFFF = empty; all empty for an id table */
  uint8_t vals[PM_LABEL_SLOTS];       /* colours: the value of the slot's key */
} pm_label_table;
/* host only. keys / vals: `count` int32 pairs; rgb: `count` int32 triples. PM_EINVAL: a null pointer (count > 0 with null arrays, or a null table), another struct_size,
 * count < 0, fill outside 0..255. A colour with a channel outside 0..255 never matches, as a key outside 0..255. PM_EUNSUPPORTED: more than PM_LABEL_MAX_COLORS distinct kept colours (the table is then unspecified). */
int pm_label_table_ids(const int32_t* keys, const int32_t* vals, int count, pm_label_table* table, int32_t struct_size);
int pm_label_table_colors(const int32_t* rgb, const int32_t* vals, int count, int fill, pm_label_table* table, int32_t struct_size);
/* lab uint8 [n][H][W][lab_c], lab_c 1 or 3; tables_dev: ntables structs of struct_size = sizeof(pm_label_table) bytes in device memory; image_table_dev: n int32 in device
 * memory, -1 (any negative) = pass-through (channel 0 unchanged), otherwise an index the kernel clamps into [0, ntables); out uint8 [n][H][W], which may not overlap lab.
 * A colour table on a one-channel slab writes its `fill`. ntables == 0: tables_dev may be null and every image passes through. A table that did not come from the
 * builders gives unspecified bytes, but the probe walk is bounded by PM_LABEL_SLOTS and every index is clamped: no access outside the arrays, no unbounded loop. */
int pm_labels_decode_u8(const uint8_t* lab, int n, int H, int W, int lab_c, const pm_label_table* tables_dev, int ntables, int32_t struct_size,
                        const int32_t* image_table_dev, uint8_t* out, void* stream);
/* pm_resample_crop_u8 with the mask decoded in its gather: lab is uint8 [n][Hs][Ws][lab_c] read through the same nearest tables, each gathered pixel decoded as
 * pm_labels_decode_u8 decodes it, the pad written as ignore_index. A per-pixel map commutes with a gather, so out_lab carries the bytes of pm_labels_decode_u8 over the
 * whole slab followed by pm_resample_crop_u8, for the window's pixels alone; out_img carries pm_resample_crop_u8's bytes. Everything else as pm_resample_crop_u8. */
int pm_resample_crop_decode_u8(const uint8_t* img, const uint8_t* lab, int n, int Hs, int Ws, const pm_geo_image* geo_dev, int32_t struct_size, const int32_t* bic_rows,
                               const int32_t* bic_cols, const int32_t* near_rows, const int32_t* near_cols, int th, int tw, int ignore_index, int lab_c,
                               const pm_label_table* tables_dev, int ntables, int32_t struct_size_table, const int32_t* image_table_dev, uint8_t* out_img,
                               uint8_t* out_lab, void* stream);

/* ---- layout edges ------------------------------------------------------------------------------------------------ */
int pm_nchw_to_nhwc(const float* x_nchw, int c_src, const pm_tensor* y, void* stream);   /* zero-fills y.c > c_src */
int pm_nhwc_to_nchw(const pm_tensor* x, float* y_nchw, void* stream);
int pm_label_nearest(const int64_t* lab, int n, int H, int W, int64_t* out, int h, int w, void* stream); /* deepv3plus.py:592-594 */

/* ---- K6 fused bilinear-upsample(align_corners) + CrossEntropy(ignore_index=255, mean) ---------------------------
 * Replaces Upsample + criterion (deepv3plus.py:575-578) and the read loss (memory.py:173-176) without materialising
 * the [B,19,H,W] logits. logits: NHWC [n,h,w,C<=32]; labels int64 [n,H,W]. loss_out[0]=mean loss, [1]=valid count. */
size_t pm_upsample_ce_workspace(int n, int H, int W);
int pm_upsample_ce_fwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out,
                       void* ws, size_t ws_bytes, void* stream);
/* dlogits = gscale * d(mean CE)/dlogits ; gscale is a device scalar pointer (upstream grad), may be NULL (=1).
 * Two separable gather passes through a [n,H,w,C] fp32 workspace (no atomics, deterministic). */
size_t pm_upsample_ce_bwd_workspace(const pm_tensor* logits, int H, int W);
int pm_upsample_ce_bwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* loss_out,
                       const float* gscale, const pm_tensor* dlogits, void* ws, size_t ws_bytes, void* stream);

/* Training forward (the logits carry a graph): the same loss, and in the same sweep over the labels the column-reduced gradient field
 *   field[n][H][w][C] = sum over hi-res columns X of (softmax - onehot)(n, Y, X)[c] * (bilinear weight of X on low-res column x)
 * (float, pm_upsample_ce_field_bytes) -- everything the backward needs from labels and up-sampled logits; the upstream scale is a scalar applied
 * last. pm_upsample_ce_bwd_field is then the row pass alone: dlogits = gscale / valid * inv_temp * (field reduced over the supporting hi-res rows).
 * Labels and logits are read once per step instead of twice (replaces autograd through deepv3plus.py:575-578 / memory.py:173-176). */
size_t pm_upsample_ce_field_bytes(const pm_tensor* logits, int H, int W);
int pm_upsample_ce_fwd_field(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out, float* field,
                             void* ws /* pm_upsample_ce_workspace */, size_t ws_bytes, void* stream);
int pm_upsample_ce_bwd_field(const pm_tensor* logits /* shape only */, float inv_temp, int H, int W, const float* loss_out, const float* gscale,
                             const float* field, const pm_tensor* dlogits, void* stream);

/* Weighted forms of K6: CrossEntropyLoss(weight=...) (loss.py:20-43,71-88), CrossEntropyLoss2d (:167-180) and ImageBasedCrossEntropyLoss2d (:120-163), still
 * without the [B,C,H,W] logits. w = weights[b * weight_stride + label] (weight_stride 0: one [C] row for the whole batch); only labels in [0, C) contribute.
 *   per_image == 0: loss = sum w nll / sum w over the batch (nn.CrossEntropyLoss(weight));
 *   per_image == 1: loss = sum over images b, in index order, of (sum w nll)_b / (sum w)_b; an image whose weight sum is 0 makes it NaN, as nll_loss does.
 * loss_out holds pm_upsample_wce_loss_floats(n) floats: [0] loss, [1] total weight sum, [2 + b] weight sum of image b. The gradient field is the unweighted one
 * with every pixel's softmax - onehot multiplied by w: same layout and size (pm_upsample_ce_field_bytes). Backward scale per element:
 * gscale * inv_temp / (per_image ? loss_out[2 + b] : loss_out[1]). With all-ones weights and per_image == 0 loss_out[0..1], the field and dlogits carry the
 * bits of the unweighted entry points. Deterministic. */
size_t pm_upsample_wce_loss_floats(int n);
size_t pm_upsample_wce_workspace(int n, int H, int W);
int pm_upsample_wce_fwd(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* weights, int64_t weight_stride,
                        int per_image, float* loss_out, void* ws /* pm_upsample_wce_workspace */, size_t ws_bytes, void* stream);
int pm_upsample_wce_fwd_field(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, const float* weights, int64_t weight_stride,
                              int per_image, float* loss_out, float* field, void* ws /* pm_upsample_wce_workspace */, size_t ws_bytes, void* stream);
int pm_upsample_wce_bwd_field(const pm_tensor* logits /* shape only */, float inv_temp, int H, int W, int per_image, const float* loss_out,
                              const float* gscale, const float* field, const pm_tensor* dlogits, void* stream);

/* ImageBasedCrossEntropyLoss2d.calculate_weights (loss.py:136-146) on the device: weights[b][c] = ((hist != 0) * upper_bound * (1 - hist)) + 1 with
 * hist = count of label c in image b / count of labels in [0, classes) in image b, evaluated in double as numpy does (product and sum rounded separately) and
 * rounded to float -- bit-equal to the numpy expression. norm: 1 / hist instead of 1 - hist. per_batch: one histogram over all images, written to every row.
 * An image without a countable label gets a NaN row (0 / 0). labels int64 [n,H,W]; weights float [n][classes], classes <= 32. Integer counts: deterministic. */
size_t pm_label_class_weights_workspace(int n);
int pm_label_class_weights(const int64_t* labels, int n, int H, int W, int classes, double upper_bound, int norm, int per_batch, float* weights,
                           void* ws, size_t ws_bytes, void* stream);

/* Relaxed-border training (--jointwtborder): RelaxedBoundaryLossToTensor (transforms/transforms.py:99-148) and ImgWtLossSoftNLL (loss.py:182-263) without the
 * [n, C + 1, H, W] multi-hot target, the host histogram, the per-image host sync and the up-sampled logits. A pixel's target is a set of classes in one uint32: bit c =
 * class c < classes, bit `classes` = the ignore class; classes <= 31.
 *   pm_relax_border_bits: bits[b][Y][X] = OR over the (2 border + 1)^2 window of the one-hot of each neighbour's class; label 255, every other label outside
 *     [0, classes) and neighbours outside the image count as the ignore class; a pixel whose own class has its bit in strict_mask keeps its plain one-hot
 *     (cfg.STRICTBORDERCLASS). border 0..3 (0: the one-hot of the labels).
 *   pm_multihot_to_bits: the reference's uint8 target [n][planes = classes + 1][H][W] (non-zero = set) packed into the same words.
 *   pm_relax_class_weights: calculate_weights (loss.py:208-220): hist_c = pixels whose set holds c / set bits of the image (ignore bit included), c = 0..classes, then
 *     the expression of pm_label_class_weights in double, bit-equal to numpy; weights float [n][classes] (the ignore entry is dropped). per_batch: one histogram over
 *     all images in every row. An image without any set bit gets weights of 1.
 *   pm_upsample_relax_*: bilinear up-sampling (align_corners) of logits [n][h][w][C] (float, `pitch` floats between pixels, channels [0, C) read) fused with the loss.
 *     With S the real classes of a pixel's set, k = |S|, p = softmax(inv_temp z): term = - W_S log(sum of p over S), W_S = (sum over S of
 *     weights[b * weight_stride + c]) / k (weight_stride 0: one row for the batch); k = 0 ignores the pixel. loss_i = sum of terms / (valid_i + 1), loss = sum_i loss_i / n.
 *     loss_out holds pm_upsample_relax_loss_floats(n) = 2 + 2 n floats: [0] loss, [1] valid pixels of the batch, [2 + i] loss_i, [2 + n + i] (valid_i + 1) n.
 *     The field is T[n][H][w][C] of W_S (p - [c in S] p / P_S) reduced over the hi-res columns (pm_upsample_relax_field_bytes; 0: the rows do not fit LDS, the
 *     _fwd_field call then returns PM_EUNSUPPORTED while _fwd serves every shape); _bwd_field is the row pass: dlogits = gscale inv_temp / loss_out[2 + n + i] x (T
 *     reduced over the supporting hi-res rows), channels [0, C) of every pixel written, dpitch floats between pixels. No atomics on floats: deterministic. */
int pm_relax_border_bits(const int64_t* labels, int n, int H, int W, int classes, int border, uint32_t strict_mask, uint32_t* bits, void* stream);
int pm_multihot_to_bits(const uint8_t* multihot, int n, int planes, int H, int W, uint32_t* bits, void* stream);
size_t pm_relax_class_weights_workspace(int n);
int pm_relax_class_weights(const uint32_t* bits, int n, int H, int W, int classes, double upper_bound, int norm, int per_batch, float* weights, void* ws,
                           size_t ws_bytes, void* stream);
size_t pm_upsample_relax_workspace(int n, int H, int W);
size_t pm_upsample_relax_loss_floats(int n);
size_t pm_upsample_relax_field_bytes(int n, int h, int w, int C, int H, int W);
int pm_upsample_relax_fwd(const float* logits, int n, int h, int w, int C, int64_t pitch, float inv_temp, const uint32_t* bits, int H, int W, const float* weights,
                          int64_t weight_stride, float* loss_out, void* ws /* pm_upsample_relax_workspace */, size_t ws_bytes, void* stream);
int pm_upsample_relax_fwd_field(const float* logits, int n, int h, int w, int C, int64_t pitch, float inv_temp, const uint32_t* bits, int H, int W,
                                const float* weights, int64_t weight_stride, float* loss_out, float* field, void* ws /* pm_upsample_relax_workspace */,
                                size_t ws_bytes, void* stream);
int pm_upsample_relax_bwd_field(int n, int h, int w, int C, float inv_temp, int H, int W, const float* loss_out, const float* gscale /* nullable: 1 */,
                                const float* field, float* dlogits, int64_t dpitch, void* stream);

/* Validation sweep (train.py:847-939 per batch: Upsample -> criterion -> output.max(1)[1] -> fast_hist) in one pass over the labels, the up-sampled logits never
 * materialised. Inputs and loss_out as pm_upsample_ce_fwd (same interpolation expression, same fixed-order reduce). Per hi-res pixel: pred = the LOWEST class index
 * among the maxima of the interpolated logits; hist[label][pred] += 1 for 0 <= label < C (fast_hist's mask, utils/misc.py:65-70; 255 and any other value are
 * skipped); pred, when given, is written as one byte for EVERY pixel, ignored ones included. hist: int64 [C][C], row = label, column = prediction; accumulate 0:
 * overwritten, 1: added to (a whole validation epoch sums into one histogram without a host round trip). Integer counts and a fixed-order loss: deterministic, and
 * independent of how the rows are dealt to blocks. The workspace query answers 0 for a shape the kernel does not take (two low-res logit rows do not fit LDS: more than
 * ~1000 low-res columns at 19 classes), as pm_upsample_ce_field_bytes does; the call then returns PM_EUNSUPPORTED. */
size_t pm_upsample_eval_workspace(const pm_tensor* logits, int H, int W);
int pm_upsample_eval(const pm_tensor* logits, float inv_temp, const int64_t* labels, int H, int W, float* loss_out, int64_t* hist, int accumulate,
                     uint8_t* pred /* nullable, [n][H][W] */, void* ws, size_t ws_bytes, void* stream);

/* ---- K7 memory read (memory.py:317-336 + get_score :167-189) ---------------------------------------------------
 * x: [N rows of d=256] (NHWC feature map); mem [m<=32][d]; writes qr = [qhat | P_m.M] (2d channels, input of
 * memory.output), score S [N][m] (raw cosine scores), P_m [N][m] (softmax over slots, or gumbel if noise given). */
int pm_mem_read_fwd(const pm_tensor* x, const float* mem, int m, const float* gumbel_noise /*nullable [N][m]*/,
                    const pm_tensor* qr, float* score, float* p_mem, void* stream);
/* softmax over all N queries per slot (memory.py:186); two-pass column reduce, deterministic */
size_t pm_mem_colsoftmax_workspace(int64_t rows, int m);
int pm_mem_colsoftmax(const float* score, const float* noise /*nullable*/, int64_t rows, int m, float* p_query,
                      void* ws, size_t ws_bytes, void* stream);
/* read + softmax over all queries (memory.py:317-336 with get_score :183-189 complete) in two launches: the read kernel also leaves
 * per-tile column (max, sum exp) partials of score + noise_q, the second launch merges them in fixed order and writes p_query [N][m].
 * noise / noise_q: the two independent gumbel draws of F.gumbel_softmax(dim=1) / (dim=0); both nullable. */
size_t pm_mem_read_fwd_pq_workspace(int64_t rows, int m);
int pm_mem_read_fwd_pq(const pm_tensor* x, const float* mem, int m, const float* gumbel_noise, const float* gumbel_noise_q,
                       const pm_tensor* qr, float* score, float* p_mem, float* p_query, void* ws, size_t ws_bytes, void* stream);
/* backward into x (and into mem when dmem != NULL): dqr [N][2d], dscore_extra [N][m] (from the read loss; nullable) */
size_t pm_mem_read_bwd_workspace(int64_t rows, int m, int d);
int pm_mem_read_bwd(const pm_tensor* x, const float* mem, int m, const float* p_mem, const pm_tensor* dqr,
                    const float* dscore_extra, const pm_tensor* dx, float* dmem /*nullable [m][d]*/,
                    void* ws, size_t ws_bytes, void* stream);

/* ---- K8 memory write (memory.py:206-239) -----------------------------------------------------------------------
 * accum: zhat = z/max(|z|,1e-12); 4-tap bilinear(align_corners) soft labels of the H x W mask at each h x w pixel
 * (== one_hot(20) -> F.interpolate, memory.py:220-223, without the one-hot); nomden[(m+1)*(d+1)] =
 * nominator[m+1][d] | denominator[m+1], summed over batch and pixels. Deterministic two-stage reduce.
 * Workspace: one partial nomden per block of the accumulating kernel, align256(min(ceil(rows / 64), 512) * (m+1) * (d+1) * 4) with
 * rows = n*h*w; query, then allocate. 2^31 rows or more: PM_EUNSUPPORTED (the kernel divides row indices in 32 bits). */
size_t pm_mem_write_accum_workspace(const pm_tensor* z, int m);
int pm_mem_write_accum(const pm_tensor* z, const int64_t* labels, int H, int W, int m, int normalize,
                       float* nomden, void* ws, size_t ws_bytes, void* stream);
/* dz from dnom [m+1][d] (label weights are constants) through the row normalisation */
int pm_mem_write_accum_bwd(const pm_tensor* z, const int64_t* labels, int H, int W, int m, int normalize,
                           const float* dnom, const pm_tensor* dz, void* stream);
/* update: U = den!=0 ? mu*M + (1-mu)*nom/den : M ; M' = U/max(|U|,1e-12) (memory.py:233-239), device-side predicate */
int pm_mem_write_update(const float* mem, const float* nomden, int m, int d, float momentum, float* mem_out,
                        float* u_out /*nullable, saved for bwd*/, void* stream);
int pm_mem_write_update_bwd(const float* u, const float* nomden, int m, int d, float momentum, const float* dmem_out,
                            float* dnom /*[m+1][d]*/, float* dmem_in /*nullable [m][d]*/, void* stream);

/* ---- optimizer (optimizer.py:21-25: SGD momentum 0.9, wd 5e-4, no nesterov) on a flat parameter arena -------------- */
int pm_sgd_momentum(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                    float weight_decay, int first_step, void* stream);
/* The same update for EVERY parameter tensor (multi-tensor apply): `entries` is a HOST array of n records; the library passes them to
 * the device by value in the kernel arguments (32 records per launch), so nothing is copied or has to outlive the call. A fresh momentum buffer
 * is all zeros (round(m * 0) + d == d: torch's first step). Roundings are torch.optim.SGD's: d = fma(wd, p, g); buf = round(m * buf) + d;
 * p = fma(-lr, buf, p). Replaces torch.optim.SGD.step of optimizer.py:21-25 on the training step. */
typedef struct pm_sgd_entry {
  float* param;
  const float* grad;
  float* momentum_buffer;
  int64_t numel;
} pm_sgd_entry;
int pm_sgd_momentum_multi(const pm_sgd_entry* entries, int n, float lr, float momentum, float weight_decay, void* stream);
/* the same with the learning rate read from device memory when lr_dev != NULL (one float; `lr` is then ignored): a training step captured in a hipGraph follows
 * the LR schedule by a 4-byte write before each replay instead of a re-capture (harness.GraphedAggStep). */
int pm_sgd_momentum_multi_dev(const pm_sgd_entry* entries, int n, float lr, const float* lr_dev, float momentum, float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif
