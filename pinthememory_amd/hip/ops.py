"""Autograd-wrapped HIP ops. Tensors crossing these functions are LOGICAL NCHW (the reference's shapes) whose
memory is NHWC (`t.permute(0,2,3,1)` is a dense pixel-major view): every call site keeps the reference's shape
arithmetic (`x.size()[2:]`, `dim=1` channel slices) while every kernel sees coalesced channel vectors.
Weights enter as Function inputs (never cached pointers) so functional re-wiring of module._parameters works."""
import os as _os

import torch

from . import kernels as K
from . import lib as L
from .. import dist as D


def nhwc(t):
    """Logical-NCHW tensor -> NHWC view usable by the kernels (zero-copy when the memory is already channels-last,
    one transpose kernel when a caller hands over a true NCHW-contiguous tensor)."""
    v = t.permute(0, 2, 3, 1)
    n, h, w, c = v.shape
    sn, sh, sw, sc = v.stride()
    pitch = sw if w > 1 else (sh if h > 1 else (sn if n > 1 else c))
    ok = (sc == 1 or c == 1) and pitch >= c and (h == 1 or w == 1 or sh == w * pitch) and (n == 1 or h * w == 1 or sn == h * w * pitch)
    if ok and v.dtype == torch.float32:
        return v
    if v.dtype == torch.bfloat16:      # the bf16 tier's activations (K.ACT_DTYPE): 16-byte rows of eight channels
        if ok and pitch % 8 == 0 and c % 8 == 0 and v.data_ptr() % 16 == 0:
            return v
        return v.contiguous()
    if h * w == 1:
        return v.contiguous().float()
    return K.nchw_to_nhwc(t.float())


def nchw(v):
    return v.permute(0, 3, 1, 2)


def _grad_view(g):
    """Incoming gradient (logical NCHW, arbitrary strides) -> NHWC view with 16B-aligned rows."""
    v = nhwc(g)
    if v.stride(2) % (8 if v.dtype == torch.bfloat16 else 4) or v.data_ptr() % 16:
        v = v.contiguous()
    return v


class BNState:
    """What the BN part of a fused op needs besides gamma/beta: the module's buffers and mode."""
    __slots__ = ('running_mean', 'running_var', 'eps', 'momentum', 'training', 'group', 'grad_enabled')

    def __init__(self, bn):
        self.running_mean, self.running_var = bn.running_mean, bn.running_var
        self.eps = bn.eps
        self.momentum = 0.1 if bn.momentum is None else bn.momentum
        self.training = bn.training or bn.running_mean is None
        # nn.SyncBatchNorm (train.py:95 convert_sync_batchnorm) -> exchange statistics over RCCL
        self.group = D.bn_group(bn)
        self.grad_enabled = torch.is_grad_enabled()      # the caller's mode: inside autograd.Function.forward it always reads False
        if bn.training and bn.num_batches_tracked is not None:
            _nbt_pending.append(bn.num_batches_tracked)


# num_batches_tracked += 1 of every BN layer that ran in training mode: one multi-tensor launch per forward pass (flush_bn_counters,
# called where the networks' forward ends) instead of 65 single-element kernels.
_nbt_pending = []


def flush_bn_counters():
    if _nbt_pending:
        torch._foreach_add_(_nbt_pending, 1)
        _nbt_pending.clear()


# ---- weight-gradient overlap ------------------------------------------------------------------------------------------
# wgrad(L) only needs x(L) and dy(L); nothing on the backward critical path (bn_bwd(L-1) -> dgrad(L-1) -> ...) needs its result.
# It is launched on a side stream so that the HBM-bound BatchNorm-backward kernels and the tile-quantisation tails of the dgrad
# kernels run under its MFMA work.
# Safety: the weight enters the conv node through a `_Defer` identity node created at the START of its stage's forward, i.e. with
# a lower autograd sequence number than every node of that stage. The engine therefore runs `_Defer.backward` -- which makes the
# main stream wait for the side stream and only then hands the gradient on -- after the whole stage's backward has been
# launched: AccumulateGrad / DDP hooks / functional-weight graphs never see a gradient that is still being written.
# Round 5, second session: on the bf16 tier the weight gradients run INLINE by default. Their kernel there (csrc/wgrad16.hip) is persistent -- one block per CU with
# 144 KB of LDS -- so a second stream cannot share the chip with it any more and the fork / join only adds contention (same box, captured step: 24.72 side stream,
# 24.46 inline; eager: level). PM_OVERLAP_WGRAD=0 / 1 forces one form on both tiers; the attribute stays the master switch (bench.py's serialised leg, tests).
_OVERLAP_ENV = _os.environ.get('PM_OVERLAP_WGRAD')
OVERLAP_WGRAD = True if _OVERLAP_ENV is None else _OVERLAP_ENV == '1'


def overlap_wgrad():
    """Do the weight gradients of the pass being recorded go to the side stream?"""
    if not OVERLAP_WGRAD:
        return False
    return not (_OVERLAP_ENV is None and K.CONV_PREC == 2 and K.ACT_DTYPE == torch.bfloat16)


_side = {}
_proxy = {}            # id(weight tensor) -> deferred proxy, valid for the current forward only


def masked_stream(n_cus, device=None, first=0):
    """A HIP stream whose kernels may only run on `n_cus` of the 256 CUs (hipExtStreamCreateWithCUMask through ctypes on the process's libamdhip64, wrapped as a
    torch ExternalStream) -- VERDICT r3 item 2a: a side stream that owns a fixed CU set instead of alternating whole-GPU kernels with the main stream. The mask
    takes every (256 / n_cus)-th CU starting at `first`, so the set is spread evenly over the 8 XCDs / 32 shader engines."""
    import ctypes
    dev = torch.cuda.current_device() if device is None else device
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    n_cus = max(1, min(int(n_cus), total))
    words = (total + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    picked = {(first + (i * total) // n_cus) % total for i in range(n_cus)}
    for cu in picked:
        mask[cu // 32] |= 1 << (cu % 32)
    hip = ctypes.CDLL('libamdhip64.so')
    st = ctypes.c_void_p()
    with torch.cuda.device(dev):
        err = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), ctypes.c_uint32(words), mask)
    if err != 0 or not st.value:
        raise RuntimeError('hipExtStreamCreateWithCUMask(%d CUs) failed: %d' % (n_cus, err))
    return torch.cuda.ExternalStream(st.value, device=dev)


# PM_WGRAD_CUS=n: the weight-gradient side stream is confined to n CUs (A/B knob; default: an ordinary stream sharing all 256 with the main stream)
WGRAD_CUS = int(_os.environ.get('PM_WGRAD_CUS', '0'))


def _side_stream():
    dev = torch.cuda.current_device()
    if dev not in _side:
        _side[dev] = masked_stream(WGRAD_CUS, dev) if WGRAD_CUS > 0 else torch.cuda.Stream(device=dev)
    return _side[dev]


class _Defer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w):
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        L.stream_obj().wait_stream(_side_stream())
        return g


def begin_forward():
    flush_bn_counters()      # backstop for callers that drive sub-modules directly
    _proxy.clear()


def defer_weights(module):
    """Call right before running `module` (a stage of the network) in training mode with gradients enabled."""
    if not (overlap_wgrad() and torch.is_grad_enabled()):
        return
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d) and m.bias is None and m.weight.requires_grad and id(m.weight) not in _proxy:
            _proxy[id(m.weight)] = _Defer.apply(m.weight)


def _w(weight):
    """(tensor the conv node should take as its weight input, whether its wgrad may run asynchronously)"""
    p = _proxy.get(id(weight))
    return (p, True) if p is not None else (weight, False)


def _wgrad(x, dy, wshape, geom, want_bias=False, deferred=False, wino_v=None):
    if not deferred:
        return K.conv_bwd_weight(x, dy, wshape, *geom, want_bias=want_bias, wino_v=wino_v)
    # on the side stream, behind everything the main stream has enqueued so far; the launch takes the stream explicitly (no torch.cuda.stream() context: its
    # enter / exit cost 10 us per weight gradient on a host-bound step). Outputs are allocated by the main stream's pool and first written on the side stream.
    side, main = _side_stream(), L.stream_obj()
    ev = torch.cuda.Event()
    ev.record(main)
    side.wait_event(ev)
    out = K.conv_bwd_weight(x, dy, wshape, *geom, want_bias=want_bias, wino_v=wino_v, on_stream=side)
    if wino_v is not None:
        wino_v.record_stream(side)
    x.record_stream(side)
    dy.record_stream(side)
    for t in out:
        if t is not None:
            t.record_stream(side)
    return out


# harness.agg_train_step runs the memory-commit forward on its own stream; it READS every weight there. device index -> event recorded at its end.
# Whoever writes weights on another stream waits for it first (optim.SGD.step, checkpoint.restore_snapshot, harness.sync_commit).
commit_done = {}


def wait_commit():
    if not commit_done or not torch.cuda.is_available():
        return
    ev = commit_done.pop(torch.cuda.current_device(), None)
    if ev is not None:
        torch.cuda.current_stream().wait_event(ev)


def _same_exchange(groups, widths):
    """Do these BatchNorm layers share an exchange? Every one a SyncBatchNorm of the same process group (more than one rank, or forced collectives) and width."""
    return D.is_dist() and all(g is not None and g is groups[0] for g in groups) and len(set(widths)) == 1


def _bn_train_stats_multi(ys, bns, partials):
    """Batch statistics of independent BatchNorm layers -> [(mean, invstd)]; running moments updated in place.
    partials[i]: the (mean, M2) slab partials the producing convolution's epilogue emitted for ys[i] (K.conv_fwd(bn_partials=...)), or None: with them no kernel
    re-reads ys[i] for its statistics.
    Local statistics: one finalising launch per layer. SyncBatchNorm: local moments of each layer, ONE all-gather of their concatenation for layers that share an
    exchange (ASPP's five branches, a stage's first block's bn3 + downsample.1), one merge + finalise per layer -- per layer the arithmetic of a lone exchange (the
    merge kernel sees the same per-rank moments in the same rank order). Layers that cannot travel together are served one by one."""
    n = len(ys)
    if n > 1 and not _same_exchange([b.group for b in bns], [y.shape[3] for y in ys]):
        return [_bn_train_stats(y, bn, part) for y, bn, part in zip(ys, bns, partials)]
    pixels = [y.shape[0] * y.shape[1] * y.shape[2] for y in ys]
    if bns[0].group is None:
        y, bn, part = ys[0], bns[0], partials[0]
        if part is not None:
            return [K.bn_partials_finalize(part, pixels[0], y.shape[3], bn.eps, bn.running_mean, bn.running_var, bn.momentum)]
        return [K.bn_stats_finalize(y, bn.eps, bn.running_mean, bn.running_var, bn.momentum)]
    c = ys[0].shape[3]
    moms = [K.bn_partials_moments(part, px, c) if part is not None else K.bn_stats(y) for y, part, px in zip(ys, partials, pixels)]
    flat, world = D.gather_moments(moms[0] if n == 1 else torch.cat(moms), bns[0].group)      # SyncBN: stats, all-gather, merge + finalise, apply
    parts = flat.view(world, n, 3 * c)
    return [K.bn_merge_finalize(parts[:, i].contiguous().view(-1), world, c, bn.eps, bn.running_mean, bn.running_var, bn.momentum) for i, bn in enumerate(bns)]


def _bn_train_stats(y, bn, partials=None):
    """Batch statistics of y (merged across ranks for SyncBN) -> (mean, invstd): the one-layer case of _bn_train_stats_multi."""
    return _bn_train_stats_multi([y], [bn], [partials])[0]


def _bn_train_fwd(y, gamma, beta, bn, residual, relu, out=None, partials=None):
    """Batch statistics (_bn_train_stats) -> normalise + residual + ReLU. Returns (o, mean, invstd)."""
    mean, invstd = _bn_train_stats(y, bn, partials)
    return K.bn_apply(y, mean, invstd, gamma, beta, residual=residual, relu=relu, out=out), mean, invstd


class _BnSums:
    """The backward sums of n BatchNorm layers of width c that share an exchange: slot i = [sum dy | sum dy * xhat (| count)] of layer i, 2c (+ 1) floats. A BatchNorm
    backward is three phases over these slots --
      reduce:   K.bn_bwd_reduce / K.bn_bwd_reduce_mask / K.bn_bwd_reduce_pool(sums=slot(i)) writes layer i's local sums, and its count under SyncBatchNorm;
      exchange: ONE all-reduce over all slots (nothing without a process group). The global count travels with the sums (uneven batches);
      apply:    K.bn_bwd_apply / K.bn_bwd_apply_mask / K.bn_bwd_apply_pool(total(i), count(y)).
    dgamma / dbeta are THIS rank's sums (torch.nn.SyncBatchNorm returns the local grad_weight / grad_bias and lets DDP average them); only the input gradient needs
    the sums over all ranks. Slots start at multiples of 4 floats: the apply passes read them 16 bytes at a time."""

    def __init__(self, n, c, group, device):
        self.c, self.group, self.with_count = c, group, group is not None
        self.len = 2 * c + (1 if self.with_count else 0)
        self.stride = (self.len + 3) // 4 * 4
        self.local = torch.empty((n - 1) * self.stride + self.len, dtype=torch.float32, device=device)
        self.summed = self.local

    def slot(self, i):
        return self.local[i * self.stride:i * self.stride + self.len]

    def exchange(self):
        if self.group is not None:
            self.summed = D.all_reduce_sum_copy(self.local, self.group)      # out of place: the local sums are the parameter gradients

    def total(self, i):
        return self.summed[i * self.stride:i * self.stride + self.len]

    def count(self, y):
        """The count argument of the apply pass: the local element count, or -1 (on the device, behind the sums) under SyncBatchNorm."""
        return -1.0 if self.with_count else float(y.shape[0] * y.shape[1] * y.shape[2])

    def grads(self, i):
        """-> (dgamma, dbeta) of layer i"""
        s = self.slot(i)
        return s[self.c:2 * self.c], s[:self.c]


def _bn_train_bwd(dv, o, y, mean, invstd, gamma, beta, relu, group, want_dres, has_res, mask=None):
    """-> (dy, dres, dgamma, dbeta): gradient of the conv output, of the residual input, and of the affine parameters.
    ReLU mask: rebuilt from the conv output when no residual entered the activation (the forward output is not read at all);
    otherwise taken from the mask bytes (or the forward output) once, in the reduce pass, which then hands the masked gradient (= dres) to the apply pass."""
    mode = 0 if not relu else (1 if has_res else 2)
    hand_over = mode == 1 and want_dres
    S = _BnSums(1, y.shape[3], group, y.device)
    if hand_over and mask is not None:
        _, gm = K.bn_bwd_reduce_mask(dv, mask, y, mean, invstd, want_gmask=True, with_count=S.with_count, sums=S.slot(0))
    else:
        _, gm = K.bn_bwd_reduce(dv, o, y, mean, invstd, mode, gamma, beta, want_gmask=hand_over, with_count=S.with_count, sums=S.slot(0))
    S.exchange()
    if hand_over:
        dy, dres = K.bn_bwd_apply(gm, None, y, mean, invstd, gamma, S.total(0), S.count(y), 0, False)[0], gm
    else:
        dy, dres = K.bn_bwd_apply(dv, o, y, mean, invstd, gamma, S.total(0), S.count(y), mode, want_dres, beta)
    return (dy, dres, *S.grads(0))


def _bn_bwd_masked(dv, mask, y, mean, invstd, gamma, group):
    """-> (dy, dgamma, dbeta) of a BatchNorm whose output gradient is dv masked by `mask` (bn_apply(want_mask=True)'s bytes): what _bn_train_bwd computes from the
    stored masked gradient, without storing it. y / mean / invstd / gamma: the BatchNorm the mask came from, or the downsample BatchNorm behind the same ReLU. fp32."""
    S = _BnSums(1, y.shape[3], group, y.device)
    K.bn_bwd_reduce_mask(dv, mask, y, mean, invstd, want_gmask=False, with_count=S.with_count, sums=S.slot(0))
    S.exchange()
    return (K.bn_bwd_apply_mask(dv, mask, y, mean, invstd, gamma, S.total(0), S.count(y)), *S.grads(0))


class _Bottleneck(torch.autograd.Function):
    """One ResNet Bottleneck (Resnet.py:181-216) as a single autograd node in train mode: the gradient of the block input is
    produced by conv1's dgrad with the skip-path gradient fused in (`add`), so autograd never launches a separate add, and the
    16 blocks cost 16 nodes instead of ~60."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd, geoms, bns, deferred):
        xv = nhwc(x)
        k1, k2, k3 = K.krsc(w1), K.krsc(w2), K.krsc(w3)
        ps = []                                            # BatchNorm statistics handed out by the convolution epilogues (None: separate pass)
        y1 = K.conv_fwd(xv, k1, *geoms[0], bn_partials=ps)
        o1, m1, i1 = _bn_train_fwd(y1, g1, b1, bns[0], None, True, partials=ps[0])
        kv = []
        y2 = K.conv_fwd(o1, k2, *geoms[1], keep_v=kv, bn_partials=ps)      # Winograd layers keep the transformed input for the weight gradient
        o2, m2, i2 = _bn_train_fwd(y2, g2, b2, bns[1], None, True, partials=ps[1])
        y3 = K.conv_fwd(o2, k3, *geoms[2], bn_partials=ps)
        m3 = None
        if wd is not None:
            kd = K.krsc(wd)
            yd = K.conv_fwd(xv, kd, *geoms[3], bn_partials=ps)
            # fp32: the normalised downsample output is never stored -- bn3's apply pass evaluates it from yd (K.bn_apply_res_affine). The bf16 tier keeps its two launches.
            fold = y3.dtype == torch.float32 and yd.dtype == torch.float32
            if fold or _same_exchange([bns[3].group, bns[2].group], [yd.shape[3], y3.shape[3]]):
                # both statistics before either apply pass; under SyncBN the two independent exchanges of the block's tail travel as one
                (md, idd), (m3, i3) = _bn_train_stats_multi([yd, y3], [bns[3], bns[2]], [ps[3], ps[2]])
                res = None if fold else K.bn_apply(yd, md, idd, gd, bd, residual=None, relu=False)
            else:
                res, md, idd = _bn_train_fwd(yd, gd, bd, bns[3], None, False, partials=ps[3])
        else:
            kd = yd = md = idd = None
            res = xv
        if m3 is None:
            m3, i3 = _bn_train_stats(y3, bns[2], ps[2])
        # BN + residual + ReLU: one byte per 16-byte channel group tells the backward which gradients the ReLU passes (1 / 16 of re-reading the output)
        if res is None:
            out, mask3 = K.bn_apply_res_affine(y3, m3, i3, g3, b3, yd, md, idd, gd, bd, relu=True, want_mask=True)
        else:
            out, mask3 = K.bn_apply(y3, m3, i3, g3, b3, residual=res, relu=True, want_mask=True)
        ctx.geoms, ctx.groups, ctx.has_ds, ctx.deferred = geoms, [b.group for b in bns], wd is not None, deferred
        ctx.save_for_backward(xv, k1, k2, k3, kd, y1, o1, y2, o2, y3, yd, out, m1, i1, m2, i2, m3, i3, md, idd, g1, g2, g3, gd, b1, b2, b3, kv[0], mask3)
        return nchw(out)

    @staticmethod
    def backward(ctx, dout):
        xv, k1, k2, k3, kd, y1, o1, y2, o2, y3, yd, out, m1, i1, m2, i2, m3, i3, md, idd, g1, g2, g3, gd, b1, b2, b3, v2, mask3 = ctx.saved_tensors
        ge, gr, df = ctx.geoms, ctx.groups, ctx.deferred
        dv = _grad_view(dout)
        pair = None
        if ctx.has_ds and _same_exchange([gr[2], gr[3]], [y3.shape[3], yd.shape[3]]):
            # SyncBN, first block of a stage: bn3's masked gradient (= the skip gradient) is known after bn3's REDUCE pass, before its exchange -- so the downsample
            # BatchNorm's reduce pass runs on it right away and the two sum exchanges travel as ONE all-reduce; then both apply passes.
            S = _BnSums(2, y3.shape[3], gr[2], y3.device)
            _, gm = K.bn_bwd_reduce_mask(dv, mask3, y3, m3, i3, want_gmask=True, with_count=True, sums=S.slot(0))
            K.bn_bwd_reduce(gm, None, yd, md, idd, 0, gd, None, want_gmask=False, with_count=True, sums=S.slot(1))
            S.exchange()
            dy3, _ = K.bn_bwd_apply(gm, None, y3, m3, i3, g3, S.total(0), -1.0, 0, False)
            dyd, _ = K.bn_bwd_apply(gm, None, yd, md, idd, gd, S.total(1), -1.0, 0, False, None)
            dres, (dg3, db3), pair = gm, S.grads(0), (dyd, *S.grads(1))
        elif dv.dtype == torch.float32 and K.CONV_PREC != 2:
            # fp32: the masked gradient dv * mask3 (bn3's input gradient AND the skip gradient) is never stored -- every reader takes (dv, mask3). ('bf16_operands' sends
            # conv1's data gradient to the bf16 kernels, whose epilogue takes no masked add: that configuration keeps the stored form.)
            dy3, dg3, db3 = _bn_bwd_masked(dv, mask3, y3, m3, i3, g3, gr[2])
            dres = None
        else:
            dy3, dres, dg3, db3 = _bn_train_bwd(dv, out, y3, m3, i3, g3, b3, True, gr[2], True, True, mask=mask3)
        dw3, _ = _wgrad(o2, dy3, tuple(k3.shape), ge[2], deferred=df[2])
        do2 = K.conv_bwd_data(dy3, k3, tuple(o2.shape), *ge[2])
        dy2, _, dg2, db2 = _bn_train_bwd(do2, o2, y2, m2, i2, g2, b2, True, gr[1], False, False)
        dw2, _ = _wgrad(o1, dy2, tuple(k2.shape), ge[1], deferred=df[1], wino_v=v2)
        do1 = K.conv_bwd_data(dy2, k2, tuple(o1.shape), *ge[1])
        dy1, _, dg1, db1 = _bn_train_bwd(do1, o1, y1, m1, i1, g1, b1, True, gr[0], False, False)
        dw1, _ = _wgrad(xv, dy1, tuple(k1.shape), ge[0], deferred=df[0])
        dwd = dgd = dbd = None
        skip, skip_mask = (dres, None) if dres is not None else (dv, mask3)
        if ctx.has_ds:
            if pair is not None:
                dyd, dgd, dbd = pair
            elif dres is None:
                dyd, dgd, dbd = _bn_bwd_masked(dv, mask3, yd, md, idd, gd, gr[3])
            else:
                dyd, _, dgd, dbd = _bn_train_bwd(dres, None, yd, md, idd, gd, None, False, gr[3], False, False)
            dwdk, _ = _wgrad(xv, dyd, tuple(kd.shape), ge[3], deferred=df[3])
            dwd = dwdk.permute(0, 3, 1, 2)
            skip, skip_mask = (K.conv_bwd_data(dyd, kd, tuple(xv.shape), *ge[3]) if ctx.needs_input_grad[0] else None), None
        dx = nchw(K.conv_bwd_data(dy1, k1, tuple(xv.shape), *ge[0], add=skip, add_mask=skip_mask)) if ctx.needs_input_grad[0] else None
        p = lambda d: d.permute(0, 3, 1, 2)
        return dx, p(dw1), dg1, db1, p(dw2), dg2, db2, p(dw3), dg3, db3, dwd, dgd, dbd, None, None, None


# ---- eval-mode forward: every BatchNorm folded in ONE launch ---------------------------------------------------------------------
# The no-grad eval forward folds each BN into its conv's epilogue; doing that per layer puts 64 four-microsecond kernels (plus their
# launch boundaries) on the critical chain of the memory-commit forward. `prefold(model)` folds all of them at once when the forward
# starts; _ConvBnAct picks its (scale, shift) views from the cache (keyed by the running_mean storage) and falls back to the per-layer
# fold for anything not covered (a conv with a bias, a module swapped in later). PM_FOLD_BATCH=0 disables it.
FOLD_BATCH = _os.environ.get('PM_FOLD_BATCH', '1') == '1'
_fold_cache = None
fold_misses = 0
last_prefold_event = None      # recorded right after the one fold launch: from there on the forward no longer reads any BatchNorm running moment


class prefold:
    def __init__(self, model):
        self.model, self.active = model, False

    def __enter__(self):
        global _fold_cache, last_prefold_event
        last_prefold_event = None
        m = self.model
        if not FOLD_BATCH or m.training or torch.is_grad_enabled() or _fold_cache is not None:
            return self
        bns = getattr(m, '_pm_bn_list', None)
        if bns is None:
            bns = [b for b in m.modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]
            m.__dict__['_pm_bn_list'] = bns
        bns = [b for b in bns if b.running_mean is not None and b.weight is not None and b.running_mean.is_cuda and not b.training]
        if not bns or len({b.eps for b in bns}) != 1:
            return self
        ptrs = tuple(t.data_ptr() for b in bns for t in (b.weight, b.bias, b.running_mean, b.running_var))
        plan = m.__dict__.get('_pm_fold_plan')
        if plan is None or plan[0] != ptrs:            # pointers only change when parameters / buffers are re-created (load, .to, put_theta)
            dev = bns[0].running_mean.device
            cs = [b.num_features for b in bns]
            offs, tot = [], 0
            for c in cs:
                offs.append(tot)
                tot += (c + 3) // 4 * 4                # 16-byte aligned views
            as_i64 = [p - (1 << 64) if p >= (1 << 63) else p for p in ptrs]
            plan = (ptrs, torch.tensor(as_i64, dtype=torch.int64, device=dev), torch.tensor(cs, dtype=torch.int32, device=dev),
                    torch.tensor(offs, dtype=torch.int32, device=dev), cs, offs, tot)
            m.__dict__['_pm_fold_plan'] = plan
        _, table, dcs, doffs, cs, offs, tot = plan
        arena = K.bn_fold_multi(table, dcs, doffs, len(cs), max(cs), tot, bns[0].eps)
        _fold_cache = {b.running_mean.data_ptr(): (arena[o:o + c], arena[tot + o:tot + o + c]) for b, c, o in zip(bns, cs, offs)}
        self.active = True
        last_prefold_event = torch.cuda.current_stream().record_event() if len(bns) == len(m.__dict__['_pm_bn_list']) else None
        return self

    def __exit__(self, *exc):
        global _fold_cache
        if self.active:
            _fold_cache = None
        return False


class _ConvBnAct(torch.autograd.Function):
    """conv -> BatchNorm(train: batch statistics | eval: folded into the conv epilogue) -> (+residual) -> ReLU.
    Replaces e.g. Resnet.py:195-216 conv/bn/relu triples and every Sequential(Conv2d, Norm2d, ReLU) of deepv3plus.py."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, residual, geom, bn, relu, out, deferred=False):
        stride, pad, dil = geom
        xv, wk = nhwc(x), K.krsc(w)
        rv = nhwc(residual) if residual is not None else None
        ov = nhwc(out) if out is not None else None
        ctx.geom, ctx.relu, ctx.train, ctx.deferred = geom, relu, bn.training, deferred and bias is None
        needs_grad = bn.grad_enabled and any(ctx.needs_input_grad[:6])   # needs_input_grad alone ignores torch.no_grad()
        if not bn.training and not needs_grad:     # inference: BN folded into the conv epilogue, nothing saved
            hit = _fold_cache.get(bn.running_mean.data_ptr()) if (_fold_cache is not None and bias is None) else None
            if hit is None:
                global fold_misses
                fold_misses += 1                   # this forward reads running moments after its fold launch (harness: no early hand-back of the main stream)
            scale, shift = hit if hit is not None else K.bn_fold(gamma, beta, bn.running_mean, bn.running_var, bn.eps, bias)
            o = K.conv_fwd(xv, wk, stride, pad, dil, scale=scale, shift=shift, residual=rv, relu=relu, out=ov)
            return nchw(o)
        kv, ps = [], []
        y = K.conv_fwd(xv, wk, stride, pad, dil, bias=bias, keep_v=kv if ctx.needs_input_grad[1] else None, bn_partials=ps if bn.training else None)
        if bn.training:
            o, mean, invstd = _bn_train_fwd(y, gamma, beta, bn, rv, relu, ov, partials=ps[0])
        else:                                      # frozen statistics with a graph: normalise by the running moments, keep y for backward
            mean, invstd = bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)
            o = K.bn_apply(y, mean, invstd, gamma, beta, residual=rv, relu=relu, out=ov)
        ctx.group, ctx.has_bias, ctx.has_res = bn.group, bias is not None, residual is not None
        ctx.save_for_backward(xv, wk, y, o, mean, invstd, gamma, beta, kv[0] if kv else None)
        return nchw(o)

    @staticmethod
    def backward(ctx, dout):
        xv, wk, y, o, mean, invstd, gamma, beta, vk = ctx.saved_tensors
        stride, pad, dil = ctx.geom
        dv = _grad_view(dout)
        want_dres = ctx.has_res and ctx.needs_input_grad[5]
        if ctx.train:
            dy, dres, dgamma, dbeta = _bn_train_bwd(dv, o, y, mean, invstd, gamma, beta, ctx.relu, ctx.group, want_dres, ctx.has_res)
        else:
            # frozen statistics (eval mode): xhat does not depend on the batch, so dy = g * gamma * invstd with g the ReLU-masked
            # gradient; dgamma = sum(g * xhat), dbeta = sum(g) come from the same reduce pass as in training
            c = y.shape[3]
            mode = 0 if not ctx.relu else (1 if ctx.has_res else 2)
            sums, g = K.bn_bwd_reduce(dv, o, y, mean, invstd, mode, gamma, beta, want_gmask=mode != 0)
            g = dv if g is None else g
            dy = K.scale_shift_act(g, gamma * invstd, torch.zeros_like(gamma))
            dres, dgamma, dbeta = (g if want_dres else None), sums[c:], sums[:c]
        dx = nchw(K.conv_bwd_data(dy, wk, tuple(xv.shape), stride, pad, dil, dtype=xv.dtype)) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dwk, db = _wgrad(xv, dy, tuple(wk.shape), (stride, pad, dil), want_bias=ctx.has_bias, deferred=ctx.deferred, wino_v=vk)
            dw = dwk.permute(0, 3, 1, 2)
        return dx, dw, db, dgamma, dbeta, (nchw(dres) if dres is not None else None), None, None, None, None, None


class _Stem(torch.autograd.Function):
    """The stem tail, conv -> BatchNorm(train) -> ReLU -> 3x3 / s2 max pool (Resnet.py:471-478), as one node on the fp32 tier: the pool normalises its taps itself and
    the BatchNorm backward gathers its incoming gradient from the pooled gradient and the argmax bytes, so neither the full-resolution activation nor its gradient
    (302 MB each at 8 x 768^2) is ever written. Same kernels' arithmetic as _ConvBnAct + _MaxPool, bit for bit."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, geom, bn):
        xv, wk = nhwc(x), K.krsc(w)
        kv, ps = [], []
        y = K.conv_fwd(xv, wk, *geom, keep_v=kv if ctx.needs_input_grad[1] else None, bn_partials=ps)
        mean, invstd = _bn_train_stats(y, bn, ps[0])
        out, arg = K.maxpool_bn_relu_fwd(y, mean, invstd, gamma, beta)
        ctx.geom, ctx.group = geom, bn.group
        ctx.save_for_backward(xv, wk, y, mean, invstd, gamma, beta, arg, kv[0] if kv else None)
        return nchw(out)

    @staticmethod
    def backward(ctx, dout):
        xv, wk, y, mean, invstd, gamma, beta, arg, vk = ctx.saved_tensors
        dv = _grad_view(dout)
        S = _BnSums(1, y.shape[3], ctx.group, y.device)
        K.bn_bwd_reduce_pool(dv, arg, y, mean, invstd, gamma, beta, with_count=S.with_count, sums=S.slot(0))
        S.exchange()
        dy = K.bn_bwd_apply_pool(dv, arg, y, mean, invstd, gamma, beta, S.total(0), S.count(y))
        dx = nchw(K.conv_bwd_data(dy, wk, tuple(xv.shape), *ctx.geom, dtype=xv.dtype)) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dwk, _ = _wgrad(xv, dy, tuple(wk.shape), ctx.geom, wino_v=vk)
            dw = dwk.permute(0, 3, 1, 2)
        return (dx, dw, *S.grads(0), None, None)


def stem_tail(x, w, conv, bn):
    """conv(x, w) -> bn -> ReLU -> maxpool3x3s2. w: the weight the convolution runs with (the stem pads conv.weight to four input channels). One fused node in train
    mode with gradients on the fp32 tier; everywhere else (eval, no-grad, the bf16 tier) the two separate nodes. The stem convolution has no bias (Resnet.py:404)."""
    st = BNState(bn)
    if st.training and torch.is_grad_enabled() and K.ACT_DTYPE == torch.float32 and x.dtype == torch.float32 and w.shape[0] % 4 == 0:
        return _Stem.apply(x, w, bn.weight, bn.bias, _geom(conv), st)
    return maxpool3x3s2(_ConvBnAct.apply(x, w, None, bn.weight, bn.bias, None, _geom(conv), st, True, None))


class _ConvBnActN(torch.autograd.Function):
    """N independent conv -> SyncBatchNorm(train) -> ReLU branches of equal width as ONE autograd node whose BatchNorm exchanges travel together: the
    five branches of the ASPP head (deepv3plus.py:72-101: four convolutions of the trunk output + the image-pooling branch). Forward: every convolution, every local
    statistic, ONE all-gather, every finalise + apply; backward: every reduce pass, ONE all-reduce, every apply pass, then the data / weight gradients. Per branch the
    same kernels on the same values as _ConvBnAct -- only the number of collectives changes (10 -> 2 for the ASPP head). Used only with more than one rank."""

    @staticmethod
    def forward(ctx, n, geoms, bns, outs, deferreds, *ts):
        xs, ws, gammas, betas = ts[0:n], ts[n:2 * n], ts[2 * n:3 * n], ts[3 * n:4 * n]
        xvs, wks = [nhwc(x) for x in xs], [K.krsc(w) for w in ws]
        ys, kvs, parts = [], [], []
        for i in range(n):
            kv, ps = [], []
            ys.append(K.conv_fwd(xvs[i], wks[i], *geoms[i], keep_v=kv if ctx.needs_input_grad[5 + n + i] else None, bn_partials=ps))
            kvs.append(kv[0] if kv else None)
            parts.append(ps[0])
        stats = _bn_train_stats_multi(ys, bns, parts)
        os_ = [K.bn_apply(ys[i], stats[i][0], stats[i][1], gammas[i], betas[i], residual=None, relu=True, out=nhwc(outs[i]) if outs[i] is not None else None) for i in range(n)]
        ctx.n, ctx.geoms, ctx.group, ctx.deferreds = n, geoms, bns[0].group, deferreds
        ctx.save_for_backward(*xvs, *wks, *ys, *os_, *[st[0] for st in stats], *[st[1] for st in stats], *gammas, *betas, *kvs)
        return tuple(nchw(o) for o in os_)

    @staticmethod
    def backward(ctx, *douts):
        n = ctx.n
        sv = ctx.saved_tensors
        xvs, wks, ys, os_, means, invs, gammas, betas, kvs = (sv[i * n:(i + 1) * n] for i in range(9))
        S = _BnSums(n, ys[0].shape[3], ctx.group, ys[0].device)
        for i in range(n):
            K.bn_bwd_reduce(_grad_view(douts[i]), os_[i], ys[i], means[i], invs[i], 2, gammas[i], betas[i], want_gmask=False, with_count=True, sums=S.slot(i))
        S.exchange()
        dxs, dws, dgs, dbs = [], [], [], []
        for i in range(n):
            dy, _ = K.bn_bwd_apply(_grad_view(douts[i]), os_[i], ys[i], means[i], invs[i], gammas[i], S.total(i), -1.0, 2, False, betas[i])
            dxs.append(nchw(K.conv_bwd_data(dy, wks[i], tuple(xvs[i].shape), *ctx.geoms[i], dtype=xvs[i].dtype)) if ctx.needs_input_grad[5 + i] else None)
            dwk, _ = _wgrad(xvs[i], dy, tuple(wks[i].shape), ctx.geoms[i], deferred=ctx.deferreds[i], wino_v=kvs[i])
            dws.append(dwk.permute(0, 3, 1, 2))
            dg, db = S.grads(i)
            dgs.append(dg), dbs.append(db)
        return (None, None, None, None, None, *dxs, *dws, *dgs, *dbs)


def conv_bn_act_n(xs, seqs, outs):
    """[conv_bn_act(x, seq[0], seq[1], relu=True, out=o)] for independent (x, Sequential(conv, bn, relu)) branches; ONE SyncBatchNorm exchange per direction when the
    branches qualify (training, gradients on, more than one rank, equal width, no conv bias), the per-branch path otherwise."""
    convs, bns_m = [q[0] for q in seqs], [q[1] for q in seqs]
    ok = (torch.is_grad_enabled() and all(b.training for b in bns_m) and all(cv.bias is None for cv in convs)
          and _same_exchange([D.bn_group(b) for b in bns_m], [cv.out_channels for cv in convs]))
    if not ok:
        return [conv_bn_act(x, cv, bn, relu=True, out=o) for x, cv, bn, o in zip(xs, convs, bns_m, outs)]
    states = [BNState(b) for b in bns_m]      # (registers each layer's num_batches_tracked increment: once, here)
    wd = [_w(cv.weight) for cv in convs]
    n = len(xs)
    return list(_ConvBnActN.apply(n, [_geom(cv) for cv in convs], states, list(outs), [d for _, d in wd], *xs, *[w for w, _ in wd],
                                  *[b.weight for b in bns_m], *[b.bias for b in bns_m]))


class _Conv(torch.autograd.Function):
    """Plain convolution (+bias): final2 / dsn.4 (deepv3plus.py:416-417,424)."""

    @staticmethod
    def forward(ctx, x, w, bias, geom):
        stride, pad, dil = geom
        xv, wk = nhwc(x), K.krsc(w)
        y = K.conv_fwd(xv, wk, stride, pad, dil, bias=bias, out_dtype=torch.float32)      # the class logits (and every other un-normalised head) stay fp32 on the bf16 tier
        ctx.geom, ctx.has_bias = geom, bias is not None
        ctx.save_for_backward(xv, wk)
        return nchw(y)

    @staticmethod
    def backward(ctx, dout):
        xv, wk = ctx.saved_tensors
        stride, pad, dil = ctx.geom
        dv = _grad_view(dout)
        dx = nchw(K.conv_bwd_data(dv, wk, tuple(xv.shape), stride, pad, dil, dtype=xv.dtype)) if ctx.needs_input_grad[0] else None
        dwk, db = _wgrad(xv, dv, tuple(wk.shape), (stride, pad, dil), want_bias=ctx.has_bias)
        return dx, dwk.permute(0, 3, 1, 2), db, None


class _InstNormAct(torch.autograd.Function):
    """nn.InstanceNorm2d(affine = weight is not None) -> ReLU: the tail of an IBN Bottleneck (Resnet.py:205-214: out += residual; out = instance_norm_layer(out);
    relu) and the IBN stem's bn1 + relu (Resnet.py:471-477). Per-image statistics in train and eval mode alike; no running moments, no cross-rank exchange."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu):
        xv = _grad_view(x)
        o, mean, invstd = K.instnorm_fwd(xv, weight, bias, eps, relu)
        ctx.relu, ctx.affine = relu, weight is not None
        ctx.save_for_backward(xv, o if relu else None, weight, mean, invstd)
        return nchw(o)

    @staticmethod
    def backward(ctx, dout):
        xv, o, weight, mean, invstd = ctx.saved_tensors
        dx, dgamma, dbeta = K.instnorm_bwd(_grad_view(dout), xv, o, weight, mean, invstd, ctx.relu, want_affine=ctx.affine)
        return nchw(dx), dgamma, dbeta, None, None


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xv = nhwc(x)
        y, arg = K.maxpool_fwd(xv)
        ctx.shape = tuple(xv.shape)
        ctx.save_for_backward(arg)
        return nchw(y)

    @staticmethod
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        return nchw(K.maxpool_bwd(_grad_view(dout), arg, ctx.shape))


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xv = nhwc(x)
        ctx.shape = tuple(xv.shape)
        return nchw(K.global_avgpool_fwd(xv))

    @staticmethod
    def backward(ctx, dout):
        return nchw(K.global_avgpool_bwd(_grad_view(dout), ctx.shape))


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, out):
        xv = nhwc(x)
        ctx.shape = tuple(xv.shape)
        return nchw(K.resize_fwd(xv, (int(size[0]), int(size[1])), out=nhwc(out) if out is not None else None))

    @staticmethod
    def backward(ctx, dout):
        return nchw(K.resize_bwd(_grad_view(dout), ctx.shape)), None, None


class _Concat(torch.autograd.Function):
    """The branches already wrote their channel slices of `buf`; this node only ties the graph together and
    hands each branch its slice of the incoming gradient (no copy either way)."""

    @staticmethod
    def forward(ctx, buf, *parts):
        ctx.widths = [p.shape[1] for p in parts]
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, dout):
        outs, off = [], 0
        for wd in ctx.widths:
            outs.append(dout[:, off:off + wd])
            off += wd
        return (None,) + tuple(outs)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return nchw(K.add(nhwc(a), nhwc(b)))

    @staticmethod
    def backward(ctx, g):
        return g, g


class _Fanout(torch.autograd.Function):
    """n aliases of a tensor that feeds n branches (the ASPP input, deepv3plus.py:72-95): their gradients are summed left to right
    in ONE pass (pm_add_n) instead of autograd's chain of n - 1 two-operand adds over the 151 MB feature map."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [_grad_view(g) for g in gs if g is not None]
        return (nchw(K.add_n(gs)) if len(gs) > 1 else nchw(gs[0])), None


def fanout(x, n):
    if n < 2 or n > 8 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    return _Fanout.apply(x, n)


class _UpsampleLoss(torch.autograd.Function):
    """A loss of bilinearly up-sampled logits against full-resolution labels, logits never materialised; `form` names the label form of csrc/loss.hip. With a graph
    attached the forward also leaves the column-reduced gradient field (K.upsample_*_fwd_field), so the backward is one short row pass.
    'ce': mean CE(ignore 255) against int64 labels. 'wce': the same with w = weights[label] ([C]) or weights[image][label] ([n, C]); per_image: the sum over images of
    each image's weighted mean (ImageBasedCrossEntropyLoss2d), else sum w nll / sum w over the batch (CrossEntropyLoss(weight)). 'relax': the relaxed-border loss
    (ImgWtLossSoftNLL, loss.py:182-263) against border-set words. The weights carry no gradient."""

    @staticmethod
    def forward(ctx, logits, labels, inv_temp, want_grad, form='ce', weights=None, per_image=None):
        lv = nhwc(logits)
        labels = labels.contiguous()
        ctx.form, ctx.inv_temp, ctx.hw, ctx.per_image = form, inv_temp, tuple(labels.shape[1:]), per_image
        if not want_grad:
            return K._loss_fwd(form, lv, labels, inv_temp, weights, per_image, None, False)[0]
        out, field = K._loss_fwd(form, lv, labels, inv_temp, weights, per_image, None, True)
        ctx.save_for_backward(lv, out, field)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lv, out, field = ctx.saved_tensors
        dl = K._loss_bwd_field(ctx.form, lv, ctx.hw, out, field, g.reshape(1).float().contiguous(), ctx.inv_temp, ctx.per_image)
        return nchw(dl), None, None, None, None, None, None


class _MemRead(torch.autograd.Function):
    """memory.py:317-336. Returns (qr [B,2d,h,w], score [B,h,w,m], p_mem [B,h,w,m])."""

    @staticmethod
    def forward(ctx, x, mem, noise, noise_q=None, with_pq=False):
        xv = nhwc(x)
        mem = mem.contiguous()
        if with_pq:
            qr, score, pmem, pq = K.mem_read_fwd_pq(xv, mem, noise, noise_q)
        else:
            qr, score, pmem = K.mem_read_fwd(xv, mem, noise)
        n, h, w, _ = xv.shape
        m = mem.shape[0]
        ctx.save_for_backward(xv, mem, pmem)
        score, pmem = score.view(n, h, w, m), pmem.view(n, h, w, m)
        ctx.with_pq = with_pq
        if with_pq:
            pq = pq.view(n, h, w, m)
            ctx.mark_non_differentiable(pmem, pq)
            return nchw(qr), score, pmem, pq
        ctx.mark_non_differentiable(pmem)
        return nchw(qr), score, pmem

    @staticmethod
    def backward(ctx, dqr, dscore, _dp, _dq=None):
        xv, mem, pmem = ctx.saved_tensors
        n, h, w, d = xv.shape
        dq = _grad_view(dqr) if dqr is not None else torch.zeros((n, h, w, 2 * d), dtype=torch.float32, device=xv.device)
        ds = dscore.contiguous() if dscore is not None else None
        dx, dmem = K.mem_read_bwd(xv, mem, pmem, dq, ds, want_dmem=ctx.needs_input_grad[1])
        return nchw(dx), dmem, None, None, None


class _MemWriteAccum(torch.autograd.Function):
    """memory.py:219-231 without the one-hot: flat [nominator (m+1,d) | denominator (m+1)]."""

    @staticmethod
    def forward(ctx, z, labels, m):
        zv = nhwc(z)
        labels = labels.contiguous()
        ctx.m = m
        ctx.save_for_backward(zv, labels)
        return K.mem_write_accum(zv, labels, m, normalize=True)

    @staticmethod
    def backward(ctx, dnomden):
        zv, labels = ctx.saved_tensors
        m, d = ctx.m, zv.shape[3]
        dnom = dnomden[:(m + 1) * d].contiguous()
        return nchw(K.mem_write_accum_bwd(zv, labels, m, dnom, normalize=True)), None, None


class _MemWriteUpdate(torch.autograd.Function):
    """memory.py:233-239: momentum update of the slots whose class occurs, then row-normalise."""

    @staticmethod
    def forward(ctx, mem, nomden, momentum):
        mem = mem.contiguous()
        out, u = K.mem_write_update(mem, nomden, momentum, want_u=True)
        ctx.momentum = momentum
        ctx.save_for_backward(u, nomden)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, nomden = ctx.saved_tensors
        m, d = u.shape
        dnom = K.mem_write_update_bwd(u, nomden, ctx.momentum, dout.contiguous())
        g = torch.zeros_like(nomden)
        g[:(m + 1) * d] = dnom.reshape(-1)
        return None, g, None


# ---- functional front-ends (module holders in, logical-NCHW tensors out) ---------------------------------------------
def _geom(conv):
    assert conv.kernel_size[0] == conv.kernel_size[1] and conv.stride[0] == conv.stride[1] and conv.groups == 1
    assert conv.padding[0] == conv.padding[1] and conv.dilation[0] == conv.dilation[1]
    return conv.stride[0], conv.padding[0], conv.dilation[0]


def conv_bn_act(x, conv, bn, relu=True, residual=None, out=None):
    w, deferred = _w(conv.weight)
    return _ConvBnAct.apply(x, w, conv.bias, bn.weight, bn.bias, residual, _geom(conv), BNState(bn), relu, out, deferred)


def bottleneck(x, blk):
    """Whole Bottleneck as one autograd node (train mode with gradients); eval / no-grad keeps the fused-epilogue per-conv path."""
    ds = blk.downsample
    mods = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)] + ([(ds[0], ds[1])] if ds is not None else [])
    geoms = [_geom(c) for c, _ in mods]
    bns = [BNState(b) for _, b in mods]
    ws = [_w(c.weight) for c, _ in mods]
    wd, gd, bd = (ws[3][0], ds[1].weight, ds[1].bias) if ds is not None else (None, None, None)
    return _Bottleneck.apply(x, ws[0][0], blk.bn1.weight, blk.bn1.bias, ws[1][0], blk.bn2.weight, blk.bn2.bias,
                             ws[2][0], blk.bn3.weight, blk.bn3.bias, wd, gd, bd, geoms, bns, [d for _, d in ws] + [False])


def conv(x, conv_mod):
    return _Conv.apply(x, conv_mod.weight, conv_mod.bias, _geom(conv_mod))


def conv_raw(x, weight, bias, geom):
    return _Conv.apply(x, weight, bias, geom)


def instance_norm_act(x, weight, bias, eps=1e-5, relu=True):
    """relu?(instance_norm(x) * weight + bias); weight / bias: both None (nn.InstanceNorm2d(affine=False)) or both parameters."""
    assert (weight is None) == (bias is None), 'instance_norm_act: weight and bias come together'
    return _InstNormAct.apply(x, weight, bias, float(eps), bool(relu))


def instance_norm_module(x, m, relu=True):
    """nn.InstanceNorm2d module `m` (no running statistics: the reference never asks for them) applied to x, then ReLU."""
    assert isinstance(m, torch.nn.InstanceNorm2d) and not m.track_running_stats, 'instance norm with running statistics is not served'
    return instance_norm_act(x, m.weight, m.bias, m.eps, relu)


def maxpool3x3s2(x):
    return _MaxPool.apply(x)


def global_avgpool(x):
    return _GlobalAvgPool.apply(x)


def resize(x, size, out=None):
    return _Resize.apply(x, size, out)


def concat_buffer(like, channels, hw):
    """Logical-NCHW [B, sum(channels), h, w] buffer (NHWC memory) for branches to write into, of the dtype of `like` (bf16 on the bf16 tier: a channel
    total that is not a multiple of 64 -- the decoder's 48 + 256 -- comes with zero pad channels, K.new)."""
    return nchw(K.new((like.shape[0], hw[0], hw[1], sum(channels)), like, dtype=like.dtype if like.dtype == torch.bfloat16 else torch.float32))


def concat(buf, parts):
    return _Concat.apply(buf, *parts)


def add(a, b):
    return _Add.apply(a, b)


class _Cast(torch.autograd.Function):
    """fp32 <-> bf16 at the edges of the bf16 tier (the memory module and the losses stay fp32): one conversion kernel each way."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return nchw(K.cast(nhwc(x), dtype))

    @staticmethod
    def backward(ctx, g):
        return nchw(K.cast(_grad_view(g), ctx.src)), None


def cast(x, dtype):
    return x if x.dtype == dtype else _Cast.apply(x, dtype)


def upsample_ce(logits, labels, inv_temp=1.0):
    if not K.upsample_ce_fused_ok(nhwc(logits), tuple(labels.shape[1:])):
        # rows too wide for the fused kernels' LDS (> ~1000 low-res columns: no training crop of the reference reaches it): the same loss composed from the
        # bilinear kernel and torch's cross entropy on the materialised logits -- correct for any size, not tuned
        full = resize(logits, tuple(labels.shape[1:]))
        return torch.nn.functional.cross_entropy(full * float(inv_temp), labels, ignore_index=255, reduction='mean')
    return _UpsampleLoss.apply(logits, labels, float(inv_temp), bool(torch.is_grad_enabled() and logits.requires_grad))


def weighted_ce(full, labels, weights, per_image):
    """The weighted loss of upsample_wce on materialised logits, composed from torch ops (no host sync): the route of shapes the fused kernels do not take."""
    lp = torch.nn.functional.log_softmax(full, dim=1)
    weights = weights.to(device=full.device, dtype=lp.dtype)
    if weights.dim() == 1 and not per_image:
        return torch.nn.functional.nll_loss(lp, labels, weight=weights, ignore_index=255, reduction='mean')
    rows = weights.expand(full.shape[0], -1) if weights.dim() == 1 else weights
    num = [torch.nn.functional.nll_loss(lp[b:b + 1], labels[b:b + 1], weight=rows[b], ignore_index=255, reduction='sum') for b in range(full.shape[0])]
    valid = (labels >= 0) & (labels < full.shape[1])
    den = [torch.where(valid[b], rows[b][labels[b].clamp(0, full.shape[1] - 1)], lp.new_zeros(())).sum() for b in range(full.shape[0])]
    if per_image:
        return sum(nu / de for nu, de in zip(num, den))
    return sum(num) / sum(den)


def upsample_wce(logits, labels, weights, per_image, inv_temp=1.0):
    """Weighted cross entropy (ignore_index 255) of the bilinearly up-sampled logits, logits never materialised. weights: [C], or [n, C] rows per image (for the
    image-based criterion: K.label_class_weights). per_image False: sum w nll / sum w over the batch; True: the sum over images of each image's weighted mean."""
    per_image = bool(per_image)
    if not K.upsample_ce_fused_ok(nhwc(logits), tuple(labels.shape[1:])):      # as upsample_ce: rows too wide for the fused kernels' LDS
        return weighted_ce(resize(logits, tuple(labels.shape[1:])) * float(inv_temp), labels, weights, per_image)
    return _UpsampleLoss.apply(logits, labels, float(inv_temp), bool(torch.is_grad_enabled() and logits.requires_grad), 'wce', weights.detach(), per_image)


def relax_sets(target, classes):
    """-> bool [n, classes, H, W]: the real classes of every pixel's border set, from int32 words [n,H,W] or the reference's uint8 multi-hot [n, classes + 1, H, W]."""
    if target.dim() == 4:
        return target[:, :classes] != 0
    return ((target.unsqueeze(1) >> torch.arange(classes, device=target.device).view(1, -1, 1, 1)) & 1).bool()


def relaxed_soft_nll(full, target, weights):
    """The loss of upsample_relax on materialised logits `full` [n,C,H,W], composed from torch ops without a host sync: the route of CPU tensors and of shapes the
    fused kernel does not take. Per pixel - W_S log P_S with log P_S = logsumexp over the set - logsumexp over all classes; classes outside the set are masked, never
    multiplied by zero, so an underflowing probability outside the set cannot make a NaN (the reference's 0 * log 0). weights: [C] or [n, C]."""
    n, C = full.shape[:2]
    inset = relax_sets(target, C)
    k = inset.sum(1)
    valid = k > 0
    rows = weights.to(device=full.device, dtype=full.dtype)
    rows = (rows.expand(n, -1) if rows.dim() == 1 else rows).view(n, C, 1, 1)
    wbar = torch.where(inset, rows, rows.new_zeros(())).sum(1) / k.clamp(min=1).to(full.dtype)
    # a pixel without a set keeps all its logits (its term is dropped below): a logsumexp over nothing would be -inf with a NaN gradient
    log_ps = torch.logsumexp(torch.where(inset | ~valid.unsqueeze(1), full, full.new_full((), float('-inf'))), dim=1) - torch.logsumexp(full, dim=1)
    terms = torch.where(valid, -wbar * log_ps, full.new_zeros(()))
    per_image = terms.flatten(1).sum(1) / (valid.flatten(1).sum(1).to(full.dtype) + 1)
    return per_image.sum() / n


def upsample_relax(logits, bits, weights, inv_temp=1.0):
    """ImgWtLossSoftNLL of the bilinearly up-sampled logits [n,C,h,w] against border-set words [n,H,W] (K.relax_border_bits / K.multihot_to_bits), the logits
    never materialised. weights: [C] or [n, C] rows (K.relax_class_weights). Tiers as upsample_wce: fp32 logits."""
    size = tuple(bits.shape[1:])
    if not logits.is_cuda:
        return relaxed_soft_nll(torch.nn.functional.interpolate(logits, size=size, mode='bilinear', align_corners=True) * float(inv_temp), bits, weights)
    if not K.upsample_relax_ok(nhwc(logits), size):      # rows too wide for the fused kernel's LDS: as upsample_ce
        return relaxed_soft_nll(resize(logits, size) * float(inv_temp), bits, weights)
    return _UpsampleLoss.apply(logits, bits, float(inv_temp), bool(torch.is_grad_enabled() and logits.requires_grad), 'relax', weights.detach())


def mem_read(x, mem, noise=None):
    return _MemRead.apply(x, mem, noise, None, False)


def mem_read_pq(x, mem, noise=None, noise_q=None):
    """(qr, score, p_mem, p_query): the read with the softmax over all queries (memory.py:183-186) finished from the read kernel's column partials."""
    return _MemRead.apply(x, mem, noise, noise_q, True)


def mem_write_accum(z, labels, m):
    return _MemWriteAccum.apply(z, labels, m)


def mem_write_update(mem, nomden, momentum):
    return _MemWriteUpdate.apply(mem, nomden, float(momentum))
