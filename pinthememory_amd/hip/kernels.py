"""Raw (non-autograd) launches of the HIP kernels on torch-owned NHWC fp32 tensors.
Every function enqueues on torch's current stream and returns torch tensors; no CPU fallback exists."""
import ctypes
from ctypes import byref

import os
import weakref

import torch

from . import lib as L
from .lib import PmConvEpilogue, PmConvParams, check, ptr, stream, tdesc, workspace


def _lib():
    return L.load()


# 0: fp32 MFMA (parity path, BASELINE configs[1]). 2: configs[2], the bf16 tier -- each convolution's operands are converted to bf16 in HBM
# (one streaming pass, RNE), bf16 tiles of 64 k-values per row in LDS, v_mfma_f32_32x32x16_bf16 with fp32 accumulation; activations between
# layers, BatchNorm, losses and the memory stay fp32. 1: the first form of that tier (fp32 tiles staged in LDS, rounded per fragment), which
# prec 2 falls back to for the call sites it does not cover (3-channel stem, 19-class heads, stride-2 data gradients).
CONV_PREC = 0
# Element type of the activations BETWEEN layers. 'bf16' (round 4) = the whole tier: convolutions write bf16, every elementwise / reduction kernel between them
# (BatchNorm: csrc/bn.hip; pooling, resize: csrc/pool_resize.hip; adds, copies: csrc/misc.hip -- one kernel template per pass for both element types) reads and writes bf16 with fp32 arithmetic; the image, the class logits, the losses, the memory module,
# every statistic and every parameter / parameter gradient stay fp32. 'bf16_operands' = round 2-3's form (fp32 activations, operands cast per convolution).
ACT_DTYPE = torch.float32


def set_conv_precision(name):
    global CONV_PREC, ACT_DTYPE
    CONV_PREC = {'f32': 0, 'fp32': 0, 'bf16': 2, 'bf16_operands': 2, 'bf16_staged': 1}[name]
    ACT_DTYPE = torch.bfloat16 if name == 'bf16' else torch.float32


def _act_dtype(like):
    return like.dtype if like.dtype in (torch.float32, torch.bfloat16) else torch.float32


def new(shape, like, pitch_pad=False, zero_pad=True, dtype=None):
    """Fresh NHWC tensor of `dtype` (default: like.dtype). fp32: channel counts that are not a multiple of 4 (the 19 logits) get a padded pitch so rows
    stay 16B aligned; the pad lanes are zero unless the producer writes them itself (zero_pad=False). bf16: a channel count that is not a multiple of 64
    (the 48-channel skip branch, the 304-channel decoder gradient) is allocated with zero pad channels up to the next multiple and registered, so that a
    convolution gathers it in place (lib.register_zero_pad)."""
    n, h, w, c = shape
    dtype = _act_dtype(like) if dtype is None else dtype
    if dtype == torch.bfloat16:
        if c % 64:
            base = torch.empty((n, h, w, (c + 63) // 64 * 64), dtype=dtype, device=like.device)
            base[..., c:].zero_()              # only the pad channels: every producer writes all c valid ones (a full clear of the 304 -> 320 concat buffer was 31 us)
            L.register_zero_pad(base, c, base.shape[3])
            return base[..., :c]
        return torch.empty((n, h, w, c), dtype=dtype, device=like.device)
    if c % 4 and pitch_pad:
        cp = (c + 3) // 4 * 4
        alloc = torch.zeros if zero_pad else torch.empty
        return alloc((n, h, w, cp), dtype=torch.float32, device=like.device)[..., :c]
    return torch.empty((n, h, w, c), dtype=torch.float32, device=like.device)


def cast(x, dtype):
    """NHWC tensor -> the same values as `dtype` (fp32 <-> bf16, round to nearest even): the edges of the bf16 tier."""
    if x.dtype == dtype:
        return x
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(_lib().pm_cast(byref(tdesc(x)), byref(tdesc(y)), stream()), 'pm_cast')
    return y


def conv_out_hw(h, w, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1


def krsc(w):
    """[Cout,Cin,kh,kw] parameter -> contiguous KRSC memory (a free view when the parameter is channels_last)."""
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


KEEP_WINOGRAD_V = os.environ.get('PM_KEEP_V', '1') == '1'   # forward keeps the Winograd-transformed input for the weight gradient


# BatchNorm statistics handed out by the producing convolution's epilogue: the unbatched direct GEMMs (every 1x1 and direct
# 3x3 convolution) emit (mean, M2) per 32-row slab and channel from their staged epilogue, merged in double by pm_bn_partials_finalize, so that no
# separate pass re-reads the convolution output: -1.0 ms/step of statistics passes for +0.35 ms of epilogue and the slab merge. Same-box A/B over
# five alternated pairs (tools/gpu_env_abn.sh): 66.41 vs 66.60 ms/step, every pair in favour (-0.08 ... -0.34). It stays opt-in (PM_BN_EPILOGUE=1):
# the statistics are as accurate as the separate pass (kernel test: 1e-6 of torch's double) but rounded differently, other ReLU units sit within
# round-off of zero, and with the default flipped one bias gradient of the mldg test (layer4.2.bn3.bias: 5.9e-3 of its norm, inside the fixed 1e-2
# bound) lands outside that test's RELATIVE bar (3 x the reference's own fp32 error + 1e-4). A 0.3 % gain is not worth a looser gate.
BN_EPILOGUE = os.environ.get('PM_BN_EPILOGUE', '0') == '1'
# bf16 tier (round 4): the same epilogue exists in both bf16 kernels (pm_slab_stats16) and measures SLOWER than the separate pass -- same box, two alternated
# pairs (tools/gpu_r4_envab.sh PM_BN_EPILOGUE16): 26.52 / 26.61 ms/step without, 26.94 / 26.94 with. The statistics pass reads a tensor the convolution has just
# left in the 256 MB infinity cache (10 us per layer), while the epilogue form adds two LDS sweeps and 48 lane exchanges per slab to an MFMA-bound kernel and
# hands the finalize 9 216 slab partials instead of <= 288 block partials. Opt-in (PM_BN_EPILOGUE16=1), covered by test_conv_epilogue_bn_statistics_bf16.
BN_EPILOGUE16 = os.environ.get('PM_BN_EPILOGUE16', '0') == '1'
# Round 5: per shape. Where the PRODUCING convolution is HBM-bound and its output does not stay in the 256 MB infinity cache -- the 1x1 convolutions onto the 192 x 192
# and 96 x 96 maps, 75-151 MB of bf16 output -- the separate statistics pass is a full HBM read (28-54 us per layer) while the epilogue's extra LDS sweeps hide under
# the convolution's own memory time. PM_BN_EP16_MIN_MB: outputs of at least this many MB take the epilogue route (0 = never).
BN_EP16_MIN_BYTES = int(float(os.environ.get('PM_BN_EP16_MIN_MB', '0')) * (1 << 20))
BN_EP_MIN_BYTES = int(float(os.environ.get('PM_BN_EP_MIN_MB', '0')) * (1 << 20))      # the same per-shape rule on the fp32 tier (outputs of at least this many MB)


# Transformed filters -- the Winograd U = G w G^T, or the bf16 copy of the weights in the bf16 tier -- kept between calls: the eval-mode forward of
# step t and the training forward of step t + 1 read the same weights. The cache is SCOPED TO AN OWNER that vouches for its updates: optim.SGD
# registers the parameters it owns (register_filter_owners) and bumps their tensor VERSION for its fused raw-pointer update; only registered leaf
# parameters are cached, keyed by storage address + transformed size, validated by (the owner is alive, still at that address, same version).
# Every in-place update through torch's ops bumps the version too. What does NOT bump it is a write through `w.data` or raw pointers by code that
# is not the owner (legacy optimizers, manual EMA, an in-place collective on parameters): weights nobody registered are never cached, so such code
# cannot meet a stale filter. Entries hold a WEAK reference to the owner -- functional weights (train_memory_mldg's theta), `.contiguous()` copies and
# models that are gone are neither cached nor retained. PM_KEEP_U=0 switches the cache off, PM_KEEP_U=1 caches every weight (A/B runs and tests).
KEEP_WINOGRAD_U = {'0': False, '1': True}.get(os.environ.get('PM_KEEP_U', ''))      # None = owner-scoped (default)

_U_OWNERS = {}      # storage address -> weakref to the registered leaf parameter
_U_CACHE_MAX = 256
_U_CACHE_BYTES = int(os.environ.get('PM_KEEP_U_MB', '2048')) << 20     # one ResNet-50 DeepLabV3+ keeps 0.43 GB, a ResNet-101 DeepLabV2 0.65 GB


def register_filter_owners(params):
    """Called by an optimizer for the weights it owns: it promises that every update of them moves the tensor version (optim.SGD does)."""
    for p in params:
        if isinstance(p, torch.nn.Parameter) and p.is_leaf and p.is_cuda and p.dim() == 4 and p.dtype == torch.float32:
            _U_OWNERS[p.data_ptr()] = weakref.ref(p)


def unregister_filter_owners(params=None):
    """Forget the owner's weights (all of them when params is None) and drop their cached filters."""
    ptrs = None if params is None else {p.data_ptr() for p in params}
    for k in [k for k in _U_OWNERS if ptrs is None or k in ptrs]:
        del _U_OWNERS[k]
    _U_CACHE.drop_if(lambda ent: ptrs is None or ent.ptr in ptrs)


def _filter_owner(w_krsc):
    ref = _U_OWNERS.get(w_krsc.data_ptr())
    p = ref() if ref is not None else None
    if p is None:
        if ref is not None:
            del _U_OWNERS[w_krsc.data_ptr()]
        return None
    return p if (p.data_ptr() == w_krsc.data_ptr() and p.numel() == w_krsc.numel() and p.is_leaf) else None


class _KeptFilter:
    """One kept transform. ptr ... dgrad are the fields of its lookup key: the weight's storage address and KRSC shape, the bytes of the transform, the device
    index, the tier (CONV_PREC) and whether it is the rotated / transposed bf16 filter of a data gradient.
    owner: call it -> the tensor whose version vouches for the buffer, or None once that tensor is gone (a weak reference to the registered parameter; forced
    mode holds the unregistered weight of the call itself). version: the owner's version the buffer holds, -1 while a rewrite is pending.
    event / stream: recorded behind the launch that last wrote buf, and that launch's raw stream (None: nothing to wait for). used: read since the last refresh."""
    __slots__ = ('ptr', 'shape', 'nbytes', 'device', 'prec', 'dgrad', 'owner', 'version', 'buf', 'event', 'stream', 'used')


class _FilterCache(dict):
    """lookup key -> _KeptFilter, oldest first (dicts keep insertion order; hits are re-inserted)."""
    def __init__(self):
        self.nbytes = 0         # of all kept buffers
        self.streams = {}       # raw handle -> every stream that ever read or wrote a kept transform (main stream, the harness' commit stream)

    def _stream(self):
        raw = stream()
        cur = self.streams.get(raw)
        if cur is None:
            cur = self.streams[raw] = L.stream_obj()
        return raw, cur

    def _drop(self, key):
        """The one way an entry leaves. The buffer goes back to the pool of the stream that allocated it, while a launch on ANOTHER stream (the commit forward) may still
        be reading it: tell the allocator about every stream that uses the cache, so that the block is not handed out again before their queued work is done."""
        ent = self.pop(key)
        self.nbytes -= ent.nbytes
        if ent.buf.is_cuda:
            for s in self.streams.values():
                ent.buf.record_stream(s)

    def drop_if(self, pred):
        for key in [k for k, ent in self.items() if pred(ent)]:
            self._drop(key)

    def clear(self):
        """Drop every kept transform (the registered owners stay)."""
        self.drop_if(lambda ent: True)

    def lookup(self, p, w_krsc, nbu, dgrad=False):
        """Point the call's parameters `p` at the kept transform of this weight, allocating one on a miss. nbu: bytes of the transformed filter of this call
        (pm_conv_wxf_bytes / _dgrad; 0: none). -> None when the call finds it valid (or nothing is kept), else (entry, version): the call rewrites the buffer and
        hands the pair to commit() once its launch is enqueued."""
        if KEEP_WINOGRAD_U is False or not nbu:
            return None
        registered = _filter_owner(w_krsc)
        if registered is None and KEEP_WINOGRAD_U is not True:
            return None
        owner = w_krsc if registered is None else registered      # forced mode keeps unregistered weights too: the tensor of this call stands in for an owner
        key = (w_krsc.data_ptr(), tuple(w_krsc.shape), nbu, w_krsc.device.index, p.prec, dgrad)
        ent = self.get(key)
        if ent is not None and ent.owner() is not owner:
            self._drop(key)            # another tensor now lives at this address: the kept transform is somebody else's
            ent = None
        if ent is None:
            # only a miss evicts (a captured step has the buffer addresses of its hits baked in): models that are gone release their buffers here, then the oldest go
            self.drop_if(lambda e: e.owner() is None)
            while self and (len(self) >= _U_CACHE_MAX or self.nbytes + nbu > _U_CACHE_BYTES):
                self._drop(next(iter(self)))
            ent = _KeptFilter()
            ent.ptr, ent.shape, ent.nbytes, ent.device, ent.prec, ent.dgrad = key
            ent.owner = (lambda: w_krsc) if registered is None else weakref.ref(registered)
            ent.version, ent.buf, ent.event, ent.stream = -1, torch.empty(nbu // 4, dtype=torch.float32, device=w_krsc.device), None, None
            self.nbytes += nbu
        else:
            del self[key]       # a hit moves to the young end
        self[key] = ent
        ent.used = True
        version = owner._version
        valid = ent.version == version
        if not valid:
            ent.version = -1            # invalid until the launch that fills it has been enqueued (the caller commits the version after check())
        p.wxf, p.wxf_bytes, p.wxf_valid = ent.buf.data_ptr(), nbu, 1 if valid else 0
        raw, cur = self._stream()
        if valid and ent.event is not None and ent.stream != raw:
            cur.wait_event(ent.event)   # the transform was written by a launch on another stream (harness: the commit forward runs on its own)
        return None if valid else (ent, version)

    def commit(self, *pending):
        """pending: (entry, version) pairs whose buffers the launch just enqueued on the current stream writes (check() has passed): only now are they valid;
        hits from another stream wait for this event."""
        raw, cur = self._stream()
        event = cur.record_event()
        for ent, version in pending:
            ent.version, ent.event, ent.stream = version, event, raw

    def forget_events(self):
        """Drop the 'written by a launch on another stream' events of every kept transform. Call after torch.cuda.synchronize(): harness.GraphedAggStep does once its capture
        has ended -- events recorded inside a stream capture must not be waited for from eager code, and a replay (a single launch in stream order) needs none."""
        for ent in self.values():
            ent.event = ent.stream = None


_U_CACHE = _FilterCache()
clear_filters, forget_filter_events = _U_CACHE.clear, _U_CACHE.forget_events

# tier (CONV_PREC) -> (the library's batched rewrite, does it take only the forward transforms of 3x3 filters).
# 2: every kept bf16 filter (forward copy, rotated copy of the data gradient) in ONE or two launches instead of one small cast in front of each of the ~142 convolution
# calls of the next step. 0: every kept Winograd FORWARD transform (U = G g Gt of the wide stride-1 3x3 layers) in one launch instead of ~20 latency-bound per-layer
# launches in front of the next forward pass. Same kernel bodies as the per-call transforms, same bits.
_REFRESH = {2: ('pm_conv_wxf_refresh_bf16', False), 0: ('pm_conv_wxf_refresh_f32', True)}


def refresh_filters():
    """Called by the optimizer right after it moved the weights: rewrite every kept filter transform of the active tier that was used since the last call and is now
    out of date, in one call of the library. Entries nobody used in the last step are left to go stale (their convolution re-derives them if it returns), dead or moved
    owners are skipped. The caller has already made sure no other stream still reads the buffers (optim.SGD.step: ops.wait_commit()). Returns the number of filters
    rewritten (0: no launch)."""
    if KEEP_WINOGRAD_U is False or not _U_CACHE or CONV_PREC not in _REFRESH:
        return 0
    entry_point, forward_3x3_only = _REFRESH[CONV_PREC]
    dev = torch.cuda.current_device()
    todo = []
    for ent in _U_CACHE.values():
        if ent.prec != CONV_PREC or ent.device != dev or not ent.used:
            continue
        cout, kh, kw, cin = ent.shape
        if forward_3x3_only and (ent.dgrad or kh != 3 or kw != 3):
            continue
        ent.used = False
        owner = ent.owner()
        if owner is None or owner.data_ptr() != ent.ptr or ent.version == owner._version or not ent.buf.is_cuda:
            continue
        todo.append((ent, owner._version))
    if not todo:
        return 0
    jobs = (L.PmWxfJob * len(todo))()
    for j, (ent, version) in zip(jobs, todo):
        cout, kh, kw, cin = ent.shape
        j.w, j.wxf, j.wxf_bytes, j.cout, j.kh, j.kw, j.cin, j.dgrad = ent.ptr, ent.buf.data_ptr(), ent.nbytes, cout, kh, kw, cin, 1 if ent.dgrad else 0
        ent.version = -1
    check(getattr(_lib(), entry_point)(jobs, len(todo), stream()), entry_point)
    _U_CACHE.commit(*todo)
    return len(todo)


# Size queries of the convolution entry points (workspace, kept Winograd V, transformed filter, statistics partials) depend on shapes and on the library's
# process-wide switches only: asked once per distinct call signature instead of three ctypes round trips per launch (the bf16 tier is host-bound).
_SIZES = {}
_GEN = [0]      # bumped by every switch that changes the library's routing (set_winograd, set_conv16, ...)


def _sizes(key, fn):
    v = _SIZES.get(key)
    if v is None:
        if len(_SIZES) > 8192:
            _SIZES.clear()
        v = _SIZES[key] = fn()
    return v


_XFORM_COUNT = [0, False]      # [convolution calls that had to derive a transformed filter (Winograd U / bf16 copy) instead of finding a kept one, counting on]


def filter_transform_count(enable=None):
    """Diagnostic (bench.py --workload mldg): number of forward convolutions that transformed their filter while counting was on."""
    if enable is not None:
        _XFORM_COUNT[1] = bool(enable)
    return _XFORM_COUNT[0]


def conv_fwd(x, w_krsc, stride, pad, dil, bias=None, scale=None, shift=None, residual=None, relu=False, out=None, keep_v=None, bn_partials=None, out_dtype=None):
    """keep_v: a list; if this convolution and its weight gradient both take the Winograd route, the transformed input V is written
    to a fresh tensor that is appended to the list (else None is appended) -- pass it to conv_bwd_weight(wino_v=...).
    bn_partials: a list; if this call can hand the train-mode BatchNorm statistics of its output out of its own epilogue ((mean, M2) per
    32-row slab and channel), the partials tensor is appended (else None) -- merge it with bn_partials_finalize(...) instead of bn_stats(y)."""
    cout, kh, kw, cin = w_krsc.shape
    n, h, w_, c = x.shape
    assert c == cin, 'conv: Cin mismatch %d vs %d' % (c, cin)
    ho, wo = conv_out_hw(h, w_, kh, stride, pad, dil)
    y = out if out is not None else new((n, ho, wo, cout), x, pitch_pad=True, dtype=out_dtype if out_dtype is not None else ACT_DTYPE)
    assert residual is None or residual.dtype == y.dtype, 'conv_fwd: the fused residual has the dtype of the output'
    xd, yd = tdesc(x), tdesc(y)
    p = L.conv_params(kh, kw, stride, pad, dil, CONV_PREC)
    lib = _lib()
    nbv, nbu, nb, npb = _sizes(('f', x.shape, x.stride(), x.dtype, xd.flags, w_krsc.shape, y.stride(), y.dtype, stride, pad, dil, CONV_PREC, _GEN[0]),
                               lambda: (lib.pm_conv_winograd_v_bytes(byref(xd), byref(yd), byref(p)), lib.pm_conv_wxf_bytes(byref(xd), byref(yd), byref(p)),
                                        lib.pm_conv_workspace(byref(xd), byref(yd), byref(p), 0), lib.pm_conv_bn_partials_bytes(byref(xd), byref(yd), byref(p))))
    if keep_v is not None:
        nbv = nbv if KEEP_WINOGRAD_V else 0
        v = torch.empty(nbv // 4, dtype=torch.float32, device=x.device) if nbv else None
        keep_v.append(v)
        if v is not None:
            p.wino_v, p.wino_v_bytes = v.data_ptr(), nbv
    u_ent = None
    if (kh == 3 and CONV_PREC == 0) or CONV_PREC == 2:
        u_ent = _U_CACHE.lookup(p, w_krsc, nbu)        # (cache entry this call is about to (re)write, version to commit once the launch is enqueued) or None
    if _XFORM_COUNT[1] and p.wxf_valid == 0 and nbu:
        _XFORM_COUNT[0] += 1      # this call transforms its filter
    ws = workspace(nb, x.device) if nb else None
    part = None
    if bn_partials is not None:
        ep16 = BN_EPILOGUE16 or (BN_EP16_MIN_BYTES > 0 and y.numel() * 2 >= BN_EP16_MIN_BYTES)
        ep32 = BN_EPILOGUE or (BN_EP_MIN_BYTES > 0 and y.numel() * 4 >= BN_EP_MIN_BYTES)
        npb = npb if ((ep16 if y.dtype == torch.bfloat16 else ep32) and residual is None and not relu and scale is None) else 0
        part = torch.empty(npb // 4, dtype=torch.float32, device=x.device) if npb else None
        bn_partials.append(part)
    ep = None
    if bias is not None or scale is not None or residual is not None or relu or part is not None:
        rd = tdesc(residual) if residual is not None else None
        ep = L.conv_epilogue(ptr(bias), ptr(scale), ptr(shift), rd.ptr if rd else None, rd.pitch if rd else 0, 1 if relu else 0, ptr(part),
                            part.numel() * 4 if part is not None else 0)
    check(lib.pm_conv_fwd(byref(xd), w_krsc.data_ptr(), byref(yd), byref(p), byref(ep) if ep else None, ptr(ws), nb, stream()), 'pm_conv_fwd')
    if u_ent is not None:
        _U_CACHE.commit(u_ent)
    return y


def conv_bwd_data(dy, w_krsc, x_shape, stride, pad, dil, add=None, dtype=None, add_mask=None):
    """dtype: element type of dx = the type of the tensor it is the gradient of (default: dy's). add_mask: bn_apply(want_mask=True)'s bytes -- `add` enters as
    (bit ? add : 0); fp32, and only where the call routes to the implicit-GEMM kernels (the library refuses it elsewhere)."""
    cout, kh, kw, cin = w_krsc.shape
    dx = new(x_shape, dy, dtype=dtype)
    dyd, dxd = tdesc(dy), tdesc(dx)
    p = L.conv_params(kh, kw, stride, pad, dil, CONV_PREC)
    lib = _lib()
    nb, nbu = _sizes(('d', dy.shape, dy.stride(), dy.dtype, dyd.flags, w_krsc.shape, dx.shape, dx.stride(), dx.dtype, stride, pad, dil, CONV_PREC, _GEN[0]),
                     lambda: (lib.pm_conv_workspace(byref(dxd), byref(dyd), byref(p), 1), lib.pm_conv_wxf_bytes_dgrad(byref(dyd), byref(dxd), byref(p))))
    ws = workspace(nb, dy.device) if nb else None
    ad = tdesc(add) if add is not None else None
    u_ent = _U_CACHE.lookup(p, w_krsc, nbu, dgrad=True) if CONV_PREC == 2 else None      # bf16 tier: the rotated bf16 filter is kept per weight version
    if add_mask is not None:
        check(lib.pm_conv_bwd_data_masked(byref(dyd), w_krsc.data_ptr(), byref(dxd), byref(p), byref(ad), add_mask.data_ptr(), ptr(ws), nb, stream()), 'pm_conv_bwd_data_masked')
    else:
        check(lib.pm_conv_bwd_data(byref(dyd), w_krsc.data_ptr(), byref(dxd), byref(p), byref(ad) if ad else None, ptr(ws), nb, stream()), 'pm_conv_bwd_data')
    if u_ent is not None:
        _U_CACHE.commit(u_ent)
    return dx


def conv_bwd_weight(x, dy, w_shape_krsc, stride, pad, dil, want_bias=False, wino_v=None, on_stream=None):
    """on_stream: launch on that torch stream instead of the current one (the caller orders it and tells the allocator: ops._wgrad)."""
    cout, kh, kw, cin = w_shape_krsc
    dw = torch.empty(w_shape_krsc, dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    xd, dyd = tdesc(x), tdesc(dy)
    p = L.conv_params(kh, kw, stride, pad, dil, CONV_PREC)
    if wino_v is not None:       # Winograd-transformed x kept by conv_fwd(keep_v=...)
        p.wino_v, p.wino_v_bytes = wino_v.data_ptr(), wino_v.numel() * 4
    lib = _lib()
    nb = _sizes(('w', x.shape, x.stride(), x.dtype, dy.shape, dy.stride(), dy.dtype, w_shape_krsc, stride, pad, dil, CONV_PREC, wino_v is not None, _GEN[0]),
                lambda: lib.pm_conv_workspace(byref(xd), byref(dyd), byref(p), 2))
    raw = stream() if on_stream is None else on_stream.cuda_stream
    ws = workspace(nb, x.device, on_stream)
    check(lib.pm_conv_bwd_weight(byref(xd), byref(dyd), dw.data_ptr(), ptr(db), byref(p), ptr(ws), nb, raw), 'pm_conv_bwd_weight')
    return dw, db


# ---- batch norm --------------------------------------------------------------------------------------------------
def bn_stats(x):
    """-> moments float[3C] = mean | M2 | count (local to this rank)."""
    c = x.shape[3]
    mom = torch.empty(3 * c, dtype=torch.float32, device=x.device)
    xd = tdesc(x)
    lib = _lib()
    nb = _sizes(('bn', x.shape, x.dtype), lambda: lib.pm_bn_workspace(byref(xd)))
    ws = workspace(nb, x.device)
    check(lib.pm_bn_stats(byref(xd), mom.data_ptr(), ptr(ws), nb, stream()), 'pm_bn_stats')
    return mom


def bn_stats_finalize(x, eps, running_mean=None, running_var=None, momentum=0.1):
    """bn_stats + bn_finalize for local statistics in one library call -> (mean, invstd); running moments updated in place."""
    c = x.shape[3]
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    xd = tdesc(x)
    lib = _lib()
    nb = _sizes(('bn', x.shape, x.dtype), lambda: lib.pm_bn_workspace(byref(xd)))
    ws = workspace(nb, x.device)
    check(lib.pm_bn_stats_finalize(byref(xd), eps, mean.data_ptr(), invstd.data_ptr(), ptr(running_mean), ptr(running_var), momentum, ptr(ws), nb, stream()),
          'pm_bn_stats_finalize')
    return mean, invstd


def bn_partials_finalize(part, pixels, c, eps, running_mean=None, running_var=None, momentum=0.1):
    """(mean, M2) slab partials emitted by a convolution epilogue -> (mean, invstd); running moments updated in place."""
    mean = torch.empty(c, dtype=torch.float32, device=part.device)
    invstd = torch.empty_like(mean)
    check(_lib().pm_bn_partials_finalize(part.data_ptr(), pixels, c, eps, mean.data_ptr(), invstd.data_ptr(), ptr(running_mean), ptr(running_var), momentum, None,
                                         stream()), 'pm_bn_partials_finalize')
    return mean, invstd


def bn_partials_moments(part, pixels, c):
    """the same partials -> moments float[3C] = mean | M2 | count (the SyncBatchNorm exchange format of bn_stats)."""
    mom = torch.empty(3 * c, dtype=torch.float32, device=part.device)
    check(_lib().pm_bn_partials_finalize(part.data_ptr(), pixels, c, 0.0, None, None, None, None, 0.0, mom.data_ptr(), stream()), 'pm_bn_partials_finalize')
    return mom


def bn_merge(parts, world, c):
    """parts: float[world, 3c] gathered per-rank moments -> merged float[3c]."""
    out = torch.empty(3 * c, dtype=torch.float32, device=parts.device)
    check(_lib().pm_bn_merge(parts.data_ptr(), world, c, out.data_ptr(), stream()), 'pm_bn_merge')
    return out


def bn_merge_finalize(parts, world, c, eps, running_mean=None, running_var=None, momentum=0.1):
    """bn_merge + bn_finalize in one launch: gathered per-rank moments float[world, 3c] -> (mean, invstd); running moments in place."""
    mean = torch.empty(c, dtype=torch.float32, device=parts.device)
    invstd = torch.empty_like(mean)
    check(_lib().pm_bn_merge_finalize(parts.data_ptr(), world, c, eps, mean.data_ptr(), invstd.data_ptr(), ptr(running_mean), ptr(running_var), momentum,
                                      stream()), 'pm_bn_merge_finalize')
    return mean, invstd


def bn_finalize(moments, c, eps, running_mean=None, running_var=None, momentum=0.1):
    mean = torch.empty(c, dtype=torch.float32, device=moments.device)
    invstd = torch.empty_like(mean)
    check(_lib().pm_bn_finalize(moments.data_ptr(), c, eps, mean.data_ptr(), invstd.data_ptr(), ptr(running_mean), ptr(running_var), momentum, stream()),
          'pm_bn_finalize')
    return mean, invstd


def bn_fold_multi(table, cs, offs, n, max_c, total, eps):
    """n BatchNorm layers folded in one launch -> arena float[2 * total] (scales | shifts); table / cs / offs are device tensors."""
    arena = torch.empty(2 * total, dtype=torch.float32, device=table.device)
    check(_lib().pm_bn_fold_multi(table.data_ptr(), cs.data_ptr(), offs.data_ptr(), n, max_c, total, eps, arena.data_ptr(), stream()), 'pm_bn_fold_multi')
    return arena


def bn_fold(gamma, beta, running_mean, running_var, eps, conv_bias=None):
    c = gamma.numel()
    scale = torch.empty(c, dtype=torch.float32, device=gamma.device)
    shift = torch.empty_like(scale)
    check(_lib().pm_bn_fold(gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), ptr(conv_bias), c, eps, scale.data_ptr(),
                            shift.data_ptr(), stream()), 'pm_bn_fold')
    return scale, shift


def bn_apply(x, mean, invstd, gamma, beta, residual=None, relu=False, out=None, want_mask=False):
    """want_mask: also -> uint8 [pixels, C / 4], bit e of a byte = output e of that float4 group is positive (the ReLU mask for bn_bwd_reduce_mask)."""
    y = out if out is not None else torch.empty_like(x, memory_format=torch.contiguous_format)
    rd = tdesc(residual) if residual is not None else None
    grp = 8 if x.dtype == torch.bfloat16 else 4      # channels per mask byte = channels per 16-byte lane access
    mask = torch.empty((x.shape[0] * x.shape[1] * x.shape[2], x.shape[3] // grp), dtype=torch.uint8, device=x.device) if want_mask else None
    check(_lib().pm_bn_apply_mask(byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), byref(rd) if rd else None,
                                  1 if relu else 0, byref(tdesc(y)), ptr(mask), stream()), 'pm_bn_apply_mask')
    return (y, mask) if want_mask else y


def bn_apply_res_affine(x, mean, invstd, gamma, beta, r, r_mean, r_invstd, r_gamma, r_beta, relu=False, want_mask=False):
    """bn_apply(x, ..., residual=bn_apply(r, r_mean, r_invstd, r_gamma, r_beta)) in one launch: the normalised residual is never stored (fp32; same bits)."""
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    mask = torch.empty((x.shape[0] * x.shape[1] * x.shape[2], x.shape[3] // 4), dtype=torch.uint8, device=x.device) if want_mask else None
    check(_lib().pm_bn_apply_mask_affine(byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), byref(tdesc(r)), r_mean.data_ptr(),
                                         r_invstd.data_ptr(), r_gamma.data_ptr(), r_beta.data_ptr(), 1 if relu else 0, byref(tdesc(y)), ptr(mask), stream()),
          'pm_bn_apply_mask_affine')
    return (y, mask) if want_mask else y


def _bwd_sums(x, with_count, sums):
    """Where a backward reduce pass writes: `sums` (a slot of a buffer several layers share, ops._BnSums) or a new float[2c (+ 1)]; with_count: [2c] = this rank's
    element count (SyncBatchNorm all-reduces it together with the sums)."""
    c = x.shape[3]
    n = 2 * c + (1 if with_count else 0)
    if sums is None:
        sums = torch.empty(n, dtype=torch.float32, device=x.device)
    assert sums.numel() == n and sums.is_contiguous()
    if with_count:
        sums[2 * c:].fill_(float(x.shape[0] * x.shape[1] * x.shape[2]))
    return sums


def bn_bwd_apply_mask(dy, mask, x, mean, invstd, gamma, sums, count):
    """bn_bwd_apply(dy * mask, relu=0) with the mask read from bn_apply(want_mask=True)'s bytes; x: any tensor of that shape with its own statistics (fp32)."""
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(_lib().pm_bn_bwd_apply_mask(byref(tdesc(dy)), mask.data_ptr(), byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), sums.data_ptr(),
                                      float(count), byref(tdesc(dx)), stream()), 'pm_bn_bwd_apply_mask')
    return dx


def bn_bwd_reduce_mask(dy, mask, x, mean, invstd, want_gmask=True, with_count=False, sums=None):
    """bn_bwd_reduce(relu=1) with the ReLU mask read from bn_apply(want_mask=True)'s bytes instead of the forward output."""
    sums = _bwd_sums(x, with_count, sums)
    xd = tdesc(x)
    lib = _lib()
    nb = _sizes(('bn', x.shape, x.dtype), lambda: lib.pm_bn_workspace(byref(xd)))
    ws = workspace(nb, x.device)
    gm = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_gmask else None
    gd = tdesc(gm) if want_gmask else None
    check(lib.pm_bn_bwd_reduce_mask(byref(tdesc(dy)), mask.data_ptr(), byref(xd), mean.data_ptr(), invstd.data_ptr(), byref(gd) if gd else None,
                                    sums.data_ptr(), ptr(ws), nb, stream()), 'pm_bn_bwd_reduce_mask')
    return sums, gm


def scale_shift_act(x, scale, shift, residual=None, relu=False):
    """y = relu?(x * scale[c] + shift[c] + residual?) -- per-channel affine on an NHWC tensor."""
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    rd = tdesc(residual) if residual is not None else None
    check(_lib().pm_scale_shift_act(byref(tdesc(x)), scale.data_ptr(), shift.data_ptr(), byref(rd) if rd else None, 1 if relu else 0, byref(tdesc(y)), stream()),
          'pm_scale_shift_act')
    return y


def bn_bwd_reduce(dy, y, x, mean, invstd, relu, gamma=None, beta=None, want_gmask=False, with_count=False, sums=None):
    """relu: 0 / False none, 1 / True mask from the forward output y, 2 mask rebuilt from x (needs gamma, beta). -> (sums, dy * mask or None).
    with_count: sums gets a third section [2c] = this rank's element count. sums: write there instead of allocating (_bwd_sums)."""
    relu = int(relu)
    sums = _bwd_sums(x, with_count, sums)
    xd = tdesc(x)
    lib = _lib()
    nb = _sizes(('bn', x.shape, x.dtype), lambda: lib.pm_bn_workspace(byref(xd)))
    ws = workspace(nb, x.device)
    yd = tdesc(y) if relu == 1 else None
    gm = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_gmask else None
    gd = tdesc(gm) if want_gmask else None
    check(lib.pm_bn_bwd_reduce(byref(tdesc(dy)), byref(yd) if yd else None, byref(xd), mean.data_ptr(), invstd.data_ptr(), ptr(gamma), ptr(beta), relu,
                               byref(gd) if gd else None, sums.data_ptr(), ptr(ws), nb, stream()), 'pm_bn_bwd_reduce')
    return sums, gm


def bn_bwd_apply(dy, y, x, mean, invstd, gamma, sums, count, relu, want_dres, beta=None):
    relu = int(relu)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    dres = torch.empty(x.shape, dtype=x.dtype, device=x.device) if want_dres else None
    yd = tdesc(y) if relu == 1 else None
    dr = tdesc(dres) if want_dres else None
    check(_lib().pm_bn_bwd_apply(byref(tdesc(dy)), byref(yd) if yd else None, byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                 ptr(beta), sums.data_ptr(), float(count), relu, byref(tdesc(dx)), byref(dr) if dr else None, stream()), 'pm_bn_bwd_apply')
    return dx, dres


# ---- instance norm (the IBN trunks) ---------------------------------------------------------------------------------
def _instnorm_ws(lib, x):
    n, h, w, c = x.shape
    nb = _sizes(('in', x.shape), lambda: lib.pm_instnorm_workspace(n, h, w, c))
    return workspace(nb, x.device), nb


def instnorm_fwd(x, gamma, beta, eps, relu=False, out=None):
    """nn.InstanceNorm2d (+ ReLU) of an NHWC fp32 / bf16 view: per-(image, channel) statistics, biased variance -> (y, mean [n, c], invstd [n, c]). gamma / beta:
    both None (affine=False) or both float[c]. out: the view to write (may be x itself); include/pinmem_hip.h pm_instnorm_fwd."""
    d = tdesc(x)
    y = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    yd = tdesc(y)
    assert yd.dtype == d.dtype and tuple(y.shape) == tuple(x.shape), 'instnorm_fwd: out has the shape and dtype of x'
    mean = torch.empty((d.n, d.c), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    lib = _lib()
    ws, nb = _instnorm_ws(lib, x)
    check(lib.pm_instnorm_fwd(d.ptr, yd.ptr, d.n, d.h, d.w, d.c, d.pitch, yd.pitch, d.dtype, ptr(gamma), ptr(beta), float(eps), 1 if relu else 0, mean.data_ptr(),
                              invstd.data_ptr(), ptr(ws), nb, stream()), 'pm_instnorm_fwd')
    return y, mean, invstd


def instnorm_bwd(dy, x, y, gamma, mean, invstd, relu=False, want_affine=True, out=None):
    """Backward of instnorm_fwd -> (dx, dgamma, dbeta); y (the forward output) is read only when relu. dgamma / dbeta: float[c], or None when not wanted."""
    d, gd = tdesc(x), tdesc(dy)
    dx = out if out is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    xd = tdesc(dx)
    yd = tdesc(y) if relu else None
    assert gd.dtype == d.dtype == xd.dtype and tuple(dy.shape) == tuple(x.shape) == tuple(dx.shape), 'instnorm_bwd: dy and dx have the shape and dtype of x'
    assert yd is None or (yd.dtype == d.dtype and tuple(y.shape) == tuple(x.shape)), 'instnorm_bwd: y has the shape and dtype of x'
    dgamma = torch.empty(d.c, dtype=torch.float32, device=x.device) if want_affine else None
    dbeta = torch.empty_like(dgamma) if want_affine else None
    lib = _lib()
    ws, nb = _instnorm_ws(lib, x)
    check(lib.pm_instnorm_bwd(gd.ptr, d.ptr, yd.ptr if yd else None, xd.ptr, d.n, d.h, d.w, d.c, gd.pitch, d.pitch, yd.pitch if yd else 0, xd.pitch, d.dtype, ptr(gamma),
                              mean.data_ptr(), invstd.data_ptr(), 1 if relu else 0, ptr(dgamma), ptr(dbeta), ptr(ws), nb, stream()), 'pm_instnorm_bwd')
    return dx, dgamma, dbeta


def relu_bwd(dy, y):
    dx = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    check(_lib().pm_relu_bwd(byref(tdesc(dy)), byref(tdesc(y)), byref(tdesc(dx)), stream()), 'pm_relu_bwd')
    return dx


def add_n(xs):
    """Sum of 2..8 same-shape NHWC tensors in one pass."""
    from .lib import PmTensor
    from ctypes import POINTER, pointer
    descs = [tdesc(x) for x in xs]
    arr = (POINTER(PmTensor) * len(xs))(*[pointer(d) for d in descs])
    y = torch.empty(xs[0].shape, dtype=xs[0].dtype, device=xs[0].device)
    check(_lib().pm_add_n(arr, len(xs), byref(tdesc(y)), stream()), 'pm_add_n')
    return y


def add(a, b, out=None):
    y = out if out is not None else torch.empty(a.shape, dtype=a.dtype, device=a.device)
    check(_lib().pm_add(byref(tdesc(a)), byref(tdesc(b)), byref(tdesc(y)), stream()), 'pm_add')
    return y


def copy(src, dst):
    check(_lib().pm_copy(byref(tdesc(src)), byref(tdesc(dst)), stream()), 'pm_copy')
    return dst


# ---- pooling / resize / layout -------------------------------------------------------------------------------------
def maxpool_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
    arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
    check(_lib().pm_maxpool3x3s2_fwd(byref(tdesc(x)), byref(tdesc(y)), arg.data_ptr(), stream()), 'pm_maxpool3x3s2_fwd')
    return y, arg


def maxpool_bn_relu_fwd(x, mean, invstd, gamma, beta):
    """maxpool_fwd(bn_apply(x, ..., relu=True)) without the normalised tensor: -> (pooled, argmax bytes), the same bits (fp32)."""
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
    arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
    check(_lib().pm_maxpool3x3s2_bn_relu_fwd(byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), byref(tdesc(y)), arg.data_ptr(), stream()),
          'pm_maxpool3x3s2_bn_relu_fwd')
    return y, arg


def bn_bwd_reduce_pool(dyp, arg, x, mean, invstd, gamma, beta, with_count=False, sums=None):
    """bn_bwd_reduce(relu=2) whose incoming gradient is maxpool_bwd(dyp, arg), gathered inside the pass: -> local sums [sum dy | sum dy xhat (| count)] (fp32)."""
    sums = _bwd_sums(x, with_count, sums)
    xd = tdesc(x)
    lib = _lib()
    nb = _sizes(('bn', x.shape, x.dtype), lambda: lib.pm_bn_workspace(byref(xd)))
    ws = workspace(nb, x.device)
    check(lib.pm_bn_bwd_reduce_pool(byref(tdesc(dyp)), arg.data_ptr(), byref(xd), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sums.data_ptr(),
                                    ptr(ws), nb, stream()), 'pm_bn_bwd_reduce_pool')
    return sums


def bn_bwd_apply_pool(dyp, arg, x, mean, invstd, gamma, beta, sums, count):
    """bn_bwd_apply(relu=2) on the same gathered gradient -> dx; sums / count as bn_bwd_apply."""
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(_lib().pm_bn_bwd_apply_pool(byref(tdesc(dyp)), arg.data_ptr(), byref(tdesc(x)), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      sums.data_ptr(), float(count), byref(tdesc(dx)), stream()), 'pm_bn_bwd_apply_pool')
    return dx


def bn_relu_bwd_pool(dyp, arg, x, mean, invstd, gamma, beta, with_count=False):
    """Backward of relu(bn(x)) followed by the 3x3 / s2 max pool, from the pooled gradient dyp and the argmax bytes: -> (dx, local sums [sum dy | sum dy xhat (| count)]).
    = maxpool_bwd, bn_bwd_reduce(relu=2), bn_bwd_apply(relu=2) without the full-resolution gradient, on this rank alone (ops._Stem puts the exchange between the two)."""
    sums = bn_bwd_reduce_pool(dyp, arg, x, mean, invstd, gamma, beta, with_count)
    count = -1.0 if with_count else float(x.shape[0] * x.shape[1] * x.shape[2])
    return bn_bwd_apply_pool(dyp, arg, x, mean, invstd, gamma, beta, sums, count), sums


def maxpool_bwd(dy, arg, x_shape):
    dx = torch.empty(x_shape, dtype=dy.dtype, device=dy.device)
    check(_lib().pm_maxpool3x3s2_bwd(byref(tdesc(dy)), arg.data_ptr(), byref(tdesc(dx)), stream()), 'pm_maxpool3x3s2_bwd')
    return dx


def global_avgpool_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty((n, 1, 1, c), dtype=x.dtype, device=x.device)
    check(_lib().pm_global_avgpool_fwd(byref(tdesc(x)), byref(tdesc(y)), stream()), 'pm_global_avgpool_fwd')
    return y


def global_avgpool_bwd(dy, x_shape):
    dx = torch.empty(x_shape, dtype=dy.dtype, device=dy.device)
    check(_lib().pm_global_avgpool_bwd(byref(tdesc(dy)), byref(tdesc(dx)), 0, stream()), 'pm_global_avgpool_bwd')
    return dx


def resize_fwd(x, size, out=None):
    n, h, w, c = x.shape
    # pitch-padded input (zero pad lanes) -> the float4 path writes the output's pad lanes too: no zero fill of a 358 MB tensor
    own_pad = c % 4 != 0 and x.stride(2) == (c + 3) // 4 * 4
    y = out if out is not None else new((n, size[0], size[1], c), x, pitch_pad=True, zero_pad=not own_pad)
    check(_lib().pm_resize_bilinear_fwd(byref(tdesc(x)), byref(tdesc(y)), stream()), 'pm_resize_bilinear_fwd')
    return y


def resize_bwd(dy, x_shape, separable=True):
    """separable=False: the gather formulation everywhere."""
    dx = new(x_shape, dy, pitch_pad=True)
    lib, dyd, dxd = _lib(), tdesc(dy), tdesc(dx)
    nb = lib.pm_resize_bilinear_bwd_workspace(byref(dyd), byref(dxd)) if separable else 0
    if nb:      # up-sampling by >= 2: column pass + row pass, the large gradient is read once
        ws = workspace(nb, dy.device)
        check(lib.pm_resize_bilinear_bwd_separable(byref(dyd), byref(dxd), 0, ptr(ws), nb, stream()), 'pm_resize_bilinear_bwd_separable')
    else:
        check(lib.pm_resize_bilinear_bwd(byref(dyd), byref(dxd), 0, stream()), 'pm_resize_bilinear_bwd')
    return dx


def resize_hp_fwd(x, size, flip_w=False):
    """F.interpolate(mode='bilinear', align_corners=False) of an NHWC tensor, optionally un-flipping the width on the way out."""
    n, h, w, c = x.shape
    y = torch.empty((n, size[0], size[1], c), dtype=torch.float32, device=x.device)
    check(_lib().pm_resize_bilinear_hp_fwd(byref(tdesc(x)), byref(tdesc(y)), 1 if flip_w else 0, stream()), 'pm_resize_bilinear_hp_fwd')
    return y


def softmax_mean_update(logits, buffer, counter):
    check(_lib().pm_softmax_mean_update(byref(tdesc(logits)), buffer.data_ptr(), counter, stream()), 'pm_softmax_mean_update')


def sliding_stitch(logits, tiles, H, W, flip_w, acc=None):
    """logits NHWC [T, th, tw, C] of the tiles [(x1, y1, x2, y2)] -> float64 [C, H, W]: sum over covering tiles / count, un-flipped; added to `acc` if given."""
    import ctypes
    T, th, tw, c = logits.shape
    arr = (ctypes.c_int32 * (4 * T))(*[int(v) for t in tiles for v in t])
    out = acc if acc is not None else torch.empty((c, H, W), dtype=torch.float64, device=logits.device)
    check(L.load().pm_sliding_stitch(byref(tdesc(logits)), arr, T, H, W, 1 if flip_w else 0, out.data_ptr(), 1 if acc is not None else 0, stream()), 'pm_sliding_stitch')
    return out


def _sliding_outputs(C, H, W, device, labels, hist, pred, want_pred, logits_out, want_logits):
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (H, W)
        if hist is None:
            hist = torch.zeros((C, C), dtype=torch.int64, device=device)
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.is_cuda and hist.is_contiguous() and tuple(hist.shape) == (C, C)
    if pred is None and want_pred:
        pred = torch.empty((H, W), dtype=torch.uint8, device=device)
    if pred is not None:
        assert pred.dtype == torch.uint8 and pred.is_cuda and pred.is_contiguous() and tuple(pred.shape) == (H, W)
    if logits_out is None and want_logits:
        logits_out = torch.empty((C, H, W), dtype=torch.float64, device=device)
    if logits_out is not None:
        assert logits_out.dtype == torch.float64 and logits_out.is_cuda and logits_out.is_contiguous() and tuple(logits_out.shape) == (C, H, W)
    return hist, pred, logits_out


def sliding_eval(logits, tiles, scaled_hw, out_hw, flips=2, labels=None, hist=None, accumulate=True, pred=None, want_pred=False, logits_out=None,
                 want_logits=False, acc=None, acc_add=False):
    """Sliding-window evaluation of one (image, scale) from the low-res logits NHWC [flips * T, h, w, C] of the tiles [(x1, y1, x2, y2)] in the scaled image
    `scaled_hw` (the un-flipped tiles first, then the mirrored image's), include/pinmem_hip.h pm_sliding_eval.
    acc None (one scale, scaled_hw == out_hw) -> (pred, hist, logits_out): the uint8 [H, W] class map (want_pred, or `pred` to write into), hist[label][pred] (int64
    [C, C]; only with `labels`; created zeroed when None, else added to -- overwritten with accumulate=False) and the float64 [C, H, W] mean logits (want_logits).
    acc given (float64 [C, H, W]) -> acc: this scale's map resampled to out_hw as cv2.resize(INTER_LINEAR) and written to it (acc_add=False) or added
    (acc_add=True); sliding_eval_finish then yields the class map and the histogram."""
    n, h, w, C = logits.shape
    (Hs, Ws), (H, W) = scaled_hw, out_hw
    T = len(tiles)
    ld = tdesc(logits)
    assert ld.dtype == L.PM_F32, 'sliding_eval: fp32 logits'
    arr = (ctypes.c_int32 * (4 * T))(*[int(v) for t in tiles for v in t])
    if acc is None:
        hist, pred, logits_out = _sliding_outputs(C, H, W, logits.device, labels, hist, pred, want_pred, logits_out, want_logits)
    else:
        assert labels is None and pred is None and logits_out is None and not want_pred and not want_logits
        assert acc.dtype == torch.float64 and acc.is_cuda and acc.is_contiguous() and tuple(acc.shape) == (C, H, W)
    lib = _lib()
    nb = lib.pm_sliding_eval_workspace(T, C, H, W)
    ws = workspace(nb, logits.device)
    check(lib.pm_sliding_eval(logits.data_ptr(), n, h, w, C, ld.pitch, int(flips), arr, T, Hs, Ws, H, W, ptr(labels), ptr(hist) if labels is not None else None,
                              int(bool(accumulate)), ptr(pred), ptr(logits_out), ptr(acc), int(bool(acc_add)), ptr(ws), nb, stream()), 'pm_sliding_eval')
    return acc if acc is not None else (pred, hist, logits_out)


def sliding_eval_finish(acc, nscales, labels=None, hist=None, accumulate=True, pred=None, want_pred=False, logits_out=None, want_logits=False):
    """The accumulator of sliding_eval after the last scale -> (pred, hist, logits_out) as sliding_eval yields them at one scale: acc / nscales (np.mean over the
    scales, eval.py:647), its argmax and the histogram. logits_out may be `acc` itself."""
    C, H, W = acc.shape
    assert acc.dtype == torch.float64 and acc.is_cuda and acc.is_contiguous()
    hist, pred, logits_out = _sliding_outputs(C, H, W, acc.device, labels, hist, pred, want_pred, logits_out, want_logits)
    lib = _lib()
    nb = lib.pm_sliding_eval_workspace(0, C, H, W)
    ws = workspace(nb, acc.device)
    check(lib.pm_sliding_eval_finish(acc.data_ptr(), C, H, W, int(nscales), ptr(labels), ptr(hist) if labels is not None else None, int(bool(accumulate)), ptr(pred),
                                     ptr(logits_out), ptr(ws), nb, stream()), 'pm_sliding_eval_finish')
    return pred, hist, logits_out


# ---- ablation sweep (ablation.py / tsnelib.py; include/pinmem_hip.h "ablation sweep") --------------------------------------------------------------------------
def label_splat(labels, size, classes=19):
    """int64 labels [n, H, W] -> (splat fp32 [n, h, w, classes + 1], counts int64 [n, classes + 1]) for size = (h, w): the labels pushed through the transpose of the
    bilinear up-sampling h x w -> H x W (row `classes` = label 255, other values outside [0, classes) skipped) and the exact pixel counts. One splat serves every
    feature map of that size (class_sums)."""
    n, H, W = labels.shape
    h, w = int(size[0]), int(size[1])
    assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
    splat = torch.empty((n, h, w, classes + 1), dtype=torch.float32, device=labels.device)
    counts = torch.empty((n, classes + 1), dtype=torch.int64, device=labels.device)
    check(_lib().pm_label_splat(labels.data_ptr(), n, H, W, h, w, int(classes), splat.data_ptr(), counts.data_ptr(), stream()), 'pm_label_splat')
    return splat, counts


def class_sums(feat, splat):
    """feat: a logical-NCHW [n, C, h, w] tensor in channels-last memory (fp32 or bf16; may be a channel slice of a wider buffer), splat from label_splat ->
    sums fp32 [n, classes + 1, C]: per class the sum of the L2-normalised feature vectors weighted by the splat, i.e. tsnelib.py:51-65's
    matmul(upsample(normalize(feat)), one_hot(labels)) without the up-sampled map and the one-hot. sums[k] / counts[k] is the class mean vector."""
    v = feat.permute(0, 2, 3, 1)
    if v.stride(3) != 1 and v.shape[3] != 1:
        v = v.contiguous()
    d = tdesc(v)
    assert splat.dtype == torch.float32 and splat.is_cuda and splat.is_contiguous() and tuple(splat.shape[:3]) == (d.n, d.h, d.w), 'class_sums: splat is [n, h, w, classes + 1]'
    classes = splat.shape[3] - 1
    sums = torch.empty((d.n, classes + 1, d.c), dtype=torch.float32, device=feat.device)
    lib = _lib()
    nb = _sizes(('csum', d.n, d.h, d.w, d.c, classes), lambda: lib.pm_class_sums_workspace(d.n, d.h, d.w, d.c, classes))
    ws = workspace(nb, feat.device)
    check(lib.pm_class_sums(d.ptr, d.n, d.h, d.w, d.c, d.pitch, d.dtype, splat.data_ptr(), classes, sums.data_ptr(), ptr(ws), nb, stream()), 'pm_class_sums')
    return sums


ACTMAP_OUTPUTS = ('act', 'bytes', 'rgb', 'blend')


def mem_actmap(p_mem, nhw, size, slots, palette=None, image=None, alpha=0.65, want=('bytes',)):
    """The memory activation maps of ablation.py:371-399 from the LOW-RES soft-max over the memory slots. p_mem: fp32 [n * h * w, m] or [n, h, w, m] rows (row stride
    >= m), nhw = (n, h, w), size = (H, W), slots: the slot indices to map, in output order. want: any of 'act' (fp32 [n, S, H, W], the per-pixel min-max normalised
    score), 'bytes' (uint8 [n, S, H, W], np.uint8(clip * 255)), 'rgb' (uint8 [n, S, H, W, 3] = palette[bytes]; palette uint8 [256, 3] RGB) and 'blend' (uint8
    [n, S, H, W, 3] = Image.blend(image, rgb, alpha); image uint8 [n, H, W, 3]). -> dict name -> tensor."""
    n, h, w = (int(v) for v in nhw)
    H, W = int(size[0]), int(size[1])
    m = p_mem.shape[-1]
    assert p_mem.dtype == torch.float32 and p_mem.is_cuda and p_mem.numel() == n * h * w * m, 'mem_actmap: p_mem is fp32 [n * h * w, m]'
    rows = p_mem.reshape(n * h * w, m) if p_mem.dim() != 2 else p_mem
    pitch = rows.stride(0) if rows.shape[0] > 1 else m
    assert rows.stride(1) == 1 or m == 1
    want = tuple(want)
    assert want and all(k in ACTMAP_OUTPUTS for k in want), 'mem_actmap: want is a non-empty subset of %s' % (ACTMAP_OUTPUTS,)
    slots = [int(s) for s in slots]
    S = len(slots)
    dev = p_mem.device
    for name, t, shape in (('palette', palette, (256, 3)), ('image', image, (n, H, W, 3))):
        assert t is None or (t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape), 'mem_actmap: %s is uint8 %s' % (name, shape)
    res = {}
    for k in want:
        res[k] = torch.empty((n, S, H, W, 3) if k in ('rgb', 'blend') else (n, S, H, W), dtype=torch.float32 if k == 'act' else torch.uint8, device=dev)
    arr = (ctypes.c_int32 * max(S, 1))(*slots)
    check(_lib().pm_mem_actmap(rows.data_ptr(), n, h, w, m, pitch, H, W, arr, S, ptr(res.get('act')), ptr(res.get('bytes')), ptr(palette), ptr(image), float(alpha),
                               ptr(res.get('rgb')), ptr(res.get('blend')), stream()), 'pm_mem_actmap')
    return res


DUMP_OUTPUTS = ('color', 'compose', 'diff', 'ids')


def trainid_table(id_to_trainid):
    """The label-id map of eval.py:690-692 as a table: uint8 [256] on the host with table[train_id] = label_id, 0 where no entry names the value; where several
    ids share a train id the LAST one in the dict's order wins, as in the reference's loop. An entry whose train id lies outside 0 .. 255 is skipped (the reference's
    `pred == -1` never matches); one inside that range whose label id does not fit a byte raises ValueError."""
    table = torch.zeros(256, dtype=torch.uint8)
    for label_id, train_id in id_to_trainid.items():
        label_id, train_id = int(label_id), int(train_id)
        if not 0 <= train_id <= 255:
            continue
        if not 0 <= label_id <= 255:
            raise ValueError('trainid_table: label id %d (train id %d) does not fit a byte' % (label_id, train_id))
        table[train_id] = label_id
    return table


def eval_dump(pred, palette=None, image=None, labels=None, id_table=None, alpha=0.5, want=('color',)):
    """The images RunEval.inf writes under --dump_images (eval.py:664-693) from the class map of an evaluation, in one launch. pred: uint8 [H, W] or [n, H, W] on the
    device. want: any of 'color' (uint8 [..., 3] = palette[pred]; palette uint8 [256, 3] RGB), 'compose' (uint8 [..., 3] = Image.blend(image, color, alpha); image
    uint8 [..., 3]), 'diff' (uint8 [..., 3]: the compose pixel where labels != 255 and labels != pred, else white; labels int64 [...] train ids) and 'ids' (uint8
    [...] = id_table[pred]; id_table uint8 [256], see trainid_table). -> dict name -> tensor."""
    assert pred.dtype == torch.uint8 and pred.is_cuda and pred.is_contiguous() and pred.dim() in (2, 3) and pred.numel() > 0, 'eval_dump: pred is uint8 [H, W] or [n, H, W]'
    shape = tuple(pred.shape)
    want = tuple(want)
    assert want and all(k in DUMP_OUTPUTS for k in want), 'eval_dump: want is a non-empty subset of %s' % (DUMP_OUTPUTS,)
    for name, t, dtype, shp in (('palette', palette, torch.uint8, (256, 3)), ('image', image, torch.uint8, shape + (3,)), ('labels', labels, torch.int64, shape),
                                ('id_table', id_table, torch.uint8, (256,))):
        assert t is None or (t.dtype == dtype and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp), 'eval_dump: %s is %s %s' % (name, dtype, shp)
    need = dict(color=('palette',), compose=('palette', 'image'), diff=('palette', 'image', 'labels'), ids=('id_table',))
    given = dict(palette=palette, image=image, labels=labels, id_table=id_table)
    for k in want:
        for name in need[k]:
            assert given[name] is not None, 'eval_dump: %s needs %s' % (k, name)
    res = {k: torch.empty(shape if k == 'ids' else shape + (3,), dtype=torch.uint8, device=pred.device) for k in want}
    check(_lib().pm_eval_dump(pred.data_ptr(), pred.numel(), ptr(palette), ptr(image), ptr(labels), ptr(id_table), float(alpha), ptr(res.get('color')),
                              ptr(res.get('compose')), ptr(res.get('diff')), ptr(res.get('ids')), stream()), 'pm_eval_dump')
    return res


def argmax_f64(buffer):
    n, h, w, c = buffer.shape
    cls = torch.empty((n, h, w), dtype=torch.int64, device=buffer.device)
    prob = torch.empty((n, h, w), dtype=torch.float64, device=buffer.device)
    check(_lib().pm_argmax_f64(buffer.data_ptr(), n, h, w, c, cls.data_ptr(), prob.data_ptr(), stream()), 'pm_argmax_f64')
    return prob, cls


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # datasets/gtav.py:284, eval.py:128


def image_u8_to_nhwc4(img_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [N,H,W,3] -> normalised fp32 NHWC4 [N,H,W,4] (ToTensor + Normalize, zero 4th channel)."""
    import ctypes
    n, h, w, c = img_u8.shape
    assert c == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
    out = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_u8.device)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(_lib().pm_image_u8_to_nhwc4(img_u8.data_ptr(), n * h * w, m, s, out.data_ptr(), stream()), 'pm_image_u8_to_nhwc4')
    return out


def labels_u8_to_i64(lab_u8, params=None):
    """uint8 label maps -> int64. params (aug_params / upload_aug_params of the batch, lab_u8 then [N,H,W]): the columns of every image whose flip flag is set are mirrored."""
    assert lab_u8.dtype == torch.uint8 and lab_u8.is_contiguous()
    out = torch.empty(lab_u8.shape, dtype=torch.int64, device=lab_u8.device)
    if params is None:
        check(_lib().pm_labels_u8_to_i64(lab_u8.data_ptr(), lab_u8.numel(), out.data_ptr(), stream()), 'pm_labels_u8_to_i64')
        return out
    n, h, w = lab_u8.shape
    pd = upload_aug_params(params, lab_u8.device, n)
    check(_lib().pm_labels_u8_flip_to_i64(lab_u8.data_ptr(), n, h, w, pd.data_ptr(), ctypes.sizeof(L.PmAugImage), out.data_ptr(), stream()), 'pm_labels_u8_flip_to_i64')
    return out


# ---- augmenting input edge (csrc/augment.hip) ------------------------------------------------------------------------------
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = 0, 1, 2, 3      # torchvision's fn_idx values = bit positions of pm_aug_image.enabled
AUG_MAX_RADIUS = 5


def aug_blur_weights(sigma):
    """(radius, [w0 .. w5]) of scipy.ndimage's Gaussian kernel with truncate = 4.0 (host only). sigma outside (0, 1.375) raises."""
    r, w = ctypes.c_int32(), (ctypes.c_double * 6)()
    check(_lib().pm_aug_blur_weights(float(sigma), byref(r), w), 'pm_aug_blur_weights')
    return r.value, list(w)


def aug_params(n):
    """A host array of n pm_aug_image structs that do nothing: identity order, no op enabled, no flip, no blur."""
    arr = (L.PmAugImage * n)()
    for p in arr:
        p.order[:] = (0, 1, 2, 3)
        p.brightness = p.contrast = p.saturation = 1.0
    return arr


def set_aug_image(p, order=(0, 1, 2, 3), enabled=0, flip=False, hue=0.0, brightness=1.0, contrast=1.0, saturation=1.0, sigma=0.0):
    """Fill one pm_aug_image from the quantities the host pipeline draws: hue is torchvision's hue_factor in [-0.5, 0.5] (the shift is np.uint8(hue * 255) as the
    reference's numpy computed it: truncated toward zero, wrapped to a byte), sigma 0 = no blur."""
    p.order[:] = [int(o) for o in order]
    p.enabled, p.flip, p.hue_shift = int(enabled), 1 if flip else 0, int(hue * 255) & 255
    p.brightness, p.contrast, p.saturation = float(brightness), float(contrast), float(saturation)
    if sigma > 0:
        p.radius, w = aug_blur_weights(sigma)
        p.w[:] = w
    else:
        p.radius = 0
        p.w[:] = [0.0] * 6
    return p


def upload_aug_params(params, device, n=None):
    """Host pm_aug_image array -> the device copy the kernels read: checked here for what the device cannot report (order a permutation, radius <= 5), staged in
    pinned memory and copied without blocking on the current stream (no host synchronisation: the prefetcher's side stream keeps running; the pinned block returns to
    torch's host allocator, which holds it until the copy has run). A tensor that already went through here is passed on, so one upload serves image and labels."""
    size = ctypes.sizeof(L.PmAugImage)
    if isinstance(params, torch.Tensor):
        assert params.is_cuda and params.dtype == torch.uint8 and params.is_contiguous() and params.numel() % size == 0, 'not an upload_aug_params tensor'
        assert n is None or params.numel() == n * size, 'augmentation parameters for %d images, batch of %d' % (params.numel() // size, n)
        return params
    assert n is None or len(params) == n, 'augmentation parameters for %d images, batch of %d' % (len(params), n)
    for i, p in enumerate(params):
        if sorted(p.order) != [0, 1, 2, 3]:
            raise ValueError('pm_aug_image[%d].order %s is not a permutation of 0..3' % (i, list(p.order)))
        if not 0 <= p.radius <= AUG_MAX_RADIUS:
            raise ValueError('pm_aug_image[%d].radius %d outside 0..%d' % (i, p.radius, AUG_MAX_RADIUS))
    host = torch.empty(max(len(params), 1) * size, dtype=torch.uint8, pin_memory=True)
    ctypes.memmove(host.data_ptr(), ctypes.addressof(params), len(params) * size)
    return host.to(device, non_blocking=True)


def augment_u8(img_u8, params, want_u8=False, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [N,H,W,3] -> colour jitter, Gaussian blur, horizontal flip per image as `params` says (aug_params / input_edge.PhotometricAugment.sample, or their
    upload_aug_params copy), then ToTensor + Normalize: fp32 NHWC4 [N,H,W,4] with a zero 4th channel. want_u8: also the augmented uint8 pixels, (float, uint8)."""
    n, h, w, c = img_u8.shape
    assert c == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.is_cuda
    pd = upload_aug_params(params, img_u8.device, n)
    out = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_u8.device)
    out8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=img_u8.device) if want_u8 else None
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    need = _lib().pm_augment_workspace(n)
    ws = workspace(need, img_u8.device)
    check(_lib().pm_augment_u8(img_u8.data_ptr(), n, h, w, pd.data_ptr(), ctypes.sizeof(L.PmAugImage), m, s, out.data_ptr(), ptr(out8), ws.data_ptr(), need, stream()),
          'pm_augment_u8')
    return (out, out8) if want_u8 else out


# ---- resampling input edge (csrc/resample.hip) ----------------------------------------------------------------------------
class GeoParams:
    """The geometry of one batch on the host: `images`, a ctypes array of pm_geo_image (one per image: source size, resized size, pad, crop origin), the crop
    size (th, tw) all images share, and the label value of the padding. What input_edge.GeometricAugment.sample returns and resample_crop_u8 takes."""

    def __init__(self, n, crop, ignore_index=255):
        self.images = (L.PmGeoImage * n)()
        self.crop = (int(crop[0]), int(crop[1]))
        self.ignore_index = int(ignore_index)

    def __len__(self):
        return len(self.images)


class GeoDevice:
    """upload_geo's result: one uint8 device tensor holding the pm_geo_image array and the four tables of every image, and where each part starts."""

    def __init__(self, buf, n, crop, ignore_index, slab, offsets):
        self.buf, self.n, self.crop, self.ignore_index, self.slab, self.offsets = buf, n, crop, ignore_index, slab, offsets


def _geo_offsets(n, crop, with_image_table=False):
    """Byte offsets of (structs, bicubic rows, bicubic columns, nearest rows, nearest columns[, the label decode's image_table]) in the staged block, and its size."""
    th, tw = crop
    sizes = (n * ctypes.sizeof(L.PmGeoImage), n * th * L.RESAMPLE_REC * 4, n * tw * L.RESAMPLE_REC * 4, n * th * 4, n * tw * 4) + ((n * 4,) if with_image_table else ())
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs[:-1], offs[-1]


def resample_tables(g, slab, crop):
    """The four host tables of ONE pm_geo_image for a th x tw window (pm_resample_tables; no device involved): ctypes int32 arrays bic_rows [th * REC], bic_cols [tw * REC],
    near_rows [th], near_cols [tw]. Raises PinmemError for a geometry the library refuses (crop outside the padded image, image larger than its slab, too many taps)."""
    th, tw = int(crop[0]), int(crop[1])
    assert th > 0 and tw > 0, 'empty crop'
    i32 = ctypes.c_int32
    t = ((i32 * (th * L.RESAMPLE_REC))(), (i32 * (tw * L.RESAMPLE_REC))(), (i32 * th)(), (i32 * tw)())
    check(_lib().pm_resample_tables(ctypes.addressof(g), ctypes.sizeof(L.PmGeoImage), int(slab[0]), int(slab[1]), th, tw, *[ctypes.addressof(a) for a in t]), 'pm_resample_tables')
    return t


def upload_geo(geo, device, slab, image_table=None):
    """GeoParams -> GeoDevice: the library writes every image's tables straight into one pinned block behind the structs (validating each geometry against the
    [Hs, Ws] slab on the way), and the block is copied without blocking on the current stream, as upload_aug_params does. A GeoDevice is passed on.
    image_table (the label decode's table index per image, -1 = pass-through): n int32 staged behind the tables in the same block, at offsets[5]."""
    if isinstance(geo, GeoDevice):
        assert geo.slab == (int(slab[0]), int(slab[1])), 'geometry uploaded for slab %s, batch has %s' % (geo.slab, tuple(slab))
        assert image_table is None or len(geo.offsets) == 6, 'geometry uploaded without an image_table'
        return geo
    n, (th, tw) = len(geo), geo.crop
    offs, total = _geo_offsets(n, geo.crop, image_table is not None)
    host = torch.empty(max(total, 4), dtype=torch.uint8, pin_memory=True)
    base, size, lib = host.data_ptr(), ctypes.sizeof(L.PmGeoImage), _lib()
    ctypes.memmove(base, ctypes.addressof(geo.images), n * size)
    if image_table is not None:
        assert len(image_table) == n, 'image_table for %d images, geometry for %d' % (len(image_table), n)
        staged = _i32(image_table)
        ctypes.memmove(base + offs[5], ctypes.addressof(staged), n * 4)
    rec = L.RESAMPLE_REC * 4
    for i in range(n):
        check(lib.pm_resample_tables(ctypes.addressof(geo.images[i]), size, int(slab[0]), int(slab[1]), th, tw, base + offs[1] + i * th * rec, base + offs[2] + i * tw * rec,
                                     base + offs[3] + i * th * 4, base + offs[4] + i * tw * 4), 'pm_resample_tables (image %d)' % i)
    return GeoDevice(host.to(device, non_blocking=True), n, geo.crop, geo.ignore_index, (int(slab[0]), int(slab[1])), offs)


def resample_crop_u8(img_u8, lab_u8, geo):
    """RandomSizeAndCrop on the device: uint8 [N,Hs,Ws,3] images and uint8 [N,Hs,Ws] label maps (image i in the top-left h_in x w_in corner of its slab) -> the
    crop window of the bicubic-resized, padded image, uint8 [N,th,tw,3], and of the nearest-resized mask, uint8 [N,th,tw], with PIL's bytes. geo: a GeoParams
    (input_edge.GeometricAugment.sample) or its upload_geo copy."""
    n, hs, ws, c = img_u8.shape
    assert c == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.is_cuda
    assert lab_u8.shape == (n, hs, ws) and lab_u8.dtype == torch.uint8 and lab_u8.is_contiguous() and lab_u8.device == img_u8.device
    gd = upload_geo(geo, img_u8.device, (hs, ws))
    assert gd.n == n, 'geometry for %d images, batch of %d' % (gd.n, n)
    th, tw = gd.crop
    out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=img_u8.device)
    out_lab = torch.empty((n, th, tw), dtype=torch.uint8, device=img_u8.device)
    p, o = gd.buf.data_ptr(), gd.offsets
    check(_lib().pm_resample_crop_u8(img_u8.data_ptr(), lab_u8.data_ptr(), n, hs, ws, p + o[0], ctypes.sizeof(L.PmGeoImage), p + o[1], p + o[2], p + o[3], p + o[4], th, tw,
                                     gd.ignore_index, out.data_ptr(), out_lab.data_ptr(), stream()), 'pm_resample_crop_u8')
    return out, out_lab


# ---- evaluation input edge (csrc/resample.hip): scaled, mirrored, normalised sliding-window crops ---------------------------
def resize_axis_tables(n_in, n_out, filter=L.FILTER_BILINEAR):
    """PIL's coefficient records of a whole axis resized from n_in to n_out (pm_resize_axis_tables; no device involved): a ctypes int32 array [n_out * REC].
    Raises PinmemError for what the library refuses (empty sizes, an unknown filter, more taps than the records hold)."""
    rec = (ctypes.c_int32 * (max(int(n_out), 0) * L.RESAMPLE_REC))()
    check(_lib().pm_resize_axis_tables(int(n_in), int(n_out), int(filter), ctypes.addressof(rec)), 'pm_resize_axis_tables')
    return rec


class EvalTilePlan:
    """What eval_tiles_u8 needs for one (image size, scale): the scaled size (Hs, Ws) = (int(H * scale), int(W * scale)) of eval.py:357, tiles =
    harness.sliding_tiles(Hs, Ws, crop, overlap, scale) with their common size (th, tw), and ONE uint8 device tensor holding the bilinear row table, the column table
    and the tile table (offsets). The library writes the tables straight into one pinned block, the tiles are checked here (inside the scaled image, equal sizes: the
    kernel cannot report them) and the block is copied once without blocking on the current stream, as upload_geo does. uploads counts those copies."""
    uploads = 0

    def __init__(self, H, W, scale, crop, overlap, device, tiles=None):
        from .. import harness
        self.H, self.W, self.scale = int(H), int(W), float(scale)
        self.Hs, self.Ws = int(H * scale), int(W * scale)
        if self.Hs <= 0 or self.Ws <= 0:
            raise ValueError('EvalTilePlan: %d x %d at scale %g is empty' % (H, W, scale))
        # tiles: a caller's own windows (x1, y1, x2, y2) of the scaled image instead (crop and overlap are then not looked at)
        self.tiles = harness.sliding_tiles(self.Hs, self.Ws, crop, overlap, scale) if tiles is None else [tuple(int(v) for v in t) for t in tiles]
        x1, y1, x2, y2 = self.tiles[0] if self.tiles else (0, 0, 0, 0)      # eval.py:168-170 yields no tile for an axis shorter than the tile by a stride or more
        self.th, self.tw = y2 - y1, x2 - x1
        for t in self.tiles:
            if not (0 <= t[0] < t[2] <= self.Ws and 0 <= t[1] < t[3] <= self.Hs and (t[3] - t[1], t[2] - t[0]) == (self.th, self.tw)):
                raise ValueError('EvalTilePlan: tile %s outside the scaled image %d x %d or of another size than %d x %d' % (t, self.Hs, self.Ws, self.th, self.tw))
        rec, lib = L.RESAMPLE_REC * 4, _lib()
        self.offsets = (0, self.Hs * rec, (self.Hs + self.Ws) * rec)
        host = torch.empty(self.offsets[2] + len(self.tiles) * 16, dtype=torch.uint8, pin_memory=torch.device(device).type == 'cuda')
        base = host.data_ptr()
        check(lib.pm_resize_axis_tables(self.H, self.Hs, L.FILTER_BILINEAR, base + self.offsets[0]), 'pm_resize_axis_tables (rows)')
        check(lib.pm_resize_axis_tables(self.W, self.Ws, L.FILTER_BILINEAR, base + self.offsets[1]), 'pm_resize_axis_tables (columns)')
        staged = _i32([v for t in self.tiles for v in t])
        ctypes.memmove(base + self.offsets[2], ctypes.addressof(staged), len(self.tiles) * 16)
        self.buf = host.to(device, non_blocking=True)
        EvalTilePlan.uploads += 1
        self.streams = {}                   # raw handle -> every stream that read the block
        self.stream = self.event = None     # the copy's raw stream and an event behind it, for a reader on another stream
        if self.buf.is_cuda:
            self.stream, self.event = stream(), L.stream_obj().record_event()

    def use(self):
        """Called in front of a launch on the current stream that reads the block."""
        raw = stream()
        if raw not in self.streams:
            self.streams[raw] = L.stream_obj()
            if raw != self.stream:
                self.streams[raw].wait_event(self.event)

    def release(self):
        """The block leaves the cache and goes back to the pool of the stream that allocated it: tell the allocator about every stream whose queued launches may
        still read it (as _FilterCache._drop does)."""
        for s in self.streams.values():
            self.buf.record_stream(s)


class _EvalPlanCache(dict):
    """constructor arguments -> EvalTilePlan, at most EVAL_PLAN_CACHE_MAX of them, evicted in insertion order: the second image of a dataset at a scale does no host
    table work and uploads nothing."""

    def get_plan(self, H, W, scale, crop, overlap, device):
        key = (int(H), int(W), float(scale), int(crop), float(overlap), str(torch.device(device)))
        plan = self.get(key)
        if plan is None:
            plan = EvalTilePlan(H, W, scale, crop, overlap, device)      # raises before anything is evicted
            while len(self) >= EVAL_PLAN_CACHE_MAX:
                self.pop(next(iter(self))).release()
            self[key] = plan
        return plan

    def clear(self):
        while self:
            self.pop(next(iter(self))).release()


EVAL_PLAN_CACHE_MAX = 8
_EVAL_PLANS = _EvalPlanCache()
eval_tile_plan, clear_eval_tile_plans = _EVAL_PLANS.get_plan, _EVAL_PLANS.clear


def eval_tiles_u8(img_u8, plan, flips=2, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """uint8 [H, W, 3] on the device -> fp32 NHWC4 [flips * T, th, tw, 4]: the crops of plan.tiles from the image resized to (plan.Hs, plan.Ws) with the bytes of PIL's
    Image.resize(BILINEAR), normalised as image_u8_to_nhwc4 does; with flips=2 the same windows of the mirrored scaled image follow (pm_eval_tiles_u8). Neither the
    scaled image nor its mirror is written. out: a contiguous fp32 tensor of that shape to write into."""
    assert img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.is_cuda, 'a contiguous uint8 [H, W, 3] device image'
    assert tuple(img_u8.shape[:2]) == (plan.H, plan.W), 'plan for %d x %d, image %d x %d' % (plan.H, plan.W, img_u8.shape[0], img_u8.shape[1])
    assert plan.buf.device == img_u8.device, 'plan on %s, image on %s' % (plan.buf.device, img_u8.device)
    T, shape = len(plan.tiles), (int(flips) * len(plan.tiles), plan.th, plan.tw, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=img_u8.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == img_u8.device
    if T == 0:
        return out                          # an empty [0, 0, 0, 4]
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    plan.use()
    p, o = plan.buf.data_ptr(), plan.offsets
    check(_lib().pm_eval_tiles_u8(img_u8.data_ptr(), plan.H, plan.W, p + o[0], p + o[1], plan.Hs, plan.Ws, p + o[2], T, plan.th, plan.tw, int(flips), m, s, out.data_ptr(),
                                  stream()), 'pm_eval_tiles_u8')
    return out


# ---- label-decoding input edge (csrc/resample.hip) -------------------------------------------------------------------------
def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*[int(v) for v in values])


def label_table_ids(mapping):
    """{id: value} as a dataset holds it (synthia.trainid_to_trainid, cityscapes.id_to_trainid) -> a host pm_label_table (pm_label_table_ids; no device involved)."""
    items = list(dict(mapping).items())
    t, keys, vals = L.PmLabelTable(), _i32([k for k, _ in items]), _i32([v for _, v in items])
    check(_lib().pm_label_table_ids(ctypes.addressof(keys), ctypes.addressof(vals), len(items), ctypes.addressof(t), ctypes.sizeof(L.PmLabelTable)), 'pm_label_table_ids')
    return t


def label_table_colors(mapping, fill=255):
    """{(r, g, b): value} (gtav.color_to_trainid) -> a host pm_label_table (pm_label_table_colors): entries of value 255 / -1 dropped, every other colour `fill`."""
    items = list(dict(mapping).items())
    for k, _ in items:
        if len(k) != 3:
            raise ValueError('colour key %r is not an (r, g, b) triple' % (k,))
    t, rgb, vals = L.PmLabelTable(), _i32([c for k, _ in items for c in k]), _i32([v for _, v in items])
    check(_lib().pm_label_table_colors(ctypes.addressof(rgb), ctypes.addressof(vals), len(items), int(fill), ctypes.addressof(t), ctypes.sizeof(L.PmLabelTable)),
          'pm_label_table_colors')
    return t


def upload_label_tables(tables, device):
    """A list of host pm_label_table -> the uint8 device tensor the kernels read, staged in pinned memory and copied without blocking on the current stream."""
    size = ctypes.sizeof(L.PmLabelTable)
    host = torch.zeros(max(len(tables), 1) * size, dtype=torch.uint8).pin_memory()
    for i, t in enumerate(tables):
        assert isinstance(t, L.PmLabelTable)
        ctypes.memmove(host.data_ptr() + i * size, ctypes.addressof(t), size)
    return host.to(device, non_blocking=True)


def upload_image_table(image_table, device):
    """Table index per image (-1 = pass-through) -> int32 device tensor, staged in pinned memory and copied without blocking on the current stream. A tensor is passed on."""
    if isinstance(image_table, torch.Tensor):
        assert image_table.is_cuda and image_table.dtype == torch.int32 and image_table.is_contiguous(), 'not an upload_image_table tensor'
        return image_table
    host = torch.tensor([int(v) for v in image_table], dtype=torch.int32).pin_memory()
    return host.to(device, non_blocking=True)


def _label_channels(lab_u8, lead):
    """1 for a [*lead] mask, 3 for [*lead, 3]"""
    if tuple(lab_u8.shape) == tuple(lead):
        return 1
    assert tuple(lab_u8.shape) == tuple(lead) + (3,), 'label slab %s, expected %s or %s' % (tuple(lab_u8.shape), tuple(lead), tuple(lead) + (3,))
    return 3


def labels_decode_u8(lab_u8, tables_dev, image_table):
    """Colour- or id-coded masks, uint8 [N,H,W,3] or [N,H,W] -> uint8 train ids [N,H,W] (pm_labels_decode_u8). tables_dev: upload_label_tables' tensor (or
    input_edge.LabelDecode.device_tables); image_table: per image the index of its table, -1 for the pass-through (channel 0 unchanged) -- a list or its
    upload_image_table copy. A colour table on a one-channel slab gives its fill: input_edge.LabelDecode refuses that on the host."""
    assert lab_u8.dim() in (3, 4) and lab_u8.dtype == torch.uint8 and lab_u8.is_contiguous() and lab_u8.is_cuda
    n, h, w = lab_u8.shape[:3]
    c = _label_channels(lab_u8, (n, h, w))
    size = ctypes.sizeof(L.PmLabelTable)
    assert tables_dev.is_cuda and tables_dev.dtype == torch.uint8 and tables_dev.is_contiguous() and tables_dev.numel() % size == 0, 'not an upload_label_tables tensor'
    it = upload_image_table(image_table, lab_u8.device)
    assert it.numel() == n, 'image_table for %d images, batch of %d' % (it.numel(), n)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=lab_u8.device)
    check(_lib().pm_labels_decode_u8(lab_u8.data_ptr(), n, h, w, c, tables_dev.data_ptr(), tables_dev.numel() // size, size, it.data_ptr(), out.data_ptr(), stream()),
          'pm_labels_decode_u8')
    return out


def resample_crop_decode_u8(img_u8, lab_u8, geo, tables_dev, image_table):
    """resample_crop_u8 with the mask decoded in its gather (pm_resample_crop_decode_u8): lab_u8 is the raw uint8 [N,Hs,Ws,3] or [N,Hs,Ws] slab, tables_dev and
    image_table as labels_decode_u8 takes them. The label crop equals labels_decode_u8 of the whole slab followed by resample_crop_u8, the image crop resample_crop_u8's.
    image_table travels in the geometry's pinned block (upload_geo); with an uploaded GeoDevice it must have been uploaded with one."""
    n, hs, ws, c = img_u8.shape
    assert c == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.is_cuda
    assert lab_u8.dtype == torch.uint8 and lab_u8.is_contiguous() and lab_u8.device == img_u8.device
    lc = _label_channels(lab_u8, (n, hs, ws))
    size = ctypes.sizeof(L.PmLabelTable)
    assert tables_dev.is_cuda and tables_dev.dtype == torch.uint8 and tables_dev.is_contiguous() and tables_dev.numel() % size == 0, 'not an upload_label_tables tensor'
    gd = upload_geo(geo, img_u8.device, (hs, ws), image_table)
    assert gd.n == n, 'geometry for %d images, batch of %d' % (gd.n, n)
    th, tw = gd.crop
    out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=img_u8.device)
    out_lab = torch.empty((n, th, tw), dtype=torch.uint8, device=img_u8.device)
    p, o = gd.buf.data_ptr(), gd.offsets
    check(_lib().pm_resample_crop_decode_u8(img_u8.data_ptr(), lab_u8.data_ptr(), n, hs, ws, p + o[0], ctypes.sizeof(L.PmGeoImage), p + o[1], p + o[2], p + o[3], p + o[4],
                                            th, tw, gd.ignore_index, lc, tables_dev.data_ptr(), tables_dev.numel() // size, size, p + o[5], out.data_ptr(),
                                            out_lab.data_ptr(), stream()), 'pm_resample_crop_decode_u8')
    return out, out_lab


def nchw_to_nhwc(x, c_pad=None):
    n, c, h, w = x.shape
    x = x.contiguous()
    y = torch.empty((n, h, w, c_pad or c), dtype=torch.float32, device=x.device)
    check(_lib().pm_nchw_to_nhwc(x.data_ptr(), c, byref(tdesc(y)), stream()), 'pm_nchw_to_nhwc')
    return y


def nhwc_to_nchw(x):
    n, h, w, c = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(_lib().pm_nhwc_to_nchw(byref(tdesc(x)), y.data_ptr(), stream()), 'pm_nhwc_to_nchw')
    return y


def label_nearest(lab, size):
    n, H, W = lab.shape
    lab = lab.contiguous()
    out = torch.empty((n, size[0], size[1]), dtype=torch.int64, device=lab.device)
    check(_lib().pm_label_nearest(lab.data_ptr(), n, H, W, out.data_ptr(), size[0], size[1], stream()), 'pm_label_nearest')
    return out


# ---- fused upsample + loss: cross entropy plain and weighted (CrossEntropyLoss(weight) / ImageBasedCrossEntropyLoss2d, loss.py:20-43,71-88,120-180) and relaxed ----
# One private function per operation over the label forms of csrc/loss.hip. A form: the stem of its entry points, whether the logits travel as a descriptor or as
# flat arguments, the floats of loss_out for n images, and its workspace query. The weighted forms pass (weights, stride) and, 'wce' alone, per_image.
def _flat(t):
    """NHWC fp32 tensor whose pixels are `pitch` floats apart -> the flat arguments (ptr, n, h, w, C, pitch) of the pm_upsample_relax_* entry points"""
    assert t.dtype == torch.float32, 'the relaxed-border loss takes fp32 logits'
    d = tdesc(t)
    return d.ptr, d.n, d.h, d.w, d.c, d.pitch


_FORMS = {
    'ce': dict(logits=lambda lg: (byref(tdesc(lg)),), loss_floats=lambda lib, n: 2, workspace='pm_upsample_ce_workspace'),
    'wce': dict(logits=lambda lg: (byref(tdesc(lg)),), loss_floats=lambda lib, n: lib.pm_upsample_wce_loss_floats(n), workspace='pm_upsample_wce_workspace'),
    'relax': dict(logits=_flat, loss_floats=lambda lib, n: lib.pm_upsample_relax_loss_floats(n), workspace='pm_upsample_relax_workspace'),
}


def _wce_weights(weights, logits):
    """[C] (one row for the batch: stride 0) or [n, C] float32 weights -> (tensor kept alive, row stride)."""
    n, C = logits.shape[0], logits.shape[3]
    weights = weights.to(device=logits.device, dtype=torch.float32)
    if weights.dim() == 1:
        assert weights.shape[0] == C, 'expected %d class weights, got %s' % (C, tuple(weights.shape))
        return weights.contiguous(), 0
    assert weights.dim() == 2 and tuple(weights.shape) == (n, C), 'expected [%d, %d] weight rows, got %s' % (n, C, tuple(weights.shape))
    if weights.stride(1) != 1:
        weights = weights.contiguous()
    return weights, (weights.stride(0) if n > 1 else C)


def _field_floats(form, logits, H, W):
    lib = _lib()
    if form == 'relax':
        return lib.pm_upsample_relax_field_bytes(*_flat(logits)[1:5], H, W) // 4
    return lib.pm_upsample_ce_field_bytes(byref(tdesc(logits)), H, W) // 4


def _loss_fwd(form, logits, labels, inv_temp, weights, per_image, out, want_field):
    """-> loss_out, or (loss_out, field) for the training forward. labels: int64 labels, or ('relax') int32 set words."""
    n, H, W = labels.shape
    F, lib = _FORMS[form], _lib()
    if form == 'relax':
        assert labels.dtype == torch.int32 and labels.is_contiguous() and n == logits.shape[0]
    need = F['loss_floats'](lib, n)
    if out is None:
        out = torch.empty(need, dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= need
    largs = F['logits'](logits)
    field = torch.empty(_field_floats(form, logits, H, W), dtype=torch.float32, device=logits.device) if want_field else None
    nb = getattr(lib, F['workspace'])(n, H, W)
    ws = workspace(nb, logits.device)
    wargs = ()
    if weights is not None:
        wt, stride = _wce_weights(weights, logits)
        wargs = (wt.data_ptr(), stride) + ((int(bool(per_image)),) if form == 'wce' else ())
    name = 'pm_upsample_%s_fwd%s' % (form, '_field' if want_field else '')
    fargs = (field.data_ptr(),) if want_field else ()
    check(getattr(lib, name)(*largs, inv_temp, labels.data_ptr(), H, W, *wargs, out.data_ptr(), *fargs, ptr(ws), nb, stream()), name)
    return (out, field) if want_field else out


def _ce_dlogits(logits):
    return new(tuple(logits.shape), logits, pitch_pad=(logits.stride(2) != logits.shape[3]))   # same pitch as the logits


def _loss_bwd_field(form, logits, label_hw, loss_out, field, gscale, inv_temp, per_image=None):
    H, W = label_hw
    dl = _ce_dlogits(logits)
    name = 'pm_upsample_%s_bwd_field' % form
    tail = (loss_out.data_ptr(), ptr(gscale), field.data_ptr())
    if form == 'relax':      # flat arguments: the shape first, dlogits and its pitch last
        dptr, n, h, w, C, dpitch = _flat(dl)
        args = (n, h, w, C, inv_temp, H, W) + tail + (dptr, dpitch)
    else:
        args = (byref(tdesc(logits)), inv_temp, H, W) + ((int(bool(per_image)),) if form == 'wce' else ()) + tail + (byref(tdesc(dl)),)
    check(getattr(_lib(), name)(*args, stream()), name)
    return dl


def upsample_ce_fwd(logits, labels, inv_temp=1.0):
    return _loss_fwd('ce', logits, labels, inv_temp, None, None, None, False)


def upsample_ce_bwd(logits, labels, loss_out, gscale, inv_temp=1.0):
    """The backward after upsample_ce_fwd: the field is rebuilt in the workspace by a second sweep over labels and logits."""
    n, H, W = labels.shape
    dl = _ce_dlogits(logits)
    lib, ld = _lib(), tdesc(logits)
    nb = lib.pm_upsample_ce_bwd_workspace(byref(ld), H, W)
    ws = workspace(nb, logits.device)
    check(lib.pm_upsample_ce_bwd(byref(ld), inv_temp, labels.data_ptr(), H, W, loss_out.data_ptr(), ptr(gscale), byref(tdesc(dl)), ptr(ws), nb, stream()),
          'pm_upsample_ce_bwd')
    return dl


def upsample_ce_fused_ok(logits, label_hw):
    """Can the fused up-sample + CE kernels take this shape (two low-res logit rows + one label row in LDS: up to ~1000 low-res columns at 19 classes)?"""
    return _sizes(('ce', logits.shape, logits.stride(), tuple(label_hw)), lambda: _lib().pm_upsample_ce_field_bytes(byref(tdesc(logits)), label_hw[0], label_hw[1])) != 0


def upsample_ce_fwd_field(logits, labels, inv_temp=1.0):
    """Training forward: -> (loss_out[2], field). The field is what upsample_ce_bwd_field needs instead of a second sweep over labels and logits."""
    return _loss_fwd('ce', logits, labels, inv_temp, None, None, None, True)


def upsample_ce_bwd_field(logits, label_hw, loss_out, field, gscale, inv_temp=1.0):
    return _loss_bwd_field('ce', logits, label_hw, loss_out, field, gscale, inv_temp)


def upsample_wce_fwd(logits, labels, weights, per_image, inv_temp=1.0, out=None):
    """-> loss_out[2 + n]: [0] the loss, [1] the total weight sum, [2 + b] the weight sum of image b (include/pinmem_hip.h)."""
    return _loss_fwd('wce', logits, labels, inv_temp, weights, per_image, out, False)


def upsample_wce_fwd_field(logits, labels, weights, per_image, inv_temp=1.0, out=None):
    """Training forward: -> (loss_out[2 + n], field); the field has the layout and size of upsample_ce_fwd_field's."""
    return _loss_fwd('wce', logits, labels, inv_temp, weights, per_image, out, True)


def upsample_wce_bwd_field(logits, label_hw, loss_out, field, gscale, per_image, inv_temp=1.0):
    return _loss_bwd_field('wce', logits, label_hw, loss_out, field, gscale, inv_temp, per_image)


def label_class_weights(labels, classes, upper_bound=1.0, norm=False, per_batch=False, out=None):
    """ImageBasedCrossEntropyLoss2d.calculate_weights on the device: int64 labels [n,H,W] -> float32 [n, classes] weight rows, bit-equal to the numpy
    expression, without a host sync (per_batch: the batch histogram in every row). `out`: a contiguous float32 buffer of at least n * classes elements."""
    n, H, W = labels.shape
    labels = labels.contiguous()
    assert labels.dtype == torch.int64 and labels.is_cuda
    if out is None:
        out = torch.empty((n, classes), dtype=torch.float32, device=labels.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * classes
    lib = _lib()
    nb = lib.pm_label_class_weights_workspace(n)
    ws = workspace(nb, labels.device)
    check(lib.pm_label_class_weights(labels.data_ptr(), n, H, W, classes, float(upper_bound), int(bool(norm)), int(bool(per_batch)), out.data_ptr(), ptr(ws), nb,
                                     stream()), 'pm_label_class_weights')
    return out


# ---- relaxed-border training (--jointwtborder): border sets as uint32 words, their class weights, fused up-sample + ImgWtLossSoftNLL (loss.py:182-263) -----------
# Bit words travel as int32 tensors (torch has no arithmetic on uint32): bit c = class c, bit `classes` = the ignore class.
def relax_border_bits(labels, classes, border=1, strict_mask=0, out=None):
    """int64 labels [n,H,W] -> int32 words [n,H,W]: the classes of the (2 border + 1)^2 window around every pixel (RelaxedBoundaryLossToTensor on the device)."""
    n, H, W = labels.shape
    labels = labels.contiguous()
    assert labels.dtype == torch.int64 and labels.is_cuda
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.int32, device=labels.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n * H * W
    check(_lib().pm_relax_border_bits(labels.data_ptr(), n, H, W, classes, int(border), int(strict_mask) & 0xFFFFFFFF, out.data_ptr(), stream()), 'pm_relax_border_bits')
    return out


def multihot_to_bits(multihot, out=None):
    """the reference's uint8 target [n, classes + 1, H, W] (non-zero = set) -> the words of relax_border_bits"""
    n, planes, H, W = multihot.shape
    multihot = multihot.contiguous()
    assert multihot.dtype == torch.uint8 and multihot.is_cuda
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.int32, device=multihot.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n * H * W
    check(_lib().pm_multihot_to_bits(multihot.data_ptr(), n, planes, H, W, out.data_ptr(), stream()), 'pm_multihot_to_bits')
    return out


def relax_class_weights(bits, classes, upper_bound=1.0, norm=False, per_batch=False, out=None):
    """ImgWtLossSoftNLL.calculate_weights on the device: words [n,H,W] -> float32 [n, classes] weight rows, bit-equal to the numpy expression, no host sync."""
    n, H, W = bits.shape
    assert bits.dtype == torch.int32 and bits.is_cuda and bits.is_contiguous()
    if out is None:
        out = torch.empty((n, classes), dtype=torch.float32, device=bits.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * classes
    lib = _lib()
    nb = lib.pm_relax_class_weights_workspace(n)
    ws = workspace(nb, bits.device)
    check(lib.pm_relax_class_weights(bits.data_ptr(), n, H, W, classes, float(upper_bound), int(bool(norm)), int(bool(per_batch)), out.data_ptr(), ptr(ws), nb, stream()),
          'pm_relax_class_weights')
    return out


def upsample_relax_ok(logits, label_hw):
    """Can the fused relaxed-loss field kernel take this shape (two low-res logit rows + one row of set words in LDS)?"""
    n, h, w, C = logits.shape
    if logits.dtype != torch.float32:      # fp32 tensors only, as pm_upsample_ce_field_bytes answers: the caller composes resize + loss
        return False
    return _sizes(('relax', logits.shape, tuple(label_hw)), lambda: _lib().pm_upsample_relax_field_bytes(n, h, w, C, label_hw[0], label_hw[1])) != 0


def upsample_relax_fwd(logits, bits, weights, inv_temp=1.0, out=None):
    """-> loss_out[2 + 2n]: [0] the loss, [1] the valid pixels, [2 + i] the loss of image i, [2 + n + i] (valid_i + 1) n (include/pinmem_hip.h)."""
    return _loss_fwd('relax', logits, bits, inv_temp, weights, None, out, False)


def upsample_relax_fwd_field(logits, bits, weights, inv_temp=1.0, out=None):
    """Training forward: -> (loss_out[2 + 2n], field)."""
    return _loss_fwd('relax', logits, bits, inv_temp, weights, None, out, True)


def upsample_relax_bwd_field(logits, label_hw, loss_out, field, gscale, inv_temp=1.0):
    return _loss_bwd_field('relax', logits, label_hw, loss_out, field, gscale, inv_temp)


# ---- validation sweep: loss + argmax + confusion matrix of the up-sampled logits (train.py:847-939) -------------------------------
def upsample_eval_ok(logits, label_hw):
    """Can the validation kernel take this shape (two low-res logit rows in LDS: up to ~1000 low-res columns at 19 classes)?"""
    return _sizes(('eval', logits.shape, logits.stride(), tuple(label_hw)), lambda: _lib().pm_upsample_eval_workspace(byref(tdesc(logits)), label_hw[0], label_hw[1])) != 0


def upsample_eval(logits, labels, inv_temp=1.0, hist=None, want_pred=False, accumulate=True, pred=None):
    """-> (loss_out[2], hist, pred or None): mean CE (ignore 255) and valid count as upsample_ce_fwd, the confusion matrix hist[label][prediction] (int64 [C, C]; created
    zeroed when None, else added to -- overwritten with accumulate=False) and, with want_pred, the uint8 [n, H, W] class map (`pred`: a buffer to write it into)."""
    n, H, W = labels.shape
    C = logits.shape[3]
    assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
    if hist is None:
        hist = torch.zeros((C, C), dtype=torch.int64, device=logits.device)
    assert hist.dtype == torch.int64 and hist.is_cuda and hist.is_contiguous() and tuple(hist.shape) == (C, C)
    if pred is None and want_pred:
        pred = torch.empty((n, H, W), dtype=torch.uint8, device=logits.device)
    if pred is not None:
        assert pred.dtype == torch.uint8 and pred.is_cuda and pred.is_contiguous() and tuple(pred.shape) == (n, H, W)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    lib, ld = _lib(), tdesc(logits)
    nb = lib.pm_upsample_eval_workspace(byref(ld), H, W)
    ws = workspace(nb, logits.device)
    check(lib.pm_upsample_eval(byref(ld), inv_temp, labels.data_ptr(), H, W, out.data_ptr(), hist.data_ptr(), int(bool(accumulate)), ptr(pred), ptr(ws), nb,
                               stream()), 'pm_upsample_eval')
    return out, hist, pred


# ---- memory ---------------------------------------------------------------------------------------------------------
def mem_read_fwd(x, mem, noise=None):
    n, h, w, d = x.shape
    m = mem.shape[0]
    qr = torch.empty((n, h, w, 2 * d), dtype=torch.float32, device=x.device)
    score = torch.empty((n * h * w, m), dtype=torch.float32, device=x.device)
    pmem = torch.empty_like(score)
    check(_lib().pm_mem_read_fwd(byref(tdesc(x)), mem.data_ptr(), m, ptr(noise), byref(tdesc(qr)), score.data_ptr(), pmem.data_ptr(), stream()), 'pm_mem_read_fwd')
    return qr, score, pmem


def mem_read_fwd_pq(x, mem, noise=None, noise_q=None):
    """mem_read_fwd + the softmax over all queries (p_query) from the read kernel's column partials: two launches instead of three."""
    n, h, w, d = x.shape
    m = mem.shape[0]
    qr = torch.empty((n, h, w, 2 * d), dtype=torch.float32, device=x.device)
    score = torch.empty((n * h * w, m), dtype=torch.float32, device=x.device)
    pmem, pq = torch.empty_like(score), torch.empty_like(score)
    lib = _lib()
    nb = lib.pm_mem_read_fwd_pq_workspace(n * h * w, m)
    ws = workspace(nb, x.device)
    check(lib.pm_mem_read_fwd_pq(byref(tdesc(x)), mem.data_ptr(), m, ptr(noise), ptr(noise_q), byref(tdesc(qr)), score.data_ptr(), pmem.data_ptr(), pq.data_ptr(),
                                 ptr(ws), nb, stream()), 'pm_mem_read_fwd_pq')
    return qr, score, pmem, pq


def mem_colsoftmax(score, noise=None):
    rows, m = score.shape
    out = torch.empty_like(score)
    lib = _lib()
    nb = lib.pm_mem_colsoftmax_workspace(rows, m)
    ws = workspace(nb, score.device)
    check(lib.pm_mem_colsoftmax(score.data_ptr(), ptr(noise), rows, m, out.data_ptr(), ptr(ws), nb, stream()), 'pm_mem_colsoftmax')
    return out


def mem_read_bwd(x, mem, pmem, dqr, dscore_extra=None, want_dmem=False):
    n, h, w, d = x.shape
    m = mem.shape[0]
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dmem = torch.empty_like(mem) if want_dmem else None
    lib = _lib()
    nb = lib.pm_mem_read_bwd_workspace(n * h * w, m, d) if want_dmem else 0
    ws = workspace(nb, x.device) if nb else None
    check(lib.pm_mem_read_bwd(byref(tdesc(x)), mem.data_ptr(), m, pmem.data_ptr(), byref(tdesc(dqr)), ptr(dscore_extra), byref(tdesc(dx)), ptr(dmem),
                              ptr(ws), nb, stream()), 'pm_mem_read_bwd')
    return dx, dmem


def mem_write_accum(z, labels, m, normalize=True):
    n, H, W = labels.shape
    d = z.shape[3]
    nomden = torch.empty((m + 1) * (d + 1), dtype=torch.float32, device=z.device)
    zd = tdesc(z)
    lib = _lib()
    nb = lib.pm_mem_write_accum_workspace(byref(zd), m)
    ws = workspace(nb, z.device)
    check(lib.pm_mem_write_accum(byref(zd), labels.data_ptr(), H, W, m, 1 if normalize else 0, nomden.data_ptr(), ptr(ws), nb, stream()), 'pm_mem_write_accum')
    return nomden


def mem_write_accum_bwd(z, labels, m, dnom, normalize=True):
    n, H, W = labels.shape
    dz = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    check(_lib().pm_mem_write_accum_bwd(byref(tdesc(z)), labels.data_ptr(), H, W, m, 1 if normalize else 0, dnom.data_ptr(), byref(tdesc(dz)), stream()),
          'pm_mem_write_accum_bwd')
    return dz


def mem_write_update(mem, nomden, momentum, want_u=False):
    m, d = mem.shape
    out = torch.empty_like(mem)
    u = torch.empty_like(mem) if want_u else None
    check(_lib().pm_mem_write_update(mem.data_ptr(), nomden.data_ptr(), m, d, momentum, out.data_ptr(), ptr(u), stream()), 'pm_mem_write_update')
    return out, u


def mem_write_update_bwd(u, nomden, momentum, dout):
    m, d = u.shape
    dnom = torch.empty((m + 1, d), dtype=torch.float32, device=u.device)
    check(_lib().pm_mem_write_update_bwd(u.data_ptr(), nomden.data_ptr(), m, d, momentum, dout.data_ptr(), dnom.data_ptr(), None, stream()),
          'pm_mem_write_update_bwd')
    return dnom


def sgd_momentum(param, grad, buf, lr, momentum, wd, first):
    check(_lib().pm_sgd_momentum(param.data_ptr(), grad.data_ptr(), buf.data_ptr(), param.numel(), lr, momentum, wd, 1 if first else 0, stream()), 'pm_sgd_momentum')


def sgd_momentum_multi(triples, lr, momentum, wd, lr_device=None):
    """triples: [(param, grad, momentum_buffer)] of same-layout dense fp32 CUDA tensors; updated in place by a few launches.
    lr_device: a one-element fp32 CUDA tensor the kernel reads the learning rate from (captured steps); `lr` is then ignored."""
    arr = (L.PmSgdEntry * len(triples))()
    for i, (p, g, m) in enumerate(triples):
        arr[i].param, arr[i].grad, arr[i].momentum_buffer, arr[i].numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel()
    check(_lib().pm_sgd_momentum_multi_dev(arr, len(triples), lr, ptr(lr_device), momentum, wd, stream()), 'pm_sgd_momentum_multi')


def set_winograd(mode):
    """Winograd route of the wide stride-1 3x3 convs: 4 / True = prefer F(4x4,3x3) (default), 2 = F(2x2,3x3) only, 0 / False = direct."""
    mode = 4 if mode is True else (0 if mode is False else int(mode))
    check(_lib().pm_set_winograd(mode), 'pm_set_winograd')
    _GEN[0] += 1


def set_winograd_fused(on):
    """F(4x4) layers: GEMMs + output transform in one kernel (opt-in; slower than the two-pass form on the flagship layers)."""
    check(_lib().pm_set_winograd_fused(1 if on else 0), 'pm_set_winograd_fused')
    _GEN[0] += 1


def set_conv16(on):
    """bf16 tier, forward / stride-1 data gradient: 1 = per shape (default: the LDS-DMA kernels where they win), 2 = LDS-DMA everywhere on the narrow tiles,
    0 = register-staged everywhere; 3 / 7 / 8 = the wide kernels wherever the shape allows (persistent ring / 256 x 256 / ring with one block per tile), 4-6 A/B
    routes (include/pinmem_hip.h pm_set_conv16)."""
    check(_lib().pm_set_conv16(int(on)), 'pm_set_conv16')
    _GEN[0] += 1


def set_wgrad16(on):
    """bf16 tier, weight gradient of bf16 x / dy: True (default) = the LDS-DMA persistent ring (csrc/wgrad16.hip) where the shape allows, False = register-staged everywhere."""
    check(_lib().pm_set_wgrad16(1 if on else 0), 'pm_set_wgrad16')
    _GEN[0] += 1


def routing(**fields):
    """The library's routing state (include/pinmem_hip.h pm_routing) as a dict; keyword arguments replace fields -- ONE pm_routing_set call, the form a production caller
    uses (once, before the first convolution). Returns the state before the change."""
    from .lib import PmRouting
    r = PmRouting()
    r.struct_size = ctypes.sizeof(PmRouting)
    check(_lib().pm_routing_get(byref(r)), 'pm_routing_get')
    before = {k: getattr(r, k) for k, _ in PmRouting._fields_ if k != 'struct_size'}
    if fields:
        for k, v in fields.items():
            if k not in before:
                raise KeyError('pm_routing has no field %r' % k)
            setattr(r, k, int(v))
        check(_lib().pm_routing_set(byref(r)), 'pm_routing_set')
        _GEN[0] += 1
    return before


def set_split(on):
    """fp32 tier: True (default) = eligible fp32 convolutions / Winograd GEMMs on the bf16 matrix pipe (three-way exact bf16 split, six products, fp32 accumulation:
    csrc/conv_split.hip), False = the fp32-MFMA kernel everywhere."""
    check(_lib().pm_set_split(1 if on else 0), 'pm_set_split')
    _GEN[0] += 1


def set_bf16_wgrad(on):
    check(_lib().pm_set_bf16_wgrad(1 if on else 0), 'pm_set_bf16_wgrad')
    _GEN[0] += 1


def profile_enable(on):
    check(_lib().pm_profile_enable(1 if on else 0), 'pm_profile_enable')


def profile_dump(path):
    check(_lib().pm_profile_dump(str(path).encode()), 'pm_profile_dump')


def profile_read_bytes(mode=-1, bm=-1, bn=-1, km=-1, nst=-1, prec=-1):
    """-> algorithmic HBM bytes (operands once + output) summed over the recorded launches of one instantiation: what bench.py's roofline.traffic is held against."""
    b = ctypes.c_double(0)
    check(_lib().pm_profile_read_bytes(mode, bm, bn, km, nst, prec, byref(b)), 'pm_profile_read_bytes')
    return b.value


def profile_read(mode=-1, bm=-1, bn=-1, km=-1, nst=-1, clear=False, prec=-1):
    """-> (total_ms, total_flops, launches) of the conv_igemm_kernel<mode, bm, bn, .., km, prec, nst> launches recorded since the last clear."""
    import ctypes
    ms, fl, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
    check(_lib().pm_profile_read_prec(mode, bm, bn, km, nst, prec, byref(ms), byref(fl), byref(n), 1 if clear else 0), 'pm_profile_read_prec')
    return ms.value, fl.value, n.value
