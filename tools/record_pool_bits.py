"""Records the output bits of the pooling, resize and elementwise entry points (csrc/pool_resize.hip, csrc/misc.hip, pm_cast in csrc/bf16.hip) on both element types
into tests/golden/pool_bits.json; tests/test_pool_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_pool_bits.py

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. The workspace answers and the
refusals are pure host code and are recorded on any machine; the digests need the GPU and are kept as they are when there is none. Every output is fixed-order and
deterministic, so a digest (sha256 of the output's bytes) either matches or the change altered a bit.

The library is called directly (ctypes), so both `accumulate` values are recorded where the wrappers of hip/kernels.py fix it to 0. Inputs come from CPU generators
with fixed seeds. A call the library turns down is recorded as 'refused:<code>'; EXPECT_REFUSED names the only calls for which that may happen."""
import hashlib
import json
import os
import sys
from ctypes import POINTER, byref, c_void_p, pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'pool_bits.json')
DTYPES = ('f32', 'bf16')
BIG = (2, 384, 384, 64)      # more than the 8192 blocks of the grid-stride kernels and the 4096 of the elementwise drivers at both vector widths

# (name, kind, arguments, element types)
POOL_CASES = [
    ('pool-21x18', 'pool', dict(shape=(2, 21, 18), c=8), DTYPES),                      # odd, ragged window rows; one bf16 group, two fp32 groups
    ('pool-8x8-c72', 'pool', dict(shape=(1, 8, 8), c=72), DTYPES),
    ('pool-1x5', 'pool', dict(shape=(2, 1, 5), c=8), DTYPES),                          # a single row
    ('pool-pitch', 'pool', dict(shape=(2, 9, 7), c=8, pad=8), DTYPES),                 # pitch = C + 8 on every tensor
    ('pool-c19-scalar', 'pool', dict(shape=(1, 9, 7), c=19), ('f32',)),
    ('pool-relu-ties', 'pool', dict(shape=(1, 10, 9), c=8, fill='relu'), DTYPES),      # windows tie at zero
    ('pool-nan', 'pool', dict(shape=(1, 7, 7), c=8, fill='nan'), DTYPES),
    ('pool-neg-inf', 'pool', dict(shape=(1, 7, 7), c=8, fill='-inf'), DTYPES),
    ('pool-argmax-unaligned', 'pool', dict(shape=(1, 6, 5), c=8, arg_offset=1), DTYPES),   # fp32: forward takes it, backward takes the scalar route; bf16: refused
    ('pool-bn-13x11', 'pool_bn', dict(shape=(2, 13, 11), c=8), ('f32',)),
    ('pool-big', 'pool', dict(shape=BIG[:3], c=BIG[3]), DTYPES),
]
GAP_CASES = [('gap-hw%d' % (h * w), 'gap', dict(shape=(2, h, w), cs=(8, 72, 136)), DTYPES)      # fewer pixels than row lanes / the tail loop only / main loop + tail
             for h, w in ((1, 1), (3, 5), (7, 9), (10, 20))] + [('gap-big', 'gap', dict(shape=BIG[:3], cs=(BIG[3],), fwd=False), DTYPES)]
RESIZE_CASES = [
    ('resize-12x12-48x48', 'resize', dict(lo=(12, 12), hi=(48, 48)), DTYPES),
    ('resize-11x7-30x41', 'resize', dict(lo=(11, 7), hi=(30, 41)), DTYPES),
    ('resize-50x70-13x18', 'resize', dict(lo=(50, 70), hi=(13, 18)), DTYPES),          # down-sampling
    ('resize-10x10-10x10', 'resize', dict(lo=(10, 10), hi=(10, 10)), DTYPES),
    ('resize-1x1-12x12', 'resize', dict(lo=(1, 1), hi=(12, 12)), DTYPES),              # backward: the column-sum route
    ('resize-12x12-1x1', 'resize', dict(lo=(12, 12), hi=(1, 1)), DTYPES),              # scale 0
    ('resize-6x6-96x96', 'resize', dict(lo=(6, 6), hi=(96, 96)), DTYPES),              # backward window past MAXT: the generic loop
    ('resize-ratio2-one-way', 'resize', dict(lo=(12, 12), hi=(24, 18)), DTYPES),       # separable: workspace 0, refused
    ('resize-slice', 'resize', dict(lo=(5, 6), hi=(11, 13), c=64, slice_of=128), DTYPES),   # forward writes the upper 64 channels of a 128-channel buffer
    ('resize-c19-padded', 'resize', dict(lo=(7, 5), hi=(15, 12), c=19, pad=1), ('f32',)),   # the padded-lane float4 path, pad lane digested too
    ('resize-c19-scalar', 'resize', dict(lo=(7, 5), hi=(15, 12), c=19), ('f32',)),
    ('resize-1x1-c19', 'resize', dict(lo=(1, 1), hi=(9, 11), c=19), ('f32',)),         # backward: the generic loop over the whole map
    ('resize-big-up', 'resize', dict(lo=(192, 192), hi=BIG[1:3], c=BIG[3], gather=False), DTYPES),      # forward and separable backward
    ('resize-big-down', 'resize', dict(lo=BIG[1:3], hi=(96, 96), c=BIG[3], fwd=False), DTYPES),         # gather backward over the large side
]
EW_CASES = [
    ('add', 'add', dict(shape=(2, 5, 7), c=24, pads=(0, 8, 16)), DTYPES),              # add, add_n at n = 2, 5, 8; operands of different pitches
    ('add-c19', 'add', dict(shape=(2, 5, 7), c=19, pads=(0, 0, 0), ns=()), ('f32',)),
    ('copy-slice', 'copy', dict(shape=(2, 5, 7), c=16, slice_of=32, slice_at=8), DTYPES),
    ('copy-c19', 'copy', dict(shape=(2, 5, 7), c=19), ('f32',)),
    ('ew-big', 'ew_big', dict(), DTYPES),
    ('cast', 'cast', dict(shape=(2, 5, 7)), ('f32',)),                                 # both ways, vector (a channel slice) and odd (19 channels)
    ('cast-big', 'cast', dict(shape=BIG[:3], cs=(BIG[3],)), ('f32',)),
]
CASES = POOL_CASES + GAP_CASES + RESIZE_CASES + EW_CASES
RUNS = [(c, dt) for c in CASES for dt in c[3]]
# calls recorded as refused, and nothing else: case/dtype -> calls
EXPECT_REFUSED = {
    'pool-argmax-unaligned/bf16': {'maxpool_fwd': -1, 'maxpool_bwd': -1},
    'resize-ratio2-one-way/f32': {'resize_bwd_separable[acc=0]': -4, 'resize_bwd_separable[acc=1]': -4},
    'resize-ratio2-one-way/bf16': {'resize_bwd_separable[acc=0]': -4, 'resize_bwd_separable[acc=1]': -4},
}

# pm_resize_bilinear_bwd_workspace: (name, n, dy hw, dx hw, c, pitch pad): the small cases, the workload's shapes, ineligible pairs
WORKSPACE_SHAPES = [('12x12<-48x48', 2, (48, 48), (12, 12), 8, 0), ('6x6<-96x96', 2, (96, 96), (6, 6), 8, 0), ('ratio-2-one-way', 2, (24, 18), (12, 12), 8, 0),
                    ('1x1-source', 2, (12, 12), (1, 1), 8, 0), ('same-size', 2, (10, 10), (10, 10), 8, 0), ('padded-pitch', 2, (48, 48), (12, 12), 8, 8),
                    ('c19', 2, (48, 48), (12, 12), 19, 1), ('decoder', 8, (192, 192), (48, 48), 256, 0), ('logits', 8, (768, 768), (192, 192), 19, 1),
                    ('logits-c24', 8, (768, 768), (192, 192), 24, 0)]


def _types(L, dt):
    import torch
    return (torch.float32, L.PM_F32) if dt == 'f32' else (torch.bfloat16, L.PM_BF16)


def workspaces(lib, L):
    """-> {shape: [fp32 answer, bf16 answer, answer for an fp32 dy with a bf16 dx, answer for a misaligned fp32 dy]} (fake pointers: the query never dereferences)."""
    out = {}
    for name, n, (H, W), (h, w), c, pad in WORKSPACE_SHAPES:
        def ask(dt_dy, dt_dx, ptr=0x10000):
            return lib.pm_resize_bilinear_bwd_workspace(byref(L.PmTensor(ptr, n, H, W, c, c + pad, dt_dy, 0)), byref(L.PmTensor(0x20000, n, h, w, c, c + pad, dt_dx, 0)))
        out[name] = [ask(L.PM_F32, L.PM_F32), ask(L.PM_BF16, L.PM_BF16), ask(L.PM_F32, L.PM_BF16), ask(L.PM_F32, L.PM_F32, 0x10004)]
    return out


def refusals(lib, L):
    """Calls the library has to turn down before any launch -> {call: status}. The descriptors are fakes with n = 0, so a call that is wrongly accepted finds no work
    (but for the one that asks for a workspace it is not given)."""
    f32, b16, p = L.PM_F32, L.PM_BF16, c_void_p

    def t(dt, h, w, c=16, pitch=None, addr=0x100000):
        return byref(L.PmTensor(addr, 0, h, w, c, c if pitch is None else pitch, dt, 0))
    arg, ws = p(0x200000), p(0x300000)
    out = {}
    for a, b in ((f32, b16), (b16, f32)):      # a mixed-type call
        k = 'mixed[%d,%d]/' % (a, b)
        out[k + 'maxpool_fwd'] = lib.pm_maxpool3x3s2_fwd(t(a, 8, 8), t(b, 4, 4), arg, None)
        out[k + 'maxpool_bwd'] = lib.pm_maxpool3x3s2_bwd(t(a, 4, 4), arg, t(b, 8, 8), None)
        out[k + 'global_avgpool_fwd'] = lib.pm_global_avgpool_fwd(t(a, 8, 8), t(b, 1, 1), None)
        out[k + 'global_avgpool_bwd'] = lib.pm_global_avgpool_bwd(t(a, 1, 1), t(b, 8, 8), 0, None)
        out[k + 'resize_fwd'] = lib.pm_resize_bilinear_fwd(t(a, 4, 4), t(b, 8, 8), None)
        out[k + 'resize_bwd'] = lib.pm_resize_bilinear_bwd(t(a, 8, 8), t(b, 4, 4), 0, None)
        out[k + 'resize_bwd_separable'] = lib.pm_resize_bilinear_bwd_separable(t(a, 8, 8), t(b, 4, 4), 0, ws, 1 << 20, None)
        out[k + 'copy'] = lib.pm_copy(t(a, 8, 8), t(b, 8, 8), None)
        out[k + 'add[operand,output]'] = lib.pm_add(t(a, 8, 8), t(a, 8, 8), t(b, 8, 8), None)
        two = (POINTER(L.PmTensor) * 2)(pointer(L.PmTensor(0x100000, 0, 8, 8, 16, 16, a, 0)), pointer(L.PmTensor(0x100000, 0, 8, 8, 16, 16, a, 0)))
        out[k + 'add_n[operands,output]'] = lib.pm_add_n(two, 2, t(b, 8, 8), None)
    for dt, tag in ((f32, 'f32'), (b16, 'bf16')):
        one = (POINTER(L.PmTensor) * 2)(pointer(L.PmTensor(0x100000, 0, 8, 8, 16, 16, dt, 0)), pointer(L.PmTensor(0x100000, 0, 8, 8, 16, 16, dt, 0)))
        out[tag + '/add_n[n=1]'] = lib.pm_add_n(one, 1, t(dt, 8, 8), None)
        out[tag + '/add_n[output no vector view]'] = lib.pm_add_n(one, 2, t(dt, 8, 8, pitch=18), None)
        out[tag + '/add[shapes differ]'] = lib.pm_add(t(dt, 8, 8), t(dt, 8, 4), t(dt, 8, 8), None)
        out[tag + '/resize_bwd_separable[ineligible]'] = lib.pm_resize_bilinear_bwd_separable(t(dt, 8, 6), t(dt, 4, 4), 0, ws, 1 << 20, None)
        one_image = [byref(L.PmTensor(0x100000, 1, hw, hw, 16, 16, dt, 0)) for hw in (8, 4)]      # n = 1: an empty tensor needs no workspace
        out[tag + '/resize_bwd_separable[no workspace]'] = lib.pm_resize_bilinear_bwd_separable(one_image[0], one_image[1], 0, None, 0, None)
        out[tag + '/global_avgpool_fwd[no vector view]'] = lib.pm_global_avgpool_fwd(t(dt, 8, 8, pitch=18), t(dt, 1, 1), None)
        out[tag + '/global_avgpool_bwd[no vector view]'] = lib.pm_global_avgpool_bwd(t(dt, 1, 1), t(dt, 8, 8, pitch=18), 0, None)
        out[tag + '/maxpool_fwd[shape]'] = lib.pm_maxpool3x3s2_fwd(t(dt, 8, 8), t(dt, 5, 4), arg, None)
    # what only the bf16 tier refuses: a view that is no 16-byte vector view, an argmax that is not 8-byte aligned, a misaligned row of pooled gradients
    out['bf16/maxpool_fwd[pitch]'] = lib.pm_maxpool3x3s2_fwd(t(b16, 8, 8, pitch=20), t(b16, 4, 4), arg, None)
    out['bf16/maxpool_fwd[argmax]'] = lib.pm_maxpool3x3s2_fwd(t(b16, 8, 8), t(b16, 4, 4), p(0x200004), None)
    out['bf16/maxpool_bwd[argmax]'] = lib.pm_maxpool3x3s2_bwd(t(b16, 4, 4), p(0x200004), t(b16, 8, 8), None)
    out['bf16/global_avgpool_bwd[dy]'] = lib.pm_global_avgpool_bwd(t(b16, 1, 1, addr=0x100002), t(b16, 8, 8), 0, None)
    out['bf16/resize_fwd[c]'] = lib.pm_resize_bilinear_fwd(t(b16, 4, 4, c=12, pitch=16), t(b16, 8, 8, c=12, pitch=16), None)
    out['bf16/resize_bwd[pitch]'] = lib.pm_resize_bilinear_bwd(t(b16, 8, 8, pitch=20), t(b16, 4, 4), 0, None)
    out['bf16/copy[pitch]'] = lib.pm_copy(t(b16, 8, 8, pitch=20), t(b16, 8, 8), None)
    return out


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def _view(buf, c, at=0):
    return buf[..., at:at + c]


def _dev(cpu, dtype, pad=0):
    """CPU NHWC fp32 values -> device tensor of `dtype` whose pitch is C + pad (pad lanes zero)."""
    import torch
    n, h, w, c = cpu.shape
    buf = torch.zeros((n, h, w, c + pad), dtype=dtype, device='cuda')
    v = _view(buf, c)
    v.copy_(cpu)
    return v


def _randn(shape, seed):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _rec(lib, out, name, code, tensors):
    out[name] = {k: digest(v) for k, v in tensors.items()} if code == 0 else 'refused:%d' % code


def _pool_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def run_pool(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    (n, h, w), c, pad, fill, off = a['shape'], a['c'], a.get('pad', 0), a.get('fill'), a.get('arg_offset', 0)
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    x = _randn((n, h, w, c), 31)
    if fill == 'relu':
        x = x.clamp(min=0)
    elif fill in ('nan', '-inf'):
        bad = float('nan') if fill == 'nan' else float('-inf')
        x[0, 2, 3, :] = bad                      # inside every window around it, every channel
        x[0, 5, 1::2, 1] = bad                   # and alternating pixels of one row, one channel
        x[0, 0, 0, 2] = bad                      # the corner
    ho, wo = _pool_hw(h, w)
    x, dy = _dev(x, dtype, pad), _dev(_randn((n, ho, wo, c), 32), dtype, pad)
    y, dx = _dev(torch.zeros(n, ho, wo, c), dtype, pad), _dev(torch.zeros(n, h, w, c), dtype, pad)
    argbuf = torch.zeros(n * ho * wo * c + 16, dtype=torch.uint8, device='cuda')
    arg = argbuf[off:off + n * ho * wo * c]
    out = {}
    _rec(lib, out, 'maxpool_fwd', lib.pm_maxpool3x3s2_fwd(T(x), T(y), arg.data_ptr(), st), dict(y=y, argmax=arg))
    if out['maxpool_fwd'] == 'refused:-1':       # the backward needs argmax bytes: those of the aligned forward, moved
        al = torch.zeros(n * ho * wo * c, dtype=torch.uint8, device='cuda')
        L.check(lib.pm_maxpool3x3s2_fwd(T(x), T(y), al.data_ptr(), st), 'pm_maxpool3x3s2_fwd')
        arg.copy_(al)
    _rec(lib, out, 'maxpool_bwd', lib.pm_maxpool3x3s2_bwd(T(dy), arg.data_ptr(), T(dx), st), dict(dx=dx))
    return out


def run_pool_bn(lib, L, a, dt):
    import torch
    (n, h, w), c = a['shape'], a['c']
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    g = torch.Generator().manual_seed(33)
    x = (torch.randn((n, h, w, c), generator=g) * 1.5 + 0.3).cuda()
    mean, beta = (torch.randn(c, generator=g) * 0.2).cuda(), (torch.randn(c, generator=g) * 0.2).cuda()
    invstd, gamma = (torch.rand(c, generator=g) + 0.5).cuda(), (torch.rand(c, generator=g) + 0.5).cuda()
    gamma[1::3] *= -1.0
    ho, wo = _pool_hw(h, w)
    y, arg = torch.zeros(n, ho, wo, c, device='cuda'), torch.zeros(n, ho, wo, c, dtype=torch.uint8, device='cuda')
    out = {}
    _rec(lib, out, 'maxpool_bn_relu_fwd', lib.pm_maxpool3x3s2_bn_relu_fwd(T(x), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), T(y), arg.data_ptr(), st),
         dict(y=y, argmax=arg))
    return out


def run_gap(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    (n, h, w) = a['shape']
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    out = {}
    for c in a['cs']:
        if a.get('fwd', True):
            x, y = _dev(_randn((n, h, w, c), 41) + 0.5, dtype), _dev(torch.zeros(n, 1, 1, c), dtype)
            _rec(lib, out, 'global_avgpool_fwd[c=%d]' % c, lib.pm_global_avgpool_fwd(T(x), T(y), st), dict(y=y))
        dy = _dev(_randn((n, 1, 1, c), 42), dtype)
        for acc in (0, 1):
            dx = _dev(_randn((n, h, w, c), 43), dtype)
            _rec(lib, out, 'global_avgpool_bwd[c=%d,acc=%d]' % (c, acc), lib.pm_global_avgpool_bwd(T(dy), T(dx), acc, st), dict(dx=dx))
    return out


def run_resize(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    (h, w), (H, W), c, pad, n = a['lo'], a['hi'], a.get('c', 8), a.get('pad', 0), 2
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    out = {}
    if a.get('fwd', True):
        x = _dev(_randn((n, h, w, c), 51), dtype, pad)
        if a.get('slice_of'):
            ybuf = torch.zeros((n, H, W, a['slice_of']), dtype=dtype, device='cuda')
            y = _view(ybuf, c, a['slice_of'] - c)
        else:
            y = _dev(_randn((n, H, W, c), 52), dtype, pad)
            ybuf = y._base
        _rec(lib, out, 'resize_fwd', lib.pm_resize_bilinear_fwd(T(x), T(y), st), dict(y=ybuf))      # the whole buffer: pad lanes / the other channels too
    dy = _dev(_randn((n, H, W, c), 53), dtype, pad)
    fresh = lambda: _dev(_randn((n, h, w, c), 54), dtype, pad)
    if a.get('gather', True):
        for acc in (0, 1):
            dx = fresh()
            _rec(lib, out, 'resize_bwd[acc=%d]' % acc, lib.pm_resize_bilinear_bwd(T(dy), T(dx), acc, st), dict(dx=dx._base))
    nb = lib.pm_resize_bilinear_bwd_workspace(T(dy), T(fresh()))
    out['workspace'] = nb
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device='cuda')
    for acc in (0, 1):
        dx = fresh()
        _rec(lib, out, 'resize_bwd_separable[acc=%d]' % acc, lib.pm_resize_bilinear_bwd_separable(T(dy), T(dx), acc, ws.data_ptr(), ws.numel(), st), dict(dx=dx._base))
    if nb == 0 and not a.get('expect_refused'):
        for acc in (0, 1):                       # an ineligible pair: only the case that is about the refusal keeps it
            out.pop('resize_bwd_separable[acc=%d]' % acc)
    return out


def _add_n(lib, L, xs, y):
    descs = [L.tdesc(x) for x in xs]
    arr = (POINTER(L.PmTensor) * len(xs))(*[pointer(d) for d in descs])
    return lib.pm_add_n(arr, len(xs), byref(L.tdesc(y)), L.stream())


def run_add(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    (n, h, w), c, pads = a['shape'], a['c'], a['pads']
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    xs = [_dev(_randn((n, h, w, c), 60 + i), dtype, pads[i % 3]) for i in range(8)]
    out = {}
    y = _dev(torch.zeros(n, h, w, c), dtype, pads[2])
    _rec(lib, out, 'add', lib.pm_add(T(xs[0]), T(xs[1]), T(y), st), dict(y=y))
    for k in a.get('ns', (2, 5, 8)):
        y = _dev(torch.zeros(n, h, w, c), dtype, pads[1])
        _rec(lib, out, 'add_n[n=%d]' % k, _add_n(lib, L, xs[:k], y), dict(y=y))
    return out


def run_copy(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    (n, h, w), c = a['shape'], a['c']
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    x = _dev(_randn((n, h, w, c), 70), dtype)
    buf = torch.zeros((n, h, w, a.get('slice_of', c)), dtype=dtype, device='cuda')
    out = {}
    _rec(lib, out, 'copy', lib.pm_copy(T(x), T(_view(buf, c, a.get('slice_at', 0))), st), dict(y=buf))
    return out


def run_ew_big(lib, L, a, dt):
    import torch
    dtype, _ = _types(L, dt)
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    x0, x1 = _dev(_randn(BIG, 80), dtype), _dev(_randn(BIG, 81), dtype)
    y = torch.zeros(BIG, dtype=dtype, device='cuda')
    out = {}
    _rec(lib, out, 'add_n[n=2]', _add_n(lib, L, [x0, x1], y), dict(y=y))
    _rec(lib, out, 'copy', lib.pm_copy(T(x0), T(y), st), dict(y=y))
    return out


def run_cast(lib, L, a, dt):
    import torch
    (n, h, w) = a['shape']
    st, T = L.stream(), lambda t: byref(L.tdesc(t))
    out = {}
    for c in a.get('cs', (24, 19)):
        x = _randn((n, h, w, c), 90) * 3
        pad = 8 if c % 8 == 0 and n * h * w < 1000 else 0      # the vector form between channel slices of wider buffers
        xf, yb = _dev(x, torch.float32, pad), _dev(torch.zeros(n, h, w, c), torch.bfloat16, pad)
        _rec(lib, out, 'cast[f32->bf16,c=%d]' % c, lib.pm_cast(T(xf), T(yb), st), dict(y=yb))
        xb, yf = _dev(x, torch.bfloat16, pad), _dev(torch.zeros(n, h, w, c), torch.float32, pad)
        _rec(lib, out, 'cast[bf16->f32,c=%d]' % c, lib.pm_cast(T(xb), T(yf), st), dict(y=yf))
    return out


RUNNERS = dict(pool=run_pool, pool_bn=run_pool_bn, gap=run_gap, resize=run_resize, add=run_add, copy=run_copy, ew_big=run_ew_big, cast=run_cast)


def run_case(lib, L, case, dt):
    """Every call of the case's family on its inputs -> {call: {output: sha256} or 'refused:<status>' (or the workspace answer)}."""
    import torch
    name, kind, args, _ = case
    if name == 'resize-ratio2-one-way':
        args = dict(args, expect_refused=True)
    out = RUNNERS[kind](lib, L, args, dt)
    torch.cuda.synchronize()
    return out


def check_reach(digests):
    """Every case is recorded for each of its element types, and a call is recorded as refused only where EXPECT_REFUSED names it, with that status."""
    assert sorted(digests) == sorted('%s/%s' % (c[0], dt) for c, dt in RUNS), sorted(digests)
    refused = {k: {call: int(v.split(':')[1]) for call, v in d.items() if isinstance(v, str) and v.startswith('refused')} for k, d in digests.items()}
    assert {k: v for k, v in refused.items() if v} == EXPECT_REFUSED, {k: v for k, v in refused.items() if v}
    for k, d in digests.items():
        assert d, k


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    fixture = {'digests': {}}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            fixture = json.load(f)
    fixture['workspaces'] = workspaces(lib, L)
    fixture['refusals'] = refusals(lib, L)
    if torch.cuda.is_available():
        fixture['digests'] = {'%s/%s' % (c[0], dt): run_case(lib, L, c, dt) for c, dt in RUNS}
        check_reach(fixture['digests'])
    else:
        print('no GPU: workspace answers and refusals recorded, digests kept as they were')
    with open(FIXTURE, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d case digests, %d workspace shapes, %d refusals -> %s' % (len(fixture['digests']), len(fixture['workspaces']), len(fixture['refusals']), FIXTURE))


if __name__ == '__main__':
    main()
