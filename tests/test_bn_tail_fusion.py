"""GPU: the ResNet BatchNorm tails without their widest temporaries -- the masked skip gradient (dv * ReLU mask) of every Bottleneck, the normalised downsample
output of a stage's first block, and the stem's full-resolution activation and gradient around its max pool. Every fused form is compared with torch.equal against
the same result composed from the primitives that stay in the library (bn_bwd_reduce_mask(want_gmask=True) + bn_bwd_apply(relu=0), bn_apply twice, conv_bwd_data with
a stored masked tensor as plain `add`, maxpool3x3s2 forward / backward on a materialised tensor): the arithmetic is unchanged, so no tolerance applies."""
import copy
import csv

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def padded(K, t):
    """The same values in a pitch-padded NHWC tensor (rows wider than the channel count)."""
    p = K.new(tuple(t.shape), t, pitch_pad=True)
    if p.stride(2) == t.shape[3]:      # the allocator pads only some widths: force a wider pitch
        base = torch.empty(t.shape[:3] + (t.shape[3] + 4,), dtype=t.dtype, device=t.device)
        p = base[..., :t.shape[3]]
    p.copy_(t)
    return p


def bn_params(c, seed):
    """(mean, invstd, gamma, beta) of a BatchNorm over c channels: any values do, the kernels under test take them as given."""
    return (rnd(c, seed=seed, scale=0.3), rnd(c, seed=seed + 1).abs() + 0.5, rnd(c, seed=seed + 2) * 0.5 + 1.0, rnd(c, seed=seed + 3, scale=0.2))


TAIL_SHAPES = [(2, 5, 7, 8), (1, 9, 11, 72)]      # pixels not a multiple of 16 (the reduce pass's row lanes), channels not a multiple of 64 (its channel block)


@pytest.fixture(scope='module')
def tails(K):
    """Per shape: a BN + residual + ReLU forward (output, mask bytes), an incoming gradient, and the stored-gm reference of the backward -- computed once."""
    out = {}
    for shape in TAIL_SHAPES:
        c = shape[3]
        x, r, dv, yd = rnd(*shape, seed=1), rnd(*shape, seed=2), rnd(*shape, seed=3), rnd(*shape, seed=4)
        mean, invstd, gamma, beta = bn_params(c, 10)
        md, idd, gd, _ = bn_params(c, 20)
        _, mask = K.bn_apply(x, mean, invstd, gamma, beta, residual=r, relu=True, want_mask=True)
        count = float(shape[0] * shape[1] * shape[2])
        sums, gm = K.bn_bwd_reduce_mask(dv, mask, x, mean, invstd, want_gmask=True)
        dy, _ = K.bn_bwd_apply(gm, None, x, mean, invstd, gamma, sums, count, 0, False)
        sums_d, _ = K.bn_bwd_reduce(gm, None, yd, md, idd, 0, gd, None)
        dyd, _ = K.bn_bwd_apply(gm, None, yd, md, idd, gd, sums_d, count, 0, False)
        out[shape] = dict(x=x, dv=dv, yd=yd, mask=mask, bn=(mean, invstd, gamma), bnd=(md, idd, gd), count=count, gm=gm, sums=sums, dy=dy, sums_d=sums_d, dyd=dyd)
    return out


@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('pitch', ['dense', 'padded'])
def test_bn_bwd_apply_in_mask_mode_equals_the_stored_gm_composition(K, tails, shape, pitch):
    t = tails[shape]
    x, dv = (padded(K, t['x']), padded(K, t['dv'])) if pitch == 'padded' else (t['x'], t['dv'])
    mean, invstd, gamma = t['bn']
    sums, none = K.bn_bwd_reduce_mask(dv, t['mask'], x, mean, invstd, want_gmask=False)
    assert none is None and torch.equal(sums, t['sums'])
    dy = K.bn_bwd_apply_mask(dv, t['mask'], x, mean, invstd, gamma, sums, t['count'])
    assert torch.equal(dy, t['dy'])
    # the element count read from the device (SyncBatchNorm's form): sums[2c] holds it
    sums_c, _ = K.bn_bwd_reduce_mask(dv, t['mask'], x, mean, invstd, want_gmask=False, with_count=True)
    ref_c, _ = K.bn_bwd_apply(t['gm'], None, t['x'], mean, invstd, gamma, sums_c, -1.0, 0, False)
    assert torch.equal(K.bn_bwd_apply_mask(dv, t['mask'], x, mean, invstd, gamma, sums_c, -1.0), ref_c)


@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_downsample_bn_backward_reads_dv_and_the_mask_of_the_activation_behind_it(K, tails, shape):
    """The mask mode applies to ANY x: the downsample BatchNorm (x = yd, its own statistics) behind the same ReLU."""
    t = tails[shape]
    md, idd, gd = t['bnd']
    yd = padded(K, t['yd'])
    sums, _ = K.bn_bwd_reduce_mask(t['dv'], t['mask'], yd, md, idd, want_gmask=False)
    assert torch.equal(sums, t['sums_d'])
    assert torch.equal(K.bn_bwd_apply_mask(t['dv'], t['mask'], yd, md, idd, gd, sums, t['count']), t['dyd'])


@pytest.mark.parametrize('shape', [(2, 5, 7, 8), (1, 3, 3, 68)], ids=lambda s: 'x'.join(map(str, s)))
def test_bn_apply_with_a_second_affine_residual_equals_the_two_launch_form(K, shape):
    c = shape[3]
    x, yd = rnd(*shape, seed=5), padded(K, rnd(*shape, seed=6))
    mean, invstd, gamma, beta = bn_params(c, 30)
    md, idd, gd, bd = bn_params(c, 40)
    res = K.bn_apply(yd, md, idd, gd, bd, residual=None, relu=False)
    ref, ref_mask = K.bn_apply(x, mean, invstd, gamma, beta, residual=res, relu=True, want_mask=True)
    out, mask = K.bn_apply_res_affine(x, mean, invstd, gamma, beta, yd, md, idd, gd, bd, relu=True, want_mask=True)
    assert torch.equal(out, ref) and torch.equal(mask, ref_mask)
    assert 0 < int((ref > 0).sum()) < ref.numel()      # the ReLU clamps some and passes some: both mask values occur
    assert torch.equal(K.bn_apply_res_affine(x, mean, invstd, gamma, beta, yd, md, idd, gd, bd, relu=False),
                       K.bn_apply(x, mean, invstd, gamma, beta, residual=res, relu=False))


# ---- masked `add` of the data gradient ------------------------------------------------------------------------------------------------------------------------
def records(K, path):
    """The convolution launch records filed since profile_enable(True) (mode, bm, bn, km, prec, batch, ksplit ...): the route each call resolved to."""
    torch.cuda.synchronize()
    K.profile_dump(path)
    K.profile_read(clear=True)
    with open(path) as f:
        return [{k: int(v) for k, v in row.items() if k not in ('ms', 'gflop')} for row in csv.DictReader(f)]


def dgrad_operands(K, n, h, w, cout, cin, k=1):
    dy = rnd(n, h, w, cout, seed=1)
    wt = rnd(cout, k, k, cin, seed=2, scale=(2.0 / (cout * k * k)) ** 0.5)
    add = rnd(n, h, w, cin, seed=3)
    mask = torch.randint(0, 16, (n * h * w, cin // 4), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    bits = torch.stack([(mask >> e) & 1 for e in range(4)], dim=2).reshape(n, h, w, cin).bool()
    return dy, wt, add, mask, torch.where(bits, add, torch.zeros_like(add))


def routed(K, tmp_path, fn):
    K.profile_read(clear=True)
    K.profile_enable(True)
    try:
        out = fn()
        return out, records(K, str(tmp_path / 'rec.csv'))
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)


# (n, h, w, cout = channels of dy, cin = channels of dx) -> the kernel family the library's own launch record must show
MASKED_ADD_CASES = [
    ((1, 257, 257, 64, 256), 'stream'),      # 66 049 rows: just over the streaming kernel's floor, a last tile of one row
    ((2, 9, 9, 256, 1024), 'tile5'),         # split-operand tile kernel (K >= 129), one K split; 162 rows = two 64-row tiles and a partial third
    ((2, 9, 9, 64, 256), 'tile0'),           # fp32-MFMA tile kernel (short K), the same epilogue in its other translation unit
    ((2, 9, 9, 512, 2048), 'splitk'),        # split-K: the mask is applied by splitk_reduce, one lane per output group
    ((2, 9, 9, 1024, 256), 'splitk'),        # ... four lanes per group
    ((1, 3, 3, 8192, 256), 'splitk'),        # ... sixteen lanes per group
]


@pytest.mark.parametrize('case,family', MASKED_ADD_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_masked_add_equals_the_explicitly_masked_tensor(K, tmp_path, case, family):
    n, h, w, cout, cin = case
    dy, wt, add, mask, add_masked = dgrad_operands(K, n, h, w, cout, cin)
    ref = K.conv_bwd_data(dy, wt, (n, h, w, cin), 1, 0, 1, add=add_masked)
    dx, rec = routed(K, tmp_path, lambda: K.conv_bwd_data(dy, wt, (n, h, w, cin), 1, 0, 1, add=add, add_mask=mask))
    assert len(rec) == 1 and rec[0]['mode'] == 1 and rec[0]['batch'] == 1, rec
    r = rec[0]
    got = 'stream' if (r['bm'], r['bn'], r['km']) == (32, 64, 4) else ('splitk' if r['ksplit'] > 1 else 'tile%d' % r['prec'])
    assert got == family, rec
    assert torch.equal(dx, ref)
    assert not torch.equal(dx, K.conv_bwd_data(dy, wt, (n, h, w, cin), 1, 0, 1, add=add))      # the mask mattered


def test_masked_add_is_refused_where_the_route_cannot_apply_it(K, tmp_path):
    """Documented behaviour (include/pinmem_hip.h): only the fp32 implicit-GEMM route serves a masked add; a stride-2 data gradient (the parity-class kernels) and a
    Winograd-routed 3x3 return PM_EUNSUPPORTED with the reason in pm_last_error -- never an unmasked sum."""
    from pinthememory_amd.hip import lib as L
    # 1x1 stride 2: dy 2 x 5 x 5 x 64 -> dx 2 x 9 x 9 x 32
    dy, wt, add, mask, _ = dgrad_operands(K, 2, 9, 9, 64, 32)
    with pytest.raises(L.PinmemError, match='masked'):
        K.conv_bwd_data(dy[:, :5, :5].contiguous(), wt, (2, 9, 9, 32), 2, 0, 1, add=add, add_mask=mask)
    # 3x3 stride 1 at 64 channels: refused if (and only if) the unmasked call goes to Winograd (batched point products in the record), served otherwise
    n, h, w, c = 2, 12, 12, 64
    dy, wt, add, mask, add_masked = dgrad_operands(K, n, h, w, c, c, k=3)
    ref, rec = routed(K, tmp_path, lambda: K.conv_bwd_data(dy, wt, (n, h, w, c), 1, 1, 1, add=add_masked))
    if any(r['batch'] > 1 for r in rec):
        with pytest.raises(L.PinmemError, match='Winograd'):
            K.conv_bwd_data(dy, wt, (n, h, w, c), 1, 1, 1, add=add, add_mask=mask)
    else:
        assert torch.equal(K.conv_bwd_data(dy, wt, (n, h, w, c), 1, 1, 1, add=add, add_mask=mask), ref)


# ---- the whole block -------------------------------------------------------------------------------------------------------------------------------------------
def reference_block(K, ops, blk, x, g):
    """One Bottleneck, forward and backward, assembled from the library's primitives with every temporary stored: the normalised downsample output, the masked
    gradient gm, and gm as the plain `add` of conv1's data gradient. -> (out, [every gradient _Bottleneck.backward returns, in its order])."""
    ds = blk.downsample
    mods = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)] + ([(ds[0], ds[1])] if ds is not None else [])
    ge = [ops._geom(c) for c, _ in mods]
    ks = [K.krsc(c.weight.detach()) for c, _ in mods]
    bn = [ops.BNState(b) for _, b in mods]
    ga = [b.weight.detach() for _, b in mods]
    be = [b.bias.detach() for _, b in mods]
    xv = ops.nhwc(x.detach())
    ps, kv = [], []
    y1 = K.conv_fwd(xv, ks[0], *ge[0], bn_partials=ps)
    m1, i1 = ops._bn_train_stats(y1, bn[0], ps[0])
    o1 = K.bn_apply(y1, m1, i1, ga[0], be[0], relu=True)
    y2 = K.conv_fwd(o1, ks[1], *ge[1], keep_v=kv, bn_partials=ps)
    m2, i2 = ops._bn_train_stats(y2, bn[1], ps[1])
    o2 = K.bn_apply(y2, m2, i2, ga[1], be[1], relu=True)
    y3 = K.conv_fwd(o2, ks[2], *ge[2], bn_partials=ps)
    if ds is not None:
        yd = K.conv_fwd(xv, ks[3], *ge[3], bn_partials=ps)
        md, idd = ops._bn_train_stats(yd, bn[3], ps[3])
        res = K.bn_apply(yd, md, idd, ga[3], be[3], relu=False)
    else:
        res = xv
    m3, i3 = ops._bn_train_stats(y3, bn[2], ps[2])
    out, mask = K.bn_apply(y3, m3, i3, ga[2], be[2], residual=res, relu=True, want_mask=True)

    def count(t):
        return float(t.shape[0] * t.shape[1] * t.shape[2])

    def bn_relu_bwd(d, o, y, m, i, gamma, beta):
        s, _ = K.bn_bwd_reduce(d, o, y, m, i, 2, gamma, beta)
        dy, _ = K.bn_bwd_apply(d, o, y, m, i, gamma, s, count(y), 2, False, beta)
        c = y.shape[3]
        return dy, s[c:2 * c], s[:c]

    dv = ops._grad_view(g)
    c3 = y3.shape[3]
    s3, gm = K.bn_bwd_reduce_mask(dv, mask, y3, m3, i3, want_gmask=True)
    dy3, _ = K.bn_bwd_apply(gm, None, y3, m3, i3, ga[2], s3, count(y3), 0, False)
    dw3, _ = K.conv_bwd_weight(o2, dy3, tuple(ks[2].shape), *ge[2])
    do2 = K.conv_bwd_data(dy3, ks[2], tuple(o2.shape), *ge[2])
    dy2, dg2, db2 = bn_relu_bwd(do2, o2, y2, m2, i2, ga[1], be[1])
    dw2, _ = K.conv_bwd_weight(o1, dy2, tuple(ks[1].shape), *ge[1], wino_v=kv[0])
    do1 = K.conv_bwd_data(dy2, ks[1], tuple(o1.shape), *ge[1])
    dy1, dg1, db1 = bn_relu_bwd(do1, o1, y1, m1, i1, ga[0], be[0])
    dw1, _ = K.conv_bwd_weight(xv, dy1, tuple(ks[0].shape), *ge[0])
    dwd = dgd = dbd = None
    skip = gm
    if ds is not None:
        sd, _ = K.bn_bwd_reduce(gm, None, yd, md, idd, 0, ga[3], None)
        dyd, _ = K.bn_bwd_apply(gm, None, yd, md, idd, ga[3], sd, count(yd), 0, False)
        dwd, _ = K.conv_bwd_weight(xv, dyd, tuple(ks[3].shape), *ge[3])
        dgd, dbd = sd[c3:2 * c3], sd[:c3]
        skip = K.conv_bwd_data(dyd, ks[3], tuple(xv.shape), *ge[3])
    dx = K.conv_bwd_data(dy1, ks[0], tuple(xv.shape), *ge[0], add=skip)
    p = lambda d: d.permute(0, 3, 1, 2)
    return ops.nchw(out), [ops.nchw(dx), p(dw1), dg1, db1, p(dw2), dg2, db2, p(dw3), s3[c3:2 * c3], s3[:c3], p(dwd) if dwd is not None else None, dgd, dbd]


@pytest.mark.parametrize('downsample', [False, True], ids=['identity', 'downsample'])
def test_bottleneck_node_equals_the_block_assembled_from_primitives(K, downsample):
    from pinthememory_amd.hip import ops
    from pinthememory_amd.network import Resnet, mynn
    torch.manual_seed(7)
    inplanes = 16 if downsample else 64
    ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, 64, kernel_size=1, bias=False), mynn.Norm2d(64)) if downsample else None
    blk = Resnet.Bottleneck(inplanes, 16, 1, ds).cuda().train()
    for b in (blk.bn1, blk.bn2, blk.bn3) + ((ds[1],) if downsample else ()):      # gammas / betas away from (1, 0)
        b.weight.data.uniform_(0.5, 1.5), b.bias.data.uniform_(-0.3, 0.3)
    ref_blk = copy.deepcopy(blk)      # its own running moments
    x = ops.nchw(rnd(2, 8, 8, inplanes, seed=8)).requires_grad_(True)
    g = ops.nchw(rnd(2, 8, 8, 64, seed=9))
    ops.begin_forward()
    out = ops.bottleneck(x, blk)
    out.backward(g)
    torch.cuda.synchronize()
    params = [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias, blk.conv3.weight, blk.bn3.weight, blk.bn3.bias]
    params += [ds[0].weight, ds[1].weight, ds[1].bias] if downsample else [None, None, None]
    got = [x.grad] + [p.grad if p is not None else None for p in params]
    ref_out, ref = reference_block(K, ops, ref_blk, x, g)
    assert torch.equal(out.detach(), ref_out)
    assert len(got) == len(ref) == 13
    for i, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert torch.equal(a, b), i
    for b, rb in zip((blk.bn1, blk.bn2, blk.bn3), (ref_blk.bn1, ref_blk.bn2, ref_blk.bn3)):
        assert torch.equal(b.running_mean, rb.running_mean) and torch.equal(b.running_var, rb.running_var)


# ---- the stem tail ---------------------------------------------------------------------------------------------------------------------------------------------
def stem_input(shape, seed):
    """A raw convolution output with whole pooling windows of negative pre-activations (every tap clamps to zero: the argmax is decided by tie-breaking alone)
    next to ordinary ones, and exact zeros after the affine."""
    y = rnd(*shape, seed=seed)
    n, h, w, c = shape
    y[:, : h // 2, : w // 2, :] = -y[:, : h // 2, : w // 2, :].abs() - 3.0      # a negative quadrant: with the statistics below, bn(y) < 0 there for every channel
    y[:, h // 2:, :, : c // 2] *= 0.25
    return y


@pytest.mark.parametrize('shape', [(2, 13, 11, 8), (1, 8, 8, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_fused_stem_tail_equals_the_separate_kernels(K, shape):
    n, h, w, c = shape
    y = padded(K, stem_input(shape, 50))
    mean, invstd = rnd(c, seed=51, scale=0.2), rnd(c, seed=52).abs() * 0.2 + 0.8
    gamma, beta = rnd(c, seed=53).abs() * 0.5 + 0.5, rnd(c, seed=54, scale=0.2)
    o = K.bn_apply(y, mean, invstd, gamma, beta, relu=True)
    assert bool((o[:, : h // 2 - 1, : w // 2 - 1, :] == 0).all())      # whole windows of clamped zeros exist
    ref_out, ref_arg = K.maxpool_fwd(o)
    out, arg = K.maxpool_bn_relu_fwd(y, mean, invstd, gamma, beta)
    assert torch.equal(out, ref_out) and torch.equal(arg, ref_arg)
    assert len(torch.unique(ref_arg)) > 4      # several taps win somewhere
    dyp = padded(K, rnd(*ref_out.shape, seed=55))
    g = K.maxpool_bwd(dyp, ref_arg, shape)
    count = float(n * h * w)
    sums, _ = K.bn_bwd_reduce(g, None, y, mean, invstd, 2, gamma, beta)
    ref_dy, _ = K.bn_bwd_apply(g, None, y, mean, invstd, gamma, sums, count, 2, False, beta)
    dy, local = K.bn_relu_bwd_pool(dyp, arg, y, mean, invstd, gamma, beta)
    assert torch.equal(local, sums)      # dbeta | dgamma
    assert torch.equal(dy, ref_dy)
    # the device-side count (SyncBatchNorm's form)
    sums_c, _ = K.bn_bwd_reduce(g, None, y, mean, invstd, 2, gamma, beta, with_count=True)
    ref_c, _ = K.bn_bwd_apply(g, None, y, mean, invstd, gamma, sums_c, -1.0, 2, False, beta)
    dy_c, local_c = K.bn_relu_bwd_pool(dyp, arg, y, mean, invstd, gamma, beta, with_count=True)
    assert torch.equal(local_c, sums_c) and torch.equal(dy_c, ref_c)


def test_stem_node_equals_conv_bn_relu_then_maxpool(K):
    """network.Resnet.stem in train mode (the fused node) against the two nodes it replaces, on one set of weights: output, running moments and every gradient."""
    from pinthememory_amd.hip import ops
    from pinthememory_amd.network import mynn
    torch.manual_seed(11)
    conv = torch.nn.Conv2d(4, 64, kernel_size=7, stride=2, padding=3, bias=False).cuda()
    bn = mynn.Norm2d(64).cuda().train()
    bn.weight.data.uniform_(0.5, 1.5), bn.bias.data.uniform_(-0.3, 0.3)
    conv2, bn2 = copy.deepcopy(conv), copy.deepcopy(bn)
    x = ops.nchw(rnd(2, 29, 27, 4, seed=12))
    g = None
    res = []
    for cv, b, fused in ((conv, bn, True), (conv2, bn2, False)):
        ops.begin_forward()
        if fused:
            out = ops.stem_tail(x, cv.weight, cv, b)
            assert out.grad_fn.name().startswith('_Stem')
        else:
            out = ops.maxpool3x3s2(ops._ConvBnAct.apply(x, cv.weight, None, b.weight, b.bias, None, ops._geom(cv), ops.BNState(b), True, None))
        g = ops.nchw(rnd(*ops.nhwc(out).shape, seed=13)) if g is None else g
        out.backward(g)
        torch.cuda.synchronize()
        res.append((out.detach(), cv.weight.grad, b.weight.grad, b.bias.grad, b.running_mean, b.running_var))
    for a, r in zip(*res):
        assert torch.equal(a, r)
