"""GPU parity of each HIP kernel (called through the C ABI via ctypes) against stock torch fp32 ops on the CPU.
Tolerances: fp32 accumulation-order differences only -> 2e-5 relative to the tensor's scale unless noted."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


CONV_CASES = [
    # n, cin, h, w, cout, k, stride, pad, dil, bias
    (2, 64, 24, 20, 64, 1, 1, 0, 1, False),
    (2, 64, 24, 20, 256, 1, 1, 0, 1, False),
    (1, 32, 17, 19, 48, 3, 1, 1, 1, False),
    (2, 128, 24, 24, 128, 3, 2, 1, 1, False),
    (2, 256, 24, 24, 512, 1, 2, 0, 1, False),
    (1, 64, 20, 20, 64, 3, 1, 2, 2, False),
    (1, 128, 13, 13, 32, 3, 1, 6, 6, False),
    (1, 64, 26, 26, 40, 3, 1, 12, 12, True),
    (2, 4, 40, 36, 64, 7, 2, 3, 1, False),
    (2, 256, 16, 16, 19, 1, 1, 0, 1, True),
    (1, 304, 16, 16, 256, 3, 1, 1, 1, False),
    (3, 2048, 4, 4, 256, 1, 1, 0, 1, False),
    (2, 512, 1, 1, 256, 1, 1, 0, 1, False),
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_fwd_bwd(K, case):
    n, cin, h, w, cout, k, s, p, d, has_bias = case
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    b = rnd(cout, seed=3) if has_bias else None
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if has_bias else None
    y_ref = F.conv2d(xr, wr, br, stride=s, padding=p, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    y_ref.backward(dy)

    xg, wg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda()
    y = K.conv_fwd(xg, wg, s, p, d, bias=b.cuda() if has_bias else None)
    assert rel(nchw(y), y_ref.detach()) < 2e-5
    dyg = K.new(tuple(y.shape), y, pitch_pad=True)
    dyg.copy_(nhwc(dy))
    dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s, p, d)
    assert rel(nchw(dx), xr.grad) < 2e-5
    dw, db = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s, p, d, want_bias=has_bias)
    assert rel(dw.permute(0, 3, 1, 2), wr.grad) < 5e-5
    if has_bias:
        assert rel(db, br.grad) < 2e-5


SPLIT_CASES = [
    # n, cin, h, w, cout, k, stride, pad, dil   -- the split path (conv_split.hip) at small sizes, with and without the Winograd route. With at most 1 152 output rows and
    # output widths of at most 24 the direct route takes only the 64-row tiles in the forward pass and the data gradient and only the K_SMALL weight gradient on the
    # 128 x 128 tile; tests/test_split_kernels.py reaches every tile and K-state instantiation at the same bar and proves it by the launch record
    (2, 256, 24, 24, 512, 1, 1, 0, 1),      # pointwise, K_FAST forward / data gradient; weight gradient over 1 152 pixels
    (2, 512, 24, 24, 128, 1, 1, 0, 1),      # 128-column output (128 x 128 or 64 x 128 tile)
    (1, 160, 20, 20, 192, 3, 1, 1, 1),      # direct 3x3 (channels below the Winograd route's 128 x 128 rule? no: taken -- see wino below), K_FAST
    (2, 144, 17, 19, 136, 3, 1, 2, 2),      # channel counts that are no multiple of 32: K_MID gathers, ragged tiles
    (2, 256, 24, 24, 256, 3, 2, 1, 1),      # stride 2: the parity-class data gradient (K_MID), a strided weight gradient
    (2, 20, 12, 12, 192, 3, 1, 1, 1),       # Cin < 32: K_SMALL forward / weight gradient
    (1, 2048, 12, 12, 256, 3, 1, 6, 6),     # ASPP-like deep reduction (Winograd F(4x4) point GEMMs when the route is on)
]


@pytest.mark.parametrize('case', SPLIT_CASES)
def test_split_path_accuracy_vs_fp64(K, case, capsys):
    """Round 6: the fp32 tier on the bf16 matrix pipe -- fp32 operands split exactly into three bf16 pieces, six cross products, fp32 accumulation --
    must be an fp32 kernel, not a 16-bit-mantissa one: forward, input gradient and weight gradient against an fp64 convolution, next to the fp32-MFMA kernel
    (pm_set_split(0)) on the same operands. A dropped or doubled piece would show as ~2^-16 = 1.5e-5 of the output scale (under the 2e-5 bar of the older kernel tests);
    here the error must stay within 2 x the fp32 kernel's + 2e-7, both printed. With and without the Winograd route."""
    n, cin, h, w, cout, k, s_, p, d = case
    x = torch.relu(rnd(n, cin, h, w, seed=1)) + 0.01 * rnd(n, cin, h, w, seed=7)      # post-ReLU-like: mostly one sign, large sums
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=s_, padding=p, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    y_ref.backward(dy.double())
    xg, wg, dyg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy)
    errs = {}
    try:
        for wino in (4, 0):
            K.set_winograd(wino)
            for split in (True, False):
                K.set_split(split)
                y = K.conv_fwd(xg, wg, s_, p, d)
                dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s_, p, d)
                dw, _ = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s_, p, d)
                errs[(wino, split)] = (rel(nchw(y), y_ref.detach()), rel(nchw(dx), xr.grad), rel(dw.permute(0, 3, 1, 2), wr.grad))
    finally:
        K.set_split(True)
        K.set_winograd(4)
    with capsys.disabled():
        print('\n[split vs fp64 %s] ' % (case,) + '; '.join('wino %d %s: y %.1e dx %.1e dw %.1e' % ((wn, 'split' if sp else 'fp32 ') + e) for (wn, sp), e in errs.items()))
    for wino in (4, 0):
        for es, e0 in zip(errs[(wino, True)], errs[(wino, False)]):
            assert es <= 2.0 * e0 + 2e-7, (wino, errs)


PWSTREAM_CASES = [
    # n, cin, h, w, cout: pointwise, stride 1 -- the forward takes the streaming kernel when cin is 64 / 128, the data gradient when cout is
    (2, 64, 192, 192, 256),       # layer1 conv3 / downsample (Resnet.py:145-150): K = 64, four 64-column slabs, whole 32-row tiles
    (1, 64, 257, 257, 64),        # one slab, a last tile of ONE row (66 049 rows): the predicated store path
    (2, 128, 192, 192, 512),      # layer2-like: K = 128, eight slabs
    (2, 256, 192, 192, 64),       # data gradient: K = cout = 64 (weights read with the transposed strides), N = cin = 256
    (2, 512, 160, 208, 128),      # data gradient: K = 128, N = 512, 66 560 rows
]


@pytest.mark.parametrize('case', PWSTREAM_CASES)
def test_pwstream_short_pointwise_reductions(K, case, capsys):
    """Round 6: the wave-streamed pointwise GEMM of csrc/pwstream.hip (K = 64 / 128, >= 65 536 rows) against fp64, next to the fp32-MFMA tile kernel (pm_set_split(0))
    on the same operands -- same bar as the split tile kernel (<= 2 x the fp32 kernel's error + 2e-7) -- with the launch record proving which kernel ran. Then the
    epilogue forms it carries: eval-mode fold + residual + ReLU into a channel slice of a wider buffer from a channel slice of a wider input, and the data gradient's fused add."""
    n, cin, h, w, cout = case
    x = torch.relu(rnd(n, cin, h, w, seed=1)) + 0.01 * rnd(n, cin, h, w, seed=7)
    wt = rnd(cout, cin, 1, 1, seed=2, scale=(2.0 / cin) ** 0.5)
    dy = rnd(n, cout, h, w, seed=4)
    xg, wg, dyg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy)
    w64 = wg.view(cout, cin).double()
    y_ref = (xg.view(-1, cin).double() @ w64.t()).view(n, h, w, cout)
    dx_ref = (dyg.view(-1, cout).double() @ w64).view(n, h, w, cin)
    fwd_streams, bwd_streams = cin in (64, 128), cout in (64, 128)
    errs = {}
    try:
        for split in (True, False):
            K.set_split(split)
            K.profile_enable(True)
            K.profile_read(clear=True)
            y = K.conv_fwd(xg, wg, 1, 0, 1)
            nf = K.profile_read(mode=0, bm=32, bn=64, km=4)[2]
            dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), 1, 0, 1)
            nb = K.profile_read(mode=1, bm=32, bn=64, km=4, clear=True)[2]
            K.profile_enable(False)
            assert nf == (1 if (split and fwd_streams) else 0) and nb == (1 if (split and bwd_streams) else 0), (split, nf, nb)
            errs[split] = (rel(y, y_ref), rel(dx, dx_ref))
    finally:
        K.profile_enable(False)
        K.set_split(True)
    with capsys.disabled():
        print('\n[pwstream vs fp64 %s] stream: y %.1e dx %.1e; fp32 tile kernel: y %.1e dx %.1e' % ((case,) + errs[True] + errs[False]))
    for es, e0 in zip(errs[True], errs[False]):
        assert es <= 2.0 * e0 + 2e-7, errs
    if fwd_streams:       # epilogue + slices: pitch-padded input rows, output into channels [64, 64 + cout) of a wider buffer
        sc, sh, res = (rnd(cout, seed=3).abs() + 0.5).cuda(), rnd(cout, seed=5).cuda(), nhwc(rnd(n, cout, h, w, seed=6))
        wide = torch.zeros(n, h, w, cin + 32, device='cuda')
        wide[..., :cin] = xg
        xin = wide[..., :cin]                 # rows of K floats, K + 32 apart
        buf = torch.zeros(n, h, w, cout + 96, device='cuda')
        K.profile_enable(True)
        K.profile_read(clear=True)
        out = K.conv_fwd(xin, wg, 1, 0, 1, scale=sc, shift=sh, residual=res, relu=True, out=buf[..., 64:64 + cout])
        assert K.profile_read(mode=0, bm=32, bn=64, km=4, clear=True)[2] == 1
        K.profile_enable(False)
        ref = torch.relu(y_ref * sc.double() + sh.double() + res.double())
        assert rel(out, ref) < 2e-6
        assert buf[..., :64].abs().max().item() == 0 and buf[..., 64 + cout:].abs().max().item() == 0
    if bwd_streams:
        add = nhwc(rnd(n, cin, h, w, seed=8))
        dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), 1, 0, 1, add=add)
        assert rel(dx, dx_ref + add.double()) < 2e-6


def test_pwstream_leaves_the_bf16_operand_forms_alone(K):
    """The stream computes on fp32 operands. With bf16 OPERANDS requested on fp32 tensors (BASELINE configs[2] before round 4's bf16 activations: conv precision 'bf16') the
    launcher hands the kernel a float-typed view of bf16 pairs -- 256 bf16 channels look like a 128-float reduction -- and must keep such a launch away from the stream
    (a round-6 review finding: the first hook only excluded the staged form). Shape: 256 -> 128 on 2 x 192 x 192 pixels; oracle: fp32 convolution of bf16-rounded operands."""
    n, cin, h, w, cout = 2, 256, 192, 192, 128
    r16 = lambda t: t.bfloat16().float()
    x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 1, 1, seed=2, scale=(2.0 / cin) ** 0.5)
    xg, wg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda()
    y_ref = (r16(xg).view(-1, cin).double() @ r16(wg).view(cout, cin).double().t()).view(n, h, w, cout)
    K.set_conv_precision('bf16')
    try:
        K.profile_enable(True)
        K.profile_read(clear=True)
        y = K.conv_fwd(xg, wg, 1, 0, 1, out_dtype=torch.float32)      # fp32 in, fp32 out, bf16 operands: the launch that looked like an fp32 128-float reduction
        taken = K.profile_read(mode=0, bm=32, bn=64, km=4, clear=True)[2]
    finally:
        K.profile_enable(False)
        K.set_conv_precision('f32')
    assert taken == 0 and y.dtype == torch.float32
    assert rel(y, y_ref) < 1e-4


WINO_CASES = [
    # n, cin, h, w, cout, dil   (3x3, stride 1, pad == dil, both channel counts >= 128 -> Winograd F(2x2,3x3) route)
    (1, 304, 16, 16, 256, 1),
    (2, 128, 24, 24, 128, 2),
    (1, 256, 13, 15, 128, 1),      # odd extents: partial edge tiles
    (1, 128, 36, 36, 160, 6),
    (1, 2048, 24, 24, 256, 12),
    (2, 132, 8, 8, 140, 1),        # channel counts that are not multiples of 32 / 128
    (1, 128, 48, 48, 128, 6),      # F(4x4) on the dilation sub-lattices (8x8 each)
    (1, 256, 48, 44, 128, 12),     # 4x4 / 4x3.67 sub-lattices: one F(4x4) tile each
    # production shapes: the layers as they run at 768^2 / 1024^2, every tap in range
    (1, 2048, 48, 48, 256, 18),    # ASPP d18 @48x48 (deepv3plus.py:75-81): F(4x4) on sub-lattices of 3 / 2 rows padded to one 4-row tile
    (1, 2048, 64, 64, 256, 24),    # DeepLabV2 ASPP d24 (deepv2.py:44-51): taps at +-24 inside the map
    (1, 304, 96, 96, 256, 1),      # final1.0 (deepv3plus.py:408-414), 24 x 24 F(4x4) tiles per image
    (1, 512, 48, 48, 512, 2),      # layer4 conv2 at output stride 16 (deepv3plus.py:374-379)
]


def wino_route(h, w, d, mode):
    """The planner's choice (conv_igemm.hip wino_plan): the tile size m in {mode, ..., 2} with the fewest multiplies per output,
    if below 0.6 of the direct algorithm's; 0 = direct."""
    m, best = 0, 0.6
    for cand in range(mode, 1, -2):
        ty, tx = -(-(-(-h // d)) // cand), -(-(-(-w // d)) // cand)
        ratio = (cand * ty * d) * (cand * tx * d) / (h * w) * (cand + 2) ** 2 / (9.0 * cand * cand)
        if ratio <= best:
            m, best = cand, ratio
    return m


@pytest.mark.parametrize('case', WINO_CASES)
def test_conv_winograd(K, case):
    """Winograd routes (4 = prefer F(4x4,3x3), 2 = F(2x2,3x3)) vs an fp64 convolution, next to the direct implicit GEMM (0) on the
    same inputs: all within fp32 rounding of the truth, and the route is really taken (results differ from the direct ones in the
    last bits)."""
    n, cin, h, w, cout, d = case
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(2.0 / (cin * 9)) ** 0.5)
    b = rnd(cout, seed=3)
    xr, wr, br = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, br, padding=d, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    y_ref.backward(dy.double())
    add = rnd(n, cin, h, w, seed=5)
    xg, wg, dyg, addg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy), nhwc(add)
    buf = torch.zeros(n, h, w, cout + 64, device='cuda')
    res = {}
    for wino in (4, 2, 0):
        K.set_winograd(wino)
        try:
            y = K.conv_fwd(xg, wg, 1, d, d, bias=b.cuda(), out=buf[..., 32:32 + cout])
            dw, db = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), 1, d, d, want_bias=True)
            kv = []      # transformed input kept by the forward pass and handed to the weight gradient: the same bits
            y_k = K.conv_fwd(xg, wg, 1, d, d, bias=b.cuda(), keep_v=kv)
            dw_k, _ = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), 1, d, d, want_bias=True, wino_v=kv[0])
            assert torch.equal(y_k, y) and torch.equal(dw_k, dw)
            assert (kv[0] is not None) == (wino_route(h, w, d, wino) != 0 and cin * cout >= 256 * 256), (wino, kv[0] is None)
            res[wino] = (nchw(y).clone(), nchw(K.conv_bwd_data(dyg, wg, tuple(xg.shape), 1, d, d, add=addg)), dw.permute(0, 3, 1, 2).cpu(), db.cpu())
        finally:
            K.set_winograd(True)
        assert buf[..., :32].abs().max().item() == 0 and buf[..., 32 + cout:].abs().max().item() == 0
    for wino in (4, 2, 0):
        assert rel(res[wino][0], y_ref.detach()) < 2e-5, wino
        assert rel(res[wino][1], xr.grad + add.double()) < 2e-5, wino
        assert rel(res[wino][2], wr.grad) < 5e-5, wino
        assert rel(res[wino][3], br.grad) < 2e-5, wino
    # the routes are really taken (results differ from the direct ones in the last bits) wherever the planner admits them; on the
    # wide-dilation production maps a tile size may be rejected (too much sub-lattice padding) and falls back to the direct kernel
    taken = [wino for wino in (4, 2) if not torch.equal(res[wino][0], res[0][0])]
    assert taken == [wino for wino in (4, 2) if wino_route(h, w, d, wino)] and 4 in taken, (case, taken)
    # F(4x4) with the point GEMMs and the output transform in ONE kernel (pm_set_winograd_fused: M = V U^T never reaches HBM): forward with the
    # fused epilogue into a channel slice, and the data gradient with its fused skip add, against the same fp64 truth; the kernel is really
    # taken (other bits than the two-pass form) wherever F(4x4) is
    K.set_winograd(4)
    K.set_winograd_fused(True)
    try:
        buf.zero_()
        yf = nchw(K.conv_fwd(xg, wg, 1, d, d, bias=b.cuda(), out=buf[..., 32:32 + cout])).clone()
        dxf = nchw(K.conv_bwd_data(dyg, wg, tuple(xg.shape), 1, d, d, add=addg))
    finally:
        K.set_winograd_fused(False)
    assert buf[..., :32].abs().max().item() == 0 and buf[..., 32 + cout:].abs().max().item() == 0
    assert rel(yf, y_ref.detach()) < 2e-5 and rel(dxf, xr.grad + add.double()) < 2e-5
    assert torch.equal(yf, res[4][0]) == (wino_route(h, w, d, 4) != 4)


@pytest.mark.parametrize('case', [(2, 64, 24, 20, 256, 1, 1, 0, 1), (3, 64, 45, 37, 64, 3, 1, 1, 1), (2, 256, 47, 33, 64, 1, 1, 0, 1), (1, 32, 40, 36, 128, 3, 2, 1, 1)])
def test_conv_epilogue_bn_statistics(K, case):
    """Train-mode BatchNorm statistics handed out by the convolution epilogue itself ((mean, M2) per 32-row slab, merged by
    pm_bn_partials_finalize) against the statistics pass over y (pm_bn_stats_finalize) and against torch on the same output: mean /
    invstd / running moments, incl. ragged last slabs (pixel counts that are no multiple of 32 or of the block tile) and the SyncBN
    moment format."""
    n, cin, h, w, cout, k, s, p, d = case
    x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    b = rnd(cout, seed=3)
    xg, wg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda()
    ps = []
    prev = K.BN_EPILOGUE
    K.BN_EPILOGUE = True                 # opt-in route (PM_BN_EPILOGUE=1): -0.2 ms/step in the same-box A/B, kept off for the gradient gates
    try:
        y = K.conv_fwd(xg, wg, s, p, d, bias=b.cuda(), bn_partials=ps)
    finally:
        K.BN_EPILOGUE = prev
    assert ps[0] is not None, 'this shape must take the epilogue-statistics route'
    pixels = y.shape[0] * y.shape[1] * y.shape[2]
    rm1, rv1 = torch.zeros(cout, device='cuda'), torch.ones(cout, device='cuda')
    rm2, rv2 = rm1.clone(), rv1.clone()
    mean1, inv1 = K.bn_partials_finalize(ps[0], pixels, cout, 1e-5, rm1, rv1, 0.1)
    mean2, inv2 = K.bn_stats_finalize(y, 1e-5, rm2, rv2, 0.1)
    yr = nchw(y).double()
    assert rel(mean1, yr.mean((0, 2, 3))) < 1e-6 and rel(inv1, 1.0 / torch.sqrt(yr.var((0, 2, 3), unbiased=False) + 1e-5)) < 1e-6
    assert rel(mean1, mean2) < 1e-6 and rel(inv1, inv2) < 1e-6 and rel(rm1, rm2) < 1e-6 and rel(rv1, rv2) < 1e-6
    mom = K.bn_partials_moments(ps[0], pixels, cout)
    assert rel(mom[:cout], yr.mean((0, 2, 3))) < 1e-6 and rel(mom[cout:2 * cout], ((yr - yr.mean((0, 2, 3), keepdim=True)) ** 2).sum((0, 2, 3))) < 1e-5
    assert torch.all(mom[2 * cout:] == pixels)
    # the same convolution without the request writes the same y
    assert torch.equal(K.conv_fwd(xg, wg, s, p, d, bias=b.cuda()), y)
    # routes that cannot emit the partials say so: Winograd (wide 3x3) and the 19-class head
    ps2 = []
    K.BN_EPILOGUE = True
    try:
        K.conv_fwd(nhwc(rnd(1, 128, 16, 16, seed=5)), rnd(128, 3, 3, 128, seed=6).cuda() * 0.05, 1, 1, 1, bn_partials=ps2)
        K.conv_fwd(nhwc(rnd(1, 64, 8, 8, seed=5)), rnd(19, 1, 1, 64, seed=6).cuda() * 0.05, 1, 0, 1, bn_partials=ps2)
        K.BN_EPILOGUE = False
        K.conv_fwd(xg, wg, s, p, d, bias=b.cuda(), bn_partials=ps2)          # switched off: the caller falls back to the statistics pass
    finally:
        K.BN_EPILOGUE = prev
    assert ps2 == [None, None, None]


@pytest.mark.parametrize('route', [1, 2, 0])
@pytest.mark.parametrize('case', [(2, 64, 24, 20, 256, 1, 1, 0, 1, False), (3, 64, 45, 37, 64, 3, 1, 1, 1, True), (2, 256, 47, 33, 128, 1, 1, 0, 1, False),
                                  (8, 128, 60, 52, 128, 3, 1, 2, 2, False), (8, 512, 48, 48, 256, 3, 1, 6, 6, False)])
def test_conv_epilogue_bn_statistics_bf16(K, case, route):
    """The same on the bf16 tier (round 4): both bf16 kernels (route 2: LDS-DMA everywhere, 0: register-staged everywhere, 1: the per-shape default) hand out
    the statistics of the ROUNDED bf16 output they store -- the tensor the BatchNorm reads -- so they must agree with the statistics pass over that tensor
    (pm_bn_stats_finalize on bf16) and with torch on its values, incl. ragged last slabs, a bias, and the SyncBN moment format; the output bits do not depend on
    the request."""
    n, cin, h, w, cout, k, s, p, d, with_bias = case
    x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    b = rnd(cout, seed=3).cuda() if with_bias else None
    K.set_conv_precision('bf16')
    K.set_conv16(route)
    try:
        xg, wg = K.cast(nhwc(x), torch.bfloat16), wt.permute(0, 2, 3, 1).contiguous().cuda()
        ps = []
        prev = K.BN_EPILOGUE16
        K.BN_EPILOGUE16 = True               # opt-in (PM_BN_EPILOGUE16=1): measured slower than the separate statistics pass, see hip/kernels.py
        try:
            y = K.conv_fwd(xg, wg, s, p, d, bias=b, bn_partials=ps)
        finally:
            K.BN_EPILOGUE16 = prev
        assert y.dtype == torch.bfloat16 and (ps[0] is not None or route != 1), 'the default routing must take the epilogue-statistics route on these shapes'
        assert torch.equal(K.conv_fwd(xg, wg, s, p, d, bias=b), y)
        if ps[0] is None:      # a forced kernel that splits K on this shape: no statistics, the caller runs the pass
            return
        pixels = y.shape[0] * y.shape[1] * y.shape[2]
        rm1, rv1 = torch.zeros(cout, device='cuda'), torch.ones(cout, device='cuda')
        rm2, rv2 = rm1.clone(), rv1.clone()
        mean1, inv1 = K.bn_partials_finalize(ps[0], pixels, cout, 1e-5, rm1, rv1, 0.1)
        mean2, inv2 = K.bn_stats_finalize(y, 1e-5, rm2, rv2, 0.1)
        yr = y.double().permute(0, 3, 1, 2)
        assert rel(mean1, yr.mean((0, 2, 3))) < 1e-6 and rel(inv1, 1.0 / torch.sqrt(yr.var((0, 2, 3), unbiased=False) + 1e-5)) < 1e-6
        assert rel(mean1, mean2) < 1e-6 and rel(inv1, inv2) < 1e-6 and rel(rm1, rm2) < 1e-6 and rel(rv1, rv2) < 1e-6
        mom = K.bn_partials_moments(ps[0], pixels, cout)
        assert rel(mom[cout:2 * cout], ((yr - yr.mean((0, 2, 3), keepdim=True)) ** 2).sum((0, 2, 3))) < 1e-5 and torch.all(mom[2 * cout:] == pixels)
        assert torch.equal(K.conv_fwd(xg, wg, s, p, d, bias=b), y)
        ps2 = []
        K.conv_fwd(xg, wg, s, p, d, bias=b, bn_partials=ps2)      # default: off, the caller runs the statistics pass
        assert ps2 == [None]
    finally:
        K.set_conv16(1)
        K.set_conv_precision('f32')


def test_conv_epilogue_and_slices(K):
    """eval-mode fold (scale/shift), residual, relu, and writing into a channel slice of a wider concat buffer."""
    x, wt = rnd(2, 64, 12, 12, seed=1), rnd(32, 64, 3, 3, seed=2, scale=0.05)
    sc, sh, res = rnd(32, seed=3).abs() + 0.5, rnd(32, seed=4), rnd(2, 32, 12, 12, seed=5)
    ref = torch.relu(F.conv2d(x, wt, padding=1) * sc[None, :, None, None] + sh[None, :, None, None] + res)
    buf = torch.zeros(2, 12, 12, 96, device='cuda')
    out = K.conv_fwd(nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), 1, 1, 1, scale=sc.cuda(), shift=sh.cuda(), residual=nhwc(res), relu=True,
                     out=buf[..., 32:64])
    assert rel(nchw(out), ref) < 2e-5
    assert buf[..., :32].abs().max().item() == 0 and buf[..., 64:].abs().max().item() == 0
    # dgrad fused accumulate
    dy, add = rnd(2, 32, 12, 12, seed=6), rnd(2, 64, 12, 12, seed=7)
    xr = x.clone().requires_grad_(True)
    F.conv2d(xr, wt, padding=1).backward(dy)
    dx = K.conv_bwd_data(nhwc(dy), wt.permute(0, 2, 3, 1).contiguous().cuda(), (2, 12, 12, 64), 1, 1, 1, add=nhwc(add))
    assert rel(nchw(dx), xr.grad + add) < 2e-5


@pytest.mark.parametrize('shape,relu,res', [((4, 64, 20, 20), True, False), ((2, 256, 9, 11), True, True), ((3, 48, 16, 16), False, False),
                                           ((8, 256, 1, 1), True, False)])
def test_batchnorm_train(K, shape, relu, res):
    n, c, h, w = shape
    x = rnd(*shape, seed=1) * 2 + 3
    r = rnd(*shape, seed=2) if res else None
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(rnd(c, seed=3) * 0.2 + 1), bn.bias.copy_(rnd(c, seed=4) * 0.1)
        bn.running_mean.copy_(rnd(c, seed=5)), bn.running_var.copy_(rnd(c, seed=6).abs() + 0.5)
    rm, rv = bn.running_mean.clone().cuda(), bn.running_var.clone().cuda()
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    y_ref = bn(xr)
    if res:
        y_ref = y_ref + rr
    if relu:
        y_ref = torch.relu(y_ref)
    dy = rnd(*shape, seed=7)
    y_ref.backward(dy)

    xg = nhwc(x)
    rm2, rv2 = rm.clone(), rv.clone()
    mom = K.bn_stats(xg)
    mean, invstd = K.bn_finalize(mom, c, bn.eps, rm, rv, 0.1)
    mean2, invstd2 = K.bn_stats_finalize(xg, bn.eps, rm2, rv2, 0.1)       # the fused local-statistics entry point: the same bits
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2) and torch.equal(rm, rm2) and torch.equal(rv, rv2)
    assert rel(mean, x.mean((0, 2, 3))) < 1e-5
    assert rel(rm, bn.running_mean) < 1e-5 and rel(rv, bn.running_var) < 1e-5
    g, b = bn.weight.detach().cuda(), bn.bias.detach().cuda()
    y = K.bn_apply(xg, mean, invstd, g, b, residual=nhwc(r) if res else None, relu=relu)
    assert rel(nchw(y), y_ref.detach()) < 1e-5
    dyg = nhwc(dy)
    sums, _ = K.bn_bwd_reduce(dyg, y, xg, mean, invstd, relu)
    dx, dres = K.bn_bwd_apply(dyg, y, xg, mean, invstd, g, sums, n * h * w, relu, res)
    assert rel(sums[:c], bn.bias.grad) < 2e-5 and rel(sums[c:], bn.weight.grad) < 2e-5
    assert rel(nchw(dx), xr.grad) < 5e-5
    if res:
        assert rel(nchw(dres), rr.grad) < 1e-6
    if relu and not res:     # mask rebuilt from x instead of read from y: the same bits
        sums2, _ = K.bn_bwd_reduce(dyg, None, xg, mean, invstd, 2, g, b)
        dx2, _ = K.bn_bwd_apply(dyg, None, xg, mean, invstd, g, sums2, n * h * w, 2, False, b)
        assert torch.equal(sums2, sums) and torch.equal(dx2, dx)
    if relu and res:         # reduce pass hands the masked gradient (= dres) to the apply pass
        sums3, gm = K.bn_bwd_reduce(dyg, y, xg, mean, invstd, 1, want_gmask=True)
        dx3, _ = K.bn_bwd_apply(gm, None, xg, mean, invstd, g, sums3, n * h * w, 0, False)
        assert torch.equal(sums3, sums) and torch.equal(dx3, dx) and torch.equal(gm, dres)
        # ... with the ReLU mask read from the byte per float4 group the forward left behind instead of the forward output: the same bits
        y_m, mask = K.bn_apply(xg, mean, invstd, g, b, residual=nhwc(r), relu=True, want_mask=True)
        assert torch.equal(y_m, y) and tuple(mask.shape) == (n * h * w, c // 4) and mask.dtype == torch.uint8
        assert torch.equal(((mask.view(n, h, w, c // 4, 1) >> torch.arange(4, device='cuda', dtype=torch.uint8)) & 1).view(n, h, w, c).bool(), y > 0)
        sums4, gm4 = K.bn_bwd_reduce_mask(dyg, mask, xg, mean, invstd)
        assert torch.equal(sums4, sums) and torch.equal(gm4, gm)


def test_pool_and_resize(K):
    x = rnd(2, 64, 21, 18, seed=1)
    xr = x.clone().requires_grad_(True)
    y_ref = F.max_pool2d(torch.relu(xr), 3, 2, 1)
    dy = rnd(*y_ref.shape, seed=2)
    y_ref.backward(dy)
    xg = nhwc(torch.relu(x))
    y, arg = K.maxpool_fwd(xg)
    assert rel(nchw(y), y_ref.detach()) == 0
    dx = K.maxpool_bwd(nhwc(dy), arg, tuple(xg.shape))
    dx = dx * (xg > 0)                                   # relu mask, as the full graph applies it
    assert rel(nchw(dx), xr.grad) < 1e-6

    x = rnd(3, 128, 7, 9, seed=3)
    xr = x.clone().requires_grad_(True)
    y_ref = F.adaptive_avg_pool2d(xr, 1)
    dy = rnd(3, 128, 1, 1, seed=4)
    y_ref.backward(dy)
    y = K.global_avgpool_fwd(nhwc(x))
    assert rel(nchw(y), y_ref.detach()) < 1e-6
    assert rel(nchw(K.global_avgpool_bwd(nhwc(dy), (3, 7, 9, 128))), xr.grad) < 1e-6

    for (shape, size) in [((2, 64, 12, 12), (48, 48)), ((2, 19, 24, 24), (96, 96)), ((2, 256, 1, 1), (12, 12)), ((1, 32, 11, 7), (30, 41)), ((1, 16, 13, 18), (50, 70)),
                          ((1, 8, 10, 10), (10, 10))]:
        x = rnd(*shape, seed=5)
        xr = x.clone().requires_grad_(True)
        y_ref = F.interpolate(xr, size=size, mode='bilinear', align_corners=True)
        dy = rnd(*y_ref.shape, seed=6)
        y_ref.backward(dy)
        xg = K.new((shape[0], shape[2], shape[3], shape[1]), torch.zeros(1, device='cuda'), pitch_pad=True)
        xg.copy_(nhwc(x))
        y = K.resize_fwd(xg, size)
        assert rel(nchw(y), y_ref.detach()) < 2e-6, (shape, size)
        if shape[1] % 4:      # pitch-padded 19-channel logits: float4 path over the padded width, pad lane written as zero
            assert y.stride(2) == 20 and y.as_strided((y.shape[0], y.shape[1], y.shape[2], 20), y.stride())[..., 19].abs().max().item() == 0
            xs = nhwc(x)      # unpadded (pitch 19) view of the same data takes the scalar path: same result
            assert rel(K.resize_fwd(xs, size), y) < 1e-6
        dyg = K.new(tuple(y.shape), y, pitch_pad=True)
        dyg.copy_(nhwc(dy))
        dx = K.resize_bwd(dyg, tuple(xg.shape))             # separable (column pass + row pass) where the up-sampling ratio is >= 2
        assert rel(nchw(dx), xr.grad) < 1e-5, (shape, size)
        dx_g = K.resize_bwd(dyg, tuple(xg.shape), separable=False)      # the gather formulation: same operator, other summation order
        assert rel(nchw(dx_g), xr.grad) < 1e-5 and rel(dx, dx_g) < 2e-6, (shape, size)


@pytest.mark.parametrize('h,w,crop,overlap', [(160, 288, 128, 1.0 / 3), (96, 200, 64, 0.5), (128, 128, 128, 1.0 / 3)])
def test_sliding_stitch(K, h, w, crop, overlap):
    """pm_sliding_stitch against the host formulation of eval.py:210-274 (float64 sum in tile order / count, un-flip, add the flips):
    same additions in the same order, so the same bits."""
    from pinthememory_amd import harness
    tiles = harness.sliding_tiles(h, w, crop, overlap)
    acc, ref = None, None
    for flip in (False, True):
        lg = rnd(len(tiles), 19, crop, crop, seed=5 + flip)
        full = torch.zeros(19, h, w, dtype=torch.float64)
        cnt = torch.zeros(1, h, w, dtype=torch.float64)
        for i, (x1, y1, x2, y2) in enumerate(tiles):
            full[:, y1:y2, x1:x2] += lg[i].double()
            cnt[:, y1:y2, x1:x2] += 1
        full = full / cnt
        if flip:
            full = torch.flip(full, dims=[2])
        ref = full if ref is None else ref + full
        acc = K.sliding_stitch(nhwc(lg), tiles, h, w, flip, acc)
    assert torch.equal(acc.cpu(), ref)
    with pytest.raises(RuntimeError):
        K.sliding_stitch(nhwc(lg), [(0, 0, crop + 1, crop)] * len(tiles), h, w, False)


def test_winograd_filter_cache(K):
    """The transformed filter U is kept between forward calls on the same weight storage and recomputed when the tensor version moves:
    torch's in-place ops bump it, the fused SGD bumps it explicitly (optim.SGD) -- a stale U would show as the old weights' output."""
    from pinthememory_amd import optim
    x = nhwc(rnd(2, 128, 24, 24, seed=1))
    w = torch.nn.Parameter(rnd(128, 128, 3, 3, seed=2).mul(0.05).cuda().contiguous(memory_format=torch.channels_last))
    wk = w.detach().permute(0, 2, 3, 1)                       # KRSC view of the parameter's own memory
    assert wk.data_ptr() == w.data_ptr() and wk.is_contiguous()
    ref = lambda: F.conv2d(nchw(x), w.detach().cpu(), padding=1)
    K.clear_filters()
    K.unregister_filter_owners()
    was = K.KEEP_WINOGRAD_U
    K.KEEP_WINOGRAD_U = None                                  # the default: only weights an optimizer registered are cached
    y0 = K.conv_fwd(x, wk, 1, 1, 1)
    assert len(K._U_CACHE) == 0                               # nobody vouches for this weight: never cached ...
    with torch.no_grad():
        w.data.mul_(2.0)                                      # ... so a write through .data (no version bump) cannot meet a stale filter
    assert rel(nchw(K.conv_fwd(x, wk, 1, 1, 1)), ref()) < 2e-5 and len(K._U_CACHE) == 0
    with torch.no_grad():
        w.data.mul_(0.5)
    assert torch.equal(K.conv_fwd(x, wk, 1, 1, 1), y0)
    opt = optim.SGD([w], lr=0.1, momentum=0.9, weight_decay=0.0)      # the owner: registers w, bumps its version in step()
    y1 = K.conv_fwd(x, wk, 1, 1, 1)
    assert torch.equal(y1, y0)
    theta = w.detach().clone(memory_format=torch.preserve_format)      # a functional weight (mldg's theta): not registered, not cached, not retained
    K.conv_fwd(x, theta.permute(0, 2, 3, 1), 1, 1, 1)
    assert len(K._U_CACHE) == 1
    assert len(K._U_CACHE) == 1 and rel(nchw(y1), ref()) < 2e-5
    ent = next(iter(K._U_CACHE.values()))
    u_before = ent.buf.clone()
    y2 = K.conv_fwd(x, wk, 1, 1, 1)                           # hit: same bits, U untouched
    assert torch.equal(y1, y2) and torch.equal(ent.buf, u_before) and len(K._U_CACHE) == 1
    with torch.no_grad():
        w.mul_(0.5)                                           # torch in-place op: version bump -> recomputed
    y3 = K.conv_fwd(x, wk, 1, 1, 1)
    assert rel(nchw(y3), ref()) < 2e-5 and not torch.equal(ent.buf, u_before)
    w.grad = torch.ones_like(w)                               # one fused SGD step (raw-pointer update inside the library)
    opt.step()
    y4 = K.conv_fwd(x, wk, 1, 1, 1)
    assert rel(nchw(y4), ref()) < 2e-5 and rel(y4, y3) > 1e-3
    K.KEEP_WINOGRAD_U = False
    try:
        assert torch.equal(K.conv_fwd(x, wk, 1, 1, 1), y4)
        K.KEEP_WINOGRAD_U = None
        K.unregister_filter_owners([w])                       # the owner lets go: entries dropped, nothing cached afterwards
        assert len(K._U_CACHE) == 0
        assert torch.equal(K.conv_fwd(x, wk, 1, 1, 1), y4) and len(K._U_CACHE) == 0
    finally:
        K.KEEP_WINOGRAD_U = was


def test_filter_cache_eviction(K):
    """Who leaves the filter cache, and when: a miss over the byte cap evicts the oldest entry, a hit makes its entry the youngest, entries whose owner is gone are
    swept by the next miss before anything live goes, and unregister + clear leave nothing. Every output has the bits of the same call without the cache."""
    import gc
    from pinthememory_amd import optim
    x = nhwc(rnd(2, 128, 24, 24, seed=1))                     # test_winograd_filter_cache's shape: the smallest that takes the Winograd route and keeps a transform
    ws = {n: torch.nn.Parameter(rnd(128, 128, 3, 3, seed=2 + i).mul(0.05).cuda().contiguous(memory_format=torch.channels_last)) for i, n in enumerate('abc')}
    conv = lambda n: K.conv_fwd(x, ws[n].detach().permute(0, 2, 3, 1), 1, 1, 1)
    owners = lambda: [next((n for n, w in ws.items() if w is e.owner()), None) for e in K._U_CACHE.values()]      # names, oldest entry first; None: the owner is gone
    K.clear_filters()
    K.unregister_filter_owners()
    was, cap = K.KEEP_WINOGRAD_U, K._U_CACHE_BYTES
    try:
        K.KEEP_WINOGRAD_U = False
        want = {n: conv(n) for n in 'abc'}
        K.KEEP_WINOGRAD_U = None
        opt = optim.SGD(list(ws.values()), lr=0.1, momentum=0.9, weight_decay=0.0)
        got = [('a', conv('a'))]
        first = next(iter(K._U_CACHE.values()))
        assert len(K._U_CACHE) == 1 and first.owner() is ws['a'] and first.nbytes == first.buf.numel() * 4
        K._U_CACHE_BYTES = first.nbytes * 5 // 2                  # room for two transforms, not for three
        got += [('b', conv('b')), ('c', conv('c'))]
        assert owners() == ['b', 'c']                             # (1) a was the oldest
        kept_b = next(iter(K._U_CACHE.values())).buf
        got += [('b', conv('b')), ('a', conv('a'))]
        assert owners() == ['b', 'a']                             # (2) the hit on b made c the oldest
        assert next(iter(K._U_CACHE.values())).buf is kept_b      # a hit never reallocates
        opt.param_groups[0]['params'][:] = [ws['b'], ws['c']]
        del ws['a']                                               # the youngest entry: the byte cap alone would evict b and keep it
        gc.collect()
        got.append(('c', conv('c')))
        assert owners() == ['b', 'c']                             # (3) the miss swept the dead owner's entry first
        for n, y in got:
            assert torch.equal(y, want[n]), n                     # (4)
        K.unregister_filter_owners()
        K.clear_filters()
        assert len(K._U_CACHE) == 0                               # (5)
    finally:
        K.KEEP_WINOGRAD_U, K._U_CACHE_BYTES = was, cap
        K.unregister_filter_owners()
        K.clear_filters()


def test_layout_and_labels(K):
    x = rnd(2, 3, 37, 41, seed=1).cuda()
    y = K.nchw_to_nhwc(x, c_pad=4)
    assert torch.equal(y[..., :3], x.permute(0, 2, 3, 1)) and y[..., 3].abs().max().item() == 0
    for c, cp in ((3, 3), (1, 4), (4, 4), (2, 2), (5, 8), (3, 8)):       # thread-per-pixel image kernel (<= 4 channels) and the tiled transpose beyond
        xs = rnd(3, c, 19, 23, seed=10 + c).cuda()
        ys = K.nchw_to_nhwc(xs, c_pad=cp)
        assert torch.equal(ys[..., :c], xs.permute(0, 2, 3, 1)) and (cp == c or ys[..., c:].abs().max().item() == 0)
    z = rnd(2, 19, 9, 13, seed=2)
    assert torch.equal(K.nhwc_to_nchw(nhwc(z)).cpu(), z)
    lab = torch.randint(0, 19, (2, 64, 48), generator=torch.Generator().manual_seed(3))
    ref = F.interpolate(lab.unsqueeze(1).float(), size=(4, 3), mode='nearest').squeeze(1).long()
    assert torch.equal(K.label_nearest(lab.cuda(), (4, 3)).cpu(), ref)
    ref = F.interpolate(lab.unsqueeze(1).float(), size=(9, 7), mode='nearest').squeeze(1).long()
    assert torch.equal(K.label_nearest(lab.cuda(), (9, 7)).cpu(), ref)


@pytest.mark.parametrize('hw,HW,temp,C', [((12, 12), (48, 48), 1.0, 19), ((6, 6), (96, 96), 0.5, 19), ((16, 16), (16, 16), 1.0, 19), ((5, 7), (33, 29), 2.0, 19),
                                          ((1, 1), (8, 8), 1.0, 19), ((24, 24), (384, 384), 0.07, 19), ((9, 9), (4, 6), 1.0, 19), ((7, 5), (30, 41), 1.0, 8),
                                          ((192, 48), (768, 192), 1.0, 19), ((3, 300), (7, 611), 1.0, 19), ((2, 130), (5, 2100), 1.0, 19), ((4, 4), (4, 700), 1.0, 5),
                                          # the interval form of the training forward (19 classes, <= 256 low-res columns, up-sampling ratio < 8): several waves per row group
                                          # (B handed across wave edges), intervals with one row more than the others, ratio 1 and ~2, the flagship's 192 columns
                                          ((48, 192), (192, 768), 1.0, 19), ((10, 70), (25, 200), 0.5, 19), ((33, 65), (65, 129), 1.0, 19), ((20, 256), (41, 520), 1.0, 19),
                                          ((7, 100), (50, 399), 1.0, 19)])
def test_upsample_ce(K, hw, HW, temp, C):
    n = 2
    lg = rnd(n, C, *hw, seed=1) * 3
    g = torch.Generator().manual_seed(2)
    lab = torch.randint(0, C, (n, *HW), generator=g)
    lab[torch.rand(n, *HW, generator=g) < 0.1] = 255
    lab[:, :2] = 255
    # the gradient reference is the fp64 evaluation of the reference's expression: torch's own fp32 gradient sits up to 2.2e-5 (of the largest
    # entry) from it on the wide two-fold up-sampling cases, the kernels 8e-6 (tools/ce_dbg.py)
    lr = lg.double().requires_grad_(True)
    loss_ref = F.cross_entropy(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), lab, ignore_index=255)
    (loss_ref * 1.7).backward()
    loss_ref = F.cross_entropy(F.interpolate(lg / temp, size=HW, mode='bilinear', align_corners=True), lab, ignore_index=255)     # the loss itself: fp32 as the reference runs it
    lgg = K.new((n, hw[0], hw[1], C), torch.zeros(1, device='cuda'), pitch_pad=True)
    lgg.copy_(nhwc(lg))
    labg = lab.cuda()
    out = K.upsample_ce_fwd(lgg, labg, 1.0 / temp)
    assert abs(out[0].item() - loss_ref.item()) < 2e-6 * max(1, abs(loss_ref.item()))
    assert out[1].item() == (lab != 255).sum().item()
    dl = K.upsample_ce_bwd(lgg, labg, out, torch.tensor([1.7], device='cuda'), 1.0 / temp)
    assert rel(nchw(dl), lr.grad) < 2e-5
    # the training forward that leaves the column-reduced gradient field behind + the row-pass-only backward (one sweep over the labels per step)
    out_f, field = K.upsample_ce_fwd_field(lgg, labg, 1.0 / temp)
    assert abs(out_f[0].item() - loss_ref.item()) < 2e-6 * max(1, abs(loss_ref.item())) and out_f[1].item() == out[1].item()
    dlf = K.upsample_ce_bwd_field(lgg, HW, out_f, field, torch.tensor([1.7], device='cuda'), 1.0 / temp)
    assert rel(nchw(dlf), lr.grad) < 2e-5 and rel(dlf, dl) < 1e-5
    out_f2, field2 = K.upsample_ce_fwd_field(lgg, labg, 1.0 / temp)
    assert torch.equal(out_f, out_f2) and torch.equal(field, field2)                       # fixed association order: run-to-run deterministic
    # edge cases of the reference's criterion (CrossEntropyLoss(ignore_index=255), loss.py:38-39): one image with every pixel ignored
    # contributes nothing; a batch with every pixel ignored gives NaN (0 / 0) exactly as torch does, and a valid-pixel count of zero
    lab1 = lab.clone()
    lab1[0] = 255
    ref1 = F.cross_entropy(F.interpolate(lg / temp, size=HW, mode='bilinear', align_corners=True), lab1, ignore_index=255)
    out1 = K.upsample_ce_fwd(lgg, lab1.cuda(), 1.0 / temp)
    assert abs(out1[0].item() - ref1.item()) < 2e-6 * max(1, abs(ref1.item())) and out1[1].item() == (lab1 != 255).sum().item()
    dl1 = K.upsample_ce_bwd(lgg, lab1.cuda(), out1, None, 1.0 / temp)
    assert nchw(dl1)[0].abs().max().item() == 0.0                      # no gradient into the fully ignored image
    out0 = K.upsample_ce_fwd(lgg, torch.full_like(lab, 255).cuda(), 1.0 / temp)
    assert torch.isnan(out0[0]).item() and out0[1].item() == 0
    o1f, f1 = K.upsample_ce_fwd_field(lgg, lab1.cuda(), 1.0 / temp)
    assert abs(o1f[0].item() - ref1.item()) < 2e-6 * max(1, abs(ref1.item())) and o1f[1].item() == out1[1].item()
    assert nchw(K.upsample_ce_bwd_field(lgg, HW, o1f, f1, None, 1.0 / temp))[0].abs().max().item() == 0.0
    o0f, _ = K.upsample_ce_fwd_field(lgg, torch.full_like(lab, 255).cuda(), 1.0 / temp)
    assert torch.isnan(o0f[0]).item() and o0f[1].item() == 0


def test_memory_read(K):
    n, h, w, d, m = 2, 9, 7, 256, 19
    x = torch.relu(rnd(n, d, h, w, seed=1))
    x[0, :, 0, 0] = 0                                     # an all-zero row exercises the eps clamp
    mem = F.normalize(rnd(m, d, seed=2), dim=1)
    xr = x.clone().requires_grad_(True)
    mr = mem.clone().requires_grad_(True)
    q = F.normalize(xr, dim=1).permute(0, 2, 3, 1).contiguous()
    s = torch.matmul(q, mr.t()).view(-1, m)
    pq, pm = F.softmax(s, 0), F.softmax(s, 1)
    qr_ref = torch.cat((q.view(-1, d), torch.matmul(pm, mr)), 1)
    dqr, dsx = rnd(n * h * w, 2 * d, seed=3), rnd(n * h * w, m, seed=4) * 0.1
    ((qr_ref * dqr).sum() + (s * dsx).sum()).backward()

    xg, memg = nhwc(x), mem.cuda()
    qr, score, pmem = K.mem_read_fwd(xg, memg)
    assert rel(qr.view(-1, 2 * d), qr_ref.detach()) < 2e-6
    assert rel(score, s.detach()) < 2e-6 and rel(pmem, pm.detach()) < 2e-6
    assert rel(K.mem_colsoftmax(score), pq.detach()) < 2e-6
    dx, dmem = K.mem_read_bwd(xg, memg, pmem, dqr.view(n, h, w, 2 * d).cuda(), dsx.cuda(), want_dmem=True)
    assert rel(nchw(dx)[:, :, 1:], xr.grad[:, :, 1:]) < 2e-5
    assert rel(dmem, mr.grad) < 2e-5
    # dx alone (m_items detached: the training step's case) takes the MFMA kernel; the row kernel above is the dmem variant
    dx2, none = K.mem_read_bwd(xg, memg, pmem, dqr.view(n, h, w, 2 * d).cuda(), dsx.cuda())
    assert none is None and rel(nchw(dx2)[:, :, 1:], xr.grad[:, :, 1:]) < 2e-5
    assert rel(dx2, dx) < 1e-5                           # incl. the all-zero row (gradient scaled by 1 / eps in both)
    dx3, _ = K.mem_read_bwd(xg, memg, pmem, dqr.view(n, h, w, 2 * d).cuda(), None)
    dx4, _ = K.mem_read_bwd(xg, memg, pmem, dqr.view(n, h, w, 2 * d).cuda(), None, want_dmem=True)
    assert rel(dx3[:, 1:], dx4[:, 1:]) < 1e-5
    m7 = F.normalize(rnd(7, d, seed=6), dim=1).cuda()    # a slot count without a specialised instantiation
    _, _, p7 = K.mem_read_fwd(xg, m7)
    a7, _ = K.mem_read_bwd(xg, m7, p7, dqr.view(n, h, w, 2 * d).cuda(), dsx[:, :7].contiguous().cuda())
    b7, _ = K.mem_read_bwd(xg, m7, p7, dqr.view(n, h, w, 2 * d).cuda(), dsx[:, :7].contiguous().cuda(), want_dmem=True)
    assert rel(a7[:, 1:], b7[:, 1:]) < 1e-5
    # gumbel path with injected noise (memory.py:181-184): softmax((S + g) / 1)
    noise = -torch.empty(n * h * w, m).exponential_(generator=torch.Generator().manual_seed(5)).log()
    _, _, pg = K.mem_read_fwd(xg, memg, noise.cuda())
    assert rel(pg, F.softmax(s.detach() + noise, 1)) < 2e-6
    assert rel(K.mem_colsoftmax(score, noise.cuda()), F.softmax(s.detach() + noise, 0)) < 2e-6
    # ... and its BACKWARD (the default configuration reads with noise, deepv3plus.py:472): d/dx through R = softmax(S + g) M and the concat
    # half, both kernels (MFMA dx-only and the dmem row kernel), against autograd of the same formula with the same noise
    xn, mn = x.clone().requires_grad_(True), mem.clone().requires_grad_(True)
    qn = F.normalize(xn, dim=1).permute(0, 2, 3, 1).contiguous()
    sn = torch.matmul(qn, mn.t()).view(-1, m)
    qrn = torch.cat((qn.view(-1, d), torch.matmul(F.softmax(sn + noise, 1), mn)), 1)
    ((qrn * dqr).sum() + (sn * dsx).sum()).backward()
    qg, _, _ = K.mem_read_fwd(xg, memg, noise.cuda())
    assert rel(qg.view(-1, 2 * d), qrn.detach()) < 2e-6
    dxn, dmn = K.mem_read_bwd(xg, memg, pg, dqr.view(n, h, w, 2 * d).cuda(), dsx.cuda(), want_dmem=True)
    assert rel(nchw(dxn)[:, :, 1:], xn.grad[:, :, 1:]) < 2e-5 and rel(dmn, mn.grad) < 2e-5
    dxn2, _ = K.mem_read_bwd(xg, memg, pg, dqr.view(n, h, w, 2 * d).cuda(), dsx.cuda())
    assert rel(nchw(dxn2)[:, :, 1:], xn.grad[:, :, 1:]) < 2e-5
    assert rel(nchw(dxn2)[:, :, 1:], xr.grad[:, :, 1:]) > 1e-3          # the noise does change the gradient: the comparison above is not vacuous
    # read + p_query from the read kernel's column partials (pm_mem_read_fwd_pq): same q / S / P_m bits as the plain read, p_query against torch, with
    # the two INDEPENDENT gumbel draws of memory.py:183-184 (126 rows = three full 32-row tiles + a ragged one)
    noise_q = -torch.empty(n * h * w, m).exponential_(generator=torch.Generator().manual_seed(7)).log()
    for nz, nq in ((None, None), (noise, noise_q), (None, noise_q)):
        qa, sa, pa, pqa = K.mem_read_fwd_pq(xg, memg, nz.cuda() if nz is not None else None, nq.cuda() if nq is not None else None)
        qb, sb, pb = K.mem_read_fwd(xg, memg, nz.cuda() if nz is not None else None)
        assert torch.equal(qa, qb) and torch.equal(sa, sb) and torch.equal(pa, pb)
        assert rel(pqa, F.softmax(s.detach() + (nq if nq is not None else 0), 0)) < 2e-6
        assert abs(pqa.sum(0) - 1).max().item() < 1e-5
    _, s7, _, pq7 = K.mem_read_fwd_pq(xg, m7)
    assert rel(pq7, F.softmax(s7.cpu(), 0)) < 2e-6


def test_memory_read_pq_at_the_flagship_row_count(K):
    """18 432 queries (bs=8, 48 x 48): 576 tiles of column partials merged in fixed order; twice the same bits."""
    n, h, w, d, m = 8, 48, 48, 256, 19
    xg = torch.relu(rnd(n, h, w, d, seed=11)).cuda()
    memg = F.normalize(rnd(m, d, seed=12), dim=1).cuda()
    _, sc, pm_, pq = K.mem_read_fwd_pq(xg, memg)
    ref = F.softmax(sc.double(), 0)
    assert rel(pq.double(), ref) < 2e-6 and abs(pq.double().sum(0) - 1).max().item() < 1e-5
    assert rel(K.mem_colsoftmax(sc), ref.float()) < 2e-6
    _, _, _, pq2 = K.mem_read_fwd_pq(xg, memg)
    assert torch.equal(pq, pq2)


def test_memory_read_more_rows_than_resident_tiles(K):
    """> 98 304 rows: the 32-row tiles outnumber the launched blocks (3072), so every block walks several tiles (grid-stride path of the
    MFMA read kernels, with a ragged last tile); forward and the dx-only backward against torch. Then read + p_query with a noise_q: the read kernel writes its
    column partials from that grid-stride loop (3 081 tiles on the 3 072-block cap) and the apply kernel merges 3 081 > 768 = 32 x CSA_PER of them, which only
    its re-reading branch does; p_query against fp64 at 2e-6, its columns sum to 1 within 1e-5, and mem_colsoftmax (771 partials of 128 rows) agrees at 2e-6."""
    n, h, w, d, m = 1, 317, 311, 256, 19                      # 98 587 rows = 3080 tiles + 27 rows
    x = torch.relu(rnd(n, d, h, w, seed=11))
    mem = F.normalize(rnd(m, d, seed=12), dim=1)
    xr = x.clone().requires_grad_(True)
    q = F.normalize(xr, dim=1).permute(0, 2, 3, 1).contiguous()
    s = torch.matmul(q, mem.t()).view(-1, m)
    pm = F.softmax(s, 1)
    qr_ref = torch.cat((q.view(-1, d), torch.matmul(pm, mem)), 1)
    dqr, dsx = rnd(n * h * w, 2 * d, seed=13), rnd(n * h * w, m, seed=14) * 0.1
    ((qr_ref * dqr).sum() + (s * dsx).sum()).backward()
    xg, memg = nhwc(x), mem.cuda()
    qr, score, pmem = K.mem_read_fwd(xg, memg)
    assert rel(qr.view(-1, 2 * d), qr_ref.detach()) < 2e-6 and rel(score, s.detach()) < 2e-6 and rel(pmem, pm.detach()) < 2e-6
    dx, _ = K.mem_read_bwd(xg, memg, pmem, dqr.view(n, h, w, 2 * d).cuda(), dsx.cuda())
    live = (x.abs().sum(1, keepdim=True) > 0).expand_as(x)   # rows that are all zero after the ReLU take the eps branch (torch: different sub-gradient)
    assert rel(nchw(dx)[live], xr.grad[live]) < 2e-5
    # read + p_query on the same rows: the only place where the column partials are WRITTEN from the grid-stride loop (3 081 tiles on 3 072 blocks, colpart at
    # tile = row0 >> 5) and MERGED by the branch of the apply kernel that re-reads its partials (ceil(3081 / 32) = 97 > 24 per thread). Same q / score / p_mem bits as
    # the plain read; p_query against the fp64 softmax of the kernel's own score plus the noise (torch's fp32 softmax over 98 587 rows is itself 5.5e-4 off)
    noise_q = (-torch.empty(n * h * w, m).exponential_(generator=torch.Generator().manual_seed(15)).log()).cuda()
    qa, sa, pa, pq = K.mem_read_fwd_pq(xg, memg, None, noise_q)
    assert torch.equal(qa, qr) and torch.equal(sa, score) and torch.equal(pa, pmem)
    pq_ref = F.softmax(score.double().cpu() + noise_q.double().cpu(), 0)
    assert rel(pq, pq_ref) < 2e-6 and abs(pq.double().sum(0) - 1).max().item() < 1e-5
    assert rel(K.mem_colsoftmax(score, noise_q), pq_ref) < 2e-6      # 771 partials of 128 rows: the same branch


def test_memory_write(K):
    n, h, w, d, m, H, W = 2, 6, 5, 256, 19, 48, 40
    z = torch.relu(rnd(n, d, h, w, seed=1))
    g = torch.Generator().manual_seed(2)
    lab = torch.randint(0, 12, (n, H, W), generator=g)      # classes 12..18 absent -> slots keep their value
    lab[torch.rand(n, H, W, generator=g) < 0.1] = 255
    mem = F.normalize(rnd(m, d, seed=3), dim=1)
    mu = 0.8
    zr = z.clone().requires_grad_(True)
    zh = F.normalize(zr, dim=1).view(n, d, -1)
    t = lab.clone()
    t[t == 255] = m
    y = F.interpolate(F.one_hot(t, m + 1).permute(0, 3, 1, 2).float(), [h, w], mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(n, -1, m + 1)
    nom, den = torch.matmul(zh, y).sum(0).t(), y.sum(1).sum(0)
    upd = mem.clone()
    for j in range(m):
        if den[j] != 0:
            upd[j] = mu * mem[j] + (1 - mu) * nom[j] / den[j]
    new = F.normalize(upd, dim=1)
    dout = rnd(m, d, seed=4)
    (new * dout).sum().backward()

    zg, labg = nhwc(z), lab.cuda()
    nomden = K.mem_write_accum(zg, labg, m)
    assert rel(nomden[:(m + 1) * d].view(m + 1, d), nom.detach()) < 2e-6
    assert rel(nomden[(m + 1) * d:], den) < 2e-6
    out, u = K.mem_write_update(mem.cuda(), nomden, mu, want_u=True)
    assert rel(out, new.detach()) < 2e-6
    assert rel(out[12:], mem[12:]) < 1e-6                 # absent classes keep their slot (memory.py:235)
    dnom = K.mem_write_update_bwd(u, nomden, mu, dout.cuda())
    dz = K.mem_write_accum_bwd(zg, labg, m, dnom)
    assert rel(nchw(dz), zr.grad) < 2e-5


@pytest.mark.parametrize('n,h,w,H,W,m', [(2, 24, 24, 192, 192, 19),      # 18 chunks of 64 rows, one per block
                                         (8, 48, 48, 768, 768, 19),      # the flagship: 288 chunks
                                         (4, 96, 100, 200, 333, 19),     # 600 chunks on 512 blocks: blocks that carry two chunks; ragged last chunk; odd sizes
                                         (1, 9, 7, 30, 20, 6)])          # one ragged chunk, a slot count whose partial slab is not 16-byte sized
def test_memory_write_accum_on_the_matrix_cores(K, n, h, w, H, W, m):
    """pm_mem_write_accum (split-K MFMA form) against the one-hot -> F.interpolate -> matmul formulation of memory.py:219-231 in fp64."""
    d = 256
    z = torch.relu(rnd(n, d, h, w, seed=21))
    z[0, :, 0, 0] = 0                                       # eps clamp
    g = torch.Generator().manual_seed(22)
    lab = torch.randint(0, max(2, m - 3), (n, H, W), generator=g)
    lab[torch.rand(n, H, W, generator=g) < 0.1] = 255
    t = lab.clone()
    t[t == 255] = m
    y = F.interpolate(F.one_hot(t, m + 1).permute(0, 3, 1, 2).double(), [h, w], mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(n, -1, m + 1)
    zh = F.normalize(z.double(), dim=1).view(n, d, -1)
    nom, den = torch.matmul(zh, y).sum(0).t(), y.sum(1).sum(0)
    zg, labg = nhwc(z), lab.cuda()
    nomden = K.mem_write_accum(zg, labg, m)
    assert rel(nomden[:(m + 1) * d].view(m + 1, d), nom) < 3e-6
    assert rel(nomden[(m + 1) * d:], den) < 3e-6
    assert torch.equal(nomden, K.mem_write_accum(zg, labg, m))          # fixed-order reduce: run-to-run identical
    raw = K.mem_write_accum(zg, labg, m, normalize=False)
    nom_raw = torch.matmul(z.double().view(n, d, -1), y).sum(0).t()
    assert rel(raw[:(m + 1) * d].view(m + 1, d), nom_raw) < 3e-6


def test_sgd(K):
    p, g = rnd(1000, seed=1), rnd(1000, seed=2)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.01, momentum=0.9, weight_decay=5e-4)
    pg, buf = p.cuda(), torch.zeros(1000, device='cuda')
    for it in range(3):
        pr.grad = g.clone() * (it + 1)
        opt.step()
        K.sgd_momentum(pg, (g * (it + 1)).cuda(), buf, 0.01, 0.9, 5e-4, it == 0)
    assert rel(pg, pr.detach()) < 1e-6


def test_sgd_multi_tensor_optimizer(K):
    """pinthememory_amd.optim.SGD (one pm_sgd_momentum_multi launch for all tensors) against torch.optim.SGD on the same parameters / gradients:
    mixed shapes (channels-last 4-D weights, odd lengths, one tensor larger than a chunk), three steps, LR changed in between, then a
    state_dict round trip through torch's own optimizer."""
    from pinthememory_amd.optim import SGD
    shapes = [(64, 3, 7, 7), (19,), (256, 64, 1, 1), (5001,), (128, 128, 3, 3), (1,)]
    ref = [rnd(*s, seed=i).requires_grad_(True) for i, s in enumerate(shapes)]
    got = [t.detach().clone().cuda() for t in ref]
    got = [(t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t).requires_grad_(True) for t in got]
    o_ref = torch.optim.SGD(ref, lr=0.01, momentum=0.9, weight_decay=5e-4)
    o_got = SGD(got, lr=0.01, momentum=0.9, weight_decay=5e-4)
    for it in range(3):
        for i, (a, b) in enumerate(zip(ref, got)):
            g = rnd(*a.shape, seed=100 + 10 * it + i)
            a.grad = g.clone()
            b.grad = (g.cuda().contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g.cuda())
        for o in (o_ref, o_got):
            o.param_groups[0]['lr'] = 0.01 * (0.5 ** it)
            o.step()
        for a, b in zip(ref, got):
            assert rel(b.detach(), a.detach()) < 2e-7          # same formula; CPU / GPU fma contraction may differ in the last bit
            assert rel(o_got.state[b]['momentum_buffer'], o_ref.state[a]['momentum_buffer']) < 2e-7
    sd = o_got.state_dict()
    assert sorted(sd['state'].keys()) == list(range(len(shapes))) and all('momentum_buffer' in v for v in sd['state'].values())
    o2 = torch.optim.SGD([t.detach().clone().requires_grad_(True) for t in got], lr=0.01, momentum=0.9, weight_decay=5e-4)
    o2.load_state_dict(sd)                                  # the reference's checkpoint 'optimizer' entry: interchangeable with torch's own


def test_bn_merge(K):
    """SyncBN moment merge kernel == the host formula used by the gloo tests == statistics of the concatenated batch."""
    from pinthememory_amd import dist as D
    c = 48
    x = rnd(6, c, 7, 5, seed=1) * 2 + 1
    parts = []
    for r in range(3):
        xl = x[r * 2:r * 2 + 2]
        mean = xl.mean((0, 2, 3))
        parts.append(torch.cat([mean, ((xl - mean[None, :, None, None]) ** 2).sum((0, 2, 3)), torch.full((c,), float(xl.numel() // c))]))
    got = K.bn_merge(torch.stack(parts).cuda().contiguous(), 3, c).cpu()
    assert rel(got, D.merge_moments_list(parts, c)) < 1e-6
    assert rel(got[:c], x.mean((0, 2, 3))) < 1e-6 and rel(got[c:2 * c], ((x - x.mean((0, 2, 3))[None, :, None, None]) ** 2).sum((0, 2, 3))) < 1e-5
    # merge + finalize in one launch (the SyncBN forward path) == the two separate launches, bit for bit, running moments included
    gp = torch.stack(parts).cuda().contiguous()
    rm1, rv1 = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    rm2, rv2 = rm1.clone(), rv1.clone()
    mean1, inv1 = K.bn_finalize(K.bn_merge(gp, 3, c), c, 1e-5, rm1, rv1, 0.1)
    mean2, inv2 = K.bn_merge_finalize(gp, 3, c, 1e-5, rm2, rv2, 0.1)
    assert torch.equal(mean1, mean2) and torch.equal(inv1, inv2) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2)


BF16_CASES = [CONV_CASES[1], CONV_CASES[3], CONV_CASES[5], CONV_CASES[8], CONV_CASES[9], CONV_CASES[10],
              (2, 256, 24, 24, 128, 3, 1, 6, 6, False),        # dilated 3x3, every K-slab inside one tap
              (1, 1280, 16, 16, 256, 1, 1, 0, 1, False),       # bot_aspp: long K
              (2, 96, 19, 21, 80, 3, 1, 1, 1, False),          # channels padded 96 -> 128 by the cast, ragged tiles
              (1, 512, 12, 12, 512, 3, 1, 2, 2, False)]


@pytest.mark.parametrize('form', ['bf16_operands', 'bf16_staged', 'bf16_operands+wgrad'])
@pytest.mark.parametrize('case', BF16_CASES)
def test_conv_bf16_operands(K, case, form):
    """BASELINE configs[2]: operands rounded to bf16 (RNE) feeding v_mfma_f32_32x32x16_bf16, fp32 accumulation -- the bf16-operand form
    (bf16 in HBM and LDS, csrc/bf16.hip) and the staged-fp32 form it falls back to. Oracle: the same convolution in fp32 on inputs
    pre-rounded to bf16 -- only the accumulation order differs."""
    n, cin, h, w, cout, k, s, p, d, has_bias = case
    r16 = lambda t: t.bfloat16().float()
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    xr, wr = r16(x).requires_grad_(True), r16(wt).requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=s, padding=p, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    K.set_conv_precision(form.split('+')[0])
    K.set_bf16_wgrad(form.endswith('+wgrad'))       # weight gradient on pixel-contiguous bf16 copies (off by default)
    try:
        xg, wg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda()
        y = K.conv_fwd(xg, wg, s, p, d)
        assert rel(nchw(y), y_ref.detach()) < 1e-4
        dyg = K.new(tuple(y.shape), y, pitch_pad=True)
        dyg.copy_(nhwc(dy))
        dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s, p, d)
        dw, _ = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s, p, d)
    finally:
        K.set_conv_precision('f32')
        K.set_bf16_wgrad(False)
    # backward oracles: dgrad rounds (dy, w); wgrad rounds (x, dy)
    F.conv2d(x.clone().requires_grad_(True), wr, None, stride=s, padding=p, dilation=d)
    x2 = x.clone().requires_grad_(True)
    F.conv2d(x2, r16(wt), None, stride=s, padding=p, dilation=d).backward(r16(dy))
    assert rel(nchw(dx), x2.grad) < 1e-4
    w2 = wt.clone().requires_grad_(True)
    F.conv2d(r16(x), w2, None, stride=s, padding=p, dilation=d).backward(r16(dy))
    assert rel(dw.permute(0, 3, 1, 2), w2.grad) < 2e-4


# ---- BASELINE configs[2], round 4: bf16 ACTIVATIONS (pm_tensor.dtype == PM_BF16) ------------------------------------------------------------------
def b16(t):
    """logical NCHW fp32 (CPU) -> NHWC bf16 on the GPU"""
    return t.permute(0, 2, 3, 1).contiguous().cuda().bfloat16()


def close16(got, want, ulps=1.0):
    """bf16 result vs an fp32 reference of the same formula on the same (bf16) inputs: equal up to `ulps` bf16 roundings of the reference (2^-8 relative:
    the reference may sit on a rounding boundary), plus the same slack relative to the tensor's scale for values that cancel to ~0."""
    g, w = got.float().cpu().double(), want.float().cpu().double()
    tol = ulps * 2.0 ** -8 * w.abs() + ulps * 2.0 ** -9 * w.abs().max() * 1e-2 + 1e-30
    bad = (g - w).abs() > tol
    assert not bad.any(), 'max |err| %.3e at ref %.3e (scale %.3e), %d of %d off' % ((g - w).abs().max().item(), w[bad][0].item(), w.abs().max().item(), int(bad.sum()), bad.numel())


@pytest.mark.parametrize('shape', [(2, 64, 24, 20), (3, 48, 9, 11), (2, 256, 12, 12), (1, 1280, 6, 6), (2, 128, 1, 1)])
def test_act16_batchnorm(K, shape):
    """csrc/act16.hip: train-mode BatchNorm forward / backward on bf16 activations (fp32 statistics) against the fp32 formulas evaluated on the same bf16
    values: statistics to fp32 round-off, bf16 outputs to one rounding; ReLU masks from the forward output, rebuilt from x, and from the mask bytes."""
    n, c, h, w = shape
    x = (rnd(n, c, h, w, seed=1) * 2 + 0.5).bfloat16().float()
    res = rnd(n, c, h, w, seed=2).bfloat16().float()
    dy = rnd(n, c, h, w, seed=3).bfloat16().float()
    gamma, beta = rnd(c, seed=4) * 0.2 + 1.0, rnd(c, seed=5) * 0.1
    x16, res16, dy16 = b16(x), b16(res), b16(dy)
    rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    mean, invstd = K.bn_stats_finalize(x16, 1e-5, rm, rv, 0.1)
    xd = x.double()
    m_ref, v_ref = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    assert rel(mean, m_ref) < 1e-6 and rel(invstd, 1.0 / torch.sqrt(v_ref + 1e-5)) < 1e-5
    assert rel(rm, 0.1 * m_ref) < 1e-5
    mom = K.bn_stats(x16)
    assert rel(mom[:c], m_ref) < 1e-6 and rel(mom[c:2 * c], v_ref * (n * h * w)) < 1e-5 and (mom[2 * c:] == n * h * w).all()
    mu, isd = mean.cpu(), invstd.cpu()
    bc = lambda t: t[None, :, None, None]
    aff = (x - bc(mu)) * bc(isd) * bc(gamma) + bc(beta)
    # forward: plain, ReLU, residual + ReLU (+ mask bytes)
    o0 = K.bn_apply(x16, mean, invstd, gamma.cuda(), beta.cuda())
    close16(nchw(o0.float()), aff)
    o2 = K.bn_apply(x16, mean, invstd, gamma.cuda(), beta.cuda(), relu=True)
    close16(nchw(o2.float()), aff.clamp_min(0))
    o1, mask = K.bn_apply(x16, mean, invstd, gamma.cuda(), beta.cuda(), residual=res16, relu=True, want_mask=True)
    pre = aff + res
    close16(nchw(o1.float()), pre.clamp_min(0))
    assert tuple(mask.shape) == (n * h * w, c // 8)
    # backward reduce: the three mask sources agree with the fp32 formula wherever the pre-activation is not within rounding of zero
    xhat = (x - bc(mu)) * bc(isd)
    for mode, fwd_out, m in ((0, None, None), (2, None, None), (1, o1, None), (3, None, mask)):
        if mode == 3:
            sums, gm = K.bn_bwd_reduce_mask(dy16, m, x16, mean, invstd, want_gmask=True)
            keep = pre > 0
        else:
            sums, gm = K.bn_bwd_reduce(dy16, fwd_out, x16, mean, invstd, mode, gamma.cuda(), beta.cuda(), want_gmask=mode != 0)
            keep = torch.ones_like(dy, dtype=torch.bool) if mode == 0 else (aff > 0 if mode == 2 else nchw(o1.float()) > 0)
        g = dy * keep
        ref_s = torch.cat([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))])
        edge = (aff.abs() < 1e-2) | (pre.abs() < 1e-2)                       # units whose sign the two evaluations may see differently
        slack = (dy.abs() * edge).sum((0, 2, 3))
        slack = torch.cat([slack, slack * xhat.abs().amax((0, 2, 3))]) + 1e-4 * ref_s.abs().max()
        assert ((sums.cpu() - ref_s).abs() <= slack + 1e-5 * ref_s.abs()).all(), mode
        if gm is not None:
            ok = ~edge
            assert torch.equal(nchw(gm.float())[ok], g[ok]), mode
    # backward apply (relu 0, the masked gradient as input): dx = gamma invstd (g - s1 / n - xhat s2 / n)
    sums, _ = K.bn_bwd_reduce(dy16, None, x16, mean, invstd, 0)
    cnt = float(n * h * w)
    dx, _ = K.bn_bwd_apply(dy16, None, x16, mean, invstd, gamma.cuda(), sums, cnt, 0, False)
    s1, s2 = sums[:c].cpu(), sums[c:].cpu()
    ref_dx = (dy - bc(s1) / cnt - xhat * bc(s2) / cnt) * bc(isd * gamma)
    close16(nchw(dx.float()), ref_dx, ulps=2.0)
    dx2, dres = K.bn_bwd_apply(dy16, o1, x16, mean, invstd, gamma.cuda(), sums, cnt, 1, True)
    assert dres.dtype == torch.bfloat16 and torch.equal(nchw(dres.float()), dy * (nchw(o1.float()) > 0))


def test_act16_pool_resize_add_cast(K):
    """csrc/act16.hip against the fp32 kernels of the library (themselves tested against torch above) on the widened inputs: identical arithmetic, so
    the bf16 outputs are the fp32 results rounded once."""
    x = rnd(2, 64, 23, 19, seed=1).bfloat16().float()
    x16, x32 = b16(x), nhwc(x)
    assert torch.equal(K.cast(x16, torch.float32), x32) and torch.equal(K.cast(x32, torch.bfloat16), x16)
    odd = nhwc(rnd(2, 19, 5, 7, seed=9))
    assert torch.equal(K.cast(odd, torch.bfloat16).float(), odd.bfloat16().float())
    # max pool
    y16, a16 = K.maxpool_fwd(x16)
    y32, a32 = K.maxpool_fwd(x32)
    assert torch.equal(y16.float(), y32) and torch.equal(a16, a32)
    dy = rnd(*nchw(y32).shape, seed=2).bfloat16().float()
    close16(K.maxpool_bwd(b16(dy), a16, tuple(x16.shape)).float(), K.maxpool_bwd(nhwc(dy), a32, tuple(x32.shape)))
    # global average pool (+ backward), 1x1-source resize backward (a column sum)
    close16(K.global_avgpool_fwd(x16).float(), K.global_avgpool_fwd(x32))
    g = rnd(2, 64, 1, 1, seed=3).bfloat16().float()
    close16(K.global_avgpool_bwd(b16(g), tuple(x16.shape)).float(), K.global_avgpool_bwd(nhwc(g), tuple(x32.shape)))
    close16(K.resize_bwd(x16, (2, 1, 1, 64)).float(), K.resize_bwd(x32, (2, 1, 1, 64)), ulps=2.0)
    # bilinear resize forward, backward (gather and separable), into a channel slice of a wider buffer
    up16, up32 = K.resize_fwd(x16, (47, 41)), K.resize_fwd(x32, (47, 41))
    close16(up16.float(), up32)
    buf = torch.zeros(2, 47, 41, 128, device='cuda', dtype=torch.bfloat16)
    K.resize_fwd(x16, (47, 41), out=buf[..., 64:])
    assert torch.equal(buf[..., 64:], up16) and buf[..., :64].abs().max().item() == 0
    du = rnd(2, 64, 47, 41, seed=4).bfloat16().float()
    for sep in (False, True):
        close16(K.resize_bwd(b16(du), tuple(x16.shape), separable=sep).float(), K.resize_bwd(nhwc(du), tuple(x32.shape), separable=sep), ulps=2.0)
    # n-ary add, copy
    ts = [rnd(2, 64, 23, 19, seed=10 + i).bfloat16().float() for i in range(5)]
    close16(K.add_n([b16(t) for t in ts]).float(), K.add_n([nhwc(t) for t in ts]))
    close16(K.add(b16(ts[0]), b16(ts[1])).float(), K.add(nhwc(ts[0]), nhwc(ts[1])))
    dst = torch.zeros(2, 23, 19, 128, device='cuda', dtype=torch.bfloat16)
    K.copy(x16, dst[..., 32:96])
    assert torch.equal(dst[..., 32:96], x16) and dst[..., :32].abs().max().item() == 0


ACT16_CASES = [CONV_CASES[0], CONV_CASES[1], CONV_CASES[3], CONV_CASES[4], CONV_CASES[5], CONV_CASES[10], CONV_CASES[11], CONV_CASES[12],
               (2, 256, 24, 24, 128, 3, 1, 6, 6, False),        # dilated 3x3
               (1, 1280, 16, 16, 256, 1, 1, 0, 1, False),       # bot_aspp: long K
               (2, 256, 20, 20, 48, 1, 1, 0, 1, False),         # bot_fine: 48 output channels (weight-gradient rows beyond Cout, dgrad of a 48-channel dy)
               (1, 1024, 12, 12, 512, 3, 1, 1, 1, True),        # dsn.0: bias + bias gradient over a bf16 dy
               (1, 512, 12, 12, 512, 3, 1, 2, 2, False)]


@pytest.mark.parametrize('route', ['lds_dma', 'lds_dma_wide', 'lds_dma_ring', 'lds_dma_256', 'reg_staged'])
@pytest.mark.parametrize('case', ACT16_CASES)
def test_conv_bf16_activations(K, case, route):
    """BASELINE configs[2], round 4: bf16 tensors in, bf16 tensors out (x, y, dy, dx), fp32 weights / dw, fp32 accumulation. Oracle: the fp32 convolution of
    the bf16-rounded operands; outputs agree to one bf16 rounding, dw to fp32 accumulation order."""
    n, cin, h, w, cout, k, s, p, d, has_bias = case
    r16 = lambda t: t.bfloat16().float()
    x, wt = r16(rnd(n, cin, h, w, seed=1)), rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    b = rnd(cout, seed=3) if has_bias else None
    y_ref = F.conv2d(x, r16(wt), b, stride=s, padding=p, dilation=d)
    dy = r16(rnd(*y_ref.shape, seed=4))
    skip = r16(rnd(n, cin, h, w, seed=5))
    K.set_conv_precision('bf16')
    # csrc/conv16.hip on every shape (2: its narrow tiles; conv16w.hip: 3 the persistent producer / consumer ring, 8 the ring with one block per tile, 7 the 256 x 256
    # two-stage form), or the register-staged kernel on bf16 rows
    K.set_conv16({'lds_dma': 2, 'lds_dma_wide': 3, 'lds_dma_ring': 8, 'lds_dma_256': 7}.get(route, 0))
    try:
        wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
        xg = K.new((n, h, w, cin), wg, dtype=torch.bfloat16)      # zero-padded + registered when cin % 64 != 0 (304): gathered in place
        xg.copy_(b16(x))
        y = K.conv_fwd(xg, wg, s, p, d, bias=b.cuda() if has_bias else None)
        assert y.dtype == torch.bfloat16
        close16(nchw(y.float()), y_ref, ulps=1.5)
        dyg = K.new(tuple(y.shape), y)
        dyg.copy_(b16(dy))
        dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s, p, d, add=b16(skip))
        dw, db = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s, p, d, want_bias=has_bias)
        # the same through tensors WITHOUT the zero-pad promise (dense 48 / 304-channel rows: copied to a padded buffer by the library)
        if cin % 64 or cout % 64:
            y2 = K.conv_fwd(b16(x), wg, s, p, d, bias=b.cuda() if has_bias else None)
            dx2 = K.conv_bwd_data(b16(dy), wg, tuple(xg.shape), s, p, d, add=b16(skip))
            assert torch.equal(y2, y) and torch.equal(dx2, dx)
    finally:
        K.set_conv_precision('f32')
        K.set_conv16(True)
    x2 = x.clone().requires_grad_(True)
    F.conv2d(x2, r16(wt), None, stride=s, padding=p, dilation=d).backward(dy)
    assert dx.dtype == torch.bfloat16
    close16(nchw(dx.float()), x2.grad + skip, ulps=1.5)
    w2 = wt.clone().requires_grad_(True)
    b2 = b.clone().requires_grad_(True) if has_bias else None
    F.conv2d(x, w2, b2, stride=s, padding=p, dilation=d).backward(dy)
    assert dw.dtype == torch.float32 and rel(dw.permute(0, 3, 1, 2), w2.grad) < 2e-4
    if has_bias:
        assert rel(db, b2.grad) < 2e-5


@pytest.mark.parametrize('case', [(8, 512, 48, 48, 256, 3, 6, 6), (8, 1024, 48, 48, 512, 1, 0, 1), (8, 256, 47, 49, 256, 3, 1, 1), (5, 512, 48, 48, 19, 1, 0, 1),
                                  (3, 128, 48, 48, 256, 3, 18, 18), (2, 192, 48, 40, 128, 3, 12, 12),      # ASPP rates 18 / 12: whole filter rows invisible to the top / bottom tiles (skipped K-steps)
                                  (1, 256, 192, 192, 256, 3, 1, 1)])      # the decoder's 3x3 at its real map size (36 864 rows: 144 tiles of the persistent ring) against the CPU formula
def test_conv16_on_the_48x48_maps(K, case):
    """The LDS-DMA kernel at the shapes it carries in the step (bs=8: 18 432 rows, 576 ... 1 152 tiles of 64 x 128 on 256 CUs, a ragged last tile, the 19-column
    fp32 logits): forward with bias / folded scale-shift / residual / ReLU and the data gradient with its fused skip, each against the fp32 formula on the same
    bf16 values and against the register-staged kernel. (Written for the hybrid K-split of the last partial round of tiles and the 3 / 4-stage LDS ring with
    counted vmcnt waits, both measured and dropped -- DESIGN section 7; kept as the full-size check of the kernel.)"""
    n, cin, h, w, cout, k, p, d = case
    r16 = lambda t: t.bfloat16().float()
    x, wt = r16(rnd(n, cin, h, w, seed=1)), rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    logits = cout == 19
    b = rnd(cout, seed=3)
    sc, sh = rnd(cout, seed=6).abs() + 0.5, rnd(cout, seed=7)
    res = r16(rnd(n, cout, h, w, seed=8))
    y_lin = F.conv2d(x, r16(wt), None, padding=p, dilation=d)
    dy, skip = r16(rnd(*y_lin.shape, seed=4)), r16(rnd(n, cin, h, w, seed=5))
    K.set_conv_precision('bf16')
    outs = {}
    try:
        wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
        for route in (2, 3, 8, 7, 0):      # narrow LDS-DMA tiles; conv16w.hip: persistent ring, ring with one block per tile, 256 x 256 two-stage form; the register-staged kernel
            K.set_conv16(route)
            if logits:
                y = K.conv_fwd(b16(x), wg, 1, p, d, bias=b.cuda(), out_dtype=torch.float32)
                outs[route] = (y,)
                continue
            y0 = K.conv_fwd(b16(x), wg, 1, p, d, bias=b.cuda())
            y1 = K.conv_fwd(b16(x), wg, 1, p, d, scale=sc.cuda(), shift=sh.cuda(), residual=b16(res), relu=True)
            dx = K.conv_bwd_data(b16(dy), wg, (n, h, w, cin), 1, p, d, add=b16(skip))
            outs[route] = (y0, y1, dx)
    finally:
        K.set_conv16(1)
        K.set_conv_precision('f32')
    if logits:
        assert outs[2][0].dtype == torch.float32
        assert rel(nchw(outs[2][0]), y_lin + b.view(1, -1, 1, 1)) < 2e-5 and rel(outs[2][0], outs[0][0]) < 2e-5
        for r in (3, 8, 7):
            assert rel(nchw(outs[r][0]), y_lin + b.view(1, -1, 1, 1)) < 2e-5, r
        return
    y0, y1, dx = outs[2]
    close16(nchw(y0.float()), y_lin + b.view(1, -1, 1, 1), ulps=1.5)
    close16(nchw(y1.float()), torch.relu(y_lin * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + res), ulps=1.5)
    x2 = x.clone().requires_grad_(True)
    F.conv2d(x2, r16(wt), None, padding=p, dilation=d).backward(dy)
    close16(nchw(dx.float()), x2.grad + skip, ulps=1.5)
    for a, c in zip(outs[2], outs[0]):      # the two kernels differ by accumulation order only: neighbouring bf16 values at most (one spacing = 2^-7)
        close16(a.float(), c.float(), ulps=2.5)
    y0w, y1w, dxw = outs[3]                 # the wide kernel: against the formula and against the narrow kernel
    close16(nchw(y0w.float()), y_lin + b.view(1, -1, 1, 1), ulps=1.5)
    close16(nchw(y1w.float()), torch.relu(y_lin * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + res), ulps=1.5)
    close16(nchw(dxw.float()), x2.grad + skip, ulps=1.5)
    for a, c in zip(outs[3], outs[2]):
        close16(a.float(), c.float(), ulps=2.5)
    for a, c in zip(outs[7], outs[2]):      # the 256 x 256 form: same sums in another order
        close16(a.float(), c.float(), ulps=2.5)
    for a, c in zip(outs[8], outs[3]):      # the ring with one block per tile against its persistent form: same tiles, same K order, same epilogue arithmetic
        assert torch.equal(a, c)


WGRAD16_CASES = [  # n, cin, h, w, cout, k, stride, pad, dil
    (2, 256, 48, 48, 256, 3, 1, 1, 1),       # layer3-like: 4608 pixels, 18 tiles x split
    (1, 512, 24, 20, 512, 3, 1, 2, 2),       # dilated, 480 pixels: a partial last 64-pixel step
    (2, 128, 33, 31, 128, 3, 1, 1, 1),       # Cout = 128: the 128 x 256 tile is not taken (Cin % 256), rows beyond Cout of the 256-row tile are masked; odd sizes
    (1, 256, 40, 40, 384, 1, 1, 0, 1),       # 1x1; Cout = 384 -> three 128-row tiles of the 128 x 256 form
    (2, 256, 31, 29, 256, 3, 2, 1, 1),       # stride 2 (the first 3x3 of a stage)
    (1, 1024, 12, 12, 2048, 1, 1, 0, 1),     # wide 1x1, 144 pixels: three K-steps, most units a single split
    (3, 128, 17, 19, 256, 3, 1, 12, 12),     # dilation beyond the map: most taps see only padding
    (1, 304, 40, 36, 256, 3, 1, 1, 1),       # the decoder's concat: 2.5 channel blocks, the last one half empty (zeros fetched, columns beyond Cin not stored)
    (1, 200, 20, 20, 128, 1, 1, 0, 1),       # 1.56 blocks
    (2, 256, 96, 96, 256, 3, 1, 1, 1),       # 18 432 pixels -- a reduction as long per split as the step's (the 48 x 48 maps at bs=8), against the CPU formula
]


@pytest.mark.parametrize('case', WGRAD16_CASES)
def test_wgrad16_lds_dma_weight_gradient(K, case):
    """csrc/wgrad16.hip (round 5): the bf16 tier's weight gradient on the LDS-DMA persistent ring against the fp32 formula on the same bf16 values and against the
    register-staged kernel (pm_set_wgrad16(0)); repeated launches are bit-identical (fixed-order split-K reduce)."""
    n, cin, h, w, cout, k, s_, p, d = case
    r16 = lambda t: t.bfloat16().float()
    x = r16(rnd(n, cin, h, w, seed=1))
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    y_ref = F.conv2d(x, wt, None, stride=s_, padding=p, dilation=d)
    dy = r16(rnd(*y_ref.shape, seed=4))
    w2 = wt.clone().requires_grad_(True)
    F.conv2d(x, w2, None, stride=s_, padding=p, dilation=d).backward(dy)
    K.set_conv_precision('bf16')
    outs = {}
    try:
        for on in (True, False):
            K.set_wgrad16(on)
            K.profile_enable(True)
            K.profile_read(clear=True)
            dw, _ = K.conv_bwd_weight(b16(x), b16(dy), (cout, k, k, cin), s_, p, d)
            dw2, _ = K.conv_bwd_weight(b16(x), b16(dy), (cout, k, k, cin), s_, p, d)
            taken = any(K.profile_read(mode=2, bm=bm, bn=bn, km=2, nst=3, prec=4)[2] for bm, bn in ((256, 128), (128, 256)))
            K.profile_enable(False)
            assert taken == on, 'the LDS-DMA kernel must (not) take this shape'
            assert torch.equal(dw, dw2)
            outs[on] = dw
    finally:
        K.set_wgrad16(True)
        K.profile_enable(False)
        K.set_conv_precision('f32')
    assert outs[True].dtype == torch.float32
    assert rel(outs[True].permute(0, 3, 1, 2), w2.grad) < 2e-4
    assert rel(outs[True], outs[False]) < 2e-5


@pytest.mark.parametrize('case', [(8, 256, 192, 192, 256, 3, 1, 1),        # decoder final1.3: the persistent ring by the planner's rule (M = 294 912)
                                  (8, 320, 192, 192, 256, 3, 1, 1),        # decoder final1.0 (304 + 16 zero-pad channels as the concat buffer has them)
                                  (8, 2048, 48, 48, 256, 3, 12, 12)])      # ASPP rate 12: 288 K-steps, filter rows skipped per tile
def test_persistent_kernels_at_production_size_under_default_routing(K, case):
    """ROUTING + AGREEMENT OF TWO HIP KERNELS, NOT AN ORACLE COMPARISON (the formula checks are test_conv16_on_the_48x48_maps -- incl. 1 x 256 x 192 x 192 -- and
    test_wgrad16_lds_dma_weight_gradient -- incl. an 18 432-pixel reduction). BASELINE configs[2] sizes (bs=8, 768^2): the shapes the planner hands to the persistent
    producer / consumer kernels (conv16w.hip conv16p_kernel, wgrad16.hip) under
    DEFAULT routing really take them, and agree with the register-staged kernels on the same bf16 values: forward and input gradient to neighbouring bf16 values, the
    weight gradient to fp32 accumulation order. (The fp32 formula on the CPU would take minutes at this size: the independent kernel is the reference here, each of the
    two is checked against the formula on small shapes above.)"""
    n, cin, h, w, cout, k, p, d = case
    g = torch.Generator(device='cuda').manual_seed(11)
    x = torch.randn(n, h, w, cin, device='cuda', generator=g).bfloat16()
    dy = torch.randn(n, h, w, cout, device='cuda', generator=g).bfloat16()
    wt = torch.randn(cout, k, k, cin, device='cuda', generator=g) * (2.0 / (cin * k * k)) ** 0.5
    K.set_conv_precision('bf16')
    outs = {}
    try:
        for route in (1, 0):
            K.set_conv16(route)
            K.set_wgrad16(route == 1)
            K.profile_enable(True)
            K.profile_read(clear=True)
            y = K.conv_fwd(x, wt, 1, p, d)
            dx = K.conv_bwd_data(dy, wt, (n, h, w, cin), 1, p, d)
            dw, _ = K.conv_bwd_weight(x, dy, (cout, k, k, cin), 1, p, d)
            ring = sum(K.profile_read(mode=5, bm=bm, bn=bn, km=1, nst=3, prec=5)[2] for bm, bn in ((256, 128), (128, 256)))
            wg = sum(K.profile_read(mode=2, bm=bm, bn=bn, km=2, nst=3, prec=4)[2] for bm, bn in ((256, 128), (128, 256)))
            K.profile_enable(False)
            if route == 1:
                assert ring >= 1 and wg == 1, ('default routing must take the persistent kernels on this shape', ring, wg)
            else:
                assert ring == 0 and wg == 0
            outs[route] = (y, dx, dw)
    finally:
        K.profile_enable(False)
        K.set_conv16(1)
        K.set_wgrad16(True)
        K.set_conv_precision('f32')
    close16(outs[1][0].float(), outs[0][0].float(), ulps=2.5)
    close16(outs[1][1].float(), outs[0][1].float(), ulps=2.5)
    assert rel(outs[1][2], outs[0][2]) < 2e-5


def test_bf16_filter_refresh_after_optimizer_step(K):
    """bf16 tier: optim.SGD.step() rewrites the kept bf16 filters (forward copy and the rotated copy of the data gradient) of the weights it moved in one batched
    launch (pm_conv_wxf_refresh_bf16). The next convolutions must find them valid and compute exactly what a freshly derived filter gives -- for a 3x3, a 1x1,
    and channel counts that need padding to 64 on either side."""
    from pinthememory_amd import optim
    K.set_conv_precision('bf16')
    was = K.KEEP_WINOGRAD_U
    K.KEEP_WINOGRAD_U = None
    K.clear_filters()
    K.unregister_filter_owners()
    try:
        cases = [(128, 64, 3, 1, 1), (96, 160, 1, 0, 1), (64, 256, 3, 2, 2)]        # (cout, cin, k, pad, dil)
        ws, xs = [], []
        for i, (co, ci, k, pad, dil) in enumerate(cases):
            ws.append(torch.nn.Parameter(rnd(co, ci, k, k, seed=10 + i).mul(0.05).cuda().contiguous(memory_format=torch.channels_last)))
            xs.append(K.cast(nhwc(rnd(2, ci, 20, 24, seed=20 + i)), torch.bfloat16))
        opt = optim.SGD(ws, lr=0.1, momentum=0.9, weight_decay=0.0)

        def run():
            out = []
            for w, x, (co, ci, k, pad, dil) in zip(ws, xs, cases):
                wk = w.detach().permute(0, 2, 3, 1)
                y = K.conv_fwd(x, wk, 1, pad, dil)
                dx = K.conv_bwd_data(y, wk, x.shape, 1, pad, dil)
                out += [y, dx]
            return out
        first = run()
        assert len(K._U_CACHE) == 2 * len(cases)
        for w in ws:
            w.grad = torch.full_like(w, 0.01)
        K.filter_transform_count(True)
        n0 = K.filter_transform_count()
        opt.step()                                                   # moves the weights, bumps the versions, refreshes the six kept filters
        assert all(e.version == w._version for e in K._U_CACHE.values() for w in ws if (e.owner() is w))
        second = run()
        assert K.filter_transform_count() == n0                      # no forward call derived a filter again
        K.filter_transform_count(False)
        assert not any(torch.equal(a, b) for a, b in zip(first, second))
        K.KEEP_WINOGRAD_U = False                                    # the same calls with filters derived on the spot
        fresh = run()
        for a, b in zip(second, fresh):
            assert torch.equal(a, b)
        K.KEEP_WINOGRAD_U = None
        assert K.refresh_filters() == 0                              # nothing out of date: no launch
    finally:
        K.filter_transform_count(False)
        K.KEEP_WINOGRAD_U = was
        K.unregister_filter_owners()
        K.clear_filters()
        K.set_conv_precision('f32')


def test_f32_winograd_filter_refresh_after_optimizer_step(K):
    """fp32 tier: optim.SGD.step() rewrites the kept Winograd forward transforms U = G g Gt of the weights it moved in ONE batched launch (pm_conv_wxf_refresh_f32).
    The next forward convolutions must find them valid (no per-layer transform) and compute exactly what a freshly derived transform gives -- wide 3x3 layers on the
    Winograd route at dilation 1 and 2, channel counts that pad K to 32; a layer off the route (1x1) keeps nothing and is unaffected."""
    from pinthememory_amd import optim
    K.set_conv_precision('f32')
    was = K.KEEP_WINOGRAD_U
    K.KEEP_WINOGRAD_U = None
    K.clear_filters()
    K.unregister_filter_owners()
    try:
        cases = [(128, 128, 3, 1, 1, 48), (256, 144, 3, 2, 2, 48), (128, 256, 3, 1, 1, 24), (64, 128, 1, 0, 1, 24)]        # (cout, cin, k, pad, dil, map)
        ws, xs = [], []
        for i, (co, ci, k, pad, dil, hw) in enumerate(cases):
            ws.append(torch.nn.Parameter(rnd(co, ci, k, k, seed=30 + i).mul(0.05).cuda().contiguous(memory_format=torch.channels_last)))
            xs.append(nhwc(rnd(2, ci, hw, hw, seed=40 + i)))
        opt = optim.SGD(ws, lr=0.1, momentum=0.9, weight_decay=0.0)

        def run():
            return [K.conv_fwd(x, w.detach().permute(0, 2, 3, 1), 1, pad, dil) for w, x, (co, ci, k, pad, dil, hw) in zip(ws, xs, cases)]
        first = run()
        kept = len(K._U_CACHE)
        assert kept >= 2                                             # the wide 3x3 layers took the Winograd route and kept their transform
        for w in ws:
            w.grad = torch.full_like(w, 0.01)
        K.filter_transform_count(True)
        n0 = K.filter_transform_count()
        opt.step()                                                   # moves the weights, bumps the versions, refreshes the kept transforms in one launch
        assert all(e.version == w._version for e in K._U_CACHE.values() for w in ws if (e.owner() is w))
        second = run()
        assert K.filter_transform_count() == n0                      # no forward call transformed its filter again
        K.filter_transform_count(False)
        assert not any(torch.equal(a, b) for a, b in zip(first, second))
        K.KEEP_WINOGRAD_U = False                                    # the same calls with transforms derived on the spot
        for a, b in zip(second, run()):
            assert torch.equal(a, b)
        K.KEEP_WINOGRAD_U = None
        assert K.refresh_filters() == 0                              # nothing out of date: no launch
    finally:
        K.filter_transform_count(False)
        K.KEEP_WINOGRAD_U = was
        K.unregister_filter_owners()
        K.clear_filters()


def test_conv_bf16_tier_mixed_edges(K):
    """The mixed-type call sites of the tier: the stem (fp32 NHWC4 image -> bf16, weight gradient from a bf16 dy), a 19-class head (bf16 -> fp32 logits with
    bias, fp32 dy -> bf16 dx, weight / bias gradient), a stride-2 3x3 and a stride-2 1x1 data gradient (bf16 dy -> bf16 dx + bf16 skip)."""
    r16 = lambda t: t.bfloat16().float()
    K.set_conv_precision('bf16')
    try:
        # stem
        x, wt = rnd(2, 4, 40, 36, seed=1), rnd(64, 4, 7, 7, seed=2, scale=0.1)
        x[:, 3] = 0
        wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
        y = K.conv_fwd(nhwc(x), wg, 2, 3, 1)
        y_ref = F.conv2d(r16(x), r16(wt), None, stride=2, padding=3)
        assert y.dtype == torch.bfloat16
        close16(nchw(y.float()), y_ref, ulps=1.5)
        dy = r16(rnd(*y_ref.shape, seed=3))
        dw, _ = K.conv_bwd_weight(nhwc(x), b16(dy), tuple(wg.shape), 2, 3, 1)
        w2 = wt.clone().requires_grad_(True)
        F.conv2d(r16(x), w2, None, stride=2, padding=3).backward(dy)
        assert rel(dw.permute(0, 3, 1, 2), w2.grad) < 2e-4
        # class head
        x, wt, b = r16(rnd(2, 256, 16, 16, seed=4)), rnd(19, 256, 1, 1, seed=5, scale=0.06), rnd(19, seed=6)
        wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
        y = K.conv_fwd(b16(x), wg, 1, 0, 1, bias=b.cuda(), out_dtype=torch.float32)
        assert y.dtype == torch.float32 and rel(nchw(y), F.conv2d(x, r16(wt), b)) < 1e-4
        dy = rnd(2, 19, 16, 16, seed=7)
        dyg = K.new(tuple(y.shape), y, pitch_pad=True)
        dyg.copy_(nhwc(dy))
        dx = K.conv_bwd_data(dyg, wg, (2, 16, 16, 256), 1, 0, 1, dtype=torch.bfloat16)
        x2 = x.clone().requires_grad_(True)
        F.conv2d(x2, r16(wt), None).backward(r16(dy))
        assert dx.dtype == torch.bfloat16
        close16(nchw(dx.float()), x2.grad, ulps=1.5)
        dw, db = K.conv_bwd_weight(b16(x), dyg, tuple(wg.shape), 1, 0, 1, want_bias=True)
        w2, b2 = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        F.conv2d(x, w2, b2).backward(r16(dy))
        assert rel(dw.permute(0, 3, 1, 2), w2.grad) < 2e-4 and rel(db, dy.sum((0, 2, 3))) < 2e-5
        # stride-2 data gradients
        # (round 4: each parity class is a forward convolution of the bf16 dy with its sub-filter, on the LDS-DMA kernel; odd map sizes leave the classes unequal;
        #  a 96-channel dy -- not a multiple of 64 -- takes the older fp32-row form)
        for cin, cout, k, p, hh, ww in ((128, 128, 3, 1, 24, 24), (256, 512, 1, 0, 24, 24), (128, 128, 3, 1, 25, 23), (64, 192, 1, 0, 17, 31), (64, 96, 3, 1, 20, 18)):
            wt = rnd(cout, cin, k, k, seed=8, scale=(2.0 / (cin * k * k)) ** 0.5)
            wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
            x2 = torch.zeros(2, cin, hh, ww, requires_grad=True)
            yr = F.conv2d(x2, r16(wt), None, stride=2, padding=p)
            dy, skip = r16(rnd(*yr.shape, seed=9)), r16(rnd(2, cin, hh, ww, seed=10))
            yr.backward(dy)
            dx = K.conv_bwd_data(b16(dy), wg, (2, hh, ww, cin), 2, p, 1, add=b16(skip))
            assert dx.dtype == torch.bfloat16
            close16(nchw(dx.float()), x2.grad + skip, ulps=1.5)
            dx0 = K.conv_bwd_data(b16(dy), wg, (2, hh, ww, cin), 2, p, 1)      # without the fused skip gradient
            close16(nchw(dx0.float()), x2.grad, ulps=1.5)
    finally:
        K.set_conv_precision('f32')


def test_input_edge_u8(K):
    """GPU-side ToTensor + Normalize + MaskToTensor vs the torch formulas of the reference's loader."""
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (2, 37, 29, 3), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 256, (2, 37, 29), generator=g, dtype=torch.uint8)
    out = K.image_u8_to_nhwc4(img.cuda()).cpu()
    mean, std = torch.tensor(K.IMAGENET_MEAN), torch.tensor(K.IMAGENET_STD)
    ref = (img.float() / 255.0 - mean) / std
    assert (out[..., :3] - ref).abs().max().item() < 1e-6 and out[..., 3].abs().max().item() == 0
    assert torch.equal(K.labels_u8_to_i64(lab.cuda()).cpu(), lab.long())


def test_c_abi_error_conventions(K):
    """the library never throws or exits across the boundary -- bad calls return a negative pm_status and leave a message in
    pm_last_error(); nothing is launched, the next good call works. Called through the raw ctypes table (hip/lib.py), as a foreign host would."""
    from ctypes import byref
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    st = L.stream()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
    x, y = nhwc(rnd(1, 64, 8, 8, seed=1)), torch.empty(1, 8, 8, 64, device='cuda')
    w = rnd(64, 3, 3, 64, seed=2).cuda()
    xd, yd = L.tdesc(x), L.tdesc(y)
    p = L.conv_params(3, 3, 1, 1, 1, 0)
    need = lib.pm_conv_workspace(byref(xd), byref(yd), byref(p), 0)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    assert lib.pm_conv_fwd(byref(xd), None, byref(yd), byref(p), None, ws.data_ptr(), need, st) == EINVAL          # no weight
    assert b'weight' in lib.pm_last_error()
    y7 = L.tdesc(torch.empty(1, 7, 7, 64, device='cuda'))
    assert lib.pm_conv_fwd(byref(xd), w.data_ptr(), byref(y7), byref(p), None, ws.data_ptr(), need, st) == EINVAL  # output extent does not follow from the geometry
    # a large split-K / Winograd problem with no workspace
    xl, yl = nhwc(rnd(1, 128, 24, 24, seed=3)), torch.empty(1, 24, 24, 128, device='cuda')
    wl = rnd(128, 3, 3, 128, seed=4).cuda()
    xld, yld = L.tdesc(xl), L.tdesc(yl)
    assert lib.pm_conv_workspace(byref(xld), byref(yld), byref(p), 0) > 0
    assert lib.pm_conv_fwd(byref(xld), wl.data_ptr(), byref(yld), byref(p), None, None, 0, st) == EWORKSPACE
    assert b'workspace' in lib.pm_last_error()
    # memory read: too many slots / a feature width the kernels are not built for
    q, mem40 = nhwc(rnd(1, 256, 4, 4, seed=5)), rnd(40, 256, seed=6).cuda()
    qr = torch.empty(1, 4, 4, 512, device='cuda')
    sc = torch.empty(16, 40, device='cuda')
    assert lib.pm_mem_read_fwd(byref(L.tdesc(q)), mem40.data_ptr(), 40, None, byref(L.tdesc(qr)), sc.data_ptr(), sc.data_ptr(), st) == EINVAL
    q128 = nhwc(rnd(1, 128, 4, 4, seed=7))
    assert lib.pm_mem_read_fwd(byref(L.tdesc(q128)), mem40.data_ptr(), 19, None, byref(L.tdesc(qr)), sc.data_ptr(), sc.data_ptr(), st) == EUNSUPPORTED
    # BatchNorm statistics of a single value per channel (torch raises in train mode too); 64 classes for the fused CE (built for <= 32)
    one = L.tdesc(torch.zeros(1, 1, 1, 64, device='cuda'))
    m = torch.zeros(64, device='cuda')
    wsb = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    assert lib.pm_bn_stats_finalize(byref(one), 1e-5, m.data_ptr(), m.data_ptr(), None, None, 0.1, wsb.data_ptr(), 1 << 16, st) == EINVAL
    lg = L.tdesc(torch.zeros(1, 4, 4, 64, device='cuda'))
    lab = torch.zeros(1, 16, 16, dtype=torch.int64, device='cuda')
    assert lib.pm_upsample_ce_fwd(byref(lg), 1.0, lab.data_ptr(), 16, 16, m.data_ptr(), wsb.data_ptr(), 1 << 16, st) == EUNSUPPORTED
    assert lib.pm_sliding_stitch(byref(lg), None, 1, 4, 4, 0, m.data_ptr(), 0, st) == EINVAL
    # and the library is still usable
    torch.cuda.synchronize()
    assert rel(nchw(K.conv_fwd(x, w, 1, 1, 1)), F.conv2d(nchw(x), w.permute(0, 3, 1, 2).cpu(), padding=1)) < 2e-5


def test_upsample_ce_rows_too_wide_for_lds_take_the_composed_route(K):
    """the fused up-sample + CE kernels keep two low-res logit rows and one label row in LDS (159 KB: ~1000 low-res columns at 19 classes). Wider
    shapes are reported by pm_upsample_ce_field_bytes == 0 and ops.upsample_ce composes the same loss from the bilinear kernel and torch's cross entropy instead
    of raising -- value and gradient against the reference's expression."""
    from pinthememory_amd.hip import ops
    n, C, hw, HW = 1, 19, (3, 1100), (9, 4400)
    lg = rnd(n, C, *hw, seed=1) * 3
    lab = torch.randint(0, C, (n, *HW), generator=torch.Generator().manual_seed(2))
    lab[:, :1] = 255
    assert not K.upsample_ce_fused_ok(nhwc(lg), HW) and K.upsample_ce_fused_ok(nhwc(lg[..., :900]), (9, 3600))
    lr = lg.clone().requires_grad_(True)
    F.cross_entropy(F.interpolate(lr, size=HW, mode='bilinear', align_corners=True), lab, ignore_index=255).backward()
    lgg = nhwc(lg).permute(0, 3, 1, 2).requires_grad_(True)      # logical NCHW over NHWC memory, as the networks hand it over
    loss = ops.upsample_ce(lgg, lab.cuda())
    loss.backward()
    ref = F.cross_entropy(F.interpolate(lg, size=HW, mode='bilinear', align_corners=True), lab, ignore_index=255)
    assert abs(loss.item() - ref.item()) < 1e-5 * max(1, abs(ref.item()))
    assert rel(lgg.grad.cpu(), lr.grad) < 1e-4


# ---- one case per route of conv_igemm.hip route_conv, at the smallest shape that still takes it ------------------------------------------------------------------
# which (0 forward / 1 data gradient / 2 weight gradient), tier, (n, cin, h, w, cout, k, stride, pad, dil), routing fields, options, profiler record that proves the kernel
# (mode, prec): mode 0 / 1 / 2 the implicit-GEMM template (the Winograd point products run as mode 0), 4 the LDS-DMA bf16 kernel; prec 4 with km 2 / nst 3 the wgrad16 ring
ROUTE_CASES = {
    'fwd-winograd-f4':        (0, 'f32', (1, 128, 16, 16, 128, 3, 1, 1, 1), {}, {'wxf_points': 36}, (0, None)),
    'fwd-winograd-f2-dilated': (0, 'f32', (1, 128, 12, 12, 128, 3, 1, 6, 6), {}, {'wxf_points': 16}, (0, None)),
    'fwd-bf16-reg-staged':    (0, 'bf16', (1, 64, 8, 8, 64, 3, 1, 1, 1), {}, {}, (0, 2)),
    'fwd-bf16-lds-dma':       (0, 'bf16', (1, 64, 16, 16, 64, 3, 1, 1, 1), {}, {}, (4, 5)),
    'fwd-bf16-48ch-padded':   (0, 'bf16', (1, 48, 16, 16, 64, 3, 1, 1, 1), {}, {'padded_copy': True}, (4, 5)),
    'fwd-direct-splitk':      (0, 'f32', (1, 2048, 4, 4, 256, 3, 1, 1, 1), {'winograd': 0}, {'slabs': True}, (0, 5)),
    'dgrad-winograd':         (1, 'f32', (1, 128, 16, 16, 128, 3, 1, 1, 1), {}, {}, (0, None)),
    'dgrad-s2-parity-f32':    (1, 'f32', (1, 8, 9, 9, 8, 3, 2, 1, 1), {}, {}, (1, 0)),
    'dgrad-s2-native-bf16':   (1, 'bf16', (1, 64, 10, 10, 64, 3, 2, 1, 1), {}, {}, (4, 5)),
    'dgrad-s2-bf16-dy32':     (1, 'bf16', (1, 64, 10, 10, 32, 3, 2, 1, 1), {}, {'upcast_dy': True}, (1, 1)),
    'wgrad-winograd-kept-v':  (2, 'f32', (1, 256, 16, 16, 256, 3, 1, 1, 1), {}, {'keep_v': True}, (2, None)),
    'wgrad-winograd':         (2, 'f32', (1, 256, 16, 16, 256, 3, 1, 1, 1), {}, {'v_bytes': True}, (2, None)),
    'wgrad-direct-splitk-dbias': (2, 'f32', (2, 64, 24, 20, 64, 3, 1, 1, 1), {}, {'dbias': True, 'slabs': True}, (2, None)),
    'wgrad-mixed-stem-dbias': (2, 'stem', (2, 4, 40, 36, 64, 7, 2, 3, 1), {}, {'dbias': True, 'upcast_dy': True}, (2, 3)),
    # (the ring wants Cout >= 128: 128 -> 64 stays on the register-staged bf16 gather, 128 -> 128 is the smallest shape on the ring)
    'wgrad-bf16-native-dbias': (2, 'bf16', (1, 128, 16, 16, 64, 3, 1, 1, 1), {}, {'dbias': True, 'upcast_dy': True}, (2, 4)),
    'wgrad-bf16-ring-dbias':  (2, 'bf16', (1, 128, 16, 16, 128, 3, 1, 1, 1), {}, {'dbias': True, 'upcast_dy': True, 'ring': True}, (2, 4)),
    'wgrad-bf16-ring-off':    (2, 'bf16', (1, 128, 16, 16, 128, 3, 1, 1, 1), {'wgrad16': 0}, {'dbias': True, 'upcast_dy': True, 'ring': False}, (2, 4)),
    'wgrad-bf16-transposed':  (2, 'bf16_operands', (1, 64, 16, 16, 64, 3, 1, 1, 1), {'bf16_wgrad': 1}, {'transposed': True}, (0, 2)),
}


@pytest.mark.parametrize('name', list(ROUTE_CASES))
def test_conv_routes_stay_inside_the_workspace_they_ask_for(K, name):
    """Every route of route_conv through the C ABI with EXACTLY the workspace pm_conv_workspace answers: the allocation carries 4096 guard bytes behind it that must
    come back untouched, the size queries and the profiler's record confirm the route, and the result meets the comparator and tolerance of the route's own test above
    (fp32: fp64 convolution, 2e-5 / 5e-5 for dw; bf16 tensors: one-and-a-half bf16 roundings of the fp32 formula on the rounded operands; dw of the bf16 forms 2e-4)."""
    import ctypes
    from ctypes import byref
    from pinthememory_amd.hip import lib as L
    which, tier, (n, cin, h, w, cout, k, s, p, d), route, opt, (rec_mode, rec_prec) = ROUTE_CASES[name]
    lib = L.load()
    r16 = (lambda t: t) if tier == 'f32' else (lambda t: t.bfloat16().float())
    dev = lambda t, dt: nhwc(t).to(dt)
    xdt = torch.float32 if tier in ('f32', 'stem', 'bf16_operands') else torch.bfloat16
    ydt = torch.float32 if tier in ('f32', 'bf16_operands') else torch.bfloat16
    prec = 0 if tier == 'f32' else 2
    x = rnd(n, cin, h, w, seed=1) if tier in ('stem', 'bf16_operands') else r16(rnd(n, cin, h, w, seed=1))
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    ref_t = torch.float64 if tier == 'f32' else torch.float32
    xr, wr = r16(x).to(ref_t).requires_grad_(True), (wt if which == 2 else r16(wt)).to(ref_t).requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=s, padding=p, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    y_ref.backward(r16(dy).to(ref_t))
    wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
    xg = dev(x, xdt)
    yg = torch.empty((n,) + tuple(y_ref.shape[2:]) + (cout,), dtype=ydt, device='cuda') if which == 0 else dev(r16(dy) if tier != 'bf16_operands' else dy, ydt)
    if which == 1:
        xg = torch.empty_like(xg)
    before = K.routing(**route)
    try:
        xd, yd, prm = L.tdesc(xg), L.tdesc(yg), L.conv_params(k, k, s, p, d, prec)
        need = lib.pm_conv_workspace(byref(xd), byref(yd), byref(prm), which)
        nbv, nbu = lib.pm_conv_winograd_v_bytes(byref(xd), byref(yd), byref(prm)), lib.pm_conv_wxf_bytes(byref(xd), byref(yd), byref(prm))
        # -- the route, as the size queries tell it
        al = lambda v: (v + 255) // 256 * 256
        kp = (cin + 31) // 32 * 32
        if 'wxf_points' in opt:
            assert nbu == al(opt['wxf_points'] * cout * kp * 4) and wino_route(h, w, d, 4) == {36: 4, 16: 2}[opt['wxf_points']]
        elif which == 0 and tier == 'bf16':
            assert nbu == al(cout * k * k * ((cin + 63) // 64 * 64) * 2)
            assert (need - nbu >= al(n * h * w * 64 * 2)) == bool(opt.get('padded_copy'))
        elif which == 0:
            assert nbu == 0 and need >= 2 * n * y_ref.shape[2] * y_ref.shape[3] * cout * 4      # no transformed filter, at least two split-K slabs
        if which == 1 and tier == 'bf16':
            assert lib.pm_conv_wxf_bytes_dgrad(byref(yd), byref(xd), byref(prm)) == 0      # stride 2: no kept rotated filter
        if which == 2:
            P = n * y_ref.shape[2] * y_ref.shape[3]
            cb = max(1, (cout + 63) // 64)
            want = 256 if cb == 1 else max(1, 1024 // cb)
            bias_part = al(-(-P // min(2048, max(64, -(-P // want)))) * cout * 4)      # conv_igemm.hip colsum_rows
            own = need - bias_part - (al(P * cout * 4) if opt.get('upcast_dy') else 0) - (al(n * h * w * cin * 4) if (tier == 'bf16' and xdt == torch.bfloat16) else 0)
            assert (nbv > 0) == ('keep_v' in opt or 'v_bytes' in opt)
            if nbv:
                assert own > 2 * nbv                                        # V, Z and the slabs
            if opt.get('slabs'):
                assert own >= 2 * cout * k * k * cin * 4                    # at least two split-K slabs of dw
            if opt.get('transposed'):
                assert own >= al(cout * P * 2) + al(k * k * cin * P * 2)    # dy^T and the per-tap x^T
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        K.profile_enable(True)
        K.profile_read(clear=True)
        st = L.stream()
        if which == 0:
            L.check(lib.pm_conv_fwd(byref(xd), wg.data_ptr(), byref(yd), byref(prm), None, ws.data_ptr(), need, st), 'pm_conv_fwd')
        elif which == 1:
            L.check(lib.pm_conv_bwd_data(byref(yd), wg.data_ptr(), byref(xd), byref(prm), None, ws.data_ptr(), need, st), 'pm_conv_bwd_data')
        else:
            dw = torch.empty_like(wg)
            db = torch.empty(cout, device='cuda') if opt.get('dbias') else None
            if opt.get('keep_v'):      # the forward pass leaves its transformed input for the weight gradient
                v, y0 = torch.empty(nbv // 4, device='cuda'), torch.empty_like(yg)
                pf = L.conv_params(k, k, s, p, d, prec)
                pf.wino_v, pf.wino_v_bytes = v.data_ptr(), nbv
                nf = lib.pm_conv_workspace(byref(xd), byref(yd), byref(pf), 0)
                wf = torch.full((nf + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
                L.check(lib.pm_conv_fwd(byref(xd), wg.data_ptr(), byref(L.tdesc(y0)), byref(pf), None, wf.data_ptr(), nf, st), 'pm_conv_fwd')
                assert bool((wf[nf:] == 0xA5).all())
                K.profile_read(clear=True)
                prm.wino_v, prm.wino_v_bytes = v.data_ptr(), nbv
            L.check(lib.pm_conv_bwd_weight(byref(xd), byref(yd), dw.data_ptr(), L.ptr(db), byref(prm), ws.data_ptr(), need, st), 'pm_conv_bwd_weight')
        torch.cuda.synchronize()
        K.profile_enable(False)
        assert bool((ws[need:] == 0xA5).all()), 'the call wrote behind the workspace it asked for'
        # -- the kernel, as the profiler recorded it
        assert K.profile_read(mode=rec_mode, prec=-1 if rec_prec is None else rec_prec)[2] > 0, 'no launch of the expected kernel form'
        if which != rec_mode and rec_mode != 4 and not opt.get('transposed'):
            assert K.profile_read(mode=which)[2] == 0      # Winograd point products run as forward GEMMs, never the direct data gradient
        if 'ring' in opt:
            assert any(K.profile_read(mode=2, bm=bm, bn=bn, km=2, nst=3, prec=4)[2] for bm, bn in ((256, 128), (128, 256))) == opt['ring']
        K.profile_read(clear=True)
    finally:
        K.profile_enable(False)
        K.routing(**before)
    if which == 0:
        if ydt == torch.bfloat16:
            close16(nchw(yg.float()), y_ref.detach(), ulps=1.5)
        else:
            assert rel(nchw(yg), y_ref.detach()) < 2e-5
    elif which == 1:
        if xdt == torch.bfloat16:
            close16(nchw(xg.float()), xr.grad, ulps=1.5)
        else:
            assert rel(nchw(xg), xr.grad) < 2e-5
    else:
        assert rel(dw.permute(0, 3, 1, 2), wr.grad) < (5e-5 if tier == 'f32' else 2e-4)
        if db is not None:
            assert rel(db, r16(dy).sum((0, 2, 3))) < 2e-5
