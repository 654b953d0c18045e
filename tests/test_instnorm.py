"""GPU: the per-image normalisation kernels (csrc/instnorm.hip: pm_instnorm_fwd / pm_instnorm_bwd) against fp64 torch on the same values.

Tolerance, per output tensor: err_hip <= 2 * err_ref + 8 * 2^-24 * max(1, max|want|), all errors max-abs against the fp64 truth. err_ref is the error of torch's own
fp32 instance norm (+ autograd) on CPU -- the factor 2 covers another summation order; the floor is four roundings of the apply chain plus those of mean and invstd,
so that a lucky err_ref cannot fail a correct kernel. torch.instance_norm is called directly: it is what F.instance_norm calls after a size check that refuses one
value per channel, which is one of the cases here (HW = 1: variance 0). mean / invstd of the reference come from torch.native_batch_norm on the [1, N * C, H, W] view,
the call instance norm makes internally. The backward pass is held as the function of (dy, x, y) it is: its ReLU mask comes from the y it is handed (the fp64 forward
rounded to fp32), the same for the kernel, the fp32 reference and the truth, so a unit within round-off of zero cannot flip between them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (n, h, w, c): HW = 1 (variance 0) | HW = 63, one ragged chunk | several row chunks with a ragged tail, C neither a power of two nor a multiple of 64 | layer2 at the test size
SHAPES = [(3, 1, 1, 8), (2, 7, 9, 8), (3, 49, 47, 264), (2, 16, 16, 512)]
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def inputs(shape, affine, seed=0, offset=False):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(1000 * seed + c + h)
    x = torch.randn(shape, generator=g)
    if offset:      # channel means of 1e3 with a deviation of 1e-2: what the shifted sums are for
        x = 1e3 * (1 + torch.rand(c, generator=g)) + 1e-2 * x
    dy = torch.randn(shape, generator=g)
    gamma = (1 + 0.3 * torch.randn(c, generator=g)) if affine else None
    beta = 0.2 * torch.randn(c, generator=g) if affine else None
    return x, dy, gamma, beta


def forward_ref(x, gamma, beta, dtype):
    """-> (y before the ReLU [n,h,w,c], mean [n,c], invstd [n,c]) in `dtype` on CPU"""
    n, h, w, c = x.shape
    xv = x.to(dtype).permute(0, 3, 1, 2).contiguous()
    ga, be = (gamma.to(dtype), beta.to(dtype)) if gamma is not None else (None, None)
    y = torch.instance_norm(xv, ga, be, None, None, True, 0.1, EPS, False)
    _, mean, invstd = torch.native_batch_norm(xv.reshape(1, n * c, h, w), None, None, None, None, True, 0.1, EPS)
    return y.permute(0, 2, 3, 1), mean.view(n, c), invstd.view(n, c)


def backward_ref(x, g, gamma, beta, dtype):
    """autograd of torch's instance norm for the (already masked) output gradient g -> (dx [n,h,w,c], dgamma, dbeta)"""
    xv = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ga, be = (gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)) if gamma is not None else (None, None)
    y = torch.instance_norm(xv, ga, be, None, None, True, 0.1, EPS, False)
    y.backward(g.to(dtype).permute(0, 3, 1, 2))
    return xv.grad.permute(0, 2, 3, 1), (ga.grad if ga is not None else None), (be.grad if be is not None else None)


_REF = {}


def reference(shape, relu, affine, offset=False):
    """Computed once per case and shared: inputs, the fp64 truth and the error of torch's fp32 pass against it, per output tensor."""
    key = (shape, relu, affine, offset)
    if key not in _REF:
        x, dy, gamma, beta = inputs(shape, affine, offset=offset)
        y64, m64, i64 = forward_ref(x, gamma, beta, torch.float64)
        y32, m32, i32 = forward_ref(x, gamma, beta, torch.float32)
        act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
        y_in = act(y64).float().contiguous()                                   # the forward output handed to every backward pass
        g = dy * (y_in > 0) if relu else dy
        want = dict(zip(('y', 'mean', 'invstd', 'dx', 'dgamma', 'dbeta'), (act(y64), m64, i64, *backward_ref(x, g, gamma, beta, torch.float64))))
        ref = dict(zip(('y', 'mean', 'invstd', 'dx', 'dgamma', 'dbeta'), (act(y32), m32, i32, *backward_ref(x, g, gamma, beta, torch.float32))))
        err_ref = {k: (ref[k].double() - want[k]).abs().max().item() for k in want if want[k] is not None}
        _REF[key] = (x, dy, gamma, beta, y_in, want, err_ref)
    return _REF[key]


def cuda(t):
    return None if t is None else t.cuda()


def check(case, got, want, err_ref):
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
            continue
        err = (got[k].double().cpu() - w).abs().max().item()
        bound = 2 * err_ref[k] + 8 * 2.0 ** -24 * max(1.0, w.abs().max().item())
        print('instnorm %s %-6s err_hip %.3e err_ref %.3e bound %.3e' % (case, k, err, err_ref[k], bound))
        assert err <= bound, (case, k, err, err_ref[k], bound)


def run(K, x, dy, gamma, beta, y_in, relu):
    xg, gg, bg = x.cuda(), cuda(gamma), cuda(beta)
    y, mean, invstd = K.instnorm_fwd(xg, gg, bg, EPS, relu)
    dx, dgamma, dbeta = K.instnorm_bwd(dy.cuda(), xg, y_in.cuda(), gg, mean, invstd, relu, want_affine=gamma is not None)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_forward_and_backward_against_fp64(K, shape, relu, affine):
    x, dy, gamma, beta, y_in, want, err_ref = reference(shape, relu, affine)
    check('%s relu%d affine%d' % (ids(shape), relu, affine), run(K, x, dy, gamma, beta, y_in, relu), want, err_ref)


@pytest.mark.parametrize('shape', [(2, 7, 9, 8), (3, 49, 47, 264)], ids=ids)
def test_large_offset_input(K, shape):
    """channel means of 1e3 with a deviation of 1e-2, under the same rule"""
    x, dy, gamma, beta, y_in, want, err_ref = reference(shape, True, True, offset=True)
    check('%s offset' % ids(shape), run(K, x, dy, gamma, beta, y_in, True), want, err_ref)


POISON = 777.25      # exact in bf16


def slab(t, width, off, dtype):
    """-> (slab [n,h,w,width] of POISON on the device, its channel slice [off : off + c] holding t, or left poisoned when t is None)"""
    n, h, w, c = t.shape if torch.is_tensor(t) else t
    s = torch.full((n, h, w, width), POISON, dtype=dtype, device='cuda')
    v = s[..., off:off + c]
    if torch.is_tensor(t):
        v.copy_(t)
    return s, v


def untouched(s, off, c):
    q = s.clone()
    q[..., off:off + c] = POISON
    return bool((q == POISON).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 7, 9, 8), (3, 49, 47, 264)], ids=ids)
def test_pitched_views_in_poisoned_slabs(K, shape, dtype):
    """x, y, dy, dx as channel slices of wider, poisoned slabs: every byte outside [.., :c] is unchanged afterwards, results bit-equal to the dense call"""
    c = shape[3]
    x, dy, gamma, beta = inputs(shape, True, seed=3)
    x, dy, gg, bg = x.to(dtype).cuda(), dy.to(dtype).cuda(), gamma.cuda(), beta.cuda()
    y, mean, invstd = K.instnorm_fwd(x, gg, bg, EPS, True)
    dx, dgamma, dbeta = K.instnorm_bwd(dy, x, y, gg, mean, invstd, True)
    (xs, xv), (ys, yv), (ds, dv), (gs, gv) = slab(x, c + 8, 8, dtype), slab(shape, c + 16, 0, dtype), slab(dy, c + 24, 16, dtype), slab(shape, c + 8, 0, dtype)
    y2, mean2, invstd2 = K.instnorm_fwd(xv, gg, bg, EPS, True, out=yv)
    dx2, dgamma2, dbeta2 = K.instnorm_bwd(dv, xv, yv, gg, mean2, invstd2, True, out=gv)
    torch.cuda.synchronize()
    assert y2.data_ptr() == yv.data_ptr() and dx2.data_ptr() == gv.data_ptr()
    for a, b in ((y, yv), (mean, mean2), (invstd, invstd2), (dx, gv), (dgamma, dgamma2), (dbeta, dbeta2)):
        assert torch.equal(a, b)
    assert torch.equal(xv, x) and torch.equal(dv, dy)
    assert untouched(xs, 8, c) and untouched(ys, 0, c) and untouched(ds, 16, c) and untouched(gs, 0, c)


def ordered(t):
    """bf16 bit patterns as integers in value order: neighbours differ by one"""
    b = t.view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7fff), b)


@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('shape', SHAPES[1:], ids=ids)
def test_bf16_against_the_fp32_instantiation(K, shape, relu):
    """mean / invstd bit-equal to the fp32 instantiation run on the widened input; y and dx within one bf16 ulp of that instantiation's result rounded to bf16"""
    x, dy, gamma, beta = inputs(shape, True, seed=5)
    x, dy, gg, bg = x.bfloat16().cuda(), dy.bfloat16().cuda(), gamma.cuda(), beta.cuda()
    y16, m16, i16 = K.instnorm_fwd(x, gg, bg, EPS, relu)
    y32, m32, i32 = K.instnorm_fwd(x.float(), gg, bg, EPS, relu)
    assert y16.dtype == torch.bfloat16 and torch.equal(m16, m32) and torch.equal(i16, i32)
    dx16, dg16, db16 = K.instnorm_bwd(dy, x, y16, gg, m16, i16, relu)
    dx32, dg32, db32 = K.instnorm_bwd(dy.float(), x.float(), y16.float(), gg, m32, i32, relu)
    torch.cuda.synchronize()
    for got, want in ((y16, y32), (dx16, dx32)):
        assert got.dtype == torch.bfloat16
        assert (ordered(got) - ordered(want.bfloat16())).abs().max().item() <= 1
    assert torch.equal(dg16, dg32) and torch.equal(db16, db32)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_two_runs_are_bit_equal_and_y_may_alias_x(K, dtype):
    shape = (3, 49, 47, 264)
    x, dy, gamma, beta = inputs(shape, True, seed=7)
    x, dy, gg, bg = x.to(dtype).cuda(), dy.to(dtype).cuda(), gamma.cuda(), beta.cuda()
    runs = []
    for _ in range(2):
        y, mean, invstd = K.instnorm_fwd(x, gg, bg, EPS, True)
        runs.append((y, mean, invstd, *K.instnorm_bwd(dy, x, y, gg, mean, invstd, True)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    xa = x.clone()
    ya, ma, ia = K.instnorm_fwd(xa, gg, bg, EPS, True, out=xa)
    torch.cuda.synchronize()
    assert ya.data_ptr() == xa.data_ptr() and torch.equal(xa, runs[0][0]) and torch.equal(ma, runs[0][1]) and torch.equal(ia, runs[0][2])


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
def test_autograd_node_on_strided_views_and_without_grad(K, affine):
    """ops.instance_norm_act: logical NCHW in and out over the strided NHWC views ops.nhwc hands on; the same bits with and without a graph; gradients against
    torch's own autograd under the rule above (the ReLU mask is the node's own output: units within round-off of zero are screened out)"""
    from pinthememory_amd.hip import ops
    shape = (2, 7, 9, 8)
    x, dy, gamma, beta = inputs(shape, affine, seed=9)
    wide = torch.full((2, 7, 9, 24), POISON, device='cuda')
    wide[..., 8:16] = x.cuda()
    xl = wide[..., 8:16].permute(0, 3, 1, 2).requires_grad_(True)              # logical NCHW over a channel slice
    gg, bg = (gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)) if affine else (None, None)
    out = ops.instance_norm_act(xl, gg, bg, EPS, True)
    with torch.no_grad():
        out0 = ops.instance_norm_act(xl, gg, bg, EPS, True)
    assert out.shape == xl.shape and not out0.requires_grad and torch.equal(out, out0)
    y64, _, _ = forward_ref(x, gamma, beta, torch.float64)
    y32, _, _ = forward_ref(x, gamma, beta, torch.float32)
    far = y64.abs() > 1e-4                                                       # units whose ReLU branch no rounding decides
    assert bool(far.all()), 'the seeded case has no unit within 1e-4 of zero'
    g = dy * (y64 > 0)
    want = backward_ref(x, g, gamma, beta, torch.float64)
    ref = backward_ref(x, g, gamma, beta, torch.float32)
    grads = torch.autograd.grad(out, [xl] + ([gg, bg] if affine else []), dy.cuda().permute(0, 3, 1, 2))
    got = [grads[0].permute(0, 2, 3, 1)] + list(grads[1:])
    ey = (out.permute(0, 2, 3, 1).double().cpu() - y64.clamp_min(0)).abs().max().item()
    assert ey <= 2 * (y32.double() - y64).abs().max().item() + 8 * 2.0 ** -24 * max(1.0, y64.abs().max().item())
    for a, w, r in zip(got, want, ref):
        err, err_ref = (a.double().cpu() - w).abs().max().item(), (r.double() - w).abs().max().item()
        assert err <= 2 * err_ref + 8 * 2.0 ** -24 * max(1.0, w.abs().max().item()), (err, err_ref)
