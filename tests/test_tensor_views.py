"""Every tensor entry point of the C ABI on strided views inside poisoned slabs (tools/view_slabs.py), called through the raw ctypes table as a foreign host would.

A pm_tensor is (ptr, n, h, w, c, pitch >= c): the header promises that a call touches channels [0, c) of its n*h*w pixels and nothing else, and the network relies on
it (channel slices of the ASPP / decoder concat buffers). Each case here puts every tensor of one call into memory the test owns -- 256 poisoned pixels of the slab's
full width before and after the view, poisoned channels left and right of it, 64 poisoned elements around every flat array -- and holds the call to

    PM_OK, the family's fp64 reference met at the bar of the family's existing test, every output element finite, every byte outside the views as it was, every byte
    of every input as it was;  or
    a negative status before any launch: every byte as it was, pm_last_error() not empty -- and the (entry point, layout) pair is listed in REFUSES.

Layouts (view_slabs.geometry): dense; slice (fp32 offset 32 / pitch c + 64, bf16 offset 64 / pitch c + 128); odd (fp32 only: offset 1, pitch c + 3 -- base not
16-byte aligned, pitch no multiple of 4; an entry point takes it on element-wise accesses or refuses it, checked by READING its host function before the case was
written); ownpad (fp32: 19 channels on pitch 20 with a zero pad lane that stays zero); ownpad64 (view_slabs' ownpad for bf16: c % 64 != 0 with zero lanes up to
the next multiple of 64 inside a wider pitch -- the 48- and 304-channel concat parts).

What this cannot show: NaN poison shows an over-read only where the value REACHES A RESULT (0 * NaN does, a load that a select discards does not), and an
over-write only inside the slab (256 pixels either side)."""
import ctypes
import importlib.util
import os
from ctypes import POINTER, byref, pointer

import pytest
import torch
import torch.nn.functional as F

from test_hip_kernels import close16, rel, rnd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('view_slabs', os.path.join(ROOT, 'tools', 'view_slabs.py'))
VS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VS)

EINVAL, EUNSUPPORTED = -1, -4
F32, B16 = torch.float32, torch.bfloat16

# The (entry point, layout) pairs that are turned down, with the status -- asserted exactly: a listed pair that is accepted fails its case, and so does any other pair
# that is refused. Every one was read off the entry point's host function: it needs 16-byte vector views and has no scalar twin.
REFUSES = {
    ('pm_add_n', 'odd'): EINVAL,                               # misc.hip add_n: pm_elem<T>::vec() on every operand and the output
    ('pm_global_avgpool_fwd', 'odd'): EINVAL,                  # pool_resize.hip gap_fwd: vec(x)
    ('pm_global_avgpool_bwd', 'odd'): EINVAL,                  # gap_bwd: vec(dx)
    ('pm_resize_bilinear_bwd_separable', 'odd'): EUNSUPPORTED,      # its workspace query answers 0 for views that are no vectors: the gather takes them
    ('pm_resize_bilinear_bwd_separable', 'ownpad'): EUNSUPPORTED,   # the same answer for c % 4 != 0 (hip/kernels.py sends the 19-class gradient to the gather)
}
# every entry point a case below calls (tests/test_tensor_views_cpu.py holds the header against it)
COVERED = set()
# entry points of the table that take flat arrays only (no pm_tensor in the header)
FLAT_ONLY = {'pm_label_nearest', 'pm_image_u8_to_nhwc4', 'pm_labels_u8_to_i64', 'pm_bn_fold', 'pm_bn_fold_multi', 'pm_argmax_f64', 'pm_mem_colsoftmax', 'pm_mem_write_update',
             'pm_mem_write_update_bwd'}
# pm_tensor entry points without a case, name -> one-line reason. None today: the size queries are exempt as a class (they dereference nothing), and the optimizer
# (pm_sgd_momentum*: flat parameter arenas) and the augmenting input edge (flat uint8 batches, margin-checked by bit-equality with PIL) take no pm_tensor at all.
EXEMPT = {}


def covers(*names):
    COVERED.update(names)
    return lambda f: f


@pytest.fixture(scope='module')
def env():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import lib as L
    return L, L.load()


class Call:
    """The buffers of one call and its verdict."""

    def __init__(self, env, entry, layout):
        self.L, self.lib = env
        self.entry, self.layout, self.bufs, self.keep = entry, layout, [], []

    def tensor(self, shape, dtype, role, data=None, layout=None, flags=0):
        """-> (NHWC view inside its own slab, pointer to its pm_tensor)"""
        lay = layout or self.layout
        buf, view = VS.slab(shape, dtype, 'ownpad' if lay == 'ownpad64' else lay, role, data, device='cuda')
        self.bufs.append(buf)
        n, h, w, c = shape
        d = self.L.PmTensor(view.data_ptr(), n, h, w, c, buf.pitch, self.L.PM_F32 if dtype == F32 else self.L.PM_BF16, flags)
        self.keep.append(d)
        return view, pointer(d)

    def flat(self, numel, dtype, role, data=None):
        buf, arr = VS.flat(numel, dtype, role, data, device='cuda')
        self.bufs.append(buf)
        return arr

    def workspace(self, need):
        """exactly `need` bytes, 4096 guard bytes behind them"""
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        self.keep.append((ws, need))
        return ws.data_ptr()

    def run(self, *args, entry=None):
        """Calls the entry point; -> True: PM_OK and the call kept to its views (the caller compares the values); False: refused as REFUSES says, nothing touched."""
        entry = entry or self.entry
        torch.cuda.synchronize()
        before = VS.snapshot(self.bufs)
        status = getattr(self.lib, entry)(*args, self.L.stream())
        torch.cuda.synchronize()
        want = REFUSES.get((entry, self.layout), 0)
        assert status == want, '%s on %s: status %d, expected %d (%s)' % (entry, self.layout, status, want, self.lib.pm_last_error().decode())
        for item in self.keep:
            if isinstance(item, tuple):
                assert bool((item[0][item[1]:] == 0xA5).all()), '%s wrote behind the workspace it asked for' % entry
        if status != 0:
            assert self.lib.pm_last_error(), 'a refusal without a message'
            for old, b in zip(before, self.bufs):
                assert torch.equal(old, b.bytes()), '%s refused the call and still wrote' % entry
            return False
        VS.check(before, self.bufs)
        return True


def fp32_layouts(c):
    return ['dense', 'slice', 'odd'] if c % 4 == 0 else ['dense', 'slice', 'odd', 'ownpad']


def data(shape, dtype, seed, scale=1.0, shift=0.0):
    """CPU values of `shape`, already rounded to dtype (a bf16 case is compared on the rounded values)"""
    return (rnd(*shape, seed=seed) * scale + shift).to(dtype).float()


def cpu(t):
    return t.float().cpu()


def scale_close(got, want, bar):
    assert rel(got, want) < bar, 'rel %.3e >= %.1e' % (rel(got, want), bar)


EW_CASES = [(F32, (2, 5, 7, 8), lay) for lay in ('dense', 'slice', 'odd')] + [(F32, (2, 5, 7, 19), lay) for lay in ('dense', 'slice', 'odd', 'ownpad')] + \
           [(B16, (2, 5, 7, 8), lay) for lay in ('dense', 'slice')] + [(B16, (2, 5, 7, 72), 'ownpad64')]
ew_ids = lambda v: ('f32' if v == F32 else 'bf16') if isinstance(v, torch.dtype) else ('x'.join(map(str, v)) if isinstance(v, tuple) else str(v))


# ---- misc.hip / bf16.hip -------------------------------------------------------------------------------------------------------------------------------------
@covers('pm_add', 'pm_add_n', 'pm_copy')
@pytest.mark.parametrize('dtype,shape,layout', EW_CASES, ids=ew_ids)
def test_add_add_n_copy(env, dtype, shape, layout):
    """fp32: IEEE additions in the documented left-to-right order, so the bits of the same sum in torch; bf16: that sum rounded once (close16, test_act16_pool_resize_add_cast)."""
    xs = [data(shape, dtype, 10 + i) for i in range(5)]

    def same(got, want):
        if dtype == F32:
            assert torch.equal(cpu(got), want)
        else:
            close16(cpu(got), want)
    c = Call(env, 'pm_add', layout)
    (_, a), (_, b), (y, yd) = c.tensor(shape, dtype, 'in', xs[0]), c.tensor(shape, dtype, 'in', xs[1]), c.tensor(shape, dtype, 'out')
    if c.run(a, b, yd):
        same(y, xs[0] + xs[1])
    if shape[3] % 4 == 0:      # pm_add_n has no scalar form (a 19-channel fp32 sum is refused on every layout: tests/golden/pool_bits.json add-c19)
        c = Call(env, 'pm_add_n', layout)
        ds = [c.tensor(shape, dtype, 'in', x)[1] for x in xs]      # five operands, each in its own slab
        arr = (POINTER(c.L.PmTensor) * 5)(*ds)
        y, yd = c.tensor(shape, dtype, 'out')
        if c.run(arr, 5, yd):
            want = xs[0]
            for x in xs[1:]:
                want = want + x
            same(y, want)
    c = Call(env, 'pm_copy', layout)
    (_, a), (y, yd) = c.tensor(shape, dtype, 'in', xs[2]), c.tensor(shape, dtype, 'out')
    if c.run(a, yd):
        assert torch.equal(cpu(y), xs[2])


@covers('pm_cast')
@pytest.mark.parametrize('shape,lay32,lay16', [((2, 5, 7, 8), 'dense', 'dense'), ((2, 5, 7, 8), 'slice', 'slice'), ((2, 5, 7, 8), 'odd', 'dense'), ((2, 5, 7, 8), 'odd', 'slice'),
                                               ((2, 5, 7, 19), 'dense', 'dense'), ((2, 5, 7, 19), 'slice', 'dense'), ((2, 5, 7, 19), 'odd', 'dense'),
                                               ((2, 5, 7, 19), 'ownpad', 'dense'), ((2, 5, 7, 72), 'slice', 'ownpad64')], ids=ew_ids)
def test_cast_both_directions(env, shape, lay32, lay16):
    """Exact both ways (test_act16_pool_resize_add_cast): bf16 -> fp32 widens, fp32 -> bf16 rounds to nearest even as torch does. The fp32 side takes every fp32 layout;
    only the c channels of a pixel are written."""
    x = rnd(*shape, seed=90) * 3
    c = Call(env, 'pm_cast', lay32)
    (_, a), (y, yd) = c.tensor(shape, F32, 'in', x), c.tensor(shape, B16, 'out', layout=lay16)
    assert c.run(a, yd)
    assert torch.equal(cpu(y), x.bfloat16().float())
    c = Call(env, 'pm_cast', lay32)
    (_, a), (y, yd) = c.tensor(shape, B16, 'in', x.bfloat16(), layout=lay16), c.tensor(shape, F32, 'out')
    assert c.run(a, yd)
    assert torch.equal(cpu(y), x.bfloat16().float())


@covers('pm_cast')
def test_cast_into_an_fp32_view_whose_rows_are_8_byte_aligned_only(env):
    """bf16 -> fp32 where both pitches are multiples of 8 but the fp32 view starts 8 bytes into a 16-byte row: the conversion's 16-byte stores do not apply (the
    kernel has to look at the base pointers too, not at the pitches alone). Channels 2 .. 9 of a 16-channel slice are written, the other channels keep their values."""
    L, lib = env
    shape, sub = (2, 5, 7, 16), (2, 5, 7, 8)
    x, old = (rnd(*sub, seed=91) * 3).bfloat16(), rnd(*shape, seed=92)
    c = Call(env, 'pm_cast', 'slice')
    _, a = c.tensor(sub, B16, 'in', x)
    buf, wide = VS.slab(shape, F32, 'slice', 'inout', old, device='cuda')
    c.bufs.append(buf)
    y = wide[..., 2:10]
    assert y.data_ptr() % 16 == 8 and buf.pitch % 8 == 0
    yd = L.PmTensor(y.data_ptr(), 2, 5, 7, 8, buf.pitch, L.PM_F32, 0)
    assert c.run(a, byref(yd))
    want = old.clone()
    want[..., 2:10] = x.float()
    assert torch.equal(cpu(wide), want)


@covers('pm_nchw_to_nhwc', 'pm_nhwc_to_nchw')
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd'])
def test_layout_edges(env, layout):
    """Exact (test_layout_and_labels): 3 -> 4 channels on the thread-per-pixel image kernel, 5 -> 8 on the tiled transpose, channels beyond the source zero-filled;
    19 channels back to planes from an input view."""
    for c_src, c_dst in ((3, 4), (5, 8)):
        x = rnd(2, c_src, 5, 7, seed=20 + c_src)
        c = Call(env, 'pm_nchw_to_nhwc', layout)
        src = c.flat(x.numel(), F32, 'in', x)
        y, yd = c.tensor((2, 5, 7, c_dst), F32, 'out')
        assert c.run(src.data_ptr(), c_src, yd)
        assert torch.equal(cpu(y[..., :c_src]), x.permute(0, 2, 3, 1)) and cpu(y[..., c_src:]).abs().max().item() == 0
    lays = [layout] + (['ownpad'] if layout == 'dense' else [])
    for lay in lays:
        z = rnd(2, 5, 7, 19, seed=30)
        c = Call(env, 'pm_nhwc_to_nchw', lay)
        _, xd = c.tensor((2, 5, 7, 19), F32, 'in', z)
        out = c.flat(z.numel(), F32, 'out')
        assert c.run(xd, out.data_ptr())
        assert torch.equal(cpu(out).view(2, 19, 5, 7), z.permute(0, 3, 1, 2))


@covers('pm_label_nearest', 'pm_image_u8_to_nhwc4', 'pm_labels_u8_to_i64')
def test_flat_input_edges(env):
    """The entry points that take flat arrays only, between margins: nearest labels exact against F.interpolate (test_layout_and_labels), the uint8 image within 1e-6 of
    the loader's formula with a zero fourth lane, labels widened exactly (test_input_edge_u8)."""
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 19, (2, 30, 20), generator=g)
    lab[0, :3] = 255
    for (h, w) in ((4, 3), (9, 7)):
        c = Call(env, 'pm_label_nearest', 'dense')
        src, out = c.flat(lab.numel(), torch.int64, 'in', lab), c.flat(2 * h * w, torch.int64, 'out')
        assert c.run(src.data_ptr(), 2, 30, 20, out.data_ptr(), h, w)
        assert torch.equal(out.cpu().view(2, h, w), F.interpolate(lab.unsqueeze(1).float(), size=(h, w), mode='nearest').squeeze(1).long())
    img = torch.randint(0, 256, (2, 9, 7, 3), generator=g, dtype=torch.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    c = Call(env, 'pm_image_u8_to_nhwc4', 'dense')
    src, out = c.flat(img.numel(), torch.uint8, 'in', img), c.flat(2 * 9 * 7 * 4, F32, 'out')
    assert c.run(src.data_ptr(), 2 * 9 * 7, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), out.data_ptr())
    got = out.cpu().view(2, 9, 7, 4)
    assert (got[..., :3] - (img.float() / 255.0 - torch.tensor(mean)) / torch.tensor(std)).abs().max().item() < 1e-6 and got[..., 3].abs().max().item() == 0
    l8 = torch.randint(0, 256, (2 * 9 * 7,), generator=g, dtype=torch.uint8)
    c = Call(env, 'pm_labels_u8_to_i64', 'dense')
    src, out = c.flat(l8.numel(), torch.uint8, 'in', l8), c.flat(l8.numel(), torch.int64, 'out')
    assert c.run(src.data_ptr(), l8.numel(), out.data_ptr())
    assert torch.equal(out.cpu(), l8.long())


# ---- first references: pm_relu_bwd, pm_scale_shift_act, pm_bn_fold(_multi), pm_argmax_f64, pm_softmax_mean_update, pm_resize_bilinear_hp_fwd -------------------
F32_EW = [((2, 5, 7, 8), lay) for lay in fp32_layouts(8)] + [((2, 5, 7, 19), lay) for lay in fp32_layouts(19)]


@covers('pm_relu_bwd')
@pytest.mark.parametrize('shape,layout', F32_EW, ids=ew_ids)
def test_relu_bwd(env, shape, layout):
    """dx = dy * (y > 0), exact; y == 0 and y == -0.0 pass nothing."""
    dy, y = rnd(*shape, seed=1), rnd(*shape, seed=2)
    y[0, 0, :, 0], y[0, 1, :, 1], y[1, 2, 3, :] = 0.0, -0.0, 0.0
    c = Call(env, 'pm_relu_bwd', layout)
    (_, a), (_, b), (dx, dxd) = c.tensor(shape, F32, 'in', dy), c.tensor(shape, F32, 'in', y), c.tensor(shape, F32, 'out')
    assert c.run(a, b, dxd)
    assert torch.equal(cpu(dx), dy * (y > 0))


@covers('pm_scale_shift_act')
@pytest.mark.parametrize('res,relu', [(False, 0), (True, 1), (True, 0), (False, 1)])
@pytest.mark.parametrize('shape,layout', F32_EW, ids=ew_ids)
def test_scale_shift_act(env, shape, layout, res, relu):
    """y = relu?(x * scale + shift + residual?) against fp64 at the elementwise bar of test_hip_kernels.py, 1e-6 of the tensor's scale."""
    ch = shape[3]
    x, r, sc, sh = rnd(*shape, seed=1) * 2 + 0.5, rnd(*shape, seed=2), rnd(ch, seed=3) * 0.3 + 1.0, rnd(ch, seed=4)
    c = Call(env, 'pm_scale_shift_act', layout)
    _, xd = c.tensor(shape, F32, 'in', x)
    rd = c.tensor(shape, F32, 'in', r)[1] if res else None
    scg, shg = c.flat(ch, F32, 'in', sc), c.flat(ch, F32, 'in', sh)
    y, yd = c.tensor(shape, F32, 'out')
    assert c.run(xd, scg.data_ptr(), shg.data_ptr(), rd, relu, yd)
    want = x.double() * sc.double() + sh.double() + (r.double() if res else 0.0)
    scale_close(y, want.clamp_min(0) if relu else want, 1e-6)


def _fold_ref(g, b, rm, rv, cb, eps):
    s = g.double() / torch.sqrt(rv.double() + eps)
    return s, b.double() - rm.double() * s + (cb.double() * s if cb is not None else 0.0)


@covers('pm_bn_fold', 'pm_bn_fold_multi')
def test_bn_fold_and_fold_multi(env):
    """Eval-mode fold against fp64 at 1e-6 of the tensor's scale, with and without a convolution bias, on flat arrays between margins; the multi-layer form (two layers
    of unequal width, the second wider than one block) against the same reference and bit-equal to pm_bn_fold per layer, as bn.hip says of its expressions."""
    eps, cs = 1e-5, (19, 300)
    par = [[rnd(ch, seed=10 * i + 1) * 0.2 + 1.0, rnd(ch, seed=10 * i + 2) * 0.1, rnd(ch, seed=10 * i + 3), rnd(ch, seed=10 * i + 4).abs() + 0.5] for i, ch in enumerate(cs)]
    single = []
    for i, ch in enumerate(cs):
        for bias in (None, rnd(ch, seed=10 * i + 5)):
            c = Call(env, 'pm_bn_fold', 'dense')
            dev = [c.flat(ch, F32, 'in', p) for p in par[i]]
            cb = c.flat(ch, F32, 'in', bias) if bias is not None else None
            sc, sh = c.flat(ch, F32, 'out'), c.flat(ch, F32, 'out')
            assert c.run(*[d.data_ptr() for d in dev], cb.data_ptr() if bias is not None else None, ch, eps, sc.data_ptr(), sh.data_ptr())
            s_ref, h_ref = _fold_ref(*par[i], bias, eps)
            scale_close(sc, s_ref, 1e-6), scale_close(sh, h_ref, 1e-6)
            if bias is None:
                single.append((sc.clone(), sh.clone()))
    c = Call(env, 'pm_bn_fold_multi', 'dense')
    dev = [[c.flat(ch, F32, 'in', p) for p in par[i]] for i, ch in enumerate(cs)]
    total, offs = sum(cs), (0, cs[0])
    table = c.flat(8, torch.int64, 'in', torch.tensor([d.data_ptr() for layer in dev for d in layer], dtype=torch.int64))
    csd = c.flat(2, torch.int32, 'in', torch.tensor(cs, dtype=torch.int32))
    offd = c.flat(2, torch.int32, 'in', torch.tensor(offs, dtype=torch.int32))
    arena = c.flat(2 * total, F32, 'out')
    assert c.run(table.data_ptr(), csd.data_ptr(), offd.data_ptr(), 2, max(cs), total, eps, arena.data_ptr())
    for i, ch in enumerate(cs):
        sc, sh = arena[offs[i]:offs[i] + ch], arena[total + offs[i]:total + offs[i] + ch]
        s_ref, h_ref = _fold_ref(*par[i], None, eps)
        scale_close(sc, s_ref, 1e-6), scale_close(sh, h_ref, 1e-6)
        assert torch.equal(sc, single[i][0]) and torch.equal(sh, single[i][1])


@covers('pm_argmax_f64')
@pytest.mark.parametrize('with_prob', [True, False])
def test_argmax_f64(env, with_prob):
    """Classes and probabilities exact against torch.max(dim=-1), the FIRST maximum on ties: ties between two and between three classes, maxima in class 0 and in the last."""
    n, h, w, ch = 2, 9, 7, 19
    buf = torch.rand(n, h, w, ch, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    buf[0, 0, 0, 3] = buf[0, 0, 0, 11] = 2.0                      # two-way tie
    buf[0, 1, 2, 4] = buf[0, 1, 2, 5] = buf[0, 1, 2, 18] = 2.0    # three-way tie, the last class among them
    buf[0, 2, :, 0] = 3.0                                         # the maximum in class 0
    buf[1, 3, :, 18] = 3.0                                        # and in the last class
    buf[1, 4, 0, 0] = buf[1, 4, 0, 18] = 2.5                      # first and last tie
    c = Call(env, 'pm_argmax_f64', 'dense')
    src = c.flat(buf.numel(), torch.float64, 'in', buf)
    cls = c.flat(n * h * w, torch.int64, 'out')
    prob = c.flat(n * h * w, torch.float64, 'out') if with_prob else None
    assert c.run(src.data_ptr(), n, h, w, ch, cls.data_ptr(), prob.data_ptr() if with_prob else None)
    flat = buf.view(-1, ch)
    want = torch.tensor([int((row == row.max()).nonzero()[0]) for row in flat])      # the lowest index among the maxima
    assert torch.equal(cls.cpu(), want) and torch.equal(flat.max(dim=-1).values, flat.gather(1, want[:, None])[:, 0])
    assert want[0] == 3 and want[1 * 7 + 2] == 4 and want[(1 * 9 + 4) * 7] == 0
    if with_prob:
        assert torch.equal(prob.cpu(), flat.max(dim=-1).values)


@covers('pm_softmax_mean_update')
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd', 'ownpad'])
def test_softmax_mean_update(env, layout):
    """MeanFusion: three successive updates (counter 1, 2, 3) of the dense float64 buffer with 19 classes, against b + (softmax_fp32(l).double() - b) / cnt in torch at
    the softmax bar of test_memory_read (2e-6); the rows of the final buffer sum to 1 within 1e-6. 33 classes: PM_EINVAL, nothing written."""
    L, lib = env
    shape = (2, 5, 7, 19)
    ref = torch.zeros(shape, dtype=torch.float64)
    c0 = Call(env, 'pm_softmax_mean_update', 'dense')
    acc = c0.flat(ref.numel(), torch.float64, 'inout', torch.full(shape, 0.25, dtype=torch.float64))      # counter 1 replaces whatever is there: b + (p - b) / 1
    ref.fill_(0.25)
    for cnt in (1, 2, 3):
        lg = rnd(*shape, seed=40 + cnt) * 3
        c = Call(env, 'pm_softmax_mean_update', layout)
        c.bufs.append(c0.bufs[0])
        _, ld = c.tensor(shape, F32, 'in', lg)
        assert c.run(ld, acc.data_ptr(), cnt)
        ref = ref + (torch.softmax(lg, dim=-1).double() - ref) / cnt
        assert (acc.cpu().view(shape) - ref).abs().max().item() < 2e-6, cnt
    assert (acc.cpu().view(shape).sum(-1) - 1.0).abs().max().item() < 1e-6
    c = Call(env, 'pm_softmax_mean_update', 'dense')
    big = (1, 3, 3, 33)
    _, ld = c.tensor(big, F32, 'in', rnd(*big, seed=44))
    keep = c.flat(9 * 33, torch.float64, 'inout', torch.zeros(9 * 33, dtype=torch.float64))
    torch.cuda.synchronize()
    before = VS.snapshot(c.bufs)
    assert lib.pm_softmax_mean_update(ld, keep.data_ptr(), 1, L.stream()) == EINVAL and lib.pm_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(o, b.bytes()) for o, b in zip(before, c.bufs))


@covers('pm_resize_bilinear_hp_fwd')
@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('shape,size', [((1, 9, 7, 19), (14, 20)), ((1, 20, 14, 19), (9, 7)), ((2, 5, 5, 8), (5, 5))], ids=ew_ids)
def test_resize_bilinear_hp_fwd(env, shape, size, flip, capsys):
    """Half-pixel bilinear (F.interpolate(align_corners=False)) with the un-flip on the way out, on every fp32 layout. The kernel follows ATen's fp32 coordinate
    arithmetic, so its distance from fp64 is held to ATen's own: err(kernel, fp64) <= 2 * err(ATen fp32, fp64) + 2e-7 (the project's three-way criterion)."""
    n, h, w, ch = shape
    x = rnd(*shape, seed=50)
    nchw = x.permute(0, 3, 1, 2)
    unflip = (lambda t: torch.flip(t, dims=[3])) if flip else (lambda t: t)
    aten = unflip(F.interpolate(nchw, size=size, mode='bilinear', align_corners=False)).permute(0, 2, 3, 1)
    ref = unflip(F.interpolate(nchw.double(), size=size, mode='bilinear', align_corners=False)).permute(0, 2, 3, 1)
    e_aten = rel(aten, ref)
    for layout in fp32_layouts(ch):
        c = Call(env, 'pm_resize_bilinear_hp_fwd', layout)
        (_, xd), (y, yd) = c.tensor(shape, F32, 'in', x), c.tensor((n,) + size + (ch,), F32, 'out')
        assert c.run(xd, yd, flip)
        e_kernel = rel(y, ref)
        with capsys.disabled():
            print('\n[hp resize %s -> %s flip %d %s] kernel vs fp64 %.3e, ATen fp32 vs fp64 %.3e' % (shape, size, flip, layout, e_kernel, e_aten))
        assert e_kernel <= 2.0 * e_aten + 2e-7, (e_kernel, e_aten)


# ---- pool_resize.hip -----------------------------------------------------------------------------------------------------------------------------------------
TIERS = [(F32, lay) for lay in ('dense', 'slice', 'odd')] + [(B16, lay) for lay in ('dense', 'slice', 'ownpad64')]      # ownpad64: the 48- / 304-channel concat parts' layout


def _same16(dtype, got, want, ulps=1.0):
    """fp32: the bar the caller names; bf16: the fp32 formula on the rounded values, one rounding (test_act16_pool_resize_add_cast)"""
    close16(cpu(got), want, ulps=ulps)


@covers('pm_maxpool3x3s2_fwd', 'pm_maxpool3x3s2_bwd')
@pytest.mark.parametrize('dtype,layout', TIERS, ids=ew_ids)
def test_maxpool(env, dtype, layout):
    """(2, 21, 18, 8): odd extents, ragged window rows. Forward exact against F.max_pool2d and the argmax bytes name a tap that holds the maximum; backward against
    autograd at 1e-6 (test_pool_and_resize) / one bf16 rounding."""
    shape = (2, 21, 18, 8)
    x = data(shape, dtype, 1)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y_ref = F.max_pool2d(xr, 3, 2, 1)
    oshape = (2, y_ref.shape[2], y_ref.shape[3], 8)
    dy = data(oshape, dtype, 2)
    y_ref.backward(dy.permute(0, 3, 1, 2).double())
    c = Call(env, 'pm_maxpool3x3s2_fwd', layout)
    (_, xd), (y, yd) = c.tensor(shape, dtype, 'in', x), c.tensor(oshape, dtype, 'out')
    arg = c.flat(y_ref.numel(), torch.uint8, 'out')
    assert c.run(xd, yd, arg.data_ptr())
    assert torch.equal(cpu(y).double(), y_ref.detach().permute(0, 2, 3, 1))
    assert int(arg.max()) <= 8
    c = Call(env, 'pm_maxpool3x3s2_bwd', layout)
    _, dyd = c.tensor(oshape, dtype, 'in', dy)
    argin = c.flat(arg.numel(), torch.uint8, 'in', arg)
    dx, dxd = c.tensor(shape, dtype, 'out')
    assert c.run(dyd, argin.data_ptr(), dxd)
    want = xr.grad.permute(0, 2, 3, 1)
    if dtype == F32:
        scale_close(dx, want, 1e-6)
    else:
        close16(cpu(dx), want.float())


@covers('pm_global_avgpool_fwd', 'pm_global_avgpool_bwd')
@pytest.mark.parametrize('ch', [8, 72])
@pytest.mark.parametrize('dtype,layout', TIERS, ids=ew_ids)
def test_global_avgpool(env, dtype, layout, ch):
    """(3, 7, 9, c): 63 pixels -- fewer than one trip of the unrolled row loop, so the tail loop alone; c = 72 is more than one block of channels on fp32. fp64 mean
    at 1e-6 (test_pool_and_resize) / one bf16 rounding; the backward non-accumulating and accumulating."""
    shape, pooled = (3, 7, 9, ch), (3, 1, 1, ch)
    x = data(shape, dtype, 3, shift=0.5)
    c = Call(env, 'pm_global_avgpool_fwd', layout)
    (_, xd), (y, yd) = c.tensor(shape, dtype, 'in', x), c.tensor(pooled, dtype, 'out')
    if c.run(xd, yd):
        want = x.double().mean((1, 2), keepdim=True)
        scale_close(y, want, 1e-6) if dtype == F32 else close16(cpu(y), want.float())
    dy, old = data(pooled, dtype, 4), data(shape, dtype, 5)
    for acc in (0, 1):
        c = Call(env, 'pm_global_avgpool_bwd', layout)
        _, dyd = c.tensor(pooled, dtype, 'in', dy)
        dx, dxd = c.tensor(shape, dtype, 'inout', old) if acc else c.tensor(shape, dtype, 'out')
        if c.run(dyd, dxd, acc):
            want = (dy.double() / 63.0).expand(shape) + (old.double() if acc else 0.0)
            scale_close(dx, want, 1e-6) if dtype == F32 else close16(cpu(dx), want.float())


RESIZE_CASES = [((1, 11, 7, 8), (30, 41)), ((1, 13, 18, 16), (50, 70)), ((2, 1, 1, 8), (12, 12))]
RESIZE_RUNS = [(dt, lay, s, z) for dt, lay in TIERS for s, z in RESIZE_CASES] + [(F32, 'ownpad', (1, 6, 5, 19), (24, 20))]


@covers('pm_resize_bilinear_fwd', 'pm_resize_bilinear_bwd', 'pm_resize_bilinear_bwd_separable')
@pytest.mark.parametrize('dtype,layout,shape,size', RESIZE_RUNS, ids=ew_ids)
def test_resize_bilinear(env, dtype, layout, shape, size):
    """align_corners=True against F.interpolate in fp64 and its autograd: forward 2e-6, gather and separable backward 1e-5 (test_pool_and_resize); bf16 one rounding
    forward, two backward (test_act16_pool_resize_add_cast). Backward non-accumulating and accumulating. The separable form is asked only where its workspace query
    answers (an up-sampling ratio >= 2 both ways) -- and under the layouts where REFUSES says it answers 0, to see the refusal."""
    L, lib = env
    n, h, w, ch = shape
    big = (n,) + size + (ch,)
    x = data(shape, dtype, 5)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y_ref = F.interpolate(xr, size=size, mode='bilinear', align_corners=True)
    dy = data(big, dtype, 6)
    y_ref.backward(dy.permute(0, 3, 1, 2).double())
    c = Call(env, 'pm_resize_bilinear_fwd', layout)
    (_, xd), (y, yd) = c.tensor(shape, dtype, 'in', x), c.tensor(big, dtype, 'out')
    assert c.run(xd, yd)
    want = y_ref.detach().permute(0, 2, 3, 1)
    scale_close(y, want, 2e-6) if dtype == F32 else close16(cpu(y), want.float())
    old = data(shape, dtype, 7)
    gwant = xr.grad.permute(0, 2, 3, 1)
    eligible = h >= 2 and w >= 2 and size[0] >= 2 * h and size[1] >= 2 * w
    for entry in ('pm_resize_bilinear_bwd', 'pm_resize_bilinear_bwd_separable'):
        if entry.endswith('separable') and not eligible:
            continue
        for acc in (0, 1):
            c = Call(env, entry, layout)
            _, dyd = c.tensor(big, dtype, 'in', dy)
            dx, dxd = c.tensor(shape, dtype, 'inout', old) if acc else c.tensor(shape, dtype, 'out')
            if entry.endswith('separable'):
                need = lib.pm_resize_bilinear_bwd_workspace(dyd, dxd)
                assert (need == 0) == ((entry, layout) in REFUSES)
                ok = c.run(dyd, dxd, acc, c.workspace(need), need)
            else:
                ok = c.run(dyd, dxd, acc)
            if ok:
                w_acc = gwant + (old.double() if acc else 0.0)
                scale_close(dx, w_acc, 1e-5) if dtype == F32 else close16(cpu(dx), w_acc.float(), ulps=2.0)


@covers('pm_sliding_stitch')
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd', 'ownpad'])
def test_sliding_stitch(env, layout):
    """(96, 200), crop 64, overlap 0.5, the tiles' logits as a view, first overwriting and then accumulating the flipped pass: the bits of the host formulation
    (float64 sums in tile order / count, un-flip, add), as test_sliding_stitch demands."""
    from pinthememory_amd import harness
    H, W, crop, C = 96, 200, 64, 19
    tiles = harness.sliding_tiles(H, W, crop, 0.5)
    xyxy = (ctypes.c_int32 * (4 * len(tiles)))(*[v for t in tiles for v in t])
    ref, c0 = None, Call(env, 'pm_sliding_stitch', layout)
    acc = c0.flat(C * H * W, torch.float64, 'out')
    for flip in (0, 1):
        lg = rnd(len(tiles), crop, crop, C, seed=5 + flip)
        full, cnt = torch.zeros(C, H, W, dtype=torch.float64), torch.zeros(1, H, W, dtype=torch.float64)
        for i, (x1, y1, x2, y2) in enumerate(tiles):
            full[:, y1:y2, x1:x2] += lg[i].permute(2, 0, 1).double()
            cnt[:, y1:y2, x1:x2] += 1
        full = full / cnt
        full = torch.flip(full, dims=[2]) if flip else full
        ref = full if ref is None else ref + full
        c = Call(env, 'pm_sliding_stitch', layout)
        c.bufs.append(c0.bufs[0])
        c0.bufs[0].role = 'inout'
        _, ld = c.tensor((len(tiles), crop, crop, C), F32, 'in', lg)
        assert c.run(ld, xyxy, len(tiles), H, W, flip, acc.data_ptr(), flip)
        assert torch.equal(acc.cpu().view(C, H, W), ref)


# ---- bn.hip, both tiers ------------------------------------------------------------------------------------------------------------------------------------------
BN_RUNS = [(F32, s, lay) for s in ((2, 5, 7, 8), (1, 3, 3, 68), (2, 9, 11, 64)) for lay in ('dense', 'slice')] + \
          [(B16, s, lay) for s in ((2, 5, 7, 8), (2, 9, 11, 64)) for lay in ('dense', 'slice')] + [(B16, (2, 5, 7, 8), 'ownpad64')]
BN_ENTRIES = ('pm_bn_stats', 'pm_bn_stats_finalize', 'pm_bn_apply', 'pm_bn_apply_mask', 'pm_bn_apply_mask_affine', 'pm_bn_bwd_reduce', 'pm_bn_bwd_reduce_mask',
              'pm_bn_bwd_apply', 'pm_bn_bwd_apply_mask', 'pm_maxpool3x3s2_bn_relu_fwd', 'pm_bn_bwd_reduce_pool', 'pm_bn_bwd_apply_pool')
# bn.hip: every entry point starts with pm_elem<T>::check() on each tensor -- 16-byte vector views or PM_EINVAL; the file has no scalar form
REFUSES.update({(e, 'odd'): EINVAL for e in BN_ENTRIES})


def _unpack_mask(mask, shape, V):
    n, h, w, c = shape
    bits = (mask.cpu().view(n, h, w, c // V, 1) >> torch.arange(V, dtype=torch.uint8)) & 1
    return bits.view(n, h, w, c).bool()


@covers(*BN_ENTRIES)
@pytest.mark.parametrize('dtype,shape,layout', BN_RUNS, ids=ew_ids)
def test_batchnorm(env, dtype, shape, layout):
    """Train-mode BatchNorm forward and backward, every entry point of bn.hip, each tensor in its own slab and each parameter array between margins, against the fp64
    formulas on the same values. fp32 bars are test_batchnorm_train's (statistics and y 1e-5, sums 2e-5, dx 5e-5, masked gradients exact, the mask sources bit-equal);
    bf16 bars are test_act16_batchnorm's (statistics 1e-6 / 1e-5, outputs one rounding, dx two, sums within the slack of the units within 1e-2 of the ReLU edge,
    masked gradients exact off that edge). The stem trio (fp32) is bit-equal to the separate kernels, as the header says."""
    L, lib = env
    n, h, w, ch = shape
    P, V, f32 = n * h * w, 4 if dtype == F32 else 8, dtype == F32
    x, res, dy, r2 = data(shape, dtype, 1, 2.0, 0.5), data(shape, dtype, 2), data(shape, dtype, 3), data(shape, dtype, 8, 0.7, -0.2)
    gamma, beta = rnd(ch, seed=4) * 0.2 + 1.0, rnd(ch, seed=5) * 0.1
    eps, mom = 1e-5, 0.1
    xd64 = x.double()
    m_ref, v_ref = xd64.mean((0, 1, 2)), xd64.var((0, 1, 2), unbiased=False)

    def call(entry):
        return Call(env, entry, layout)

    def params(c, *ts):
        return [c.flat(t.numel(), F32, 'in', t).data_ptr() for t in ts]

    def ws_for(c, xd):
        need = lib.pm_bn_workspace(xd)
        return c.workspace(need), need

    # statistics
    c = call('pm_bn_stats')
    _, xd = c.tensor(shape, dtype, 'in', x)
    moments = c.flat(3 * ch, F32, 'out')
    assert c.run(xd, moments.data_ptr(), *ws_for(c, xd))
    assert rel(moments[:ch], m_ref) < (1e-5 if f32 else 1e-6) and rel(moments[ch:2 * ch], v_ref * P) < 1e-5 and bool((moments[2 * ch:] == P).all())
    c = call('pm_bn_stats_finalize')
    _, xd = c.tensor(shape, dtype, 'in', x)
    mean, invstd = c.flat(ch, F32, 'out'), c.flat(ch, F32, 'out')
    rm0, rv0 = rnd(ch, seed=6), rnd(ch, seed=7).abs() + 0.5
    rm, rv = c.flat(ch, F32, 'inout', rm0), c.flat(ch, F32, 'inout', rv0)
    assert c.run(xd, eps, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), mom, *ws_for(c, xd))
    assert rel(mean, m_ref) < (1e-5 if f32 else 1e-6) and rel(invstd, 1.0 / torch.sqrt(v_ref + eps)) < 1e-5
    assert rel(rm, 0.9 * rm0.double() + 0.1 * m_ref) < 1e-5 and rel(rv, 0.9 * rv0.double() + 0.1 * v_ref * P / (P - 1)) < 1e-5
    mu, isd = mean.cpu(), invstd.cpu()
    aff = (xd64 - mu.double()) * isd.double() * gamma.double() + beta.double()      # fp64 formula on the kernel's own (fp32) statistics
    pre = aff + res.double()
    xhat = (xd64 - mu.double()) * isd.double()
    # bf16 only: units whose sign the two evaluations may see differently (test_act16_batchnorm excludes the union of the two everywhere; here each mask source
    # excludes its own pre-activation alone, which is stricter and stays under 1 % of the tensor at these shapes)
    none = torch.zeros(shape, dtype=torch.bool)
    edge_aff, edge_pre = (none, none) if f32 else (aff.abs() < 1e-2, pre.abs() < 1e-2)
    assert edge_aff.float().mean().item() < 0.01 and edge_pre.float().mean().item() < 0.01

    def out_close(got, want, ulps=1.0, bar=1e-5):
        scale_close(got, want, bar) if f32 else close16(cpu(got), want.float(), ulps=ulps)

    # forward: plain, ReLU, residual + ReLU with the mask bytes, residual = BatchNorm of a second raw tensor
    fwd = {}
    for has_res, relu, want_mask in ((False, 0, False), (False, 1, False), (True, 1, True)):
        c = call('pm_bn_apply_mask' if want_mask else 'pm_bn_apply')
        _, xd = c.tensor(shape, dtype, 'in', x)
        rd = c.tensor(shape, dtype, 'in', res)[1] if has_res else None
        y, yd = c.tensor(shape, dtype, 'out')
        mask = c.flat(P * ch // V, torch.uint8, 'out') if want_mask else None
        args = [xd] + params(c, mu, isd, gamma, beta) + [rd, relu, yd] + ([mask.data_ptr()] if want_mask else [])
        assert c.run(*args)
        want = pre if has_res else aff
        out_close(y, want.clamp_min(0) if relu else want)
        fwd[(has_res, relu)] = cpu(y)
        if want_mask:
            bits, ok = _unpack_mask(mask, shape, V), ~edge_pre
            assert torch.equal(bits[ok], (cpu(y) > 0)[ok] if f32 else (pre > 0)[ok])
            mask_bytes = mask.cpu()
    y1, y2 = fwd[(True, 1)], fwd[(False, 1)]
    if f32:
        c = call('pm_bn_apply_mask_affine')
        (_, xd), (_, rd) = c.tensor(shape, dtype, 'in', x), c.tensor(shape, dtype, 'in', r2)
        rp = [rnd(ch, seed=20) * 0.2 - 0.2, torch.rand(ch, generator=torch.Generator().manual_seed(21)) + 0.5, rnd(ch, seed=22) * 0.2 + 1.0, rnd(ch, seed=23) * 0.1]
        y, yd = c.tensor(shape, dtype, 'out')
        mask = c.flat(P * ch // V, torch.uint8, 'out')
        assert c.run(*([xd] + params(c, mu, isd, gamma, beta) + [rd] + params(c, *rp) + [1, yd, mask.data_ptr()]))
        pre_a = aff + (r2.double() - rp[0].double()) * rp[1].double() * rp[2].double() + rp[3].double()
        scale_close(y, pre_a.clamp_min(0), 1e-5)
        assert torch.equal(_unpack_mask(mask, shape, V), cpu(y) > 0)

    # backward reduce: no activation, mask from y (with a residual: y1; without: y2), mask rebuilt from x, mask bytes
    def sums_ref(keep):
        g = dy.double() * keep
        return torch.cat([g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))])

    def sums_close(got, keep, edge):
        ref_s = sums_ref(keep)
        if f32:
            assert rel(got[:ch], ref_s[:ch]) < 2e-5 and rel(got[ch:], ref_s[ch:]) < 2e-5
        else:
            slack = (dy.double().abs() * edge).sum((0, 1, 2))
            slack = torch.cat([slack, slack * xhat.abs().amax((0, 1, 2))]) + 1e-4 * ref_s.abs().max()
            assert bool(((got.cpu().double() - ref_s).abs() <= slack + 1e-5 * ref_s.abs()).all())

    sums, gms = {}, {}
    from_x = y2 > 0 if f32 else aff > 0      # fp32: the rebuilt mask is the one of the stored output, bit for bit
    for tag, mode, yfwd, want_g, keep, edge in (('none', 0, None, False, ~none, none), ('y1', 1, y1, True, y1 > 0, none), ('y2', 1, y2, False, y2 > 0, none),
                                                ('x', 2, None, False, from_x, edge_aff), ('x+g', 2, None, True, from_x, edge_aff),
                                                ('bytes', 3, None, True, y1 > 0 if f32 else pre > 0, edge_pre)):
        c = call('pm_bn_bwd_reduce_mask' if mode == 3 else 'pm_bn_bwd_reduce')
        _, dyd = c.tensor(shape, dtype, 'in', dy)
        yd = c.tensor(shape, dtype, 'in', yfwd)[1] if yfwd is not None else None
        _, xd = c.tensor(shape, dtype, 'in', x)
        gm, gd = c.tensor(shape, dtype, 'out') if want_g else (None, None)
        s = c.flat(2 * ch, F32, 'out')
        if mode == 3:
            mb = c.flat(mask_bytes.numel(), torch.uint8, 'in', mask_bytes)
            assert c.run(*([dyd, mb.data_ptr(), xd] + params(c, mu, isd) + [gd, s.data_ptr(), *ws_for(c, xd)]))
        else:
            assert c.run(*([dyd, yd, xd] + params(c, mu, isd, gamma, beta) + [mode, gd, s.data_ptr(), *ws_for(c, xd)]))
        sums_close(s, keep, edge)
        sums[tag] = s.clone()
        if want_g:
            ok = ~edge
            assert torch.equal(cpu(gm)[ok], (dy * keep)[ok]), tag
            gms[tag] = cpu(gm)
    if f32:      # the mask sources agree to the bit (test_batchnorm_train)
        assert torch.equal(sums['x'], sums['y2']) and torch.equal(sums['x+g'], sums['x']) and torch.equal(sums['bytes'], sums['y1']) and torch.equal(gms['bytes'], gms['y1'])

    # backward apply: dx = gamma invstd (g - s1 / n - xhat s2 / n) on the kernel's own sums
    def dx_ref(g, s):
        s = s.cpu().double()
        return (g.double() - s[:ch] / P - xhat * s[ch:] / P) * (isd.double() * gamma.double())

    dxs = {}
    for tag, mode, yfwd, want_dres, s, g in (('none', 0, None, False, sums['none'], dy), ('y1', 1, y1, True, sums['y1'], dy * (y1 > 0)), ('gm', 0, None, False, sums['y1'], dy * (y1 > 0)),
                                             ('x', 2, None, False, sums['x'], None)):
        c = call('pm_bn_bwd_apply')
        _, dyd = c.tensor(shape, dtype, 'in', gms['y1'] if tag == 'gm' else dy)
        yd = c.tensor(shape, dtype, 'in', yfwd)[1] if yfwd is not None else None
        _, xd = c.tensor(shape, dtype, 'in', x)
        dx, dxd = c.tensor(shape, dtype, 'out')
        dres, drd = c.tensor(shape, dtype, 'out') if want_dres else (None, None)
        assert c.run(*([dyd, yd, xd] + params(c, mu, isd, gamma, beta, s) + [float(P), mode, dxd, drd]))
        if g is not None and (f32 or tag == 'none'):
            out_close(dx, dx_ref(g, s), ulps=2.0, bar=5e-5)
        if want_dres:
            assert torch.equal(cpu(dres), dy * (y1 > 0))
        dxs[tag] = cpu(dx)
    if f32:
        assert torch.equal(dxs['gm'], dxs['y1'])
        c = call('pm_bn_bwd_apply_mask')      # bit-identical to pm_bn_bwd_apply on the stored masked gradient
        (_, dyd), (_, xd) = c.tensor(shape, dtype, 'in', dy), c.tensor(shape, dtype, 'in', x)
        mb = c.flat(mask_bytes.numel(), torch.uint8, 'in', mask_bytes)
        dx, dxd = c.tensor(shape, dtype, 'out')
        assert c.run(*([dyd, mb.data_ptr(), xd] + params(c, mu, isd, gamma, sums['bytes']) + [float(P), dxd]))
        assert torch.equal(cpu(dx), dxs['gm'])

        # the stem: pool of relu(bn(x)) and the backward that gathers its gradient from the pooled one == the separate kernels, bit for bit
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        pshape = (n, ho, wo, ch)
        c = call('pm_maxpool3x3s2_bn_relu_fwd')
        _, xd = c.tensor(shape, dtype, 'in', x)
        yp, ypd = c.tensor(pshape, dtype, 'out')
        arg = c.flat(n * ho * wo * ch, torch.uint8, 'out')
        assert c.run(*([xd] + params(c, mu, isd, gamma, beta) + [ypd, arg.data_ptr()]))
        c = call('pm_maxpool3x3s2_fwd')
        _, ad = c.tensor(shape, dtype, 'in', y2)
        yq, yqd = c.tensor(pshape, dtype, 'out')
        arg2 = c.flat(arg.numel(), torch.uint8, 'out')
        assert c.run(ad, yqd, arg2.data_ptr())
        assert torch.equal(cpu(yp), cpu(yq)) and torch.equal(arg, arg2)
        scale_close(yp, F.max_pool2d(aff.clamp_min(0).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1), 1e-5)
        dyp = rnd(*pshape, seed=9)
        c = call('pm_maxpool3x3s2_bwd')
        _, dpd = c.tensor(pshape, dtype, 'in', dyp)
        full, fd = c.tensor(shape, dtype, 'out')
        assert c.run(dpd, c.flat(arg.numel(), torch.uint8, 'in', arg).data_ptr(), fd)
        dy_full = cpu(full)
        sep = {}
        for entry in ('pm_bn_bwd_reduce', 'pm_bn_bwd_reduce_pool'):
            c = call(entry)
            pool = entry.endswith('pool')
            _, dyd = c.tensor(pshape, dtype, 'in', dyp) if pool else c.tensor(shape, dtype, 'in', dy_full)
            _, xd = c.tensor(shape, dtype, 'in', x)
            s = c.flat(2 * ch, F32, 'out')
            if pool:
                assert c.run(*([dyd, c.flat(arg.numel(), torch.uint8, 'in', arg).data_ptr(), xd] + params(c, mu, isd, gamma, beta) + [s.data_ptr(), *ws_for(c, xd)]))
            else:
                assert c.run(*([dyd, None, xd] + params(c, mu, isd, gamma, beta) + [2, None, s.data_ptr(), *ws_for(c, xd)]))
            sep[entry] = s.clone()
        assert torch.equal(sep['pm_bn_bwd_reduce'], sep['pm_bn_bwd_reduce_pool'])
        g = dy_full.double() * (aff > 0)
        ref_s = torch.cat([g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))])
        assert rel(sep['pm_bn_bwd_reduce_pool'][:ch], ref_s[:ch]) < 2e-5 and rel(sep['pm_bn_bwd_reduce_pool'][ch:], ref_s[ch:]) < 2e-5
        for entry in ('pm_bn_bwd_apply', 'pm_bn_bwd_apply_pool'):
            c = call(entry)
            pool = entry.endswith('pool')
            _, dyd = c.tensor(pshape, dtype, 'in', dyp) if pool else c.tensor(shape, dtype, 'in', dy_full)
            _, xd = c.tensor(shape, dtype, 'in', x)
            dx, dxd = c.tensor(shape, dtype, 'out')
            s = sep['pm_bn_bwd_reduce_pool']
            if pool:
                assert c.run(*([dyd, c.flat(arg.numel(), torch.uint8, 'in', arg).data_ptr(), xd] + params(c, mu, isd, gamma, beta, s) + [float(P), dxd]))
            else:
                assert c.run(*([dyd, None, xd] + params(c, mu, isd, gamma, beta, s) + [float(P), 2, dxd, None]))
            sep[entry] = cpu(dx)
        assert torch.equal(sep['pm_bn_bwd_apply'], sep['pm_bn_bwd_apply_pool'])
        scale_close(sep['pm_bn_bwd_apply_pool'], dx_ref(g, s), 5e-5)


def test_batchnorm_turns_down_views_that_are_no_16_byte_vectors(env):
    """bn.hip under the odd layout: every entry point starts with pm_elem<T>::check on each tensor and has no scalar form, so each call is refused with PM_EINVAL
    before any launch -- nothing written, a message left."""
    L, lib = env
    shape, pshape, ch = (2, 5, 7, 8), (2, 3, 4, 8), 8
    x = rnd(*shape, seed=1)
    for entry in BN_ENTRIES:
        c = Call(env, entry, 'odd')
        t = lambda role='in', s=shape: c.tensor(s, F32, role, rnd(*s, seed=2) if role == 'in' else None)[1]
        p = lambda k=ch: c.flat(k, F32, 'in', rnd(k, seed=3).abs() + 0.5).data_ptr()
        o = lambda k: c.flat(k, F32, 'out').data_ptr()
        b = lambda k: c.flat(k, torch.uint8, 'in', torch.zeros(k, dtype=torch.uint8)).data_ptr()
        ws = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device='cuda')
        W = (ws.data_ptr(), ws.numel())
        args = {
            'pm_bn_stats': lambda: (t(), o(3 * ch), *W),
            'pm_bn_stats_finalize': lambda: (t(), 1e-5, o(ch), o(ch), None, None, 0.1, *W),
            'pm_bn_apply': lambda: (t(), p(), p(), p(), p(), None, 1, t('out')),
            'pm_bn_apply_mask': lambda: (t(), p(), p(), p(), p(), t(), 1, t('out'), o(70)),
            'pm_bn_apply_mask_affine': lambda: (t(), p(), p(), p(), p(), t(), p(), p(), p(), p(), 1, t('out'), o(70)),
            'pm_bn_bwd_reduce': lambda: (t(), t(), t(), p(), p(), p(), p(), 1, t('out'), o(2 * ch), *W),
            'pm_bn_bwd_reduce_mask': lambda: (t(), b(140), t(), p(), p(), t('out'), o(2 * ch), *W),
            'pm_bn_bwd_apply': lambda: (t(), t(), t(), p(), p(), p(), p(), p(2 * ch), 70.0, 1, t('out'), t('out')),
            'pm_bn_bwd_apply_mask': lambda: (t(), b(140), t(), p(), p(), p(), p(2 * ch), 70.0, t('out')),
            'pm_maxpool3x3s2_bn_relu_fwd': lambda: (t(), p(), p(), p(), p(), t('out', pshape), c.flat(192, torch.uint8, 'out').data_ptr()),
            'pm_bn_bwd_reduce_pool': lambda: (t('in', pshape), b(192), t(), p(), p(), p(), p(), o(2 * ch), *W),
            'pm_bn_bwd_apply_pool': lambda: (t('in', pshape), b(192), t(), p(), p(), p(), p(), p(2 * ch), 70.0, t('out')),
        }[entry]()
        assert not c.run(*args)
        assert bool((ws == 0xA5).all())


# ---- loss.hip -------------------------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [((2, 5, 7, 19), (33, 29), 2.0), ((2, 10, 70, 19), (25, 200), 0.5)]      # the flat forward + interval field; the interval form of the training forward
LOSS_ENTRIES = ('pm_upsample_ce_fwd', 'pm_upsample_ce_bwd', 'pm_upsample_ce_fwd_field', 'pm_upsample_ce_bwd_field', 'pm_upsample_wce_fwd', 'pm_upsample_wce_fwd_field',
                'pm_upsample_wce_bwd_field', 'pm_upsample_eval')
_LOSS_REFS = {}


def _loss_refs(shape, HW, temp):
    """Inputs and the torch compositions of one shape, computed once and never written: fp32 loss and fp64 gradient (upstream scale 1.7) as test_upsample_ce and
    test_upsample_wce take them, ATen's fp32 argmax with its top-2 margin as test_upsample_eval_against_aten_fp32 does."""
    from test_validate import MARGIN, ref_hist
    from test_weighted_loss import compose, ref_weight_rows
    key = (shape, HW, temp)
    if key not in _LOSS_REFS:
        n, h, w, C = shape
        lg = rnd(n, C, h, w, seed=1) * 3
        g = torch.Generator().manual_seed(2)
        lab = torch.randint(0, C, (n, *HW), generator=g)
        lab[torch.rand(n, *HW, generator=g) < 0.1] = 255
        lab[:, :2] = 255
        vec, rows = torch.rand(C, generator=torch.Generator().manual_seed(4)) + 0.5, ref_weight_rows(lab, C)
        up = lambda t, tt: F.interpolate(t / tt, size=HW, mode='bilinear', align_corners=True)
        r = dict(lg=lg, lab=lab, w_vec=vec, w_rows=rows)
        for tag, wt, per_image in (('ce', None, False), ('vec', vec, False), ('rows', rows, True)):
            lr = lg.double().requires_grad_(True)
            f = (lambda u, dt: F.cross_entropy(u, lab, ignore_index=255)) if wt is None else (lambda u, dt: compose(u, lab, wt.to(dt), per_image))
            (f(up(lr, temp), torch.float64) * 1.7).backward()
            full = wt if wt is None or wt.dim() == 2 else wt.expand(n, -1)
            r[tag] = dict(loss=f(up(lg, temp), torch.float32).item(), grad=lr.grad.permute(0, 2, 3, 1),
                          sums=None if wt is None else torch.stack([full[b].double()[lab[b][lab[b] != 255]].sum() for b in range(n)]))
        u1 = up(lg, 1.0)
        top = u1.topk(2, dim=1)
        r['eval'] = dict(loss=F.cross_entropy(u1, lab, ignore_index=255).item(), arg=u1.argmax(1), top2=top.indices, safe=(top.values[:, 0] - top.values[:, 1]) >= MARGIN,
                         hist=ref_hist(u1.argmax(1), lab, C))
        _LOSS_REFS[key] = r
    return _LOSS_REFS[key]


@covers(*LOSS_ENTRIES)
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd', 'ownpad'])
@pytest.mark.parametrize('shape,HW,temp', LOSS_SHAPES, ids=ew_ids)
def test_upsample_losses(env, shape, HW, temp, layout):
    """The fused up-sample + cross-entropy family with the 19-class logits and their gradient as views (the network's own pitch-20 layout among them; loss.hip reads
    and writes element by element, so the odd layout is served too), labels with 255s between margins of a valid class, loss_out / field / hist / pred between margins,
    exact workspaces. Bars of test_upsample_ce / test_upsample_wce (loss 2e-6, gradient 2e-5 of the largest entry against fp64, weight sums 1e-6) and of
    test_upsample_eval_against_aten_fp32 (prediction exact above the reference's top-2 margin, one of its top two below; the histogram is fast_hist of the kernel's map)."""
    from test_validate import SHARE_CAP, ref_hist
    L, lib = env
    n, h, w, C = shape
    H, W = HW
    R = _loss_refs(shape, HW, temp)
    lg, lab = R['lg'].permute(0, 2, 3, 1), R['lab']
    it = 1.0 / temp

    def start(entry):
        c = Call(env, entry, layout)
        _, ld = c.tensor(shape, F32, 'in', lg)
        return c, ld, c.flat(lab.numel(), torch.int64, 'in', lab).data_ptr()

    def loss_close(got, want):
        assert abs(got - want) < 2e-6 * max(1, abs(want)), (got, want)

    gs = torch.tensor([1.7])
    # unweighted: forward, backward that rebuilds the field, training forward + row pass
    c, ld, lb = start('pm_upsample_ce_fwd')
    out = c.flat(2, F32, 'out')
    need = lib.pm_upsample_ce_workspace(n, H, W)
    assert c.run(ld, it, lb, H, W, out.data_ptr(), c.workspace(need), need)
    loss_close(out[0].item(), R['ce']['loss'])
    assert out[1].item() == (lab != 255).sum().item()
    loss_out = out.cpu()
    c, ld, lb = start('pm_upsample_ce_bwd')
    dl, dd = c.tensor(shape, F32, 'out')
    need = lib.pm_upsample_ce_bwd_workspace(ld, H, W)
    assert c.run(ld, it, lb, H, W, c.flat(2, F32, 'in', loss_out).data_ptr(), c.flat(1, F32, 'in', gs).data_ptr(), dd, c.workspace(need), need)
    scale_close(dl, R['ce']['grad'], 2e-5)
    dl0 = cpu(dl)
    nfield = lib.pm_upsample_ce_field_bytes(ld, H, W) // 4
    assert nfield > 0
    for tag, wt, stride, per_image in (('ce', None, 0, 0), ('vec', R['w_vec'], 0, 0), ('rows', R['w_rows'], C, 1)):
        weighted = wt is not None
        nout = 2 + n if weighted else 2
        c, ld, lb = start('pm_upsample_wce_fwd_field' if weighted else 'pm_upsample_ce_fwd_field')
        out, field = c.flat(nout, F32, 'out'), c.flat(nfield, F32, 'out')
        need = (lib.pm_upsample_wce_workspace if weighted else lib.pm_upsample_ce_workspace)(n, H, W)
        wargs = [c.flat(wt.numel(), F32, 'in', wt).data_ptr(), stride, per_image] if weighted else []
        assert c.run(*([ld, it, lb, H, W] + wargs + [out.data_ptr(), field.data_ptr(), c.workspace(need), need]))
        loss_close(out[0].item(), R[tag]['loss'])
        got = out.cpu().double()
        if weighted:
            sums = R[tag]['sums']
            assert abs(got[1].item() - sums.sum().item()) <= 1e-6 * sums.sum().item()
            assert all(abs(got[2 + b].item() - sums[b].item()) <= 1e-6 * sums[b].item() for b in range(n))
        else:
            assert got[1].item() == (lab != 255).sum().item()
        c2 = Call(env, 'pm_upsample_wce_bwd_field' if weighted else 'pm_upsample_ce_bwd_field', layout)
        _, ld2 = c2.tensor(shape, F32, 'in', lg)
        dl, dd = c2.tensor(shape, F32, 'out')
        tail = [c2.flat(nout, F32, 'in', out).data_ptr(), c2.flat(1, F32, 'in', gs).data_ptr(), c2.flat(nfield, F32, 'in', field).data_ptr(), dd]
        assert c2.run(*([ld2, it, H, W] + ([per_image] if weighted else []) + tail))
        scale_close(dl, R[tag]['grad'], 2e-5)
        if not weighted:
            scale_close(dl, dl0, 1e-5)
        if weighted:      # eval form: no field
            c, ld, lb = start('pm_upsample_wce_fwd')
            out_e = c.flat(nout, F32, 'out')
            assert c.run(ld, it, lb, H, W, c.flat(wt.numel(), F32, 'in', wt).data_ptr(), stride, per_image, out_e.data_ptr(), c.workspace(need), need)
            loss_close(out_e[0].item(), R[tag]['loss'])
            assert all(abs(out_e[i].item() - out[i].item()) <= 1e-6 * abs(out[i].item()) for i in range(nout))
    # validation sweep, overwriting and then accumulating into the same histogram
    E = R['eval']
    assert 1.0 - E['safe'].float().mean().item() <= SHARE_CAP
    c0 = Call(env, 'pm_upsample_eval', layout)
    hist = c0.flat(C * C, torch.int64, 'out')
    for acc in (0, 1):
        c, ld, lb = start('pm_upsample_eval')
        c.bufs.append(c0.bufs[0])
        out, pred = c.flat(2, F32, 'out'), c.flat(n * H * W, torch.uint8, 'out')
        need = lib.pm_upsample_eval_workspace(ld, H, W)
        assert need > 0
        assert c.run(ld, 1.0, lb, H, W, out.data_ptr(), hist.data_ptr(), acc, pred.data_ptr(), c.workspace(need), need)
        loss_close(out[0].item(), E['loss'])
        assert out[1].item() == (lab != 255).sum().item()
        p, safe = pred.cpu().long().view(n, H, W), E['safe']
        assert torch.equal(p[safe], E['arg'][safe]) and bool(((p == E['top2'][:, 0]) | (p == E['top2'][:, 1]))[~safe].all())
        own = ref_hist(p, lab, C)
        assert torch.equal(hist.cpu().view(C, C), (1 + acc) * own)
        countable = (lab >= 0) & (lab < C)
        assert (own - E['hist']).abs().sum().item() <= 2 * int((~safe & countable).sum())


# ---- memory.hip -----------------------------------------------------------------------------------------------------------------------------------------------
MEM_TENSOR_ENTRIES = ('pm_mem_read_fwd', 'pm_mem_read_fwd_pq', 'pm_mem_read_bwd', 'pm_mem_write_accum', 'pm_mem_write_accum_bwd')
# memory.hip: each of these asks pm_vec_ok() of every tensor before it launches (the rows are read and written 16 bytes at a time) -> PM_EUNSUPPORTED
REFUSES.update({(e, 'odd'): EUNSUPPORTED for e in MEM_TENSOR_ENTRIES})
D = 256


def _gumbel(rows, m, seed):
    return -torch.empty(rows, m).exponential_(generator=torch.Generator().manual_seed(seed)).log()


@covers('pm_mem_read_fwd', 'pm_mem_read_fwd_pq', 'pm_mem_colsoftmax', 'pm_mem_read_bwd')
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd'])
@pytest.mark.parametrize('noisy', [False, True], ids=['plain', 'gumbel'])
@pytest.mark.parametrize('m', [19, 7])
def test_memory_read(env, m, noisy, layout):
    """(2, 9, 7, 256) = 126 rows: three full 32-row tiles and a ragged one of 30, whose missing rows the kernels mask by multiplication -- behind x, dqr and the flat
    score / noise arrays lies poison here. x, qr, dqr, dx as views; score, p_mem, p_query, the two noise draws, dsx, mem, dmem between margins. Against the fp64
    formulation of test_memory_read at its bars (forward and softmaxes 2e-6, gradients 2e-5, p_query columns sum to 1 within 1e-5); the one all-zero row (the eps
    clamp: torch takes another sub-gradient there) is left out of the dx comparison, 1 row of 126."""
    L, lib = env
    n, h, w = 2, 9, 7
    rows = n * h * w
    x = torch.relu(rnd(n, h, w, D, seed=1))
    x[0, 0, 0, :] = 0
    mem = F.normalize(rnd(m, D, seed=2), dim=1)
    noise, noise_q = (_gumbel(rows, m, 5), _gumbel(rows, m, 7)) if noisy else (None, None)
    dqr, dsx = rnd(n, h, w, 2 * D, seed=3), rnd(rows, m, seed=4) * 0.1
    xr, mr = x.double().requires_grad_(True), mem.double().requires_grad_(True)
    q = F.normalize(xr, dim=3).view(rows, D)
    s = torch.matmul(q, mr.t())
    pm_ref = F.softmax(s + (noise.double() if noisy else 0.0), 1)
    pq_ref = F.softmax(s.detach() + (noise_q.double() if noisy else 0.0), 0)
    qr_ref = torch.cat((q, torch.matmul(pm_ref, mr)), 1)
    ((qr_ref * dqr.double().view(rows, 2 * D)).sum() + (s * dsx.double()).sum()).backward()

    def fwd(entry):
        c = Call(env, entry, layout)
        _, xd = c.tensor((n, h, w, D), F32, 'in', x)
        memg = c.flat(m * D, F32, 'in', mem)
        nz = c.flat(rows * m, F32, 'in', noise).data_ptr() if noisy else None
        qr, qd = c.tensor((n, h, w, 2 * D), F32, 'out')
        score, pmem = c.flat(rows * m, F32, 'out'), c.flat(rows * m, F32, 'out')
        return c, xd, memg, nz, qr, qd, score, pmem

    c, xd, memg, nz, qr, qd, score, pmem = fwd('pm_mem_read_fwd')
    if not c.run(xd, memg.data_ptr(), m, nz, qd, score.data_ptr(), pmem.data_ptr()):
        layout_refused = True
    else:
        layout_refused = False
        scale_close(qr.reshape(rows, 2 * D), qr_ref.detach(), 2e-6), scale_close(score.view(rows, m), s.detach(), 2e-6), scale_close(pmem.view(rows, m), pm_ref.detach(), 2e-6)
    first = (cpu(qr), score.cpu(), pmem.cpu())
    c, xd, memg, nz, qr, qd, score, pmem = fwd('pm_mem_read_fwd_pq')
    nq = c.flat(rows * m, F32, 'in', noise_q).data_ptr() if noisy else None
    pq = c.flat(rows * m, F32, 'out')
    need = lib.pm_mem_read_fwd_pq_workspace(rows, m)
    if c.run(xd, memg.data_ptr(), m, nz, nq, qd, score.data_ptr(), pmem.data_ptr(), pq.data_ptr(), c.workspace(need), need):
        assert torch.equal(cpu(qr), first[0]) and torch.equal(score.cpu(), first[1]) and torch.equal(pmem.cpu(), first[2])      # the same bits as the plain read
        scale_close(pq.view(rows, m), pq_ref, 2e-6)
        assert (pq.view(rows, m).double().sum(0) - 1).abs().max().item() < 1e-5
    if layout_refused:
        score_in, pmem_in = s.detach().float(), pm_ref.detach().float()
    else:
        score_in, pmem_in = first[1], first[2]
    if layout != 'odd':      # flat arrays only: nothing a layout changes
        c = Call(env, 'pm_mem_colsoftmax', layout)
        sc = c.flat(rows * m, F32, 'in', score_in)
        nq = c.flat(rows * m, F32, 'in', noise_q).data_ptr() if noisy else None
        pq = c.flat(rows * m, F32, 'out')
        need = lib.pm_mem_colsoftmax_workspace(rows, m)
        assert c.run(sc.data_ptr(), nq, rows, m, pq.data_ptr(), c.workspace(need), need)
        scale_close(pq.view(rows, m), pq_ref, 2e-6)
    live = torch.ones(n, h, w, dtype=torch.bool)
    live[0, 0, 0] = False
    both = []
    for want_dmem in (True, False):      # the row kernel that also reduces dmem; the MFMA kernel for dx alone
        c = Call(env, 'pm_mem_read_bwd', layout)
        _, xd = c.tensor((n, h, w, D), F32, 'in', x)
        memg, pg = c.flat(m * D, F32, 'in', mem), c.flat(rows * m, F32, 'in', pmem_in)
        _, dqd = c.tensor((n, h, w, 2 * D), F32, 'in', dqr)
        dsg = c.flat(rows * m, F32, 'in', dsx)
        dx, dxd = c.tensor((n, h, w, D), F32, 'out')
        dmem = c.flat(m * D, F32, 'out') if want_dmem else None
        need = lib.pm_mem_read_bwd_workspace(rows, m, D) if want_dmem else 0
        if c.run(xd, memg.data_ptr(), m, pg.data_ptr(), dqd, dsg.data_ptr(), dxd, dmem.data_ptr() if want_dmem else None, c.workspace(need), need):
            scale_close(cpu(dx)[live], xr.grad[live], 2e-5)
            if want_dmem:
                scale_close(dmem.view(m, D), mr.grad, 2e-5)
            both.append(cpu(dx))
    if both:
        scale_close(both[1], both[0], 1e-5)      # the all-zero row included: scaled by 1 / eps in both kernels


@covers('pm_mem_write_accum', 'pm_mem_write_accum_bwd')
@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd'])
@pytest.mark.parametrize('normalize', [1, 0])
@pytest.mark.parametrize('m', [6, 19])
def test_memory_write_accum(env, m, normalize, layout):
    """z (1, 9, 7, 256) as a view -- one ragged chunk of 63 rows --, labels (30, 20) between margins, m = 6 (a partial slab that is not 16-byte sized) and 19. Against
    the one-hot -> F.interpolate -> matmul formulation in fp64: nominator and denominator at 3e-6 (test_memory_write_accum_on_the_matrix_cores, an all-zero row
    included), dz at 2e-5 (test_memory_write; on a z without the zero row, so that no element is left out)."""
    L, lib = env
    n, h, w, H, W = 1, 9, 7, 30, 20
    z = torch.relu(rnd(n, h, w, D, seed=21))
    zb = z.clone()
    z[0, 0, 0, :] = 0
    g = torch.Generator().manual_seed(22)
    lab = torch.randint(0, max(2, m - 3), (n, H, W), generator=g)
    lab[torch.rand(n, H, W, generator=g) < 0.1] = 255
    t = lab.clone()
    t[t == 255] = m
    y = F.interpolate(F.one_hot(t, m + 1).permute(0, 3, 1, 2).double(), [h, w], mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(n * h * w, m + 1)

    def nom_of(zz):
        zz = zz.view(n * h * w, D)
        return torch.matmul(y.t(), F.normalize(zz, dim=1) if normalize else zz)      # [m + 1][d]

    c = Call(env, 'pm_mem_write_accum', layout)
    _, zd = c.tensor((n, h, w, D), F32, 'in', z)
    lb = c.flat(lab.numel(), torch.int64, 'in', lab)
    nomden = c.flat((m + 1) * (D + 1), F32, 'out')
    need = lib.pm_mem_write_accum_workspace(zd, m)
    if c.run(zd, lb.data_ptr(), H, W, m, normalize, nomden.data_ptr(), c.workspace(need), need):
        scale_close(nomden[:(m + 1) * D].view(m + 1, D), nom_of(z.double()), 3e-6)
        scale_close(nomden[(m + 1) * D:], y.sum(0), 3e-6)
    dnom = rnd(m + 1, D, seed=23)
    zr = zb.double().requires_grad_(True)
    (nom_of(zr) * dnom.double()).sum().backward()
    c = Call(env, 'pm_mem_write_accum_bwd', layout)
    _, zd = c.tensor((n, h, w, D), F32, 'in', zb)
    lb, dn = c.flat(lab.numel(), torch.int64, 'in', lab), c.flat(dnom.numel(), F32, 'in', dnom)
    dz, dzd = c.tensor((n, h, w, D), F32, 'out')
    if c.run(zd, lb.data_ptr(), H, W, m, normalize, dn.data_ptr(), dzd):
        scale_close(dz, zr.grad, 2e-5)


@covers('pm_mem_write_update', 'pm_mem_write_update_bwd')
@pytest.mark.parametrize('m', [6, 19])
def test_memory_write_update(env, m):
    """Flat arrays between margins: U = den != 0 ? mu M + (1 - mu) nom / den : M, M' = U / |U| against fp64 at 2e-6, absent classes keep their slot (1e-6), and the
    backward into the nominator and the old memory against autograd at 2e-5 (test_memory_write)."""
    mu = 0.8
    mem = F.normalize(rnd(m, D, seed=3), dim=1)
    nom, den = rnd(m + 1, D, seed=31), torch.rand(m + 1, generator=torch.Generator().manual_seed(32)) * 20 + 1
    den[m - 2:m] = 0                                       # two absent classes
    nom[m - 2:m] = 0
    nomden = torch.cat([nom.reshape(-1), den])
    mr, nr = mem.double().requires_grad_(True), nom.double().requires_grad_(True)
    safe = torch.where(den[:m] != 0, den[:m], torch.ones(m)).double()[:, None]
    upd = torch.where((den[:m] != 0)[:, None], mu * mr + (1 - mu) * nr[:m] / safe, mr)
    new = F.normalize(upd, dim=1)
    dout = rnd(m, D, seed=4)
    (new * dout.double()).sum().backward()
    c = Call(env, 'pm_mem_write_update', 'dense')
    out, u = c.flat(m * D, F32, 'out'), c.flat(m * D, F32, 'out')
    assert c.run(c.flat(m * D, F32, 'in', mem).data_ptr(), c.flat(nomden.numel(), F32, 'in', nomden).data_ptr(), m, D, mu, out.data_ptr(), u.data_ptr())
    scale_close(out.view(m, D), new.detach(), 2e-6), scale_close(u.view(m, D), upd.detach(), 2e-6)
    scale_close(out.view(m, D)[m - 2:], mem[m - 2:], 1e-6)
    c = Call(env, 'pm_mem_write_update_bwd', 'dense')
    dnom, dmem = c.flat((m + 1) * D, F32, 'out'), c.flat(m * D, F32, 'out')
    assert c.run(c.flat(m * D, F32, 'in', u).data_ptr(), c.flat(nomden.numel(), F32, 'in', nomden).data_ptr(), m, D, mu, c.flat(m * D, F32, 'in', dout).data_ptr(),
                 dnom.data_ptr(), dmem.data_ptr())
    scale_close(dnom.view(m + 1, D), nr.grad, 2e-5), scale_close(dmem.view(m, D), mr.grad, 2e-5)


# ---- convolutions: every route of route_conv again, each tensor in its own slab ------------------------------------------------------------------------------
from test_hip_kernels import ROUTE_CASES      # noqa: E402

CONV_RUNS = [(name, 'slice') for name in ROUTE_CASES] + [('fwd-bf16-48ch-padded', 'ownpad+flag'), ('fwd-bf16-48ch-padded', 'ownpad')]


@covers('pm_conv_fwd', 'pm_conv_bwd_data', 'pm_conv_bwd_weight')
@pytest.mark.parametrize('name,layout', CONV_RUNS)
def test_conv_routes_on_views(env, name, layout):
    """ROUTE_CASES of test_conv_routes_stay_inside_the_workspace_they_ask_for with x / y (+ the epilogue's residual) of the forward, dy / dx (+ add) of the data gradient
    and x / dy of the weight gradient as channel slices inside poisoned slabs; weights, dw, db, the kept filter and the kept Winograd V between margins; the workspace
    exactly as large as the query answers, guard bytes behind it. The profiler's record still shows the route's kernel form and the result meets the route test's bars
    (fp32 2e-5 against fp64, dw 5e-5; bf16 tensors one-and-a-half roundings of the fp32 formula on the rounded operands, dw 2e-4). The 48-channel bf16 input also runs
    with zero pad lanes up to 64 inside its pitch: with PM_TF_ZERO_PAD64 it is gathered in place (no padded copy in the workspace), without the flag it is copied."""
    from pinthememory_amd.hip import kernels as K
    L, lib = env
    which, tier, (n, cin, h, w, cout, k, s, p, d), route, opt, (rec_mode, rec_prec) = ROUTE_CASES[name]
    xlay, flag = ('ownpad', L.PM_TF_ZERO_PAD64 if layout.endswith('flag') else 0) if layout.startswith('ownpad') else (layout, 0)
    lay = 'slice'
    r16 = (lambda t: t) if tier == 'f32' else (lambda t: t.bfloat16().float())
    xdt = F32 if tier in ('f32', 'stem', 'bf16_operands') else B16
    ydt = F32 if tier in ('f32', 'bf16_operands') else B16
    prec = 0 if tier == 'f32' else 2
    x = rnd(n, cin, h, w, seed=1) if tier in ('stem', 'bf16_operands') else r16(rnd(n, cin, h, w, seed=1))
    wt = rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    ref_t = torch.float64 if tier == 'f32' else torch.float32
    xr, wr = r16(x).to(ref_t).requires_grad_(True), (wt if which == 2 else r16(wt)).to(ref_t).requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=s, padding=p, dilation=d)
    dy = rnd(*y_ref.shape, seed=4)
    y_ref.backward(r16(dy).to(ref_t))
    ho, wo = y_ref.shape[2:]
    xs, ys = (n, h, w, cin), (n, ho, wo, cout)
    nhwc_ = lambda t: t.permute(0, 2, 3, 1)
    res = rnd(n, cout, ho, wo, seed=5).to(ydt).float()      # the epilogue's residual / the data gradient's add, already of the output's type
    add = rnd(n, cin, h, w, seed=6).to(xdt).float()
    dyv = r16(dy) if tier != 'bf16_operands' else dy
    before = K.routing(**route)
    c = Call(env, ('pm_conv_fwd', 'pm_conv_bwd_data', 'pm_conv_bwd_weight')[which], lay)
    try:
        wg = c.flat(wt.numel(), F32, 'in', wt.permute(0, 2, 3, 1))
        if which == 0:
            (xg, xd), (yg, yd) = c.tensor(xs, xdt, 'in', nhwc_(x), layout=xlay, flags=flag), c.tensor(ys, ydt, 'out')
            rg, _ = c.tensor(ys, ydt, 'in', nhwc_(res))
        elif which == 1:
            (xg, xd), (yg, yd) = c.tensor(xs, xdt, 'out'), c.tensor(ys, ydt, 'in', nhwc_(dyv))
            _, ad = c.tensor(xs, xdt, 'in', nhwc_(add))
        else:
            (xg, xd), (yg, yd) = c.tensor(xs, xdt, 'in', nhwc_(x)), c.tensor(ys, ydt, 'in', nhwc_(dyv))
        prm = L.conv_params(k, k, s, p, d, prec)
        nbv, nbu = lib.pm_conv_winograd_v_bytes(xd, yd, byref(prm)), lib.pm_conv_wxf_bytes(xd, yd, byref(prm))
        if which == 0 and nbu:      # the filter the forward derives from w, kept by the caller
            kept = c.flat(nbu, torch.uint8, 'out')
            prm.wxf, prm.wxf_bytes, prm.wxf_valid = kept.data_ptr(), nbu, 0
        if opt.get('keep_v'):       # the forward pass leaves its transformed input for the weight gradient
            cf = Call(env, 'pm_conv_fwd', lay)
            (_, xfd), (_, yfd) = cf.tensor(xs, xdt, 'in', nhwc_(x)), cf.tensor(ys, ydt, 'out')
            v = cf.flat(nbv // 4, F32, 'out')
            pf = L.conv_params(k, k, s, p, d, prec)
            pf.wino_v, pf.wino_v_bytes = v.data_ptr(), nbv
            nf = lib.pm_conv_workspace(xfd, yfd, byref(pf), 0)
            assert cf.run(xfd, cf.flat(wt.numel(), F32, 'in', wt.permute(0, 2, 3, 1)).data_ptr(), yfd, byref(pf), None, cf.workspace(nf), nf)
            cf.bufs[-2].role = 'in'
            c.bufs.append(cf.bufs[-2])
            prm.wino_v, prm.wino_v_bytes = v.data_ptr(), nbv
        need = lib.pm_conv_workspace(xd, yd, byref(prm), which)
        if which == 0 and tier == 'bf16':      # the padded copy of a narrow bf16 input lives in the workspace, behind the room for the filter
            copied = need - nbu >= (n * h * w * 64 * 2 + 255) // 256 * 256
            assert copied == (bool(opt.get('padded_copy')) and not flag), (need, nbu)
        K.profile_enable(True)
        K.profile_read(clear=True)
        if which == 0:
            ep = L.conv_epilogue(None, None, None, rg.data_ptr(), c.bufs[3].pitch, 0, None, 0)
            assert c.run(xd, wg.data_ptr(), yd, byref(prm), byref(ep), c.workspace(need), need)
        elif which == 1:
            assert c.run(yd, wg.data_ptr(), xd, byref(prm), ad, c.workspace(need), need)
        else:
            dw = c.flat(wt.numel(), F32, 'out')
            db = c.flat(cout, F32, 'out') if opt.get('dbias') else None
            assert c.run(xd, yd, dw.data_ptr(), db.data_ptr() if db is not None else None, byref(prm), c.workspace(need), need)
        K.profile_enable(False)
        assert K.profile_read(mode=rec_mode, prec=-1 if rec_prec is None else rec_prec)[2] > 0, 'no launch of the expected kernel form'
        if which != rec_mode and rec_mode != 4 and not opt.get('transposed'):
            assert K.profile_read(mode=which)[2] == 0
        if 'ring' in opt:
            assert any(K.profile_read(mode=2, bm=bm, bn=bn, km=2, nst=3, prec=4)[2] for bm, bn in ((256, 128), (128, 256))) == opt['ring']
        K.profile_read(clear=True)
    finally:
        K.profile_enable(False)
        K.routing(**before)
    if which == 0:
        want = nhwc_(y_ref.detach() + res.to(ref_t))
        close16(cpu(yg), want, ulps=1.5) if ydt == B16 else scale_close(yg, want, 2e-5)
    elif which == 1:
        want = nhwc_(xr.grad + add.to(ref_t))
        close16(cpu(xg), want, ulps=1.5) if xdt == B16 else scale_close(xg, want, 2e-5)
    else:
        scale_close(dw.view(cout, k, k, cin).permute(0, 3, 1, 2), wr.grad, 5e-5 if tier == 'f32' else 2e-4)
        if db is not None:
            scale_close(db, r16(dy).sum((0, 2, 3)), 2e-5)


@covers('pm_conv_bwd_data_masked')
@pytest.mark.parametrize('layout', ['dense', 'slice'])
def test_conv_bwd_data_masked_on_views(env, layout):
    """The stride-1 1x1 data gradient with a masked add, dx = dgrad(dy) + (bit ? add : 0): dy, dx and add as views, the ReLU bytes ([pixels][c / 4], bit e = element e)
    between margins. fp64 convolution gradient at the data-gradient bar, 2e-5; masked-out elements carry the convolution gradient alone."""
    L, lib = env
    n, cin, h, w, cout = 2, 64, 9, 7, 32
    wt, dy, add = rnd(cout, cin, 1, 1, seed=2, scale=(2.0 / cin) ** 0.5), rnd(n, cout, h, w, seed=4), rnd(n, cin, h, w, seed=6)
    xr = rnd(n, cin, h, w, seed=1).double().requires_grad_(True)
    F.conv2d(xr, wt.double()).backward(dy.double())
    bits = torch.rand(n, h, w, cin, generator=torch.Generator().manual_seed(7)) < 0.5
    mask = (bits.view(n * h * w, cin // 4, 4).to(torch.uint8) << torch.arange(4, dtype=torch.uint8)).sum(-1).to(torch.uint8)
    c = Call(env, 'pm_conv_bwd_data_masked', layout)
    (_, dyd), (dx, dxd) = c.tensor((n, h, w, cout), F32, 'in', dy.permute(0, 2, 3, 1)), c.tensor((n, h, w, cin), F32, 'out')
    _, ad = c.tensor((n, h, w, cin), F32, 'in', add.permute(0, 2, 3, 1))
    wg, mb = c.flat(wt.numel(), F32, 'in', wt.permute(0, 2, 3, 1)), c.flat(mask.numel(), torch.uint8, 'in', mask)
    prm = L.conv_params(1, 1, 1, 0, 1, 0)
    need = lib.pm_conv_workspace(dxd, dyd, byref(prm), 1)
    assert c.run(dyd, wg.data_ptr(), dxd, byref(prm), ad, mb.data_ptr(), c.workspace(need), need)
    scale_close(dx, xr.grad.permute(0, 2, 3, 1) + torch.where(bits, add.permute(0, 2, 3, 1).double(), torch.zeros(()).double()), 2e-5)
