"""GPU: the resampling input edge (csrc/resample.hip) against tests/golden/resample_cases.npz, the bytes PIL produces for the same images and geometry
(tools/make_resample_golden.py; test_resample_cpu.py regenerates them and holds the host tables to them). Image and label crops carry 0 differing bytes -- the
arithmetic is integer, the bar is derived, not measured -- whatever lies around the image in its slab; the edge entry points with a geometry equal the kernels
they chain, and without one their output of before."""
import numpy as np
import pytest
import torch

from pinthememory_amd import harness, input_edge
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

pytestmark = pytest.mark.gpu

CASES = ('sq', 'ns', 'pre', 'pad1', 'pad2', 'big', 'mixed', 'ramp')


@pytest.fixture(scope='module')
def fx(golden):
    with golden('resample_cases.npz') as f:
        return {k: f[k] for k in f.files}


def _batch(fx, name, poison=None, slab=None):
    """(images [n,Hs,Ws,3], labels [n,Hs,Ws], GeoParams) of a case: every image in the top-left corner of a slab as large as the largest (or `slab`), the rest of the
    slab filled with `poison` (None: zeros)."""
    src, geo = fx[name + '_src'], fx[name + '_geo']
    hs, ws = slab or (int(geo[:, 0].max()), int(geo[:, 1].max()))
    img = np.full((len(src), hs, ws, 3), poison or 0, dtype=np.uint8)
    lab = np.full((len(src), hs, ws), poison or 0, dtype=np.uint8)
    g = K.GeoParams(len(src), tuple(int(v) for v in fx[name + '_crop']))
    for i, k in enumerate(src):
        h, w = geo[i, :2]
        img[i, :h, :w], lab[i, :h, :w] = fx['src%d_img' % k], fx['src%d_lab' % k]
        p = g.images[i]
        p.h_in, p.w_in, p.h, p.w, p.pad_h, p.pad_w, p.y1, p.x1 = (int(v) for v in geo[i])
    return torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), g


@pytest.fixture(scope='module')
def device_out(fx):
    """(image crop, label crop) of every case, every image filling its slab (or, in `mixed`, its corner of it): computed once, shared, never modified."""
    out = {}
    for name in CASES:
        img, lab, g = _batch(fx, name)
        a, b = K.resample_crop_u8(img, lab, g)
        out[name] = (a.cpu(), b.cpu())
    return out


@pytest.mark.parametrize('name', CASES)
def test_crops_are_bit_equal_to_pil(fx, device_out, name):
    got, got_lab = (t.numpy() for t in device_out[name])
    want, want_lab = fx[name + '_img'], fx[name + '_lab']
    assert got.shape == want.shape and got_lab.shape == want_lab.shape and got.dtype == want.dtype == np.uint8
    for i in range(want.shape[0]):
        bad, bad_lab = int((got[i] != want[i]).sum()), int((got_lab[i] != want_lab[i]).sum())
        print('case %s image %d (scale %.4f): %d of %d image bytes, %d of %d label bytes differ from PIL' % (name, i, fx[name + '_scale'][i], bad, want[i].size, bad_lab,
                                                                                                              want_lab[i].size))
        assert bad == 0 and bad_lab == 0


def test_scale_one_without_pad_is_a_plain_slice_of_the_source(fx, device_out):
    hits = 0
    for name in ('sq', 'ns'):
        for i, row in enumerate(fx[name + '_geo']):
            if fx[name + '_scale'][i] == 1.0:
                k, (th, tw) = int(fx[name + '_src'][i]), fx[name + '_crop']
                assert tuple(row[:2]) == tuple(row[2:4]) and not row[4:6].any()
                sl = (slice(row[6], row[6] + th), slice(row[7], row[7] + tw))
                assert np.array_equal(device_out[name][0][i].numpy(), fx['src%d_img' % k][sl]) and np.array_equal(device_out[name][1][i].numpy(), fx['src%d_lab' % k][sl])
                hits += 1
    assert hits == 2


@pytest.mark.parametrize('name', ['mixed', 'pad2', 'big', 'sq'])
def test_nothing_outside_the_image_or_the_footprint_reaches_the_output(fx, device_out, name):
    """The slab around every image (19 rows and 23 columns wider than the largest) poisoned with 0x5a, then with 0xa5: both runs give the bytes of the clean run, which are
    PIL's. Then the source pixels outside the crop's own footprint are poisoned as well -- rows and columns the window's taps do not reach, from the tables -- and nothing changes."""
    geo = fx[name + '_geo']
    slab = (int(geo[:, 0].max()) + 19, int(geo[:, 1].max()) + 23)
    for poison in (0x5a, 0xa5):
        img, lab, g = _batch(fx, name, poison, slab)
        a, b = K.resample_crop_u8(img, lab, g)
        assert torch.equal(a.cpu(), device_out[name][0]) and torch.equal(b.cpu(), device_out[name][1]), poison
    crop = tuple(int(v) for v in fx[name + '_crop'])
    for poison in (0x5a, 0xa5):
        img, lab, g = _batch(fx, name, poison, slab)
        for i in range(len(g)):
            br, bc, nr, nc = (np.ctypeslib.as_array(t) for t in K.resample_tables(g.images[i], slab, crop))
            br, bc = br.reshape(crop[0], -1), bc.reshape(crop[1], -1)
            rows, cols = br[br[:, 1] > 0], bc[bc[:, 1] > 0]
            keep = torch.zeros(slab, dtype=torch.bool)
            if len(rows) and len(cols):
                keep[int(rows[:, 0].min()):int((rows[:, 0] + rows[:, 1]).max()), int(cols[:, 0].min()):int((cols[:, 0] + cols[:, 1]).max())] = True
            img[i][~keep.cuda()] = poison
            keep = torch.zeros(slab, dtype=torch.bool)
            if (nr >= 0).any() and (nc >= 0).any():
                keep[int(nr[nr >= 0].min()):int(nr.max()) + 1, int(nc[nc >= 0].min()):int(nc.max()) + 1] = True
            lab[i][~keep.cuda()] = poison
        a, b = K.resample_crop_u8(img, lab, g)
        assert torch.equal(a.cpu(), device_out[name][0]) and torch.equal(b.cpu(), device_out[name][1]), poison


def test_two_launches_give_identical_bytes_and_an_uploaded_geometry_serves_both(fx, device_out):
    img, lab, g = _batch(fx, 'big')
    gd = K.upload_geo(g, img.device, img.shape[1:3])
    for geo in (g, gd, gd):
        a, b = K.resample_crop_u8(img, lab, geo)
        assert torch.equal(a.cpu(), device_out['big'][0]) and torch.equal(b.cpu(), device_out['big'][1])
    img, lab, g = _batch(fx, 'pad2')
    other = K.GeoParams(len(g), g.crop, ignore_index=7)                                         # the pad label is the caller's
    for p, q in zip(other.images, g.images):
        ctypes_copy(p, q)
    b7 = K.resample_crop_u8(img, lab, other)[1].cpu()
    want = device_out['pad2'][1].clone()
    pad = torch.ones(want.shape, dtype=torch.bool)
    q = g.images[0]
    pad[0, max(q.pad_h - q.y1, 0):q.pad_h - q.y1 + q.h, max(q.pad_w - q.x1, 0):q.pad_w - q.x1 + q.w] = False
    assert pad.any() and (want[pad] == 255).all()
    want[pad] = 7
    assert torch.equal(b7, want)


def ctypes_copy(dst, src):
    for name, _ in src._fields_:
        setattr(dst, name, getattr(src, name))


class _Source:
    """A loader stand-in that yields the third item: images of two sizes in the corners of their slabs, and a centroid for every other image."""

    def __init__(self, batch, domains, slab, seed):
        self.inner = input_edge.SyntheticDomainSource(batch, domains, slab, seed=seed)
        self.bufs = self.inner.bufs
        n = batch * domains
        self.meta = dict(sizes=[(slab[0], slab[1]) if i % 2 else (slab[0] - 17, slab[1] - 30) for i in range(n)],
                         centroids=[(40 + i, 30 + i) if i % 2 else None for i in range(n)])

    def __iter__(self):
        return self

    def __next__(self):
        img, lab = next(self.inner)
        return img, lab, self.meta


def test_edge_with_geometry_is_the_chain_of_its_kernels_and_without_it_unchanged():
    """prepare_batch_u8(geometry=g, augment=a) == augment_u8 / labels_u8_to_i64 on resample_crop_u8's output; DevicePrefetcher(geometry=g) yields the same bytes for the
    same seeds, over three batches (slots and pinned buffers come round again); geometry=None yields what the edge yielded before."""
    B, D, slab, crop = 2, 2, (80, 120), (48, 72)
    pf = input_edge.DevicePrefetcher(_Source(B, D, slab, 7), augment=input_edge.PhotometricAugment(seed=5), hard_domains={1},
                                     geometry=input_edge.GeometricAugment(crop, seed=9))
    pg = input_edge.DevicePrefetcher(_Source(B, D, slab, 7), geometry=input_edge.GeometricAugment(crop, seed=9))
    plain = input_edge.DevicePrefetcher(_Source(B, D, slab, 7))
    src = _Source(B, D, slab, 7)
    g1, g2, g3 = (input_edge.GeometricAugment(crop, seed=9) for _ in range(3))
    a1, a2 = (input_edge.PhotometricAugment(seed=5) for _ in range(2))
    for _ in range(3):
        img, lab, meta = next(src)
        img, lab = img.clone(), lab.clone()
        x, gt = pf.next()
        wx, wgt = harness.prepare_batch_u8(img, lab, augment=a1, hard=[False, True] * B, geometry=g1, **meta)
        assert x.shape == (B * D, 4) + crop and gt.shape == (B * D,) + crop and torch.equal(x, wx) and torch.equal(gt, wgt)
        # the chain, spelled out
        geo = g2.sample(meta['sizes'], meta['centroids'])
        assert g2.last == g1.last
        ci, cl = K.resample_crop_u8(img.reshape(-1, *slab, 3).cuda(), lab.reshape(-1, *slab).cuda(), geo)
        params = K.upload_aug_params(a2.sample(B * D, [False, True] * B), ci.device)
        assert torch.equal(ops.nhwc(x), K.augment_u8(ci, params)) and torch.equal(gt, K.labels_u8_to_i64(cl, params))
        # geometry alone: the plain conversion of the crop
        x, gt = pg.next()
        wx, wgt = harness.prepare_batch_u8(img, lab, geometry=g3, **meta)
        assert torch.equal(x, wx) and torch.equal(gt, wgt) and torch.equal(ops.nhwc(x), K.image_u8_to_nhwc4(ci)) and torch.equal(gt, cl.long())
        # no geometry: bit-equal to the edge of before, third item or not
        px, pgt = plain.next()
        ox, ogt = harness.prepare_batch_u8(img, lab)
        assert torch.equal(px, ox) and torch.equal(pgt, ogt)
        assert torch.equal(ops.nhwc(ox), K.image_u8_to_nhwc4(img.reshape(-1, *slab, 3).cuda())) and torch.equal(ogt, lab.reshape(-1, *slab).cuda().long())
    torch.cuda.synchronize()
