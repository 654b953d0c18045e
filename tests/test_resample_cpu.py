"""CPU: the host side of the resampling input edge -- the coefficient tables of pm_resample_tables against PIL (through tests/golden/resample_cases.npz, written by
tools/make_resample_golden.py from PIL alone), argument validation in front of any device call, the tap cap, and the geometry sampler. No GPU here."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from pinthememory_amd import harness, input_edge
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC, PREC = L.RESAMPLE_REC, 22


def _tool():
    spec = importlib.util.spec_from_file_location('make_resample_golden', os.path.join(ROOT, 'tools', 'make_resample_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def geo_image(h_in, w_in, h, w, pad_h, pad_w, y1, x1):
    g = L.PmGeoImage()
    g.h_in, g.w_in, g.h, g.w, g.pad_h, g.pad_w, g.y1, g.x1 = (int(v) for v in (h_in, w_in, h, w, pad_h, pad_w, y1, x1))
    return g


def tables(g, slab, crop):
    """The library's four tables as numpy arrays: bicubic [t][REC] per axis, nearest [t] per axis."""
    br, bc, nr, nc = (np.ctypeslib.as_array(a).copy() for a in K.resample_tables(g, slab, crop))
    return br.reshape(crop[0], REC), bc.reshape(crop[1], REC), nr, nc


def filter_axis(src, rec):
    """One pass of PIL's 8-bit resampling along axis 0 with the integer rule of the header: clip8(((1 << 21) + sum pixel * k) >> 22), int32 accumulators."""
    out = np.zeros((rec.shape[0],) + src.shape[1:], dtype=np.uint8)
    for i, r in enumerate(rec):
        first, cnt = int(r[0]), int(r[1])
        if cnt == 0:
            continue                                                           # pad: 0
        k = r[2:2 + cnt].astype(np.int64).reshape((cnt,) + (1,) * (src.ndim - 1))
        s = (1 << (PREC - 1)) + (src[first:first + cnt].astype(np.int64) * k).sum(0)
        assert np.abs(s).max() < 2 ** 31                                       # int32 holds it, as in PIL and in the kernel
        out[i] = np.clip(s >> PREC, 0, 255)
    return out


def apply_tables(img, lab, tabs, ignore=255):
    """The kernel's arithmetic in numpy: along W into bytes, then along H; labels gathered through the nearest tables."""
    br, bc, nr, nc = tabs
    mid = filter_axis(img.transpose(1, 0, 2), bc).transpose(1, 0, 2)           # [H][tw][3]
    out = filter_axis(mid, br)
    out_lab = np.where((nr[:, None] < 0) | (nc[None, :] < 0), ignore, lab[np.maximum(nr, 0)[:, None], np.maximum(nc, 0)[None, :]]).astype(np.uint8)
    return out, out_lab


def test_fixture_is_what_pil_computes_and_covers_what_it_is_there_for():
    pytest.importorskip('PIL')
    tool = _tool()
    arrays = tool.generate()
    assert os.path.getsize(tool.FIXTURE) < 200 * 1024
    with np.load(tool.FIXTURE, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(arrays)
        for k, v in arrays.items():
            assert f[k].dtype == v.dtype and np.array_equal(f[k], v), k
    c = tool.cases()
    for name in ('sq', 'ns'):
        assert tuple(s for _, s, _ in c[name][1]) == (0.5, 0.613, 0.77, 1.0, 1.31, 1.999, 2.0) and {o for _, _, o in c[name][1]} == {'zero', 'max', 'mid'}
        assert not arrays[name + '_geo'][:, 4:6].any()                                          # no padding there
    assert c['sq'][0][0] == c['sq'][0][1] and c['ns'][0][0] != c['ns'][0][1]
    for n in c:
        for row in arrays[n + '_geo']:                                                           # every window lies inside its padded image
            assert 0 <= row[6] <= row[2] + 2 * row[4] - c[n][0][0] and 0 <= row[7] <= row[3] + 2 * row[5] - c[n][0][1]
    g = arrays['pad1_geo']
    assert (g[:, 4] == (38 - 32) // 2 + 1).all() and not g[:, 5].any() and g[0, 6] == 0 and g[1, 6] == 32 + 2 * 4 - 38
    g = arrays['pad2_geo'][0]
    assert (g[4], g[5]) == ((45 - 26) // 2 + 1, (83 - 48) // 2 + 1) and g[2] < 45 and g[3] < 83
    th, tw = c['big'][0]
    assert th > tool.TILE[0] and tw > tool.TILE[1] and th % tool.TILE[0] and tw % tool.TILE[1] and not arrays['big_geo'][:, 4:6].any()
    assert {tuple(r[:2]) for r in arrays['mixed_geo']} == {(52, 97), (97, 161)}
    labs = np.concatenate([arrays['src%d_lab' % k].ravel() for k in range(4)])
    assert set(np.unique(labs)) == set(range(19)) | {255}
    for name in c:                                                                             # pad pixels are black / ignore; the ignore label survives inside too
        assert arrays[name + '_img'].shape[1:3] == tuple(c[name][0]) and (arrays[name + '_lab'] == 255).any()


def test_library_tables_reproduce_every_case_with_no_differing_byte(golden):
    """The library's tables applied in numpy with the integer rule: 0 bytes off PIL in every bicubic crop and every nearest crop of the fixture."""
    with golden('resample_cases.npz') as f:
        fx = {k: f[k] for k in f.files}
    names = sorted(k[:-4] for k in fx if k.endswith('_geo'))
    assert len(names) == 8
    for name in names:
        crop = tuple(int(v) for v in fx[name + '_crop'])
        for i, row in enumerate(fx[name + '_geo']):
            k = int(fx[name + '_src'][i])
            img, lab = fx['src%d_img' % k], fx['src%d_lab' % k]
            got, got_lab = apply_tables(img, lab, tables(geo_image(*row), img.shape[:2], crop))
            bad, bad_lab = int((got != fx[name + '_img'][i]).sum()), int((got_lab != fx[name + '_lab'][i]).sum())
            print('case %s image %d (scale %.4f): %d image bytes, %d label bytes differ from PIL' % (name, i, fx[name + '_scale'][i], bad, bad_lab))
            assert bad == 0 and bad_lab == 0
            if row[2] == row[0] and row[3] == row[1] and not row[4] and not row[5]:            # scale 1.0: PIL skips both passes, a plain slice
                assert np.array_equal(got, img[row[6]:row[6] + crop[0], row[7]:row[7] + crop[1]])


def test_nearest_tables_follow_pil_where_the_closed_form_does_not():
    """Image.resize(NEAREST) accumulates its source coordinate from output position 0; int(a * (x + 0.5)) is other pixels. On a 128 x 255 mask the accumulated tables
    give PIL's bytes at every size tried and the closed form does not, also for a window far from the origin."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 20, size=(128, 255)).astype(np.uint8)
    closed_off = 0
    for h, w in ((96, 191), (80, 160), (112, 223), (192, 383), (72, 143), (255, 509)):
        want = np.array(Image.fromarray(lab, 'L').resize((w, h), Image.NEAREST))
        th, tw = h // 2, w // 2
        y1, x1 = h - th, w - tw                                                                 # the far corner: the longest accumulation
        _, _, nr, nc = tables(geo_image(128, 255, h, w, 0, 0, y1, x1), (128, 255), (th, tw))
        assert np.array_equal(lab[nr[:, None], nc[None, :]], want[y1:, x1:]), (h, w)
        cy = (128 / h * (np.arange(y1, h) + 0.5)).astype(np.int64)
        cx = (255 / w * (np.arange(x1, w) + 0.5)).astype(np.int64)
        closed_off += int((cy != nr).sum() + (cx != nc).sum())
    assert closed_off > 0


def test_tap_cap_holds_every_scale_from_a_quarter_to_four():
    """PM_RESAMPLE_MAX_TAPS: int() of the resized size pushes in / out past 1 / scale, most for small images; every size up to 300 at the ends of [0.25, 4] and at
    scales whose resized size just misses an integer stays under the cap, and every tap count written is PIL's bound min(in, 2 * support + 1) at the most."""
    lib = L.load()
    assert L.RESAMPLE_MAX_TAPS == 24 and REC == 26 and ctypes.sizeof(L.PmGeoImage) == 32
    most = 0
    for size in list(range(4, 301)) + [1024, 1052, 1914, 2048]:
        for scale in (0.25, 0.2501, 0.26, 0.3333, 0.5, 3.999, 4.0):
            out = int(size * scale)
            br, bc, _, _ = tables(geo_image(size, size, out, out, 0, 0, 0, 0), (size, size), (out, out))
            assert np.array_equal(br, bc)
            most = max(most, int(br[:, 1].max()))
            assert br[:, 1].min() >= 1 and (br[:, 0] + br[:, 1] <= size).all() and (np.diff(br[:, 0]) >= 0).all()
            assert (br[:, 2:].sum(1) - (1 << PREC)).__abs__().max() <= 16                       # the coefficients of a position sum to 2^22 up to their rounding
            assert np.abs(br[:, 2:]).sum(1).max() < 1 << 23                                     # so 255 * sum |k| fits int32
    assert 17 <= most <= L.RESAMPLE_MAX_TAPS
    g = geo_image(1000, 1000, 100, 100, 0, 0, 0, 0)
    bufs = [(ctypes.c_int32 * (100 * REC))(), (ctypes.c_int32 * (100 * REC))(), (ctypes.c_int32 * 100)(), (ctypes.c_int32 * 100)()]
    assert lib.pm_resample_tables(ctypes.byref(g), 32, 1000, 1000, 100, 100, *bufs) == -4 and b'PM_RESAMPLE_MAX_TAPS' in lib.pm_last_error()      # PM_EUNSUPPORTED
    with pytest.raises(L.PinmemError, match='taps'):
        K.resample_tables(g, (1000, 1000), (100, 100))


def test_argument_validation_happens_before_anything_touches_a_device():
    """Fake aligned pointers, no GPU in this container: every refusal below returns before a launch."""
    lib = L.load()
    size = ctypes.sizeof(L.PmGeoImage)
    t = [(ctypes.c_int32 * (8 * REC))(), (ctypes.c_int32 * (8 * REC))(), (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()]
    tab = lib.pm_resample_tables

    def run(g, hs=16, ws=20, th=8, tw=8, size=size, bufs=t):
        return tab(ctypes.byref(g) if g is not None else None, size, hs, ws, th, tw, *bufs)
    ok = geo_image(16, 20, 12, 15, 0, 0, 4, 7)
    assert run(ok) == 0
    assert run(ok, size=size - 4) == -1 and b'struct_size' in lib.pm_last_error()
    assert run(None) == -1 and b'resample_tables' in lib.pm_last_error()
    for k in range(4):
        assert run(ok, bufs=t[:k] + [None] + t[k + 1:]) == -1
    assert run(ok, hs=15) == -1 and b'slab' in lib.pm_last_error()                             # h_in > Hs
    assert run(ok, ws=19) == -1 and b'slab' in lib.pm_last_error()
    assert run(geo_image(16, 20, 12, 15, 0, 0, 5, 7)) == -1 and b'outside the padded image' in lib.pm_last_error()      # y1 + th > h
    assert run(geo_image(16, 20, 12, 15, 0, 0, 4, 8)) == -1 and b'outside the padded image' in lib.pm_last_error()
    assert run(geo_image(16, 20, 12, 15, 0, 0, -1, 0)) == -1
    assert run(geo_image(16, 20, 6, 15, 2, 0, 2, 0)) == 0 and run(geo_image(16, 20, 6, 15, 2, 0, 3, 0)) == -1           # the pad counts on both sides
    assert run(geo_image(16, 20, 0, 15, 0, 0, 0, 0)) == -1 and run(geo_image(0, 20, 12, 15, 0, 0, 0, 0)) == -1
    assert run(geo_image(16, 20, 12, 15, -1, 0, 0, 0)) == -1
    assert run(ok, th=0) == -1
    assert run(geo_image(16, 2000, 12, 15, 0, 0, 4, 7), ws=2000) == -4                          # 2000 -> 15 columns: beyond the tap cap, PM_EUNSUPPORTED

    IMG, LAB, GEO, T0, T1, T2, T3, OUT, OUTL = (0x1000000 * k for k in range(1, 10))
    call = lib.pm_resample_crop_u8
    args = [IMG, LAB, 2, 16, 20, GEO, size, T0, T1, T2, T3, 8, 8, 255, OUT, OUTL, None]

    def crop(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    assert crop(a6=size + 8) == -1 and b'struct_size' in lib.pm_last_error()
    for k in (0, 1, 5, 7, 8, 9, 10, 14, 15):
        assert crop(**{'a%d' % k: None}) == -1 and b'null' in lib.pm_last_error(), k
    assert crop(a2=-1) == -1 and crop(a3=0) == -1 and crop(a4=0) == -1 and crop(a11=0) == -1 and crop(a12=-3) == -1
    assert crop(a13=256) == -1 and crop(a13=-1) == -1 and b'ignore_index' in lib.pm_last_error()
    assert crop(a14=IMG) == -1 and b'overlaps' in lib.pm_last_error()                          # output aliasing input
    assert crop(a14=IMG + 2 * 16 * 20 * 3 - 1) == -1 and crop(a15=LAB) == -1 and crop(a15=IMG + 5) == -1 and crop(a14=LAB + 7) == -1
    assert crop(a15=OUT + 2 * 8 * 8 * 3 - 1) == -1                                             # the two outputs overlap
    assert crop(a2=70000) == -4 and b'launch grid' in lib.pm_last_error()
    assert crop(a2=0) == 0                                                                     # an empty batch launches nothing


def test_binding_refuses_a_geometry_the_library_refuses():
    geo = K.GeoParams(2, (8, 8))
    assert len(geo) == 2 and geo.crop == (8, 8) and geo.ignore_index == 255
    for p in geo.images:
        p.h_in, p.w_in, p.h, p.w, p.y1, p.x1 = 16, 20, 12, 15, 4, 7
    assert [len(a) for a in K.resample_tables(geo.images[0], (16, 20), (8, 8))] == [8 * REC, 8 * REC, 8, 8]
    with pytest.raises(L.PinmemError, match='slab'):
        K.resample_tables(geo.images[0], (15, 20), (8, 8))
    geo.images[1].x1 = 8
    with pytest.raises(L.PinmemError, match='outside the padded image'):
        K.resample_tables(geo.images[1], (16, 20), (8, 8))


def _fields(geo):
    return [(p.h_in, p.w_in, p.h, p.w, p.pad_h, p.pad_w, p.y1, p.x1) for p in geo.images]


SIZES = [(1052, 1914), (1024, 2048), (512, 1024), (760, 1280)]


def test_sampler_is_deterministic_per_seed_and_independent_of_the_split():
    sizes = [SIZES[i % 4] for i in range(24)]
    cents = [None if i % 3 else (100 + 37 * i, 50 + 11 * i) for i in range(24)]
    a = _fields(input_edge.GeometricAugment(768, seed=3).sample(sizes, cents))
    assert a == _fields(input_edge.GeometricAugment(768, seed=3).sample(sizes, cents))
    assert a != _fields(input_edge.GeometricAugment(768, seed=4).sample(sizes, cents))
    s = input_edge.GeometricAugment(768, seed=3)
    parts = []
    for lo, hi in ((0, 5), (5, 6), (6, 22), (22, 24)):
        parts += _fields(s.sample(sizes[lo:hi], cents[lo:hi]))
    assert parts == a and s.count == 24


def test_sampler_keeps_the_distributions_of_the_host_pipeline():
    N, (th, tw) = 6000, (768, 640)
    A = input_edge.GeometricAugment((th, tw), seed=11)
    sizes = [SIZES[i % 4] for i in range(N)]
    geo = A.sample(sizes)
    assert geo.crop == (th, tw) and geo.ignore_index == 255 and len(geo) == N
    d = A.last
    scales = np.array(d['scale'])
    assert 0.5 <= scales.min() < 0.51 and 1.99 < scales.max() <= 2.0 and abs(scales.mean() - 1.25) < 0.02      # U[0.5, 2]: sd of the mean over 6 000 draws 0.0056
    fx, fy, padded = [], [], 0
    for i, p in enumerate(geo.images):
        H, W = sizes[i]
        assert (p.h_in, p.w_in) == (H, W) and (p.h, p.w) == (int(H * d['scale'][i]), int(W * d['scale'][i]))
        assert p.pad_h == ((th - p.h) // 2 + 1 if th > p.h else 0) and p.pad_w == ((tw - p.w) // 2 + 1 if tw > p.w else 0)
        max_y, max_x = p.h + 2 * p.pad_h - th, p.w + 2 * p.pad_w - tw
        assert 0 <= p.y1 <= max_y and 0 <= p.x1 <= max_x                                       # the crop lies inside the padded image
        padded += bool(p.pad_h or p.pad_w)
        if max_x > 50 and max_y > 50:
            fx.append(p.x1 / max_x), fy.append(p.y1 / max_y)
    assert padded > 100 and len(fx) > 3000
    for f in (np.array(fx), np.array(fy)):                                                     # the origin is uniform over [0, max] and reaches both ends
        assert f.min() < 0.01 and f.max() > 0.99 and abs(f.mean() - 0.5) < 0.02
    # pre_size: the shorter edge goes to pre_size first
    P = input_edge.GeometricAugment(64, scale_min=1.0, scale_max=1.0, pre_size=100, seed=1)
    g = P.sample([(200, 300), (300, 150)])
    assert _fields(g)[0][:4] == (200, 300, 100, 150) and _fields(g)[1][:4] == (300, 150, 200, 100)
    # an image of exactly the crop size: the window is the image
    g = input_edge.GeometricAugment((50, 70), scale_min=1.0, scale_max=1.0, seed=2).sample([(50, 70)] * 5, [(3, 4)] * 5)
    assert all(f == (50, 70, 50, 70, 0, 0, 0, 0) for f in _fields(g))


def test_sampler_covers_the_centroid():
    N, (th, tw) = 3000, (96, 128)
    A = input_edge.GeometricAugment((th, tw), seed=7)
    rng = np.random.default_rng(3)
    sizes = [(256, 512)] * N
    cents = [(int(rng.integers(0, 512)), int(rng.integers(0, 256))) for _ in range(N)]
    geo = A.sample(sizes, cents)
    offs = []
    for i, p in enumerate(geo.images):
        cx, cy = (int(c * A.last['scale'][i]) for c in cents[i])
        assert A.last['centroid'][i] == (cx, cy)
        assert 0 <= p.y1 <= p.h + 2 * p.pad_h - th and 0 <= p.x1 <= p.w + 2 * p.pad_w - tw
        if not p.pad_w:                                                                         # the reference does not shift the centroid by the pad
            assert p.x1 <= cx <= p.x1 + tw
            offs.append(cx - p.x1)
        if not p.pad_h:
            assert p.y1 <= cy <= p.y1 + th
    assert min(offs) == 0 and max(offs) == tw                                                  # randint(c - tw, c): both ends are drawn


def test_crop_nopad_is_served_only_while_nothing_has_to_shrink():
    A = input_edge.GeometricAugment(64, scale_min=1.0, scale_max=1.0, crop_nopad=True, seed=0)
    g = A.sample([(64, 100), (200, 64)])
    assert all(f[4:6] == (0, 0) for f in _fields(g)) and A.count == 2
    with pytest.raises(NotImplementedError, match='crop_nopad'):
        A.sample([(63, 100)])
    with pytest.raises(NotImplementedError):
        input_edge.GeometricAugment(768, crop_nopad=True, scale_min=0.5, scale_max=0.5).sample([(1052, 1914)])
    with pytest.raises(ValueError):
        input_edge.GeometricAugment(8, scale_min=0.01, scale_max=0.01).sample([(50, 50)])


def test_edge_without_geometry_does_not_go_near_the_resampling_bindings(monkeypatch):
    """geometry=None is the default of both entry points and takes exactly the old calls: the new bindings are replaced by bombs, the old ones by recorders."""
    for fn in (harness.prepare_batch_u8, input_edge.DevicePrefetcher.__init__):
        assert inspect.signature(fn).parameters['geometry'].default is None
    assert [inspect.signature(harness.prepare_batch_u8).parameters[k].default for k in ('sizes', 'centroids')] == [None, None]

    def bomb(*a, **k):
        raise AssertionError('the edge without geometry called a resampling binding')
    calls = []
    for name in ('resample_crop_u8', 'upload_geo', 'resample_tables', 'GeoParams'):
        monkeypatch.setattr(K, name, bomb)
    monkeypatch.setattr(input_edge, 'sample_geometry', bomb)
    monkeypatch.setattr(K, 'image_u8_to_nhwc4', lambda img: calls.append(('img', tuple(img.shape))) or torch.zeros(img.shape[:3] + (4,)))
    monkeypatch.setattr(K, 'labels_u8_to_i64', lambda lab: calls.append(('lab', tuple(lab.shape))) or lab.long())
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    img, lab = torch.zeros((2, 3, 4, 6, 3), dtype=torch.uint8), torch.full((2, 3, 4, 6), 255, dtype=torch.uint8)
    x, gt = harness.prepare_batch_u8(img, lab)
    assert calls == [('img', (6, 4, 6, 3)), ('lab', (6, 4, 6))] and tuple(x.shape) == (6, 4, 4, 6) and gt.dtype == torch.int64
