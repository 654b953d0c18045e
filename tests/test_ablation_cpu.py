"""CPU: the ablation sweep without a GPU -- every refusal of pm_label_splat / pm_class_sums / pm_mem_actmap in front of any device call, the bookkeeping of
harness.FeatureBasket on injected sums and counts, and the premise of the activation-byte rule of tests/test_ablation.py held by the reference alone (torch's fp32
F.interpolate formulation against the same formulation in fp64) on exactly the inputs the GPU test uses."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from pinthememory_amd.harness import FeatureBasket
from pinthememory_amd.hip import lib as L

import ablation_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
BUF = ctypes.create_string_buffer(1 << 16)      # host memory: nothing below may dereference it (the slot list excepted, which IS a host array)
P = (ctypes.addressof(BUF) + 15) // 16 * 16
N, H, W, h, w, C, M = 2, 9, 10, 3, 4, 16, 19
SLOTS = (ctypes.c_int32 * 3)(18, 0, 5)


def splat_args(**over):
    a = dict(labels=P, n=N, H=H, W=W, h=h, w=w, classes=19, splat=P + 4096, counts=P + 8192, stream=None)
    a.update(over)
    return list(a.values())


def sums_args(**over):
    a = dict(feat=P, n=N, h=h, w=w, c=C, feat_pitch=C, dtype=L.PM_F32, splat=P + 4096, classes=19, sums=P + 8192, ws=P + 16384, ws_bytes=1 << 40, stream=None)
    a.update(over)
    return list(a.values())


def act_args(**over):
    a = dict(p_mem=P, n=N, h=h, w=w, m=M, pitch=M, H=H, W=W, slots=SLOTS, nslots=3, act=P + 4096, bytes=P + 8192, palette=P + 12288, image=P + 16384, alpha=0.65,
             rgb=P + 20480, blend=P + 24576, stream=None)
    a.update(over)
    return list(a.values())


SPLAT_REFUSALS = [
    ('null labels', dict(labels=None), EINVAL), ('null splat', dict(splat=None), EINVAL), ('null counts', dict(counts=None), EINVAL),
    ('n = 0', dict(n=0), EINVAL), ('H < 0', dict(H=-1), EINVAL), ('W = 0', dict(W=0), EINVAL), ('h = 0', dict(h=0), EINVAL), ('w < 0', dict(w=-2), EINVAL),
    ('classes = 0', dict(classes=0), EINVAL),
    ('classes = 32', dict(classes=32), EUNSUPPORTED),
]
SUMS_REFUSALS = [
    ('null feat', dict(feat=None), EINVAL), ('null splat', dict(splat=None), EINVAL), ('null sums', dict(sums=None), EINVAL), ('null ws', dict(ws=None), EINVAL),
    ('n = 0', dict(n=0), EINVAL), ('h < 0', dict(h=-1), EINVAL), ('w = 0', dict(w=0), EINVAL), ('c = 0', dict(c=0), EINVAL), ('classes = 0', dict(classes=0), EINVAL),
    ('pitch below c', dict(feat_pitch=C - 4), EINVAL), ('pitch off the fp32 vector', dict(feat_pitch=C + 2), EINVAL),
    ('pitch off the bf16 vector', dict(dtype=L.PM_BF16, feat_pitch=C + 4), EINVAL), ('feat off 16 bytes', dict(feat=P + 4), EINVAL),
    ('ws off 16 bytes', dict(ws=P + 16388), EINVAL),
    ('unknown dtype', dict(dtype=2), EUNSUPPORTED), ('negative dtype', dict(dtype=-1), EUNSUPPORTED),
    ('c = 12', dict(c=12, feat_pitch=12), EUNSUPPORTED), ('c = 4', dict(c=4), EUNSUPPORTED), ('classes = 32', dict(classes=32), EUNSUPPORTED),
    ('short workspace', dict(ws_bytes='short'), EWORKSPACE), ('no workspace bytes', dict(ws_bytes=0), EWORKSPACE),
]
ACT_REFUSALS = [
    ('null p_mem', dict(p_mem=None), EINVAL), ('null slots', dict(slots=None), EINVAL),
    ('n = 0', dict(n=0), EINVAL), ('h = 0', dict(h=0), EINVAL), ('w < 0', dict(w=-1), EINVAL), ('m = 0', dict(m=0), EINVAL), ('H = 0', dict(H=0), EINVAL),
    ('W < 0', dict(W=-5), EINVAL), ('nslots = 0', dict(nslots=0), EINVAL), ('nslots > m', dict(m=2, pitch=2, nslots=3), EINVAL),
    ('pitch below m', dict(pitch=M - 1), EINVAL),
    ('slot = m', dict(slots=(ctypes.c_int32 * 3)(18, 19, 5)), EINVAL), ('negative slot', dict(slots=(ctypes.c_int32 * 3)(-1, 0, 5)), EINVAL),
    ('no output', dict(act=None, bytes=None, rgb=None, blend=None), EINVAL),
    ('rgb without palette', dict(palette=None, blend=None), EINVAL), ('blend without palette', dict(palette=None, rgb=None), EINVAL),
    ('blend without image', dict(image=None), EINVAL),
    ('m = 33', dict(m=33, pitch=33), EUNSUPPORTED),
]


def _call(fn, maker, over):
    lib = L.load()
    if over.get('ws_bytes') == 'short':
        over = dict(over, ws_bytes=lib.pm_class_sums_workspace(N, h, w, C, 19) - 1)
    return getattr(lib, fn)(*maker(**over)), lib.pm_last_error()


@pytest.mark.parametrize('what,over,status', SPLAT_REFUSALS, ids=[r[0] for r in SPLAT_REFUSALS])
def test_label_splat_refusals(what, over, status):
    code, msg = _call('pm_label_splat', splat_args, over)
    assert code == status, (what, code, msg)
    assert b'label_splat' in msg


@pytest.mark.parametrize('what,over,status', SUMS_REFUSALS, ids=[r[0] for r in SUMS_REFUSALS])
def test_class_sums_refusals(what, over, status):
    code, msg = _call('pm_class_sums', sums_args, over)
    assert code == status, (what, code, msg)
    assert b'class_sums' in msg


@pytest.mark.parametrize('what,over,status', ACT_REFUSALS, ids=[r[0] for r in ACT_REFUSALS])
def test_mem_actmap_refusals(what, over, status):
    code, msg = _call('pm_mem_actmap', act_args, over)
    assert code == status, (what, code, msg)
    assert b'mem_actmap' in msg


def test_workspace_query_abi_number_and_header():
    lib = L.load()
    assert L.ABI_VERSION == 460 and lib.pm_version() == 460
    for bad in ((0, 3, 4, 16, 19), (2, -3, 4, 16, 19), (2, 3, 0, 16, 19), (2, 3, 4, -8, 19), (2, 3, 4, 16, 0)):
        assert lib.pm_class_sums_workspace(*bad) == 0, bad
    for n, hh, ww, c, k in ((1, 1, 1, 8, 19), (2, 12, 20, 256, 19), (1, 45, 80, 256, 19), (3, 7, 5, 24, 4)):
        nb = lib.pm_class_sums_workspace(n, hh, ww, c, k)
        # one [classes + 1][c] row of fp32 partials per chunk of a fixed number of pixels: at least one chunk per image, at most one per pixel
        assert nb % 256 == 0 and n * (k + 1) * c * 4 <= nb <= n * hh * ww * (k + 1) * c * 4 + 256, (n, hh, ww, c, k, nb)
    hdr = open(os.path.join(ROOT, 'include', 'pinmem_hip.h')).read()
    sect = hdr[hdr.index('/* ---- ablation sweep'):hdr.index('/* ---- input edge (SURVEY 8(f) rank 4)')]
    for name in ('int pm_label_splat(', 'size_t pm_class_sums_workspace(', 'int pm_class_sums(', 'int pm_mem_actmap('):
        assert name in sect, name
    assert 'pm_tensor' not in sect
    assert 'WITHOUT a version step' in hdr[hdr.index('460:'):hdr.index('#define PM_ABI_VERSION')]


# ---- FeatureBasket: bookkeeping on injected sums and counts, no kernel involved ----------------------------------------------------------------------------------
def _inject(n, C, seed, absent):
    g = AC.gen(seed)
    sums = torch.randn((n, 20, C), generator=g)
    counts = torch.randint(1, 50, (n, 20), generator=g)
    for i, k in absent:
        counts[i, k] = 0
    return sums, counts


def test_feature_basket_rows_order_normalisation_and_memory():
    sel = [13, 0, 5]
    b = FeatureBasket(sel)
    s0, c0 = _inject(2, 8, 1, absent=[(0, 0), (1, 13), (1, 5)])
    s1, c1 = _inject(1, 8, 2, absent=[])
    b.add_sums(s0, c0, domain_id=3)
    b.add_sums(s1, c1, domain_id=1)
    vecs, labels, domains = b.vectors()
    # image-major, then the order of `sel`, absent classes dropped: what input2basket appends (tsnelib.py:67-74)
    want_rows = [(s0, c0, 0, 13, 3), (s0, c0, 0, 5, 3), (s0, c0, 1, 0, 3), (s1, c1, 0, 13, 1), (s1, c1, 0, 0, 1), (s1, c1, 0, 5, 1)]
    assert labels.tolist() == [r[3] for r in want_rows] and domains.tolist() == [r[4] for r in want_rows]
    assert labels.dtype == torch.int64 and domains.dtype == torch.int64
    want = torch.stack([s[i, k] / c[i, k] for s, c, i, k, _ in want_rows])
    assert torch.equal(vecs, F.normalize(want, dim=1))
    assert torch.allclose(vecs.norm(dim=1), torch.ones(6), atol=1e-6) and bool(torch.isfinite(vecs).all())
    # memory rows follow as they are, labelled with their slot and domain -1 (draw_tsne(plot_memory=True), tsnelib.py:145-147)
    items = torch.randn((19, 8), generator=AC.gen(3))
    b.input_memory_item(items)
    v2, l2, d2 = b.vectors()
    assert torch.equal(v2[:6], vecs) and torch.equal(v2[6:], items[sel]) and l2.tolist()[6:] == sel and d2.tolist()[6:] == [-1, -1, -1]
    b.init_basket()
    v3, l3, d3 = b.vectors()
    assert v3.shape[0] == 0 and l3.numel() == 0 and d3.numel() == 0 and b.mem_vecs is None
    # an image without any selected class contributes no row and no NaN
    b.add_sums(*_inject(1, 8, 4, absent=[(0, 13), (0, 0), (0, 5)]), domain_id=0)
    assert b.vectors()[0].shape[0] == 0
    with pytest.raises(AssertionError):
        FeatureBasket([19])


# ---- the premise of the byte rule, held by the reference alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', AC.ACT_SHAPES, ids=['%dx%d_%dx%d_m%d' % (s[2], s[3], s[4], s[5], s[1]) for s in AC.ACT_SHAPES])
def test_reference_fp32_keeps_the_activation_rule(shape):
    """torch's own fp32 formulation (F.interpolate -> min / max -> divide -> clip * 255 -> uint8) against the same in fp64, on the inputs of the GPU test: the float map
    stays within 32 * 2^-23 / range_p, its bytes differ from the fp64 bytes only inside the band (by one), the extreme slots hold exactly, and the band holds at most
    1 % of the bytes -- so a change of inputs that breaks the rule's premise fails here, without a GPU. Measured on the CPU with these seeds: the map error 3.3 / 7.2 / 10.8 units
    at the three 19-slot shapes and 0.5 at the seven-slot one, band share 0.54-0.59 % and 0.28 % (the share leaves out each pixel's arg-min / arg-max slot, which sits
    on an integer exactly and has the exact rule instead)."""
    n, m, hh, ww, HH, WW = shape
    sc = AC.scores(n, m, hh, ww)
    a64, r64 = AC.act_ref(sc, HH, WW, torch.float64)
    a32, _ = AC.act_ref(sc, HH, WW, torch.float32)
    fig = AC.check_act_rule(a32, AC.act_bytes(a32), a64, r64)
    print(shape, fig)
    assert fig['band_share'] <= 0.01, fig
