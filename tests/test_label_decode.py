"""GPU: the label-decoding input edge (csrc/resample.hip pm_labels_decode_u8, pm_resample_crop_decode_u8; input_edge.LabelDecode) against the dicts of the reference's
datasets (tests/golden/label_tables.json) and the masks a per-pixel dict lookup makes of them (label_decode_cases.npz, tools/make_label_golden.py). uint8 in, uint8 out,
a table lookup: every comparison is exact. The fused crop equals the whole-slab decode followed by pm_resample_crop_u8, and the edge entry points with decode= equal the
path of before fed host-decoded masks."""
import json
import os

import numpy as np
import pytest
import torch

from pinthememory_amd import harness, input_edge
from pinthememory_amd.hip import kernels as K

from test_label_decode_cpu import by_unique, neighbours

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def dicts():
    with open(os.path.join(GOLDEN, 'label_tables.json')) as f:
        t = json.load(f)
    return ({tuple(r[:3]): r[3] for r in t['color2trainId']}, {k: v for k, v in t['label2trainid']}, {k: v for k, v in t['trainid_to_trainid']})


@pytest.fixture(scope='module')
def fx(golden):
    with golden('label_decode_cases.npz') as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def dec(dicts):
    """table 0: GTAV colours, 1: Synthia ids, 2: Cityscapes ids"""
    d = input_edge.LabelDecode()
    assert (d.add_colors(dicts[0]), d.add_ids(dicts[2]), d.add_ids(dicts[1])) == (0, 1, 2)
    return d


def host_decode(raw, entry, dicts, channels=3):
    """numpy, any leading axes: entry -1 / None pass-through, 0 colours, 1 synthia, 2 cityscapes"""
    kinds = {-1: (None, None), 0: ('colors', dicts[0]), 1: ('ids', dicts[2]), 2: ('ids', dicts[1])}
    return np.ascontiguousarray(by_unique(raw, *kinds[-1 if entry is None else int(entry)], channels=channels))


def weighted_pool(colors, seed):
    """colours to draw masks from: the table's own six times over, their +-1 neighbours and 32 random ones"""
    return np.concatenate([np.array(list(colors) * 6, dtype=np.uint8), colour_set(colors, seed, 32)])


def test_whole_slab_decode_three_modes_in_one_call(fx, dec, dicts):
    raw, table, want = fx['mixed_raw'], fx['mixed_table'].tolist(), fx['mixed_want']
    assert raw.shape == (3, 37, 53, 3) and table == [-1, 1, 0]
    tabs = dec.device_tables('cuda')
    got = K.labels_decode_u8(torch.from_numpy(raw).cuda(), tabs, table)
    assert got.dtype == torch.uint8 and got.shape == (3, 37, 53) and np.array_equal(got.cpu().numpy(), want)
    # one channel: pass-through and ids as before; a colour table has no colour to look at and writes its fill
    one = np.ascontiguousarray(raw[..., 0])
    got1 = K.labels_decode_u8(torch.from_numpy(one).cuda(), tabs, table).cpu().numpy()
    assert np.array_equal(got1[:2], want[:2]) and (got1[2] == 255).all()
    with pytest.raises(ValueError, match='colour table'):
        dec.decode(torch.from_numpy(one).cuda(), table)
    assert np.array_equal(dec.decode(torch.from_numpy(raw).cuda(), table).cpu().numpy(), want)
    # an index past the tables is clamped to the last one (cityscapes ids), not followed
    far = K.labels_decode_u8(torch.from_numpy(one[:1]).cuda(), tabs, [1000]).cpu().numpy()
    assert np.array_equal(far[0], host_decode(one[0], 2, dicts, 1))
    # the single-table fixtures (pixel counts that are multiples of four: the four-pixel path), and 553 ids as 7 x 79 (pixel by pixel)
    for name, entry in (('gtav', 0), ('synthia', 1), ('city', 2)):
        got = K.labels_decode_u8(torch.from_numpy(fx[name + '_raw'][None]).cuda(), tabs, [entry])
        assert np.array_equal(got[0].cpu().numpy(), fx[name + '_want']), name
    flat = fx['city_raw'].reshape(-1)[:553].reshape(7, 79)
    assert np.array_equal(K.labels_decode_u8(torch.from_numpy(np.ascontiguousarray(flat[None])).cuda(), tabs, [2])[0].cpu().numpy(), host_decode(flat, 2, dicts, 1))


def colour_set(colors, seed, n_random=4096):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(neighbours(list(colors)), dtype=np.uint8), rng.integers(0, 256, size=(n_random, 3), dtype=np.uint8)])


def both_paths(px, tabs, entry):
    """the pixels as one image of a size the four-pixel path takes (several blocks) and of a size it does not, -> the two results as flat arrays"""
    n = len(px) // 4 * 4
    a = K.labels_decode_u8(torch.from_numpy(np.ascontiguousarray(px[:n].reshape(1, 4, n // 4, 3))).cuda(), tabs, [entry]).cpu().numpy().reshape(-1)
    m = n - 1
    w = next(w for w in (7, 5, 3, 1) if m % w == 0)
    assert (m // w * w) % 4 != 0
    b = K.labels_decode_u8(torch.from_numpy(np.ascontiguousarray(px[:m].reshape(1, m // w, w, 3))).cuda(), tabs, [entry]).cpu().numpy().reshape(-1)
    return n, a, m, b


def test_colour_test_set_every_table_colour_its_neighbours_and_random_colours(dec, dicts):
    colors = dicts[0]
    px = colour_set(colors, 11)
    listed = {tuple(int(v) for v in p) for p in px}
    assert set(colors) <= listed and (153, 153, 154) in listed and (0, 0, 143) in listed and (0, 0, 141) in listed and len(px) > 4096 + 150
    want = by_unique(px[None], 'colors', colors)[0]
    assert set(range(19)) <= set(want.tolist())
    n, a, m, b = both_paths(px, dec.device_tables('cuda'), 0)
    assert n // 4 > 256 and np.array_equal(a, want[:n]) and np.array_equal(b, want[:m])
    for c, v in colors.items():                                                                 # spelled out for the pairs one unit apart
        i = next(i for i, p in enumerate(px) if tuple(p) == c)
        assert a[i] == (255 if v in (255, -1) else v)
    assert a[[tuple(p) for p in px].index((0, 0, 142))] == 13 and a[[tuple(p) for p in px].index((0, 0, 143))] == 255
    assert a[[tuple(p) for p in px].index((153, 153, 153))] == 5 and a[[tuple(p) for p in px].index((153, 153, 154))] == 255


def test_a_full_table_of_128_random_colours(dicts):
    rng = np.random.default_rng(3)
    packed = rng.choice(1 << 24, size=128, replace=False)
    table = {(int(p) & 255, (int(p) >> 8) & 255, int(p) >> 16): int(v) for p, v in zip(packed, rng.integers(0, 254, size=128))}
    homes = [(((c[0] | c[1] << 8 | c[2] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 24 for c in table]
    assert len(set(homes)) < 128                                                                # home slots collide: the walk is exercised
    d = input_edge.LabelDecode(ignore_index=254)
    d.add_ids({1: 2})
    t = d.add_colors(table)
    px = colour_set(table, 12)
    want = by_unique(px[None], 'colors', table, fill=254)[0]
    assert (want != 254).sum() >= 128
    n, a, m, b = both_paths(px, d.device_tables('cuda'), t)
    assert np.array_equal(a, want[:n]) and np.array_equal(b, want[:m])


@pytest.mark.parametrize('hw', [(364, 364), (181, 183)])
def test_whole_slab_blocks_stride_over_their_image(dec, dicts, hw):
    """16 images large enough that every block takes several trips over its image: 364 x 364 on the four-pixel path, 181 x 183 pixel by pixel; the three modes mixed."""
    rng = np.random.default_rng(hw[0])
    n, entries = 16, [0, 1, -1, 2] * 4
    assert (hw[0] * hw[1] % 4 == 0) == (hw == (364, 364)) and hw[0] * hw[1] // (4 if hw == (364, 364) else 1) > 256 * (2048 // n)
    pool = weighted_pool(dicts[0], 15)
    raw = pool[rng.integers(0, len(pool), size=(n,) + hw)]
    for i in range(n):
        if entries[i] != 0:
            raw[i, :, :, 0] = rng.integers(0, 40, size=hw)
    got = K.labels_decode_u8(torch.from_numpy(raw).cuda(), dec.device_tables('cuda'), entries).cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], host_decode(raw[i], entries[i], dicts)), i


def _geometry(scales, sizes, crop, seed):
    """one image per scale, origins as GeometricAugment draws them"""
    g = K.GeoParams(len(scales), crop)
    for i, s in enumerate(scales):
        one = input_edge.GeometricAugment(crop, scale_min=s, scale_max=s, seed=seed + i).sample([sizes[i]])
        for name, _ in one.images[0]._fields_:
            setattr(g.images[i], name, getattr(one.images[0], name))
    return g


@pytest.mark.parametrize('crop,scales', [((32, 32), (0.5, 1.25, 2.0, 0.75)), ((40, 72), (2.0, 1.9, 2.0, 1.5))])
def test_fused_crop_is_decode_then_crop(dec, dicts, crop, scales):
    """40 x 56 images in 48 x 64 slabs whose other bytes are poison; tables per image: colours, synthia ids, pass-through, colours. (32, 32): scales 0.5 (padded on both axes),
    1.25, 2.0 and 0.75 (30 x 42: rows padded). (40, 72): a window of 2 x 2 tiles with ragged edges."""
    rng = np.random.default_rng(sum(crop))
    n, (hs, ws), (h, w) = 4, (48, 64), (40, 56)
    entries = [0, 1, -1, 0]
    pool = weighted_pool(dicts[0], 13)
    img = rng.integers(0, 256, size=(n, hs, ws, 3), dtype=np.uint8)
    img[:, h:], img[:, :, w:] = 0x5a, 0x5a
    lab = np.full((n, hs, ws, 3), 0x5a, dtype=np.uint8)
    lab[:, :h, :w] = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    lab[1, :h, :w, 0], lab[2, :h, :w, 0] = rng.integers(0, 25, size=(h, w)), rng.integers(0, 20, size=(h, w))
    for i in (0, 3):
        lab[i, :h, :w] = pool[rng.integers(0, len(pool), size=(h // 4, w // 4))].repeat(4, 0).repeat(4, 1)
    g = _geometry(scales, [(h, w)] * n, crop, 40)
    if crop == (32, 32):
        assert [(p.pad_h > 0, p.pad_w > 0) for p in g.images] == [(True, True), (False, False), (False, False), (True, False)]
    tabs, table = dec.device_tables('cuda'), dec.image_table(entries, n, 3)
    img_d, lab_d = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    whole = K.labels_decode_u8(lab_d, tabs, table)
    assert np.array_equal(whole.cpu().numpy()[:, :h, :w], np.stack([host_decode(lab[i, :h, :w], entries[i], dicts) for i in range(n)]))
    want_img, want_lab = K.resample_crop_u8(img_d, whole, g)
    got_img, got_lab = K.resample_crop_decode_u8(img_d, lab_d, g, tabs, table)
    assert got_lab.shape == (n,) + crop and torch.equal(got_lab, want_lab) and torch.equal(got_img, want_img)
    assert len(torch.unique(got_lab)) > 10
    # other poison around the images: nothing outside h_in x w_in is read
    lab2, img2 = lab.copy(), img.copy()
    lab2[:, h:], lab2[:, :, w:], img2[:, h:], img2[:, :, w:] = 0xa5, 0xa5, 0xa5, 0xa5
    again_img, again_lab = K.resample_crop_decode_u8(torch.from_numpy(img2).cuda(), torch.from_numpy(lab2).cuda(), g, tabs, table)
    assert torch.equal(again_lab, want_lab) and torch.equal(again_img, want_img)
    # an uploaded geometry carries the image_table in its block and serves a second call
    gd = K.upload_geo(g, img_d.device, (hs, ws), table)
    for _ in range(2):
        a, b = K.resample_crop_decode_u8(img_d, lab_d, gd, tabs, table)
        assert torch.equal(a, want_img) and torch.equal(b, want_lab)
    # one channel: ids and pass-through alone
    e1 = [1, 2, -1, None]
    one = torch.from_numpy(np.ascontiguousarray(lab[..., 0] % 34)).cuda()
    t1 = dec.image_table(e1, n, 1)
    w_img, w_lab = K.resample_crop_u8(img_d, K.labels_decode_u8(one, tabs, t1), g)
    g_img, g_lab = K.resample_crop_decode_u8(img_d, one, g, tabs, t1)
    assert torch.equal(g_lab, w_lab) and torch.equal(g_img, w_img)


class _RawSource:
    """A loader stand-in over three precomputed batches: [B, 2, H, W, 3] images and raw masks -- domain 0 colour-coded, domain 1 id-coded with its id in channel 0 -- or,
    with decoded=True, the same images and the masks decoded on the host ([B, 2, H, W] train ids)."""

    def __init__(self, batch, slab, dicts, decoded, one_channel=False):
        rng = np.random.default_rng(77)
        pool = weighted_pool(dicts[0], 14)
        h, w = slab
        self.bufs, self.i = [], 0
        for _ in range(3):
            img = rng.integers(0, 256, size=(batch, 2, h, w, 3), dtype=np.uint8)
            raw = rng.integers(0, 256, size=(batch, 2, h, w, 3), dtype=np.uint8)
            raw[:, 0] = pool[rng.integers(0, len(pool), size=(batch, h // 8, w // 8))].repeat(8, 1).repeat(8, 2)
            raw[:, 1, :, :, 0] = rng.integers(0, 24, size=(batch, h // 4, w // 4)).repeat(4, 1).repeat(4, 2)
            if one_channel:                                                                     # both domains id-coded: synthia ids / train ids
                raw = np.ascontiguousarray(raw[..., 0] % 23)
                host = np.stack([raw[:, 0], host_decode(raw[:, 1], 1, dicts, 1)], 1)
            else:
                host = np.stack([host_decode(raw[:, 0], 0, dicts), host_decode(raw[:, 1], 1, dicts)], 1)
            lab = np.ascontiguousarray(host) if decoded else raw
            self.bufs.append((torch.from_numpy(img).pin_memory(), torch.from_numpy(lab).pin_memory()))

    def __iter__(self):
        return self

    def __next__(self):
        self.i += 1
        return self.bufs[(self.i - 1) % 3]


@pytest.mark.parametrize('geometry', [False, True])
@pytest.mark.parametrize('augment', [False, True])
def test_edge_with_decode_equals_the_edge_of_before_on_host_decoded_masks(dec, dicts, geometry, augment):
    B, slab, crop = 2, (64, 96), (40, 56)
    geo = (lambda: input_edge.GeometricAugment(crop, seed=9)) if geometry else (lambda: None)
    aug = (lambda: input_edge.PhotometricAugment(seed=5)) if augment else (lambda: None)
    new = input_edge.DevicePrefetcher(_RawSource(B, slab, dicts, False), augment=aug(), geometry=geo(), decode=dec, domain_tables=[0, 1])
    old = input_edge.DevicePrefetcher(_RawSource(B, slab, dicts, True), augment=aug(), geometry=geo())
    raw_src, host_src = _RawSource(B, slab, dicts, False), _RawSource(B, slab, dicts, True)
    g1, g2, a1, a2 = geo(), geo(), aug(), aug()
    flips = 0
    for _ in range(4):                                                                          # slots and pinned buffers come round again
        x, gt = new.next()
        ox, ogt = old.next()
        assert gt.dtype == torch.int64 and gt.shape == (2 * B,) + (crop if geometry else slab) and torch.equal(gt, ogt) and torch.equal(x, ox)
        (img, raw), (_, host) = next(raw_src), next(host_src)
        px, pgt = harness.prepare_batch_u8(img, raw, augment=a1, geometry=g1, decode=dec, tables=[0, 1] * B)
        qx, qgt = harness.prepare_batch_u8(img, host, augment=a2, geometry=g2)
        assert torch.equal(pgt, qgt) and torch.equal(px, qx) and torch.equal(pgt, gt) and torch.equal(px, x)
        if augment:
            flips += sum(a1.last['flip'])
        assert len(torch.unique(gt)) > 8
    assert not augment or 0 < flips < 16                                                        # flipped and unflipped images both went through
    torch.cuda.synchronize()


def test_edge_with_decode_on_one_channel_masks_and_its_refusals(dec, dicts):
    B, slab = 2, (64, 96)
    new = input_edge.DevicePrefetcher(_RawSource(B, slab, dicts, False, one_channel=True), decode=dec, domain_tables=[None, 1])
    old = input_edge.DevicePrefetcher(_RawSource(B, slab, dicts, True, one_channel=True))
    for _ in range(2):
        (x, gt), (ox, ogt) = new.next(), old.next()
        assert torch.equal(gt, ogt) and torch.equal(x, ox)
    img, raw = _RawSource(B, slab, dicts, False, one_channel=True).bufs[0]
    with pytest.raises(ValueError, match='colour table'):
        harness.prepare_batch_u8(img, raw, decode=dec, tables=[0, 1] * B)
    with pytest.raises(ValueError):
        harness.prepare_batch_u8(img, raw, decode=dec, tables=[1])
    with pytest.raises(ValueError, match='colour table'):
        input_edge.DevicePrefetcher(_RawSource(B, slab, dicts, False, one_channel=True), decode=dec, domain_tables=[0, 1])
    torch.cuda.synchronize()


def test_validate_with_decode_gives_the_histogram_of_pre_decoded_labels(dec, dicts):
    import torch.nn as nn
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    crit = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    net = synth.load_det_weights(deepv3plus.DeepR50V3PlusD(synth.model_args(), 19, crit, crit)).cuda()
    x, _ = synth.make_batch(2, (64, 64), seed=21)
    rng = np.random.default_rng(8)
    pool = np.array([c for c, v in dicts[0].items()], dtype=np.uint8)
    raw = pool[rng.integers(0, len(pool), size=(2, 8, 8))].repeat(8, 1).repeat(8, 2)
    host = torch.from_numpy(host_decode(raw, 0, dicts)).long()
    assert len(torch.unique(host)) > 10 and (host == 255).any()
    want = harness.validate(net, [(x, host)])
    got = harness.validate(net, [(x, torch.from_numpy(raw))], decode=dec, tables=0)
    assert torch.equal(got['hist'], want['hist']) and int(want['hist'].sum()) == int((host != 255).sum())
    assert got['val_loss'] == want['val_loss'] and got['read_loss'] == want['read_loss'] and torch.equal(got['predictions'][0], want['predictions'][0])
    ids = (raw[..., 0] % 23).astype(np.uint8)
    want = harness.validate(net, [(x, torch.from_numpy(host_decode(ids, 1, dicts, 1)).long())])
    got = harness.validate(net, [(x, torch.from_numpy(ids))], decode=dec, tables=[1, 1])
    assert torch.equal(got['hist'], want['hist']) and got['val_loss'] == want['val_loss']
