"""CPU: the host side of the label-decoding input edge -- pm_label_table_ids / pm_label_table_colors (no device involved) against the dicts of the reference's
datasets (tests/golden/label_tables.json, tools/make_label_golden.py), read back through the probe walk include/pinmem_hip.h documents; the rules of the contract
(dropped 255 / -1 colours, -1 stored as 255, keys outside 0..255, identity default, the colour cap, struct_size); input_edge.LabelDecode's argument checks; and the
fixture's expected masks (a per-pixel dict lookup) against an independent numpy formulation (packed colours + np.unique)."""
import ctypes
import json
import os

import numpy as np
import pytest

from pinthememory_amd import input_edge
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope='module')
def dicts():
    with open(os.path.join(GOLDEN, 'label_tables.json')) as f:
        t = json.load(f)
    return ({tuple(r[:3]): r[3] for r in t['color2trainId']}, {k: v for k, v in t['label2trainid']}, {k: v for k, v in t['trainid_to_trainid']})


def lookup(t, px):
    """A pixel through a host pm_label_table, as the header describes the device's walk."""
    if t.mode == L.LABEL_IDS:
        return t.lut[px[0]]
    key = px[0] | px[1] << 8 | px[2] << 16
    s = ((key * 0x9E3779B1) & 0xFFFFFFFF) >> 24
    for _ in range(L.LABEL_SLOTS):
        if t.keys[s] == key:
            return t.vals[s]
        if t.keys[s] == 0xFFFFFFFF:
            break
        s = (s + 1) % L.LABEL_SLOTS
    return t.fill


def neighbours(colors):
    out = set(colors)
    for c in colors:
        for ch in range(3):
            for d in (-1, 1):
                n = list(c)
                n[ch] += d
                if 0 <= n[ch] <= 255:
                    out.add(tuple(n))
    return sorted(out)


def test_fixture_dicts_are_the_datasets_tables(dicts):
    colors, city, synthia = dicts
    assert len(colors) == 31 and colors[(128, 64, 128)] == 0 and colors[(0, 0, 142)] == 13 and colors[(0, 0, 143)] == -1 and colors[(153, 153, 154)] == 255
    assert len(city) == 35 and city[7] == 0 and city[33] == 18 and city[-1] == -1 and city[0] == 255
    assert len(synthia) == 23 and synthia[1] == 10 and synthia[0] == 255 and synthia[3] == 0 and synthia[22] == 255


def test_colour_builder_against_the_dict(dicts):
    colors = dicts[0]
    t = K.label_table_colors(colors, 255)
    assert ctypes.sizeof(L.PmLabelTable) == 1544 and t.mode == L.LABEL_COLORS and t.fill == 255
    kept = {k: v for k, v in colors.items() if v not in (255, -1)}
    assert len(kept) == 19 and sum(1 for k in t.keys if k != 0xFFFFFFFF) == 19                 # dropped entries take no slot
    for c in neighbours(list(colors)):
        assert lookup(t, c) == kept.get(c, 255), c
    assert lookup(t, (0, 0, 143)) == 255 and lookup(t, (0, 0, 142)) == 13 and lookup(t, (153, 153, 154)) == 255 and lookup(t, (153, 153, 153)) == 5
    assert list(t.lut) == list(range(256))
    t7 = K.label_table_colors(colors, 7)                                                       # the fill is the caller's
    assert lookup(t7, (1, 2, 3)) == 7 and lookup(t7, (0, 0, 143)) == 7 and lookup(t7, (70, 70, 70)) == 2


def test_id_builder_against_the_dicts(dicts):
    for table in dicts[1:]:
        t = K.label_table_ids(table)
        assert t.mode == L.LABEL_IDS and all(k == 0xFFFFFFFF for k in t.keys)
        for i in range(256):
            assert t.lut[i] == (table[i] & 255 if i in table else i), i
    city = K.label_table_ids(dicts[1])
    assert -1 in dicts[1] and city.lut[255] == 255                                             # the key -1 never matches; 255 stays 255 by identity


def test_id_rules_wrap_range_no_chain_identity():
    t = K.label_table_ids({3: -1, 4: 5, 5: 6, -1: 9, 256: 9, 300: 1, 7: 255})
    assert t.lut[3] == 255 and t.lut[7] == 255                                                 # -1 is stored as a uint8
    assert t.lut[4] == 5 and t.lut[5] == 6                                                     # original ids: 4 -> 5 does not go on to 6
    assert t.lut[0] == 0 and t.lut[255] == 255 and t.lut[44] == 44                             # keys outside 0..255 match nothing, the rest is the identity
    assert [i for i in range(256) if t.lut[i] != i] == [3, 4, 5, 7]
    empty = L.PmLabelTable()
    assert L.load().pm_label_table_ids(None, None, 0, ctypes.addressof(empty), ctypes.sizeof(empty)) == 0 and list(empty.lut) == list(range(256))


def test_colour_cap_collisions_and_duplicates():
    rng = np.random.default_rng(5)
    packed = rng.choice(1 << 24, size=129, replace=False)
    cols = [(int(p) & 255, (int(p) >> 8) & 255, int(p) >> 16) for p in packed]
    full = {c: i % 200 for i, c in enumerate(cols[:128])}
    t = K.label_table_colors(full, 255)                                                        # 128 colours in 256 slots: home slots collide
    homes = [(((c[0] | c[1] << 8 | c[2] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 24 for c in full]
    assert len(set(homes)) < 128
    for c, v in full.items():
        assert lookup(t, c) == v
    assert lookup(t, cols[128]) == 255
    with pytest.raises(L.PinmemError, match='PM_LABEL_MAX_COLORS'):
        K.label_table_colors({c: 1 for c in cols}, 255)
    lib, tab = L.load(), L.PmLabelTable()
    rgb, vals = (ctypes.c_int32 * (129 * 3))(*[v for c in cols for v in c]), (ctypes.c_int32 * 129)(*([1] * 129))
    assert lib.pm_label_table_colors(rgb, vals, 129, 255, ctypes.addressof(tab), ctypes.sizeof(tab)) == EUNSUPPORTED
    vals[5], vals[77] = 255, -1                                                                # dropped entries do not count
    assert lib.pm_label_table_colors(rgb, vals, 129, 255, ctypes.addressof(tab), ctypes.sizeof(tab)) == 0
    assert lookup(tab, cols[5]) == 255 and lookup(tab, cols[77]) == 255 and lookup(tab, cols[128]) == 1
    # a colour listed twice (the raw ABI can; a dict cannot): the last kept value stands, and it takes one slot
    rgb2, vals2 = (ctypes.c_int32 * 9)(1, 2, 3, 1, 2, 3, 1, 2, 3), (ctypes.c_int32 * 3)(4, 6, 255)
    assert lib.pm_label_table_colors(rgb2, vals2, 3, 255, ctypes.addressof(tab), ctypes.sizeof(tab)) == 0
    assert lookup(tab, (1, 2, 3)) == 6 and sum(1 for k in tab.keys if k != 0xFFFFFFFF) == 1
    assert K.label_table_colors({(300, 0, 0): 3, (0, -1, 0): 4, (9, 9, 9): 2}).keys[:].count(0xFFFFFFFF) == L.LABEL_SLOTS - 1      # no uint8 pixel equals them


def test_bad_arguments_are_refused():
    lib, tab = L.load(), L.PmLabelTable()
    size = ctypes.sizeof(tab)
    k, v = (ctypes.c_int32 * 2)(1, 2), (ctypes.c_int32 * 2)(3, 4)
    rgb = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    assert lib.pm_label_table_ids(k, v, 2, ctypes.addressof(tab), size - 4) == EINVAL and b'struct_size' in lib.pm_last_error()
    assert lib.pm_label_table_colors(rgb, v, 2, 255, ctypes.addressof(tab), size + 4) == EINVAL and b'struct_size' in lib.pm_last_error()
    assert lib.pm_label_table_ids(k, v, 2, None, size) == EINVAL
    assert lib.pm_label_table_ids(None, v, 2, ctypes.addressof(tab), size) == EINVAL
    assert lib.pm_label_table_ids(k, v, -1, ctypes.addressof(tab), size) == EINVAL
    assert lib.pm_label_table_colors(rgb, None, 2, 255, ctypes.addressof(tab), size) == EINVAL
    assert lib.pm_label_table_colors(rgb, v, 2, 255, None, size) == EINVAL
    assert lib.pm_label_table_colors(rgb, v, 2, 256, ctypes.addressof(tab), size) == EINVAL and b'fill' in lib.pm_last_error()
    # the device entry points turn the same things down before any launch (fake aligned pointers, no GPU here)
    P = 0x10000
    assert lib.pm_labels_decode_u8(P, 1, 4, 4, 3, 2 * P, 1, size - 4, 3 * P, 4 * P, None) == EINVAL and b'struct_size' in lib.pm_last_error()
    assert lib.pm_labels_decode_u8(P, 1, 4, 4, 2, 2 * P, 1, size, 3 * P, 4 * P, None) == EINVAL and b'channels' in lib.pm_last_error()
    assert lib.pm_labels_decode_u8(P, 1, 4, 4, 3, None, 1, size, 3 * P, 4 * P, None) == EINVAL
    assert lib.pm_labels_decode_u8(P, 1, 4, 4, 3, 2 * P, 1, size, None, 4 * P, None) == EINVAL
    assert lib.pm_labels_decode_u8(P, 1, 4, 4, 3, 2 * P, 1, size, 3 * P, P + 8, None) == EINVAL and b'overlaps' in lib.pm_last_error()
    geo = ctypes.sizeof(L.PmGeoImage)
    args = (P, 2 * P, 1, 8, 8, 3 * P, geo, 4 * P, 5 * P, 6 * P, 7 * P, 4, 4, 255)
    assert lib.pm_resample_crop_decode_u8(*args, 3, 8 * P, 1, size - 4, 9 * P, 10 * P, 11 * P, None) == EINVAL and b'pm_label_table struct_size' in lib.pm_last_error()
    assert lib.pm_resample_crop_decode_u8(*(args[:6] + (geo - 4,) + args[7:]), 3, 8 * P, 1, size, 9 * P, 10 * P, 11 * P, None) == EINVAL
    assert lib.pm_resample_crop_decode_u8(*args, 4, 8 * P, 1, size, 9 * P, 10 * P, 11 * P, None) == EINVAL and b'channels' in lib.pm_last_error()
    assert lib.pm_resample_crop_decode_u8(*args, 3, 8 * P, 1, size, None, 10 * P, 11 * P, None) == EINVAL


def test_label_decode_argument_validation(dicts):
    colors, city, synthia = dicts
    with pytest.raises(ValueError):
        input_edge.LabelDecode(ignore_index=256)
    dec = input_edge.LabelDecode()
    assert len(dec) == 0
    g, s, c = dec.add_colors(colors), dec.add_ids(synthia), dec.add_ids(city)
    assert (g, s, c) == (0, 1, 2) and len(dec) == 3 and dec.kinds == ['colors', 'ids', 'ids']
    for bad in ({}, [(1, 2, 3)], {(1, 2): 3}, {5: 3}, {(1, 2, 3): 'a'}, {(1.5, 2, 3): 1}):
        with pytest.raises((ValueError, TypeError)):
            dec.add_colors(bad)
    for bad in ({}, [1], {(1, 2, 3): 3}, {1.5: 2}, {1: 2.5}):
        with pytest.raises((ValueError, TypeError)):
            dec.add_ids(bad)
    assert len(dec) == 3
    assert dec.image_table([g, None, -1, s], 4, 3) == [0, -1, -1, 1]
    assert dec.image_table([s, c, None], 3, 1) == [1, 2, -1]
    with pytest.raises(ValueError, match='colour table'):
        dec.image_table([s, g], 2, 1)                                                          # a colour table needs the three channels
    with pytest.raises(ValueError):
        dec.image_table([3], 1, 3)
    with pytest.raises(ValueError):
        dec.image_table([-2], 1, 3)
    with pytest.raises(ValueError):
        dec.image_table([g], 2, 3)
    assert input_edge.domain_entries([g, s], (2, 2)) == [0, 1, 0, 1] and input_edge.domain_entries(None, (3,)) == [None] * 3
    with pytest.raises(ValueError):
        input_edge.domain_entries([g], (2, 2))
    assert input_edge.LabelDecode(ignore_index=7).add_colors({(1, 2, 3): 4}) == 0


def by_unique(raw, kind, table, fill=255, channels=None):
    """The decode with numpy: colours packed into one integer, np.unique, one dict lookup per DISTINCT value, scattered back through the inverse. raw: [.., 3] or,
    with channels=1, ids alone (default: an [H, W, 3] or [H, W] image)."""
    channels = channels or (3 if raw.ndim == 3 else 1)
    if kind is None:
        return raw[..., 0] if channels == 3 else raw
    if kind == 'ids':
        ids = raw[..., 0] if channels == 3 else raw
        u, inv = np.unique(ids, return_inverse=True)
        return np.array([np.uint8(table[int(k)] & 255) if int(k) in table else np.uint8(k) for k in u], dtype=np.uint8)[inv].reshape(ids.shape)
    if channels != 3:
        return np.full(raw.shape, fill, dtype=np.uint8)
    packed = raw[..., 0].astype(np.int64) << 16 | raw[..., 1].astype(np.int64) << 8 | raw[..., 2]
    keep = {k[0] << 16 | k[1] << 8 | k[2]: v for k, v in table.items() if v not in (255, -1)}
    u, inv = np.unique(packed, return_inverse=True)
    return np.array([keep.get(int(k), fill) for k in u], dtype=np.uint8)[inv].reshape(packed.shape)


def test_fixture_masks_reproduce_with_numpy_and_the_host_tables(dicts, golden):
    colors, city, synthia = dicts
    with golden('label_decode_cases.npz') as f:
        fx = {k: f[k] for k in f.files}
    assert np.array_equal(by_unique(fx['gtav_raw'], 'colors', colors), fx['gtav_want'])
    assert np.array_equal(by_unique(fx['synthia_raw'], 'ids', synthia), fx['synthia_want'])
    assert np.array_equal(by_unique(fx['city_raw'], 'ids', city), fx['city_want'])
    kinds = {-1: (None, None), 0: ('colors', colors), 1: ('ids', synthia)}
    for i, t in enumerate(fx['mixed_table']):
        assert np.array_equal(by_unique(fx['mixed_raw'][i], *kinds[int(t)]), fx['mixed_want'][i]), i
    # the fixture exercises what it is for: every kept class, ignored colours, +-1 neighbours of table colours, ids the tables change and ids they leave
    assert set(range(19)) <= set(fx['gtav_want'].ravel().tolist()) and (fx['gtav_want'] == 255).sum() > 400
    assert fx['gtav_raw'].shape == (24, 40, 3) and max(fx[k].shape[0] for k in ('gtav_raw', 'synthia_raw', 'city_raw')) <= 64
    assert len(np.unique(fx['synthia_raw'])) == 256 and len(np.unique(fx['city_raw'])) == 256
    # and the library's host tables, walked as the header says, give the same masks
    tc = K.label_table_colors(colors, 255)
    assert np.array_equal(np.array([lookup(tc, [int(v) for v in px]) for px in fx['gtav_raw'].reshape(-1, 3)], dtype=np.uint8).reshape(24, 40), fx['gtav_want'])
    ts = K.label_table_ids(synthia)
    assert np.array_equal(np.array(list(ts.lut), dtype=np.uint8)[fx['synthia_raw']], fx['synthia_want'])
