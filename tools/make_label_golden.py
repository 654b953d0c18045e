"""Fixtures of the label-decoding input edge (csrc/resample.hip pm_label_table_* / pm_labels_decode_u8 / pm_resample_crop_decode_u8, input_edge.LabelDecode).

    python tools/make_label_golden.py            # writes tests/golden/label_tables.json and label_decode_cases.npz (needs the reference tree)
    python tools/make_label_golden.py --check    # regenerates in memory and compares with the committed files

label_tables.json: the three dicts of the reference's datasets AS PYTHON EVALUATES THEM, as lists of numbers -- data, no program text is copied:
  color2trainId [[r, g, b, v], ...] and label2trainid [[k, v], ...] of datasets/cityscapes_labels.py, loaded by file path (its only import is namedtuple);
  trainid_to_trainid [[k, v], ...] of datasets/synthia.py, whose dict literal is cut out of the file and read with ast.literal_eval after `ignore_label` is replaced
  by the module's own `ignore_label = <number>` line (the module itself imports the datasets' whole dependency chain).
A dict holds a colour once: where two labels share a colour the later one stands, which the JSON records as it is.

label_decode_cases.npz: a few raw masks of at most 64 x 64 and their decoded form, the expectation from decode_expected() below -- a per-pixel Python dict lookup
written from the semantics in include/pinmem_hip.h (colour tables: gtav.py:440-445; id tables: synthia.py:254-257), not from the library:
  gtav_raw u8 [H,W,3] / gtav_want u8 [H,W]: every table colour, every +-1 neighbour per channel of every table colour, and seeded random colours;
  synthia_raw u8 [H,W] / synthia_want, city_raw / city_want: every id 0..255 and seeded random ids through trainid_to_trainid / label2trainid;
  mixed_raw u8 [3,H,W,3] / mixed_want u8 [3,H,W] / mixed_table [3]: one batch of a pass-through image (-1), an id image (its id in channel 0, table 1 = synthia) and
  a colour image (table 0 = gtav)."""
import ast
import importlib.util
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLES = os.path.join(ROOT, 'tests', 'golden', 'label_tables.json')
CASES = os.path.join(ROOT, 'tests', 'golden', 'label_decode_cases.npz')
IGNORE = 255


def reference_tables():
    from oracle.import_reference import REF
    path = os.path.join(REF, 'datasets', 'cityscapes_labels.py')
    spec = importlib.util.spec_from_file_location('cityscapes_labels', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(REF, 'datasets', 'synthia.py')) as f:
        text = f.read()
    ignore = int(re.search(r'^ignore_label\s*=\s*(\d+)\s*$', text, flags=re.M).group(1))
    literal = re.search(r'^trainid_to_trainid\s*=\s*(\{.*?\})', text, flags=re.M | re.S).group(1)
    synthia = ast.literal_eval(re.sub(r'\bignore_label\b', str(ignore), literal))
    return dict(color2trainId=[[int(c) for c in k] + [int(v)] for k, v in mod.color2trainId.items()],
                label2trainid=[[int(k), int(v)] for k, v in mod.label2trainid.items()],
                trainid_to_trainid=[[int(k), int(v)] for k, v in synthia.items()])


def dumps(tables):
    return json.dumps(tables, indent=0, separators=(',', ':')).replace('\n', '') + '\n'


def decode_expected(raw, kind, table, fill=IGNORE):
    """Pixel by pixel. kind 'colors': table {(r, g, b): v}; 'ids': {k: v}; None: channel 0."""
    raw = np.asarray(raw)
    h, w = raw.shape[:2]
    out = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            px = raw[y, x]
            if kind is None:
                out[y, x] = px[0] if raw.ndim == 3 else px
            elif kind == 'ids':
                k = int(px[0] if raw.ndim == 3 else px)
                out[y, x] = table[k] & 255 if k in table else k
            else:
                v = table.get(tuple(int(c) for c in px), fill) if raw.ndim == 3 else fill
                out[y, x] = fill if v in (255, -1) else v & 255
    return out


def as_dicts(tables):
    return ({tuple(r[:3]): r[3] for r in tables['color2trainId']}, {k: v for k, v in tables['label2trainid']}, {k: v for k, v in tables['trainid_to_trainid']})


def color_probe_set(colors, rng, total):
    """every table colour, its +-1 neighbours per channel (inside 0..255), then random colours up to `total` pixels"""
    px = [list(c) for c in colors]
    for c in colors:
        for ch in range(3):
            for d in (-1, 1):
                n = list(c)
                n[ch] += d
                if 0 <= n[ch] <= 255:
                    px.append(n)
    px = np.array(px, dtype=np.uint8)
    assert len(px) <= total
    return np.concatenate([px, rng.integers(0, 256, size=(total - len(px), 3), dtype=np.uint8)])


def cases(tables):
    colors, city, synthia = as_dicts(tables)
    rng = np.random.default_rng(20)
    out = {}
    out['gtav_raw'] = color_probe_set(list(colors), rng, 24 * 40).reshape(24, 40, 3)
    out['gtav_want'] = decode_expected(out['gtav_raw'], 'colors', colors)
    ids = np.concatenate([np.arange(256, dtype=np.uint8), rng.integers(0, 40, size=16 * 35 - 256, dtype=np.uint8)])
    out['synthia_raw'] = rng.permutation(ids).reshape(16, 35)
    out['synthia_want'] = decode_expected(out['synthia_raw'], 'ids', synthia)
    out['city_raw'] = rng.permutation(ids).reshape(35, 16)
    out['city_want'] = decode_expected(out['city_raw'], 'ids', city)
    h, w = 37, 53
    mixed = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
    mixed[0, :, :, 0] = rng.integers(0, 20, size=(h, w))
    mixed[1, :, :, 0] = rng.integers(0, 30, size=(h, w))
    pool = color_probe_set(list(colors), rng, 400)
    mixed[2] = pool[rng.integers(0, len(pool), size=(h, w))]
    out['mixed_raw'] = mixed
    out['mixed_table'] = np.array([-1, 1, 0], dtype=np.int32)
    out['mixed_want'] = np.stack([decode_expected(mixed[0], None, None), decode_expected(mixed[1], 'ids', synthia), decode_expected(mixed[2], 'colors', colors)])
    return out


if __name__ == '__main__':
    tables = reference_tables()
    made = cases(tables)
    if '--check' in sys.argv:
        with open(TABLES) as f:
            assert f.read() == dumps(tables), 'label_tables.json differs from the reference tree'
        with np.load(CASES) as f:
            assert sorted(f.files) == sorted(made) and all(np.array_equal(f[k], made[k]) for k in made), 'label_decode_cases.npz differs'
        print('fixtures match')
    else:
        with open(TABLES, 'w') as f:
            f.write(dumps(tables))
        np.savez_compressed(CASES, **made)
        print('wrote', TABLES, CASES)
