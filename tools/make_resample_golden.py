"""CPU oracle of the device-side resize + pad + crop (csrc/resample.hip): joint_transforms.RandomSizeAndCrop with its RandomCrop, restated with PIL alone for FIXED
draws -- `img.resize((w, h), Image.BICUBIC)`, `mask.resize((w, h), Image.NEAREST)` with w, h = int(W * s), int(H * s), ImageOps.expand by (t - size) // 2 + 1 on both
sides of an axis shorter than the crop (image 0, mask 255), then `crop((x1, y1, x1 + tw, y1 + th))` -- on a few small uint8 images. Nothing is imported from the
reference; PIL and numpy only.

    python tools/make_resample_golden.py            # writes tests/golden/resample_cases.npz
    python tools/make_resample_golden.py --check    # regenerates in memory and compares with the committed file

The file holds the sources srcK_img [H,W,3] u8 / srcK_lab [H,W] u8 (train ids 0..18 and 255) and per case C: C_src [n] (source index per image), C_scale [n] f64
(the scale_amt that was applied), C_crop [2] (th, tw), C_geo [n,8] i32 (h_in, w_in, h, w, pad_h, pad_w, y1, x1: the fields of pm_geo_image), and the expected crops
C_img [n,th,tw,3] u8 and C_lab [n,th,tw] u8.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'resample_cases.npz')

SCALES = (0.5, 0.613, 0.77, 1.0, 1.31, 1.999, 2.0)
IGNORE = 255
SIZES = ((52, 97), (64, 128), (97, 161), (64, 128))      # the last one is the smooth ramp
RAMP = 3
TILE = (32, 64)                                          # the kernel's output tile (csrc/resample.hip TH, TW): `big` and `pad2` are larger in both axes, no multiple


def sources():
    rng = np.random.default_rng(20240911)
    out = []
    for k, (h, w) in enumerate(SIZES):
        if k == RAMP:
            y, x = np.mgrid[0:h, 0:w]
            img = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (h + w - 2)], axis=-1).astype(np.uint8)
        else:
            img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 20, size=(h, w)).astype(np.uint8)
        lab[lab == 19] = IGNORE
        out.append((img, lab))
    return out


def geometry(size, scale, crop, origin):
    """(h_in, w_in, h, w, pad_h, pad_w, y1, x1) of RandomSizeAndCrop(crop_nopad=False) for a fixed scale_amt; origin 'zero' | 'max' | 'mid' picks the crop position."""
    (H, W), (th, tw) = size, crop
    w, h = int(W * scale), int(H * scale)
    pad_h = (th - h) // 2 + 1 if th > h else 0
    pad_w = (tw - w) // 2 + 1 if tw > w else 0
    max_y, max_x = h + 2 * pad_h - th, w + 2 * pad_w - tw
    y1, x1 = {'zero': (0, 0), 'max': (max_y, max_x), 'mid': (max_y // 3, (2 * max_x + 2) // 3)}[origin]
    return (H, W, h, w, pad_h, pad_w, y1, x1)


def pil_crop(img, lab, geo, crop):
    """What the host pipeline returns for this geometry: (image crop [th,tw,3], mask crop [th,tw])."""
    from PIL import Image, ImageOps
    H, W, h, w, pad_h, pad_w, y1, x1 = (int(v) for v in geo)
    th, tw = crop
    assert img.shape[:2] == (H, W) and lab.shape == (H, W)
    im = Image.fromarray(np.ascontiguousarray(img), 'RGB').resize((w, h), Image.BICUBIC)
    mk = Image.fromarray(np.ascontiguousarray(lab), 'L').resize((w, h), Image.NEAREST)
    if pad_h or pad_w:
        border = (pad_w, pad_h, pad_w, pad_h)
        im = ImageOps.expand(im, border=border, fill=(0, 0, 0))
        mk = ImageOps.expand(mk, border=border, fill=IGNORE)
    box = (x1, y1, x1 + tw, y1 + th)
    assert x1 >= 0 and y1 >= 0 and box[2] <= im.size[0] and box[3] <= im.size[1], 'the crop leaves the padded image'
    return np.array(im.crop(box), dtype=np.uint8), np.array(mk.crop(box), dtype=np.uint8)


def cases():
    """name -> (crop, [(source index, scale_amt, origin)])."""
    origins = ('zero', 'max', 'mid')
    out = {}
    # every scale, square and non-square windows, the three origins in turn; at 0.5 the resized image still holds the window
    out['sq'] = ((20, 20), [(0, s, origins[i % 3]) for i, s in enumerate(SCALES)])
    out['ns'] = ((16, 33), [(1, s, origins[(i + 1) % 3]) for i, s in enumerate(SCALES)])
    # pre_size 48 on the shorter edge (97) times a drawn 1.31
    out['pre'] = ((20, 20), [(2, 48 / 97 * 1.31, 'mid')])
    # 64 x 128 -> 32 x 64 under a 38 x 33 window: rows padded by (38 - 32) // 2 + 1 = 4, columns not
    out['pad1'] = ((38, 33), [(1, 0.5, 'zero'), (1, 0.5, 'max')])
    # 52 x 97 -> 26 x 48 under 45 x 83: both axes padded, by 10 and 18; more than one kernel tile each way
    out['pad2'] = ((45, 83), [(0, 0.5, 'max')])
    # more than one kernel tile each way inside the image, shrinking and enlarging
    out['big'] = ((37, 71), [(2, 0.613, 'mid'), (2, 1.31, 'mid')])
    # two images of different sizes in one batch: 52 x 97 in the corner of a 97 x 161 slab next to one that fills it
    out['mixed'] = ((20, 20), [(0, 0.77, 'max'), (2, 1.31, 'max')])
    # the smooth ramp: neighbouring taps nearly cancel, every rounding step shows
    out['ramp'] = ((16, 33), [(RAMP, 0.77, 'mid'), (RAMP, 1.999, 'max')])
    return out


def generate():
    """Every array of the fixture, keyed as in the file."""
    src = sources()
    arrays = {}
    for k, (img, lab) in enumerate(src):
        arrays['src%d_img' % k], arrays['src%d_lab' % k] = img, lab
    for name, (crop, rows) in cases().items():
        geo = [geometry(SIZES[k], s, crop, o) for k, s, o in rows]
        got = [pil_crop(src[k][0], src[k][1], g, crop) for (k, _, _), g in zip(rows, geo)]
        arrays[name + '_src'] = np.array([k for k, _, _ in rows], dtype=np.int32)
        arrays[name + '_scale'] = np.array([s for _, s, _ in rows], dtype=np.float64)
        arrays[name + '_crop'] = np.array(crop, dtype=np.int32)
        arrays[name + '_geo'] = np.array(geo, dtype=np.int32)
        arrays[name + '_img'] = np.stack([g[0] for g in got])
        arrays[name + '_lab'] = np.stack([g[1] for g in got])
    return arrays


def main():
    arrays = generate()
    if '--check' in sys.argv:
        with np.load(FIXTURE) as f:
            assert sorted(f.files) == sorted(arrays), 'key sets differ'
            bad = [k for k in arrays if not (f[k].dtype == arrays[k].dtype and np.array_equal(f[k], arrays[k]))]
        print('differs: %s' % bad if bad else 'identical: %d arrays' % len(arrays))
        sys.exit(1 if bad else 0)
    np.savez_compressed(FIXTURE, **arrays)
    print('wrote %s: %d bytes' % (FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == '__main__':
    main()
