"""CPU oracle of the device-side image scaling of sliding-window evaluation (csrc/resample.hip, pm_eval_tiles_u8): eval.py:357-358 restated with PIL alone --
`img.resize((int(w * scale), int(h * scale)), Image.BILINEAR)` -- on a few small uint8 images. Nothing is imported from the reference; PIL and numpy only.

    python tools/make_eval_scale_golden.py            # writes tests/golden/eval_scale_cases.npz
    python tools/make_eval_scale_golden.py --check    # regenerates in memory and compares with the committed file

The file holds the sources srcK [H,W,3] u8 and per case N = 0, 1, ...: caseN_src (source index), caseN_scale (f64) and caseN_img [int(H*s), int(W*s), 3] u8, the
scaled image. Widths 97, 161 and 37 give source rows whose byte length is no multiple of 4, and odd scaled widths.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'eval_scale_cases.npz')
LIMIT = 512 * 1024

SIZES = ((52, 97), (64, 128), (97, 161), (64, 128), (20, 37))      # the fourth one is the smooth ramp of the resample fixture
RAMP = 3
# (source index, scales); 64 x 128 random at 2.0 would take the file past LIMIT (random bytes do not compress) and is left out: 52 x 97 covers that scale
CASES = ((0, (0.25, 0.5, 0.613, 0.75, 1.0, 1.31, 2.0)), (1, (0.5,)), (2, (0.613, 1.31)), (RAMP, (0.77, 1.999)), (4, (0.25, 4.0)))


def sources():
    rng = np.random.default_rng(20250318)
    out = []
    for k, (h, w) in enumerate(SIZES):
        if k == RAMP:
            y, x = np.mgrid[0:h, 0:w]
            out.append(np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (h + w - 2)], axis=-1).astype(np.uint8))
        else:
            out.append(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    return out


def cases():
    """[(source index, scale)] in the file's order."""
    return [(k, s) for k, scales in CASES for s in scales]


def pil_scaled(img, scale):
    """eval.py:357-358 for one image."""
    from PIL import Image
    h, w = img.shape[:2]
    return np.array(Image.fromarray(np.ascontiguousarray(img), 'RGB').resize((int(w * scale), int(h * scale)), Image.BILINEAR), dtype=np.uint8)


def generate():
    """Every array of the fixture, keyed as in the file."""
    src = sources()
    arrays = {'src%d' % k: img for k, img in enumerate(src)}
    for n, (k, s) in enumerate(cases()):
        arrays['case%d_src' % n] = np.array(k, dtype=np.int32)
        arrays['case%d_scale' % n] = np.array(s, dtype=np.float64)
        arrays['case%d_img' % n] = pil_scaled(src[k], s)
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
    size = os.path.getsize(FIXTURE)
    assert size < LIMIT, '%d bytes: drop the 64 x 128 @ 2.0 case' % size
    print('wrote %s: %d bytes' % (FIXTURE, size))


if __name__ == '__main__':
    main()
