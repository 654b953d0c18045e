"""CPU oracle of the device-side photometric augmentation (csrc/augment.hip): the host pipeline of the reference's training scripts -- torchvision 0.10's
ColorJitter on PIL images (ImageEnhance.Brightness / Contrast / Color, the HSV round trip of adjust_hue), skimage 0.16's gaussian(multichannel=True) restated with
scipy (float64, x / 255.0, truncate 4.0, mode 'nearest', H then W, `(y * 255).astype(uint8)`), a horizontal flip -- applied with PIL and scipy alone to a few
small uint8 images, each result quantised to uint8 after every step exactly as the host pipeline does. Nothing is imported from the reference.

    python tools/make_augment_golden.py            # writes tests/golden/augment_cases.npz
    python tools/make_augment_golden.py --check    # regenerates in memory and compares with the committed file

Per case K the file holds K_img [n,H,W,3] u8, K_order [n,4] u8 (torchvision's op ids: 0 brightness, 1 contrast, 2 saturation, 3 hue), K_enabled [n] u8 (bit per op id),
K_flip [n] u8, K_factors [n,3] f64 (brightness, contrast, saturation), K_hue [n] f64 (hue factor), K_sigma [n] f64 (0: no blur), and the expected bytes K_colour
(after the colour ops and the flip) and K_blur (after the blur as well).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'augment_cases.npz')

FACTORS = (0.0, 0.2, 0.73, 1.0, 1.4, 1.8)            # both blend branches (0 <= f <= 1 truncates, f > 1 clips) and both clip sides
HUES = (-0.5, -0.3, -0.004, 0.05, 0.3, 0.5)
SIGMAS = (0.15, 0.4, 0.77, 1.0, 1.3)                 # radius 1 .. 5
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
ALL = 15


def hue_shift(hue_factor):
    """np.uint8(hue_factor * 255) of torchvision 0.10's adjust_hue under the numpy it was written for: truncated toward zero, wrapped to a byte."""
    return int(hue_factor * 255) & 255


def colour_ops(arr, order, enabled, factors, hue):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(arr), 'RGB')
    for op in order:
        if not (int(enabled) >> int(op)) & 1:
            continue
        if op == BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(factors[0]))
        elif op == CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(factors[1]))
        elif op == SATURATION:
            im = ImageEnhance.Color(im).enhance(float(factors[2]))
        else:
            h, s, v = im.convert('HSV').split()
            h = ((np.array(h, dtype=np.uint8).astype(np.int32) + hue_shift(float(hue))) & 255).astype(np.uint8)
            im = Image.merge('HSV', (Image.fromarray(h, 'L'), s, v)).convert('RGB')
    return np.array(im, dtype=np.uint8)


def blur(arr, sigma):
    from scipy.ndimage import gaussian_filter
    if sigma <= 0:
        return arr.copy()
    x = arr / 255.0
    y = np.stack([gaussian_filter(x[..., c], sigma, mode='nearest', truncate=4.0) for c in range(3)], axis=-1)
    return (y * 255).astype(np.uint8)


def blur_weights(sigma):
    """scipy.ndimage's _gaussian_kernel1d (order 0): radius and the weights centre .. one side."""
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (h + w - 2)], axis=-1).astype(np.uint8)


def _extremes(h, w, rng):
    vals = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    img = vals[rng.integers(0, 6, size=(h, w, 3))]
    img[:, : w // 2] = img[:, : w // 2, :1]          # the left half is grey: H = S = 0, the hue shift must leave it alone
    return img


def cases():
    """name -> dict of the input arrays (see the module docstring)."""
    rng = np.random.default_rng(20240607)

    def rand(n, h, w):
        return rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)

    def pack(img, rows):
        # rows: (order, enabled, flip, (b, c, s), hue, sigma) per image
        return dict(img=img, order=np.array([r[0] for r in rows], dtype=np.uint8), enabled=np.array([r[1] for r in rows], dtype=np.uint8),
                    flip=np.array([r[2] for r in rows], dtype=np.uint8), factors=np.array([r[3] for r in rows], dtype=np.float64),
                    hue=np.array([r[4] for r in rows], dtype=np.float64), sigma=np.array([r[5] for r in rows], dtype=np.float64))

    out = {}
    # (a) smaller than the blur radius in both directions: the clamped indices repeat
    out['a'] = pack(rand(1, 7, 9), [((2, 0, 3, 1), ALL, 1, (1.4, 0.2, 1.8), -0.3, 1.3)])
    # (b) per-image order and flags inside one launch: nothing at all | blur only | everything
    out['b'] = pack(rand(3, 37, 53), [((0, 1, 2, 3), 0, 0, (1.0, 1.0, 1.0), 0.0, 0.0),
                                      ((0, 1, 2, 3), 0, 0, (1.0, 1.0, 1.0), 0.0, 0.4),
                                      ((3, 1, 0, 2), ALL, 1, (0.73, 1.4, 0.2), 0.05, 0.77)])
    # (c) crosses tile boundaries in both directions: smooth ramp | extreme and grey values
    out['c'] = pack(np.stack([_ramp(70, 150), _extremes(70, 150, rng)]), [((0, 1, 2, 3), ALL, 0, (1.8, 0.73, 1.4), 0.5, 1.0),
                                                                          ((1, 3, 2, 0), ALL, 1, (0.2, 1.8, 0.0), -0.5, 0.15)])
    # (d) contrast third: the grey sum depends on two preceding ops
    out['d'] = pack(rand(1, 67, 93), [((2, 3, 1, 0), ALL, 0, (1.0, 0.0, 0.73), 0.3, 0.77)])
    # (e) the remaining factor / hue / sigma values, partly enabled op sets, every op in every position
    out['e'] = pack(rand(6, 5, 11), [((0, 2, 1, 3), ALL, 0, (0.0, 1.0, 1.0), -0.004, 0.15),
                                     ((1, 0, 3, 2), ALL, 1, (0.2, 0.2, 0.2), 0.3, 0.4),
                                     ((3, 2, 0, 1), 1 << HUE | 1 << CONTRAST, 0, (1.4, 1.8, 1.4), -0.5, 1.3),
                                     ((2, 1, 3, 0), 1 << SATURATION | 1 << BRIGHTNESS, 1, (1.8, 1.4, 1.8), 0.5, 1.0),
                                     ((1, 2, 3, 0), 1 << CONTRAST, 0, (1.0, 0.73, 0.0), 0.05, 0.0),
                                     ((3, 0, 2, 1), 1 << HUE, 1, (0.73, 0.0, 1.0), -0.3, 0.77)])
    return out


def generate():
    """Every array of the fixture, keyed as in the file."""
    arrays = {}
    for name, c in cases().items():
        colour, blurred = [], []
        for i in range(c['img'].shape[0]):
            x = colour_ops(c['img'][i], c['order'][i], c['enabled'][i], c['factors'][i], c['hue'][i])
            y = blur(x, float(c['sigma'][i]))
            if c['flip'][i]:
                x, y = x[:, ::-1], y[:, ::-1]
            colour.append(x)
            blurred.append(y)
        for k, v in c.items():
            arrays['%s_%s' % (name, k)] = v
        arrays[name + '_colour'] = np.stack(colour)
        arrays[name + '_blur'] = np.stack(blurred)
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
