"""CPU: what tests/test_sliding_eval.py leans on -- the tile tables of harness.sliding_tiles cover every pixel of its geometries, the numpy restatement of
cv2.resize(INTER_LINEAR) for float64 (the contract of the multi-scale path; cv2 itself is not a dependency of this repository, so bit-equality with cv2 is not
checked anywhere) gives the identity at ratio 1 and the border values worked out by hand -- and the entry points of the sliding-window evaluation are exported
and refuse bad arguments before touching the device (no compute calls here)."""
import ctypes

import numpy as np

from pinthememory_amd.hip import lib as L

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4

# (H, W, crop, overlap, low-res ratio): one tile; odd W, ragged last tile, 4 covers and more; 9 covers and more; 72 tiles; clamped tiles with th != tw
GEOMETRIES = [(12, 12, 12, 1.0 / 3, 4), (20, 37, 12, 1.0 / 3, 4), (23, 31, 12, 2.0 / 3, 3), (64, 128, 16, 1.0 / 3, 4), (10, 24, 16, 1.0 / 3, 4)]
# (H, W, crop, scales)
MULTI = [(24, 40, 16, (0.5, 1.0, 2.0)), (21, 35, 12, (0.75, 1.0))]


def cover_count(tiles, h, w):
    cnt = np.zeros((h, w), dtype=np.int64)
    for x1, y1, x2, y2 in tiles:
        cnt[y1:y2, x1:x2] += 1
    return cnt


def cv2_taps(D, S):
    """One axis of cv2.resize(INTER_LINEAR), S source -> D destination samples: f = float((d + 0.5) * (double(S) / D) - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0;
    s >= S - 1: s = S - 1, f = 0 (one tap of weight 1). -> (i0, i1, w0, w1) with float32 weights 1.f - f and f."""
    d = np.arange(D, dtype=np.float64)
    f = ((d + 0.5) * (np.float64(S) / np.float64(D)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= S - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = S - 1, 0
    return s, np.minimum(s + 1, S - 1), (np.float32(1) - f).astype(np.float32), f


def cv2_linear(a, H, W):
    """cv2.resize(a, (W, H), interpolation=cv2.INTER_LINEAR) of float64 [..., S_h, S_w] restated: horizontal a * w0 + b * w1 in double, then vertical the same way."""
    a = np.asarray(a, dtype=np.float64)
    y0, y1, wy0, wy1 = cv2_taps(H, a.shape[-2])
    x0, x1, wx0, wx1 = cv2_taps(W, a.shape[-1])
    h = a[..., :, x0] * wx0.astype(np.float64) + a[..., :, x1] * wx1.astype(np.float64)
    return h[..., y0, :] * wy0.astype(np.float64)[:, None] + h[..., y1, :] * wy1.astype(np.float64)[:, None]


def test_tile_tables_cover_every_pixel():
    from pinthememory_amd import harness
    for H, W, crop, overlap, _ in GEOMETRIES:
        tiles = harness.sliding_tiles(H, W, crop, overlap)
        cnt = cover_count(tiles, H, W)
        assert cnt.min() >= 1 and len({(x2 - x1, y2 - y1) for x1, y1, x2, y2 in tiles}) == 1
        assert all(0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H for x1, y1, x2, y2 in tiles)
    tiles = harness.sliding_tiles(64, 128, 16, 1.0 / 3)
    assert len(tiles) == 72                                                       # past the 64 tiles pm_sliding_stitch takes
    assert cover_count(harness.sliding_tiles(23, 31, 12, 2.0 / 3), 23, 31).max() >= 9      # 3 x 3 from the stride of a third, more where the clamped last tiles fall
    assert cover_count(harness.sliding_tiles(20, 37, 12, 1.0 / 3), 20, 37).max() >= 4
    x1, y1, x2, y2 = harness.sliding_tiles(10, 24, 16, 1.0 / 3)[0]
    assert (y2 - y1, x2 - x1) == (10, 16)                                         # clamped to the image: th != tw
    for H, W, crop, scales in MULTI:
        for s in scales:
            Hs, Ws = int(H * s), int(W * s)
            tiles = harness.sliding_tiles(Hs, Ws, crop, 1.0 / 3, s)
            assert len(tiles) >= 1 and cover_count(tiles, Hs, Ws).min() >= 1
            assert len({(x2 - x1, y2 - y1) for x1, y1, x2, y2 in tiles}) == 1


def test_cv2_linear_is_the_identity_at_ratio_one():
    a = np.random.default_rng(0).standard_normal((3, 7, 11))
    assert np.array_equal(cv2_linear(a, 7, 11), a)
    i0, i1, w0, w1 = cv2_taps(11, 11)
    assert np.array_equal(i0, np.arange(11)) and np.all(w0 == 1) and np.all(w1 == 0)


def test_cv2_linear_border_values_by_hand():
    """2 -> 4 samples: f = -0.25, 0.25, 0.75, 1.25 -> the first sample clamps to a[0], the last to a[1]. 4 -> 2: f = 0.5, 2.5 -> midpoints of (a0, a1) and (a2, a3).
    3 -> 2: f = 0.25, 1.75 -> 0.75 a0 + 0.25 a1 and 0.25 a1 + 0.75 a2."""
    assert np.array_equal(cv2_linear(np.array([[0.0, 4.0]]), 1, 4), [[0.0, 1.0, 3.0, 4.0]])
    assert np.array_equal(cv2_linear(np.array([[0.0, 2.0, 4.0, 10.0]]), 1, 2), [[1.0, 7.0]])
    assert np.array_equal(cv2_linear(np.array([[0.0, 4.0, 8.0]]), 1, 2), [[1.0, 7.0]])
    assert np.array_equal(cv2_linear(np.array([[0.0], [4.0]]), 4, 1), [[0.0], [1.0], [3.0], [4.0]])      # the vertical pass alike
    assert np.array_equal(cv2_linear(np.array([[5.0]]), 3, 2), np.full((3, 2), 5.0))                       # one source sample: weight 1 everywhere
    i0, i1, w0, w1 = cv2_taps(4, 2)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and w1.tolist() == [0.0, 0.25, 0.75, 0.0] and w0.dtype == np.float32


# ---- the entry points, without a device -----------------------------------------------------------------------------------------------------------------------
def rejections(lib, logits, labels, hist, pred, out, acc, ws, stream=None):
    """Every refusal include/pinmem_hip.h lists for pm_sliding_eval / pm_sliding_eval_finish, each with its status; the pointers are whatever the caller has (host
    arrays here, device memory in tests/test_sliding_eval.py -- no call below gets as far as a launch). 2 x 2 tiles of 8 x 8 on a 12 x 12 image, 2 x 2 logits."""
    tiles = [(0, 0, 8, 8), (0, 4, 8, 12), (4, 0, 12, 8), (4, 4, 12, 12)]

    def table(ts):
        return (ctypes.c_int32 * (4 * len(ts)))(*[v for t in ts for v in t])

    def call(logits=logits, n=8, C=19, flips=2, ts=tiles, nt=None, hw=(12, 12), HW=(12, 12), labels=labels, hist=hist, accumulate=0, pred=pred, out=None, acc=None,
             ws=ws, nb=None):
        nt = len(ts) if nt is None else nt
        nb = lib.pm_sliding_eval_workspace(nt, min(max(C, 1), 32), HW[0], HW[1]) if nb is None else nb
        return lib.pm_sliding_eval(logits, n, 2, 2, C, 20, flips, table(ts) if ts else None, nt, hw[0], hw[1], HW[0], HW[1], labels, hist, accumulate, pred, out, acc, 0,
                                   ws, nb, stream)

    need = lib.pm_sliding_eval_workspace(4, 19, 12, 12)
    assert need > 0 and need % 256 == 0 and need >= 4 * 16 + 361 * 4
    assert lib.pm_sliding_eval_workspace(4, 33, 12, 12) == 0 and lib.pm_sliding_eval_workspace(4, 0, 12, 12) == 0 and lib.pm_sliding_eval_workspace(-1, 19, 12, 12) == 0
    assert call(logits=None) == EINVAL and b'sliding_eval' in lib.pm_last_error()
    assert call(ts=None, nt=4) == EINVAL
    assert call(hist=None) == EINVAL                                                       # labels without a histogram
    assert call(labels=None, hist=None, pred=None) == EINVAL                               # nothing to write
    for flips in (0, 3):
        assert call(flips=flips, n=flips * 4) == EINVAL and b'flips' in lib.pm_last_error()
    assert call(n=4) == EINVAL                                                             # logits of one flip for two
    assert call(accumulate=2) == EINVAL
    for C in (0, 33):
        assert call(C=C) == EUNSUPPORTED and b'classes' in lib.pm_last_error()
    assert call(ts=tiles[:3] + [(4, 4, 12, 13)]) == EINVAL and b'tile 3' in lib.pm_last_error()      # leaves the image (and is 9 rows high)
    assert call(ts=tiles[:3] + [(5, 4, 12, 12)]) == EINVAL and b'tile 3' in lib.pm_last_error()      # another size than tile 0
    assert call(ts=[(-1, 0, 7, 8)] + tiles[1:]) == EINVAL and b'tile 0' in lib.pm_last_error()
    assert call(ts=tiles[:3], n=6) == EINVAL and b'uncovered' in lib.pm_last_error()                  # the lower right corner has no tile
    assert call(ts=[(0, 0, 8, 8), (4, 4, 12, 12)], n=4) == EINVAL and b'uncovered' in lib.pm_last_error()
    assert call(hw=(12, 12), HW=(24, 24)) == EINVAL and b'accumulator' in lib.pm_last_error()         # another scale without the accumulator
    assert call(acc=acc) == EINVAL                                                         # an accumulator together with labels / hist / pred
    assert call(nb=need - 1) == EWORKSPACE and b'workspace' in lib.pm_last_error()
    assert call(ws=None) == EWORKSPACE
    assert call(labels=None, hist=None, pred=None, acc=acc, nb=need - 1) == EWORKSPACE

    def finish(acc=acc, C=19, ns=2, labels=labels, hist=hist, accumulate=0, pred=pred, ws=ws, nb=None):
        nb = lib.pm_sliding_eval_workspace(0, min(max(C, 1), 32), 12, 12) if nb is None else nb
        return lib.pm_sliding_eval_finish(acc, C, 12, 12, ns, labels, hist, accumulate, pred, None, ws, nb, stream)

    assert finish(acc=None) == EINVAL and b'sliding_eval_finish' in lib.pm_last_error()
    assert finish(C=33) == EUNSUPPORTED
    assert finish(ns=0) == EINVAL and finish(accumulate=2) == EINVAL
    assert finish(hist=None) == EINVAL and finish(labels=None, hist=None, pred=None) == EINVAL
    assert finish(nb=lib.pm_sliding_eval_workspace(0, 19, 12, 12) - 1) == EWORKSPACE and finish(ws=None) == EWORKSPACE


def test_library_exports_the_sliding_evaluation_entry_points():
    lib = L.load()
    for name in ('pm_sliding_eval', 'pm_sliding_eval_finish', 'pm_sliding_eval_workspace'):
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_bad_arguments_are_refused_without_a_gpu():
    lib = L.load()
    logits, labels, hist = (ctypes.c_float * (8 * 2 * 2 * 20))(), (ctypes.c_int64 * 144)(), (ctypes.c_int64 * 1024)()
    pred, out, ws = (ctypes.c_uint8 * 144)(), (ctypes.c_double * (19 * 144))(), (ctypes.c_char * (1 << 16))()
    rejections(lib, logits, labels, hist, pred, out, out, ws)
    assert not any(hist) and not any(pred)


def test_workspace_query_for_one_cityscapes_image():
    """16 tiles at crop 768, 72 at crop 256: the table is part of the workspace, so there is no tile ceiling; one row of C x C counters per block."""
    lib = L.load()
    a, b = lib.pm_sliding_eval_workspace(16, 19, 1024, 2048), lib.pm_sliding_eval_workspace(72, 19, 1024, 2048)
    assert a % 256 == 0 and b - a == (72 * 16 + 255) // 256 * 256 - 256 and a >= 16 * 16 + 361 * 4
    assert lib.pm_sliding_eval_workspace(100000, 19, 1024, 2048) - a == 100000 * 16 - 256 + (-100000 * 16) % 256
