"""Shared by tests/test_eval_dump_cpu.py and tests/test_eval_dump.py: the byte rules of the evaluation image dumps (include/pinmem_hip.h, pm_eval_dump) restated in
numpy, the seeded inputs and the case list. The palette and the label table are data of this file."""
import numpy as np

# (n, H, W): the one-at-a-time path only (1 and 3 pixels), it behind whole groups of 4 (70 = 17 * 4 + 2), whole groups only (576), more than one block of 256 groups
# (3200 pixels = 800 groups) and an odd row length over more than one block per image (8547 = 2136 * 4 + 3): pixels % 4 takes 1, 3, 2, 0, 0, 3
CASES = [(1, 1, 1), (1, 1, 3), (2, 5, 7), (1, 9, 64), (2, 16, 100), (1, 33, 259)]
ALPHAS = [0.5, 0.3, 1.25]      # the reference's, another inside [0, 1], one outside it (PIL clips there)
OUTPUTS = ('color', 'compose', 'diff', 'ids')

# the 19 Cityscapes train classes, RGB; every other row of the 256 is zero (the reference pads its list the same way)
CITYSCAPES_COLOURS = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30), (220, 220, 0), (107, 142, 35),
                      (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32)]
PALETTE = np.zeros((256, 3), dtype=np.uint8)
PALETTE[:19] = CITYSCAPES_COLOURS

# label id -> train id in the order of the Cityscapes label list: 255 is shared by fifteen ids (the last of them, 30, wins), -1 names no byte, and two entries added
# here share train ids 13 and 0 with earlier ones (34 and 35 win over 26 and 7)
ID_TO_TRAINID = {-1: -1, 0: 255, 1: 255, 2: 255, 3: 255, 4: 255, 5: 255, 6: 255, 7: 0, 8: 1, 9: 255, 10: 255, 11: 2, 12: 3, 13: 4, 14: 255, 15: 255, 16: 255, 17: 5,
                 18: 255, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 29: 255, 30: 255, 31: 16, 32: 17, 33: 18, 34: 13, 35: 0}

_INPUTS = {}


def inputs(n, H, W):
    """-> dict(pred uint8 [n, H, W], image uint8 [n, H, W, 3], gt int64 [n, H, W]); computed once per case and never written.
    pred: classes 0 .. 18 with about 4 % bytes of 19 .. 255 (zero palette rows, the table's default and its 255 entry); gt: pred on about half of the pixels, another
    class elsewhere, then about 20 % 255 and about 2 % each of -1 and 40 (neither a class nor 255: a difference)."""
    key = (n, H, W)
    if key not in _INPUTS:
        r = np.random.RandomState(1000 * n + 10 * H + W)
        shape = (n, H, W)
        pred = r.randint(0, 19, shape)
        odd = r.rand(*shape) < 0.04
        pred[odd] = r.randint(19, 256, shape)[odd]
        if n * H * W >= 3:
            pred.reshape(-1)[-1] = 255      # the last pixel of the one-at-a-time path, with gt 255 and with gt 7 below
        gt = np.where(r.rand(*shape) < 0.5, pred, r.randint(0, 19, shape)).astype(np.int64)
        u = r.rand(*shape)
        gt[u < 0.2] = 255
        gt[(u >= 0.2) & (u < 0.22)] = -1
        gt[(u >= 0.22) & (u < 0.24)] = 40
        if n * H * W >= 3:
            gt.reshape(-1)[-1] = 255 if W % 2 else 7
        image = r.randint(0, 256, shape + (3,)).astype(np.uint8)
        d = dict(pred=pred.astype(np.uint8), image=image, gt=gt)
        for v in d.values():
            v.setflags(write=False)
        _INPUTS[key] = d
    return _INPUTS[key]


def id_table(id_to_trainid=ID_TO_TRAINID):
    """The reference's loop `for label_id, train_id in d.items(): label_out[pred == train_id] = label_id` over every possible byte of pred."""
    every = np.arange(256)
    out = np.zeros(256, dtype=np.int64)
    for label_id, train_id in id_to_trainid.items():
        out[every == train_id] = label_id
    return out.astype(np.uint8)


def blend(image, color, alpha):
    """PIL's Blend.c per channel in float32: (uint8)(i + alpha * (c - i)), truncated; clipped to 0 .. 255 first when alpha lies outside [0, 1]."""
    i, c = image.astype(np.float32), color.astype(np.float32)
    t = i + np.float32(alpha) * (c - i)
    if not 0.0 <= alpha <= 1.0:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def restate(pred, palette, image, gt, table, alpha):
    """The four images of the header's table. gt None: no diff."""
    color = palette[pred]
    compose = blend(image, color, alpha)
    out = dict(color=color, compose=compose, ids=table[pred])
    if gt is not None:
        differs = (gt != 255) & (gt != pred.astype(np.int64))
        out['diff'] = np.where(differs[..., None], compose, np.uint8(255))
    return out
