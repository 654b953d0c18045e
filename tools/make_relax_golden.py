"""CPU oracle of relaxed-border training (csrc/loss.hip pm_relax_* / pm_upsample_relax_*, pinthememory_amd.loss.ImgWtLossSoftNLL): the reference's own classes,
imported where they lie (oracle.import_reference), run on small inputs; nothing of the reference is copied.

    python tools/make_relax_golden.py            # writes tests/golden/relax_cases.npz (needs the reference tree)
    python tools/make_relax_golden.py --check    # regenerates in memory and compares with the committed file

Targets: RelaxedBoundaryLossToTensor (transforms/transforms.py:99-148), loaded by file path with stubs for its absent imports; where that fails, its lines 132-137
with scipy.ndimage.shift. `target_source` says which one wrote the file. Losses: ImgWtLossSoftNLL (loss.py:193-263) in fp32 on F.interpolate(logits / temp), with
its own calculate_weights for the weight rows; and the closed form of the same loss in fp64 (closed_form below), whose autograd gradient is the gradient reference.

Loss cases L0 .. L7 (LOSS_SHAPES: the weighted-loss table, n = 3): L_labels u8 [3,H,W]; L_target u8 [3,C+1,H,ceil(W/8)], the reference's multi-hot target with np.packbits along W (load_target() undoes it, words() gives bit c = plane c);
per variant V of VARIANTS[L]: L_V_w f32 [3,C] weight rows, L_V_loss32 (reference, fp32), L_V_loss64, L_V_img64 [3] (per image) and L_V_gmax / L_V_gsum (largest
entry and sum of |entries| of the fp64 gradient w.r.t. the low-res logits, upstream scale 1.7). The logits are logits(L): torch's seeded CPU generator, held by
L_logit_sum; the two smallest cases also carry them (L_logits) and the whole fp64 gradient of the first variant (L_img_grad) -- all of them would make the file ten times
its size.
Border cases B*: B_labels i64, B_target (packed likewise) and the scalars B_classes, B_border, B_strict (bit mask) -- labels of 200 and -1 reach the reference as 255."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'relax_cases.npz')
N = 3
GSCALE = 1.7

# (h, w) -> (H, W), temperature, classes: tests/test_weighted_loss.py's table, each selects another kernel form
LOSS_SHAPES = [((5, 7), (33, 29), 2.0, 19), ((12, 12), (48, 48), 1.0, 19), ((6, 6), (96, 96), 0.5, 19), ((7, 5), (30, 41), 1.0, 8), ((3, 300), (7, 611), 1.0, 19),
               ((20, 256), (41, 520), 1.0, 19), ((16, 16), (16, 16), 1.0, 19), ((9, 9), (4, 6), 1.0, 19)]
# variant -> (upper_bound, norm, batch_weights)
ALL_VARIANTS = {'img': (1.0, False, False), 'batch': (1.0, False, True), 'ub037': (0.37, False, False), 'ub037batch': (0.37, False, True), 'norm': (1.0, True, False),
                'normbatch': (1.0, True, True)}
VARIANTS = {i: (list(ALL_VARIANTS) if i in (0, 1) else ['img', 'batch']) for i in range(len(LOSS_SHAPES))}
FULL = (0, 3)      # cases that carry their logits and the whole gradient
# name -> (shape [n,H,W], classes, border, strict list, odd labels)
BORDER_CASES = {'Bb2': ((2, 13, 17), 19, 2, [], False), 'Bstrict': ((2, 13, 17), 19, 1, [2, 5], False), 'Bb2strict': ((2, 13, 17), 19, 2, [0, 7, 18], False),
                'Bb3': ((1, 9, 11), 8, 3, [], False), 'B1x1': ((2, 1, 1), 19, 1, [], False), 'B1x1b2': ((1, 1, 1), 19, 2, [], False), 'B2x5': ((2, 2, 5), 19, 1, [], False),
                'B2x5b2': ((2, 2, 5), 19, 2, [3], False), 'B1x9': ((1, 1, 9), 19, 2, [], False), 'B7x1': ((1, 7, 1), 19, 1, [], False), 'B2x2b3': ((1, 2, 2), 5, 3, [], False),
                'Bodd': ((2, 11, 13), 19, 1, [], True), 'Bwide': ((1, 3, 1100), 19, 2, [4], False)}


def logits(case):
    """the low-res logits of loss case `case`: randn * 3 from torch's CPU generator"""
    import torch
    (h, w), _, _, C = LOSS_SHAPES[case]
    return torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(100 + case)) * 3


def labels(case):
    """4 x 4 blocks of random classes, 10 % of the pixels and the first two rows ignored"""
    _, (H, W), _, C = LOSS_SHAPES[case]
    rng = np.random.default_rng(700 + case)
    blocks = rng.integers(0, C, size=(N, (H + 3) // 4, (W + 3) // 4))
    lab = np.repeat(np.repeat(blocks, 4, axis=1), 4, axis=2)[:, :H, :W].astype(np.uint8)
    lab[rng.random((N, H, W)) < 0.1] = 255
    lab[:, :2] = 255
    return lab


def border_labels(name):
    shape, classes, _, _, odd = BORDER_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    n, H, W = shape
    blocks = rng.integers(0, classes, size=(n, (H + 2) // 3, (W + 2) // 3))
    lab = np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)[:, :H, :W].astype(np.int64)
    lab[rng.random(shape) < 0.15] = 255
    if odd:
        lab[rng.random(shape) < 0.1] = 200
        lab[rng.random(shape) < 0.1] = -1
    return lab


def load_target(fixture, key):
    """the uint8 multi-hot target [n, planes, H, W] of case `key` of the loaded fixture"""
    return np.unpackbits(fixture[key + '_target'], axis=-1, count=fixture[key + '_labels'].shape[-1])


def words(multihot):
    """uint8 [n, planes, H, W] (non-zero = set) -> uint32 [n, H, W], bit c = plane c"""
    planes = multihot.shape[1]
    return ((multihot != 0).astype(np.uint32) << np.arange(planes, dtype=np.uint32).reshape(1, -1, 1, 1)).sum(1, dtype=np.uint32)


def closed_form(up, bits, rows):
    """The loss in the dtype of `up` [n,C,H,W] (fp64 for the reference values): per pixel - mean(w over S) log(sum of softmax over S), S the real classes of the set
    in `bits` (int64 [n,H,W]); image: sum / (pixels with a set + 1). -> (batch loss, per-image losses). Pure torch, differentiable."""
    import torch
    n, C = up.shape[:2]
    inset = ((bits.unsqueeze(1) >> torch.arange(C).view(1, -1, 1, 1)) & 1).bool()
    k = inset.sum(1)
    valid = k > 0
    p = torch.softmax(up, dim=1)
    ps = (p * inset).sum(1)
    wbar = (rows.to(up.dtype).view(n, C, 1, 1) * inset).sum(1) / k.clamp(min=1)
    terms = torch.where(valid, -wbar * torch.log(torch.where(valid, ps, torch.ones_like(ps))), torch.zeros_like(ps))
    per_image = terms.flatten(1).sum(1) / (valid.flatten(1).sum(1) + 1)
    return per_image.sum() / n, per_image


def reference_modules():
    """-> (the reference's loss module, its cfg, RelaxedBoundaryLossToTensor or None, how the targets are made)"""
    sys.path.insert(0, ROOT)
    from oracle import import_reference
    import_reference.load()
    import loss as ref_loss
    from config import cfg
    cfg.immutable(False)
    source, cls = 'scipy.ndimage.shift, transforms.py:132-137', None
    try:
        def stub(name, **kw):
            if name not in sys.modules:
                m = types.ModuleType(name)
                m.__dict__.update(kw)
                sys.modules[name] = m
        nothing = lambda *a, **k: None
        stub('skimage'), stub('skimage.filters', gaussian=nothing), stub('skimage.restoration', denoise_bilateral=nothing)
        stub('skimage.segmentation', find_boundaries=nothing), stub('skimage.util', random_noise=nothing), stub('torchvision.transforms')
        spec = importlib.util.spec_from_file_location('_ref_transforms', os.path.join(import_reference.REF, 'transforms', 'transforms.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cls, source = mod.RelaxedBoundaryLossToTensor, 'RelaxedBoundaryLossToTensor'
    except Exception as e:      # noqa: BLE001 -- any import failure of the reference's module sends us to the restated lines
        print('RelaxedBoundaryLossToTensor did not load (%s: %s)' % (type(e).__name__, e), file=sys.stderr)
    return ref_loss, cfg, cls, source


def make_target(ref, lab, classes, border, strict):
    """uint8 [n, classes + 1, H, W] of uint8-representable labels [n,H,W]"""
    _, cfg, cls, _ = ref
    cfg.BORDER_WINDOW, cfg.STRICTBORDERCLASS, cfg.REDUCE_BORDER_ITER = border, (list(strict) if strict else None), -1
    out = []
    for img in lab.astype(np.uint8):
        if cls is not None:
            out.append(cls(255, classes)(img.copy()).numpy())
            continue
        from scipy.ndimage import shift
        arr = img.copy()
        arr[arr == 255] = classes
        eye = np.eye(classes + 1, dtype=np.uint8)
        one_hot = 0
        for i in range(-border, border + 1):
            for j in range(-border, border + 1):
                one_hot = one_hot + eye[shift(arr, (i, j), cval=classes)]
        one_hot[one_hot > 1] = 1
        if strict:
            one_hot = np.where(np.isin(arr, strict)[..., None], eye[arr], one_hot)
        out.append(np.moveaxis(one_hot, -1, 0).astype(np.uint8))
    return np.stack(out)


def generate():
    import torch
    import torch.nn.functional as F
    ref = reference_modules()
    ref_loss = ref[0]
    arrays = {'target_source': np.array(ref[3])}
    for case, (hw, HW, temp, C) in enumerate(LOSS_SHAPES):
        key = 'L%d' % case
        lab, lg = labels(case), logits(case)
        target = make_target(ref, lab, C, 1, None)
        bits = words(target)
        k = target[:, :C].sum(1)
        shares = [(k == 0).mean(), (k == 1).mean(), (k > 1).mean()]
        assert shares[0] >= 0.01 and shares[1] >= 0.10 and shares[2] >= 0.10, (key, shares)
        arrays[key + '_labels'], arrays[key + '_target'], arrays[key + '_logit_sum'] = lab, np.packbits(target, axis=-1), np.float64(lg.double().sum().item())
        if case in FULL:
            arrays[key + '_logits'] = lg.numpy()
        tt = torch.from_numpy(target)
        bt = torch.from_numpy(bits.astype(np.int64))
        up32 = F.interpolate(lg / temp, size=HW, mode='bilinear', align_corners=True)
        for v in VARIANTS[case]:
            ub, norm, batch = ALL_VARIANTS[v]
            crit = ref_loss.ImgWtLossSoftNLL(classes=C, ignore_index=255, upper_bound=ub, norm=norm)
            crit.batch_weights = batch
            with np.errstate(all='ignore'):
                rows = np.stack([crit.calculate_weights(target) if batch else crit.calculate_weights(target[i]) for i in range(N)]).astype(np.float32)
                loss32 = crit(up32, tt).item()
            if not np.isfinite(rows).all():      # norm with a class no set holds: the reference's weights (and loss) are NaN; only the rows are recorded
                arrays['%s_%s_w' % (key, v)] = rows
                continue
            lr = lg.double().requires_grad_(True)
            loss64, img64 = closed_form(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), bt, torch.from_numpy(rows).double())
            (loss64 * GSCALE).backward()
            assert abs(loss32 - loss64.item()) < 2e-6 * max(1.0, abs(loss64.item())), (key, v, loss32, loss64.item())
            pre = '%s_%s_' % (key, v)
            arrays[pre + 'w'], arrays[pre + 'loss32'], arrays[pre + 'loss64'] = rows, np.float32(loss32), np.float64(loss64.item())
            arrays[pre + 'img64'] = img64.detach().numpy()
            arrays[pre + 'gmax'], arrays[pre + 'gsum'] = np.float64(lr.grad.abs().max().item()), np.float64(lr.grad.abs().sum().item())
            if case in FULL and v == 'img':
                arrays[pre + 'grad'] = lr.grad.numpy()
    for name, (shape, classes, border, strict, odd) in BORDER_CASES.items():
        lab = border_labels(name)
        seen = np.where((lab < 0) | (lab >= classes), 255, lab)      # what the reference can take: every label that is no class as the ignore label
        arrays[name + '_labels'], arrays[name + '_target'] = lab, np.packbits(make_target(ref, seen, classes, border, strict), axis=-1)
        arrays[name + '_classes'], arrays[name + '_border'] = np.int32(classes), np.int32(border)
        arrays[name + '_strict'] = np.uint32(sum(1 << c for c in strict))
    return arrays


def main():
    arrays = generate()
    if '--check' in sys.argv:
        with np.load(FIXTURE) as f:
            assert sorted(f.files) == sorted(arrays), 'key sets differ'
            bad = [k for k in arrays if not (f[k].dtype == arrays[k].dtype and np.array_equal(f[k], arrays[k], equal_nan=f[k].dtype.kind == 'f'))]
        print('differs: %s' % bad if bad else 'identical: %d arrays' % len(arrays))
        sys.exit(1 if bad else 0)
    np.savez_compressed(FIXTURE, **arrays)
    print('wrote %s: %d bytes (%s)' % (FIXTURE, os.path.getsize(FIXTURE), arrays['target_source']))


if __name__ == '__main__':
    main()
