"""GPU: the ablation sweep (csrc/ablation.hip: pm_label_splat, pm_class_sums, pm_mem_actmap; harness.FeatureBasket / memory_activation / ablation_sweep) against
torch restatements of tsnelib.py:48-74 and ablation.py:309-315,375-399 in fp64 on the CPU (tests/ablation_cases.py). Every kernel input and output sits in a
poisoned slab of tools/view_slabs.py with guard checks; the feature map is a channel slice of a wider slab (pitch > c) and p_mem has pitch > m.

Class means (sums / counts of the classes with a pixel): the bound is twice the largest error the reference's OWN fp32 formulation (normalise -> up-sample -> matmul
in torch fp32 on the CPU) shows against fp64 on the same input, computed per case here and printed next to the kernel's figure. The kernel sums a few hundred to a few
thousand terms where the reference sums H * W of them.
Activation maps: the float map within 32 * 2^-23 / range_p of fp64 at every pixel; every byte within one of the fp64 byte and equal to it wherever the fp64 value x 255
is at least 255 * 32 * 2^-23 / range_p from an integer; exactly 0 / 255 at each pixel's fp64 arg-min / arg-max slot; the bytes inside the band are at most 1 % of all
(a condition on the inputs; tests/test_ablation_cpu.py holds the reference's own fp32 formulation to the same rule on the same inputs)."""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ablation_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('view_slabs', os.path.join(ROOT, 'tools', 'view_slabs.py'))
VS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VS)
DEV = 'cuda'
K1 = AC.CLASSES + 1
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)


@pytest.fixture(scope='module')
def env():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd import harness, synth
    from pinthememory_amd.hip import kernels, lib, ops
    from pinthememory_amd.network import deepv3plus
    return dict(K=kernels, L=lib, lib=lib.load(), ops=ops, harness=harness, synth=synth, deepv3plus=deepv3plus)


def guarded(bufs, call):
    before = VS.snapshot(bufs)
    code = call()
    torch.cuda.synchronize()
    assert code == 0, code
    VS.check(before, bufs)


# ---- raw calls through the ctypes table, every array inside a poisoned buffer ------------------------------------------------------------------------------------
def run_splat(env, lab, h, w):
    n, H, W = lab.shape
    bl, dl = VS.flat(lab.numel(), torch.int64, 'in', lab, DEV)
    bs, ds = VS.flat(n * h * w * K1, torch.float32, 'out', device=DEV)
    bc, dc = VS.flat(n * K1, torch.int64, 'out', device=DEV)
    guarded([bl, bs, bc], lambda: env['lib'].pm_label_splat(dl.data_ptr(), n, H, W, h, w, AC.CLASSES, ds.data_ptr(), dc.data_ptr(), env['L'].stream()))
    return ds.view(n, h, w, K1), dc.view(n, K1)


def run_sums(env, feat, dtype, splat):
    """feat: fp32 [n, C, h, w] values; laid out as a channel slice of a wider NHWC slab of `dtype`"""
    n, C, h, w = feat.shape
    L = env['L']
    bf, vf = VS.slab((n, h, w, C), dtype, 'slice', 'in', feat.permute(0, 2, 3, 1), DEV)
    bp, dp = VS.flat(splat.numel(), torch.float32, 'in', splat, DEV)
    bo, do = VS.flat(n * K1 * C, torch.float32, 'out', device=DEV)
    nb = env['lib'].pm_class_sums_workspace(n, h, w, C, AC.CLASSES)
    bw, dw = VS.flat(nb, torch.uint8, 'out', device=DEV)
    assert bf.pitch > C
    guarded([bf, bp, bo, bw], lambda: env['lib'].pm_class_sums(vf.data_ptr(), n, h, w, C, bf.pitch, L.PM_BF16 if dtype == torch.bfloat16 else L.PM_F32, dp.data_ptr(),
                                                               AC.CLASSES, do.data_ptr(), dw.data_ptr(), nb, L.stream()))
    return do.view(n, K1, C), vf


def run_actmap(env, sc, H, W, slots, want, palette=None, image=None, alpha=0.65):
    n, h, w, m = sc.shape
    S = len(slots)
    bp, vp = VS.slab((n, h, w, m), torch.float32, 'slice', 'in', sc, DEV)
    assert bp.pitch > m
    bufs, out = [bp], {}
    for k in want:
        numel = n * S * H * W * (3 if k in ('rgb', 'blend') else 1)
        b, d = VS.flat(numel, torch.float32 if k == 'act' else torch.uint8, 'out', device=DEV)
        bufs.append(b)
        out[k] = d.view((n, S, H, W, 3) if k in ('rgb', 'blend') else (n, S, H, W))
    ins = {}
    for k, t in (('palette', palette), ('image', image)):
        if t is not None:
            b, d = VS.flat(t.numel(), torch.uint8, 'in', t, DEV)
            bufs.append(b)
            ins[k] = d
    p = lambda t: None if t is None else t.data_ptr()
    arr = (ctypes.c_int32 * S)(*slots)
    guarded(bufs, lambda: env['lib'].pm_mem_actmap(vp.data_ptr(), n, h, w, m, bp.pitch, H, W, arr, S, p(out.get('act')), p(out.get('bytes')), p(ins.get('palette')),
                                                   p(ins.get('image')), alpha, p(out.get('rgb')), p(out.get('blend')), env['L'].stream()))
    return out


# ---- class sums ------------------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def sums_reference(shape, dtype, kind):
    """Computed once per case and shared: the inputs, the fp64 truth and the bound (twice the error of the reference's fp32 formulation against it)."""
    key = (shape, dtype, kind)
    if key not in _REF:
        n, C, h, w, H, W = shape
        feat = AC.features(n, C, h, w)
        if dtype == torch.bfloat16:
            feat = feat.bfloat16().float()      # the reference is computed on the widened tensor
        lab = AC.labels(n, H, W, kind)
        s64, c64 = AC.class_sums_ref(feat, lab, torch.float64)
        s32, c32 = AC.class_sums_ref(feat, lab, torch.float32)
        m64, present = AC.means(s64, c64)
        m32, _ = AC.means(s32, c32)
        assert torch.equal(c32, c64)
        _REF[key] = (feat, lab, c64, m64, present, 2 * float((m32 - m64).abs().max()))
    return _REF[key]


def hold_sums(env, shape, dtype, kind):
    n, C, h, w, H, W = shape
    K, ops = env['K'], env['ops']
    feat, lab, counts, m64, present, bound = sums_reference(shape, dtype, kind)
    splat, cnt = run_splat(env, lab, h, w)
    sums, view = run_sums(env, feat, dtype, splat)
    assert torch.equal(cnt.cpu(), counts)                                             # exact integer counts; values of 19 .. 254 are in no row
    assert int(counts.sum()) == int(((lab < AC.CLASSES) | (lab == 255)).sum())
    got, _ = AC.means(sums.cpu(), counts)
    err = float((got - m64).abs().max())
    print('class_sums %s %s %-7s err_hip %.3e bound %.3e (2 x the fp32 reference)' % (ids(shape), str(dtype).replace('torch.', ''), kind, err, bound))
    assert bool((sums.cpu()[~present] == 0).all())                                    # a class without a pixel has a zero row, not NaN
    # the Python surface on the same views: equal bits to the raw calls, and from run to run
    s2, c2 = K.label_splat(lab.to(DEV), (h, w))
    assert torch.equal(s2, splat) and torch.equal(c2, cnt) and torch.equal(K.label_splat(lab.to(DEV), (h, w))[0], s2)
    k1 = K.class_sums(view.permute(0, 3, 1, 2), s2)
    assert torch.equal(k1, sums) and torch.equal(K.class_sums(view.permute(0, 3, 1, 2), s2), k1)
    # the device composition: ops.resize of the normalised map to the full size, then the one-hot matmul in torch on the device. The map is normalised in fp64 and
    # rounded once: torch's fp32 normalize on the device is off by one ulp where the CPU's is not (6.2e-8 against fp64 at the one-pixel shape, more than the whole
    # bound there), and that rounding is neither the kernel's nor the composition's
    fd = F.normalize(view.permute(0, 3, 1, 2).double(), dim=1).float().contiguous(memory_format=torch.channels_last)
    up = ops.resize(fd, (H, W))
    comp = torch.matmul(up.reshape(n, C, -1), AC.one_hot(lab, torch.float32).to(DEV)).transpose(1, 2)
    cm, _ = AC.means(comp.cpu(), counts)
    # Both routes are held to fp64 with the one bound. Their difference is only printed: two results that each keep the bound may lie on opposite sides of the truth
    # (one-pixel shape on an MI355X: kernel 1.7e-8, composition 2.3e-8, apart by 4.0e-8 with a bound of 3.5e-8)
    cerr = float((cm - m64).abs().max())
    print('class_sums %s composition on the device: against fp64 %.3e, |kernel - composition| %.3e' % (ids(shape), cerr, float((got - cm).abs().max())))
    assert err <= bound, (err, bound)
    assert cerr <= bound, (cerr, bound)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', AC.SUM_SHAPES, ids=ids)
def test_class_means_against_fp64(env, shape, dtype):
    """Measured on an MI355X: see the figures each case prints (recorded in profiles/ablation_probe.txt)."""
    hold_sums(env, shape, dtype, 'mixed')


@pytest.mark.parametrize('kind', ['all255', 'single'])
def test_class_means_of_degenerate_label_images(env, kind):
    hold_sums(env, AC.SUM_SHAPES[0], torch.float32, kind)


# ---- activation maps -------------------------------------------------------------------------------------------------------------------------------------------------
def pil_blend(image, rgb, alpha):
    """Image.blend per (image, slot): image uint8 [n, H, W, 3], rgb uint8 [n, S, H, W, 3] (numpy)"""
    from PIL import Image
    out = np.empty_like(rgb)
    for i in range(rgb.shape[0]):
        for s in range(rgb.shape[1]):
            out[i, s] = np.asarray(Image.blend(Image.fromarray(image[i]), Image.fromarray(rgb[i, s]), alpha))
    return out


def act_inputs(shape, seed=5):
    n, m, h, w, H, W = shape
    g = AC.gen(seed)
    return torch.randint(0, 256, (256, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize('shape', AC.ACT_SHAPES, ids=ids)
def test_activation_maps_against_fp64(env, shape):
    n, m, h, w, H, W = shape
    sc = AC.scores(n, m, h, w)
    a64, r64 = AC.act_ref(sc, H, W, torch.float64)
    palette, image = act_inputs(shape)
    out = run_actmap(env, sc, H, W, list(range(m)), ('act', 'bytes', 'rgb', 'blend'), palette, image, 0.65)
    out = {k: v.cpu() for k, v in out.items()}
    fig = AC.check_act_rule(out['act'], out['bytes'], a64, r64)
    print('mem_actmap %s %s' % (ids(shape), fig))
    assert fig['band_share'] <= 0.01, fig
    assert torch.equal(out['rgb'], palette[out['bytes'].long()])
    assert np.array_equal(out['blend'].numpy(), pil_blend(image.numpy(), out['rgb'].numpy(), 0.65))


def test_constant_scores_give_byte_zero(env):
    n, m, h, w, H, W = AC.ACT_SHAPES[0]
    sc = AC.scores(n, m, h, w, constant_block=True)
    a64, r64 = AC.act_ref(sc, H, W, torch.float64)
    # the full-res pixels all of whose taps lie in the constant 2 x 2 block, from the geometry: source coordinate <= 1 on both axes. torch's own interpolation does
    # not give the slots of such a pixel equal values on every pixel (its vector and tail lanes round differently: ranges of 7e-18 in fp64, 4e-9 in fp32), so there
    # the truth is put in by hand: range 0, a = 0
    ys, xs = torch.arange(H, dtype=torch.float64) * (h - 1) / (H - 1) <= 1, torch.arange(W, dtype=torch.float64) * (w - 1) / (W - 1) <= 1
    flat2 = ys.unsqueeze(1) & xs.unsqueeze(0)
    assert int(flat2.sum()) == 81 and float(r64[:, flat2].max()) < 1e-15
    r64[:, flat2] = 0
    a64[:, :, flat2] = 0
    flat = flat2.expand_as(a64)
    out = {k: v.cpu() for k, v in run_actmap(env, sc, H, W, list(range(m)), ('act', 'bytes')).items()}
    assert bool((out['bytes'][flat] == 0).all()) and bool((out['act'][flat] == 0).all())
    AC.check_act_rule(out['act'], out['bytes'], a64, r64)


@pytest.mark.parametrize('alpha', [0.65, 0.0, 1.0])
def test_slot_subsets_output_subsets_and_blend(env, alpha):
    shape = AC.ACT_SHAPES[0]
    n, m, h, w, H, W = shape
    sc = AC.scores(n, m, h, w)
    palette, image = act_inputs(shape)
    names = ('act', 'bytes', 'rgb', 'blend')
    full = run_actmap(env, sc, H, W, list(range(m)), names, palette, image, alpha)
    assert np.array_equal(full['blend'].cpu().numpy(), pil_blend(image.numpy(), full['rgb'].cpu().numpy(), alpha))
    for slots in ([18, 0, 5], [3]):                                                   # the list's order is the output's
        sub = run_actmap(env, sc, H, W, slots, names, palette, image, alpha)
        for k in names:
            assert torch.equal(sub[k], full[k][:, slots]), (slots, k)
    if alpha != 0.65:
        return
    for r in range(1, 5):                                                             # every subset of the four outputs, with no more inputs than it needs
        for want in itertools.combinations(names, r):
            need_pal, need_img = 'rgb' in want or 'blend' in want, 'blend' in want
            sub = run_actmap(env, sc, H, W, [18, 0, 5], want, palette if need_pal else None, image if need_img else None, alpha)
            assert sorted(sub) == sorted(want)
            for k in want:
                assert torch.equal(sub[k], full[k][:, [18, 0, 5]]), (want, k)
    # the Python surface: the same bits
    got = env['K'].mem_actmap(sc.to(DEV), (n, h, w), (H, W), [18, 0, 5], palette=palette.to(DEV), image=image.to(DEV), alpha=alpha, want=names)
    for k in names:
        assert torch.equal(got[k], full[k][:, [18, 0, 5]]), k


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------------------------------------
SEL = [13, AC.ABSENT, 0, 5]
SIZE = (64, 96)
CRIT = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)


def expected_rows(K, feats, gts):
    """What the basket holds, composed with K.* directly: per image, per selected class with a pixel, sums / counts; normalised as one matrix."""
    rows, labels = [], []
    for f, gt in zip(feats, gts):
        splat, counts = K.label_splat(gt, tuple(f.shape[2:]))
        sums = K.class_sums(f, splat)
        for i in range(f.shape[0]):
            for k in SEL:
                if int(counts[i, k]) != 0:
                    rows.append(sums[i, k] / counts[i, k].float())
                    labels.append(k)
    return F.normalize(torch.stack(rows).float(), dim=1), labels


@pytest.mark.parametrize('memory,tier', [(True, 'f32'), (False, 'f32'), (True, 'bf16')], ids=['memory', 'plain', 'memory_bf16'])
def test_ablation_sweep_equals_its_composition(env, memory, tier):
    K, harness, synth = env['K'], env['harness'], env['synth']
    K.set_conv_precision(tier)
    try:
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(memory=memory, gumbel_off=True), 19, CRIT, CRIT)).cuda()
        lab = AC.labels(2, SIZE[0], SIZE[1], 'mixed', seed=77)
        if memory:      # uint8 images: normalised on the device, and the background of the blended maps
            imgs = torch.randint(0, 256, (2, SIZE[0], SIZE[1], 3), generator=AC.gen(78), dtype=torch.uint8)
            palette = act_inputs(AC.ACT_SHAPES[0])[0].to(DEV)
        else:
            imgs, palette = synth.make_batch(2, SIZE)[0], None
        loader = [(imgs[:1], lab[:1], 'a'), (imgs[1:], lab[1:], 'b')]
        maps = []
        basket, updated = harness.ablation_sweep(net, loader, SEL, domain_id=2, on_maps=lambda i, mp: maps.append((i, mp)), palette=palette)
        assert (updated is not None) == memory and net.eval_logits_lowres is False
        # the composition from the net's own eval outputs
        feats, refined, want_maps, gts = [], [], [], []
        with torch.no_grad():
            for im, gt, _ in loader:
                x = env['ops'].nchw(K.image_u8_to_nhwc4(im.to(DEV).contiguous())) if memory else im.to(DEV)
                out = net(x)
                feats.append(out[-1]), gts.append(gt.to(DEV).contiguous())
                assert out[-1].dtype == (torch.bfloat16 if tier == 'bf16' else torch.float32)
                if memory:
                    refined.append(out[-2][-1])
                    pm = out[-2][1]
                    want_maps.append(K.mem_actmap(pm, tuple(pm.shape[:3]), SIZE, SEL, palette=palette, image=im.to(DEV).contiguous(), want=('bytes', 'rgb', 'blend')))
        for b, fs in ((basket, feats), (updated, refined)):
            if b is None:
                continue
            vecs, labels, domains = b.vectors()
            want, want_labels = expected_rows(K, fs, gts)
            assert want_labels == [13, 0, 5, 13, 0, 5]                                 # image-major, the order of SEL, the absent class dropped
            nrow = len(want_labels)
            assert labels.tolist() == want_labels + (SEL if memory else []) and domains.tolist() == [2] * nrow + ([-1] * len(SEL) if memory else [])
            assert torch.equal(vecs[:nrow], want) and not bool(torch.isnan(vecs).any())
            if memory:
                assert torch.equal(vecs[nrow:], net.memory.m_items[SEL].float())
        assert len(maps) == (2 if memory else 0)
        for (i, got), want in zip(maps, want_maps):
            assert sorted(got) == ['blend', 'bytes', 'rgb'] and i == len([m for m in maps if m[0] < i])
            for k in got:
                assert torch.equal(got[k], want[k]), k
    finally:
        K.set_conv_precision('f32')
