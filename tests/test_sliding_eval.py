"""GPU: sliding-window evaluation -- pm_sliding_eval / pm_sliding_eval_finish (up-sample the tiles' low-res logits, stitch, un-flip, mean over flips and scales,
argmax, confusion matrix, without the up-sampled tiles or a stitched map in memory) against what eval.py runs, restated on the CPU: F.interpolate(align_corners=True)
in fp32 per tile, the float64 host stitch of tests/test_hip_kernels.py::test_sliding_stitch, the mean over the flips and, for more scales, cv2.resize(INTER_LINEAR)
as tests/test_sliding_eval_cpu.py::cv2_linear restates it. cv2 is not a dependency of this repository, so bit-equality with cv2 itself is unverified: the
formula stated in include/pinmem_hip.h is the contract. And harness.evaluate_sliding / harness.evaluate against harness.sliding_logits on the same net.

The rule and the constants are those of tests/test_validate.py: the class map equals the reference's argmax wherever the reference's own top-2 margin is at least
MARGIN = 1e-4 and names one of its top two below it; the below-margin share of the reference alone is capped by SHARE_CAP. The rule presupposes that the kernel's
float64 logits stay within MARGIN / 2 of the reference's, which is asserted on the logits output (and against the device composition ops.resize + K.sliding_stitch).
Measured on an MI355X (printed by every case, recorded in profiles/sliding_eval_probe.txt): the largest logit delta against the CPU reference is 1.3e-6, against
the device composition 9.5e-7; the below-margin share is 0 in every case but the 72-tile one (2.4e-4, two pixels); no class map differs from the reference's argmax."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_sliding_eval_cpu import GEOMETRIES, MULTI, cv2_linear, rejections
from test_validate import CRIT, GUARD, MARGIN, PRED_SENTINEL, SENTINEL, SHARE_CAP, K, guarded, harness, labels_for, margins_untouched, ref_hist, rnd, v3net  # noqa: F401

pytestmark = pytest.mark.gpu

# (H, W, crop, overlap, low-res ratio, C, flips, seed)
SINGLE = [g + (19, 2, i) for i, g in enumerate(GEOMETRIES)] + [(20, 37, 12, 1.0 / 3, 4, 7, 2, 5),       # another class count
                                                               (20, 37, 12, 1.0 / 3, 4, 19, 1, 6)]      # no flip
_CASES = {}


def low_shape(th, tw, ratio):
    return -(-th // ratio), -(-tw // ratio)


def stitched(lg, tiles, Hs, Ws, th, tw):
    """eval.py:210-228 for every flip of one scale: [F][T, C, hl, wl] fp32 -> the un-flipped float64 [F, C, Hs, Ws] maps."""
    maps = []
    for f, l in enumerate(lg):
        up = F.interpolate(l, size=(th, tw), mode='bilinear', align_corners=True)
        full = torch.zeros(l.shape[1], Hs, Ws, dtype=torch.float64)
        cnt = torch.zeros(1, Hs, Ws, dtype=torch.float64)
        for i, (x1, y1, x2, y2) in enumerate(tiles):
            full[:, y1:y2, x1:x2] += up[i].double()
            cnt[:, y1:y2, x1:x2] += 1
        full = full / cnt
        maps.append(torch.flip(full, dims=[2]) if f else full)
    return torch.stack(maps)


def summarise(mean, lab, C):
    top = mean.topk(2, dim=0)
    return dict(mean=mean, arg=mean.argmax(0), top2=top.indices, safe=(top.values[0] - top.values[1]) >= MARGIN, hist=ref_hist(mean.argmax(0), lab, C), lab=lab)


def single_case(H, W, crop, overlap, ratio, C, flips, seed):
    """Inputs and the CPU reference of one single-scale case, computed once and never written."""
    key = (H, W, crop, overlap, ratio, C, flips, seed)
    if key not in _CASES:
        from pinthememory_amd import harness as hs
        tiles = hs.sliding_tiles(H, W, crop, overlap)
        th, tw = tiles[0][3] - tiles[0][1], tiles[0][2] - tiles[0][0]
        hl, wl = low_shape(th, tw, ratio)
        lg = [rnd(len(tiles), C, hl, wl, seed=100 * seed + f) * 3 for f in range(flips)]
        ref = summarise(stitched(lg, tiles, H, W, th, tw).sum(0) / flips, labels_for(1, C, (H, W), seed)[0], C)
        ref.update(lg=lg, tiles=tiles, th=th, tw=tw)
        _CASES[key] = ref
    return _CASES[key]


def multi_case(H, W, crop, scales, C=19, flips=2, seed=0):
    key = ('multi', H, W, crop, scales, C, flips, seed)
    if key not in _CASES:
        from pinthememory_amd import harness as hs
        per_scale, total = [], None
        for k, s in enumerate(scales):
            Hs, Ws = int(H * s), int(W * s)
            tiles = hs.sliding_tiles(Hs, Ws, crop, 1.0 / 3, s)
            th, tw = tiles[0][3] - tiles[0][1], tiles[0][2] - tiles[0][0]
            hl, wl = low_shape(th, tw, 4)
            lg = [rnd(len(tiles), C, hl, wl, seed=1000 * seed + 10 * k + f) * 3 for f in range(flips)]
            maps = stitched(lg, tiles, Hs, Ws, th, tw).numpy()
            one = torch.from_numpy(np.stack([cv2_linear(m, H, W) for m in maps]).sum(0) / flips)      # np.mean(batch_return, axis=0) of the resized maps
            total = one if total is None else total + one
            per_scale.append(dict(lg=lg, tiles=tiles, hw=(Hs, Ws)))
        ref = summarise(total / len(scales), labels_for(1, C, (H, W), seed)[0], C)                  # np.mean over the scales (eval.py:647)
        ref.update(scales=per_scale)
        _CASES[key] = ref
    return _CASES[key]


def guarded_logits(K, lg):
    """[F][T, C, hl, wl] -> the NHWC stack [F * T, hl, wl, C] (pitch-padded) inside a larger buffer whose margins are NaN: a read outside shows in the result."""
    x = torch.cat(lg).permute(0, 2, 3, 1).contiguous()
    n, h, w, C = x.shape
    pitch = (C + 3) // 4 * 4
    buf = torch.full((n * h * w * pitch + 2 * GUARD * pitch,), float('nan'), device='cuda')
    view = buf[GUARD * pitch:GUARD * pitch + n * h * w * pitch].view(n, h, w, pitch)
    view.zero_()
    view = view[..., :C]
    view.copy_(x.cuda())
    return buf, view, pitch


def guarded_f64(C, H, W):
    buf = torch.full((C * H * W + 2 * GUARD,), float(SENTINEL), dtype=torch.float64, device='cuda')
    return buf, buf[GUARD:GUARD + C * H * W].view(C, H, W)


def f64_margins_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def logit_margins_untouched(buf, pitch):
    return bool(torch.isnan(buf[:GUARD * pitch]).all()) and bool(torch.isnan(buf[-GUARD * pitch:]).all())


def check_against(ref, pred, hist, logits, harness, C):
    """the rule of tests/test_validate.py on one image"""
    lab = ref['lab']
    p, safe = pred.cpu().long(), ref['safe']
    share = 1.0 - safe.float().mean().item()
    delta = (logits.cpu() - ref['mean']).abs().max().item()
    print('below-margin share', share, 'pixels', int((~safe).sum()), 'disagreeing with the reference argmax', int((p != ref['arg']).sum()), 'max |logit delta|', delta)
    assert share <= SHARE_CAP
    assert delta <= MARGIN / 2
    assert torch.equal(p[safe], ref['arg'][safe])
    assert bool(((p == ref['top2'][0]) | (p == ref['top2'][1]))[~safe].all())
    assert torch.equal(hist, harness.fast_hist(pred.long(), lab.cuda(), C))
    countable = (lab >= 0) & (lab < C)
    assert hist.sum().item() == countable.sum().item()
    diff = (hist.cpu() - ref['hist']).abs().sum().item()
    print('hist |delta|', diff, 'allowed', 2 * int((~safe & countable).sum()))
    assert diff <= 2 * int((~safe & countable).sum())


@pytest.mark.parametrize('H,W,crop,overlap,ratio,C,flips,seed', SINGLE)
def test_single_scale_against_the_host_formulation(K, harness, H, W, crop, overlap, ratio, C, flips, seed):
    from pinthememory_amd.hip import ops
    ref = single_case(H, W, crop, overlap, ratio, C, flips, seed)
    tiles, lab = ref['tiles'], ref['lab'].cuda()
    lbuf, lgg, pitch = guarded_logits(K, ref['lg'])
    assert lgg.stride(2) == pitch
    hb, hist, pb, pred = guarded(1, (H, W), C)
    pred = pred[0]
    ob, out = guarded_f64(C, H, W)

    def untouched():
        return margins_untouched(hb, pb) and f64_margins_untouched(ob) and logit_margins_untouched(lbuf, pitch)

    p_ret, h_ret, o_ret = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, labels=lab, hist=hist, accumulate=False, pred=pred, logits_out=out)
    assert p_ret is pred and h_ret is hist and o_ret is out
    check_against(ref, pred, hist, out, harness, C)
    assert untouched()
    # unpadded logits (pitch C): the scalar loads give the same bits as the 16-byte ones
    dense = lgg.contiguous()
    assert dense.stride(2) == C and C % 4 != 0
    p_d, h_d, o_d = K.sliding_eval(dense, tiles, (H, W), (H, W), flips, labels=lab, want_pred=True, want_logits=True)
    assert torch.equal(p_d, pred) and torch.equal(h_d, hist) and torch.equal(o_d, out)
    # the device composition it replaces: ops.resize of every tile, one stitch per flip (stock float64 torch ops past 64 tiles, as harness.sliding_logits), / flips
    comp = None
    for f in range(flips):
        up = ops.resize(ops.nchw(lgg[f * len(tiles):(f + 1) * len(tiles)]), (ref['th'], ref['tw']))
        if len(tiles) <= harness.STITCH_MAX_TILES:
            comp = K.sliding_stitch(ops.nhwc(up), tiles, H, W, bool(f), comp)
        else:
            comp = harness._stitch_torch(up, tiles, H, W, bool(f), comp)
    delta = (out - comp / flips).abs().max().item()
    print('max |logit delta| against ops.resize + sliding_stitch', delta)
    assert delta <= MARGIN / 2
    # accumulation: a second call adds, a call with accumulate = 0 overwrites whatever was there
    single = hist.clone()
    K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, labels=lab, hist=hist, accumulate=True)
    assert torch.equal(hist, 2 * single)
    hist.fill_(SENTINEL)
    K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, labels=lab, hist=hist, accumulate=False)
    assert torch.equal(hist, single)
    # labels=None leaves the histogram alone
    hist.fill_(SENTINEL)
    p2, h2, o2 = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, hist=hist, want_pred=True)
    assert h2 is hist and bool((hist == SENTINEL).all()) and o2 is None and torch.equal(p2, pred)
    assert untouched()
    # determinism; the same bits whatever else is asked for
    p3, h3, o3 = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, labels=lab, want_pred=True, want_logits=True)
    assert torch.equal(p3, pred) and torch.equal(h3, single) and torch.equal(o3, out)
    p4, h4, o4 = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, labels=lab)
    assert p4 is None and o4 is None and torch.equal(h4, single)
    p5, h5, o5 = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, want_logits=True)
    assert p5 is None and h5 is None and torch.equal(o5, out)
    # through the accumulator (one scale of ratio 1, resampled by the identity) and the finish call: the same map
    acc = K.sliding_eval(lgg, tiles, (H, W), (H, W), flips, acc=torch.empty((C, H, W), dtype=torch.float64, device='cuda'))
    assert torch.equal(acc, out)
    p6, h6, o6 = K.sliding_eval_finish(acc, 1, labels=lab, want_pred=True)
    assert torch.equal(p6, pred) and torch.equal(h6, single) and o6 is None


@pytest.mark.parametrize('H,W,crop,scales', MULTI)
def test_scales_against_the_host_formulation(K, harness, H, W, crop, scales):
    C, flips = 19, 2
    ref = multi_case(H, W, crop, scales)
    lab = ref['lab'].cuda()
    hb, hist, pb, pred = guarded(1, (H, W), C)
    pred = pred[0]
    ab, acc = guarded_f64(C, H, W)
    ob, out = guarded_f64(C, H, W)
    inputs = [guarded_logits(K, sc['lg']) for sc in ref['scales']]

    def run(acc):
        for k, (sc, (lbuf, lgg, pitch)) in enumerate(zip(ref['scales'], inputs)):
            assert K.sliding_eval(lgg, sc['tiles'], sc['hw'], (H, W), flips, acc=acc, acc_add=k > 0) is acc
        return acc

    run(acc)
    p_ret, h_ret, o_ret = K.sliding_eval_finish(acc, len(scales), labels=lab, hist=hist, accumulate=False, pred=pred, logits_out=out)
    assert p_ret is pred and h_ret is hist and o_ret is out
    check_against(ref, pred, hist, out, harness, C)
    assert margins_untouched(hb, pb) and f64_margins_untouched(ab) and f64_margins_untouched(ob)
    assert all(logit_margins_untouched(lbuf, pitch) for lbuf, _, pitch in inputs)
    # repeat: the same bits; the first scale overwrites whatever the accumulator held; the mean may be written over the accumulator itself
    acc2 = run(torch.full((C, H, W), float('nan'), dtype=torch.float64, device='cuda'))
    assert torch.equal(acc2, acc)
    dense = torch.empty_like(acc)                                               # unpadded logits (pitch C): the scalar loads, the same bits
    for k, (sc, (_, lgg, _)) in enumerate(zip(ref['scales'], inputs)):
        K.sliding_eval(lgg.contiguous(), sc['tiles'], sc['hw'], (H, W), flips, acc=dense, acc_add=k > 0)
    assert torch.equal(dense, acc)
    single = hist.clone()
    p2, h2, o2 = K.sliding_eval_finish(acc2, len(scales), labels=lab, hist=hist, accumulate=True, want_pred=True, logits_out=acc2)
    assert o2 is acc2 and torch.equal(acc2, out) and torch.equal(p2, pred) and torch.equal(hist, 2 * single)
    hist.fill_(SENTINEL)
    p3, h3, o3 = K.sliding_eval_finish(acc, len(scales), hist=hist, want_pred=True)
    assert bool((hist == SENTINEL).all()) and torch.equal(p3, pred) and o3 is None
    assert margins_untouched(hb, pb) and f64_margins_untouched(ab)


def test_ties_go_to_the_lowest_class(K):
    """Classes 5 and 11 are 2.0 in every tile of both flips, every other logit 0: their stitched means are bit-equal and the lower class is named. All-zero
    logits: class 0. Both through the single launch and through accumulator + finish."""
    H, W, crop, overlap, ratio, C, flips, seed = SINGLE[1]
    ref = single_case(*SINGLE[1])
    tiles, lab = ref['tiles'], ref['lab']
    shape = ref['lg'][0].shape
    tied = torch.zeros(shape)
    tied[:, 5] = 2.0
    tied[:, 11] = 2.0
    for lg, want in ((tied, 5), (torch.zeros(shape), 0)):
        _, lgg, _ = guarded_logits(K, [lg, lg])
        pred, hist, out = K.sliding_eval(lgg, tiles, (H, W), (H, W), 2, labels=lab.cuda(), want_pred=True, want_logits=True)
        assert torch.equal(out[5], out[11]) and bool((pred == want).all())
        assert hist[:, want].sum().item() == hist.sum().item() == (lab != 255).sum().item()
        assert torch.equal(hist[:, want].cpu(), torch.bincount(lab[lab != 255], minlength=C))
        acc = K.sliding_eval(lgg, tiles, (H, W), (H, W), 2, acc=torch.empty_like(out))
        p2, h2, _ = K.sliding_eval_finish(acc, 1, labels=lab.cuda(), want_pred=True)
        assert torch.equal(p2, pred) and torch.equal(h2, hist)


def test_all_pixels_ignored_and_labels_outside_the_classes(K):
    H, W, crop, overlap, ratio, C, flips, seed = SINGLE[1]
    ref = single_case(*SINGLE[1])
    _, lgg, _ = guarded_logits(K, ref['lg'])
    hb, hist, pb, pred = guarded(1, (H, W), C)
    K.sliding_eval(lgg, ref['tiles'], (H, W), (H, W), flips, labels=torch.full((H, W), 255, dtype=torch.int64, device='cuda'), hist=hist, accumulate=False, pred=pred[0])
    assert not hist.any().item() and margins_untouched(hb, pb)
    p = pred[0].cpu().long()                                                     # still written, for every pixel
    assert torch.equal(p[ref['safe']], ref['arg'][ref['safe']])
    lab = ref['lab'].clone()                                                     # fast_hist's mask: only 0 <= label < C is counted
    lab[5, ::3] = C + 2
    lab[6, ::4] = -1
    p2, h2, _ = K.sliding_eval(lgg, ref['tiles'], (H, W), (H, W), flips, labels=lab.cuda(), want_pred=True)
    assert h2.sum().item() == ((lab >= 0) & (lab < C)).sum().item()
    assert torch.equal(h2.cpu(), ref_hist(p2.cpu().long(), lab, C))


def test_every_rejection_comes_before_any_launch(K):
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    logits = torch.zeros(8 * 2 * 2 * 20, device='cuda')
    labels = torch.zeros(144, dtype=torch.int64, device='cuda')
    hb, hist, pb, pred = guarded(1, (12, 12), 19)
    ob, out = guarded_f64(19, 12, 12)
    hist.fill_(SENTINEL), pred.fill_(PRED_SENTINEL), out.fill_(SENTINEL)
    ws = torch.full((1 << 16,), PRED_SENTINEL, dtype=torch.uint8, device='cuda')
    rejections(lib, logits.data_ptr(), labels.data_ptr(), hist.data_ptr(), pred.data_ptr(), out.data_ptr(), out.data_ptr(), ws.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert bool((hb == SENTINEL).all()) and bool((pb == PRED_SENTINEL).all()) and bool((ob == SENTINEL).all()) and bool((ws == PRED_SENTINEL).all())
    with pytest.raises(L.PinmemError):                                          # the Python wrapper raises on the same statuses
        K.sliding_eval(logits.view(8, 2, 2, 20)[..., :19], [(0, 0, 8, 8), (0, 4, 8, 12), (4, 0, 12, 8)] * 2, (12, 12), (12, 12), 2, want_pred=True)


# ---- the callers ------------------------------------------------------------------------------------------------------------------------------------------
HW_IMG, CROP = (96, 160), 64


def image_u8(seed=31, hw=HW_IMG):
    return torch.randint(0, 256, (*hw, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def normalised(K, img_u8):
    """the float [3, H, W] image evaluate_sliding makes of a uint8 one"""
    return K.image_u8_to_nhwc4(img_u8.cuda()[None].contiguous())[0, :, :, :3].permute(2, 0, 1).contiguous()


def image_labels(seed, hw=HW_IMG):
    from pinthememory_amd import synth
    return synth.make_batch(1, hw, seed=seed)[1][0]


def agrees_with_sliding_logits(harness, net, img_f, res, gt, flips=(False, True)):
    full = harness.sliding_logits(net, img_f, CROP, flips=flips)
    top = full.topk(2, dim=0)
    safe = (top.values[0] - top.values[1]) >= MARGIN
    share = 1.0 - safe.float().mean().item()
    print('below-margin share', share, 'disagreeing', int((res['pred'].long() != top.indices[0]).sum()))
    assert share <= SHARE_CAP
    assert torch.equal(res['pred'].long()[safe], top.indices[0][safe])
    assert bool(((res['pred'].long() == top.indices[0]) | (res['pred'].long() == top.indices[1]))[~safe].all())
    assert torch.equal(res['hist'], harness.fast_hist(res['pred'].long(), gt.cuda(), 19))
    return full


def test_evaluate_sliding_against_sliding_logits(K, harness, v3net):
    net = v3net
    img, gt = image_u8(), image_labels(41)
    res = harness.evaluate_sliding(net, img, gt, crop=CROP, want_logits=True)
    assert res['pred'].dtype == torch.uint8 and tuple(res['pred'].shape) == HW_IMG and res['hist'].dtype == torch.int64 and res['hist'].is_cuda
    full = agrees_with_sliding_logits(harness, net, normalised(K, img), res, gt)
    delta = (res['logits'] - full).abs().max().item()
    print('max |logit delta| against sliding_logits', delta)
    assert delta <= MARGIN / 2
    assert net.eval_logits_lowres is False and not net.training
    # the same image as a normalised float tensor, on the device; tile by tile; without the mirror image; into a running histogram
    again = harness.evaluate_sliding(net, normalised(K, img), gt.cuda(), crop=CROP)
    assert torch.equal(again['pred'], res['pred']) and torch.equal(again['hist'], res['hist']) and again['logits'] is None
    running = harness.evaluate_sliding(net, img.cuda(), gt, crop=CROP, hist=res['hist'].clone())
    assert torch.equal(running['pred'], res['pred']) and torch.equal(running['hist'], 2 * res['hist'])
    slow = harness.evaluate_sliding(net, img, gt, crop=CROP, batch_tiles=False)      # one tile per forward: other convolution plans, so the margin rule again
    agrees_with_sliding_logits(harness, net, normalised(K, img), slow, gt)
    one = harness.evaluate_sliding(net, img, gt, crop=CROP, flips=(False,))
    agrees_with_sliding_logits(harness, net, normalised(K, img), one, gt, flips=(False,))
    none = harness.evaluate_sliding(net, img, crop=CROP)
    assert none['hist'] is None and torch.equal(none['pred'], res['pred'])


def test_evaluate_sliding_scales(K, harness, v3net):
    """Two scales through the accumulator: the class map is the argmax of the returned mean logits, the histogram fast_hist of it; a scale of 1 alone through the
    accumulator route (scales=(1.0, 1.0): the mean of two equal maps) names the single-scale map."""
    net = v3net
    img, gt = image_u8(), image_labels(41)
    res = harness.evaluate_sliding(net, img, gt, crop=CROP, scales=(0.75, 1.0), want_logits=True)
    assert tuple(res['logits'].shape) == (19, *HW_IMG) and bool(torch.isfinite(res['logits']).all())
    assert torch.equal(res['pred'].long(), res['logits'].argmax(0))
    assert torch.equal(res['hist'], harness.fast_hist(res['pred'].long(), gt.cuda(), 19))
    twice = harness.evaluate_sliding(net, img, gt, crop=CROP, scales=(1.0, 1.0), want_logits=True)
    once = harness.evaluate_sliding(net, img, gt, crop=CROP, want_logits=True)
    assert torch.equal(twice['logits'], once['logits']) and torch.equal(twice['pred'], once['pred']) and torch.equal(twice['hist'], once['hist'])
    with pytest.raises(ValueError):
        harness.evaluate_sliding(net, normalised(K, img), gt, crop=CROP, scales=(0.75, 1.0))      # a float image cannot be re-scaled as the reference does
    with pytest.raises(ValueError):
        harness.evaluate_sliding(net, img.cuda(), gt, crop=CROP, scales=(0.75,))                  # PIL scales on the host
    assert net.eval_logits_lowres is False


def test_evaluate_sliding_hands_the_kernel_pitch_padded_logits(harness, v3net, monkeypatch):
    """Whatever the flips and the batching, K.sliding_eval gets ONE [F * T, h, w, 19] view with the heads' 16-byte pixel pitch (20 floats) at a 16-byte aligned
    address -- what its 16-byte loads ask for; a torch.cat of the forwards' outputs would pack the pixels to 19 floats and quietly take the 4-byte loads."""
    net, img = v3net, image_u8()
    T = len(harness.sliding_tiles(*HW_IMG, CROP, 1.0 / 3))
    seen, real = [], harness.K.sliding_eval

    def spy(logits, *a, **k):
        seen.append((logits.shape[0], logits.shape[3], logits.stride(), logits.data_ptr() % 16))
        return real(logits, *a, **k)
    monkeypatch.setattr(harness.K, 'sliding_eval', spy)
    for kw, n in (({}, 2 * T), ({'batch_tiles': False}, 2 * T), ({'flips': (False,)}, T), ({'flips': (False,), 'batch_tiles': False}, T)):
        harness.evaluate_sliding(net, img, crop=CROP, **kw)
        assert len(seen) == 1 and seen[0][:2] == (n, 19), (kw, seen)
        _, _, (sn, sh, sw, sc), misaligned = seen.pop()
        assert sw == 20 and sc == 1 and sh % sw == 0 and sn % sh == 0 and misaligned == 0, (kw, (sn, sh, sw, sc), misaligned)
    harness.evaluate_sliding(net, img, crop=CROP, scales=(0.75, 1.0))
    assert len(seen) == 2 and all(s[2][2] == 20 and s[2][3] == 1 and s[3] == 0 for s in seen), seen
    # the stack holds the parts' values bit for bit, pad lanes zero
    parts = [harness.K.new((n, 5, 7, 19), img.cuda().float(), pitch_pad=True).copy_(rnd(n, 5, 7, 19, seed=n).cuda()) for n in (3, 1, 2)]
    low = harness.tile_stack(parts)
    assert low.stride() == (5 * 7 * 20, 7 * 20, 20, 1) and torch.equal(low, torch.cat(parts))
    assert bool((low.as_strided((6, 5, 7, 20), low.stride(), low.storage_offset())[..., 19] == 0).all())
    assert harness.tile_stack(parts[:1]) is parts[0] and harness.tile_stack([parts[0].contiguous()]).stride(2) == 20


def test_evaluate_sliding_restores_the_switch_when_a_forward_fails(harness, v3net):
    net = v3net
    with pytest.raises(AssertionError):                                                   # past the forward: a histogram of another class count
        harness.evaluate_sliding(net, image_u8(), image_labels(41), crop=CROP, hist=torch.zeros((3, 3), dtype=torch.int64, device='cuda'))
    assert net.eval_logits_lowres is False

    def boom(*a, **k):
        raise RuntimeError('forward failed')
    handle = net.register_forward_pre_hook(boom)
    try:
        with pytest.raises(RuntimeError, match='forward failed'):
            harness.evaluate_sliding(net, image_u8(), crop=CROP)
    finally:
        handle.remove()
    assert net.eval_logits_lowres is False


def test_evaluate_sums_the_histograms_and_reports_the_reference_metrics(harness, v3net):
    net = v3net
    loader = [(image_u8(31)[None], image_labels(41)[None], ['a']), (image_u8(32), image_labels(42), ['b'])]
    res = harness.evaluate(net, loader, crop=CROP, dump=1)
    parts = [harness.evaluate_sliding(net, img.reshape(*HW_IMG, 3), gt.reshape(HW_IMG), crop=CROP) for img, gt, _ in loader]
    assert res['hist'].dtype == torch.int64 and res['hist'].is_cuda and torch.equal(res['hist'], parts[0]['hist'] + parts[1]['hist'])
    assert len(res['predictions']) == 1 and torch.equal(res['predictions'][0], parts[0]['pred'])
    hist = res['hist'].cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):                          # utils/misc.py:138-147
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        freq = hist.sum(axis=1) / hist.sum()
        mean_iu, fwavacc = np.nanmean(iu), (freq[freq > 0] * iu[freq > 0]).sum()
    for name, want in (('acc', acc), ('acc_cls', acc_cls), ('mean_iu', mean_iu), ('fwavacc', fwavacc)):
        print(name, res[name], want)
        assert abs(res[name] - want) <= 1e-12 * max(1.0, abs(want))
    noflip = harness.evaluate(net, loader, crop=CROP, no_flip=True)
    single = harness.evaluate_sliding(net, loader[1][0], loader[1][1], crop=CROP, flips=(False,))
    assert noflip['hist'].sum().item() == res['hist'].sum().item() and noflip['predictions'] == []
    assert torch.equal(noflip['hist'] - harness.evaluate_sliding(net, loader[0][0][0], loader[0][1][0], crop=CROP, flips=(False,))['hist'], single['hist'])


def test_evaluate_sliding_serves_the_v2_family(harness):
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv2
    net = synth.load_det_weights(deepv2.DeepR101V2D(synth.model_args(), 19, CRIT, CRIT)).cuda()
    img, gt = image_u8(33, (97, 129)), image_labels(43, (97, 129))
    res = harness.evaluate_sliding(net, img, gt, crop=CROP, want_logits=True)
    assert torch.equal(res['pred'].long(), res['logits'].argmax(0)) and torch.equal(res['hist'], harness.fast_hist(res['pred'].long(), gt.cuda(), 19))
    assert res['hist'].sum().item() == int((gt != 255).sum()) and net.eval_logits_lowres is False
