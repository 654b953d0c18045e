"""GPU: the validation sweep -- pm_upsample_eval (loss + predicted class + confusion matrix of the bilinearly up-sampled logits in one pass) against ATen's fp32
interpolation on the CPU, which is what the reference program runs, and harness.validate against the loop of train.py:847-939 restated on the CPU oracle.

The prediction map is compared exactly wherever the reference's own top-2 margin is at least MARGIN, and must name one of the reference's top two classes below
it. MARGIN = 1e-4 is more than twenty times the largest fp32 interpolation difference on these inputs (4.4e-6); the share of pixels below it is capped (SHARE_CAP)
so that the gate cannot hide the kernel. On the CPU that share is 0, 1.2e-4, 0, 0, 3.6e-4, 0 and 0 of the pixels for the first seven cases."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -12345
PRED_SENTINEL = 0xAB
MARGIN = 1e-4
SHARE_CAP = 0.005
CRIT = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


@pytest.fixture(scope='module')
def harness():
    from pinthememory_amd import harness
    return harness


@pytest.fixture(scope='module')
def v3net():
    """The HIP DeepLabV3+ (memory on) with the deterministic weights, shared by the caller tests: validate leaves it as it found it but for eval mode."""
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    return synth.load_det_weights(deepv3plus.DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# (n, C, (h, w), (H, W), seed)
CASES = [(2, 19, (5, 7), (33, 29), 0),
         (1, 19, (4, 230), (9, 900), 1),          # W > 768: past the three label registers of the row kernel
         (3, 19, (9, 13), (9, 13), 2),            # ratio 1
         (2, 7, (6, 5), (21, 40), 3),             # generic class count
         (1, 19, (12, 16), (45, 61), 4),
         (2, 19, (1, 1), (8, 8), 5),
         (2, 19, (9, 9), (4, 6), 6),              # down-sampling
         # enough hi-res rows that a block walks several of them: two and four rows per block, low-res rows handed from the lower to the upper LDS slot
         (2, 19, (64, 8), (512, 20), 7),
         (4, 19, (43, 6), (512, 16), 8)]
_CASES = {}


def labels_for(n, C, HW, seed):
    """As test_upsample_ce: uniform classes, 10 % set to 255, the first two rows 255."""
    g = torch.Generator().manual_seed(1000 + seed)
    lab = torch.randint(0, C, (n, *HW), generator=g)
    lab[torch.rand(n, *HW, generator=g) < 0.1] = 255
    lab[:, :2] = 255
    return lab


def ref_hist(pred, lab, C):
    k = (lab >= 0) & (lab < C)
    return torch.bincount(C * lab[k] + pred[k], minlength=C * C).view(C, C)


def make_case(n, C, hw, HW, seed):
    """Inputs and the fp32 CPU reference of one case, computed once and never written."""
    key = (n, C, hw, HW, seed)
    if key not in _CASES:
        lg = rnd(n, C, *hw, seed=seed) * 3
        lab = labels_for(n, C, HW, seed)
        up = F.interpolate(lg, size=HW, mode='bilinear', align_corners=True)
        top = up.topk(2, dim=1)
        _CASES[key] = dict(lg=lg, lab=lab, loss=F.cross_entropy(up, lab, ignore_index=255).item(), arg=up.argmax(1), top2=top.indices,
                           safe=(top.values[:, 0] - top.values[:, 1]) >= MARGIN, hist=ref_hist(up.argmax(1), lab, C))
    return _CASES[key]


def on_gpu(K, lg):
    n, C, h, w = lg.shape
    lgg = K.new((n, h, w, C), torch.zeros(1, device='cuda'), pitch_pad=True)
    lgg.copy_(nhwc(lg))
    assert lgg.stride(2) == (C + 3) // 4 * 4
    return lgg


def guarded(n, HW, C):
    """hist and pred inside larger buffers with sentinel margins on both sides."""
    hb = torch.full((C * C + 2 * GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
    pb = torch.full((n * HW[0] * HW[1] + 2 * GUARD,), PRED_SENTINEL, dtype=torch.uint8, device='cuda')
    return hb, hb[GUARD:GUARD + C * C].view(C, C), pb, pb[GUARD:GUARD + n * HW[0] * HW[1]].view(n, *HW)


def margins_untouched(hb, pb):
    return (bool((hb[:GUARD] == SENTINEL).all()) and bool((hb[-GUARD:] == SENTINEL).all())
            and bool((pb[:GUARD] == PRED_SENTINEL).all()) and bool((pb[-GUARD:] == PRED_SENTINEL).all()))


@pytest.mark.parametrize('n,C,hw,HW,seed', CASES)
def test_upsample_eval_against_aten_fp32(K, harness, n, C, hw, HW, seed):
    ref = make_case(n, C, hw, HW, seed)
    lab = ref['lab']
    lgg, labg = on_gpu(K, ref['lg']), lab.cuda()
    assert K.upsample_eval_ok(lgg, HW)
    hb, hist, pb, pred = guarded(n, HW, C)
    out, h_ret, p_ret = K.upsample_eval(lgg, labg, 1.0, hist=hist, accumulate=False, pred=pred)
    assert h_ret is hist and p_ret is pred
    # loss: the bounds test_upsample_ce holds the existing forward to
    print('loss', out[0].item(), 'ref', ref['loss'], 'delta', abs(out[0].item() - ref['loss']), 'valid', out[1].item())
    assert abs(out[0].item() - ref['loss']) < 2e-6 * max(1, abs(ref['loss']))
    assert out[1].item() == (lab != 255).sum().item()
    # prediction map
    p = pred.cpu().long()
    safe = ref['safe']
    share = 1.0 - safe.float().mean().item()
    print('below-margin share', share, 'pixels', int((~safe).sum()), 'disagreeing with the reference argmax', int((p != ref['arg']).sum()))
    assert share <= SHARE_CAP
    assert torch.equal(p[safe], ref['arg'][safe])
    assert bool(((p == ref['top2'][:, 0]) | (p == ref['top2'][:, 1]))[~safe].all())
    # histogram: exactly fast_hist of the kernel's own map; against the reference's within two counts per below-margin pixel with a countable label
    assert torch.equal(hist, harness.fast_hist(pred.long(), labg, C))
    countable = (lab >= 0) & (lab < C)
    assert hist.sum().item() == countable.sum().item()
    diff = (hist.cpu() - ref['hist']).abs().sum().item()
    print('hist |delta|', diff, 'allowed', 2 * int((~safe & countable).sum()))
    assert diff <= 2 * int((~safe & countable).sum())
    assert margins_untouched(hb, pb)
    # accumulation: a second call adds, a call with accumulate = 0 overwrites whatever was there
    single = hist.clone()
    K.upsample_eval(lgg, labg, 1.0, hist=hist, accumulate=True)
    assert torch.equal(hist, 2 * single)
    hist.fill_(SENTINEL)
    K.upsample_eval(lgg, labg, 1.0, hist=hist, accumulate=False)
    assert torch.equal(hist, single)
    assert margins_untouched(hb, pb)
    # determinism; without a prediction map the loss and the histogram carry the same bits
    out2, hist2, pred2 = K.upsample_eval(lgg, labg, 1.0, want_pred=True)
    assert torch.equal(out, out2) and torch.equal(hist2, single) and torch.equal(pred2, pred)
    out3, hist3, none = K.upsample_eval(lgg, labg, 1.0)
    assert none is None and torch.equal(out3, out) and torch.equal(hist3, single)
    # the loss is the unweighted forward's
    fwd = K.upsample_ce_fwd(lgg, labg, 1.0)
    assert abs(fwd[0].item() - out[0].item()) <= 2e-6 * max(1, abs(ref['loss'])) and fwd[1].item() == out[1].item()


def test_ties_go_to_the_lowest_class(K):
    """Classes 5 and 11 are 2.0 everywhere, every other logit 0: their interpolated values are bit-equal (as on the CPU, asserted here), and output.max(1)[1]
    names the lower one. All-zero logits: class 0."""
    HW = (10, 17)
    lg = torch.zeros(1, 19, 3, 4)
    lg[:, 5] = 2.0
    lg[:, 11] = 2.0
    up = F.interpolate(lg, size=HW, mode='bilinear', align_corners=True)
    assert torch.equal(up[:, 5], up[:, 11]) and bool((up[:, 5] > 1.0).all())
    assert bool((up.max(1)[1] == 5).all())
    lab = labels_for(1, 19, HW, 7)
    for logits, want in ((lg, 5), (torch.zeros(1, 19, 3, 4), 0)):
        out, hist, pred = K.upsample_eval(on_gpu(K, logits), lab.cuda(), 1.0, want_pred=True)
        assert bool((pred == want).all())
        assert hist[:, want].sum().item() == hist.sum().item() == (lab != 255).sum().item()
        assert torch.equal(hist[:, want].cpu(), torch.bincount(lab[lab != 255], minlength=19))


def test_all_pixels_ignored(K):
    n, C, hw, HW, seed = CASES[0]
    ref = make_case(n, C, hw, HW, seed)
    lab = torch.full((n, *HW), 255, dtype=torch.int64)
    hb, hist, pb, pred = guarded(n, HW, C)
    out, _, _ = K.upsample_eval(on_gpu(K, ref['lg']), lab.cuda(), 1.0, hist=hist, accumulate=False, pred=pred)
    assert torch.isnan(out[0]).item() and out[1].item() == 0.0
    assert not hist.any().item()
    p = pred.cpu().long()                                                        # still written, for every pixel
    assert torch.equal(p[ref['safe']], ref['arg'][ref['safe']])
    assert bool(((p == ref['top2'][:, 0]) | (p == ref['top2'][:, 1])).all())
    assert margins_untouched(hb, pb)


def test_labels_outside_the_classes_are_not_counted(K):
    """fast_hist's mask (utils/misc.py:65-70): only 0 <= label < C is counted. A label that is neither a class nor 255 still enters the loss's valid count, as in
    the unweighted forward."""
    n, C, hw, HW, seed = CASES[3]
    ref = make_case(n, C, hw, HW, seed)
    lab = ref['lab'].clone()
    lab[:, 5, ::3] = C + 2
    lab[:, 6, ::4] = -1
    lgg = on_gpu(K, ref['lg'])
    out, hist, pred = K.upsample_eval(lgg, lab.cuda(), 1.0, want_pred=True)
    assert hist.sum().item() == ((lab >= 0) & (lab < C)).sum().item()
    assert torch.equal(hist.cpu(), ref_hist(pred.cpu().long(), lab, C))
    fwd = K.upsample_ce_fwd(lgg, lab.cuda(), 1.0)
    assert abs(out[0].item() - fwd[0].item()) <= 2e-6 * max(1, abs(fwd[0].item()))
    assert out[1].item() == fwd[1].item() == (lab != 255).sum().item()


# ---- the caller ---------------------------------------------------------------------------------------------------------------------------------------
LOSS_TOL = 2e-4                # the model-level loss bound of tests/test_model_parity.py
LOGIT_TOL = 1e-3               # argmax_gate: class maps are compared where the oracle's top-2 margin exceeds 2 * LOGIT_TOL


def oracle_validate(net, batches, o_harness, classes=19):
    """train.py:847-939 on the CPU oracle net: CrossEntropyLoss(ignore_index=255), output.max(1)[1], fast_hist, the read loss through get_score, every batch's
    means weighted by n * H * W."""
    net.eval()
    loss_sum = read_sum = count = 0.0
    iou_acc = 0
    preds, safes = [], []
    for inputs, gt in batches:
        pixels = inputs.size(0) * inputs.size(2) * inputs.size(3)
        with torch.no_grad():
            outputs = net(inputs)
            output = outputs[0]
            query = F.normalize(outputs[-1].clone(), dim=1).permute(0, 2, 3, 1).contiguous()
            reading_loss = net.memory.get_score(query, gt, net.memory.m_items)[-1]
        read_sum += reading_loss.item() * pixels
        loss_sum += CRIT(output, gt).item() * pixels
        count += pixels
        predictions = output.max(1)[1]
        iou_acc = iou_acc + o_harness.fast_hist(predictions.numpy().flatten(), gt.numpy().flatten(), classes)
        top = output.topk(2, dim=1).values
        preds.append(predictions)
        safes.append((top[:, 0] - top[:, 1]) > 2 * LOGIT_TOL)
    return dict(val_loss=loss_sum / count, read_loss=read_sum / count, hist=torch.from_numpy(iou_acc), preds=preds, safes=safes)


def self_consistent(harness, res, batches, classes=19):
    """hist is exactly the sum of fast_hist of the returned maps, counts every countable label, and the figures derived from it are miou's."""
    own = sum(harness.fast_hist(p.long(), gt.cuda(), classes) for p, (_, gt) in zip(res['predictions'], batches))
    assert res['hist'].dtype == torch.int64 and res['hist'].is_cuda and torch.equal(res['hist'], own)
    assert res['hist'].sum().item() == sum(int(((gt >= 0) & (gt < classes)).sum()) for _, gt in batches)
    mean_iu, iu = harness.miou(res['hist'])
    assert res['mean_iu'] == mean_iu and torch.equal(res['iu'].nan_to_num(-1.0), iu.nan_to_num(-1.0))
    for p, (x, gt) in zip(res['predictions'], batches):
        assert p.dtype == torch.uint8 and tuple(p.shape) == tuple(gt.shape)


def test_validate_against_the_cpu_oracle(harness, v3net):
    from oracle.ref_cpu import deeplab as o_deeplab, harness as o_harness
    from pinthememory_amd import synth
    from pinthememory_amd.hip import ops
    from pinthememory_amd.network import deepv3plus
    args = synth.model_args()
    ref = synth.load_det_weights(o_deeplab.DeepR50V3PlusD(args, 19, CRIT, CRIT))
    net = v3net
    batches = [synth.make_batch(2, (96, 128), seed=21), synth.make_batch(1, (131, 203), seed=22)]
    want = oracle_validate(ref, batches, o_harness)
    x = batches[1][0].cuda()
    net.eval()
    with torch.no_grad():
        before = net(x)[0].clone()
    res = harness.validate(net, batches, CRIT)
    print('val_loss', res['val_loss'], 'ref', want['val_loss'], 'read_loss', res['read_loss'], 'ref', want['read_loss'])
    assert abs(res['val_loss'] - want['val_loss']) < LOSS_TOL * max(1, abs(want['val_loss']))
    assert abs(res['read_loss'] - want['read_loss']) < LOSS_TOL * max(1, abs(want['read_loss']))
    assert len(res['predictions']) == 2
    below = 0
    for p, o, safe in zip(res['predictions'], want['preds'], want['safes']):
        share = 1.0 - safe.float().mean().item()
        print('below-margin share', share, 'classes predicted', o.unique().numel())
        assert share <= 0.01
        assert torch.equal(p.cpu().long()[safe], o[safe])
        below += int((~safe).sum())
    self_consistent(harness, res, batches)
    diff = (res['hist'].cpu() - want['hist']).abs().sum().item()
    print('hist |delta| vs oracle', diff, 'allowed', 2 * below)
    assert diff <= 2 * below
    # criterion=None is the plain criterion
    none = harness.validate(net, batches)
    assert none['val_loss'] == res['val_loss'] and torch.equal(none['hist'], res['hist'])
    # fewer dumps: same histogram bits
    one = harness.validate(net, batches, CRIT, dump=1)
    assert len(one['predictions']) == 1 and torch.equal(one['hist'], res['hist']) and one['val_loss'] == res['val_loss']
    assert torch.equal(one['predictions'][0], res['predictions'][0])
    # the switch is restored, the net is left in eval mode and its default output is what it was
    assert net.eval_logits_lowres is False and not net.training
    with torch.no_grad():
        after = net(x)[0]
        assert tuple(after.shape) == (1, 19, 131, 203) and torch.equal(after, before)
        net.eval_logits_lowres = True
        try:
            outs = net(x)
        finally:
            net.eval_logits_lowres = False
    low = outs[0]
    assert low.dtype == torch.float32 and low.shape[:2] == (1, 19) and low.shape[2] < 131 and low.shape[3] < 203
    assert len(outs) == 3 and torch.equal(ops.resize(low, (131, 203)), before)
    # in training mode the switch changes nothing: the forward returns its losses
    assert deepv3plus._Base.eval_logits_lowres is False


def test_validate_restores_the_switch_when_a_batch_fails(harness, v3net):
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    net = v3net
    x, y = synth.make_batch(1, (96, 128), seed=21)
    with pytest.raises(AssertionError):
        harness.validate(net, [(x, y[:, :-1])])              # label size != image size (train.py:878)
    assert net.eval_logits_lowres is False


def test_validate_five_dimensional_batches_and_longer_tuples(harness, v3net):
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    net = v3net
    x, y = synth.make_batch(2, (96, 128), seed=21)
    flat = harness.validate(net, [(x, y)])
    deep = harness.validate(net, [(x.view(1, 2, 3, 96, 128), y.view(1, 2, 96, 128), ['a', 'b'], None)])
    assert deep['val_loss'] == flat['val_loss'] and deep['read_loss'] == flat['read_loss'] and torch.equal(deep['hist'], flat['hist'])
    assert torch.equal(deep['predictions'][0], flat['predictions'][0])


def test_validate_serves_the_v2_family(harness):
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv2
    net = synth.load_det_weights(deepv2.DeepR101V2D(synth.model_args(), 19, CRIT, CRIT)).cuda()
    batches = [synth.make_batch(1, (97, 129), seed=23)]
    res = harness.validate(net, batches, CRIT)
    self_consistent(harness, res, batches)
    assert math.isfinite(res['val_loss']) and math.isfinite(res['read_loss'])
    assert net.eval_logits_lowres is False


def test_validate_composed_route_for_another_criterion(harness, v3net):
    """label_smoothing makes fused_ce_ok false: resize + criterion + argmax + fast_hist on the device. The loss is torch's on the materialised logits of the same net."""
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    assert not deepv3plus.fused_ce_ok(nn.CrossEntropyLoss(ignore_index=255, label_smoothing=0.1))
    crit = nn.CrossEntropyLoss(ignore_index=255, label_smoothing=0.1)
    net = v3net
    batches = [synth.make_batch(2, (96, 128), seed=21), synth.make_batch(1, (131, 203), seed=22)]
    res = harness.validate(net, batches, crit)
    self_consistent(harness, res, batches)
    net.eval()
    num = den = 0.0
    with torch.no_grad():
        for x, y in batches:
            num += crit(net(x.cuda())[0].cpu(), y).item() * y.numel()
            den += y.numel()
    print('composed val_loss', res['val_loss'], 'ref', num / den)
    assert abs(res['val_loss'] - num / den) < 2e-6 * max(1, abs(num / den))
    # the fused route on the same batches: same class maps wherever the composed route's argmax is the lowest index of its maxima, i.e. everywhere but exact ties
    fused = harness.validate(net, batches, CRIT)
    agree = sum(int((a == b).sum()) for a, b in zip(fused['predictions'], res['predictions']))
    assert agree >= 0.9999 * sum(y.numel() for _, y in batches)
