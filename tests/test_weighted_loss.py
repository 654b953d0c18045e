"""GPU: the weighted forms of the fused up-sample + cross-entropy kernels (pm_upsample_wce_*), the class weights from the labels (pm_label_class_weights) and
the criteria of pinthememory_amd.loss inside the networks, against the torch composition the reference runs (fp32 for the loss, fp64 for the gradient).

The restatement of the reference's image-based criterion (loss.py:136-163) lives here: its own expression with np.histogram(density=True) for the removed
normed=True. Loss / gradient bounds are the project's bounds for the unweighted kernels (tests/test_hip_kernels.py::test_upsample_ce)."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TABLE = [0.8373, 0.9180, 0.8660, 1.0345, 1.0166, 0.9969, 0.9754, 1.0489, 0.8786, 1.0023, 0.9539, 0.9843, 1.1116, 0.9037, 1.0865, 1.0955, 1.0865, 1.1529, 1.0507]
N = 3
GUARD = 8
SENTINEL = -12345.0


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---- the reference's criterion, restated (CPU, numpy) ------------------------------------------------------------------------------------------------
def ref_weights(target, classes, upper_bound=1.0, norm=False):
    """calculate_weights (loss.py:136-146), density=True for normed=True."""
    with np.errstate(all='ignore'):
        hist = np.histogram(target.flatten(), range(classes + 1), density=True)[0]
        if norm:
            hist = ((hist != 0) * upper_bound * (1 / hist)) + 1
        else:
            hist = ((hist != 0) * upper_bound * (1 - hist)) + 1
    return hist


def ref_weight_rows(lab, classes, upper_bound=1.0, norm=False, batch_weights=False):
    t = lab.numpy()
    return torch.stack([torch.Tensor(ref_weights(t if batch_weights else t[i], classes, upper_bound, norm)) for i in range(lab.shape[0])])


class RefImageBasedCE(nn.Module):
    """ImageBasedCrossEntropyLoss2d (loss.py:120-163) as the reference runs it: weights from numpy on the host, one nll_loss per image."""

    def __init__(self, classes, upper_bound=1.0, norm=False, batch_weights=False):
        super().__init__()
        self.classes, self.upper_bound, self.norm, self.batch_weights = classes, upper_bound, norm, batch_weights

    def forward(self, inputs, targets):
        rows = ref_weight_rows(targets.cpu(), self.classes, self.upper_bound, self.norm, self.batch_weights).to(inputs.dtype)
        loss = 0.0
        for i in range(inputs.shape[0]):
            loss = loss + F.nll_loss(F.log_softmax(inputs[i].unsqueeze(0), dim=1), targets[i].unsqueeze(0), weight=rows[i], reduction='mean', ignore_index=255)
        return loss


def compose(up, lab, w, per_image):
    """The torch composition on materialised logits `up`: CrossEntropyLoss(weight) over the batch, or the per-image sum of the image-based criterion."""
    w = w.to(up.dtype)
    if not per_image:
        return F.cross_entropy(up, lab, weight=w, ignore_index=255)
    lp = F.log_softmax(up, dim=1)
    return sum(F.nll_loss(lp[b:b + 1], lab[b:b + 1], weight=w[b], ignore_index=255) for b in range(up.shape[0]))


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [((5, 7), (33, 29), 2.0, 19),            # flat forward + interval field
          ((12, 12), (48, 48), 1.0, 19),          # row-staged forward
          ((6, 6), (96, 96), 0.5, 19),            # PARTS > 1
          ((7, 5), (30, 41), 1.0, 8),             # generic class count
          ((3, 300), (7, 611), 1.0, 19),          # two rounds with carry
          ((33, 65), (65, 129), 1.0, 19),         # interval form, several waves
          ((20, 256), (41, 520), 1.0, 19),        # interval form, three column segments
          ((16, 16), (16, 16), 1.0, 19),          # identity size: the aux loss
          ((9, 9), (4, 6), 1.0, 19)]              # down-sampling
MODES = ['global', 'image', 'batch']
_CASES = {}


def make_case(hw, HW, temp, C):
    """Inputs of one shape, computed once and never written: logits rnd * 3, labels with 10 % and the first two rows ignored, skewed per image."""
    key = (hw, HW, temp, C)
    if key not in _CASES:
        lg = rnd(N, C, *hw, seed=1) * 3
        g = torch.Generator().manual_seed(2)
        lab = torch.randint(0, C, (N, *HW), generator=g)
        lab[torch.rand(N, *HW, generator=g) < 0.1] = 255
        lab[:, :2] = 255
        lab[0][lab[0] == 3] = 0
        lab[1][(lab[1] > 9) & (lab[1] != 255)] = 1
        _CASES[key] = (lg, lab)
    return _CASES[key]


def on_gpu(K, lg, hw, C):
    lgg = K.new((N, hw[0], hw[1], C), torch.zeros(1, device='cuda'), pitch_pad=True)
    lgg.copy_(nhwc(lg))
    return lgg


def mode_weights(K, mode, lab, labg, C):
    """-> (weights on the GPU as the kernels take them, the same values on the CPU, per_image)."""
    if mode == 'global':
        # The gradient bound (2e-5 of the largest entry, against fp64) is close to what fp32 itself allows on the two wide two-fold shapes: ATen's fp32
        # align_corners coordinates (scale * X, X up to 610) carry ~2e-5 of a pixel. The torch composition in fp32, on the CPU, sits at 1.6e-5 ... 2.2e-5 of
        # fp64 on (3, 300) -> (7, 611) for the weight seeds 0 ... 5 (1.75, 2.14, 1.94, 2.17, 1.57, 2.16e-5) and at 1.2e-5 ... 1.6e-5 on (20, 256) -> (41, 520);
        # <= 1.5e-6 on every other shape. Seed 4 is the draw on which the reference itself keeps the most room under the bound.
        w = torch.rand(C, generator=torch.Generator().manual_seed(4)) + 0.5
        return w.cuda(), w, False
    rows = K.label_class_weights(labg, C, 1.0, False, mode == 'batch')
    return rows, rows.cpu(), True


_REFS = {}


def reference(key, lg, lab, HW, temp, w, per_image):
    """fp32 loss, fp64 gradient (upstream scale 1.7) and fp64 weight sums of the torch composition: once per (shape, mode)."""
    if key not in _REFS:
        lr = lg.double().requires_grad_(True)
        (compose(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), lab, w.double(), per_image) * 1.7).backward()
        loss32 = compose(F.interpolate(lg / temp, size=HW, mode='bilinear', align_corners=True), lab, w, per_image)
        rows = (w if w.dim() == 2 else w.expand(N, -1)).double()
        sums = torch.stack([rows[b][lab[b][lab[b] != 255]].sum() for b in range(N)])
        _REFS[key] = (loss32.item(), lr.grad, sums)
    return _REFS[key]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('hw,HW,temp,C', SHAPES)
def test_upsample_wce(K, hw, HW, temp, C, mode):
    lg, lab = make_case(hw, HW, temp, C)
    lgg, labg = on_gpu(K, lg, hw, C), lab.cuda()
    wg, w, per_image = mode_weights(K, mode, lab, labg, C)
    if mode != 'global':
        assert torch.equal(w, ref_weight_rows(lab, C, 1.0, False, mode == 'batch'))
    loss_ref, grad_ref, sums = reference((hw, HW, temp, C, mode), lg, lab, HW, temp, w, per_image)
    gs = torch.tensor([1.7], device='cuda')
    # training forward (loss + gradient field) and the row-pass backward; loss_out sits in a buffer with guard floats behind it
    buf = torch.full((2 + N + GUARD,), SENTINEL, device='cuda')
    out, field = K.upsample_wce_fwd_field(lgg, labg, wg, per_image, 1.0 / temp, out=buf)
    print('loss', out[0].item(), 'ref', loss_ref, 'delta', abs(out[0].item() - loss_ref))
    assert abs(out[0].item() - loss_ref) < 2e-6 * max(1, abs(loss_ref))
    dl = K.upsample_wce_bwd_field(lgg, HW, out, field, gs, per_image, 1.0 / temp)
    print('grad rel', rel(nchw(dl), grad_ref))
    assert rel(nchw(dl), grad_ref) < 2e-5
    got = out.double().cpu()
    print('weight sums', got[1:2 + N].tolist(), 'ref', sums.sum().item(), sums.tolist())
    assert abs(got[1].item() - sums.sum().item()) <= 1e-6 * sums.sum().item()
    assert all(abs(got[2 + b].item() - sums[b].item()) <= 1e-6 * sums[b].item() for b in range(N))
    assert torch.equal(buf[2 + N:].cpu(), torch.full((GUARD,), SENTINEL))
    # eval form: no field
    buf2 = torch.full((2 + N + GUARD,), SENTINEL, device='cuda')
    out_e = K.upsample_wce_fwd(lgg, labg, wg, per_image, 1.0 / temp, out=buf2)
    assert abs(out_e[0].item() - out[0].item()) <= 1e-6 * abs(out[0].item())
    assert abs(out_e[0].item() - loss_ref) < 2e-6 * max(1, abs(loss_ref))
    assert all(abs(out_e[i].item() - out[i].item()) <= 1e-6 * abs(out[i].item()) for i in range(1, 2 + N))
    assert torch.equal(buf2[2 + N:].cpu(), torch.full((GUARD,), SENTINEL))
    # fixed association order everywhere: run-to-run deterministic
    out2, field2 = K.upsample_wce_fwd_field(lgg, labg, wg, per_image, 1.0 / temp)
    dl2 = K.upsample_wce_bwd_field(lgg, HW, out2, field2, gs, per_image, 1.0 / temp)
    assert torch.equal(out[:2 + N], out2) and torch.equal(field, field2) and torch.equal(dl, dl2)
    assert torch.equal(K.upsample_wce_fwd(lgg, labg, wg, per_image, 1.0 / temp), out_e[:2 + N])


@pytest.mark.parametrize('hw,HW,temp,C', SHAPES)
def test_all_ones_weights_carry_the_bits_of_the_unweighted_kernels(K, hw, HW, temp, C):
    lg, lab = make_case(hw, HW, temp, C)
    lgg, labg = on_gpu(K, lg, hw, C), lab.cuda()
    gs = torch.tensor([1.7], device='cuda')
    out_u, field_u = K.upsample_ce_fwd_field(lgg, labg, 1.0 / temp)
    dl_u = K.upsample_ce_bwd_field(lgg, HW, out_u, field_u, gs, 1.0 / temp)
    for ones in (torch.ones(C, device='cuda'), torch.ones(N, C, device='cuda')):
        out_w, field_w = K.upsample_wce_fwd_field(lgg, labg, ones, False, 1.0 / temp)
        dl_w = K.upsample_wce_bwd_field(lgg, HW, out_w, field_w, gs, False, 1.0 / temp)
        assert torch.equal(out_w[:2], out_u) and torch.equal(field_w, field_u) and torch.equal(dl_w, dl_u)
        assert out_w[2:].sum().item() == out_u[1].item() == (lab != 255).sum().item()


@pytest.mark.parametrize('hw,HW,temp,C', SHAPES)
def test_one_image_fully_ignored(K, hw, HW, temp, C):
    lg, lab = make_case(hw, HW, temp, C)
    lab = lab.clone()
    lab[1] = 255
    lgg, labg = on_gpu(K, lg, hw, C), lab.cuda()
    w = torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5
    up = F.interpolate(lg / temp, size=HW, mode='bilinear', align_corners=True)
    # batch form: the image contributes nothing and receives exactly no gradient
    ref = compose(up, lab, w, False).item()
    for fwd in (lambda: K.upsample_wce_fwd(lgg, labg, w.cuda(), False, 1.0 / temp), lambda: K.upsample_wce_fwd_field(lgg, labg, w.cuda(), False, 1.0 / temp)[0]):
        out = fwd()
        assert abs(out[0].item() - ref) < 2e-6 * max(1, abs(ref)) and out[3].item() == 0.0
    out, field = K.upsample_wce_fwd_field(lgg, labg, w.cuda(), False, 1.0 / temp)
    dl = nchw(K.upsample_wce_bwd_field(lgg, HW, out, field, None, False, 1.0 / temp))
    assert dl[1].abs().max().item() == 0.0 and dl[0].abs().max().item() > 0.0 and bool(torch.isfinite(dl).all())
    # per-image form with a supplied finite weight row: 0 / 0 for that image, NaN as nll_loss gives
    rows = w.expand(N, -1).contiguous()
    assert torch.isnan(compose(up, lab, rows, True)).item()
    assert torch.isnan(K.upsample_wce_fwd(lgg, labg, rows.cuda(), True, 1.0 / temp)[0]).item()
    out_p, _ = K.upsample_wce_fwd_field(lgg, labg, rows.cuda(), True, 1.0 / temp)
    assert torch.isnan(out_p[0]).item() and out_p[3].item() == 0.0 and out_p[2].item() > 0.0


FLAG_CASES = [(norm, ub, bw) for norm in (False, True) for ub in (1.0, 0.37) for bw in (False, True)]


@pytest.mark.parametrize('shape', [(3, 33, 29), (3, 192, 768), (1, 1, 1)])
def test_label_class_weights_are_bit_equal_to_numpy(K, shape):
    n, H, W = shape
    g = torch.Generator().manual_seed(7)
    lab = torch.randint(0, 19, shape, generator=g)
    lab[torch.rand(shape, generator=g) < 0.1] = 255
    if n > 1:
        lab[0][lab[0] == 3] = 0
        lab[1][(lab[1] > 9) & (lab[1] != 255)] = 1
    cases = [lab]
    if n > 1:                                      # one image without a countable pixel: a NaN row (0 / 0), as numpy
        empty = lab.clone()
        empty[2] = 255
        cases.append(empty)
    else:
        cases.append(torch.full(shape, 255))
    for t in cases:
        tg = t.cuda()
        for norm, ub, bw in FLAG_CASES:
            want = ref_weight_rows(t, 19, ub, norm, bw)
            buf = torch.full((n * 19 + GUARD,), SENTINEL, device='cuda')
            got = K.label_class_weights(tg, 19, ub, norm, bw, out=buf)[:n * 19].view(n, 19).cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (norm, ub, bw)
            assert torch.equal(torch.nan_to_num(got, nan=-7.0).view(torch.int32), torch.nan_to_num(want, nan=-7.0).view(torch.int32)), (norm, ub, bw)
            assert torch.equal(buf[n * 19:].cpu(), torch.full((GUARD,), SENTINEL))
    assert torch.isnan(K.label_class_weights(cases[1].cuda(), 19)[-1]).all().item()
    # other class counts, labels outside [0, classes) are not counted
    got = K.label_class_weights(lab.cuda(), 8, 0.37).cpu()
    keep = torch.where(lab < 8, lab, torch.full_like(lab, 255))
    want = ref_weight_rows(keep, 8, 0.37)
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


def test_ops_upsample_wce_autograd(K):
    """The autograd function: same loss and gradient as the composition, through requires_grad logits in NCHW; without a graph the eval kernel."""
    from pinthememory_amd.hip import ops
    hw, HW, temp, C = SHAPES[1]
    lg, lab = make_case(hw, HW, temp, C)
    labg = lab.cuda()
    rows = K.label_class_weights(labg, C, 0.37)
    x = lg.cuda().requires_grad_(True)
    loss = ops.upsample_wce(x, labg, rows, True, 1.0 / temp)
    (loss * 1.7).backward()
    lr = lg.double().requires_grad_(True)
    ref = compose(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), lab, rows.cpu().double(), True)
    (ref * 1.7).backward()
    assert abs(loss.item() - ref.item()) < 2e-6 * max(1, abs(ref.item())) and rel(x.grad, lr.grad) < 2e-5
    with torch.no_grad():
        assert abs(ops.upsample_wce(x, labg, rows, True, 1.0 / temp).item() - ref.item()) < 2e-6 * max(1, abs(ref.item()))


# ---- model level ----------------------------------------------------------------------------------------------------------------------------------------
def flags(**kw):
    a = dict(cls_wt_loss=True, img_wt_loss=True, jointwtborder=False, wt_bound=1.0, batch_weighting=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope='module')
def env():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from oracle.ref_cpu import deeplab as o_deeplab, harness as o_harness
    from pinthememory_amd import harness, loss, synth
    from pinthememory_amd.network import deepv2, deepv3plus
    return dict(o_deeplab=o_deeplab, o_harness=o_harness, harness=harness, synth=synth, deepv2=deepv2, deepv3plus=deepv3plus, loss=loss)


PLAIN = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)


def with_criteria(env, make_ref, make_net, ref_crit, crit, aux):
    """(oracle, HIP net) with the deterministic weights, in train mode. The criteria are attached after the weights are loaded: a weighted criterion's class
    weights are a buffer of the model, not something the weight recipe should fill."""
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(make_ref(args, 19, PLAIN, PLAIN)).train()
    net = synth.load_det_weights(make_net(args, 19, PLAIN, PLAIN)).cuda().train()
    ref.criterion, ref.criterion_aux = ref_crit, nn.CrossEntropyLoss(weight=torch.Tensor(TABLE), reduction='mean', ignore_index=255)
    net.criterion, net.criterion_aux = crit, aux
    return ref, net


def test_weighted_criteria_in_the_network_vs_oracle(env):
    """2 x 128^2 training forward + backward of DeepV3Plus-R50 under --img_wt_loss --cls_wt_loss: the oracle runs the reference's criterion on materialised
    logits (numpy weights on the host), the HIP net the objects of loss.get_loss / get_loss_aux on the fused kernels."""
    synth, L = env['synth'], env['loss']
    crit, crit_val = L.get_loss(flags())
    aux = L.get_loss_aux(flags())
    assert type(crit) is L.ImageBasedCrossEntropyLoss2d and aux.weight is not None and crit_val.weight is None
    ref, net = with_criteria(env, env['o_deeplab'].DeepR50V3PlusD, env['deepv3plus'].DeepR50V3PlusD, RefImageBasedCE(19), crit, aux)
    ref.dsn[3].p = net.dsn[3].p = 0.0
    x, y = synth.make_batch(2, 128, seed=21)
    want = ref(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=False)
    got = net(x.cuda(), gts=y.cuda(), aux_gts=y.cuda(), memory_writing=True, writing_detach=False)
    for name, a, b in (('loss1', got[0], want[0]), ('loss2', got[1], want[1])):
        print(name, float(a), float(b))
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(b))), (name, float(a), float(b))
    env['o_harness'].total_loss(want).backward()
    env['harness'].total_loss(got).backward()
    torch.cuda.synchronize()
    print('final2 weight gradient rel', rel(net.final2[-1].weight.grad, ref.final2[-1].weight.grad))
    assert rel(net.final2[-1].weight.grad, ref.final2[-1].weight.grad) < 1e-3
    # the criterion called directly on materialised GPU logits (validation code): the same loss as the reference's
    lg = rnd(2, 19, 22, 22, seed=5) * 3
    small = y[:, ::6, ::6].contiguous()
    assert abs(crit(lg.cuda(), small.cuda()).item() - RefImageBasedCE(19)(lg, small).item()) < 1e-5 * RefImageBasedCE(19)(lg, small).item()


def test_weighted_criteria_in_deepv2_vs_oracle(env):
    synth, L = env['synth'], env['loss']
    ref, net = with_criteria(env, env['o_deeplab'].DeepR50V2D, env['deepv2'].DeepR50V2D, RefImageBasedCE(19, 0.37), L.get_loss(flags(wt_bound=0.37))[0], L.get_loss_aux(flags()))
    ref.dsn[3].p = net.dsn[3].p = 0.0
    x, y = synth.make_batch(2, 128, seed=22)
    with torch.no_grad():
        want = ref(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=True)
        got = net(x.cuda(), gts=y.cuda(), aux_gts=y.cuda(), memory_writing=True, writing_detach=True)
    print('loss1', float(got[0]), float(want[0]))
    assert abs(float(got[0]) - float(want[0])) <= 2e-4 * max(1.0, abs(float(want[0])))


def test_graphed_agg_step_with_the_image_weighted_criterion(env):
    """No host sync on the way: the agg train step with the image-weighted criterion and the class-weighted aux criterion is captured in a hipGraph, and three
    replays on fresh batches carry the bits of the same number of eager steps (state dict, losses, memory). Shape of test_graphed_agg_step_is_bit_identical_to_eager."""
    synth, h, L = env['synth'], env['harness'], env['loss']

    def make():
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, PLAIN, PLAIN)).cuda()
        net.criterion, net.criterion_aux = L.get_loss(flags())[0], L.get_loss_aux(flags())
        net.dsn[3].p = 0.0
        opt, sched = h.make_optimizer(net)
        return net, opt, sched
    batches = [tuple(t.cuda() for t in synth.make_batch(2, 128, seed=50 + i)) for i in range(3)]
    pre = 3
    prev = h.COMMIT_OVERLAP
    h.COMMIT_OVERLAP = False
    try:
        net_e, opt_e, sched_e = make()
        for i in range(pre + 3):
            x, y = batches[0] if i < pre else batches[(i - pre) % 3]
            le = h.agg_train_step(net_e, opt_e, x, y, sched=sched_e)
        net_g, opt_g, sched_g = make()
        g = h.GraphedAggStep(net_g, opt_g, batches[0][0], batches[0][1], sched=sched_g, warmup=3, pipelined=False)
        for i in range(3):
            lg = g.step(*batches[i % 3])
        torch.cuda.synchronize()
        for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), k
        assert all(torch.equal(le[k], lg[k]) for k in le) and bool(torch.isfinite(le['loss1']))
        assert torch.equal(net_e.memory.m_items, g.committed_memory())
        g.close()
    finally:
        h.COMMIT_OVERLAP = prev
