"""CPU: the criterion boundary pinthememory_amd.loss (the reference's loss.py:14-43,71-88,120-180), the dispatch of segmentation_loss onto the fused
weighted kernels, and the argument validation of the new C entry points. No GPU: the fused ops are replaced by recorders where they would be reached.

The restatement of the reference's image-based criterion below is its own expression (loss.py:136-163) with np.histogram(density=True) in place of the
removed normed=True."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pinthememory_amd import loss as L
from pinthememory_amd.hip import lib as HL

TABLE = [0.8373, 0.9180, 0.8660, 1.0345, 1.0166, 0.9969, 0.9754, 1.0489, 0.8786, 1.0023, 0.9539, 0.9843, 1.1116, 0.9037, 1.0865, 1.0955, 1.0865, 1.1529, 1.0507]


def ref_weights(target, classes, upper_bound, norm):
    """calculate_weights (loss.py:136-146), density=True for normed=True."""
    with np.errstate(all='ignore'):
        hist = np.histogram(target.flatten(), range(classes + 1), density=True)[0]
        if norm:
            hist = ((hist != 0) * upper_bound * (1 / hist)) + 1
        else:
            hist = ((hist != 0) * upper_bound * (1 - hist)) + 1
    return hist


def ref_image_loss(inputs, targets, classes, upper_bound=1.0, norm=False, batch_weights=False):
    """ImageBasedCrossEntropyLoss2d.forward (loss.py:148-163) -> (loss, weight rows)."""
    target_cpu = targets.numpy()
    rows = []
    loss = 0.0
    for i in range(inputs.shape[0]):
        w = torch.Tensor(ref_weights(target_cpu if batch_weights else target_cpu[i], classes, upper_bound, norm))
        rows.append(w)
        loss = loss + F.nll_loss(F.log_softmax(inputs[i].unsqueeze(0), dim=1), targets[i].unsqueeze(0), weight=w.to(inputs.dtype), reduction='mean', ignore_index=255)
    return loss, torch.stack(rows)


def labels_case(n=3, H=17, W=23, classes=19, seed=5, all_ignored=None):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, classes, (n, H, W), generator=g)
    lab[torch.rand(n, H, W, generator=g) < 0.1] = 255
    lab[:, :2] = 255
    lab[0][lab[0] == 3] = 0              # class 3 absent from image 0
    lab[1][(lab[1] > 9) & (lab[1] != 255)] = 1
    if all_ignored is not None:
        lab[all_ignored] = 255
    return lab


def flags(**kw):
    a = dict(cls_wt_loss=False, img_wt_loss=False, jointwtborder=False, wt_bound=1.0, batch_weighting=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_get_loss_returns_the_reference_criteria():
    crit, val = L.get_loss(flags())
    assert type(crit) is nn.CrossEntropyLoss and crit.weight is None and crit.ignore_index == 255 and crit.reduction == 'mean'
    assert type(val) is nn.CrossEntropyLoss and val.weight is None and val.ignore_index == 255 and val.reduction == 'mean'
    crit, val = L.get_loss(flags(cls_wt_loss=True))
    assert type(crit) is nn.CrossEntropyLoss and torch.equal(crit.weight.cpu(), torch.Tensor(TABLE)) and crit.ignore_index == 255 and crit.reduction == 'mean'
    assert val.weight is None
    for cls_wt in (False, True):         # the image-based criterion ignores --cls_wt_loss, as the reference does
        crit, val = L.get_loss(flags(img_wt_loss=True, cls_wt_loss=cls_wt, wt_bound=0.37))
        assert type(crit) is L.ImageBasedCrossEntropyLoss2d and crit.num_classes == 19 and crit.upper_bound == 0.37 and crit.ignore_index == 255
        assert crit.batch_weights is False and crit.norm is False and type(val) is nn.CrossEntropyLoss and val.weight is None
    crit, _ = L.get_loss(flags(img_wt_loss=True, batch_weighting=True))
    assert crit.batch_weights is True and crit.upper_bound == 1.0
    crit, _ = L.get_loss(flags(img_wt_loss=True, jointwtborder=True))      # loss.py:27-32: img_wt_loss is looked at first
    assert type(crit) is L.ImageBasedCrossEntropyLoss2d
    with pytest.raises(NotImplementedError, match='jointwtborder'):
        L.get_loss(flags(jointwtborder=True))


def test_get_loss_aux_carries_the_class_weight_table():
    aux = L.get_loss_aux(flags())
    assert type(aux) is nn.CrossEntropyLoss and aux.weight is None and aux.ignore_index == 255 and aux.reduction == 'mean'
    aux = L.get_loss_aux(flags(cls_wt_loss=True, img_wt_loss=True))
    assert type(aux) is nn.CrossEntropyLoss and aux.weight.dtype == torch.float32 and torch.equal(aux.weight.cpu(), torch.Tensor(TABLE))
    assert len(L.CLASS_WEIGHTS) == 19


def test_cross_entropy_loss_2d_is_the_references():
    x = torch.randn(2, 19, 9, 7, generator=torch.Generator().manual_seed(1))
    lab = labels_case(2, 9, 7)
    w = torch.Tensor(TABLE)
    for weight in (None, w):
        c = L.CrossEntropyLoss2d(weight=weight)
        assert torch.equal(c(x, lab), F.nll_loss(F.log_softmax(x, dim=1), lab, weight=weight, ignore_index=255))
        assert c.ignore_index == 255 and (c.weight is weight)


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('upper_bound', [1.0, 0.37])
@pytest.mark.parametrize('batch_weights', [False, True])
def test_image_based_criterion_on_cpu_tensors(norm, upper_bound, batch_weights):
    classes = 19
    lab = labels_case()
    x = torch.randn(3, classes, 17, 23, generator=torch.Generator().manual_seed(2)) * 3
    crit = L.ImageBasedCrossEntropyLoss2d(classes, upper_bound=upper_bound, norm=norm, batch_weights=batch_weights)
    want, rows = ref_image_loss(x, lab, classes, upper_bound, norm, batch_weights)
    got_rows = crit.class_weights(lab)
    assert got_rows.dtype == torch.float32 and got_rows.shape == (3, classes)
    assert torch.equal(torch.isnan(got_rows), torch.isnan(rows)) and torch.equal(torch.nan_to_num(got_rows, nan=-7.0), torch.nan_to_num(rows, nan=-7.0))      # bit-equal
    if not batch_weights:                # class 3 is absent from image 0: weight 1, or 0 * inf = NaN with norm -- never gathered by the loss
        assert torch.isnan(got_rows[0, 3]).item() if norm else got_rows[0, 3].item() == 1.0
    got = crit(x, lab)
    assert torch.isfinite(want) and abs(got.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item())), (got.item(), want.item())
    # the same loss written out: sum over images of sum w nll / sum w
    lp = F.log_softmax(x.double(), dim=1)
    tot = 0.0
    for b in range(3):
        m = lab[b] != 255
        wl = rows[b].double()[lab[b][m]]
        tot += (-(lp[b].permute(1, 2, 0)[m].gather(1, lab[b][m][:, None])[:, 0]) * wl).sum() / wl.sum()
    assert abs(got.item() - tot.item()) <= 2e-6 * max(1.0, abs(tot.item()))


@pytest.mark.parametrize('batch_weights', [False, True])
def test_image_based_criterion_with_one_image_fully_ignored(batch_weights):
    classes = 19
    lab = labels_case(all_ignored=2)
    x = torch.randn(3, classes, 17, 23, generator=torch.Generator().manual_seed(2))
    crit = L.ImageBasedCrossEntropyLoss2d(classes, upper_bound=0.37, batch_weights=batch_weights)
    want, rows = ref_image_loss(x, lab, classes, 0.37, False, batch_weights)
    got_rows = crit.class_weights(lab)
    assert torch.equal(torch.isnan(got_rows), torch.isnan(rows)) and torch.equal(torch.nan_to_num(got_rows, nan=-7.0), torch.nan_to_num(rows, nan=-7.0))
    assert bool(torch.isnan(got_rows[2]).all()) == (not batch_weights)      # 0 / 0: a NaN row, as numpy
    assert torch.isnan(want) and torch.isnan(crit(x, lab))                  # that image's nll_loss is 0 / 0 either way


def test_segmentation_loss_dispatch(monkeypatch):
    from pinthememory_amd.network import deepv3plus as D
    calls = []
    monkeypatch.setattr(D.ops, 'upsample_ce', lambda logits, labels, inv_temp=1.0: calls.append(('ce',)) or torch.zeros(()))
    monkeypatch.setattr(D.ops, 'upsample_wce', lambda logits, labels, weights, per_image, inv_temp=1.0: calls.append(('wce', weights, per_image)) or torch.zeros(()))
    x = torch.randn(3, 19, 17, 23, generator=torch.Generator().manual_seed(3))
    lab = labels_case()
    w = torch.Tensor(TABLE)

    def route(criterion, labels=lab):
        del calls[:]
        D.segmentation_loss(criterion, x, labels)
        return calls[0] if calls else ('composed',)
    assert route(nn.CrossEntropyLoss(ignore_index=255)) == ('ce',)
    assert route(L.CrossEntropyLoss2d()) == ('ce',)
    for crit in (nn.CrossEntropyLoss(weight=w, ignore_index=255), L.CrossEntropyLoss2d(weight=w), L.get_loss_aux(flags(cls_wt_loss=True)).cpu()):
        r = route(crit)
        assert r[0] == 'wce' and torch.equal(r[1].cpu(), w) and r[2] is False
    for bw in (False, True):
        crit = L.ImageBasedCrossEntropyLoss2d(19, upper_bound=0.37, batch_weights=bw)
        r = route(crit)
        assert r[0] == 'wce' and r[2] is True and torch.equal(r[1], ref_image_loss(x, lab, 19, 0.37, False, bw)[1])
    # anything else is composed from the materialised logits, as before
    assert route(nn.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=0.1)) == ('composed',)
    assert route(nn.CrossEntropyLoss(weight=w, ignore_index=255, reduction='sum')) == ('composed',)
    assert route(nn.CrossEntropyLoss(ignore_index=255, reduction='sum')) == ('composed',)
    clean = lab.clamp(max=18)            # another ignore_index: torch itself would refuse the label 255
    assert route(nn.CrossEntropyLoss(weight=w, ignore_index=-100), clean) == ('composed',)
    assert route(L.ImageBasedCrossEntropyLoss2d(19, ignore_index=-100), clean) == ('composed',)
    assert route(L.CrossEntropyLoss2d(weight=w, ignore_index=0), clean) == ('composed',)
    # fused_ce_ok keeps its meaning: the unweighted reference criterion only
    assert D.fused_ce_ok(nn.CrossEntropyLoss(ignore_index=255)) and not D.fused_ce_ok(nn.CrossEntropyLoss(weight=w, ignore_index=255))
    assert not D.fused_ce_ok(L.ImageBasedCrossEntropyLoss2d(19))


def test_weighted_entry_points_validate_their_arguments_without_gpu():
    """Null / inconsistent arguments are refused with PM_EINVAL and a message before anything touches the device."""
    lib = HL.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    lg = HL.PmTensor(p, 1, 2, 2, 19, 19)
    by = ctypes.byref
    assert lib.pm_upsample_wce_loss_floats(3) == 5
    assert lib.pm_upsample_wce_workspace(3, 33, 29) >= 3 * 33 * 2 * 8 and lib.pm_label_class_weights_workspace(3) > 0
    # no weights
    assert lib.pm_upsample_wce_fwd(by(lg), 1.0, p, 4, 4, None, 0, 0, p, p, 1 << 20, None) == -1 and b'upsample_wce_fwd: null weights' in lib.pm_last_error()
    assert lib.pm_upsample_wce_fwd_field(by(lg), 1.0, p, 4, 4, None, 0, 0, p, p, p, 1 << 20, None) == -1 and b'upsample_wce_fwd_field: null weights' in lib.pm_last_error()
    # no logits / labels
    assert lib.pm_upsample_wce_fwd(None, 1.0, p, 4, 4, p, 0, 0, p, p, 1 << 20, None) == -1 and b'upsample_wce_fwd' in lib.pm_last_error()
    assert lib.pm_upsample_wce_fwd(by(lg), 1.0, None, 4, 4, p, 0, 0, p, p, 1 << 20, None) == -1 and b'upsample_wce_fwd' in lib.pm_last_error()
    assert lib.pm_upsample_wce_fwd_field(by(lg), 1.0, None, 4, 4, p, 0, 0, p, p, p, 1 << 20, None) == -1 and b'upsample_wce_fwd_field' in lib.pm_last_error()
    # a row stride shorter than a row, a per_image that is no flag
    assert lib.pm_upsample_wce_fwd(by(lg), 1.0, p, 4, 4, p, 7, 0, p, p, 1 << 20, None) == -1 and b'weight_stride' in lib.pm_last_error()
    assert lib.pm_upsample_wce_fwd_field(by(lg), 1.0, p, 4, 4, p, 19, 2, p, p, p, 1 << 20, None) == -1 and b'per_image' in lib.pm_last_error()
    # too little workspace: PM_EWORKSPACE
    assert lib.pm_upsample_wce_fwd(by(lg), 1.0, p, 4, 4, p, 0, 0, p, p, 8, None) == -2 and b'workspace' in lib.pm_last_error()
    # backward: null loss_out / field / dlogits
    assert lib.pm_upsample_wce_bwd_field(by(lg), 1.0, 4, 4, 0, None, None, p, by(lg), None) == -1 and b'upsample_wce_bwd_field' in lib.pm_last_error()
    assert lib.pm_upsample_wce_bwd_field(by(lg), 1.0, 4, 4, 0, p, None, None, by(lg), None) == -1 and b'upsample_wce_bwd_field' in lib.pm_last_error()
    assert lib.pm_upsample_wce_bwd_field(by(lg), 1.0, 4, 4, 3, p, None, p, by(lg), None) == -1 and b'per_image' in lib.pm_last_error()
    # class weights from labels
    assert lib.pm_label_class_weights(None, 1, 4, 4, 19, 1.0, 0, 0, p, p, 1 << 20, None) == -1 and b'label_class_weights' in lib.pm_last_error()
    assert lib.pm_label_class_weights(p, 1, 4, 4, 19, 1.0, 0, 0, None, p, 1 << 20, None) == -1 and b'label_class_weights' in lib.pm_last_error()
    assert lib.pm_label_class_weights(p, 0, 4, 4, 19, 1.0, 0, 0, p, p, 1 << 20, None) == -1
    assert lib.pm_label_class_weights(p, 1, 4, 4, 33, 1.0, 0, 0, p, p, 1 << 20, None) == -4 and b'classes' in lib.pm_last_error()
    assert lib.pm_label_class_weights(p, 1, 4, 4, 19, 1.0, 0, 0, p, p, 8, None) == -2 and b'workspace' in lib.pm_last_error()
