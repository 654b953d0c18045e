"""CPU: relaxed-border training in pinthememory_amd.loss (get_loss's --jointwtborder branch, relaxed_border_target, ImgWtLossSoftNLL on the torch route) against
tests/golden/relax_cases.npz -- the reference's own RelaxedBoundaryLossToTensor / ImgWtLossSoftNLL outputs and the fp64 closed form (tools/make_relax_golden.py).
Bounds: loss 2e-6 max(1, |loss|) against the reference's fp32 loss, gradient 2e-5 of the largest fp64 entry (the bounds of the fused CE kernels)."""
import importlib.util
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pinthememory_amd import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('make_relax_golden', os.path.join(ROOT, 'tools', 'make_relax_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope='module')
def fx():
    with np.load(G.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_get_loss_returns_the_relaxed_criterion():
    crit, val = L.get_loss(Namespace(cls_wt_loss=False, img_wt_loss=False, jointwtborder=True, wt_bound=0.37, batch_weighting=True, strict_bdr_cls='2,5', rlx_off_iter=-1))
    assert type(crit) is L.ImgWtLossSoftNLL and type(val) is nn.CrossEntropyLoss and val.weight is None
    assert (crit.upper_bound, crit.batch_weights, crit.border_window, crit.strict_border_classes, crit.num_classes) == (0.37, True, 1, [2, 5], 19)
    crit, _ = L.get_loss(Namespace(cls_wt_loss=False, img_wt_loss=False, jointwtborder=True, wt_bound=1.0, strict_bdr_cls='', rlx_off_iter=-1))
    assert (crit.upper_bound, crit.batch_weights, crit.border_window, crit.strict_border_classes) == (1.0, False, 1, None)
    # the other branches are what they were
    assert type(L.get_loss(Namespace(img_wt_loss=True, jointwtborder=True, wt_bound=1.0))[0]) is L.ImageBasedCrossEntropyLoss2d
    assert type(L.get_loss(Namespace())[0]) is nn.CrossEntropyLoss


def test_the_relax_off_schedule_is_refused_by_name():
    with pytest.raises(NotImplementedError, match='rlx_off_iter'):
        L.get_loss(Namespace(jointwtborder=True, wt_bound=1.0, strict_bdr_cls='', rlx_off_iter=5000))


def test_jointwtborder_needs_the_companion_flags_the_reference_reads():
    """config.py:126-130 reads strict_bdr_cls and rlx_off_iter whenever jointwtborder is set; a namespace without them is refused by name"""
    for ns in (Namespace(jointwtborder=True, wt_bound=1.0), Namespace(jointwtborder=True, strict_bdr_cls=''), Namespace(jointwtborder=True, rlx_off_iter=-1)):
        with pytest.raises(NotImplementedError, match='jointwtborder.*companion'):
            L.get_loss(ns)


def test_relaxed_border_target_is_the_reference_target_byte_for_byte(fx):
    for case, (_, _, _, C) in enumerate(G.LOSS_SHAPES):
        want = torch.from_numpy(G.load_target(fx, 'L%d' % case))
        lab = torch.from_numpy(fx['L%d_labels' % case])
        got = L.relaxed_border_target(lab, C)
        assert got.dtype == torch.uint8 and torch.equal(got, want), case
        assert torch.equal(L.relaxed_border_target(lab[1].long(), C), want[1])          # one [H, W] map, as the transform sees it
    for name, (shape, classes, border, strict, _) in G.BORDER_CASES.items():
        want = torch.from_numpy(G.load_target(fx, name))
        assert tuple(want.shape) == (shape[0], classes + 1, shape[1], shape[2])
        got = L.relaxed_border_target(torch.from_numpy(fx[name + '_labels']), classes, border, strict)
        assert torch.equal(got, want), name
        assert int(fx[name + '_strict']) == L._strict_mask(strict)
    assert {'Bb2', 'Bstrict', 'B1x1', 'B2x5'} <= set(G.BORDER_CASES)


def test_multihot_and_label_input_give_the_same_words(fx):
    for case, (_, _, _, C) in enumerate(G.LOSS_SHAPES):
        crit = L.ImgWtLossSoftNLL(C)
        target = G.load_target(fx, 'L%d' % case)
        words = torch.from_numpy(G.words(target).astype(np.int64)).to(torch.int32)
        assert torch.equal(crit.border_bits(torch.from_numpy(target)), words)
        assert torch.equal(crit.border_bits(torch.from_numpy(fx['L%d_labels' % case]).long()), words)


CASES = [(case, v) for case in range(len(G.LOSS_SHAPES)) for v in G.VARIANTS[case]]


@pytest.mark.parametrize('case,variant', CASES, ids=['L%d-%s' % c for c in CASES])
def test_criterion_on_cpu_logits_meets_the_reference(fx, case, variant):
    (hw, HW, temp, C), (ub, norm, batch) = G.LOSS_SHAPES[case], G.ALL_VARIANTS[variant]
    pre = 'L%d_%s_' % (case, variant)
    crit = L.ImgWtLossSoftNLL(C, upper_bound=ub, norm=norm, batch_weights=batch)
    target, lab = torch.from_numpy(G.load_target(fx, 'L%d' % case)), torch.from_numpy(fx['L%d_labels' % case]).long()
    rows = crit.class_weights(crit.border_bits(lab))
    want_rows = torch.from_numpy(fx[pre + 'w'])
    assert torch.equal(torch.isnan(rows), torch.isnan(want_rows)) and torch.equal(torch.nan_to_num(rows, nan=-7.0).view(torch.int32), torch.nan_to_num(want_rows, nan=-7.0).view(torch.int32))
    if pre + 'loss32' not in fx:      # norm with a class no set holds: the reference's weight rows hold NaN and so does its loss; only the rows are compared
        assert norm and bool(torch.isnan(want_rows).any())
        return
    lg = G.logits(case)
    assert lg.double().sum().item() == float(fx['L%d_logit_sum' % case])
    if 'L%d_logits' % case in fx:
        assert torch.equal(lg, torch.from_numpy(fx['L%d_logits' % case]))
    lr = lg.double().requires_grad_(True)
    ref64, img64 = G.closed_form(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), torch.from_numpy(G.words(target.numpy()).astype(np.int64)),
                                 want_rows.double())
    (ref64 * G.GSCALE).backward()
    assert abs(ref64.item() - float(fx[pre + 'loss64'])) <= 1e-12 * max(1.0, abs(ref64.item()))
    assert abs(lr.grad.abs().max().item() - float(fx[pre + 'gmax'])) <= 1e-10 * float(fx[pre + 'gmax'])
    if pre + 'grad' in fx:
        assert (lr.grad - torch.from_numpy(fx[pre + 'grad'])).abs().max().item() <= 1e-12 * float(fx[pre + 'gmax'])
    loss32 = float(fx[pre + 'loss32'])
    for tgt in (target, lab):
        x = lg.clone().requires_grad_(True)
        got = crit(F.interpolate(x / temp, size=HW, mode='bilinear', align_corners=True), tgt)
        (got * G.GSCALE).backward()
        print(pre, 'loss', got.item(), 'ref32', loss32, 'ref64', ref64.item(), 'grad', ((x.grad.double() - lr.grad).abs().max() / lr.grad.abs().max()).item())
        assert abs(got.item() - loss32) < 2e-6 * max(1.0, abs(loss32))
        assert ((x.grad.double() - lr.grad).abs().max() / lr.grad.abs().max()).item() < 2e-5


def test_a_class_at_minus_200_outside_the_sets_gives_a_finite_loss(fx):
    """softmax underflows to exactly 0 for that class; the reference multiplies 0 by log 0 there"""
    _, HW, _, C = G.LOSS_SHAPES[1]
    lab = torch.from_numpy(fx['L1_labels']).long()
    lab[lab == 4] = 5                                   # class 4 is in no set
    x = (torch.randn(G.N, C, *HW, generator=torch.Generator().manual_seed(3)) * 3)
    x[:, 4] = -200.0
    x.requires_grad_(True)
    assert bool((F.softmax(x, dim=1)[:, 4] == 0).all())
    crit = L.ImgWtLossSoftNLL(C)
    for tgt in (lab, L.relaxed_border_target(lab, C)):
        x.grad = None
        loss = crit(x, tgt)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all()) and x.grad[:, 4].abs().max().item() == 0.0


def test_fully_ignored_images_contribute_zero():
    C = 19
    crit = L.ImgWtLossSoftNLL(C)
    x = torch.randn(2, C, 6, 7, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    lab = torch.full((2, 6, 7), 255)
    loss = crit(x, lab)
    loss.backward()
    assert loss.item() == 0.0 and x.grad.abs().max().item() == 0.0
    assert torch.equal(crit.class_weights(crit.border_bits(torch.zeros(2, C + 1, 6, 7, dtype=torch.uint8))), torch.ones(2, C))      # a target without any bit


def test_networks_refuse_a_multihot_target_where_the_reference_fails():
    """With the memory on, and where the auxiliary labels would alias gts, a multi-hot gts cannot work: a ValueError that says to pass int64 labels."""
    from pinthememory_amd.network import deepv3plus
    net = deepv3plus._Base.__new__(deepv3plus._Base)
    with pytest.raises(ValueError, match='int64 labels'):
        net._run_memory(None, torch.zeros(1, 20, 4, 4, dtype=torch.uint8), True, True)


def test_the_fixture_is_what_the_tool_writes():
    from oracle import import_reference
    if not import_reference.available():
        pytest.skip('the reference tree is not present')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_relax_golden.py'), '--check'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'identical' in out.stdout, out.stdout + out.stderr
