"""Test helper (not a conftest): the IBN variant of the CPU oracle's DeepLabV3+ in stock torch ops.

oracle.ref_cpu restates only the whitening-free trunk. This builds its DeepR50V3PlusD with a zero wt_layer and then swaps in what the reference's
Resnet.py does for wt_layer values 3 / 4 (nn.InstanceNorm2d without / with affine parameters): position 2 replaces the stem's bn1, positions 3..6 give the LAST
block of layer1..layer4 an `instance_norm_layer` applied after the residual add and before the ReLU. Usable in fp32 and fp64 (`.double()`), on any device."""
import copy
import types

import torch.nn as nn

from oracle.ref_cpu import deeplab as o_deeplab


def _iw_forward(self, x):
    y = self.relu(self.bn1(self.conv1(x)))
    y = self.relu(self.bn2(self.conv2(y)))
    y = self.bn3(self.conv3(y))
    r = x if self.downsample is None else self.downsample(x)
    return self.relu(self.instance_norm_layer(y + r))


def ibn_blocks(net):
    """[(name, block)] of the blocks that carry an instance norm"""
    return [(n, m) for n, m in net.named_modules() if hasattr(m, 'instance_norm_layer')]


def build(args, num_classes, criterion, criterion_aux, factory=None):
    """The oracle's network for args.wt_layer in {0, 3, 4}^7 with positions 0 and 1 zero."""
    wt = list(args.wt_layer)
    assert len(wt) == 7 and wt[0] == 0 and wt[1] == 0 and all(v in (0, 3, 4) for v in wt), wt
    plain = copy.copy(args)
    plain.wt_layer = [0] * 7
    net = (factory or o_deeplab.DeepR50V3PlusD)(plain, num_classes, criterion, criterion_aux)
    net.args = args
    if wt[2]:
        net.layer0[1] = nn.InstanceNorm2d(64, affine=(wt[2] == 4))
    for layer, v in zip((net.layer1, net.layer2, net.layer3, net.layer4), wt[3:]):
        if v:
            blk = layer[len(layer) - 1]
            blk.instance_norm_layer = nn.InstanceNorm2d(blk.conv3.out_channels, affine=(v == 4))
            blk.forward = types.MethodType(_iw_forward, blk)
    return net
