"""ResNet-50/101 trunk whose forward runs on the HIP kernels. Mirrors the class surface and state_dict layout of
/root/reference/network/Resnet.py (Bottleneck :137-216 with its [x, w_arr] list protocol, ResNet :395-495,
resnet50/resnet101 :527-559). Served: the plain trunk (iw = 0) and the IBN trunks -- wt_layer values 3 / 4, nn.InstanceNorm2d without / with affine parameters as the
stem's bn1 and behind the residual add of a stage's last block (ops.instance_norm_act). Instance whitening (1, 2) and switchable whitening (5) are not."""
import torch
import torch.nn as nn

from . import mynn
from ..hip import ops

__all__ = ['ResNet', 'Bottleneck', 'resnet50', 'resnet101']


IN_VALUES = (0, 3, 4)      # wt_layer / iw values served: none, nn.InstanceNorm2d(affine=False), nn.InstanceNorm2d(affine=True)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, iw=0):
        super().__init__()
        assert iw in IN_VALUES, 'instance whitening is out of scope of the pinmem hot path (iw %r: 0, 3 and 4 are served)' % (iw,)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = mynn.Norm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = mynn.Norm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = mynn.Norm2d(planes * self.expansion)
        self.downsample = downsample
        self.stride = stride
        self.iw = iw
        if iw:                                         # Resnet.py:162-167: registered before relu, after downsample
            self.instance_norm_layer = nn.InstanceNorm2d(planes * self.expansion, affine=(iw == 4))
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x_tuple):
        if len(x_tuple) != 2:
            print("error!!!")
            return
        x, w_arr = x_tuple
        if self.iw:                                    # Resnet.py:199-214: out = bn3(conv3(..)); out += residual; out = instance_norm_layer(out); relu
            out = ops.conv_bn_act(x, self.conv1, self.bn1, relu=True)
            out = ops.conv_bn_act(out, self.conv2, self.bn2, relu=True)
            residual = x if self.downsample is None else ops.conv_bn_act(x, self.downsample[0], self.downsample[1], relu=False)
            out = ops.conv_bn_act(out, self.conv3, self.bn3, relu=False, residual=residual)
            return [ops.instance_norm_module(out, self.instance_norm_layer, relu=True), w_arr]
        if self.training and torch.is_grad_enabled() and all(c.bias is None for c in (self.conv1, self.conv2, self.conv3)):
            return [ops.bottleneck(x, self), w_arr]
        out = ops.conv_bn_act(x, self.conv1, self.bn1, relu=True)
        out = ops.conv_bn_act(out, self.conv2, self.bn2, relu=True)
        residual = x if self.downsample is None else ops.conv_bn_act(x, self.downsample[0], self.downsample[1], relu=False)
        out = ops.conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=residual)   # out += residual; relu
        return [out, w_arr]


class ResNet(nn.Module):
    def __init__(self, block, layers, wt_layer=None, num_classes=1000):
        self.inplanes = 64
        super().__init__()
        wt_layer = [0] * 7 if wt_layer is None else wt_layer
        check_wt_layer(wt_layer)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.InstanceNorm2d(64, affine=(wt_layer[2] == 4)) if wt_layer[2] else mynn.Norm2d(64)      # Resnet.py:412-417
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0], wt_layer=wt_layer[3])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, wt_layer=wt_layer[4])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, wt_layer=wt_layer[5])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, wt_layer=wt_layer[6])
        self.avgpool = nn.AvgPool2d(7, stride=1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        self.wt_layer = wt_layer
        for m in self.modules():                       # Resnet.py:441-448
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.SyncBatchNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1, wt_layer=0):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       mynn.Norm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, iw=0)]
        self.inplanes = planes * block.expansion
        for index in range(1, blocks):
            layers.append(block(self.inplanes, planes, iw=wt_layer if index == blocks - 1 else 0))      # Resnet.py:462-464: the stage's last block only
        return nn.Sequential(*layers)

    def forward(self, x):
        x = stem(self.conv1, self.bn1, x)
        x_tuple = self.layer4(self.layer3(self.layer2(self.layer1([x, []]))))
        return x_tuple[0]


def check_wt_layer(wt_layer):
    """The seven positions of --wt_layer (Resnet.py:400-465): two for the three-conv stem only the reference's R101-V3+ has (must stay 0), bn1, layer1 ... layer4."""
    assert len(wt_layer) == 7, 'wt_layer has seven positions'
    assert wt_layer[0] == 0 and wt_layer[1] == 0, 'wt_layer positions 0 and 1 belong to the three-conv stem, which this trunk does not have'
    assert all(v in IN_VALUES for v in wt_layer), 'whitening layers are out of scope (wt_layer values served: 0, 3, 4)'


def stem(conv1, bn1, x):
    """layer0: 7x7 s2 conv (input padded 3 -> 4 channels so every gathered row is one 16 B vector) + BN + ReLU + maxpool
    (Resnet.py:404-405,432,471-478). An IBN stem (bn1 an nn.InstanceNorm2d) runs conv -> instance norm + ReLU -> maxpool."""
    import torch.nn.functional as F
    from ..hip import kernels as K
    x4 = ops.nchw(K.nchw_to_nhwc(x.float(), c_pad=4)) if x.shape[1] == 3 else x
    w4 = F.pad(conv1.weight, (0, 0, 0, 0, 0, 4 - conv1.weight.shape[1])) if conv1.weight.shape[1] == 3 else conv1.weight
    if isinstance(bn1, nn.InstanceNorm2d):
        return ops.maxpool3x3s2(ops.instance_norm_module(ops.conv_raw(x4, w4, None, ops._geom(conv1)), bn1, relu=True))
    return ops.stem_tail(x4, w4, conv1, bn1)


def _pretrained(model, name):
    # The reference downloads ImageNet weights here (Resnet.py:535-539). There is no network on the build/bench
    # boxes; callers load checkpoints through forgiving_state_restore instead.
    return model


def resnet50(pretrained=True, wt_layer=None, **kwargs):
    return _pretrained(ResNet(Bottleneck, [3, 4, 6, 3], wt_layer=wt_layer, **kwargs), 'resnet50')


def resnet101(pretrained=True, wt_layer=None, **kwargs):
    return _pretrained(ResNet(Bottleneck, [3, 4, 23, 3], wt_layer=wt_layer, **kwargs), 'resnet101')
