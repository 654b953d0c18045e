"""CPU: the instance-norm (IBN) trunks without a GPU -- every refusal of pm_instnorm_fwd / pm_instnorm_bwd in front of any device call, the construction of the
networks for wt_layer values 3 / 4 (module types, where the instance norms sit, state_dict names, shapes and order against the reference's own list in
tests/golden/state_dict_v3plus_r50_ibn.json), what stays rejected, and -- where the reference tree is present -- the helper oracle of tests/ibn_oracle.py against the
imported reference, bit for bit."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from pinthememory_amd import synth
from pinthememory_amd.hip import lib as L
from pinthememory_amd.network import Resnet, deepv2, deepv3plus

import ibn_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WT = [0, 0, 4, 4, 4, 0, 0]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


def crit():
    return torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)


# ---- the C ABI refuses bad arguments before anything touches the device --------------------------------------------------------------------------------------------
N, H, W, C = 2, 5, 6, 16
BUF = ctypes.create_string_buffer(1 << 16)      # host memory: nothing below may dereference it
P = (ctypes.addressof(BUF) + 15) // 16 * 16


def fwd_args(**over):
    a = dict(x=P, y=P + 8192, n=N, h=H, w=W, c=C, x_pitch=C, y_pitch=C, dtype=L.PM_F32, gamma=P + 16384, beta=P + 16640, eps=1e-5, relu=1, mean=P + 17000 // 16 * 16,
             invstd=P + 18000 // 16 * 16, ws=P + 20480, ws_bytes=None, stream=None)
    a.update(over)
    if a['ws_bytes'] is None:
        a['ws_bytes'] = 1 << 40
    return list(a.values())


def bwd_args(**over):
    a = dict(dy=P, x=P + 4096, y=P + 8192, dx=P + 12288, n=N, h=H, w=W, c=C, dy_pitch=C, x_pitch=C, y_pitch=C, dx_pitch=C, dtype=L.PM_F32, gamma=P + 16384,
             mean=P + 17000 // 16 * 16, invstd=P + 18000 // 16 * 16, relu=1, dgamma=P + 19008, dbeta=P + 19520, ws=P + 20480, ws_bytes=None, stream=None)
    a.update(over)
    if a['ws_bytes'] is None:
        a['ws_bytes'] = 1 << 40
    return list(a.values())


FWD_REFUSALS = [
    ('null x', dict(x=None), EINVAL), ('null y', dict(y=None), EINVAL), ('null mean', dict(mean=None), EINVAL), ('null invstd', dict(invstd=None), EINVAL),
    ('null ws', dict(ws=None), EINVAL),
    ('n = 0', dict(n=0), EINVAL), ('h < 0', dict(h=-1), EINVAL), ('w = 0', dict(w=0), EINVAL), ('c = 0', dict(c=0), EINVAL),
    ('x pitch below c', dict(x_pitch=C - 4), EINVAL), ('y pitch below c', dict(y_pitch=8), EINVAL),
    ('x pitch off the fp32 vector', dict(x_pitch=C + 2), EINVAL), ('y pitch off the bf16 vector', dict(dtype=L.PM_BF16, y_pitch=C + 4), EINVAL),
    ('gamma without beta', dict(beta=None), EINVAL), ('beta without gamma', dict(gamma=None), EINVAL),
    ('unknown dtype', dict(dtype=2), EUNSUPPORTED), ('negative dtype', dict(dtype=-1), EUNSUPPORTED),
    ('c = 12', dict(c=12, x_pitch=12, y_pitch=12), EUNSUPPORTED), ('c = 4', dict(c=4), EUNSUPPORTED),
    ('short workspace', dict(ws_bytes='short'), EWORKSPACE), ('no workspace bytes', dict(ws_bytes=0), EWORKSPACE),
]
BWD_REFUSALS = [
    ('null dy', dict(dy=None), EINVAL), ('null x', dict(x=None), EINVAL), ('null dx', dict(dx=None), EINVAL), ('null y behind a ReLU', dict(y=None), EINVAL),
    ('null mean', dict(mean=None), EINVAL), ('null invstd', dict(invstd=None), EINVAL), ('null ws', dict(ws=None), EINVAL),
    ('n = 0', dict(n=0), EINVAL), ('h = 0', dict(h=0), EINVAL), ('w < 0', dict(w=-3), EINVAL), ('c < 0', dict(c=-8), EINVAL),
    ('dy pitch below c', dict(dy_pitch=8), EINVAL), ('dx pitch off the vector', dict(dx_pitch=C + 1), EINVAL), ('x pitch off the bf16 vector', dict(dtype=L.PM_BF16, x_pitch=C + 4), EINVAL),
    ('y pitch below c behind a ReLU', dict(y_pitch=0), EINVAL),
    ('unknown dtype', dict(dtype=7), EUNSUPPORTED), ('c = 20', dict(c=20, dy_pitch=20, x_pitch=20, y_pitch=20, dx_pitch=20), EUNSUPPORTED),
    ('short workspace', dict(ws_bytes='short'), EWORKSPACE),
]


def _call(fn, maker, over):
    lib = L.load()
    if over.get('ws_bytes') == 'short':
        over = dict(over, ws_bytes=lib.pm_instnorm_workspace(N, H, W, C) - 1)
    return getattr(lib, fn)(*maker(**over)), lib.pm_last_error()


@pytest.mark.parametrize('what,over,status', FWD_REFUSALS, ids=[r[0] for r in FWD_REFUSALS])
def test_fwd_refusals(what, over, status):
    code, msg = _call('pm_instnorm_fwd', fwd_args, over)
    assert code == status, (what, code, msg)
    assert b'instnorm_fwd' in msg


@pytest.mark.parametrize('what,over,status', BWD_REFUSALS, ids=[r[0] for r in BWD_REFUSALS])
def test_bwd_refusals(what, over, status):
    code, msg = _call('pm_instnorm_bwd', bwd_args, over)
    assert code == status, (what, code, msg)
    assert b'instnorm_bwd' in msg


def test_workspace_query_and_abi_number():
    lib = L.load()
    assert L.ABI_VERSION == 460 and lib.pm_version() == 460
    assert lib.pm_instnorm_workspace(0, 4, 4, 8) == 0 and lib.pm_instnorm_workspace(2, 4, -4, 8) == 0
    for shape in ((3, 1, 1, 8), (2, 7, 9, 8), (3, 49, 47, 264), (2, 16, 16, 512), (8, 384, 384, 64)):
        n, h, w, c = shape
        nb = lib.pm_instnorm_workspace(*shape)
        # at least the per-image sums of the backward pass behind one row of block partials per image, and no more than one partial row per 64 pixels
        assert nb % 256 == 0 and nb >= 2 * n * c * 2 * 4 and nb <= (n * ((h * w + 63) // 64) * c * 2 + n * c * 2) * 4 + 256, (shape, nb)
    hdr = open(os.path.join(ROOT, 'include', 'pinmem_hip.h')).read()
    assert '460:' in hdr and 'pm_tensor' not in hdr[hdr.index('size_t pm_instnorm_workspace'):hdr.index('/* dtype conversion between two views')]


# ---- construction -------------------------------------------------------------------------------------------------------------------------------------------
def build(wt, memory=True):
    return deepv3plus.DeepR50V3PlusD(synth.model_args(wt_layer=list(wt), memory=memory), 19, crit(), crit())


@pytest.mark.parametrize('wt', [[0, 0, 4, 4, 4, 0, 0], [0, 0, 3, 0, 0, 3, 3]], ids=['ibn_a', 'in_stem_l3_l4'])
def test_ibn_nets_build_with_the_right_modules(wt):
    net = build(wt)
    stem = net.layer0[1]
    assert isinstance(stem, nn.InstanceNorm2d) and stem.num_features == 64 and stem.affine == (wt[2] == 4) and not stem.track_running_stats
    assert stem.eps == 1e-5
    want = {}
    for name, layer, v in zip(('layer1', 'layer2', 'layer3', 'layer4'), (net.layer1, net.layer2, net.layer3, net.layer4), wt[3:]):
        for i, blk in enumerate(layer):
            last = i == len(layer) - 1
            assert blk.iw == (v if last else 0), (name, i)
            assert hasattr(blk, 'instance_norm_layer') == bool(last and v), (name, i)
            if last and v:
                m = blk.instance_norm_layer
                assert isinstance(m, nn.InstanceNorm2d) and m.affine == (v == 4) and m.num_features == blk.conv3.out_channels and m.eps == 1e-5
                want['%s.%d' % (name, i)] = v
    assert {n: m.iw for n, m in net.named_modules() if getattr(m, 'iw', 0)} == want
    assert sum(isinstance(m, nn.InstanceNorm2d) for m in net.modules()) == sum(1 for v in wt if v)
    # instance norms are no BatchNorm to anything that walks the tree
    from pinthememory_amd import harness
    assert not any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in net.modules() if isinstance(m, nn.InstanceNorm2d))
    assert harness._all_syncbn(net) is False and harness.set_mode(net, False) is net and not stem.training
    harness.set_mode(net, True)


def test_state_dict_matches_the_reference_list():
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_v3plus_r50_ibn.json')))
    assert len(want) == 398
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in build(WT).state_dict().items()]
    assert got == want
    names = [k for k, _, _ in got]
    for k in ('layer0.1.weight', 'layer0.1.bias', 'layer1.2.instance_norm_layer.weight', 'layer1.2.instance_norm_layer.bias', 'layer2.3.instance_norm_layer.weight',
              'layer2.3.instance_norm_layer.bias'):
        assert k in names
    assert not any(k.startswith('layer0.1.running') or k == 'layer0.1.num_batches_tracked' for k in names)
    plain = [k for k in build(WT, memory=False).state_dict()]
    assert plain == [k for k in names if not k.startswith('memory.')]
    # the helper oracle carries the same list: its weights load into the product net and back
    o = ibn_oracle.build(synth.model_args(wt_layer=WT), 19, crit(), crit())
    assert [[k, list(v.shape)] for k, v in o.state_dict().items()] == [[k, s] for k, s, _ in want]


@pytest.mark.parametrize('wt', [[0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 2, 0, 0, 0], [0, 0, 0, 0, 0, 0, 5], [0, 0, 5, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0], [0, 4, 0, 0, 0, 0, 0],
                                [1, 1, 1, 1, 1, 0, 0]])
def test_other_whitening_values_stay_rejected(wt):
    with pytest.raises(AssertionError):
        build(wt)
    with pytest.raises(AssertionError):
        Resnet.resnet50(wt_layer=wt)


def test_deepv2_and_whitening_flags_stay_rejected():
    for wt in ([0, 0, 4, 4, 4, 0, 0], [0, 0, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 4]):
        with pytest.raises(AssertionError):
            deepv2.DeepR50V2D(synth.model_args(wt_layer=wt), 19, crit(), crit())
    with pytest.raises(AssertionError):
        deepv3plus.DeepR50V3PlusD(synth.model_args(wt_layer=WT, use_wtloss=True), 19, crit(), crit())
    with pytest.raises(AssertionError):
        Resnet.Bottleneck(64, 16, iw=1)
    net = build(WT)
    x = torch.zeros(1, 3, 32, 32)
    for kw in (dict(cal_covstat=True), dict(visualize=True)):
        with pytest.raises(AssertionError):
            net(x, **kw)


def test_plain_train_step_is_there_and_refuses_a_memory_net():
    from pinthememory_amd import harness
    net = build(WT, memory=True)
    with pytest.raises(AssertionError):
        harness.plain_train_step(net, None, torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int64))


# ---- the helper oracle against the imported reference, bit for bit ------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('make_ibn_golden', os.path.join(ROOT, 'tools', 'make_ibn_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _oracle(memory, wt=WT):
    net = synth.load_det_weights(ibn_oracle.build(synth.model_args(wt_layer=list(wt), memory=memory), 19, crit(), crit()))
    net.dsn[3].p = 0.0
    return net


def test_helper_oracle_equals_the_reference_bit_for_bit():
    from oracle import import_reference as IR
    if not IR.available():
        pytest.skip('the reference tree is not on this machine')
    from oracle.ref_cpu import harness as o_harness
    tool = _tool()
    x, y = synth.make_batch(tool.BATCH, tool.SIZE)
    for memory in (True, False):
        ref, ora = tool.reference_net(memory), _oracle(memory)
        for (ka, va), (kb, vb) in zip(ref.state_dict().items(), ora.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        assert torch.equal(tool.eval_logits(ref, x), tool.eval_logits(ora, x)), memory
        if memory:
            lr, lo = (o_harness.agg_train_step(n, o_harness.make_optimizer(n)[0], x, y) for n in (ref, ora))
        else:
            lr, lo = (dict(zip(('loss1', 'loss2', 'total'), tool.plain_forward_backward(n, x, y))) for n in (ref, ora))
        for k in lr:
            assert torch.equal(lr[k], lo[k]), (memory, k, lr[k], lo[k])
        for (ka, pa), (kb, pb) in zip(ref.named_parameters(), ora.named_parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad)), (memory, ka)


def test_fixture_holds_what_the_helper_oracle_computes(golden):
    """Runs everywhere: the committed fixture against the helper oracle (which the test above ties to the reference where that is present). Summation order inside
    torch's CPU kernels may differ between hosts, so this one is not bit for bit: losses to 1e-5 relative, logits to 1e-4."""
    tool = _tool()
    x, y = synth.make_batch(tool.BATCH, tool.SIZE)
    with golden('ibn_v3plus_128.npz') as f:
        g = {k: f[k] for k in f.files}
    assert list(g['wt_layer']) == WT and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ibn_v3plus_128.npz')) < (1 << 20)
    for memory, pre in ((True, ''), (False, 'plain_')):
        ora = _oracle(memory)
        lg = tool.eval_logits(ora, x)
        assert np.abs(lg[:, :, ::8, ::8].numpy() - g[pre + 'sub']).max() <= 1e-4
        sure = g[pre + 'margin'].astype(np.float32) > 1e-3
        assert np.array_equal(lg.argmax(1).numpy()[sure], g[pre + 'argmax'][sure])
        if memory:
            from oracle.ref_cpu import harness as o_harness
            losses = o_harness.agg_train_step(ora, o_harness.make_optimizer(ora)[0], x, y)
        else:
            losses = dict(zip(('loss1', 'loss2', 'total'), tool.plain_forward_backward(ora, x, y)))
        for k, v in losses.items():
            assert abs(v.item() - float(g[pre + k])) <= 1e-5 * max(1.0, abs(float(g[pre + k]))), (pre, k)
        # the gradient fingerprint: the same parameters in the same order; norms within 5e-2, the cap tests/test_model_parity.py puts on any gradient of one batch
        # (equal to the last bit on the host that wrote the fixture; elsewhere another summation order can put a ReLU unit on the other branch)
        named = [(k, p) for k, p in ora.named_parameters() if p.grad is not None]
        assert [k for k, _ in named] == [str(k) for k in g[pre + 'grad_names']]
        for (k, p), want in zip(named, g[pre + 'grad_sums'][:, 2]):
            assert abs(p.grad.double().norm().item() - want) <= 5e-2 * want + 1e-6, (pre, k)      # + 1e-6: a bias in front of an instance norm has a zero gradient, round-off only
