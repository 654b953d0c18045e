"""GPU: relaxed-border training on the device -- the border-set words (pm_relax_border_bits, pm_multihot_to_bits), their class weights (pm_relax_class_weights), the
fused up-sample + ImgWtLossSoftNLL kernels (pm_upsample_relax_*), ops.upsample_relax and the criterion inside the networks -- against tests/golden/relax_cases.npz:
the reference's own targets, weight rows and fp32 losses, and the fp64 closed form for the gradient (tools/make_relax_golden.py; nothing here reads the reference).

Bounds are the project's bounds for the fused CE kernels (tests/test_hip_kernels.py::test_upsample_ce): loss 2e-6 max(1, |ref|) against the reference's fp32 loss,
gradient 2e-5 of the largest fp64 entry with an upstream scale of 1.7; valid counts exact; per-image losses 1e-6 relative against fp64."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load('make_relax_golden', 'tools', 'make_relax_golden.py')
N, GUARD, SENTINEL = G.N, 8, -12345.0
F32 = torch.float32


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


@pytest.fixture(scope='module')
def fx():
    with np.load(G.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def words_of(fx, key):
    """the fixture's target of case `key` as the int32 words the kernels take (CPU)"""
    return torch.from_numpy(G.words(G.load_target(fx, key)).astype(np.int64)).to(torch.int32)


def np_weights(target, upper_bound, norm, per_batch):
    """calculate_weights (loss.py:208-220) on the uint8 target [n, C + 1, H, W], numpy as the reference runs it; an image without a bit: ones"""
    rows = []
    with np.errstate(all='ignore'):
        for i in range(target.shape[0]):
            t = target if per_batch else target[i]
            hist = (np.sum(t, axis=(0, 2, 3)) if per_batch else np.sum(t, axis=(1, 2))) * 1.0 / t.sum()
            hist = ((hist != 0) * upper_bound * (1 / hist)) + 1 if norm else ((hist != 0) * upper_bound * (1 - hist)) + 1
            rows.append(np.ones_like(hist[:-1]) if t.sum() == 0 else hist[:-1])
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def same_bits(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=-7.0).view(torch.int32), torch.nan_to_num(want, nan=-7.0).view(torch.int32))


# ---- border sets and weights --------------------------------------------------------------------------------------------------------------------------------
def test_border_bits_equal_the_reference_targets(K, fx):
    """b = 1 on the eight loss shapes (a 611-wide row: more than two block strides; rows of 4 and 7), then b = 2 and 3, strict masks, labels of 200 and -1 as ignore,
    H or W of 1 and 2, and a row wider than one block's column chunk"""
    for case, (_, HW, _, C) in enumerate(G.LOSS_SHAPES):
        lab = torch.from_numpy(fx['L%d_labels' % case]).long().cuda()
        buf = torch.full((lab.numel() + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        got = K.relax_border_bits(lab, C, 1, 0, out=buf)
        assert torch.equal(got[:lab.numel()].view(lab.shape).cpu(), words_of(fx, 'L%d' % case)), case
        assert bool((buf[lab.numel():] == 0x5A5A5A5A).all())
    for name, (shape, classes, border, strict, _) in G.BORDER_CASES.items():
        lab = torch.from_numpy(fx[name + '_labels']).cuda()
        got = K.relax_border_bits(lab, classes, border, int(fx[name + '_strict']))
        assert torch.equal(got.cpu(), words_of(fx, name)), name
    assert any(s[0][1] == 1 for s in G.BORDER_CASES.values()) and any(s[0][2] == 1 for s in G.BORDER_CASES.values()) and any(s[0][2] > 1024 for s in G.BORDER_CASES.values())
    # border 0: the one-hot of the labels
    lab = torch.from_numpy(fx['L0_labels']).long()
    want = (torch.ones_like(lab) << torch.where(lab < 19, lab, torch.full_like(lab, 19))).to(torch.int32)
    assert torch.equal(K.relax_border_bits(lab.cuda(), 19, 0).cpu(), want)


def test_multihot_to_bits_gives_the_same_words(K, fx):
    for key in ['L%d' % c for c in range(len(G.LOSS_SHAPES))] + list(G.BORDER_CASES):
        target = torch.from_numpy(G.load_target(fx, key))
        n, _, H, W = target.shape
        buf = torch.full((n * H * W + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        got = K.multihot_to_bits((target * 3).cuda(), out=buf)       # non-zero = set
        assert torch.equal(got[:n * H * W].view(n, H, W).cpu(), words_of(fx, key)), key
        assert bool((buf[n * H * W:] == 0x5A5A5A5A).all())


FLAG_CASES = [(norm, ub, pb) for norm in (False, True) for ub in (1.0, 0.37) for pb in (False, True)]


def test_relax_class_weights_are_bit_equal_to_numpy(K, fx):
    for case, (_, _, _, C) in enumerate(G.LOSS_SHAPES):
        target = G.load_target(fx, 'L%d' % case)
        bits = words_of(fx, 'L%d' % case).cuda()
        for norm, ub, pb in FLAG_CASES:
            buf = torch.full((N * C + GUARD,), SENTINEL, device='cuda')
            got = K.relax_class_weights(bits, C, ub, norm, pb, out=buf)[:N * C].view(N, C).cpu()
            assert same_bits(got, np_weights(target, ub, norm, pb)), (case, norm, ub, pb)
            assert torch.equal(buf[N * C:].cpu(), torch.full((GUARD,), SENTINEL))
        for v in G.VARIANTS[case]:
            ub, norm, pb = G.ALL_VARIANTS[v]
            assert same_bits(K.relax_class_weights(bits, C, ub, norm, pb).cpu(), torch.from_numpy(fx['L%d_%s_w' % (case, v)])), (case, v)
    # an image without any bit (a caller's multi-hot): ones; a large image: more than one count block
    empty = words_of(fx, 'L1').clone()
    empty[1] = 0
    got = K.relax_class_weights(empty.cuda(), 19).cpu()
    target = G.load_target(fx, 'L1').copy()
    target[1] = 0
    assert torch.equal(got[1], torch.ones(19)) and same_bits(got, np_weights(target, 1.0, False, False))
    big = torch.from_numpy(np.tile(fx['L1_labels'], (1, 4, 8))).long().cuda()      # 192 x 384
    bits = K.relax_border_bits(big, 19, 1)
    tb = ((bits.cpu().unsqueeze(1) >> torch.arange(20).view(1, -1, 1, 1)) & 1).to(torch.uint8).numpy()
    for norm, ub, pb in FLAG_CASES:
        assert same_bits(K.relax_class_weights(bits, 19, ub, norm, pb).cpu(), np_weights(tb, ub, norm, pb)), (norm, ub, pb)


# ---- the fused loss ---------------------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def reference(fx, case, variant):
    """logits, words, weight rows (CPU), the reference's fp32 loss, the fp64 per-image losses and the fp64 gradient (upstream 1.7): once per (case, variant)"""
    key = (case, variant)
    if key not in _REFS:
        hw, HW, temp, C = G.LOSS_SHAPES[case]
        pre = 'L%d_%s_' % (case, variant)
        lg, bits, rows = G.logits(case), words_of(fx, 'L%d' % case), torch.from_numpy(fx[pre + 'w'])
        assert lg.double().sum().item() == float(fx['L%d_logit_sum' % case])
        lr = lg.double().requires_grad_(True)
        loss64, img64 = G.closed_form(F.interpolate(lr / temp, size=HW, mode='bilinear', align_corners=True), bits.long(), rows.double())
        (loss64 * G.GSCALE).backward()
        assert abs(loss64.item() - float(fx[pre + 'loss64'])) <= 1e-12 * max(1.0, abs(loss64.item()))
        assert abs(lr.grad.abs().max().item() - float(fx[pre + 'gmax'])) <= 1e-10 * float(fx[pre + 'gmax'])
        k = torch.from_numpy(G.load_target(fx, 'L%d' % case)[:, :C].astype(np.int64)).sum(1)
        _REFS[key] = dict(lg=lg, bits=bits, rows=rows, loss32=float(fx[pre + 'loss32']), img64=img64.detach(), grad=lr.grad, k=k)
    return _REFS[key]


def on_gpu(K, lg):
    n, C, h, w = lg.shape
    lgg = K.new((n, h, w, C), torch.zeros(1, device='cuda'), pitch_pad=True)
    lgg.copy_(nhwc(lg))
    return lgg


LOSS_CASES = [(case, v) for case in range(len(G.LOSS_SHAPES)) for v in ('img', 'batch')]


@pytest.mark.parametrize('case,variant', LOSS_CASES, ids=['L%d-%s' % c for c in LOSS_CASES])
def test_upsample_relax(K, fx, case, variant):
    hw, HW, temp, C = G.LOSS_SHAPES[case]
    R = reference(fx, case, variant)
    k = R['k']
    shares = [(k == 0).float().mean().item(), (k == 1).float().mean().item(), (k > 1).float().mean().item()]
    print('ignored / one class / several classes', shares)
    assert shares[0] >= 0.01 and shares[1] >= 0.10 and shares[2] >= 0.10
    lgg, bits, rows = on_gpu(K, R['lg']), R['bits'].cuda(), R['rows'].cuda()
    gs = torch.tensor([G.GSCALE], device='cuda')
    nout = 2 + 2 * N
    buf = torch.full((nout + GUARD,), SENTINEL, device='cuda')
    out, field = K.upsample_relax_fwd_field(lgg, bits, rows, 1.0 / temp, out=buf)
    print('loss', out[0].item(), 'ref32', R['loss32'], 'delta', abs(out[0].item() - R['loss32']))
    assert abs(out[0].item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32']))
    valid = (k > 0).flatten(1).sum(1)
    got = out.double().cpu()
    assert got[1].item() == valid.sum().item()
    print('per image', got[2:2 + N].tolist(), R['img64'].tolist())
    assert all(abs(got[2 + i].item() - R['img64'][i].item()) <= 1e-6 * abs(R['img64'][i].item()) for i in range(N))
    assert all(got[2 + N + i].item() == (valid[i].item() + 1) * N for i in range(N))
    assert torch.equal(buf[nout:].cpu(), torch.full((GUARD,), SENTINEL))
    dl = K.upsample_relax_bwd_field(lgg, HW, out, field, gs, 1.0 / temp)
    print('grad rel', rel(nchw(dl), R['grad']))
    assert rel(nchw(dl), R['grad']) < 2e-5
    # eval form: no field
    buf2 = torch.full((nout + GUARD,), SENTINEL, device='cuda')
    out_e = K.upsample_relax_fwd(lgg, bits, rows, 1.0 / temp, out=buf2)
    assert abs(out_e[0].item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32']))
    assert all(abs(out_e[i].item() - out[i].item()) <= 1e-6 * abs(out[i].item()) for i in range(nout))
    assert torch.equal(buf2[nout:].cpu(), torch.full((GUARD,), SENTINEL))
    # fixed association order everywhere: run-to-run deterministic
    out2, field2 = K.upsample_relax_fwd_field(lgg, bits, rows, 1.0 / temp)
    dl2 = K.upsample_relax_bwd_field(lgg, HW, out2, field2, gs, 1.0 / temp)
    assert torch.equal(out[:nout], out2) and torch.equal(field, field2) and torch.equal(dl, dl2)
    assert torch.equal(K.upsample_relax_fwd(lgg, bits, rows, 1.0 / temp), out_e[:nout])


@pytest.mark.parametrize('case', range(len(G.LOSS_SHAPES)))
def test_ignored_images_contribute_zero(K, fx, case):
    hw, HW, temp, C = G.LOSS_SHAPES[case]
    R = reference(fx, case, 'img')
    lgg, rows = on_gpu(K, R['lg']), R['rows'].cuda()
    bits = R['bits'].clone()
    bits[1] = 1 << C                                # every pixel of image 1 holds the ignore class alone
    want, img = G.closed_form(F.interpolate(R['lg'].double() / temp, size=HW, mode='bilinear', align_corners=True), bits.long(), R['rows'].double())
    for fwd in (lambda: K.upsample_relax_fwd(lgg, bits.cuda(), rows, 1.0 / temp), lambda: K.upsample_relax_fwd_field(lgg, bits.cuda(), rows, 1.0 / temp)[0]):
        out = fwd()
        assert out[3].item() == 0.0 and abs(out[0].item() - want.item()) < 2e-6 * max(1, abs(want.item())) and out[2 + N + 1].item() == N
    out, field = K.upsample_relax_fwd_field(lgg, bits.cuda(), rows, 1.0 / temp)
    dl = nchw(K.upsample_relax_bwd_field(lgg, HW, out, field, None, 1.0 / temp))
    assert dl[1].abs().max().item() == 0.0 and dl[0].abs().max().item() > 0.0 and bool(torch.isfinite(dl).all())
    # the whole batch ignored: 0 / (0 + 1), not NaN
    none = torch.full_like(bits, 1 << C).cuda()
    for fwd in (lambda: K.upsample_relax_fwd(lgg, none, rows, 1.0 / temp), lambda: K.upsample_relax_fwd_field(lgg, none, rows, 1.0 / temp)[0]):
        assert torch.equal(fwd()[:2 + N].cpu(), torch.zeros(2 + N))
    out, field = K.upsample_relax_fwd_field(lgg, none, rows, 1.0 / temp)
    assert K.upsample_relax_bwd_field(lgg, HW, out, field, None, 1.0 / temp)[..., :C].abs().max().item() == 0.0


@pytest.mark.parametrize('case', range(len(G.LOSS_SHAPES)))
def test_one_hot_sets_with_unit_weights_are_the_plain_fused_ce(K, fx, case):
    """bits straight from the labels (border 0) and all-ones weights: image i's loss is its mean CE times valid / (valid + 1) -- the new form tied to the existing one"""
    hw, HW, temp, C = G.LOSS_SHAPES[case]
    lg = G.logits(case)
    lab = torch.from_numpy(fx['L%d_labels' % case]).long().cuda()
    lgg = on_gpu(K, lg)
    out = K.upsample_relax_fwd_field(lgg, K.relax_border_bits(lab, C, 0), torch.ones(N, C, device='cuda'), 1.0 / temp)[0].double().cpu()
    total = 0.0
    for i in range(N):
        ce = K.upsample_ce_fwd(lgg[i:i + 1], lab[i:i + 1], 1.0 / temp).double().cpu()
        want = ce[0].item() * ce[1].item() / (ce[1].item() + 1)
        assert abs(out[2 + i].item() - want) <= 1e-6 * want, (i, out[2 + i].item(), want)
        total += want
    assert abs(out[0].item() - total / N) <= 1e-6 * total / N


# ---- views: every new entry point on strided logits inside poisoned slabs ------------------------------------------------------------------------------------------
# The (entry point, layout) pairs that are turned down. None: loss.hip reads and writes the logits element by element, so every pitch and base is served.
REFUSES = {}
VIEW_CASES = [0, 1, 4]      # interval-free small shape, row-staged forward, two rounds with carry


@pytest.mark.parametrize('layout', ['dense', 'slice', 'odd', 'ownpad'])
@pytest.mark.parametrize('case', VIEW_CASES)
def test_entry_points_on_views(fx, case, layout):
    """Raw ctypes calls as a foreign host makes them: logits and dlogits as view_slabs layouts (the network's pitch-20 layout among them), labels / target / bits /
    weights / loss_out / field between flat margins, exact workspaces. PM_OK with the bars above, every byte outside the views and every input byte unchanged."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import lib as L
    from test_tensor_views import Call
    env = (L, L.load())
    lib = env[1]
    hw, HW, temp, C = G.LOSS_SHAPES[case]
    (h, w), (H, W) = hw, HW
    R = reference(fx, case, 'img')
    shape = (N, h, w, C)
    lg = R['lg'].permute(0, 2, 3, 1)
    it = 1.0 / temp
    nout = lib.pm_upsample_relax_loss_floats(N)
    assert nout == 2 + 2 * N

    def run(c, *args):
        assert (c.entry, layout) not in REFUSES
        assert c.run(*args)

    # labels -> words, multi-hot -> words, words -> weights
    lab = torch.from_numpy(fx['L%d_labels' % case]).long()
    c = Call(env, 'pm_relax_border_bits', layout)
    bits = c.flat(lab.numel(), torch.int32, 'out')
    run(c, c.flat(lab.numel(), torch.int64, 'in', lab).data_ptr(), N, H, W, C, 1, 0, bits.data_ptr())
    assert torch.equal(bits.cpu().view(N, H, W), R['bits'])
    target = torch.from_numpy(G.load_target(fx, 'L%d' % case))
    c = Call(env, 'pm_multihot_to_bits', layout)
    bits2 = c.flat(lab.numel(), torch.int32, 'out')
    run(c, c.flat(target.numel(), torch.uint8, 'in', target).data_ptr(), N, C + 1, H, W, bits2.data_ptr())
    assert torch.equal(bits2.cpu().view(N, H, W), R['bits'])
    c = Call(env, 'pm_relax_class_weights', layout)
    wout = c.flat(N * C, F32, 'out')
    need = lib.pm_relax_class_weights_workspace(N)
    run(c, c.flat(lab.numel(), torch.int32, 'in', R['bits']).data_ptr(), N, H, W, C, 1.0, 0, 0, wout.data_ptr(), c.workspace(need), need)
    assert same_bits(wout.cpu().view(N, C), R['rows'])

    def start(entry):
        c = Call(env, entry, layout)
        view, _ = c.tensor(shape, F32, 'in', lg)
        return c, [view.data_ptr(), N, h, w, C, view.stride(2), it, c.flat(lab.numel(), torch.int32, 'in', R['bits']).data_ptr(), H, W,
                   c.flat(N * C, F32, 'in', R['rows']).data_ptr(), C]

    need = lib.pm_upsample_relax_workspace(N, H, W)
    c, args = start('pm_upsample_relax_fwd')
    out_e = c.flat(nout, F32, 'out')
    run(c, *args, out_e.data_ptr(), c.workspace(need), need)
    assert abs(out_e[0].item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32']))
    nfield = lib.pm_upsample_relax_field_bytes(N, h, w, C, H, W) // 4
    assert nfield == N * H * w * C
    c, args = start('pm_upsample_relax_fwd_field')
    out, field = c.flat(nout, F32, 'out'), c.flat(nfield, F32, 'out')
    run(c, *args, out.data_ptr(), field.data_ptr(), c.workspace(need), need)
    assert abs(out[0].item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32']))
    assert out[1].item() == (R['k'] > 0).sum().item()
    assert all(abs(out[2 + i].item() - R['img64'][i].item()) <= 1e-6 * abs(R['img64'][i].item()) for i in range(N))
    c = Call(env, 'pm_upsample_relax_bwd_field', layout)
    dl, _ = c.tensor(shape, F32, 'out')
    run(c, N, h, w, C, it, H, W, c.flat(nout, F32, 'in', out).data_ptr(), c.flat(1, F32, 'in', torch.tensor([G.GSCALE])).data_ptr(),
        c.flat(nfield, F32, 'in', field).data_ptr(), dl.data_ptr(), dl.stride(2))
    assert rel(dl.permute(0, 3, 1, 2), R['grad']) < 2e-5


def test_arguments_are_refused_before_any_launch(K):
    """status and message, nothing launched: classes beyond 31, a border beyond 3, a short workspace, a shape without a field"""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    x = torch.zeros(64, device='cuda')
    assert lib.pm_relax_border_bits(x.data_ptr(), 1, 2, 2, 32, 1, 0, x.data_ptr(), None) == -4 and b'classes' in lib.pm_last_error()
    assert lib.pm_relax_border_bits(x.data_ptr(), 1, 2, 2, 19, 4, 0, x.data_ptr(), None) == -4 and b'border' in lib.pm_last_error()
    need = lib.pm_upsample_relax_workspace(1, 2, 2)
    assert lib.pm_upsample_relax_fwd(x.data_ptr(), 1, 1, 1, 19, 19, 1.0, x.data_ptr(), 2, 2, x.data_ptr(), 0, x.data_ptr(), x.data_ptr(), need - 1, None) == -2
    assert lib.pm_upsample_relax_field_bytes(1, 2, 1100, 19, 3, 1100) == 0 and lib.pm_upsample_relax_field_bytes(1, 2, 900, 19, 3, 900) > 0
    assert lib.pm_upsample_relax_fwd_field(x.data_ptr(), 1, 2, 1100, 19, 19, 1.0, x.data_ptr(), 3, 1100, x.data_ptr(), 0, x.data_ptr(), x.data_ptr(), x.data_ptr(),
                                           lib.pm_upsample_relax_workspace(1, 3, 1100), None) == -4
    assert bool((x == 0).all())


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ops_upsample_relax_autograd(K, fx):
    """requires_grad logits in NCHW over NHWC memory; without a graph the eval kernel; a shape the size query turns down goes the composed route"""
    from pinthememory_amd.hip import ops
    case = 1
    hw, HW, temp, C = G.LOSS_SHAPES[case]
    R = reference(fx, case, 'img')
    x = R['lg'].cuda().to(memory_format=torch.channels_last).requires_grad_(True)
    bits, rows = R['bits'].cuda(), R['rows'].cuda()
    loss = ops.upsample_relax(x, bits, rows, 1.0 / temp)
    (loss * G.GSCALE).backward()
    assert abs(loss.item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32'])) and rel(x.grad, R['grad']) < 2e-5
    with torch.no_grad():
        assert abs(ops.upsample_relax(x, bits, rows, 1.0 / temp).item() - R['loss32']) < 2e-6 * max(1, abs(R['loss32']))
    # 1100 low-res columns: the rows do not fit LDS, resize + relaxed_soft_nll serve the call
    g = torch.Generator().manual_seed(11)
    lg = torch.randn(1, 19, 2, 1100, generator=g) * 3
    lab = torch.from_numpy(np.tile(fx['Bwide_labels'], (1, 1, 1)))
    bits = K.relax_border_bits(lab.cuda(), 19, 1)
    rows = K.relax_class_weights(bits, 19)
    assert not K.upsample_relax_ok(nhwc(lg), (3, 1100))
    lr = lg.double().requires_grad_(True)
    want, _ = G.closed_form(F.interpolate(lr, size=(3, 1100), mode='bilinear', align_corners=True), bits.cpu().long(), rows.cpu().double())
    (want * G.GSCALE).backward()
    x = lg.cuda().requires_grad_(True)
    loss = ops.upsample_relax(x, bits, rows)
    (loss * G.GSCALE).backward()
    assert abs(loss.item() - want.item()) < 2e-6 * max(1, abs(want.item())) and rel(x.grad, lr.grad) < 2e-5


# ---- model level ----------------------------------------------------------------------------------------------------------------------------------------------------
class RefRelax(nn.Module):
    """The oracle's criterion: the multi-hot target from the labels (loss.relaxed_border_target on the CPU: the reference's bytes, tests/test_relax_loss_cpu.py), then
    ImgWtLossSoftNLL as the reference evaluates it (loss.py:182-263): log(max(softmax, target * (softmax * target).sum(1))), weights from numpy on the host, one
    term per image over (pixels with a class + 1)."""

    def __init__(self, classes, upper_bound=1.0):
        super().__init__()
        self.classes, self.upper_bound = classes, upper_bound

    def forward(self, inputs, labels):
        from pinthememory_amd.loss import relaxed_border_target
        target = relaxed_border_target(labels.cpu(), self.classes)
        rows = np_weights(target.numpy(), self.upper_bound, False, False).to(inputs.dtype)
        t = target[:, :-1].to(inputs.dtype)
        k = t.sum(1)
        mask = k == 0
        soft = F.softmax(inputs, dim=1)
        logs = torch.log(torch.max(soft, t * (soft * t).sum(1, keepdim=True)))
        loss = 0.0
        for i in range(inputs.shape[0]):
            matrix = (-1 / k[i].masked_fill(mask[i], 1) * (t[i] * rows[i].view(-1, 1, 1) * logs[i]).sum(0)) * (1.0 - mask[i].to(inputs.dtype))
            loss = loss + matrix.sum() / (mask[i].numel() - mask[i].sum() + 1)
        return loss / inputs.shape[0]


def flags(**kw):
    a = dict(cls_wt_loss=False, img_wt_loss=False, jointwtborder=True, wt_bound=1.0, batch_weighting=False, strict_bdr_cls='', rlx_off_iter=-1)
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


def with_criteria(env, make_ref, make_net, ref_crit, crit):
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(make_ref(args, 19, PLAIN, PLAIN)).train()
    net = synth.load_det_weights(make_net(args, 19, PLAIN, PLAIN)).cuda().train()
    ref.criterion, net.criterion = ref_crit, crit
    return ref, net


def test_relaxed_criterion_in_the_network_vs_oracle(env):
    """2 x 128^2 training forward + backward of DeepV3Plus-R50 with the memory on and int64 labels under --jointwtborder: the memory and the auxiliary head see the
    labels, the main loss the border sets. The oracle evaluates the reference's expression on materialised logits."""
    synth, L = env['synth'], env['loss']
    crit, crit_val = L.get_loss(flags())
    assert type(crit) is L.ImgWtLossSoftNLL and crit_val.weight is None
    ref, net = with_criteria(env, env['o_deeplab'].DeepR50V3PlusD, env['deepv3plus'].DeepR50V3PlusD, RefRelax(19), crit)
    assert net.args.memory
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
    # a multi-hot target cannot feed the memory (nor stand in for the auxiliary labels): refused by name
    multihot = L.relaxed_border_target(y.cuda(), 19)
    with pytest.raises(ValueError, match='int64 labels'):
        net(x.cuda(), gts=multihot, aux_gts=y.cuda(), memory_writing=True, writing_detach=False)
    # the criterion called directly on materialised GPU logits, labels or multi-hot: the reference's loss
    lg = torch.randn(2, 19, 22, 22, generator=torch.Generator().manual_seed(5)) * 3
    small = y[:, ::6, ::6].contiguous()
    want = RefRelax(19)(lg, small).item()
    assert abs(crit(lg.cuda(), small.cuda()).item() - want) < 1e-5 * want
    assert abs(crit(lg.cuda(), L.relaxed_border_target(small, 19).cuda()).item() - want) < 1e-5 * want


def test_relaxed_criterion_in_deepv2_vs_oracle(env):
    synth, L = env['synth'], env['loss']
    ref, net = with_criteria(env, env['o_deeplab'].DeepR50V2D, env['deepv2'].DeepR50V2D, RefRelax(19, 0.37), L.get_loss(flags(wt_bound=0.37))[0])
    ref.dsn[3].p = net.dsn[3].p = 0.0
    x, y = synth.make_batch(2, 128, seed=22)
    with torch.no_grad():
        want = ref(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=True)
        got = net(x.cuda(), gts=y.cuda(), aux_gts=y.cuda(), memory_writing=True, writing_detach=True)
    print('loss1', float(got[0]), float(want[0]))
    assert abs(float(got[0]) - float(want[0])) <= 2e-4 * max(1.0, abs(float(want[0])))


def test_mldg_step_with_the_relaxed_criterion_vs_oracle(env):
    """harness.mldg_train_step reaches the criterion through the networks' forward alone: one 2 + 2 x 96^2 iteration under --jointwtborder against the fp32 oracle
    with the reference's expression, every loss of the step within the bound of test_mldg_step_vs_oracle (5e-4 max(1, |.|))."""
    import copy
    synth, L = env['synth'], env['loss']
    x, y = synth.make_batch(4, 96)

    def run(make, h, crit, xx, yy):
        net = synth.load_det_weights(make(synth.model_args(), 19, PLAIN, PLAIN))
        net = net.cuda() if xx.is_cuda else net
        net.criterion = crit
        net.dsn[3].p = 0.0
        u1, u2 = copy.deepcopy(net), copy.deepcopy(net)
        opt, _ = h.make_optimizer(net)
        return {k: v.item() for k, v in h.mldg_train_step(net, u1, u2, opt, xx[:2], yy[:2], xx[2:], yy[2:], inner_lr=1e-3).items()}
    want = run(env['o_deeplab'].DeepR50V3PlusD, env['o_harness'], RefRelax(19), x, y)
    got = run(env['deepv3plus'].DeepR50V3PlusD, env['harness'], L.get_loss(flags())[0], x.cuda(), y.cuda())
    print(got, want)
    assert set(got) >= set(want) and all(abs(got[k] - want[k]) < 5e-4 * max(1, abs(want[k])) for k in want)


def test_agg_step_with_the_relaxed_criterion_on_the_bf16_tier(env):
    """Tiers as upsample_wce: one 2 x 128^2 agg step under --jointwtborder on the bf16 tier beside the same step on the fp32 tier, every loss within 2.5e-3 --
    the bound the tier is held to with the plain criterion (test_model_parity.py, the bf16 eval / step test)."""
    synth, h, L = env['synth'], env['harness'], env['loss']
    from pinthememory_amd.hip import kernels as K
    x, y = synth.make_batch(2, 128, seed=23)

    def step():
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, PLAIN, PLAIN)).cuda().train()
        net.criterion = L.get_loss(flags())[0]
        net.dsn[3].p = 0.0
        opt, _ = h.make_optimizer(net)
        return {k: v.item() for k, v in h.agg_train_step(net, opt, x.cuda(), y.cuda()).items()}
    K.set_conv_precision('bf16')
    try:
        l16 = step()
    finally:
        K.set_conv_precision('f32')
    l32 = step()
    print(l16, l32)
    assert all(abs(l16[k] - l32[k]) < 2.5e-3 * max(1.0, abs(l32[k])) for k in l32)


def test_graphed_agg_step_with_the_relaxed_criterion(env):
    """No host sync on the way: the agg train step with the relaxed-border criterion is captured in a hipGraph, and three replays on fresh batches carry the bits of
    the same number of eager steps (state dict, losses, memory). Shape of test_graphed_agg_step_with_the_image_weighted_criterion."""
    synth, h, L = env['synth'], env['harness'], env['loss']

    def make():
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, PLAIN, PLAIN)).cuda()
        net.criterion = L.get_loss(flags())[0]
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
