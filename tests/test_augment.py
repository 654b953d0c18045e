"""GPU: the augmenting input edge (csrc/augment.hip) against tests/golden/augment_cases.npz, the bytes PIL and scipy produce for the same images and parameters
(tools/make_augment_golden.py; test_augment_cpu.py regenerates them). Colour stage bit-equal; blur within one level and, off the smooth ramp, a share of differing
pixels <= 1e-3; float output, labels, determinism and the prefetcher bit-equal to the plain kernels they extend."""
import numpy as np
import pytest
import torch

from pinthememory_amd import harness, input_edge
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

pytestmark = pytest.mark.gpu

CASES = 'abcde'
RAMP = ('c', 0)          # the only smooth image: its blurred values fall on integers, where the reference's truncation is a coin toss -- one-level cap only


@pytest.fixture(scope='module')
def fx(golden):
    with golden('augment_cases.npz') as f:
        return {k: f[k] for k in f.files}


def _params(fx, name, blur):
    n = fx[name + '_img'].shape[0]
    arr = K.aug_params(n)
    for i in range(n):
        b, c, s = (float(v) for v in fx[name + '_factors'][i])
        K.set_aug_image(arr[i], fx[name + '_order'][i], fx[name + '_enabled'][i], bool(fx[name + '_flip'][i]), float(fx[name + '_hue'][i]), b, c, s,
                        float(fx[name + '_sigma'][i]) if blur else 0.0)
    return arr


@pytest.fixture(scope='module')
def device_out(fx):
    """(float NHWC4, uint8) of every case, without and with the blur: computed once, shared, never modified."""
    out = {}
    for name in CASES:
        img = torch.from_numpy(fx[name + '_img']).cuda()
        for blur in (False, True):
            f4, u8 = K.augment_u8(img, _params(fx, name, blur), want_u8=True)
            out[name, blur] = (f4.cpu(), u8.cpu())
    return out


@pytest.mark.parametrize('name', CASES)
def test_colour_stage_is_bit_equal_to_pil(fx, device_out, name):
    got = device_out[name, False][1].numpy()
    want = fx[name + '_colour']
    bad = int((got != want).any(-1).sum())
    print('case %s: %d of %d pixels differ from PIL' % (name, bad, want[..., 0].size))
    assert got.shape == want.shape and bad == 0


@pytest.mark.parametrize('name', CASES)
def test_blur_is_within_one_level_of_scipy(fx, device_out, name):
    got = device_out[name, True][1].numpy().astype(np.int32)
    want = fx[name + '_blur'].astype(np.int32)
    for i in range(want.shape[0]):
        diff = np.abs(got[i] - want[i])
        share = float((diff != 0).any(-1).mean())
        print('case %s image %d sigma %.2f: max |diff| %d, share of differing pixels %.2e' % (name, i, fx[name + '_sigma'][i], diff.max(), share))
        assert diff.max() <= 1
        if (name, i) != RAMP:
            assert share <= 1e-3
        if fx[name + '_sigma'][i] == 0:
            assert diff.max() == 0


@pytest.mark.parametrize('name', CASES)
def test_float_output_is_the_plain_conversion_of_the_uint8_output(fx, device_out, name):
    for blur in (False, True):
        f4, u8 = device_out[name, blur]
        assert torch.equal(f4, K.image_u8_to_nhwc4(u8.cuda()).cpu()) and not f4[..., 3].any()
    assert torch.equal(K.augment_u8(torch.from_numpy(fx[name + '_img']).cuda(), _params(fx, name, True)).cpu(), device_out[name, True][0])      # without the uint8 output


def test_image_without_any_op_is_the_plain_conversion_of_the_input(fx, device_out):
    plain = K.image_u8_to_nhwc4(torch.from_numpy(fx['b_img'][:1]).cuda()).cpu()
    for blur in (False, True):
        assert torch.equal(device_out['b', blur][0][:1], plain)
        assert np.array_equal(device_out['b', blur][1][0].numpy(), fx['b_img'][0])
    other = K.image_u8_to_nhwc4(torch.from_numpy(fx['b_img'][:1]).cuda(), mean=(0.1, 0.2, 0.3), std=(0.5, 0.25, 2.0)).cpu()
    assert torch.equal(K.augment_u8(torch.from_numpy(fx['b_img'][:1]).cuda(), K.aug_params(1), mean=(0.1, 0.2, 0.3), std=(0.5, 0.25, 2.0)).cpu(), other)


def test_labels_flip_with_the_image(fx):
    g = torch.Generator().manual_seed(5)
    for n, h, w in ((3, 37, 53), (2, 5, 1), (4, 16, 300)):
        lab = torch.randint(0, 20, (n, h, w), generator=g).to(torch.uint8)
        lab[lab == 19] = 255
        lab[:, 0, 0] = 255                                                     # the ignore label is there at every size, first column: it must move with a flip
        arr = K.aug_params(n)
        flips = [i % 2 == 0 for i in range(n)]
        for p, f in zip(arr, flips):
            p.flip = int(f)
        got = K.labels_u8_to_i64(lab.cuda(), arr).cpu()
        want = torch.stack([torch.flip(lab[i].long(), [1]) if f else lab[i].long() for i, f in enumerate(flips)])
        assert got.dtype == torch.int64 and torch.equal(got, want) and (got == 255).any()
        assert torch.equal(K.labels_u8_to_i64(lab.cuda()).cpu(), lab.long())


def test_two_launches_give_identical_bytes(fx, device_out):
    img = torch.from_numpy(fx['b_img']).cuda()
    for _ in range(2):
        f4, u8 = K.augment_u8(img, _params(fx, 'b', True), want_u8=True)
        assert torch.equal(f4.cpu(), device_out['b', True][0]) and torch.equal(u8.cpu(), device_out['b', True][1])


def test_prefetcher_yields_the_bytes_of_prepare_batch_u8():
    """Three batches through depth 1: the device slots and the source's pinned buffers come round again. The hard (meta-test) domain is 1."""
    B, D, size = 2, 2, (64, 96)
    pf = input_edge.DevicePrefetcher(input_edge.SyntheticDomainSource(B, D, size, seed=7), augment=input_edge.PhotometricAugment(seed=5), hard_domains={1})
    twin, src = input_edge.PhotometricAugment(seed=5), input_edge.SyntheticDomainSource(B, D, size, seed=7)
    plain = input_edge.DevicePrefetcher(input_edge.SyntheticDomainSource(B, D, size, seed=7))
    changed = 0
    for _ in range(3):
        x, gt = pf.next()
        img, lab = next(src)
        img, lab = img.clone(), lab.clone()
        wx, wgt = harness.prepare_batch_u8(img, lab, augment=twin, hard=[False, True] * B)
        assert all(twin.last['applied'][1::2])
        assert x.shape == (B * D, 4, size[0], size[1]) and torch.equal(x, wx) and torch.equal(gt, wgt)
        px, pgt = plain.next()
        ox, ogt = harness.prepare_batch_u8(img, lab)
        assert torch.equal(px, ox) and torch.equal(pgt, ogt)
        assert torch.equal(ops.nhwc(ox), K.image_u8_to_nhwc4(img.reshape(-1, size[0], size[1], 3).cuda())) and torch.equal(ogt, lab.reshape(-1, *size).cuda().long())
        changed += int(not torch.equal(x, px))
        for i, f in enumerate(twin.last['flip']):
            assert torch.equal(gt[i], torch.flip(pgt[i], [1]) if f else pgt[i])
    assert changed == 3
    torch.cuda.synchronize()
