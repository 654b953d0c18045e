"""CPU: the host side of the augmenting input edge -- blur weights, argument validation in front of any device call, the parameter sampler, and the
fixture tests/golden/augment_cases.npz against the PIL + scipy pipeline that wrote it (tools/make_augment_golden.py). No GPU here."""
import ctypes
import importlib.util
import inspect
import math
import os
from ctypes import byref

import numpy as np
import pytest
import torch

from pinthememory_amd import harness, input_edge
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('make_augment_golden', os.path.join(ROOT, 'tools', 'make_augment_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_blur_weights_are_the_scipy_formula_bit_for_bit():
    """scipy.ndimage._gaussian_kernel1d: radius = int(4 sigma + 0.5), phi = exp(-0.5 / sigma^2 * x^2) over x = -radius .. radius, phi / phi.sum(). The formula is evaluated
    here with the correctly rounded scalar exp (math.exp) and numpy's own sum, and held bit for bit. numpy's VECTOR exp is not the yardstick: on an AVX-512 host it is
    off by one ulp for 3.4 % of the arguments of this formula (268 of 7 818 against a 60-digit evaluation; libm: 3), among them k = +-1 at sigma = 1.3, and on other hosts
    it is libm's -- so the tool's np.exp weights are held to one ulp, and what that ulp does to the blurred bytes is inside the blur test's share."""
    tool = _tool()
    for sigma in tool.SIGMAS:
        radius, w = K.aug_blur_weights(sigma)
        assert radius == int(4.0 * sigma + 0.5) and 1 <= radius <= 5
        x = np.arange(-radius, radius + 1)
        phi = np.array([math.exp(v) for v in (-0.5 / (sigma * sigma) * x ** 2)], dtype=np.float64)
        want = phi / phi.sum()
        assert w[:radius + 1] == list(want[radius:]), sigma
        assert w[radius + 1:] == [0.0] * (5 - radius)
        r2, w2 = tool.blur_weights(sigma)
        assert r2 == radius and all(abs(a - b) <= np.spacing(b) for a, b in zip(w, w2)), sigma


@pytest.mark.parametrize('sigma', [0.0, -1.0, 1.375, 2.0, float('nan')])
def test_blur_weights_refuse_a_sigma_whose_radius_is_not_served(sigma):
    lib = L.load()
    r, w = ctypes.c_int32(), (ctypes.c_double * 6)()
    assert lib.pm_aug_blur_weights(sigma, byref(r), w) == -4 and b'aug_blur_weights' in lib.pm_last_error()      # PM_EUNSUPPORTED
    assert lib.pm_aug_blur_weights(1.0, None, w) == -1                                                             # PM_EINVAL
    with pytest.raises(L.PinmemError):
        K.aug_blur_weights(sigma)
    r, w = K.aug_blur_weights(1.3749)
    assert r == 5


def test_argument_validation_happens_before_anything_touches_a_device():
    """Fake aligned pointers, no GPU in this container: every refusal below returns before a launch or a memset."""
    lib = L.load()
    size = ctypes.sizeof(L.PmAugImage)
    assert size == 72
    IMG, PAR, OUT4, OUT8, WS = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.pm_augment_workspace(8) == 64 and lib.pm_augment_workspace(0) == 0
    call = lib.pm_augment_u8
    assert call(IMG, 2, 8, 8, PAR, size - 8, m, m, OUT4, OUT8, WS, 16, None) == -1 and b'struct_size' in lib.pm_last_error()
    assert call(None, 2, 8, 8, PAR, size, m, m, OUT4, OUT8, WS, 16, None) == -1 and b'augment_u8' in lib.pm_last_error()
    assert call(IMG, 2, 8, 8, None, size, m, m, OUT4, OUT8, WS, 16, None) == -1
    assert call(IMG, 2, 0, 8, PAR, size, m, m, OUT4, OUT8, WS, 16, None) == -1
    assert call(IMG, -1, 8, 8, PAR, size, m, m, OUT4, OUT8, WS, 16, None) == -1
    assert call(IMG, 2, 8, 8, PAR, size, None, m, OUT4, OUT8, WS, 16, None) == -1
    assert call(IMG, 2, 8, 8, PAR, size, m, m, None, None, WS, 16, None) == -1 and b'no output' in lib.pm_last_error()
    assert call(IMG, 2, 8, 8, PAR, size, m, m, OUT4 + 4, None, WS, 16, None) == -1 and b'aligned' in lib.pm_last_error()
    assert call(IMG, 2, 8, 8, PAR, size, m, m, None, IMG, WS, 16, None) == -1                                      # in place: the halo would read augmented pixels
    assert call(IMG, 2, 8, 8, PAR, size, m, m, OUT4, None, WS, 15, None) == -2 and b'workspace' in lib.pm_last_error()      # PM_EWORKSPACE
    assert call(IMG, 2, 8, 8, PAR, size, m, m, OUT4, None, None, 16, None) == -2
    assert call(IMG, 70000, 8, 8, PAR, size, m, m, OUT4, None, WS, 1 << 20, None) == -4
    lab = lib.pm_labels_u8_flip_to_i64
    assert lab(IMG, 2, 8, 8, PAR, size + 8, OUT4, None) == -1 and b'struct_size' in lib.pm_last_error()
    assert lab(None, 2, 8, 8, PAR, size, OUT4, None) == -1 and b'labels_u8_flip_to_i64' in lib.pm_last_error()
    assert lab(IMG, 2, 8, 8, None, size, OUT4, None) == -1
    assert lab(IMG, 2, 8, 8, PAR, size, None, None) == -1
    assert lab(IMG, 2, 8, 0, PAR, size, OUT4, None) == -1


def test_binding_validates_what_the_device_cannot_report():
    p = K.aug_params(2)
    p[1].order[:] = (0, 1, 1, 3)
    with pytest.raises(ValueError, match='permutation'):
        K.upload_aug_params(p, torch.device('cpu'))
    p = K.aug_params(2)
    p[0].radius = 6
    with pytest.raises(ValueError, match='radius'):
        K.upload_aug_params(p, torch.device('cpu'))
    with pytest.raises(AssertionError):
        K.upload_aug_params(K.aug_params(2), torch.device('cpu'), n=3)
    q = K.set_aug_image(K.aug_params(1)[0], hue=-0.3, sigma=1.0, flip=True)
    assert (q.hue_shift, q.radius, q.flip) == (int(-0.3 * 255) & 255, 4, 1) and q.w[0] > q.w[4] > 0 and q.w[5] == 0.0
    assert K.set_aug_image(q, hue=0.5).hue_shift == 127 and K.set_aug_image(q, hue=-0.5).hue_shift == 129 and K.set_aug_image(q, hue=-0.004).hue_shift == 255


def _fields(arr):
    return [(list(p.order), p.enabled, p.flip, p.hue_shift, p.brightness, p.contrast, p.saturation, p.radius, list(p.w)) for p in arr]


def test_sampler_is_deterministic_per_seed_and_independent_of_the_split():
    a = _fields(input_edge.PhotometricAugment(seed=3).sample(24))
    assert a == _fields(input_edge.PhotometricAugment(seed=3).sample(24))
    assert a != _fields(input_edge.PhotometricAugment(seed=4).sample(24))
    s = input_edge.PhotometricAugment(seed=3)
    parts = _fields(s.sample(5)) + _fields(s.sample(1)) + _fields(s.sample(16)) + _fields(s.sample(2))
    assert parts == a
    hard = [i % 3 == 0 for i in range(24)]
    s = input_edge.PhotometricAugment(seed=3)
    assert _fields(input_edge.PhotometricAugment(seed=3).sample(24, hard)) == _fields(s.sample(7, hard[:7])) + _fields(s.sample(17, hard[7:]))


def test_sampler_keeps_the_distributions_of_the_host_pipeline():
    N = 10000
    A = input_edge.PhotometricAugment(seed=11)
    hard = [i % 4 == 0 for i in range(N)]
    arr = A.sample(N, hard)
    d = A.last
    f32 = np.float32
    orders = set()
    applied_soft = 0
    for i, p in enumerate(arr):
        lo, hi, hh = (0.2, 1.8, 0.3) if hard[i] else (0.6, 1.4, 0.1)
        assert sorted(p.order) == [0, 1, 2, 3]
        orders.add(tuple(p.order))
        for v, raw in zip((p.brightness, p.contrast, p.saturation), d['factors'][i]):
            assert lo - 1e-12 <= raw <= hi + 1e-12 and f32(lo) <= f32(v) <= f32(hi) and f32(v) == f32(raw)
        assert -hh <= d['hue'][i] <= hh and p.hue_shift == int(d['hue'][i] * 255) & 255
        assert 0.15 <= d['sigma'][i] < 1.30 and p.radius == int(4.0 * d['sigma'][i] + 0.5) and 1 <= p.radius <= 5
        assert abs(sum(p.w[1:]) * 2 + p.w[0] - 1.0) < 1e-15
        assert p.enabled in (0, 15) and (p.enabled == 15) == d['applied'][i] and p.flip == d['flip'][i]
        if hard[i]:
            assert p.enabled == 15                                         # the meta-test domains always get the jitter
        else:
            applied_soft += p.enabled == 15
    n_soft = N - sum(hard)
    assert abs(applied_soft / n_soft - 0.5) <= 0.02                       # RandomApply(p = 0.5); sd of the fraction over 7 500 draws: 0.0058
    assert abs(sum(p.flip for p in arr) / N - 0.5) <= 0.02
    assert len(orders) == 24
    fac = np.array(d['factors'])[~np.array(hard)]
    assert fac.min() < 0.61 and fac.max() > 1.39 and abs(fac.mean() - 1.0) < 0.01      # the whole range is used
    sig = np.array(d['sigma'])
    assert sig.min() < 0.16 and sig.max() > 1.29
    # zero strengths are torchvision's None (the op does not run); no blur / no flip when switched off
    q = input_edge.PhotometricAugment(brightness=0.0, hue=0.0, p=1.0, blur=False, flip=False, seed=1).sample(50)
    assert all(p.enabled == (1 << K.AUG_CONTRAST | 1 << K.AUG_SATURATION) and p.radius == 0 and p.flip == 0 for p in q)
    assert all(p.enabled == 0 for p in input_edge.PhotometricAugment(p=0.0, seed=1).sample(50))


def test_fixture_is_what_pil_and_scipy_compute():
    pytest.importorskip('PIL')
    pytest.importorskip('scipy')
    tool = _tool()
    arrays = tool.generate()
    assert os.path.getsize(tool.FIXTURE) < 300 * 1024
    with np.load(tool.FIXTURE, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(arrays)
        for k, v in arrays.items():
            assert f[k].dtype == v.dtype and np.array_equal(f[k], v), k
    # the cases cover what they are there for
    c = tool.cases()
    assert [c[k]['img'].shape[:3] for k in 'abcd'] == [(1, 7, 9), (3, 37, 53), (2, 70, 150), (1, 67, 93)]
    used = [(c[k]['factors'][i], c[k]['hue'][i], c[k]['sigma'][i]) for k in c for i in range(len(c[k]['hue'])) if c[k]['enabled'][i]]
    assert {float(v) for u in used for v in u[0]} == set(tool.FACTORS) and {float(u[1]) for u in used} == set(tool.HUES)
    assert {float(s) for k in c for s in c[k]['sigma']} - {0.0} == set(tool.SIGMAS)
    assert list(c['d']['order'][0]).index(tool.CONTRAST) == 2 and list(c['b']['order'][2]) == [tool.HUE, tool.CONTRAST, tool.BRIGHTNESS, tool.SATURATION]


def test_plain_edge_does_not_go_near_the_augmenting_bindings(monkeypatch):
    """augment=None is the default of both entry points and takes exactly the old calls: the new bindings are replaced by bombs, the old ones by recorders."""
    assert inspect.signature(harness.prepare_batch_u8).parameters['augment'].default is None
    assert inspect.signature(harness.prepare_batch_u8).parameters['hard'].default is None
    sig = inspect.signature(input_edge.DevicePrefetcher.__init__).parameters
    assert sig['augment'].default is None and sig['hard_domains'].default is None and list(sig)[:4] == ['self', 'source', 'depth', 'device']

    def bomb(*a, **k):
        raise AssertionError('the plain edge called an augmenting binding')
    calls = []
    monkeypatch.setattr(K, 'augment_u8', bomb)
    monkeypatch.setattr(K, 'upload_aug_params', bomb)
    monkeypatch.setattr(K, 'aug_params', bomb)
    monkeypatch.setattr(K, 'image_u8_to_nhwc4', lambda img: calls.append(('img', tuple(img.shape))) or torch.zeros(img.shape[:3] + (4,)))
    monkeypatch.setattr(K, 'labels_u8_to_i64', lambda lab: calls.append(('lab', tuple(lab.shape))) or lab.long())      # one positional argument, as before
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    img, lab = torch.zeros((2, 3, 4, 6, 3), dtype=torch.uint8), torch.full((2, 3, 4, 6), 255, dtype=torch.uint8)
    x, gt = harness.prepare_batch_u8(img, lab)
    assert calls == [('img', (6, 4, 6, 3)), ('lab', (6, 4, 6))] and tuple(x.shape) == (6, 4, 4, 6) and gt.dtype == torch.int64 and int(gt.min()) == 255
    assert input_edge.hard_flags((2, 3, 4, 6), {1}) == [False, True, False] * 2 and input_edge.hard_flags((2, 3, 4, 6), None) is None
