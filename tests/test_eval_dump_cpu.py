"""CPU: the evaluation image dumps without a GPU -- the premise of tests/test_eval_dump.py (the numpy restatement of tests/eval_dump_cases.py equals the bytes of the
reference's PIL sequence, eval.py:674-692, on every case and alpha), every refusal of pm_eval_dump in front of any device call, K.trainid_table, the ABI table and
the argument errors of harness.evaluate / harness.segment_folder that need no device."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from pinthememory_amd import harness
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import lib as L

import eval_dump_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
BUF = ctypes.create_string_buffer(1 << 16)      # host memory: nothing below may dereference it
P = (ctypes.addressof(BUF) + 15) // 16 * 16
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)


# ---- the premise: the restatement is PIL's bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', EC.ALPHAS, ids=ids)
@pytest.mark.parametrize('case', EC.CASES, ids=ids)
def test_restatement_equals_pil(case, alpha):
    """Exact with Pillow 12.2.0: colour, compose and diff on all of their bytes, the alpha plane of the reference's RGBA images constantly 255."""
    Image = pytest.importorskip('PIL.Image')
    from PIL import ImageChops, ImageOps
    x = EC.inputs(*case)
    want = EC.restate(x['pred'], EC.PALETTE, x['image'], x['gt'], EC.id_table(), alpha)
    for i in range(case[0]):
        pred, gt = x['pred'][i].astype(np.int64), x['gt'][i]                   # np.argmax's type
        colorized = Image.fromarray(pred.astype(np.uint8)).convert('P')      # colorize_mask
        colorized.putpalette(EC.PALETTE.reshape(-1).tolist())
        blend = Image.blend(Image.fromarray(x['image'][i]).convert('RGBA'), colorized.convert('RGBA'), alpha)
        diff = (pred != gt)
        diff[gt == 255] = 0
        lighter = ImageChops.lighter(blend, ImageOps.invert(Image.fromarray(diff.astype('uint8') * 255)).convert('RGBA'))
        assert np.array_equal(np.asarray(colorized.convert('RGB')), want['color'][i])
        for name, pil in (('compose', blend), ('diff', lighter)):
            rgba = np.asarray(pil)
            assert np.array_equal(rgba[..., :3], want[name][i]), name
            assert bool((rgba[..., 3] == 255).all()), name
        label_out = np.zeros_like(pred)                                        # eval.py:690-692 as written
        for label_id, train_id in EC.ID_TO_TRAINID.items():
            label_out[np.where(pred == train_id)] = label_id
        assert np.array_equal(label_out, want['ids'][i])


def test_inputs_hold_what_the_cases_are_for():
    assert sorted(n * h * w % 4 for n, h, w in EC.CASES) == [0, 0, 1, 2, 3, 3] and max(n * h * w for n, h, w in EC.CASES) > 4 * 256
    x = EC.inputs(1, 33, 259)
    pred, gt = x['pred'], x['gt']
    assert int(pred.max()) == 255 and 0.01 < float((pred > 18).mean()) < 0.08
    assert 0.15 < float((gt == 255).mean()) < 0.25 and bool((gt == -1).any()) and bool((gt == 40).any()) and 0.3 < float((gt == pred).mean()) < 0.6
    assert bool((EC.PALETTE[19:] == 0).all()) and EC.PALETTE[18].tolist() == [119, 11, 32]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
def dump_args(**over):
    a = dict(pred=P, pixels=70, palette=P + 1024, image=P + 2048, labels=P + 4096, id_table=P + 8192, alpha=0.5, color=P + 12288, compose=P + 16384, diff=P + 20480,
             ids=P + 24576, stream=None)
    a.update(over)
    return list(a.values())


NONE = dict(color=None, compose=None, diff=None, ids=None)
REFUSALS = [
    ('null pred', dict(pred=None)), ('pixels = 0', dict(pixels=0)), ('pixels < 0', dict(pixels=-3)), ('no output', NONE),
    ('color without palette', dict(NONE, color=P + 12288, palette=None)), ('compose without palette', dict(NONE, compose=P + 16384, palette=None)),
    ('diff without palette', dict(NONE, diff=P + 20480, palette=None)), ('compose without image', dict(NONE, compose=P + 16384, image=None)),
    ('diff without image', dict(NONE, diff=P + 20480, image=None)), ('diff without labels', dict(labels=None)), ('ids without id_table', dict(id_table=None)),
    ('alpha nan', dict(alpha=float('nan'))), ('alpha inf', dict(alpha=float('inf'))), ('alpha -inf', dict(alpha=float('-inf'))),
    ('image off 4 bytes', dict(image=P + 2049)), ('image off 4 bytes by 2', dict(image=P + 2050)), ('color off 4 bytes', dict(color=P + 12289)),
    ('compose off 4 bytes', dict(compose=P + 16386)), ('diff off 4 bytes', dict(diff=P + 20483)), ('labels off 8 bytes', dict(labels=P + 4100)),
]


@pytest.mark.parametrize('what,over', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_eval_dump_refusals(what, over):
    lib = L.load()
    code = lib.pm_eval_dump(*dump_args(**over))
    msg = lib.pm_last_error()
    assert code == EINVAL, (what, code, msg)
    assert b'eval_dump' in msg


def test_symbol_table_header_and_abi_number():
    lib = L.load()
    assert 'pm_eval_dump' in L.SIGNATURES and hasattr(lib, 'pm_eval_dump')
    assert L.ABI_VERSION == 460 and lib.pm_version() == 460
    hdr = open(os.path.join(ROOT, 'include', 'pinmem_hip.h')).read()
    sect = hdr[hdr.index('/* ---- evaluation image dumps'):hdr.index('/* ---- ablation sweep')]
    assert 'int pm_eval_dump(' in sect and 'pm_tensor' not in sect
    assert 'pm_eval_dump' in hdr[hdr.index('460:'):hdr.index('#define PM_ABI_VERSION')]


# ---- the label-id table ----------------------------------------------------------------------------------------------------------------------------------------------
def test_trainid_table():
    t = K.trainid_table(EC.ID_TO_TRAINID)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256,) and not t.is_cuda
    assert np.array_equal(t.numpy(), EC.id_table())
    assert int(t[255]) == 30 and int(t[13]) == 34 and int(t[0]) == 35 and int(t[1]) == 8      # the last id of a shared train id wins
    assert bool((t[19:255] == 0).all())                                                       # no entry names the value
    assert K.trainid_table({5: 1, 6: 1, 4: 1}).tolist()[:3] == [0, 4, 0]                      # the dict's order, not the ids'
    assert int(K.trainid_table({7: -1, 9: 256, 300: 1000, 3: 2}).sum()) == 3                  # train ids outside 0 .. 255 are skipped, whatever their label id
    assert int(K.trainid_table({}).sum()) == 0
    for bad in ({256: 3}, {-1: 0}, {1: 2, 1000: 255}):
        with pytest.raises(ValueError):
            K.trainid_table(bad)


# ---- harness arguments that need no device ---------------------------------------------------------------------------------------------------------------------------
def test_harness_arguments():
    sig = inspect.signature(harness.evaluate).parameters
    assert [sig[k].default for k in ('on_images', 'palette', 'id_to_trainid', 'alpha')] == [None, None, None, 0.5]
    assert [sig[k].default for k in ('crop', 'scales', 'no_flip', 'classes', 'dump', 'device_tiles')] == [768, (1.0,), False, 19, 0, False]      # as before
    seg = inspect.signature(harness.segment_folder).parameters
    assert list(seg)[:4] == ['net', 'loader', 'on_images', 'palette'] and all(seg[k].default is inspect.Parameter.empty for k in list(seg)[:4])
    assert {k: seg[k].default for k in list(seg)[4:]} == dict(id_to_trainid=None, crop=768, scales=(1.0,), overlap=1.0 / 3, no_flip=False, alpha=0.5, device_tiles=False)
    seen = lambda *a: None
    with pytest.raises(ValueError, match='palette'):
        harness.evaluate(None, [], on_images=seen)
    with pytest.raises(ValueError, match='palette'):
        harness.segment_folder(None, [], seen, None)
    for bad in (torch.zeros((19, 3), dtype=torch.uint8), torch.zeros((256, 3), dtype=torch.float32)):
        with pytest.raises(ValueError, match='palette'):
            harness.evaluate(None, [], on_images=seen, palette=bad)
        with pytest.raises(ValueError, match='palette'):
            harness.segment_folder(None, [], seen, bad)
    with pytest.raises(ValueError):
        harness.evaluate(None, [], on_images=seen, palette=torch.from_numpy(EC.PALETTE), id_to_trainid={256: 3})
