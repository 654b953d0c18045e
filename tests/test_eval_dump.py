"""GPU: the evaluation image dumps (csrc/eval_dump.hip: pm_eval_dump; K.eval_dump, harness.evaluate(on_images=...), harness.segment_folder) against the numpy
restatement of tests/eval_dump_cases.py, which tests/test_eval_dump_cpu.py holds to PIL's own bytes on the same inputs. Every comparison is exact: no tolerance, no
excluded pixel. In the raw calls every array sits in a poisoned flat buffer of tools/view_slabs.py with guard checks."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import eval_dump_cases as EC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('view_slabs', os.path.join(ROOT, 'tools', 'view_slabs.py'))
VS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VS)
DEV = 'cuda'
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)
NEEDS = dict(color=('palette',), compose=('palette', 'image'), diff=('palette', 'image', 'labels'), ids=('id_table',))
HW_IMG, CROP = (96, 160), 64      # the image and crop of the caller tests of tests/test_sliding_eval.py
CRIT = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)


@pytest.fixture(scope='module')
def env():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd import harness
    from pinthememory_amd.hip import kernels, lib
    return dict(K=kernels, L=lib, lib=lib.load(), harness=harness)


@pytest.fixture(scope='module')
def v3net(env):
    from pinthememory_amd import synth
    from pinthememory_amd.network import deepv3plus
    return synth.load_det_weights(deepv3plus.DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()


_WANT = {}


def expected(case, alpha):
    """The restatement of one case and alpha as torch tensors, computed once and never written."""
    if (case, alpha) not in _WANT:
        x = EC.inputs(*case)
        _WANT[case, alpha] = {k: torch.from_numpy(np.array(v)) for k, v in EC.restate(x['pred'], EC.PALETTE, x['image'], x['gt'], EC.id_table(), alpha).items()}
    return _WANT[case, alpha]


def run_dump(env, case, alpha, want, shift=0):
    """One raw call with no more inputs than `want` needs. shift: bytes by which pred and ids are moved off their dword (their buffers are one dword longer)."""
    x = EC.inputs(*case)
    pixels = case[0] * case[1] * case[2]
    given = dict(palette=EC.PALETTE, image=x['image'], labels=x['gt'], id_table=EC.id_table())
    bp, dp = VS.flat(pixels + 4, torch.uint8, 'in', torch.cat([torch.full((shift,), 77, dtype=torch.uint8), torch.from_numpy(np.array(x['pred'])).reshape(-1),
                                                                torch.full((4 - shift,), 77, dtype=torch.uint8)]), DEV)
    bufs, ins, out = [bp], {}, {}
    for name in sorted({n for k in want for n in NEEDS[k]}):
        t = torch.from_numpy(np.array(given[name]))
        b, d = VS.flat(t.numel(), t.dtype, 'in', t, DEV)
        bufs.append(b)
        ins[name] = d
    for k in want:
        b, d = VS.flat(pixels + 4 if k == 'ids' else pixels * 3, torch.uint8, 'out', device=DEV)
        bufs.append(b)
        out[k] = d
    p = lambda t, off=0: None if t is None else t.data_ptr() + off
    assert dp.data_ptr() % 4 == 0 and all(d.data_ptr() % 8 == 0 for d in list(ins.values()) + list(out.values()))
    before = VS.snapshot(bufs)
    code = env['lib'].pm_eval_dump(p(dp, shift), pixels, p(ins.get('palette')), p(ins.get('image')), p(ins.get('labels')), p(ins.get('id_table')), alpha,
                                   p(out.get('color')), p(out.get('compose')), p(out.get('diff')), p(out.get('ids'), shift), env['L'].stream())
    torch.cuda.synchronize()
    assert code == 0, (code, env['lib'].pm_last_error())
    VS.check(before, bufs)
    res = {}
    for k, d in out.items():
        if k == 'ids':
            full = d.cpu()
            keep = torch.ones(pixels + 4, dtype=torch.bool)
            keep[shift:shift + pixels] = False
            assert bool((full[keep] == VS.BYTE_FILL).all()), 'ids: a byte outside the shifted array was written'
            res[k] = full[shift:shift + pixels].reshape(case)
        else:
            res[k] = d.cpu().reshape(case + (3,))
    return res


# ---- raw calls -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', EC.ALPHAS, ids=ids)
@pytest.mark.parametrize('case', EC.CASES, ids=ids)
def test_outputs_equal_the_restatement(env, case, alpha):
    want = expected(case, alpha)
    got = run_dump(env, case, alpha, EC.OUTPUTS)
    for k in EC.OUTPUTS:
        assert torch.equal(got[k], want[k]), k
    for k in EC.OUTPUTS:      # each output alone, with the inputs it needs and no other
        alone = run_dump(env, case, alpha, (k,))
        assert list(alone) == [k] and torch.equal(alone[k], want[k]), k


@pytest.mark.parametrize('shift', [1, 2, 3])
@pytest.mark.parametrize('case', [(1, 1, 3), (2, 5, 7), (1, 33, 259)], ids=ids)
def test_class_map_and_id_map_off_their_dword(env, case, shift):
    """pred and ids carry no alignment rule: off a dword the call goes pixel by pixel, with the same bytes."""
    want = expected(case, 0.5)
    got = run_dump(env, case, 0.5, EC.OUTPUTS, shift=shift)
    for k in EC.OUTPUTS:
        assert torch.equal(got[k], want[k]), k


def test_two_calls_give_the_same_bytes(env):
    case = EC.CASES[-1]
    first, second = run_dump(env, case, 0.3, EC.OUTPUTS), run_dump(env, case, 0.3, EC.OUTPUTS)
    for k in EC.OUTPUTS:
        assert torch.equal(first[k], second[k]), k


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------------------------
def test_kernels_eval_dump_takes_one_image_or_a_batch(env):
    K = env['K']
    case = (2, 16, 100)
    x, want = EC.inputs(*case), expected(case, 0.5)
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    pal, table = dev(EC.PALETTE), K.trainid_table(EC.ID_TO_TRAINID).to(DEV)
    got = K.eval_dump(dev(x['pred']), palette=pal, image=dev(x['image']), labels=dev(x['gt']), id_table=table, want=EC.OUTPUTS)      # alpha: the reference's 0.5
    assert sorted(got) == sorted(EC.OUTPUTS)
    for k in EC.OUTPUTS:
        assert got[k].dtype == torch.uint8 and got[k].is_cuda and tuple(got[k].shape) == (case if k == 'ids' else case + (3,))
        assert torch.equal(got[k].cpu(), want[k]), k
    one = K.eval_dump(dev(x['pred'][1]), palette=pal, image=dev(x['image'][1]), labels=dev(x['gt'][1]), id_table=table, alpha=0.5, want=EC.OUTPUTS)
    for k in EC.OUTPUTS:
        assert tuple(one[k].shape) == (case[1:] if k == 'ids' else case[1:] + (3,)) and torch.equal(one[k].cpu(), want[k][1]), k
    default = K.eval_dump(dev(x['pred']), palette=pal)
    assert list(default) == ['color'] and torch.equal(default['color'].cpu(), want['color'])
    with pytest.raises(AssertionError):
        K.eval_dump(dev(x['pred']), palette=pal, want=('compose',))      # no image
    with pytest.raises(AssertionError):
        K.eval_dump(dev(x['pred']), palette=pal, want=())
    with pytest.raises(AssertionError):
        K.eval_dump(dev(x['pred']).long(), palette=pal)


# ---- the callers -----------------------------------------------------------------------------------------------------------------------------------------------------
def image_u8(seed):
    return torch.randint(0, 256, (*HW_IMG, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def image_labels(seed):
    from pinthememory_amd import synth
    return synth.make_batch(1, HW_IMG, seed=seed)[1][0]


def restated(pred, img, gt, alpha=0.5):
    r = EC.restate(pred.cpu().numpy(), EC.PALETTE, img.reshape(*HW_IMG, 3).numpy(), None if gt is None else gt.reshape(HW_IMG).numpy(), EC.id_table(), alpha)
    return {k: torch.from_numpy(np.array(v)) for k, v in r.items()}


def test_evaluate_hands_the_four_images_to_the_callback(env, v3net):
    K, harness, net = env['K'], env['harness'], v3net
    palette = torch.from_numpy(EC.PALETTE)
    loader = [(image_u8(31)[None], image_labels(41)[None], ['a']), (image_u8(32), image_labels(42), ['b'])]
    seen = []
    res = harness.evaluate(net, loader, crop=CROP, dump=1, on_images=lambda i, data, images: seen.append((i, data, images)), palette=palette,
                           id_to_trainid=EC.ID_TO_TRAINID)
    plain = harness.evaluate(net, loader, crop=CROP, dump=1)
    assert torch.equal(res['hist'], plain['hist']) and all(res[k] == plain[k] for k in ('acc', 'acc_cls', 'mean_iu', 'fwavacc'))
    assert len(res['predictions']) == 1 and torch.equal(res['predictions'][0], plain['predictions'][0])
    assert net.eval_logits_lowres is False
    assert [s[0] for s in seen] == [0, 1] and all(s[1] is item for s, item in zip(seen, loader))
    table = K.trainid_table(EC.ID_TO_TRAINID).to(DEV)
    for (_, _, images), (img, gt, _) in zip(seen, loader):
        pred = harness.evaluate_sliding(net, img.reshape(*HW_IMG, 3), gt.reshape(HW_IMG), crop=CROP)['pred']
        want = K.eval_dump(pred, palette=palette.to(DEV), image=img.reshape(*HW_IMG, 3).to(DEV), labels=gt.reshape(HW_IMG).to(DEV), id_table=table, alpha=0.5,
                           want=EC.OUTPUTS)
        host = restated(pred, img, gt)
        assert sorted(images) == sorted(EC.OUTPUTS)
        for k in EC.OUTPUTS:
            assert images[k].is_cuda and torch.equal(images[k], want[k]) and torch.equal(images[k].cpu(), host[k]), k
        assert bool((host['diff'] != 255).any()) and bool((host['diff'] == 255).all(-1).any())      # both branches of the diff rule occur
    # without the dict there is no id image; alpha and device_tiles pass through
    seen = []
    harness.evaluate(net, loader[1:], crop=CROP, on_images=lambda i, data, images: seen.append(images), palette=palette, alpha=0.3, device_tiles=True)
    pred = harness.evaluate_sliding(net, loader[1][0], loader[1][1], crop=CROP)['pred']
    host = restated(pred, loader[1][0], loader[1][1], 0.3)
    assert len(seen) == 1 and sorted(seen[0]) == ['color', 'compose', 'diff']
    for k in seen[0]:
        assert torch.equal(seen[0][k].cpu(), host[k]), k
    with pytest.raises(ValueError, match='float'):      # a normalised image has no bytes to blend
        harness.evaluate(net, [(torch.zeros((3, *HW_IMG)), loader[1][1])], crop=CROP, on_images=lambda *a: None, palette=palette)
    assert net.eval_logits_lowres is False


def test_segment_folder_dumps_label_free_images(env, v3net):
    harness, net = env['harness'], v3net
    loader = [image_u8(33), (image_u8(34)[None], ['name'])]
    seen = []
    count = harness.segment_folder(net, loader, lambda i, data, images: seen.append((i, data, images)), torch.from_numpy(EC.PALETTE), id_to_trainid=EC.ID_TO_TRAINID,
                                   crop=CROP)
    assert count == 2 and [s[0] for s in seen] == [0, 1] and seen[0][1] is loader[0] and seen[1][1] is loader[1] and seen[1][1][1] == ['name']
    for (_, _, images), img in zip(seen, (loader[0], loader[1][0][0])):
        pred = harness.evaluate_sliding(net, img, crop=CROP)['pred']
        host = restated(pred, img, None)
        assert sorted(images) == ['color', 'compose', 'ids'] and 'diff' not in host
        for k in images:
            assert images[k].is_cuda and images[k].dtype == torch.uint8 and torch.equal(images[k].cpu(), host[k]), k
    assert net.eval_logits_lowres is False
    seen = []
    assert harness.segment_folder(net, loader[:1], lambda i, data, images: seen.append(images), torch.from_numpy(EC.PALETTE), crop=CROP, no_flip=True) == 1
    assert sorted(seen[0]) == ['color', 'compose']
