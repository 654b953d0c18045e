"""GPU: the evaluation input edge (csrc/resample.hip, pm_eval_tiles_u8) against tests/golden/eval_scale_cases.npz, the bytes PIL's Image.resize(BILINEAR) produces
for the same images (tools/make_eval_scale_golden.py; test_eval_tiles_cpu.py regenerates them and holds the host tables to them). The crops are torch.equal to
K.image_u8_to_nhwc4 of PIL's scaled image (of its mirror) sliced per tile -- integer arithmetic up to the bytes and one shared normalisation, so the bar is
derived, not measured -- and harness.evaluate_sliding / evaluate with device_tiles=True return what the default path returns, bit for bit."""
import numpy as np
import pytest
import torch

from test_sliding_eval import CROP, HW_IMG, image_labels, image_u8
from test_validate import K, harness, v3net  # noqa: F401

pytestmark = pytest.mark.gpu

N_CASES = 14
GUARD = 64                  # floats: 256 bytes, so the guarded view stays 16-byte aligned
TILE = (32, 64)             # the kernel's piece (csrc/resample.hip TH, TW)
_REF = {}


@pytest.fixture(scope='module')
def fx(golden):
    with golden('eval_scale_cases.npz') as f:
        return {k: f[k] for k in f.files}


def case(fx, K, n):
    """(source on the device, scale, the normalised scaled image [Hs, Ws, 4] and its mirror) of fixture case n: computed once, shared, never modified."""
    if n not in _REF:
        src = torch.from_numpy(fx['src%d' % int(fx['case%d_src' % n])]).cuda()
        full = K.image_u8_to_nhwc4(torch.from_numpy(fx['case%d_img' % n]).cuda()[None].contiguous())[0]
        _REF[n] = (src, float(fx['case%d_scale' % n]), full, torch.flip(full, dims=[1]))
    return _REF[n]


def windows(harness, Hs, Ws, s):
    """The whole scaled image as one tile, then the sliding tiles of two crop sizes."""
    return [[(0, 0, Ws, Hs)]] + [harness.sliding_tiles(Hs, Ws, crop, 1.0 / 3, s) for crop in (24, 40)]


def sliced(img, tiles):
    return torch.stack([img[y1:y2, x1:x2] for x1, y1, x2, y2 in tiles])


def test_the_fixture_reaches_past_one_kernel_piece(fx):
    assert sum(k.endswith('_img') for k in fx) == N_CASES
    shapes = [fx['case%d_img' % n].shape[:2] for n in range(N_CASES)]
    assert any(h > TILE[0] and w > TILE[1] and h % TILE[0] and w % TILE[1] for h, w in shapes) and any(h < TILE[0] and w < TILE[1] for h, w in shapes)


@pytest.mark.parametrize('n', range(N_CASES))
def test_crops_are_bit_equal_to_pil_scaled_normalised_and_sliced(fx, K, harness, n):
    src, s, full, mirrored = case(fx, K, n)
    (H, W), (Hs, Ws) = src.shape[:2], full.shape[:2]
    assert (Hs, Ws) == (int(H * s), int(W * s))
    launches = 0
    for tiles in windows(harness, Hs, Ws, s):
        plan = K.EvalTilePlan(H, W, s, 0, 1.0 / 3, src.device, tiles=tiles)
        assert (plan.Hs, plan.Ws) == (Hs, Ws) and plan.tiles == tiles
        both = K.eval_tiles_u8(src, plan, 2)
        T = len(tiles)
        assert both.dtype == torch.float32 and tuple(both.shape) == (2 * T, plan.th, plan.tw, 4)
        if T == 0:                                                                  # eval.py:170 yields no tile for an axis far shorter than the tile
            continue
        launches += 1
        for name, got, want in (('image', both[:T], sliced(full, tiles)), ('mirror', both[T:], sliced(mirrored, tiles))):
            bad = int((got != want).sum())
            print('case %d (%d x %d at %.4f) %d tiles of %d x %d, %s: %d of %d floats differ' % (n, H, W, s, T, plan.th, plan.tw, name, bad, want.numel()))
            assert torch.equal(got, want)
        assert not both[..., 3].any()
        assert torch.equal(K.eval_tiles_u8(src, plan, 1), both[:T])
    assert launches >= 1


def test_scale_one_is_the_normalised_source_sliced(K, harness):
    img = torch.randint(0, 256, (70, 150, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).cuda()
    plan = K.EvalTilePlan(70, 150, 1.0, 48, 1.0 / 3, img.device)
    assert plan.tiles == harness.sliding_tiles(70, 150, 48, 1.0 / 3, 1.0) and len(plan.tiles) > 2 and (plan.th, plan.tw) == (48, 48)
    full = K.image_u8_to_nhwc4(img[None])[0]
    got = K.eval_tiles_u8(img, plan, 2)
    assert torch.equal(got[:len(plan.tiles)], sliced(full, plan.tiles)) and torch.equal(got[len(plan.tiles):], sliced(torch.flip(full, dims=[1]), plan.tiles))


def test_nothing_is_written_outside_the_output_and_nothing_read_outside_the_image(fx, K, harness):
    """The output inside a buffer with sentinel margins: the margins keep their bits. The source inside an allocation poisoned on both sides, at an odd byte
    address: the crops are those of the clean run, whatever the poison."""
    for n in (2, 5, 9, 13):
        src, s, full, mirrored = case(fx, K, n)
        (H, W), (Hs, Ws) = src.shape[:2], full.shape[:2]
        tiles = harness.sliding_tiles(Hs, Ws, 24, 1.0 / 3, s)
        plan = K.EvalTilePlan(H, W, s, 24, 1.0 / 3, src.device)
        want = torch.cat([sliced(full, tiles), sliced(mirrored, tiles)])
        buf = torch.full((want.numel() + 2 * GUARD,), -12345.0, device='cuda')
        out = buf[GUARD:GUARD + want.numel()].view(want.shape)
        assert K.eval_tiles_u8(src, plan, 2, out=out) is out and torch.equal(out, want)
        assert bool((buf[:GUARD] == -12345.0).all()) and bool((buf[-GUARD:] == -12345.0).all())
        for poison in (0x5a, 0xa5):
            slab = torch.full((H * W * 3 + 2 * 4099,), poison, dtype=torch.uint8, device='cuda')
            inside = slab[4099:4099 + H * W * 3].view(H, W, 3)
            inside.copy_(src)
            assert inside.data_ptr() % 4 and torch.equal(K.eval_tiles_u8(inside, plan, 2), want), (n, poison)


def test_a_cached_plan_serves_the_second_image_without_an_upload(fx, K):
    src, s, full, _ = case(fx, K, 5)
    H, W = src.shape[:2]
    K.clear_eval_tile_plans()
    before = K.EvalTilePlan.uploads
    plan = K.eval_tile_plan(H, W, s, 24, 1.0 / 3, src.device)
    assert K.EvalTilePlan.uploads == before + 1 and plan.buf.is_cuda and plan.buf.dtype == torch.uint8
    first = K.eval_tiles_u8(src, plan, 2)
    again = K.eval_tile_plan(H, W, s, 24, 1.0 / 3, src.device)
    second = K.eval_tiles_u8(src, again, 2)
    assert again is plan and K.EvalTilePlan.uploads == before + 1 and torch.equal(first, second)
    side = torch.cuda.Stream()                                                      # another stream waits for the copy, and eviction tells the allocator about it
    with torch.cuda.stream(side):
        third = K.eval_tiles_u8(src, plan, 2)
    side.synchronize()
    assert torch.equal(third, first) and len(plan.streams) == 2
    K.clear_eval_tile_plans()
    assert K.eval_tile_plan(H, W, s, 24, 1.0 / 3, src.device) is not plan and K.EvalTilePlan.uploads == before + 2
    torch.cuda.synchronize()


def same(a, b):
    return torch.equal(a['pred'], b['pred']) and torch.equal(a['hist'], b['hist']) and (a['logits'] is None) == (b['logits'] is None) and \
        (a['logits'] is None or torch.equal(a['logits'], b['logits']))


def test_evaluate_sliding_with_device_tiles_returns_the_default_path_bits(harness, v3net):
    net = v3net
    img, gt = image_u8(), image_labels(41)
    kw = dict(crop=CROP, scales=(0.5, 1.0, 2.0), want_logits=True)
    ref = harness.evaluate_sliding(net, img, gt, **kw)
    got = harness.evaluate_sliding(net, img, gt, device_tiles=True, **kw)
    assert got['pred'].dtype == torch.uint8 and tuple(got['pred'].shape) == HW_IMG and same(got, ref)
    assert same(harness.evaluate_sliding(net, img.cuda(), gt, device_tiles=True, **kw), ref)      # the default path refuses a device image at these scales
    assert same(harness.evaluate_sliding(net, img, gt, device_tiles=True, batch_tiles=False, **kw), harness.evaluate_sliding(net, img, gt, batch_tiles=False, **kw))
    assert net.eval_logits_lowres is False and not net.training


def test_single_scale_and_evaluate_with_device_tiles(harness, v3net):
    net = v3net
    img, gt = image_u8(), image_labels(41)
    assert same(harness.evaluate_sliding(net, img, gt, crop=CROP, scales=(1.0,), device_tiles=True), harness.evaluate_sliding(net, img, gt, crop=CROP))
    assert same(harness.evaluate_sliding(net, img, gt, crop=CROP, flips=(False,), device_tiles=True), harness.evaluate_sliding(net, img, gt, crop=CROP, flips=(False,)))
    loader = [(image_u8(31)[None], image_labels(41)[None], ['a']), (image_u8(32), image_labels(42), ['b'])]
    ref = harness.evaluate(net, loader, crop=CROP, scales=(0.75, 1.0))
    got = harness.evaluate(net, loader, crop=CROP, scales=(0.75, 1.0), device_tiles=True)
    assert torch.equal(got['hist'], ref['hist']) and got['hist'].sum().item() > 0
    assert all(got[k] == ref[k] for k in ('acc', 'acc_cls', 'mean_iu', 'fwavacc'))
    assert net.eval_logits_lowres is False
    with pytest.raises(ValueError, match='device_tiles'):
        harness.evaluate_sliding(net, torch.zeros((3, *HW_IMG), device='cuda'), gt, crop=CROP, device_tiles=True)
    assert net.eval_logits_lowres is False
