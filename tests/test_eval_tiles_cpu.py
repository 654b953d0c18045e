"""CPU: the host side of the evaluation input edge -- the whole-axis coefficient tables of pm_resize_axis_tables against PIL's Image.resize(BILINEAR) (through
tests/golden/eval_scale_cases.npz, written by tools/make_eval_scale_golden.py from PIL alone), against pm_resample_tables for the bicubic filter, the tap cap, the
argument validation of pm_eval_tiles_u8 in front of any device call, the tile plan, and the default path of evaluate_sliding. No GPU here."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from pinthememory_amd import harness
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import lib as L

from test_resample_cpu import filter_axis, geo_image, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC, PREC = L.RESAMPLE_REC, 22
# (source H, W) -> scales: what the fixture holds
WANT = {(52, 97): (0.25, 0.5, 0.613, 0.75, 1.0, 1.31, 2.0), (64, 128): (0.5,), (97, 161): (0.613, 1.31), 'ramp': (0.77, 1.999), (20, 37): (0.25, 4.0)}


def _tool():
    spec = importlib.util.spec_from_file_location('make_eval_scale_golden', os.path.join(ROOT, 'tools', 'make_eval_scale_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def fixture_cases(fx):
    """[(source image, scale, PIL's scaled image)] of the fixture."""
    n = sum(k.endswith('_img') for k in fx)
    return [(fx['src%d' % int(fx['case%d_src' % i])], float(fx['case%d_scale' % i]), fx['case%d_img' % i]) for i in range(n)]


def axis_table(n_in, n_out, filt=L.FILTER_BILINEAR):
    return np.ctypeslib.as_array(K.resize_axis_tables(n_in, n_out, filt)).copy().reshape(n_out, REC)


def scaled_by_tables(img, hs, ws):
    """The kernel's arithmetic in numpy (filter_axis of test_resample_cpu.py): along W into bytes, then along H."""
    mid = filter_axis(img.transpose(1, 0, 2), axis_table(img.shape[1], ws)).transpose(1, 0, 2)
    return filter_axis(mid, axis_table(img.shape[0], hs))


def test_fixture_is_what_pil_computes_and_holds_the_cases():
    pytest.importorskip('PIL')
    tool = _tool()
    arrays = tool.generate()
    assert os.path.getsize(tool.FIXTURE) < 512 * 1024
    with np.load(tool.FIXTURE, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(arrays)
        for k, v in arrays.items():
            assert f[k].dtype == v.dtype and np.array_equal(f[k], v), k


def test_fixture_holds_the_cases(golden):
    with golden('eval_scale_cases.npz') as f:
        fx = {k: f[k] for k in f.files}
    tool = _tool()
    assert tool.SIZES == ((52, 97), (64, 128), (97, 161), (64, 128), (20, 37)) and tool.RAMP == 3
    got = {}
    for k, s in tool.cases():
        got.setdefault('ramp' if k == tool.RAMP else tool.SIZES[k], []).append(s)
    assert {k: tuple(v) for k, v in got.items()} == WANT
    cases = fixture_cases(fx)
    assert len(cases) == len(tool.cases()) == 14
    for (k, s), (src, scale, img) in zip(tool.cases(), cases):
        assert src.shape == tool.SIZES[k] + (3,) and scale == s and img.shape == (int(src.shape[0] * s), int(src.shape[1] * s), 3) and img.dtype == np.uint8
    y, x = np.mgrid[0:64, 0:128]
    assert np.array_equal(fx['src3'][..., 0], (x * 255) // 127) and np.array_equal(fx['src3'][..., 1], (y * 255) // 63)      # the ramp of the resample fixture
    assert all((w * 3) % 4 for w in (97, 161, 37)) and {img.shape[1] % 2 for _, _, img in cases} == {0, 1}      # source rows off the dword grid, odd scaled widths


def test_bilinear_tables_reproduce_every_case_with_no_differing_byte(golden):
    """pm_resize_axis_tables(BILINEAR) for both axes, applied in numpy with the integer rule of the header: 0 bytes off PIL. Derived, not measured: integer arithmetic."""
    with golden('eval_scale_cases.npz') as f:
        fx = {k: f[k] for k in f.files}
    most = 0
    for src, scale, want in fixture_cases(fx):
        hs, ws = want.shape[:2]
        got = scaled_by_tables(src, hs, ws)
        most = max(most, int(axis_table(src.shape[0], hs)[:, 1].max()), int(axis_table(src.shape[1], ws)[:, 1].max()))
        bad = int((got != want).sum())
        print('%d x %d at %.4f -> %d x %d: %d of %d bytes differ from PIL' % (src.shape[0], src.shape[1], scale, hs, ws, bad, want.size))
        assert bad == 0
        if scale == 1.0:                                                                       # PIL skips both passes: one tap of 2^22, a copy
            t = axis_table(src.shape[0], hs)
            assert np.array_equal(t[:, 0], np.arange(hs)) and (t[:, 1] == 1).all() and (t[:, 2] == 1 << PREC).all() and not t[:, 3:].any() and np.array_equal(got, src)
    assert most <= 9


def test_bicubic_tables_are_the_unpadded_records_of_pm_resample_tables(golden):
    with golden('resample_cases.npz') as f:
        scales = sorted({float(s) for k in f.files if k.endswith('_scale') for s in f[k]})
    assert len(scales) >= 7
    for size in (52, 97, 128, 161):
        for s in scales:
            out = int(size * s)
            br, bc, _, _ = tables(geo_image(size, size, out, out, 0, 0, 0, 0), (size, size), (out, out))
            got = axis_table(size, out, L.FILTER_BICUBIC)
            assert np.array_equal(got, br) and np.array_equal(got, bc), (size, s)
    # a window of the padded image holds the same records at its un-padded positions
    br, _, _, _ = tables(geo_image(64, 128, 32, 64, 4, 0, 2, 0), (64, 128), (36, 33))
    assert not br[:2].any() and np.array_equal(br[2:34], axis_table(64, 32, L.FILTER_BICUBIC)) and not br[34:].any()


def test_tap_cap_serves_every_scale_from_a_quarter_to_four():
    lib = L.load()
    assert (L.FILTER_BILINEAR, L.FILTER_BICUBIC) == (2, 3) and L.ABI_VERSION >= 450
    most = 0
    for size in range(1, 301):
        outs = {int(size * s) for s in (0.25, 0.2501, 0.26, 0.3333, 0.5, 0.75, 1.0, 1.5, 3.999, 4.0)} | {-(-size // 4), size * 4}      # in / out in [0.25, 4] at both ends
        for out in sorted(o for o in outs if o >= 1 and 0.25 <= size / o <= 4.0):
            t = axis_table(size, out)
            most = max(most, int(t[:, 1].max()))
            assert t[:, 1].min() >= 1 and (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= size).all() and (np.diff(t[:, 0]) >= 0).all()
            assert np.abs(t[:, 2:].sum(1) - (1 << PREC)).max() <= 16 and t[:, 2:].min() >= 0                # a triangle: no negative tap, so no sum leaves int32
    assert 8 <= most <= 2 * 4 + 1 <= L.RESAMPLE_MAX_TAPS                                                    # PIL's bound: 2 * support + 1 with support = in / out
    rec = (ctypes.c_int32 * (100 * REC))()
    assert lib.pm_resize_axis_tables(1150, 100, L.FILTER_BILINEAR, rec) == 0                                # 2 * 11.5 + 1 = 24 taps
    assert lib.pm_resize_axis_tables(1300, 100, L.FILTER_BILINEAR, rec) == -4 and b'PM_RESAMPLE_MAX_TAPS' in lib.pm_last_error()      # PM_EUNSUPPORTED
    assert lib.pm_resize_axis_tables(1000, 100, L.FILTER_BICUBIC, rec) == -4
    with pytest.raises(L.PinmemError, match='taps'):
        K.resize_axis_tables(1300, 100)
    for bad in ((0, 100, 2, rec), (100, 0, 2, rec), (100, -1, 2, rec), (100, 100, 2, None), (100, 100, 0, rec), (100, 100, 4, rec)):
        assert lib.pm_resize_axis_tables(*bad) == -1 and b'resize_axis_tables' in lib.pm_last_error(), bad[:3]


def test_eval_tiles_validation_happens_before_anything_touches_a_device():
    """Fake aligned pointers, a null stream, no GPU in this container: every refusal below returns before a launch."""
    lib = L.load()
    IMG, ROWS, COLS, TILES, OUT = (0x1000000 * k for k in range(1, 6))
    m, s = (ctypes.c_float * 3)(*K.IMAGENET_MEAN), (ctypes.c_float * 3)(*K.IMAGENET_STD)
    #       0    1   2   3     4     5   6   7      8  9   10  11 12 13 14   15
    args = [IMG, 40, 60, ROWS, COLS, 20, 30, TILES, 2, 16, 16, 2, m, s, OUT, None]

    def run(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.pm_eval_tiles_u8(*a)
    for k in (0, 3, 4, 7, 12, 13, 14):
        assert run(**{'a%d' % k: None}) == -1 and b'null' in lib.pm_last_error(), k
    for k in (1, 2, 5, 6, 9, 10):
        assert run(**{'a%d' % k: 0}) == -1 and run(**{'a%d' % k: -3}) == -1 and b'empty size' in lib.pm_last_error(), k
    assert run(a8=-1) == -1
    assert run(a9=21) == -1 and run(a10=31) == -1 and b'in a scaled image' in lib.pm_last_error()           # a tile larger than the scaled image
    for flips in (0, 3, -1):
        assert run(a11=flips) == -1 and b'flips' in lib.pm_last_error()
    assert run(a14=OUT + 4) == -1 and run(a14=OUT + 8) == -1 and b'16-byte' in lib.pm_last_error()
    out_bytes = 2 * 2 * 16 * 16 * 16
    assert run(a14=IMG) == -1 and b'overlaps' in lib.pm_last_error()
    assert run(a0=OUT + out_bytes - 1) == -1 and run(a14=IMG + (40 * 60 * 3 - 1) // 16 * 16) == -1 and b'overlaps' in lib.pm_last_error()
    assert run(a3=OUT + 16) == -1 and run(a4=OUT + 32) == -1 and run(a7=OUT + 64) == -1 and b'overlaps' in lib.pm_last_error()
    assert run(a3=ROWS + 2) == -1 and b'4-byte' in lib.pm_last_error()
    assert run(a8=40000) == -4 and b'launch grid' in lib.pm_last_error()
    assert run(a2=600, a6=30) == -4 and b'staged bytes' in lib.pm_last_error()                                # 600 -> 30 columns: one row alone does not fit
    assert run(a8=0) == 0                                                                                   # no tiles: nothing launched
    assert run(a8=0, a11=3) == -1 and run(a8=0, a14=OUT + 4) == -1                                          # but checked all the same


def test_plan_tiles_are_sliding_tiles_and_the_cache_keeps_eight(monkeypatch):
    cases = [(96, 160, 0.5, 64), (96, 160, 0.5, 96), (96, 160, 1.0, 64), (96, 160, 2.0, 64), (97, 129, 0.75, 64), (52, 97, 1.31, 24), (52, 97, 0.25, 40), (1024, 2048, 0.5, 768)]
    for H, W, s, crop in cases:
        plan = K.EvalTilePlan(H, W, s, crop, 1.0 / 3, 'cpu')
        assert (plan.Hs, plan.Ws) == (int(H * s), int(W * s)) and plan.tiles == harness.sliding_tiles(plan.Hs, plan.Ws, crop, 1.0 / 3, s)
        assert all((y2 - y1, x2 - x1) == (plan.th, plan.tw) and 0 <= x1 and x2 <= plan.Ws and 0 <= y1 and y2 <= plan.Hs for x1, y1, x2, y2 in plan.tiles)
        rec = REC * 4
        assert plan.offsets == (0, plan.Hs * rec, (plan.Hs + plan.Ws) * rec) and plan.buf.numel() == plan.offsets[2] + 16 * len(plan.tiles)
        words = plan.buf.numpy().view(np.int32)
        assert np.array_equal(words[:plan.Hs * REC].reshape(-1, REC), axis_table(H, plan.Hs)) and np.array_equal(words[plan.Hs * REC:(plan.Hs + plan.Ws) * REC].reshape(-1, REC), axis_table(W, plan.Ws))
        assert words[(plan.Hs + plan.Ws) * REC:].reshape(-1, 4).tolist() == [list(t) for t in plan.tiles]
    none = K.EvalTilePlan(52, 97, 0.25, 40, 1.0 / 3, 'cpu')                         # 13 rows under a 40-tile of stride 27: eval.py:170 yields no tile
    assert none.tiles == [] and (none.th, none.tw) == (0, 0)
    # a scaled image smaller than the tile: 48 x 80 under a 64-tile is two 48 x 64 windows, under a 96-tile the whole image
    assert K.EvalTilePlan(96, 160, 0.5, 64, 1.0 / 3, 'cpu').tiles == [(0, 0, 64, 48), (16, 0, 80, 48)]
    whole = K.EvalTilePlan(96, 160, 0.5, 96, 1.0 / 3, 'cpu')
    assert whole.tiles == [(0, 0, 80, 48)] and (whole.th, whole.tw) == (48, 80)
    with pytest.raises(L.PinmemError, match='taps'):
        K.EvalTilePlan(1300, 1300, 100 / 1300 + 1e-9, 64, 1.0 / 3, 'cpu')
    with pytest.raises(ValueError):
        K.EvalTilePlan(3, 3, 0.25, 64, 1.0 / 3, 'cpu')
    monkeypatch.setattr(harness, 'sliding_tiles', lambda *a: [(0, 0, 64, 48), (32, 0, 96, 48)])              # a tile outside the scaled image never reaches the device
    with pytest.raises(ValueError, match='outside'):
        K.EvalTilePlan(96, 160, 0.5, 64, 1.0 / 3, 'cpu')
    monkeypatch.undo()
    # the cache: the same arguments give the same object and upload nothing; the ninth entry evicts the first
    K.clear_eval_tile_plans()
    before = K.EvalTilePlan.uploads
    first = K.eval_tile_plan(40, 60, 1.0, 16, 1.0 / 3, 'cpu')
    assert K.eval_tile_plan(40, 60, 1.0, 16, 1.0 / 3, 'cpu') is first and K.EvalTilePlan.uploads == before + 1
    others = [K.eval_tile_plan(40, 60 + k, 1.0, 16, 1.0 / 3, 'cpu') for k in range(1, K.EVAL_PLAN_CACHE_MAX)]
    assert K.eval_tile_plan(40, 60, 1.0, 16, 1.0 / 3, 'cpu') is first and K.EvalTilePlan.uploads == before + K.EVAL_PLAN_CACHE_MAX == before + 8
    K.eval_tile_plan(40, 60, 0.5, 16, 1.0 / 3, 'cpu')
    assert K.eval_tile_plan(40, 61, 1.0, 16, 1.0 / 3, 'cpu') is others[0] and K.EvalTilePlan.uploads == before + 9
    assert K.eval_tile_plan(40, 60, 1.0, 16, 1.0 / 3, 'cpu') is not first and K.EvalTilePlan.uploads == before + 10
    K.clear_eval_tile_plans()


class _Stop(Exception):
    pass


def test_default_path_does_not_go_near_the_new_bindings(monkeypatch):
    """device_tiles=False is the default of both entry points and takes exactly the old calls: the new bindings are replaced by bombs, the old first device call by a
    recorder that ends the run. With device_tiles=True the plan and the kernel binding are what is called, and a float image is refused."""
    for fn in (harness.evaluate_sliding, harness.evaluate):
        assert inspect.signature(fn).parameters['device_tiles'].default is False

    def bomb(*a, **k):
        raise AssertionError('the default path called a binding of the evaluation input edge')
    for name in ('eval_tiles_u8', 'eval_tile_plan', 'EvalTilePlan', 'resize_axis_tables'):
        monkeypatch.setattr(K, name, bomb)
    calls = []

    def old(img):
        calls.append(tuple(img.shape))
        raise _Stop
    monkeypatch.setattr(K, 'image_u8_to_nhwc4', old)
    net = torch.nn.Conv2d(3, 19, 1)
    net.eval_logits_lowres = False
    img = torch.zeros((48, 80, 3), dtype=torch.uint8)
    runs = [((1.0,), (1, 48, 80, 3)), ((1.0, 0.5), (1, 48, 80, 3))]
    if importlib.util.find_spec('PIL') is not None:                                 # the default path scales with PIL on the host
        runs.append(((0.5, 1.0), (1, 24, 40, 3)))
    for scales, shape in runs:
        with pytest.raises(_Stop):
            harness.evaluate_sliding(net, img, crop=32, scales=scales)
        assert calls.pop() == shape and net.eval_logits_lowres is False
    with pytest.raises(_Stop):
        harness.evaluate(net, [(img[None], torch.zeros((1, 48, 80), dtype=torch.int64))], crop=32)
    assert calls.pop() == (1, 48, 80, 3)
    # the switch: the plan is asked for, with the image's size and the scale, and nothing of the old chain runs
    seen = []

    def plan(*a):
        seen.append(a[:5])
        raise _Stop
    monkeypatch.setattr(K, 'eval_tile_plan', plan)
    with pytest.raises(_Stop):
        harness.evaluate_sliding(net, img, crop=32, scales=(0.5, 1.0), device_tiles=True)
    assert seen == [(48, 80, 0.5, 32, 1.0 / 3)] and not calls and net.eval_logits_lowres is False
    with pytest.raises(ValueError, match='device_tiles'):
        harness.evaluate_sliding(net, torch.zeros((3, 48, 80)), crop=32, device_tiles=True)
