"""The slab harness of tests/test_tensor_views.py (tools/view_slabs.py) on the CPU: stand-in "kernels" written in torch that break the view contract in the four ways
the GPU table is there to catch must each be reported, and a correct one must pass -- the harness is shown to fail without anything being provoked on a GPU. And the
header is held against the table: an exported function with a pm_tensor parameter that has neither a case nor a stated exemption fails here."""
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VS = _load('view_slabs', 'tools', 'view_slabs.py')
SHAPE = (2, 3, 5, 8)
CASES = [(torch.float32, lay) for lay in ('dense', 'slice', 'odd')] + [(torch.bfloat16, lay) for lay in ('dense', 'slice')]


def _setup(dtype, layout):
    g = torch.Generator().manual_seed(1)
    a, b = (torch.randn(SHAPE, generator=g).to(dtype) for _ in range(2))
    (ba, va), (bb, vb), (by, vy) = VS.slab(SHAPE, dtype, layout, 'in', a), VS.slab(SHAPE, dtype, layout, 'in', b), VS.slab(SHAPE, dtype, layout, 'out')
    return [ba, bb, by], va, vb, vy


def _rows(buf):
    """the slab as [rows][pitch] from the first guard row on, and the row index of the view's first pixel"""
    pitch = buf.pitch
    off = VS.geometry(SHAPE[3], buf.mem.dtype, buf.layout)[0]
    usable = (buf.mem.numel() - off) // pitch * pitch
    return buf.mem[off:off + usable].view(-1, pitch), VS.GUARD_ROWS


@pytest.mark.parametrize('dtype,layout', CASES)
def test_a_correct_stand_in_passes(dtype, layout):
    bufs, va, vb, vy = _setup(dtype, layout)
    before = VS.snapshot(bufs)
    vy.copy_(va + vb)
    assert VS.problems(before, bufs) == []
    VS.check(before, bufs)
    assert torch.equal(vy, va + vb)


@pytest.mark.parametrize('dtype,layout', [c for c in CASES if c[1] != 'dense'])
def test_a_write_one_element_right_of_the_view_is_reported(dtype, layout):
    bufs, va, vb, vy = _setup(dtype, layout)
    before = VS.snapshot(bufs)
    vy.copy_(va + vb)
    rows, first = _rows(bufs[2])
    rows[first + 7, SHAPE[3]] = 1.0      # the element behind the last channel of pixel 7: a neighbour's lane
    found = VS.problems(before, bufs)
    assert len(found) == 1 and 'outside the view changed' in found[0]
    with pytest.raises(AssertionError):
        VS.check(before, bufs)


@pytest.mark.parametrize('dtype,layout', CASES)
@pytest.mark.parametrize('side', ['before', 'behind'])
def test_a_write_into_the_first_guard_row_is_reported(dtype, layout, side):
    """the row right behind the last pixel (a ragged tile that stores one row too many) and the row right before the first"""
    bufs, va, vb, vy = _setup(dtype, layout)
    before = VS.snapshot(bufs)
    vy.copy_(va + vb)
    stray = torch.as_strided(vy, (SHAPE[3],), (1,), vy.storage_offset() + (vy.numel() // SHAPE[3] if side == 'behind' else -1) * bufs[2].pitch)
    assert bool(torch.isnan(stray.float()).all())      # a guard row: still poison
    stray.copy_((va + vb)[0, 0, 0])
    found = VS.problems(before, bufs)
    assert len(found) == 1 and 'outside the view changed' in found[0]


@pytest.mark.parametrize('dtype,layout', CASES)
def test_an_interior_element_left_unwritten_is_reported(dtype, layout):
    bufs, va, vb, vy = _setup(dtype, layout)
    before = VS.snapshot(bufs)
    want = va + vb
    keep = vy[1, 2, 4, 7].clone()
    vy.copy_(want)
    vy[1, 2, 4, 7] = keep                # the last element of the last pixel never stored
    found = VS.problems(before, bufs)
    assert found == ['buffer 2 (out): 1 interior elements are not finite']


@pytest.mark.parametrize('dtype,layout', CASES)
def test_a_guard_row_folded_into_a_result_with_weight_zero_is_reported(dtype, layout):
    """rows behind the tensor masked by multiplication instead of by a branch: 0 * poison is poison"""
    bufs, va, vb, vy = _setup(dtype, layout)
    before = VS.snapshot(bufs)
    guard = torch.as_strided(va, (SHAPE[3],), (1,), va.storage_offset() + (va.numel() // SHAPE[3]) * bufs[0].pitch)      # the row behind the input's last pixel
    out = va + vb
    out[1, 2, 4] = out[1, 2, 4] + 0 * guard
    vy.copy_(out)
    found = VS.problems(before, bufs)
    assert found == ['buffer 2 (out): %d interior elements are not finite' % SHAPE[3]]


def test_a_write_into_an_input_is_reported_interior_included():
    bufs, va, vb, vy = _setup(torch.float32, 'slice')
    before = VS.snapshot(bufs)
    vy.copy_(va + vb)
    va[0, 0, 0, 0] += 1.0
    found = VS.problems(before, bufs)
    assert len(found) == 1 and found[0].startswith('buffer 0 (in)')


def test_geometry_of_the_layouts():
    """guard rows on both sides, the offsets and pitches the layouts promise, own pad lanes zero and everything else poison"""
    for dtype, layout, c, want in ((torch.float32, 'dense', 8, (0, 8, 0)), (torch.float32, 'slice', 8, (32, 72, 0)), (torch.bfloat16, 'slice', 8, (64, 136, 0)),
                                   (torch.float32, 'odd', 8, (1, 11, 0)), (torch.float32, 'ownpad', 19, (0, 20, 1)), (torch.bfloat16, 'ownpad', 48, (64, 192, 16))):
        assert VS.geometry(c, dtype, layout) == want
        shape = (1, 3, 5, c)
        buf, v = VS.slab(shape, dtype, layout, 'in', torch.ones(shape))
        off, pitch, npad = want
        assert v.stride() == (15 * pitch, 5 * pitch, pitch, 1) and v.storage_offset() == VS.GUARD_ROWS * pitch + off
        assert buf.mem.numel() - (v.storage_offset() + 14 * pitch + c) >= VS.GUARD_ROWS * pitch
        assert int(buf.inside.sum()) == 15 * c and int(buf.pad.sum()) == 15 * npad
        assert bool((buf.mem[buf.inside] == 1).all()) and bool((buf.mem[buf.pad] == 0).all()) and bool(torch.isnan(buf.mem[~(buf.inside | buf.pad)].float()).all())
        if layout == 'odd':
            assert v.data_ptr() % 16 != 0 and pitch % 4 != 0
    with pytest.raises(AssertionError):
        VS.geometry(8, torch.bfloat16, 'odd')      # the bf16 tier has no scalar form


def test_flat_margins():
    for dtype, fill in ((torch.float32, None), (torch.float64, None), (torch.int64, VS.LABEL_FILL), (torch.uint8, VS.BYTE_FILL)):
        data = torch.arange(10).to(dtype)
        buf, arr = VS.flat(10, dtype, 'in', data)
        assert buf.mem.numel() == 10 + 2 * VS.FLAT_MARGIN and torch.equal(arr, data)
        margin = torch.cat([buf.mem[:VS.FLAT_MARGIN], buf.mem[-VS.FLAT_MARGIN:]])
        assert bool(torch.isnan(margin).all()) if fill is None else bool((margin == fill).all())
    buf, arr = VS.flat(10, torch.float32, 'out')
    before = VS.snapshot([buf])
    arr.fill_(1.0)
    assert VS.problems(before, [buf]) == []
    buf.mem[VS.FLAT_MARGIN + 10] = 1.0
    assert len(VS.problems(before, [buf])) == 1
    buf, arr = VS.flat(10, torch.uint8, 'out')
    before = VS.snapshot([buf])
    buf.mem[VS.FLAT_MARGIN - 1] = 0
    assert len(VS.problems(before, [buf])) == 1


# ---- the header against the table -----------------------------------------------------------------------------------------------------------------------------------
def exported_with_tensor_args():
    """every function include/pinmem_hip.h declares with a `pm_tensor*` parameter"""
    with open(os.path.join(ROOT, 'include', 'pinmem_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    out = set()
    for m in re.finditer(r'\b(?:int|size_t)\s+(pm_\w+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S):
        if re.search(r'\bpm_tensor\s*\*', m.group(2)):
            out.add(m.group(1))
    return out


def test_every_tensor_entry_point_has_view_cases_or_a_stated_exemption():
    T = _load('test_tensor_views', 'tests', 'test_tensor_views.py')
    names = exported_with_tensor_args()
    assert 'pm_conv_fwd' in names and 'pm_add_n' in names and 'pm_bn_apply' in names and 'pm_sgd_momentum' not in names and len(names) > 50
    queries = {n for n in names if re.search(r'(_workspace|_bytes|_bytes_dgrad|_floats)$', n)}      # size queries dereference no tensor memory: exempt as a class
    assert all(reason.strip() for reason in T.EXEMPT.values())
    assert not (T.COVERED & set(T.EXEMPT)), 'covered and exempt at once: %s' % sorted(T.COVERED & set(T.EXEMPT))
    missing = names - queries - T.COVERED - set(T.EXEMPT)
    assert not missing, 'entry points with a pm_tensor argument and no view case (tests/test_tensor_views.py): %s' % sorted(missing)
    stale = (T.COVERED | set(T.EXEMPT)) - names - T.FLAT_ONLY
    assert not stale, 'listed, but not declared with a pm_tensor argument: %s' % sorted(stale)
