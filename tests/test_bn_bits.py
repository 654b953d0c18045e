"""Every output bit of the BatchNorm entry points (csrc/bn.hip, fp32 and bf16), every answer of pm_bn_workspace and the Python paths built on them (hip/ops.py)
against tests/golden/bn_bits.json: recorded by tools/record_bn_bits.py from the commit BEFORE the two tiers' BatchNorm kernels became one body and the statistics /
backward paths of ops.py one implementation each. The inputs are built by the recorder's own functions; the outputs are fixed-order and deterministic, so the digests
have to be equal."""
import ctypes
import importlib.util
import json
import os
import socket
from ctypes import byref

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_bn_bits', os.path.join(ROOT, 'tools', 'record_bn_bits.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.FIXTURE) as f:
        return tool, json.load(f)


TOOL, FIXTURE = _tool()
RUNS = [(c, dt) for c in TOOL.CASES for dt in TOOL.DTYPES]


@pytest.fixture(scope='module')
def K():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def _same(got, want):
    assert sorted(got) == sorted(want)
    diff = {call: (got[call], want[call]) for call in want if got[call] != want[call]}
    assert not diff, diff


def test_bn_workspace_answers_what_the_recorded_table_holds():
    """pm_bn_workspace for the seven cases and four shapes of the workload, as fp32 and as bf16: pure host code, no GPU."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    assert sorted(FIXTURE['workspaces']) == sorted(c[0] for c in TOOL.CASES + TOOL.SIZE_ONLY)
    for case in TOOL.CASES + TOOL.SIZE_ONLY:
        assert TOOL.workspaces(lib, L, case) == FIXTURE['workspaces'][case[0]], case


def test_the_recorded_cases_reach_the_kernels():
    """Every case is recorded for both element types; a call family is refused for the single pixel and at most one case besides; bn_stats_finalize of one pixel is."""
    want = ['%s/%s' % (c[0], dt) for c, dt in RUNS] + [c[0] for c in TOOL.STEM_CASES] + [TOOL.SLAB_CASE[0]]
    assert sorted(FIXTURE['digests']) == sorted(want) and len(TOOL.CASES) == 7
    TOOL.check_reach(FIXTURE['digests'])
    for dt in TOOL.DTYPES:
        assert FIXTURE['digests']['one-pixel/' + dt]['bn_stats_finalize'] == 'refused'
    assert sorted(FIXTURE['paths']) == ['forced', 'plain']


def test_the_apply_passes_refuse_a_misaligned_sums_before_any_launch():
    """`sums` at base + 4 bytes -> PM_EINVAL from pm_bn_bwd_apply, _mask and _pool, for both element types; base itself passes the check and is refused later or
    not at all. The descriptors are valid fakes and nothing is dereferenced: the refusal comes before any launch, so this runs without a GPU."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    einval = -1      # include/pinmem_hip.h: PM_EINVAL
    base, p = 0x100000, ctypes.c_void_p

    def t(addr, h, w, c, dt):
        return L.PmTensor(addr, 2, h, w, c, c, dt, 0)
    for dt in (L.PM_F32, L.PM_BF16):
        x, dy, dx = t(base, 6, 6, 16, dt), t(base + 0x10000, 6, 6, 16, dt), t(base + 0x20000, 6, 6, 16, dt)
        par = [p(base + 0x30000 + 0x100 * i) for i in range(4)]
        code = lib.pm_bn_bwd_apply(byref(dy), None, byref(x), par[0], par[1], par[2], par[3], p(base + 0x40004), 72.0, 2, byref(dx), None, None)
        assert code == einval and b'16-byte aligned' in lib.pm_last_error(), (dt, code, lib.pm_last_error())
    x, dy, dx, dyp = t(base, 6, 6, 16, L.PM_F32), t(base + 0x10000, 6, 6, 16, L.PM_F32), t(base + 0x20000, 6, 6, 16, L.PM_F32), t(base + 0x50000, 3, 3, 16, L.PM_F32)
    code = lib.pm_bn_bwd_apply_mask(byref(dy), p(base + 0x60000), byref(x), par[0], par[1], par[2], p(base + 0x40004), 72.0, byref(dx), None)
    assert code == einval and b'16-byte aligned' in lib.pm_last_error(), (code, lib.pm_last_error())
    code = lib.pm_bn_bwd_apply_pool(byref(dyp), p(base + 0x60000), byref(x), par[0], par[1], par[2], par[3], p(base + 0x40004), 72.0, byref(dx), None)
    assert code == einval and b'16-byte aligned' in lib.pm_last_error(), (code, lib.pm_last_error())


@pytest.mark.gpu
@pytest.mark.parametrize('case,dt', RUNS, ids=['%s/%s' % (c[0], dt) for c, dt in RUNS])
def test_bn_bits(K, case, dt):
    _same(TOOL.run_case(K, case, dt), FIXTURE['digests']['%s/%s' % (case[0], dt)])


@pytest.mark.gpu
@pytest.mark.parametrize('case', TOOL.STEM_CASES, ids=[c[0] for c in TOOL.STEM_CASES])
def test_bn_stem_pair_bits(K, case):
    _same(TOOL.run_stem(K, case), FIXTURE['digests'][case[0]])


@pytest.mark.gpu
def test_bn_slab_partials_bits(K):
    _same(TOOL.run_slabs(K, TOOL.SLAB_CASE), FIXTURE['digests'][TOOL.SLAB_CASE[0]])


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['plain', 'forced'])
def test_bn_python_paths_bits(K, mode):
    """One forward + backward of the smallest model on both tiers (loss, every parameter gradient, every running moment, the collectives issued), of a bottleneck with
    a downsample branch and of conv_bn_act_n over three branches, in a fresh child process: the digests the parent commit's package and library gave. `forced`
    (PM_DIST_FORCE=1) sends a one-rank group through the merged exchanges; that the run ends says every `sums` the apply passes received was 16-byte aligned -- the
    library refuses any other (test_the_apply_passes_refuse_a_misaligned_sums_before_any_launch)."""
    _same(TOOL.run_paths(ROOT, mode, port=_free_port()), FIXTURE['paths'][mode])
