"""Every output bit of the memory entry points (csrc/memory.hip) and the answers of their workspace queries against tests/golden/memory_bits.json: recorded by
tools/record_memory_bits.py from the commit BEFORE the 32-row tile of the MFMA read kernels became one set of parts and the LDS-slab accumulation kernel, which no
call could reach, was removed. The inputs are built by the recorder's own functions; the outputs are fixed-order and deterministic, so the digests have to be equal.
The one answer that changed on purpose is pm_mem_write_accum_workspace below 16 321 rows: it was sized by the removed kernel's block count there."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_memory_bits', os.path.join(ROOT, 'tools', 'record_memory_bits.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.FIXTURE) as f:
        return tool, json.load(f)


TOOL, FIXTURE = _tool()
RUNS = [(TOOL.run_read, r) for r in TOOL.READ_RUNS] + [(TOOL.run_write, r) for r in TOOL.WRITE_RUNS]


@pytest.fixture(scope='module')
def K():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def test_the_recorded_cases_are_complete():
    """Every run of every case is recorded with every call and every output: 20 read runs (slots 7 x 2, views 2 x 2, tile-loop 2) and 7 write runs."""
    assert len(TOOL.READ_RUNS) == 20 and len(TOOL.WRITE_RUNS) == 7
    assert [(c[0], c[1]) for c in TOOL.READ_CASES] == [('slots', (2, 9, 7, 256)), ('views', (2, 9, 7, 256)), ('tile-loop', (1, 8, 12293, 256))]
    assert [(c[0], c[1], c[2]) for c in TOOL.WRITE_CASES] == [('write-small', (1, 9, 7, 256), (1, 30, 20)), ('write-chunks', (2, 129, 128, 256), (2, 516, 512))]
    assert sorted(FIXTURE['digests']) == sorted(TOOL.run_id(*r) for _, r in RUNS)
    read = {'mem_read_fwd': ['p_mem', 'qr', 'score'], 'mem_read_fwd_pq': ['p_mem', 'p_query', 'qr', 'score'], 'mem_colsoftmax': ['p_query'],
            'mem_read_bwd[dmem=0,dsx=0]': ['dx'], 'mem_read_bwd[dmem=0,dsx=1]': ['dx'], 'mem_read_bwd[dmem=1,dsx=0]': ['dmem', 'dx'],
            'mem_read_bwd[dmem=1,dsx=1]': ['dmem', 'dx']}
    write = {'mem_write_accum': ['nomden'], 'mem_write_accum_bwd': ['dz'], 'mem_write_update': ['mem', 'u'], 'mem_write_update_bwd': ['dnom'],
             'mem_write_update_bwd[dmem_in]': ['dmem_in', 'dnom']}
    for fn, r in RUNS:
        calls = FIXTURE['digests'][TOOL.run_id(*r)]
        assert {call: sorted(outs) for call, outs in calls.items()} == (read if fn is TOOL.run_read else write), TOOL.run_id(*r)
        assert all(len(d) == 64 for outs in calls.values() for d in outs.values())


def test_memory_workspace_answers():
    """Pure host code, no GPU. The three read queries answer what the recorded table holds for every case and the flagship. pm_mem_write_accum_workspace answers for
    the kernel that runs, align256(min(ceil(rows / 64), 512) * (m + 1) * 257 * 4): the recorded answer above 16 320 rows (tile-loop, write-chunks, the flagship),
    no more than the recorded one below."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    shapes = TOOL.workspace_shapes()
    assert sorted(FIXTURE['workspaces']) == sorted(name for name, _, _ in shapes)
    assert shapes[-1] == ('flagship', (8, 48, 48, 256), (19,))
    large = []
    for name, (n, h, w, c), ms in shapes:
        rows = n * h * w
        assert sorted(FIXTURE['workspaces'][name]) == sorted(str(m) for m in ms), name
        for m in ms:
            got, want = TOOL.workspaces(lib, (n, h, w, c), m), FIXTURE['workspaces'][name][str(m)]
            assert got[:3] == want[:3] and all(v > 0 and v % 256 == 0 for v in got), (name, m, got, want)
            formula = (min((rows + 63) // 64, 512) * (m + 1) * 257 * 4 + 255) // 256 * 256
            assert got[3] == formula <= want[3], (name, m, got, want)
            if rows > 16320:
                large.append(name)
                assert got[3] == want[3], (name, m, got, want)
    assert sorted(set(large)) == ['flagship', 'tile-loop', 'write-chunks']


@pytest.mark.gpu
@pytest.mark.parametrize('fn,run', RUNS, ids=[TOOL.run_id(*r) for _, r in RUNS])
def test_memory_bits(K, fn, run):
    got, want = fn(K, *run), FIXTURE['digests'][TOOL.run_id(*run)]
    assert sorted(got) == sorted(want)
    diff = {'%s.%s' % (call, o): (got[call][o], want[call][o]) for call in want for o in want[call] if got[call].get(o) != want[call][o]}
    assert not diff, diff
