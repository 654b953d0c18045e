"""Every output bit of the pooling, resize and elementwise entry points (csrc/pool_resize.hip, csrc/misc.hip, pm_cast; fp32 and bf16), every answer of
pm_resize_bilinear_bwd_workspace and the status of every call they have to turn down, against tests/golden/pool_bits.json: recorded by tools/record_pool_bits.py from
the commit BEFORE the two tiers' kernels became one template per pass. The inputs are built by the recorder's own functions; the outputs are fixed-order and
deterministic, so the digests have to be equal."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_pool_bits', os.path.join(ROOT, 'tools', 'record_pool_bits.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.FIXTURE) as f:
        return tool, json.load(f)


TOOL, FIXTURE = _tool()


@pytest.fixture(scope='module')
def libs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import lib as L
    return L.load(), L


def test_resize_bwd_workspace_answers_what_the_recorded_table_holds():
    """pm_resize_bilinear_bwd_workspace at the small cases, the workload's shapes (8x192x192x256 -> 48x48, 8x768x768x19 -> 192x192) and ineligible pairs, as fp32, as
    bf16, for mixed types and for a misaligned pointer: pure host code, no GPU."""
    from pinthememory_amd.hip import lib as L
    got = TOOL.workspaces(L.load(), L)
    assert got == FIXTURE['workspaces']
    assert got['decoder'][:2] == [8 * 192 * 48 * 256 * 4] * 2 and got['logits'][:2] == [0, 0] and got['ratio-2-one-way'][:2] == [0, 0]
    assert all(v[2] == 0 and v[3] == 0 for v in got.values())


def test_refused_calls_return_the_recorded_status():
    """Mixed-type calls (PM_EUNSUPPORTED, or PM_EINVAL where a bf16 sum meets an fp32 operand), bf16 views that are no 16-byte vectors, a misaligned argmax, an
    ineligible or short-of-workspace separable backward: the same status as before, decided before any launch (the descriptors are empty fakes), so no GPU."""
    from pinthememory_amd.hip import lib as L
    got = TOOL.refusals(L.load(), L)
    assert got == FIXTURE['refusals']
    assert all(v < 0 for v in got.values()), {k: v for k, v in got.items() if v >= 0}
    assert all(v == -4 for k, v in got.items() if k.startswith('mixed') and 'add' not in k)


def test_the_recorded_cases_reach_the_kernels():
    """Every case is recorded for each of its element types; a call is recorded as refused only where the recorder's EXPECT_REFUSED names it."""
    TOOL.check_reach(FIXTURE['digests'])


@pytest.mark.gpu
@pytest.mark.parametrize('case,dt', TOOL.RUNS, ids=['%s/%s' % (c[0], dt) for c, dt in TOOL.RUNS])
def test_pool_bits(libs, case, dt):
    got, want = TOOL.run_case(libs[0], libs[1], case, dt), FIXTURE['digests']['%s/%s' % (case[0], dt)]
    assert sorted(got) == sorted(want)
    diff = {call: (got[call], want[call]) for call in want if got[call] != want[call]}
    assert not diff, diff
