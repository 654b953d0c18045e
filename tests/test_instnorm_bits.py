"""Every output bit of the InstanceNorm entry points (csrc/instnorm.hip, fp32 and bf16) and every answer of pm_instnorm_workspace against
tests/golden/instnorm_bits.json: recorded by tools/record_instnorm_bits.py from the commit BEFORE the reductions and the elementwise driver of BatchNorm and
InstanceNorm became one set of parts (csrc/norm_parts.h). The inputs are built by the recorder's own functions; the outputs are fixed-order and deterministic, so the
digests have to be equal."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_instnorm_bits', os.path.join(ROOT, 'tools', 'record_instnorm_bits.py'))
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


def test_instnorm_workspace_answers_what_the_recorded_table_holds():
    """pm_instnorm_workspace for the six cases and the four shapes of the workload: pure host code, no GPU."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    shapes = [(c[0], c[1]) for c in TOOL.CASES + TOOL.SIZE_ONLY]
    assert sorted(FIXTURE['workspaces']) == sorted(name for name, _ in shapes)
    assert [s for _, s in TOOL.SIZE_ONLY] == [(8, 384, 384, 64), (8, 192, 192, 256), (8, 96, 96, 512), (8, 48, 48, 1024)]
    for name, shape in shapes:
        assert TOOL.workspace(lib, shape) == FIXTURE['workspaces'][name] > 0, name


def test_the_recorded_cases_are_complete():
    """Every case is recorded for both element types, forward and backward, in all four (relu, affine) modes; dgamma / dbeta exactly where affine is on."""
    assert sorted(FIXTURE['digests']) == sorted('%s/%s' % (c[0], dt) for c, dt in RUNS) and len(TOOL.CASES) == 6
    for key, calls in FIXTURE['digests'].items():
        assert sorted(calls) == sorted('instnorm_%s[relu=%d,affine=%d]' % (d, r, a) for d in ('fwd', 'bwd') for r, a in TOOL.MODES), key
        for call, outs in calls.items():
            want = ['invstd', 'mean', 'y'] if 'fwd' in call else (['dbeta', 'dgamma', 'dx'] if 'affine=1' in call else ['dx'])
            assert sorted(outs) == want, (key, call)


@pytest.mark.gpu
@pytest.mark.parametrize('case,dt', RUNS, ids=['%s/%s' % (c[0], dt) for c, dt in RUNS])
def test_instnorm_bits(K, case, dt):
    got, want = TOOL.run_case(K, case, dt), FIXTURE['digests']['%s/%s' % (case[0], dt)]
    assert sorted(got) == sorted(want)
    diff = {call: (got[call], want[call]) for call in want if got[call] != want[call]}
    assert not diff, diff
