"""Every output bit of the loss entry points (csrc/loss.hip), and every answer of their size queries, against tests/golden/loss_bits.json: recorded by
tools/record_loss_bits.py from a library built from the commit BEFORE the per-pixel body, the host paths and the autograd node of the cross-entropy losses were
consolidated. The inputs are built by the recorder's own functions; the outputs are fixed-order and deterministic, so the digests have to be equal."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_loss_bits', os.path.join(ROOT, 'tools', 'record_loss_bits.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.FIXTURE) as f:
        return tool, json.load(f)


TOOL, FIXTURE = _tool()


@pytest.fixture(scope='module')
def K():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def test_loss_size_queries_answer_what_the_recorded_table_holds():
    """The seven size queries for the thirteen cases, the main loss (8 x 192^2 x 19 -> 768^2) and one Cityscapes image (256 x 512 -> 1024 x 2048): pure host code, no GPU."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    assert FIXTURE['size_queries'] == TOOL.SIZE_NAMES and sorted(FIXTURE['sizes']) == sorted(c[0] for c in TOOL.CASES + TOOL.SIZE_ONLY)
    for case in TOOL.CASES + TOOL.SIZE_ONLY:
        assert TOOL.sizes(lib, L, case) == FIXTURE['sizes'][case[0]], case


def test_the_recorded_cases_reach_the_kernels():
    """At most two of the thirteen cases may be refused per call family, and every case is recorded."""
    assert sorted(FIXTURE['digests']) == sorted(c[0] for c in TOOL.CASES) and len(TOOL.CASES) == 13
    for call in {k for d in FIXTURE['digests'].values() for k in d}:
        assert sum(d[call] == 'refused' for d in FIXTURE['digests'].values()) <= TOOL.MAX_REFUSED, call


@pytest.mark.gpu
@pytest.mark.parametrize('case', TOOL.CASES, ids=[c[0] for c in TOOL.CASES])
def test_loss_bits(K, case):
    got, want = TOOL.run_case(K, case), FIXTURE['digests'][case[0]]
    assert sorted(got) == sorted(want)
    diff = {call: (got[call], want[call]) for call in want if got[call] != want[call]}
    assert not diff, diff


# ---- the relaxed-border families: recorded from the commit before their kernels became a third label form of the cross-entropy kernels --------------------------------
def test_relax_size_queries_answer_what_the_recorded_table_holds():
    """The four relaxed size queries for the same fifteen shapes; none of the thirteen cases is without a field (the set words fit LDS)."""
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    assert FIXTURE['relax_size_queries'] == TOOL.RELAX_SIZE_NAMES and sorted(FIXTURE['relax_sizes']) == sorted(c[0] for c in TOOL.CASES + TOOL.SIZE_ONLY)
    for case in TOOL.CASES + TOOL.SIZE_ONLY:
        assert TOOL.relax_sizes(lib, case) == FIXTURE['relax_sizes'][case[0]], case
    assert all(FIXTURE['relax_sizes'][c[0]][2] > 0 for c in TOOL.CASES)


def test_the_recorded_relax_cases_reach_the_kernels():
    assert sorted(FIXTURE['relax_digests']) == sorted(c[0] for c in TOOL.CASES)
    for call in {k for d in FIXTURE['relax_digests'].values() for k in d}:
        assert sum(d[call] == 'refused' for d in FIXTURE['relax_digests'].values()) <= TOOL.MAX_REFUSED, call


@pytest.mark.gpu
@pytest.mark.parametrize('case', TOOL.CASES, ids=[c[0] for c in TOOL.CASES])
def test_relax_loss_bits(K, case):
    got, want = TOOL.run_relax_case(K, case), FIXTURE['relax_digests'][case[0]]
    assert sorted(got) == sorted(want)
    diff = {call: (got[call], want[call]) for call in want if got[call] != want[call]}
    assert not diff, diff
