"""Every output bit of the bf16 tier's LDS-DMA convolution kernels (csrc/conv16.hip: the tile kernel, narrow and wide; conv16w.hip: the persistent ring; wgrad16.hip)
through pm_conv_fwd / pm_conv_bwd_data / pm_conv_bwd_weight, against tests/golden/conv16_bits.json: recorded by tools/record_conv16_bits.py from the commit BEFORE the
kernels were put together from one gather, K-step, epilogue and ring protocol (csrc/conv16_common.h). The inputs are built by the recorder's own functions; the
kernels are deterministic (fixed-order split-K reduce), so the digests have to be equal -- and the launch each case makes has to be the one that was recorded."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_conv16_bits', os.path.join(ROOT, 'tools', 'record_conv16_bits.py'))
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


def test_the_recorded_cases_launched_the_tile_forms_they_are_named_for():
    """From the in-library profile kept beside the digests: narrow 64 / 128-row tiles with one or two stages, the K-splits (the mid-tap start, the splits that see
    only invisible filter rows), the persistent ring, the ring with one block per tile, the 256 x 256 form, the weight gradient's two tiles. No GPU."""
    TOOL.check_reach(FIXTURE)
    zero = [TOOL.BY_NAME['split-invisible/%s' % r] for r in TOOL.ROUTES.values()]
    assert all(c['pad'] == c['dil'] == c['x'][2] for c in zero)      # dilation = padding = image height: only the middle filter row is ever inside the image


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c['name'] for c in TOOL.CASES])
def test_conv16_bits(K, name):
    got, reach = TOOL.run_case(K, TOOL.BY_NAME[name])
    assert reach == FIXTURE['reach'][name]
    want = FIXTURE['digests'][name]
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
