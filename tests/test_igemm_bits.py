"""Every output bit of the implicit-GEMM convolution kernel (csrc/conv_igemm_kernel.h and the pieces it is put together from, through conv_igemm.hip and
conv_split.hip), of the streaming pointwise kernel (csrc/pwstream.hip) and of the split-K reduce, through pm_conv_fwd / pm_conv_bwd_data(_masked) /
pm_conv_bwd_weight, against tests/golden/igemm_bits.json: recorded by tools/record_igemm_bits.py from the commit BEFORE the kernel's tile map, LDS layouts, window
gather and epilogues were written once (csrc/conv_igemm_parts.h). The 'wino-*' cases hold the Winograd transforms (csrc/winograd.hip) the same way, on maps that do
not tile -- ragged edge tiles, dilation sub-lattices of unequal size, zero-filled K padding, every fused epilogue, the split-K slab sum of the weight gradient, F(4 x 4),
F(2 x 2) and the fused kernel: recorded from the commit BEFORE the transforms' two-pass body and the output epilogue were written once (wino_sandwich,
wino_epilogue). The inputs are built by the recorder's own functions; the kernels are deterministic (fixed-order split-K reduce), so the digests have to be equal --
and the launches each case makes have to be the ones that were recorded."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('record_igemm_bits', os.path.join(ROOT, 'tools', 'record_igemm_bits.py'))
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


def test_the_recorded_cases_launched_the_kernel_forms_they_are_named_for():
    """From the in-library profile kept beside the digests: every gather mode and K-state variant on the fp32-MFMA and the split-operand form, one and two LDS
    stages, every tile, split-K through the reduce, the batched Winograd launches, the streaming kernel, and the bf16-operand forms PREC 1 - 4. No GPU."""
    TOOL.check_reach(FIXTURE)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c['name'] for c in TOOL.CASES])
def test_igemm_bits(K, name):
    got, reach = TOOL.run_case(K, TOOL.BY_NAME[name])
    assert reach == FIXTURE['reach'][name]
    want = FIXTURE['digests'][name]
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
