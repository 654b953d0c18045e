"""Records the output bits of the InstanceNorm entry points (csrc/instnorm.hip: K.instnorm_fwd / K.instnorm_bwd, both element types) and the answers of
pm_instnorm_workspace into tests/golden/instnorm_bits.json; tests/test_instnorm_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_instnorm_bits.py

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. The workspace answers are pure
host code and are recorded on any machine; the digests need the GPU and are kept as they are when there is none. Every output is fixed-order and deterministic, so a
digest (sha256 of the output's bytes) either matches or the change altered a bit.

A case is (name, (n, h, w, c), pitched): the smallest shapes that reach every arm of the plan (in_chunks / in_plan) and of the elementwise driver (fixed_ok).
Each is run as fp32 and bf16 with relu in {0, 1} and affine in {off, on}. pitched: x, y, dy and dx are views of pitch PITCH inside wider slabs, and the forward call
writes y over its own input. Inputs come from CPU generators with fixed seeds."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'instnorm_bits.json')
EPS = 1e-5
PITCH = 272

CASES = [
    ('one-pixel', (3, 1, 1, 8), False),                    # variance 0: invstd = 1 / sqrt(eps)
    ('one-ragged-chunk', (2, 7, 9, 8), False),             # GPR 8; the fixed driver with 2 (fp32) and 1 (bf16) channel groups
    ('ragged-column-block', (3, 49, 47, 264), False),      # 36 chunks per image, GPR 16, fp32: five column blocks, 8 of 64 channels in the last; the (pixel, group) driver
    ('fixed-128-groups', (2, 16, 16, 512), False),         # the fixed driver with 128 and 64 channel groups
    ('strided-second-stage', (1, 80, 81, 8), False),       # 102 chunks > 64 second-stage lanes
    ('pitched', (3, 49, 47, 264), True),
]
SIZE_ONLY = [('stem', (8, 384, 384, 64)), ('layer1', (8, 192, 192, 256)), ('layer2', (8, 96, 96, 512)), ('layer3', (8, 48, 48, 1024))]      # profiles/instnorm_probe.txt
DTYPES = ('f32', 'bf16')
MODES = [(relu, affine) for relu in (0, 1) for affine in (0, 1)]


def workspace(lib, shape):
    return lib.pm_instnorm_workspace(*shape)


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def _dev(cpu, dtype, pitched, off=0):
    """CPU NHWC fp32 values (or a shape) -> device tensor of `dtype`: dense, or a channel slice at `off` of a slab PITCH channels wide."""
    import torch
    n, h, w, c = cpu.shape if torch.is_tensor(cpu) else cpu
    v = torch.zeros((n, h, w, PITCH if pitched else c), dtype=dtype, device='cuda')[..., off:off + c] if pitched else torch.zeros((n, h, w, c), dtype=dtype, device='cuda')
    if torch.is_tensor(cpu):
        v.copy_(cpu)
    return v


def inputs(shape, dtype, pitched):
    """-> x, dy (device tensors of `dtype`), gamma, beta (device fp32). Channel means far from zero in every third channel; a negative gamma in every fourth."""
    import torch
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31 + c + h)
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand(c, generator=g)) + torch.randn(c, generator=g)
    x[..., ::3] += 40.0
    dy = torch.randn(shape, generator=g)
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[1::4] *= -1.0
    beta = 0.3 * torch.randn(c, generator=g)
    return _dev(x, dtype, pitched, 8), _dev(dy, dtype, pitched, 0), gamma.cuda(), beta.cuda()


def run_case(K, case, dt):
    """Forward and backward in every mode on the case's inputs -> {call: {output: sha256}}."""
    import torch
    name, shape, pitched = case
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    x, dy, gamma, beta = inputs(shape, dtype, pitched)
    out = {}
    for relu, affine in MODES:
        ga, be = (gamma, beta) if affine else (None, None)
        if pitched:
            xa = _dev(shape, dtype, True, 0)
            xa.copy_(x)
            y, mean, invstd = K.instnorm_fwd(xa, ga, be, EPS, bool(relu), out=xa)
            dx, dgamma, dbeta = K.instnorm_bwd(dy, x, y, ga, mean, invstd, bool(relu), want_affine=bool(affine), out=_dev(shape, dtype, True, 0))
        else:
            y, mean, invstd = K.instnorm_fwd(x, ga, be, EPS, bool(relu))
            dx, dgamma, dbeta = K.instnorm_bwd(dy, x, y, ga, mean, invstd, bool(relu), want_affine=bool(affine))
        tag = '[relu=%d,affine=%d]' % (relu, affine)
        out['instnorm_fwd' + tag] = dict(y=digest(y), mean=digest(mean), invstd=digest(invstd))
        out['instnorm_bwd' + tag] = {k: digest(v) for k, v in dict(dx=dx, dgamma=dgamma, dbeta=dbeta).items() if v is not None}
    torch.cuda.synchronize()
    return out


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    fixture = {'digests': {}}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            fixture = json.load(f)
    fixture['workspaces'] = {name: workspace(lib, shape) for name, shape, *_ in CASES + SIZE_ONLY}
    if torch.cuda.is_available():
        from pinthememory_amd.hip import kernels as K
        version = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--version'], capture_output=True, text=True).stdout
        fixture['hipcc'] = next((l.strip() for l in version.splitlines() if 'version' in l.lower()), '')      # for information only
        fixture['digests'] = {'%s/%s' % (c[0], dt): run_case(K, c, dt) for c in CASES for dt in DTYPES}
    else:
        print('no GPU: workspace answers recorded, digests kept as they were')
    with open(FIXTURE, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d case digests, %d workspace shapes -> %s' % (len(fixture['digests']), len(fixture['workspaces']), FIXTURE))


if __name__ == '__main__':
    main()
