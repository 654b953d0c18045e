"""Records the output bits of every BatchNorm entry point (csrc/bn.hip, both element types) and of the Python paths built on them (hip/ops.py) into
tests/golden/bn_bits.json; tests/test_bn_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_bn_bits.py [--parent-tree DIR]

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. The workspace answers are pure
host code and are recorded on any machine; the digests need the GPU and are kept as they are when there is none. Every output is fixed-order and deterministic, so a
digest (sha256 of the output's bytes) either matches or the change altered a bit.

--parent-tree DIR: an export of the parent commit (git archive) with its own library built inside. The Python paths (PATH_PROBE: one training step on both tiers,
a bottleneck with a downsample branch, three conv_bn_act_n branches; plain and with PM_DIST_FORCE=1, which sends a one-rank group through the merged exchanges) are
run there in fresh child processes and recorded under 'paths'; without the option they are kept as they were.

A case is (name, (n, h, w), C of the fp32 run, C of the bf16 run, pitch pad). Inputs come from CPU generators with fixed seeds. The tensor the ReLU masks are
rebuilt from holds values within round-off of zero after the affine: in every fourth channel beta is 0, the mean is a bf16 number and a quarter of the pixels
equal it, so that (x - mean) * invstd * gamma evaluated any other way than the library's two FMAs lands on the other side of zero."""
import hashlib
import json
import os
import subprocess
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'bn_bits.json')
MAX_REFUSED = 2      # cases a call family may be refused for: the single pixel and at most one more
EPS, MOMENTUM = 1e-5, 0.1

CASES = [
    ('one-column-block', (2, 5, 7), 8, 8, 0),                  # bf16 fixed path with one group; two pixel chunks
    ('few-pixels-past-64-channels', (1, 3, 3), 68, 72, 0),     # fewer pixels than row lanes; bf16: the generic pass, 16 lane groups
    ('padded-pitch', (2, 13, 11), 64, 64, 8),                  # bf16 with 8 lane groups; pixels no multiple of the row lanes; pitch != C
    ('strided-second-stage', (2, 50, 45), 136, 136, 0),        # 71 pixel chunks > 64 second-stage lanes; C past 128; bf16 generic (17 groups)
    ('fixed-32-groups', (4, 16, 16), 256, 256, 0),
    ('two-pixels', (1, 1, 2), 16, 16, 0),
    ('one-pixel', (1, 1, 1), 16, 16, 0),                       # bn_stats_finalize is refused
]
STEM_CASES = [('stem-13x11', (2, 13, 11), 8), ('stem-8x8', (1, 8, 8), 64)]      # the shapes of tests/test_bn_tail_fusion.py
SLAB_CASE = ('slab-partials', 2100, 24)                        # rows (66 slabs, the last one ragged), channels
SIZE_ONLY = [('stem', (8, 384, 384), 64, 64, 0), ('layer1', (8, 192, 192), 256, 256, 0), ('layer4', (8, 96, 96), 2048, 2048, 0), ('aspp-pool', (8, 1, 1), 256, 256, 0)]
DTYPES = ('f32', 'bf16')


def workspaces(lib, L, case):
    """pm_bn_workspace for the case's shape as fp32 and as bf16 (fake, aligned, non-null pointer: the query never dereferences it)."""
    _, (n, h, w), c32, c16, pad = case
    return [lib.pm_bn_workspace(byref(L.PmTensor(0x10000, n, h, w, c, c + pad, dt, 0))) for c, dt in ((c32, L.PM_F32), (c16, L.PM_BF16))]


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def _dev(cpu, dtype, pad=0):
    """CPU NHWC fp32 values -> device tensor of `dtype` whose pitch is C + pad."""
    import torch
    n, h, w, c = cpu.shape
    buf = torch.zeros((n, h, w, c + pad), dtype=dtype, device='cuda')
    v = buf[..., :c]
    v.copy_(cpu)
    return v


def inputs(shape, c, dtype, pad):
    """-> dict of device tensors: x (statistics), xz (holds the near-zero values), dy, res, r (a second raw tensor), and the per-channel fp32 parameters."""
    import torch
    n, h, w = shape
    g = torch.Generator().manual_seed(11)
    full = (n, h, w, c)
    x, dy, res, r = (torch.randn(full, generator=g) * s + o for s, o in ((1.5, 0.3), (1.0, 0.0), (1.0, 0.1), (0.7, -0.2)))
    mean, beta, r_mean, r_beta = (torch.randn(c, generator=g) * s + o for s, o in ((0.2, 0.3), (0.2, 0.0), (0.2, -0.2), (0.1, 0.0)))
    invstd, gamma, r_invstd, r_gamma, rvar = (torch.rand(c, generator=g) + 0.5 for _ in range(5))
    gamma[1::3] *= -1.0
    mean[::4] = mean[::4].bfloat16().float()
    beta[::4] = 0.0
    xz, u = x.clone(), torch.rand(full, generator=g)
    hit = u < 0.25
    hit[..., [i for i in range(c) if i % 4]] = False
    xz = torch.where(hit, mean.expand(full), xz)
    zero = mean - beta / (invstd * gamma)                                  # the other channels: the root of the affine, and its two neighbours
    for k, lo in ((0, 0.25), (1, 0.30), (-1, 0.35)):
        near = zero if k == 0 else torch.nextafter(zero, zero + k)
        sel = (u >= lo) & (u < lo + 0.05) & ~hit
        sel[..., ::4] = False
        xz = torch.where(sel, near.expand(full), xz)
    d = {k: _dev(v, dtype, pad) for k, v in dict(x=x, xz=xz, dy=dy, res=res, r=r).items()}
    d.update({k: v.cuda() for k, v in dict(mean=mean, invstd=invstd, gamma=gamma, beta=beta, r_mean=r_mean, r_invstd=r_invstd, r_gamma=r_gamma, r_beta=r_beta,
                                           rmean0=mean * 0.5, rvar0=rvar).items()})
    return d


def _rec(out, name, fn):
    """out[name] = {output: sha256} of fn()'s tensors, or 'refused' when the library turns the call down."""
    from pinthememory_amd.hip import lib as L
    try:
        out[name] = {k: digest(v) for k, v in fn().items() if v is not None}
    except L.PinmemError:
        out[name] = 'refused'


def run_case(K, case, dt):
    """Every call of every family on the case's inputs -> {call: {output: sha256} or 'refused'}."""
    import torch
    name, shape, c32, c16, pad = case
    c, dtype = (c32, torch.float32) if dt == 'f32' else (c16, torch.bfloat16)
    t = inputs(shape, c, dtype, pad)
    x, xz, dy, mean, invstd, gamma, beta = t['x'], t['xz'], t['dy'], t['mean'], t['invstd'], t['gamma'], t['beta']
    pixels = shape[0] * shape[1] * shape[2]
    out = {}

    def running(fn):
        rm, rv = t['rmean0'].clone(), t['rvar0'].clone()
        m, i = fn(rm, rv)
        return dict(mean=m, invstd=i, running_mean=rm, running_var=rv)
    _rec(out, 'bn_stats', lambda: dict(moments=K.bn_stats(x)))
    _rec(out, 'bn_stats_finalize', lambda: running(lambda rm, rv: K.bn_stats_finalize(x, EPS, rm, rv, MOMENTUM)))
    moms = [K.bn_stats(v) for v in (x, xz, t['res'])]
    _rec(out, 'bn_finalize', lambda: running(lambda rm, rv: K.bn_finalize(moms[0], c, EPS, rm, rv, MOMENTUM)))
    for world in (1, 3):
        parts = torch.cat(moms[:world])
        _rec(out, 'bn_merge[world=%d]' % world, lambda: dict(moments=K.bn_merge(parts, world, c)))
        _rec(out, 'bn_merge_finalize[world=%d]' % world, lambda: running(lambda rm, rv: K.bn_merge_finalize(parts, world, c, EPS, rm, rv, MOMENTUM)))
    if dt == 'f32':      # the folds never see an activation
        for bias in (None, t['r_beta']):
            _rec(out, 'bn_fold[bias=%d]' % (bias is not None), lambda: dict(zip(('scale', 'shift'), K.bn_fold(gamma, beta, t['rmean0'], t['rvar0'], EPS, bias))))
        layers = [(gamma, beta, t['rmean0'], t['rvar0']), (t['r_gamma'], t['r_beta'], t['r_mean'], t['rvar0'])]
        table = torch.tensor([p.data_ptr() for lay in layers for p in lay], dtype=torch.int64, device='cuda')
        cs, offs = torch.tensor([c, c], dtype=torch.int32, device='cuda'), torch.tensor([0, c], dtype=torch.int32, device='cuda')
        _rec(out, 'bn_fold_multi', lambda: dict(arena=K.bn_fold_multi(table, cs, offs, 2, c, 2 * c, EPS)))

    fwd = {}
    for has_res in (False, True):
        for want_mask in (False, True):
            for relu in (False, True):
                def apply():
                    r = K.bn_apply(xz, mean, invstd, gamma, beta, residual=t['res'] if has_res else None, relu=relu, want_mask=want_mask)
                    fwd[(has_res, want_mask, relu)] = r
                    return dict(y=r[0], mask=r[1]) if want_mask else dict(y=r)
                _rec(out, 'bn_apply[res=%d,mask=%d,relu=%d]' % (has_res, want_mask, relu), apply)
    if dt == 'f32':
        _rec(out, 'bn_apply_res_affine', lambda: dict(zip(('y', 'mask'), K.bn_apply_res_affine(xz, mean, invstd, gamma, beta, t['r'], t['r_mean'], t['r_invstd'], t['r_gamma'],
                                                                                                 t['r_beta'], relu=True, want_mask=True))))
    y, mask = fwd[(True, True, True)]
    sums = {}
    for mode in (0, 1, 2):
        for want_gmask in ((False,) if mode == 0 else (False, True)):
            for with_count in (False, True):
                def reduce():
                    s, gm = K.bn_bwd_reduce(dy, y if mode == 1 else None, xz, mean, invstd, mode, gamma, beta, want_gmask=want_gmask, with_count=with_count)
                    sums[(mode, with_count)] = s
                    return dict(sums=s, gmask=gm)
                _rec(out, 'bn_bwd_reduce[mode=%d,gmask=%d,count=%d]' % (mode, want_gmask, with_count), reduce)
    for want_gmask in (False, True):
        for with_count in (False, True):
            def reduce_mask():
                s, gm = K.bn_bwd_reduce_mask(dy, mask, xz, mean, invstd, want_gmask=want_gmask, with_count=with_count)
                sums[(3, with_count)] = s
                return dict(sums=s, gmask=gm)
            _rec(out, 'bn_bwd_reduce_mask[gmask=%d,count=%d]' % (want_gmask, with_count), reduce_mask)
    for mode in (0, 1, 2):
        for want_dres in (False, True):
            for dev_count in (False, True):
                def bwd_apply():
                    dx, dres = K.bn_bwd_apply(dy, y if mode == 1 else None, xz, mean, invstd, gamma, sums[(mode, dev_count)], -1.0 if dev_count else float(pixels), mode,
                                              want_dres, beta)
                    return dict(dx=dx, dres=dres)
                _rec(out, 'bn_bwd_apply[mode=%d,dres=%d,dev_count=%d]' % (mode, want_dres, dev_count), bwd_apply)
    if dt == 'f32':
        for dev_count in (False, True):
            _rec(out, 'bn_bwd_apply_mask[dev_count=%d]' % dev_count,
                 lambda: dict(dx=K.bn_bwd_apply_mask(dy, mask, xz, mean, invstd, gamma, sums[(3, dev_count)], -1.0 if dev_count else float(pixels))))
    torch.cuda.synchronize()
    return out


def run_stem(K, case):
    """The stem pair (fp32): the pool that normalises its taps, then the BatchNorm backward that gathers its gradient from the pooled one."""
    import torch
    _, shape, c = case
    t = inputs(shape, c, torch.float32, 0)
    pooled, arg = K.maxpool_bn_relu_fwd(t['xz'], t['mean'], t['invstd'], t['gamma'], t['beta'])
    dyp = _dev(torch.randn(tuple(pooled.shape), generator=torch.Generator().manual_seed(12)), torch.float32)
    out = {}
    for with_count in (False, True):
        _rec(out, 'bn_relu_bwd_pool[count=%d]' % with_count,
             lambda: dict(zip(('dx', 'sums'), K.bn_relu_bwd_pool(dyp, arg, t['xz'], t['mean'], t['invstd'], t['gamma'], t['beta'], with_count=with_count))))
    torch.cuda.synchronize()
    return out


def run_slabs(K, case):
    """Synthetic (mean, M2) slab partials of a convolution epilogue: more than 64 slabs, rows % 32 != 0."""
    import torch
    _, rows, c = case
    g = torch.Generator().manual_seed(13)
    part = torch.stack([torch.randn((rows + 31) // 32, c, generator=g) * 0.5 + 0.2, torch.rand((rows + 31) // 32, c, generator=g) * 30], dim=2).contiguous().cuda()
    rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    out = {}
    _rec(out, 'bn_partials_finalize', lambda: dict(zip(('mean', 'invstd'), K.bn_partials_finalize(part, rows, c, EPS, rm, rv, MOMENTUM)), running_mean=rm, running_var=rv))
    _rec(out, 'bn_partials_moments', lambda: dict(moments=K.bn_partials_moments(part, rows, c)))
    torch.cuda.synchronize()
    return out


# ---- the Python paths: run with the tree (or the parent's export) as working directory, `plain` or `forced` as the argument ----------------------------------
PATH_PROBE = r'''
import hashlib, json, os, sys
sys.path.insert(0, os.getcwd())
forced = sys.argv[1] == 'forced'
import torch
if forced:
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=sys.argv[2], RANK='0', WORLD_SIZE='1', PM_DIST_FORCE='1')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
from pinthememory_amd import dist as D, harness, synth
from pinthememory_amd.hip import kernels as K, ops
from pinthememory_amd.network import Resnet, deepv3plus, mynn
if forced:
    mynn.set_bnfunc(torch.nn.SyncBatchNorm)

def sha(ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().float().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()

def sync(m):
    return torch.nn.SyncBatchNorm.convert_sync_batchnorm(m) if forced else m

def step(prec):
    K.set_conv_precision(prec)
    crit = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    net = sync(synth.load_det_weights(deepv3plus.DeepR50V3PlusD(synth.model_args(), 19, crit, crit)).cuda())
    net.dsn[3].p = 0.0
    net.train()
    x, y = synth.make_batch(2, 128)
    x, y = x.cuda(), y.cuda()
    res = {}
    def run():
        out = net(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=False)
        res['loss'] = harness.total_loss(out)
        res['loss'].backward()
    n = D.count_collectives(run)
    torch.cuda.synchronize()
    K.set_conv_precision('f32')
    return dict(loss=sha([res['loss']]), grads=sha([p.grad for p in net.parameters() if p.grad is not None]),
                moments=sha([b for b in net.buffers() if b.dtype == torch.float32]), collectives=n)

def block():
    torch.manual_seed(21)
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, stride=2, bias=False), mynn.Norm2d(128))
    blk = sync(Resnet.Bottleneck(64, 32, stride=2, downsample=ds)).cuda().train()
    x = torch.randn(2, 64, 12, 10).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ops.begin_forward()
    out = blk([x, []])[0]
    (out * torch.linspace(-1, 1, out.numel(), device='cuda').view_as(out)).sum().backward()
    torch.cuda.synchronize()
    return dict(out=sha([out]), dx=sha([x.grad]), grads=sha([p.grad for p in blk.parameters()]), moments=sha([b for b in blk.buffers() if b.dtype == torch.float32]))

def branches():
    torch.manual_seed(22)
    seqs = [sync(torch.nn.Sequential(torch.nn.Conv2d(32, 64, k, padding=k // 2 * d, dilation=d, bias=False), mynn.Norm2d(64), torch.nn.ReLU())).cuda().train()
            for k, d in ((1, 1), (3, 2), (3, 3))]
    xs = [torch.randn(2, 32, 9, 7).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for _ in seqs]
    ops.begin_forward()
    outs = ops.conv_bn_act_n(xs, seqs, [None] * 3)
    sum((o * torch.linspace(-1, 1, o.numel(), device='cuda').view_as(o)).sum() * (i + 1) for i, o in enumerate(outs)).backward()
    torch.cuda.synchronize()
    return dict(out=sha(outs), dx=sha([x.grad for x in xs]), grads=sha([p.grad for s in seqs for p in s.parameters()]),
                moments=sha([b for s in seqs for b in s.buffers() if b.dtype == torch.float32]))

# a misaligned `sums` handed to an apply pass is refused by the library (PM_EINVAL raises here): reaching the end says every one was 16-byte aligned
res = dict(step_f32=step('f32'), step_bf16=step('bf16'), bottleneck=block(), branches=branches())
if forced:
    from pinthememory_amd import rccl
    rccl.shutdown()
    dist.destroy_process_group()
print('BN_PATHS', json.dumps(res, sort_keys=True))
'''


def run_paths(root, mode, port=29517, timeout=600):
    """PATH_PROBE in a fresh child process whose working directory (and package, and library) is `root` -> its dict."""
    env = {k: v for k, v in os.environ.items() if k != 'PM_LIB'}
    r = subprocess.run([sys.executable, '-c', PATH_PROBE, mode, str(port)], cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith('BN_PATHS ')]
    assert lines, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(lines[0][len('BN_PATHS '):])


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    fixture = {'digests': {}, 'paths': {}}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            fixture = json.load(f)
    fixture['workspaces'] = {c[0]: workspaces(lib, L, c) for c in CASES + SIZE_ONLY}
    if torch.cuda.is_available():
        from pinthememory_amd.hip import kernels as K
        version = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--version'], capture_output=True, text=True).stdout
        fixture['hipcc'] = next((l.strip() for l in version.splitlines() if 'version' in l.lower()), '')      # for information only
        fixture['digests'] = {'%s/%s' % (c[0], dt): run_case(K, c, dt) for c in CASES for dt in DTYPES}
        fixture['digests'].update({c[0]: run_stem(K, c) for c in STEM_CASES})
        fixture['digests'][SLAB_CASE[0]] = run_slabs(K, SLAB_CASE)
        check_reach(fixture['digests'])
        if '--parent-tree' in sys.argv:
            tree = os.path.abspath(sys.argv[sys.argv.index('--parent-tree') + 1])
            fixture['paths'] = {mode: run_paths(tree, mode) for mode in ('plain', 'forced')}
    else:
        print('no GPU: workspace answers recorded, digests kept as they were')
    with open(FIXTURE, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d case digests, %d workspace shapes, paths %s -> %s' % (len(fixture['digests']), len(fixture['workspaces']), sorted(fixture['paths']), FIXTURE))


def check_reach(digests):
    """A call family may be recorded as refused for the single pixel and for at most one case besides, per element type."""
    for dt in DTYPES:
        runs = {k: d for k, d in digests.items() if k.endswith('/' + dt)}
        for call in sorted({k for d in runs.values() for k in d}):
            refused = [k for k, d in runs.items() if d.get(call) == 'refused']
            assert len(refused) <= MAX_REFUSED and len([k for k in refused if not k.startswith('one-pixel/')]) <= 1, 'replace a case: %s is refused for %s' % (call, refused)
    for k, d in digests.items():
        if '/' not in k:
            assert 'refused' not in d.values(), (k, d)


if __name__ == '__main__':
    main()
