"""BatchNorm passes at the workload's shapes, both tiers: median of 30 calls (HIP events, us) per line.

    python tools/bn_probe.py                      # the in-tree library
    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/bn_probe.py

Lines: statistics (bn_stats_finalize), apply (+ residual + ReLU + mask bytes), backward reduce (mask rebuilt from x; from the mask bytes with the masked gradient
stored) and backward apply, as fp32 and as bf16; the stem pair (fp32); and, under PM_DIST_FORCE=1 in a one-rank group, forward + backward of five conv_bn_act_n
branches -- one all-gather and one all-reduce for five SyncBatchNorm layers. The package is the one this file lies in, so a copy inside an export of another
commit measures that commit's Python paths. profiles/bn_refactor_ab.txt holds a parent / tree / parent / tree series of it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=os.environ.get('MASTER_PORT', '29531'), RANK='0', WORLD_SIZE='1', PM_DIST_FORCE='1')

import torch  # noqa: E402

SHAPES = [(8, 192, 192, 64), (8, 192, 192, 256), (8, 96, 96, 512), (8, 48, 48, 2048)]
STEM = (8, 384, 384, 64)
CALLS = 30


def median_us(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    from pinthememory_amd.hip import kernels as K, lib as L, ops
    from pinthememory_amd.network import mynn
    print('bn_probe: %s, library %s, median of %d calls (HIP events, us)' % (torch.cuda.get_device_name(0), L.LIB_PATH, CALLS))
    g = torch.Generator().manual_seed(5)
    for dtype, tag in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
        for shape in SHAPES:
            c = shape[3]
            x, dy, res = (torch.randn(shape, generator=g).to('cuda', dtype) for _ in range(3))
            gamma, beta = torch.rand(c, generator=g).cuda() + 0.5, torch.randn(c, generator=g).cuda() * 0.1
            mean, invstd = K.bn_stats_finalize(x, 1e-5)
            y, mask = K.bn_apply(x, mean, invstd, gamma, beta, residual=res, relu=True, want_mask=True)
            sums, gm = K.bn_bwd_reduce_mask(dy, mask, x, mean, invstd, want_gmask=True)
            count = float(shape[0] * shape[1] * shape[2])
            name = '%s %d x %d x %d x %d' % ((tag,) + shape)
            for line, fn in (('statistics', lambda: K.bn_stats_finalize(x, 1e-5)),
                             ('apply + residual + ReLU + mask', lambda: K.bn_apply(x, mean, invstd, gamma, beta, residual=res, relu=True, want_mask=True)),
                             ('apply + ReLU', lambda: K.bn_apply(x, mean, invstd, gamma, beta, relu=True)),
                             ('backward reduce, mask from x', lambda: K.bn_bwd_reduce(dy, None, x, mean, invstd, 2, gamma, beta)),
                             ('backward reduce, mask bytes, gmask', lambda: K.bn_bwd_reduce_mask(dy, mask, x, mean, invstd, want_gmask=True)),
                             ('backward apply, mask from x', lambda: K.bn_bwd_apply(dy, None, x, mean, invstd, gamma, sums, count, 2, False, beta)),
                             ('backward apply of gmask', lambda: K.bn_bwd_apply(gm, None, x, mean, invstd, gamma, sums, count, 0, False))):
                print('%-34s | %-36s %10.1f' % (name, line, median_us(fn)))
            del x, dy, res, y, mask, gm
    x = torch.randn(STEM, generator=g).cuda()
    gamma, beta = torch.rand(STEM[3], generator=g).cuda() + 0.5, torch.randn(STEM[3], generator=g).cuda() * 0.1
    mean, invstd = K.bn_stats_finalize(x, 1e-5)
    pooled, arg = K.maxpool_bn_relu_fwd(x, mean, invstd, gamma, beta)
    dyp = torch.randn(tuple(pooled.shape), generator=g).cuda()
    print('%-34s | %-36s %10.1f' % ('fp32 %d x %d x %d x %d' % STEM, 'stem pair: reduce + apply from the pool', median_us(lambda: K.bn_relu_bwd_pool(dyp, arg, x, mean, invstd, gamma, beta))))
    del x, pooled, arg, dyp

    mynn.set_bnfunc(torch.nn.SyncBatchNorm)
    torch.manual_seed(6)
    seqs = [torch.nn.SyncBatchNorm.convert_sync_batchnorm(torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, bias=False), mynn.Norm2d(256), torch.nn.ReLU())).cuda().train()
            for _ in range(5)]
    xs = [torch.randn(8, 64, 48, 48).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for _ in seqs]

    def exchange():
        ops.begin_forward()
        outs = ops.conv_bn_act_n(xs, seqs, [None] * 5)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    print('%-34s | %-36s %10.1f' % ('fp32 5 x (8 x 48 x 48 x 64 -> 256)', 'SyncBN exchange of five layers, f + b', median_us(exchange)))
    from pinthememory_amd import rccl
    rccl.shutdown()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
