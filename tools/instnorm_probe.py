"""GPU: the per-image normalisation kernels (csrc/instnorm.hip) at the three workload shapes of an IBN trunk at bs = 8, 768^2 -- the stem 8 x 384^2 x 64, layer1
8 x 192^2 x 256, layer2 8 x 96^2 x 512 -- in fp32 and bf16: the forward + backward pair (affine, ReLU fused) of
  (new) K.instnorm_fwd + K.instnorm_bwd: six launches whatever the batch size;
  (a)   stock torch: F.relu(F.instance_norm(x, weight, bias)) and its autograd backward on the same channels-last tensor;
  (b)   n per-image calls of this project's BatchNorm kernels (K.bn_stats_finalize, K.bn_apply, K.bn_bwd_reduce, K.bn_bwd_apply on one-image views): 6 n launches.
HIP events around groups of GROUP pairs, warm-up first, the variants visited alternately so that drift hits all alike; per pair: the median over the groups, min .. max.
GB/s are ALGORITHMIC bytes over that time: ten passes over the tensor (forward: x read for the statistics, x read and y written by the apply pass; backward: dy, x, y
read by the reduction, dy, x, y read and dx written by the apply pass) -- what the two-stage scheme has to move when nothing stays in cache, the same figure for every
variant whatever it really moves. Then the step time of harness.plain_train_step on the IBN net (wt_layer 0 0 4 4 4 0 0, no memory) next to harness.agg_train_step on
the plain net with memory, bs = 8, 768^2, fp32 tier, from the same session.
Every case runs in a child process of its own under its own time limit; after a child that did not end cleanly nothing more is started.

    python tools/instnorm_probe.py [--out profiles/instnorm_probe.txt] [--groups 8] [--group 3] [--limit 240]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('stem', (8, 384, 384, 64)), ('layer1', (8, 192, 192, 256)), ('layer2', (8, 96, 96, 512))]
CASES = [(name, shape, dt) for name, shape in SHAPES for dt in ('f32', 'bf16')]
EPS = 1e-5

ap = argparse.ArgumentParser()
ap.add_argument('--groups', type=int, default=8)
ap.add_argument('--group', type=int, default=3)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--limit', type=int, default=240, help='seconds a child may take')
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--case', type=int, default=None, help='(child) index into the kernel cases')
ap.add_argument('--step', choices=['ibn_plain', 'plain_agg'], default=None, help='(child) which train step to time')
ap.add_argument('--out', default=None)
a = ap.parse_args()


def kernel_case(index):
    import torch
    import torch.nn.functional as F
    from pinthememory_amd.hip import kernels as K
    name, shape, dt = CASES[index]
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    n, h, w, c = shape
    g = torch.Generator(device='cuda').manual_seed(index)
    x = torch.randn(shape, generator=g, device='cuda').to(dtype)
    dy = torch.randn(shape, generator=g, device='cuda').to(dtype)
    gamma = 1 + 0.1 * torch.randn(c, generator=g, device='cuda')
    beta = 0.1 * torch.randn(c, generator=g, device='cuda')
    xt = x.permute(0, 3, 1, 2).requires_grad_(True)      # logical NCHW, channels-last memory: the same bytes
    dyt = dy.permute(0, 3, 1, 2)
    gt, bt = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)

    def new():
        y, mean, invstd = K.instnorm_fwd(x, gamma, beta, EPS, True)
        return y, K.instnorm_bwd(dy, x, y, gamma, mean, invstd, True)

    def stock():
        y = F.relu(F.instance_norm(xt, weight=gt, bias=bt, eps=EPS))
        return y, torch.autograd.grad(y, [xt, gt, bt], dyt)

    def per_image():
        out = []
        for i in range(n):
            xi, di = x[i:i + 1], dy[i:i + 1]
            mean, invstd = K.bn_stats_finalize(xi, EPS)
            y = K.bn_apply(xi, mean, invstd, gamma, beta, relu=True)
            sums, _ = K.bn_bwd_reduce(di, y, xi, mean, invstd, 1)
            out.append((y, K.bn_bwd_apply(di, y, xi, mean, invstd, gamma, sums, float(h * w), 1, False)[0]))
        return out

    # the variants' results before anything is timed: largest difference over the largest value, reported; anything gross ends the case
    (y1, (dx1, dg1, db1)), (y2, (dx2, dg2, db2)), pi = new(), stock(), per_image()
    rel = lambda p, q: (p.float() - q.float()).abs().max().item() / (p.float().abs().max().item() + 1e-30)
    agree = dict(y_a=rel(y1, y2.permute(0, 2, 3, 1)), dx_a=rel(dx1, dx2.permute(0, 2, 3, 1)), dgamma_a=rel(dg1, dg2), y_b=rel(y1, torch.cat([y for y, _ in pi])),
                 dx_b=rel(dx1, torch.cat([d for _, d in pi])))
    # fp32: all three agree to round-off. bf16: held against (b) -- the same fp32 arithmetic on the same bf16 values, rounded once; torch's bf16 path is only reported
    assert max(v for k, v in agree.items() if dt == 'f32' or k.endswith('_b')) < (1e-3 if dt == 'f32' else 2e-2), agree
    del y1, dx1, y2, dx2, pi
    variants = [('(new) instnorm_fwd + instnorm_bwd', new), ('(a) F.instance_norm + relu, autograd', stock), ('(b) %d per-image BatchNorm kernel calls' % n, per_image)]
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {nm: [] for nm, _ in variants}
    for _ in range(a.groups):
        for nm, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.group):
                fn()
            e.record()
            e.synchronize()
            times[nm].append(s.elapsed_time(e) * 1e3 / a.group)
    nbytes = 10 * x.numel() * x.element_size()
    print('%s %s %s: tensor %.1f MB, algorithmic bytes of the pair %.1f MB' % (name, 'x'.join(map(str, shape)), dt, x.numel() * x.element_size() / 1e6, nbytes / 1e6))
    med = {}
    for nm, _ in variants:
        v = times[nm]
        med[nm] = statistics.median(v)
        print('  %-42s %9.1f us   %9.1f .. %9.1f   %7.1f GB/s' % (nm, med[nm], min(v), max(v), nbytes / med[nm] / 1e3))
    print('  (new) / (a): %.3f   (new) / (b): %.3f' % (med[variants[0][0]] / med[variants[1][0]], med[variants[0][0]] / med[variants[2][0]]))
    print('  largest difference / largest value, (new) against (a): y %.1e dx %.1e dgamma %.1e; against (b): y %.1e dx %.1e'
          % (agree['y_a'], agree['dx_a'], agree['dgamma_a'], agree['y_b'], agree['dx_b']))


def step_case(which):
    import torch
    from pinthememory_amd import harness, synth
    from pinthememory_amd.network import deepv3plus
    crit = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    ibn = which == 'ibn_plain'
    args = synth.model_args(wt_layer=[0, 0, 4, 4, 4, 0, 0], memory=False) if ibn else synth.model_args()
    net = synth.load_det_weights(deepv3plus.DeepR50V3PlusD(args, 19, crit, crit)).cuda()
    opt, sched = harness.make_optimizer(net)
    x, y = (t.cuda() for t in synth.make_batch(8, 768))
    step = (lambda: harness.plain_train_step(net, opt, x, y, sched=sched)) if ibn else (lambda: harness.agg_train_step(net, opt, x, y, sched=sched))
    for _ in range(3):
        out = step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.steps):
        t = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    what = 'plain_train_step, IBN net (wt_layer 0 0 4 4 4 0 0, no memory)' if ibn else 'agg_train_step, plain net with memory (two forward passes per step)'
    print('step bs=8 768^2 fp32 tier, %-68s median of %d: %7.2f ms   %7.2f .. %7.2f   total loss %.4f'
          % (what, a.steps, statistics.median(ts), min(ts), max(ts), float(out['total'])))


def main():
    import torch
    from pinthememory_amd import build
    if not torch.cuda.is_available():
        sys.exit('instnorm_probe: needs a GPU')
    build.build()
    with open(build.STAMP) as f:
        stamp = f.read().strip()[:16]
    lines = ['instnorm_probe: %s, library build %s; device times per forward + backward pair: median of %d groups of %d pairs (HIP events, us), min .. max; GB/s of '
             'algorithmic bytes (ten passes over the tensor)' % (torch.cuda.get_device_name(0), stamp, a.groups, a.group)]
    common = ['--groups', str(a.groups), '--group', str(a.group), '--warmup', str(a.warmup), '--steps', str(a.steps)]
    children = [['--case', str(i)] for i in range(len(CASES))] + [['--step', 'ibn_plain'], ['--step', 'plain_agg']]
    for extra in children:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra + common, capture_output=True, text=True, timeout=a.limit)
            rc, out, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, (e.stdout or b'').decode() if isinstance(e.stdout, bytes) else (e.stdout or ''), 'time limit of %d s' % a.limit
        lines += [ln for ln in out.splitlines() if ln.startswith(('stem', 'layer', '  ', 'step'))]
        if rc != 0:
            lines.append('child %s ended with status %d: %s -- nothing more was started' % (' '.join(extra), rc, ' | '.join(err.strip().splitlines()[-3:])))
            break
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0 if not lines[-1].startswith('child') else 1


if __name__ == '__main__':
    if a.case is not None:
        kernel_case(a.case)
    elif a.step is not None:
        step_case(a.step)
    else:
        sys.exit(main())
