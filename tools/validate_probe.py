"""GPU: the validation sweep (K.upsample_eval: loss + class map + confusion matrix of the up-sampled logits in one pass) beside the composed sequence it replaces,
resize -> cross_entropy -> argmax -> fast_hist on the same device tensors, at one Cityscapes image at the head's stride (1 x 19 x 256 x 512 -> 1024 x 2048) and at the
flagship crop (8 x 19 x 192^2 -> 768^2). HIP events around every single call, warm-up first, medians over REPS calls; variants are visited round-robin so that drift
hits all alike. Algorithmic bytes: what each form must move at the least (inputs once, outputs once, every materialised intermediate written once and read by each
consumer), and the TB/s the median amounts to.

    python tools/validate_probe.py [--reps 30] [--out profiles/validate_probe.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from pinthememory_amd import build, harness, synth
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('validate_probe: needs a GPU')

C = 19
SHAPES = [(1, (256, 512), (1024, 2048)), (8, (192, 192), (768, 768))]
with open(build.STAMP) as f:
    stamp = f.read().strip()[:16]
lines = ['validate_probe: %s, library build %s, median of %d calls (HIP events, us), min .. max' % (torch.cuda.get_device_name(0), stamp, a.reps)]
ok = True
for n, hw, HW in SHAPES:
    _, lab = synth.make_batch(n, HW)
    lab = lab.cuda()
    lg = K.new((n, hw[0], hw[1], C), torch.zeros(1, device='cuda'), pitch_pad=True)
    lg.copy_(torch.randn(n, hw[0], hw[1], C, generator=torch.Generator().manual_seed(1)).cuda() * 3)
    low = ops.nchw(lg)
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    assert K.upsample_eval_ok(lg, HW)

    def composed():
        up = ops.resize(low, HW)
        loss = F.cross_entropy(up, lab, ignore_index=255)
        pred = up.argmax(1)
        return loss, harness.fast_hist(pred, lab, C)

    variants = [('fused: upsample_eval, loss + hist', lambda: K.upsample_eval(lg, lab, 1.0, hist=hist)),
                ('fused: upsample_eval, loss + hist + class map', lambda: K.upsample_eval(lg, lab, 1.0, hist=hist, want_pred=True)),
                ('composed: resize -> cross_entropy -> argmax -> fast_hist', composed)]
    pix, lowb = n * HW[0] * HW[1], n * hw[0] * hw[1] * C * 4
    up_b = pix * C * 4
    nbytes = {variants[0][0]: lowb + pix * 8,
              variants[1][0]: lowb + pix * 8 + pix,
              # up-sampled logits written once, read by cross_entropy and argmax; labels read by cross_entropy and fast_hist; the int64 class map written and read
              variants[2][0]: lowb + 3 * up_b + 2 * pix * 8 + 2 * pix * 8}
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append('%d x %d x %d x %d logits -> %d x %d labels' % (n, C, hw[0], hw[1], HW[0], HW[1]))
    for name, _ in variants:
        v = times[name]
        lines.append('  %-58s %9.1f   %9.1f .. %9.1f   %8.1f MB  %6.3f TB/s' % (name, med[name], min(v), max(v), nbytes[name] / 1e6, nbytes[name] / med[name] / 1e6))
    lines.append('  fused (with class map) / composed: %.3f' % (med[variants[1][0]] / med[variants[2][0]]))
    ok = ok and med[variants[1][0]] < med[variants[2][0]] and med[variants[0][0]] < med[variants[2][0]]
text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
assert ok, 'the fused call is not faster than the composed sequence at every shape'
