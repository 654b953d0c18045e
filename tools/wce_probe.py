"""GPU: the weighted forms of the fused up-sample + cross entropy at the flagship loss shape (8 x 19 x 192^2 logits -> 768^2 labels) beside the unweighted
kernels and beside the composed route (Upsample + weighted cross_entropy on materialised logits, forward + backward through autograd) that a weighted criterion
took before. HIP events around every single call, warm-up first, medians over REPS calls; variants are visited round-robin so that drift hits all alike.

    python tools/wce_probe.py [--reps 30] [--out profiles/wce_probe.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from pinthememory_amd import synth
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('wce_probe: needs a GPU')

B, C, h, H = 8, 19, 192, 768
_, lab = synth.make_batch(B, H)
lab = lab.cuda()
lg = K.new((B, h, h, C), torch.zeros(1, device='cuda'), pitch_pad=True)
lg.copy_(torch.randn(B, h, h, C, generator=torch.Generator().manual_seed(1)).cuda() * 3)
gs = torch.tensor([1.0], device='cuda')
wglob = (torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
rows = K.label_class_weights(lab, C)
leaf = ops.nchw(lg).detach().clone().requires_grad_(True)      # NCHW logits of the composed route


def unweighted():
    out, field = K.upsample_ce_fwd_field(lg, lab, 1.0)
    return K.upsample_ce_bwd_field(lg, (H, H), out, field, gs, 1.0)


def weighted(w, per_image):
    def run():
        out, field = K.upsample_wce_fwd_field(lg, lab, w, per_image, 1.0)
        return K.upsample_wce_bwd_field(lg, (H, H), out, field, gs, per_image, 1.0)
    return run


def image_weighted_with_rows():
    r = K.label_class_weights(lab, C)
    out, field = K.upsample_wce_fwd_field(lg, lab, r, True, 1.0)
    return K.upsample_wce_bwd_field(lg, (H, H), out, field, gs, True, 1.0)


def composed_global():
    leaf.grad = None
    F.cross_entropy(ops.resize(leaf, (H, H)), lab, weight=wglob, ignore_index=255).backward()


def composed_image():      # the image-based criterion on materialised logits, weight rows already on the device (the reference adds a host round trip per step)
    leaf.grad = None
    lp = F.log_softmax(ops.resize(leaf, (H, H)), dim=1)
    sum(F.nll_loss(lp[b:b + 1], lab[b:b + 1], weight=rows[b], ignore_index=255) for b in range(B)).backward()


VARIANTS = [('unweighted fwd_field + bwd_field', unweighted),
            ('weighted, global [C] weights', weighted(wglob, False)),
            ('weighted, per-image rows', weighted(rows, True)),
            ('label_class_weights', lambda: K.label_class_weights(lab, C)),
            ('per-image rows incl. label_class_weights', image_weighted_with_rows),
            ('composed: Upsample + weighted cross_entropy, fwd + bwd', composed_global),
            ('composed: Upsample + per-image nll_loss, fwd + bwd', composed_image)]

for _ in range(a.warmup):
    for _, fn in VARIANTS:
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in VARIANTS}
for _ in range(a.reps):
    for name, fn in VARIANTS:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times[name].append(s.elapsed_time(e) * 1e3)

med = {k: statistics.median(v) for k, v in times.items()}
base = med['unweighted fwd_field + bwd_field']
lines = ['wce_probe: %d x %d x %d^2 logits -> %d^2 labels, %s, median of %d calls (HIP events, us), min .. max' % (B, C, h, H, torch.cuda.get_device_name(0), a.reps)]
for name, _ in VARIANTS:
    v = times[name]
    lines.append('%-58s %9.1f   %9.1f .. %9.1f   x%.2f of unweighted' % (name, med[name], min(v), max(v), med[name] / base))
lines.append('fused weighted / composed, global: %.3f   per-image (rows included): %.3f' % (
    med['weighted, global [C] weights'] / med['composed: Upsample + weighted cross_entropy, fwd + bwd'],
    med['per-image rows incl. label_class_weights'] / med['composed: Upsample + per-image nll_loss, fwd + bwd']))
text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
assert med['weighted, global [C] weights'] < med['composed: Upsample + weighted cross_entropy, fwd + bwd']
assert med['per-image rows incl. label_class_weights'] < med['composed: Upsample + per-image nll_loss, fwd + bwd']
