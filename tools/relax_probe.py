"""GPU: one relaxed-border loss step (--jointwtborder) at the flagship loss shape, 8 x 19 x 192^2 logits -> 768^2 labels, forward + backward.

  fused     border-set words from the int64 labels (K.relax_border_bits), class weights from the words (K.relax_class_weights), K.upsample_relax_fwd_field and
            K.upsample_relax_bwd_field: no host sync, the up-sampled logits never materialised
  composed  what the reference does per step, as torch ops on device tensors: Upsample, ImgWtLossSoftNLL's expression (loss.py:182-263) from the uint8 multi-hot
            target, with its host copy of the target for the numpy histogram and its `.item()` per image left in, backward through autograd

Both are timed with a host clock around work that ends in a device synchronise (the composed route synchronises by itself), warm-up first, medians; the variants are
visited round-robin. The pieces of the fused route are also timed one by one with HIP events around ten back-to-back calls.

    python tools/relax_probe.py [--reps 20] [--out profiles/relax_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from pinthememory_amd import loss as L
from pinthememory_amd import synth
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--out', default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('relax_probe: needs a GPU')

B, C, h, H = 8, 19, 192, 768
_, lab = synth.make_batch(B, H)
lab = lab.cuda()
lg = K.new((B, h, h, C), torch.zeros(1, device='cuda'), pitch_pad=True)
lg.copy_(torch.randn(B, h, h, C, generator=torch.Generator().manual_seed(1)).cuda() * 3)
gs = torch.tensor([1.0], device='cuda')
leaf = ops.nchw(lg).detach().clone().requires_grad_(True)      # NCHW logits of the composed route
target = L.relaxed_border_target(lab, C)                       # the reference's input: uint8 [B, C + 1, H, H], already on the device


def fused():
    bits = K.relax_border_bits(lab, C, 1)
    rows = K.relax_class_weights(bits, C)
    out, field = K.upsample_relax_fwd_field(lg, bits, rows, 1.0)
    return out, K.upsample_relax_bwd_field(lg, (H, H), out, field, gs, 1.0)


def composed():
    leaf.grad = None
    inputs = ops.resize(leaf, (H, H))
    weights = target[:, :-1].sum(1).float()
    ignore = weights == 0
    weights[ignore] = 1
    host = target.cpu().numpy()                                # the per-step host copy
    loss = 0
    for i in range(B):
        t = host[i]
        hist = np.sum(t, axis=(1, 2)) * 1.0 / t.sum()
        cw = torch.Tensor((((hist != 0) * 1.0 * (1 - hist)) + 1)[:-1]).cuda()
        ti = target[i:i + 1, :-1].float()
        soft = F.softmax(inputs[i:i + 1], dim=1)
        logs = torch.log(torch.max(soft, ti * (soft * ti).sum(1, keepdim=True)))
        matrix = (-1 / weights[i] * (ti * cw.view(1, -1, 1, 1) * logs).sum(1)) * (1.0 - ignore[i].float())
        loss = loss + matrix.sum() / (H * H - ignore[i].sum().item() + 1)      # the per-image sync
    loss = loss / B
    loss.backward()
    return loss


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


INNER = 10      # calls between two events: one call's kernels are shorter than the host takes to enqueue them


def events(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(INNER):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / INNER


out_f, dl_f = fused()
loss_c = composed()
agree = abs(out_f[0].item() - loss_c.item()) / abs(loss_c.item())
grad_agree = ((ops.nchw(dl_f)[:, :C] - leaf.grad).abs().max() / leaf.grad.abs().max()).item()
assert agree < 1e-5 and grad_agree < 1e-3, (agree, grad_agree)

bits0 = K.relax_border_bits(lab, C, 1)
rows0 = K.relax_class_weights(bits0, C)
out0, field0 = K.upsample_relax_fwd_field(lg, bits0, rows0, 1.0)
PIECES = [('relax_border_bits (int64 labels -> words)', lambda: K.relax_border_bits(lab, C, 1)),
          ('relax_class_weights', lambda: K.relax_class_weights(bits0, C)),
          ('upsample_relax_fwd_field', lambda: K.upsample_relax_fwd_field(lg, bits0, rows0, 1.0)),
          ('upsample_relax_bwd_field', lambda: K.upsample_relax_bwd_field(lg, (H, H), out0, field0, gs, 1.0)),
          ('upsample_relax_fwd (no field)', lambda: K.upsample_relax_fwd(lg, bits0, rows0, 1.0)),
          ('relaxed_border_target (uint8 multi-hot on the device)', lambda: L.relaxed_border_target(lab, C)),
          ('unweighted CE fwd_field + bwd_field, for scale', lambda: K.upsample_ce_bwd_field(lg, (H, H), *K.upsample_ce_fwd_field(lg, lab, 1.0), gs, 1.0))]
for _ in range(a.warmup):
    fused(), composed()
    for _, fn in PIECES:
        fn()
torch.cuda.synchronize()
t_fused, t_comp, t_piece = [], [], {n: [] for n, _ in PIECES}
for _ in range(a.reps):
    t_fused.append(wall(fused))
    t_comp.append(wall(composed))
    for n, fn in PIECES:
        t_piece[n].append(events(fn))

mf, mc = statistics.median(t_fused), statistics.median(t_comp)
px = B * H * H
lines = ['relax_probe: %d x %d x %d^2 logits -> %d^2 labels, %s, medians of %d calls (us), min .. max' % (B, C, h, H, torch.cuda.get_device_name(0), a.reps),
         'both routes give the same step: loss rel %.2e, gradient %.2e of the largest entry' % (agree, grad_agree),
         '%-58s %10.1f   %10.1f .. %10.1f   host clock, synchronised' % ('fused: words + weights + fwd_field + bwd_field', mf, min(t_fused), max(t_fused)),
         '%-58s %10.1f   %10.1f .. %10.1f   host clock, synchronised' % ('composed: the reference\'s step on device tensors', mc, min(t_comp), max(t_comp)),
         'composed / fused: %.1f' % (mc / mf)]
for n, _ in PIECES:
    v = t_piece[n]
    lines.append('%-58s %10.1f   %10.1f .. %10.1f   HIP events, per call of 10 back to back' % (n, statistics.median(v), min(v), max(v)))
need = 12 * px
lines.append('relax_border_bits moves %.1f MB that the algorithm needs (8 B label in, 4 B word out per pixel): %.2f TB/s' % (
    need / 1e6, need / statistics.median(t_piece[PIECES[0][0]]) / 1e6))
text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
