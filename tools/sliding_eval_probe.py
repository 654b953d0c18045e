"""GPU: everything after the network of a sliding-window evaluation (eval.py --inference_mode sliding) of one 1024 x 2048 image at crop 768 with both flips,
from the heads' low-res logits of the 2 x 8 tiles (192^2 per tile) to the class map and the confusion matrix:
  parent route: ops.resize of the 8 tiles of each flip to 768^2, one pm_sliding_stitch per flip into the float64 accumulator, / 2, argmax, fast_hist
                (what harness.sliding_logits and its caller ran);
  new route:    what harness.evaluate_sliding runs after its forwards: harness.tile_stack of the two forwards' outputs into one pitch-padded stack, then one
                K.sliding_eval launch sequence (tile upload, up-sample + stitch + un-flip + mean + argmax + LDS counters, fold).
And the new route at scales 0.5, 1.0, 2.0 (per scale tile_stack + K.sliding_eval into the accumulator, then K.sliding_eval_finish), which the parent route never served.
Both routes start from the same per-flip tensors, pitch-padded NHWC as the heads leave them (K.new(pitch_pad=True): 20 floats per pixel). For comparison the launch
sequence alone on a stack built beforehand, and on torch.cat of the two tensors -- pixels packed to 19 floats, which sends the kernels to their 4-byte loads.
HIP events around groups of GROUP calls, warm-up first, the routes visited alternately so that drift hits both alike; per call: the median over the groups, min .. max.
Random logits * 3; the two routes' float64 mean logits and class maps are compared on the same inputs before anything is timed.

    python tools/sliding_eval_probe.py [--groups 15] [--group 4] [--out profiles/sliding_eval_probe.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pinthememory_amd import build, harness, synth
from pinthememory_amd.hip import kernels as K
from pinthememory_amd.hip import ops

ap = argparse.ArgumentParser()
ap.add_argument('--groups', type=int, default=15)
ap.add_argument('--group', type=int, default=4)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--hw', type=int, nargs=2, default=(1024, 2048))
ap.add_argument('--crop', type=int, default=768)
ap.add_argument('--out', default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('sliding_eval_probe: needs a GPU')

C, RATIO, FLIPS = 19, 4, 2
H, W = a.hw


def tile_logits(scale, seed):
    """the tile table of one scale and random low-res logits * 3 of its T tiles for each flip: one tensor per forward, pitch-padded NHWC as the heads leave them"""
    Hs, Ws = int(H * scale), int(W * scale)
    tiles = harness.sliding_tiles(Hs, Ws, a.crop, 1.0 / 3, scale)
    th, tw = tiles[0][3] - tiles[0][1], tiles[0][2] - tiles[0][0]
    shape = (len(tiles), -(-th // RATIO), -(-tw // RATIO), C)
    lg = []
    for f in range(FLIPS):
        lg.append(K.new(shape, torch.zeros(1, device='cuda'), pitch_pad=True))
        lg[f].copy_(torch.randn(shape, generator=torch.Generator().manual_seed(FLIPS * seed + f)).cuda() * 3)
    return lg, tiles, (Hs, Ws), (th, tw)


def timed(variants):
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.groups):
        for name, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.group):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / a.group)
    return times


with open(build.STAMP) as f:
    stamp = f.read().strip()[:16]
lines = ['sliding_eval_probe: %s, library build %s, %d x %d image, crop %d, both flips, %d classes; per call: median of %d groups of %d calls (HIP events, us), min .. max'
         % (torch.cuda.get_device_name(0), stamp, H, W, a.crop, C, a.groups, a.group)]
lab = synth.make_batch(1, (H, W))[1][0].cuda()
hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
lg, tiles, _, (th, tw) = tile_logits(1.0, 1)
T = len(tiles)


def parent():
    acc = None
    for f in range(FLIPS):
        up = ops.resize(ops.nchw(lg[f]), (th, tw))
        acc = K.sliding_stitch(ops.nhwc(up), tiles, H, W, bool(f), acc) if T <= harness.STITCH_MAX_TILES else harness._stitch_torch(up, tiles, H, W, bool(f), acc)
    mean = acc / FLIPS
    pred = mean.argmax(0)
    return pred, harness.fast_hist(pred, lab, C), mean


def new():
    return K.sliding_eval(harness.tile_stack(lg), tiles, (H, W), (H, W), FLIPS, labels=lab, hist=hist, want_pred=True)


stack, packed = harness.tile_stack(lg), torch.cat(lg)
assert stack.stride(2) == 20 and packed.stride(2) == C


def kernels_only():
    return K.sliding_eval(stack, tiles, (H, W), (H, W), FLIPS, labels=lab, hist=hist, want_pred=True)


def kernels_packed():
    return K.sliding_eval(packed, tiles, (H, W), (H, W), FLIPS, labels=lab, hist=hist, want_pred=True)


p_old, h_old, mean_old = parent()
p_new, h_new, mean_new = K.sliding_eval(stack, tiles, (H, W), (H, W), FLIPS, labels=lab, want_pred=True, want_logits=True)
p_pk, h_pk, mean_pk = K.sliding_eval(packed, tiles, (H, W), (H, W), FLIPS, labels=lab, want_pred=True, want_logits=True)
assert torch.equal(p_pk, p_new) and torch.equal(h_pk, h_new) and torch.equal(mean_pk, mean_new), 'the 4-byte and the 16-byte loads disagree'
del p_pk, h_pk, mean_pk
lines.append('one scale, %d tiles of %d x %d from %d x %d logits: max |mean logit delta| new - parent %.3g, class maps differ at %d of %d pixels, |hist delta| %d'
             % (T, th, tw, lg[0].shape[1], lg[0].shape[2], (mean_new - mean_old).abs().max().item(), int((p_new.long() != p_old).sum()), H * W,
                int((h_new - h_old).abs().sum())))
del p_old, h_old, mean_old, p_new, h_new, mean_new
low_b, up_b, acc_b, pix = FLIPS * lg[0].numel() * 4, FLIPS * T * th * tw * 20 * 4, C * H * W * 8, H * W
variants = [('parent: 2 x (resize + sliding_stitch), / 2, argmax, fast_hist', parent), ('new: tile_stack + sliding_eval, class map + hist', new),
            ('  of which sliding_eval on the stack (16-byte loads)', kernels_only), ('  sliding_eval on torch.cat of the tensors (4-byte loads)', kernels_packed)]
# parent: up-sampled tiles written and read, accumulator written, read + written by the second flip, read and written by / 2, read by argmax; int64 class map and labels
# new: the low-res logits read and written by tile_stack and read by the kernel; labels, class map
nbytes = {variants[0][0]: low_b + 2 * up_b + 6 * acc_b + 2 * pix * 8 + pix * 8, variants[1][0]: 3 * low_b + pix * 8 + pix, variants[2][0]: low_b + pix * 8 + pix,
          variants[3][0]: low_b + pix * 8 + pix}
times = timed(variants)
med = {k: statistics.median(v) for k, v in times.items()}
for name, _ in variants:
    v = times[name]
    lines.append('  %-64s %9.1f   %9.1f .. %9.1f   %8.1f MB at the least  %6.3f TB/s' % (name, med[name], min(v), max(v), nbytes[name] / 1e6, nbytes[name] / med[name] / 1e6))
ratio = med[variants[1][0]] / med[variants[0][0]]
lines.append('  new / parent: %.3f -- the new route is %s' % (ratio, 'not slower than the parent\'s' if ratio <= 1 else 'SLOWER than the parent\'s'))

scales = (0.5, 1.0, 2.0)
per_scale = [tile_logits(s, 10 + i) for i, s in enumerate(scales)]
acc = torch.empty((C, H, W), dtype=torch.float64, device='cuda')


def multi(join=harness.tile_stack):
    for i, (l, t, hw, _) in enumerate(per_scale):
        K.sliding_eval(join(l), t, hw, (H, W), FLIPS, acc=acc, acc_add=i > 0)
    return K.sliding_eval_finish(acc, len(scales), labels=lab, hist=hist, want_pred=True)


packed_scales = [torch.cat(l) for l, _, _, _ in per_scale]


def multi_packed():
    for i, (_, t, hw, _) in enumerate(per_scale):
        K.sliding_eval(packed_scales[i], t, hw, (H, W), FLIPS, acc=acc, acc_add=i > 0)
    return K.sliding_eval_finish(acc, len(scales), labels=lab, hist=hist, want_pred=True)


steps = [('new: scales 0.5, 1.0, 2.0: tile_stack + sliding_eval -> accumulator, finish', multi)]
for i, (l, t, hw, thw) in enumerate(per_scale):
    steps.append(('  of which scale %.1f: %d tiles of %d x %d, scaled image %d x %d' % (scales[i], len(t), thw[0], thw[1], hw[0], hw[1]),
                  lambda l=l, t=t, hw=hw: K.sliding_eval(harness.tile_stack(l), t, hw, (H, W), FLIPS, acc=acc, acc_add=False)))
steps.append(('  of which finish', lambda: K.sliding_eval_finish(acc, len(scales), labels=lab, hist=hist, want_pred=True)))
steps.append(('  the three scales and finish on torch.cat of the tensors (4-byte loads)', multi_packed))
times = timed(steps)
for name, _ in steps:
    v = times[name]
    lines.append('  %-64s %9.1f   %9.1f .. %9.1f' % (name, statistics.median(v), min(v), max(v)))
text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
