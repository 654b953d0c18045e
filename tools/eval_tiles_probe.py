"""GPU: everything in front of the network of a sliding-window evaluation (eval.py --inference_mode sliding) of one 1024 x 2048 uint8 image at crop 768 with both
flips, at scales 0.5, 1.0 and 2.0, from the decoded image to the stack of normalised crops the network is fed:
  (a) parent route: PIL's Image.resize(BILINEAR) on the host and the upload of the scaled bytes (host time, reported apart; none at scale 1.0), then on the device
      K.image_u8_to_nhwc4 of the whole scaled image, torch.flip of it, the slices and one torch.stack per flip (what harness.evaluate_sliding runs by default);
  (b) new route:    one K.eval_tiles_u8 launch from the source image on the device through a warm K.EvalTilePlan (device_tiles=True); and the host time of a cold plan
      (the two coefficient tables, the tile table, one pinned block, one copy).
HIP events around groups of GROUP calls, warm-up first, the routes visited alternately so that drift hits both alike; per call: the median over the groups, min .. max.
The two routes' crops are compared bit for bit on the same image before anything is timed (PIL must be importable for that and for the host times).

    python tools/eval_tiles_probe.py [--groups 10] [--group 3] [--out profiles/eval_tiles_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pinthememory_amd import build, harness
from pinthememory_amd.hip import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument('--groups', type=int, default=10)
ap.add_argument('--group', type=int, default=3)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--hw', type=int, nargs=2, default=(1024, 2048))
ap.add_argument('--crop', type=int, default=768)
ap.add_argument('--scales', type=float, nargs='+', default=(0.5, 1.0, 2.0))
ap.add_argument('--out', default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('eval_tiles_probe: needs a GPU')

H, W = a.hw
FLIPS, OVERLAP = 2, 1.0 / 3
dev = torch.device('cuda', torch.cuda.current_device())
img = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
img_dev = img.to(dev)


def host_ms(fn, n=3):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), r


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
lines = ['eval_tiles_probe: %s, library build %s, %d x %d uint8 image, crop %d, both flips; device times per call: median of %d groups of %d calls (HIP events, us), '
         'min .. max; host times: median of 3 (ms)' % (torch.cuda.get_device_name(0), stamp, H, W, a.crop, a.groups, a.group)]
for s in a.scales:
    K.clear_eval_tile_plans()
    cold_ms, plan = host_ms(lambda: K.EvalTilePlan(H, W, s, a.crop, OVERLAP, dev))
    tiles, T = plan.tiles, len(plan.tiles)
    if s == 1.0:
        resize_ms, scaled = 0.0, img
        upload_ms, scaled_dev = 0.0, img_dev
    else:
        resize_ms, scaled = host_ms(lambda: harness._scaled_u8(img, s))
        upload_ms, scaled_dev = host_ms(lambda: scaled.to(dev))
    assert tuple(scaled.shape[:2]) == (plan.Hs, plan.Ws)

    def parent():
        x = K.image_u8_to_nhwc4(scaled_dev[None].contiguous())[0]
        return [torch.stack([src[y1:y2, x1:x2] for (x1, y1, x2, y2) in tiles]) for src in (x, torch.flip(x, dims=[1]))]

    def new():
        return K.eval_tiles_u8(img_dev, plan, FLIPS)

    old, got = parent(), new()
    assert torch.equal(got[:T], old[0]) and torch.equal(got[T:], old[1]), 'the two routes disagree at scale %g' % s
    del old, got
    out_b, px = FLIPS * T * plan.th * plan.tw * 16, plan.Hs * plan.Ws
    # (a): scaled bytes read, fp32 image written; read and written by the flip; both read by the slices, the stacks written. (b): source bytes read, the stacks written
    bytes_a, bytes_b = px * 3 + px * 16 + 2 * px * 16 + 2 * out_b, H * W * 3 + out_b
    va, vb = '(a) image_u8_to_nhwc4 + flip + slices + stack', '(b) eval_tiles_u8, warm plan'
    times = timed([(va, parent), (vb, new)])
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append('scale %.2f: scaled image %d x %d, %d tiles of %d x %d, crops %.1f MB' % (s, plan.Hs, plan.Ws, T, plan.th, plan.tw, out_b / 1e6))
    for name, nb in ((va, bytes_a), (vb, bytes_b)):
        v = times[name]
        lines.append('  %-48s %9.1f   %9.1f .. %9.1f   %8.1f MB at the least  %6.3f TB/s' % (name, med[name], min(v), max(v), nb / 1e6, nb / med[name] / 1e6))
    lines.append('  (b) / (a): %.3f; (a) spread %.1f us' % (med[vb] / med[va], max(times[va]) - min(times[va])))
    lines.append('  host, (a) only: PIL resize %.2f ms, upload of the scaled bytes %.2f ms (%.1f MB); host, (b) with a cold plan: tables + pinned block + copy %.2f ms (%.2f MB)'
                 % (resize_ms, upload_ms, px * 3 / 1e6 if s != 1.0 else 0.0, cold_ms, plan.buf.numel() / 1e6))
    del plan, scaled_dev
    torch.cuda.empty_cache()
text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
