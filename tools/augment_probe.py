"""The augmenting input edge (K.augment_u8 + K.labels_u8_to_i64 with flips) beside the plain conversion it extends (K.image_u8_to_nhwc4 + K.labels_u8_to_i64) at
the flagship batch, 8 x 768 x 768 uint8 images already in HBM: every image with all four colour ops, the widest blur (radius 5) and a flip; and the training scripts'
setting, the jitter on half of the images, a blur of sampled sigma on all, flips on half. HIP events around every single call, warm-up first, medians over REPS calls,
variants visited round-robin. Also: register / LDS use of the kernels from the compiler's resource report (hipcc on the path), and what the host pipeline the
feature replaces -- PIL ColorJitter ops + scipy Gaussian blur, tools/make_augment_golden.py -- takes for ONE 768 x 768 image on this machine's CPU.

    python tools/augment_probe.py [--reps 30] [--out profiles/augment_probe.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from pinthememory_amd import build, input_edge
from pinthememory_amd.hip import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()

N, H, W = 8, 768, 768
with open(build.STAMP) as f:
    stamp = f.read().strip()[:16]
lines = []

if torch.cuda.is_available():
    lines.append('augment_probe: %s, library build %s, median of %d calls (HIP events, us), min .. max' % (torch.cuda.get_device_name(0), stamp, a.reps))
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    lab = torch.randint(0, 19, (N, H, W), generator=g).to(torch.uint8).cuda()
    full = K.aug_params(N)
    for i, p in enumerate(full):
        K.set_aug_image(p, [(i + k) % 4 for k in range(4)], 15, True, 0.3 - 0.1 * i, 0.6 + 0.1 * i, 1.4 - 0.1 * i, 0.7 + 0.1 * i, 1.3)
    half = input_edge.PhotometricAugment(seed=0).sample(N)
    for i, p in enumerate(half):
        p.enabled, p.flip = (15 if i % 2 == 0 else 0), i % 2
    blur_only = K.aug_params(N)
    for p in blur_only:
        K.set_aug_image(p, sigma=1.3)
    d_full, d_half, d_none, d_blur = (K.upload_aug_params(p, img.device) for p in (full, half, K.aug_params(N), blur_only))
    variants = [('plain: image_u8_to_nhwc4', lambda: K.image_u8_to_nhwc4(img)),
                ('plain: labels_u8_to_i64', lambda: K.labels_u8_to_i64(lab)),
                ('augment_u8, no op on any image', lambda: K.augment_u8(img, d_none)),
                ('augment_u8, blur radius 5 only', lambda: K.augment_u8(img, d_blur)),
                ('augment_u8, 4 ops + blur radius 5 + flip on all', lambda: K.augment_u8(img, d_full)),
                ('augment_u8, scripts: jitter on half, blur on all', lambda: K.augment_u8(img, d_half)),
                ('labels_u8_to_i64 with flips', lambda: K.labels_u8_to_i64(lab, d_half)),
                ('parameters: sample(8) + upload (host + copy)', lambda: K.upload_aug_params(input_edge.PhotometricAugment(seed=1).sample(N), img.device))]
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
    lines.append('%d x %d x %d uint8 images, radii of the scripts\' batch: %s' % (N, H, W, [p.radius for p in half]))
    for name, _ in variants:
        v = times[name]
        lines.append('  %-52s %9.1f   %9.1f .. %9.1f' % (name, statistics.median(v), min(v), max(v)))
    med = {k: statistics.median(v) for k, v in times.items()}
    plain = med[variants[0][0]] + med[variants[1][0]]
    for k in (4, 5):
        edge = med[variants[k][0]] + med[variants[6][0]]
        lines.append('  edge (image + labels) %-40s %9.1f us = %.2f x the plain edge (%.1f us)' % (variants[k][0].split(',')[1].strip()[:40], edge, edge / plain, plain))
else:
    lines.append('augment_probe: no GPU, library build %s: host sections only' % stamp)

# ---- the compiler's resource report of csrc/augment.hip ------------------------------------------------------------------------
hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
if os.path.exists(hipcc):
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'augment.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                       capture_output=True, text=True)
    cur = None
    lines.append('kernel resources (hipcc -Rpass-analysis=kernel-resource-usage; the apply kernel adds 68 208 bytes of dynamic LDS at launch):')
    for ln in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)', ln)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', m.group(2))
            cur = re.match(r'[a-z0-9_]+?_kernel', cur).group(0) if re.match(r'[a-z0-9_]+?_kernel', cur) else cur
            lines.append('  ' + cur)
        else:
            lines[-1] += '  %s %s' % (m.group(1).split(' [')[0], m.group(2))

# ---- the host pipeline, one image ------------------------------------------------------------------------------------------------
try:
    import make_augment_golden as G
    one = np.random.default_rng(0).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    t = {}
    for rep in range(3):
        t0 = time.perf_counter()
        x = G.colour_ops(one, (3, 1, 0, 2), 15, (0.8, 1.2, 0.9), 0.05)
        t1 = time.perf_counter()
        G.blur(x, 0.77)
        t2 = time.perf_counter()
        t.setdefault('jitter', []).append(t1 - t0)
        t.setdefault('blur', []).append(t2 - t1)
    lines.append('host pipeline, one %d x %d image, best of 3 on this CPU (one thread): PIL colour jitter %.1f ms + scipy blur (sigma 0.77) %.1f ms' %
                 (H, W, min(t['jitter']) * 1e3, min(t['blur']) * 1e3))
except ImportError as e:
    lines.append('host pipeline not timed: %s' % e)

text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
