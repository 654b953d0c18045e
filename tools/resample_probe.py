"""The resampling input edge (K.resample_crop_u8) at the flagship batch: 8 crops of 768 x 768 from 1052 x 1914 uint8 images already in HBM, every image at scale 0.5
(padded rows), 1.0 and 2.0, and at the scales and origins GeometricAugment draws. HIP events around groups of INNER back-to-back calls (the host needs tens of
microseconds to allocate the outputs and enqueue one launch; a single call between two events would time that gap), warm-up first, medians over REPS groups of the
time per call, variants visited round-robin; next to each time the bytes the case must move -- the source footprint of every window (image and mask) plus the two
outputs -- and the bandwidth that makes. Also: what the host spends on the tables and their upload, the register / LDS use of the kernel from the compiler's resource report (hipcc on
the path), and what the host step the feature replaces -- PIL's RandomSizeAndCrop, tools/make_resample_golden.py -- takes for ONE such image on this machine's CPU.

    python tools/resample_probe.py [--reps 30] [--out profiles/resample_probe.txt]
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
ap.add_argument('--inner', type=int, default=8)
ap.add_argument('--out', default=None)
a = ap.parse_args()

N, H, W, CROP = 8, 1052, 1914, (768, 768)
with open(build.STAMP) as f:
    stamp = f.read().strip()[:16]
lines = []


def fixed(scale):
    """Every image at one scale, the origins spread over their range."""
    A = input_edge.GeometricAugment(CROP, scale_min=scale, scale_max=scale, seed=1)
    return A.sample([(H, W)] * N)


def moved_bytes(geo):
    """Source footprint of every window (3 bytes per image pixel inside the bounding box of the bicubic taps, 1 per mask pixel the gather reads) + both outputs."""
    total = 0
    for p in geo.images:
        br, bc, nr, nc = (np.ctypeslib.as_array(t) for t in K.resample_tables(p, (H, W), geo.crop))
        br, bc = br.reshape(geo.crop[0], -1), bc.reshape(geo.crop[1], -1)
        rows, cols = br[br[:, 1] > 0], bc[bc[:, 1] > 0]
        total += 3 * int((rows[:, 0] + rows[:, 1]).max() - rows[:, 0].min()) * int((cols[:, 0] + cols[:, 1]).max() - cols[:, 0].min())
        total += len(np.unique(nr[nr >= 0])) * len(np.unique(nc[nc >= 0]))
    return total + len(geo) * geo.crop[0] * geo.crop[1] * 4


if torch.cuda.is_available():
    lines.append('resample_probe: %s, library build %s, median of %d groups of %d calls (HIP events, us per call), min .. max' % (torch.cuda.get_device_name(0), stamp, a.reps, a.inner))
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    lab = torch.randint(0, 19, (N, H, W), generator=g).to(torch.uint8).cuda()
    sampler = input_edge.GeometricAugment(CROP, seed=0)
    cases = [('scale 0.5 (526 x 957: rows padded)', fixed(0.5)), ('scale 1.0 (a copy)', fixed(1.0)), ('scale 2.0 (2104 x 3828)', fixed(2.0)),
             ('sampled scales', sampler.sample([(H, W)] * N))]
    sampled = ', '.join('%.2f' % s for s in sampler.last['scale'])
    dev = [K.upload_geo(geo, img.device, (H, W)) for _, geo in cases]
    variants = [(name, (lambda d=d: K.resample_crop_u8(img, lab, d))) for (name, _), d in zip(cases, dev)]
    variants.append(('tables + upload: sample(8), 8 x pm_resample_tables, copy', lambda: K.upload_geo(input_edge.GeometricAugment(CROP, seed=2).sample([(H, W)] * N), img.device, (H, W))))
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.inner):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / a.inner)
    lines.append('%d crops of %d x %d from %d x %d uint8 images + masks; sampled scales: %s' % (N, CROP[0], CROP[1], H, W, sampled))
    for k, (name, _) in enumerate(variants):
        v = times[name]
        med = statistics.median(v)
        tail = ''
        if k < len(cases):
            b = moved_bytes(cases[k][1])
            tail = '   %7.2f MB to move = %6.2f TB/s' % (b / 1e6, b / med / 1e6)
        lines.append('  %-60s %9.1f   %9.1f .. %9.1f%s' % (name, med, min(v), max(v), tail))
    gpu_us = {name: statistics.median(times[name]) for name, _ in variants}
else:
    gpu_us = None
    lines.append('resample_probe: no GPU, library build %s: host sections only' % stamp)

# ---- the compiler's resource report of csrc/resample.hip -------------------------------------------------------------------------
hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
if os.path.exists(hipcc):
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'resample.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                       capture_output=True, text=True)
    lines.append('kernel resources (hipcc -Rpass-analysis=kernel-resource-usage; the kernel adds 58 112 bytes of dynamic LDS at launch: two blocks per CU):')
    for ln in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)', ln)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', m.group(2))
            lines.append('  ' + (re.match(r'[a-z0-9_]+?_kernel', cur).group(0) if re.match(r'[a-z0-9_]+?_kernel', cur) else cur))
        else:
            lines[-1] += '  %s %s' % (m.group(1).split(' [')[0], m.group(2))

# ---- the host step, one image ------------------------------------------------------------------------------------------------------
try:
    import make_resample_golden as G
    rng = np.random.default_rng(0)
    one, mask = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 19, size=(H, W)).astype(np.uint8)
    host_ms = {}
    for scale in (0.5, 1.0, 1.25, 2.0):
        geo = G.geometry((H, W), scale, CROP, 'mid')
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            G.pil_crop(one, mask, geo, CROP)
            best = min(best, time.perf_counter() - t0)
        host_ms[scale] = best * 1e3
    lines.append('host step, PIL RandomSizeAndCrop of ONE %d x %d image + mask to %d x %d, best of 3 on this CPU (one thread): %s' %
                 (H, W, CROP[0], CROP[1], ', '.join('scale %.2f %.1f ms' % kv for kv in host_ms.items())))
    if gpu_us:
        per = gpu_us['sampled scales'] / N
        lines.append('  device, per image at sampled scales: %.1f us kernel = 1 / %.0f of the host step at the mean scale 1.25 (%.1f ms)' % (per, host_ms[1.25] * 1e3 / per, host_ms[1.25]))
except ImportError as e:
    lines.append('host step not timed: %s' % e)

text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
