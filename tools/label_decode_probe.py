"""The label-decoding input edge at the flagship batch: 8 slabs of 1052 x 1914 cropped to 768 x 768 at the scales GeometricAugment draws.
  (a) the yardstick, K.resample_crop_u8 on pre-decoded one-channel masks, against the fused K.resample_crop_decode_u8 on three-channel colour masks (GTAV's table) and on
      one-channel id masks (Synthia's), and the whole-slab K.labels_decode_u8 of both forms; the fused outputs are first held byte for byte to decode-then-crop;
  (b) the host-to-device copy of the one-channel and the three-channel label slab from pinned memory;
  (c) what the host loops the feature replaces take for ONE mask on this machine's CPU: per table entry three whole-image channel compares, an AND and a masked
      assignment (the colour form, datasets/gtav.py:440-445), and one compare and assignment (the id form, synthia.py:254-257), in numpy, mean of 3.
HIP events around groups of INNER back-to-back calls, warm-up first, variants visited round-robin, medians over REPS groups of the time per call with min .. max.
The tables are the reference's dicts as tests/golden/label_tables.json records them.

    python tools/label_decode_probe.py [--reps 30] [--out profiles/label_decode_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
assert a.reps >= 20, 'at least 20 repetitions'

N, H, W, CROP = 8, 1052, 1914, (768, 768)
with open(build.STAMP) as f:
    stamp = f.read().strip()[:16]
with open(os.path.join(ROOT, 'tests', 'golden', 'label_tables.json')) as f:
    T = json.load(f)
COLORS = {tuple(r[:3]): r[3] for r in T['color2trainId']}
SYNTHIA = {k: v for k, v in T['trainid_to_trainid']}
lines = []


def blocks(rng, values, n):
    """[n, H, W(, 3)] masks of 16 x 16 blocks drawn from `values`"""
    idx = rng.integers(0, len(values), size=(n, (H + 15) // 16, (W + 15) // 16))
    return np.ascontiguousarray(values[idx].repeat(16, 1).repeat(16, 2)[:, :H, :W])


def host_colour_form(mask, table, ignore=255):
    out = np.full(mask.shape[:2], ignore, dtype=np.uint8)
    for k, v in table.items():
        if v != 255 and v != -1:
            key = np.array(k)
            out[(mask == key)[:, :, 0] & (mask == key)[:, :, 1] & (mask == key)[:, :, 2]] = v
    return out


def host_id_form(mask, table):
    out = mask.copy()
    for k, v in table.items():
        out[mask == k] = v
    return out


rng = np.random.default_rng(0)
col_h = blocks(rng, np.array(list(COLORS), dtype=np.uint8), N)                    # [N, H, W, 3]: every table colour, the ignored ones included
ids_h = blocks(rng, np.arange(23, dtype=np.uint8), N)                             # [N, H, W]: Synthia's ids

if torch.cuda.is_available():
    lines.append('label_decode_probe: %s, library build %s, median of %d groups of %d calls (HIP events, us per call), min .. max' %
                 (torch.cuda.get_device_name(0), stamp, a.reps, a.inner))
    dec = input_edge.LabelDecode()
    g, s = dec.add_colors(COLORS), dec.add_ids(SYNTHIA)
    tabs = dec.device_tables('cuda')
    img = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).cuda()
    col_p, ids_p = torch.from_numpy(col_h).pin_memory(), torch.from_numpy(ids_h).pin_memory()
    col, ids = col_p.cuda(), ids_p.cuda()
    sampler = input_edge.GeometricAugment(CROP, seed=0)
    geo = sampler.sample([(H, W)] * N)
    tg, ts = dec.image_table([g] * N, N, 3), dec.image_table([s] * N, N, 1)
    gd_plain, gd_g, gd_s = K.upload_geo(geo, img.device, (H, W)), K.upload_geo(geo, img.device, (H, W), tg), K.upload_geo(geo, img.device, (H, W), ts)
    tg_d, ts_d = K.upload_image_table(tg, img.device), K.upload_image_table(ts, img.device)
    # the results first: fused == decode, then crop; the image crop is the parent's
    pre_g, pre_s = K.labels_decode_u8(col, tabs, tg_d), K.labels_decode_u8(ids, tabs, ts_d)
    want_img, want_g = K.resample_crop_u8(img, pre_g, gd_plain)
    _, want_s = K.resample_crop_u8(img, pre_s, gd_plain)
    got_img, got_g = K.resample_crop_decode_u8(img, col, gd_g, tabs, tg)
    got_img_s, got_s = K.resample_crop_decode_u8(img, ids, gd_s, tabs, ts)
    same = torch.equal(got_g, want_g) and torch.equal(got_s, want_s) and torch.equal(got_img, want_img) and torch.equal(got_img_s, want_img)
    host_ok = np.array_equal(pre_g[0].cpu().numpy(), host_colour_form(col_h[0], COLORS)) and np.array_equal(pre_s[0].cpu().numpy(), host_id_form(ids_h[0], SYNTHIA))
    lines.append('%d crops of %d x %d from %d x %d slabs, sampled scales %s; fused outputs byte-equal to decode-then-crop: %s; device decode of slab 0 equal to the host loops: %s' %
                 (N, CROP[0], CROP[1], H, W, ', '.join('%.2f' % v for v in sampler.last['scale']), same, host_ok))
    assert same and host_ok
    lab_dst1, lab_dst3 = torch.empty_like(ids), torch.empty_like(col)
    variants = [('(a) parent: resample_crop_u8, pre-decoded 1-channel masks', lambda: K.resample_crop_u8(img, pre_g, gd_plain)),
                ('(a) fused: resample_crop_decode_u8, 3-channel colour masks', lambda: K.resample_crop_decode_u8(img, col, gd_g, tabs, tg)),
                ('(a) fused: resample_crop_decode_u8, 1-channel id masks', lambda: K.resample_crop_decode_u8(img, ids, gd_s, tabs, ts)),
                ('    whole slab: labels_decode_u8, 3-channel colour masks', lambda: K.labels_decode_u8(col, tabs, tg_d)),
                ('    whole slab: labels_decode_u8, 1-channel id masks', lambda: K.labels_decode_u8(ids, tabs, ts_d)),
                ('(b) host-to-device copy, 1-channel label slab (%.1f MB, pinned)' % (ids_p.numel() / 1e6), lambda: lab_dst1.copy_(ids_p, non_blocking=True)),
                ('(b) host-to-device copy, 3-channel label slab (%.1f MB, pinned)' % (col_p.numel() / 1e6), lambda: lab_dst3.copy_(col_p, non_blocking=True))]
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fn in variants:
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            for _ in range(a.inner):
                fn()
            e.record()
            e.synchronize()
            times[name].append(b.elapsed_time(e) * 1e3 / a.inner)
    med = {}
    for name, _ in variants:
        v = times[name]
        med[name] = statistics.median(v)
        lines.append('  %-66s %9.1f   %9.1f .. %9.1f' % (name, med[name], min(v), max(v)))
    names = [n for n, _ in variants]
    extra = N * CROP[0] * CROP[1] * 2
    lines.append('  fused colour - parent: %+.1f us per batch (the parent\'s own min .. max spans %.1f us); the algorithm adds 2 bytes read per output label pixel = %.1f MB per batch' %
                 (med[names[1]] - med[names[0]], max(times[names[0]]) - min(times[names[0]]), extra / 1e6))
    lines.append('  3-channel copy - 1-channel copy: %+.1f us per batch = %.1f us per image' % (med[names[6]] - med[names[5]], (med[names[6]] - med[names[5]]) / N))
else:
    med = None
    lines.append('label_decode_probe: no GPU, library build %s: host section only' % stamp)

# ---- (c) the host loops, one mask ------------------------------------------------------------------------------------------------------
host_ms = {}
for name, fn, args in (('colour form (GTAV, %d entries, %d kept)' % (len(COLORS), sum(1 for v in COLORS.values() if v not in (255, -1))), host_colour_form, (col_h[0], COLORS)),
                       ('id form (Synthia, %d entries)' % len(SYNTHIA), host_id_form, (ids_h[0], SYNTHIA))):
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn(*args)
        t.append(time.perf_counter() - t0)
    host_ms[name] = sum(t) / 3 * 1e3
    lines.append('(c) host, numpy, ONE %d x %d mask, mean of 3 on this CPU (%d torch threads; numpy runs one): %s %.1f ms' % (H, W, torch.get_num_threads(), name, host_ms[name]))
if med:
    per = (med[names[1]] - med[names[0]] + med[names[6]] - med[names[5]]) / N
    lines.append('  device, per image: fused decode (over the parent) + the two extra mask channels over the bus = %.1f us, against %.0f ms of the colour form on the host' %
                 (per, list(host_ms.values())[0]))

text = '\n'.join(lines)
print(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text + '\n')
