"""GPU: the evaluation image dumps (csrc/eval_dump.hip) at the size of a Cityscapes frame -- one 1024 x 2048 class map, its uint8 image and int64 labels, all four
outputs -- against the same four images made otherwise:
  (new)    K.eval_dump, one launch;
  (stock)  torch ops on the same device: palette gather, float blend, torch.where, table gather;
  (host)   where Pillow is importable: the reference's sequence on the host (eval.py:674-692): palette image, two RGBA conversions, Image.blend, invert, lighter and
           the loop of np.where passes over id_to_trainid. Host time, a few repeats; no transfer is counted for it.
(new) and (stock): HIP events around groups of GROUP calls, warm-up first, the two visited alternately so that drift hits both alike; per call: the median over the
groups (GROUPS x GROUP timed calls each, at least 50), min .. max. GB/s are ALGORITHMIC bytes over that time: what the pass has to move (per pixel 1 byte of class map,
3 of image, 8 of labels in, 10 out), the same figure for both whatever they really move. The 46 MB of one frame stay inside the 256 MiB Infinity Cache from call to
call, so the figure is no HBM rate. Before anything is timed the results are compared and reported.

    python tools/eval_dump_probe.py [--out profiles/eval_dump_probe.txt] [--groups 50] [--group 4]
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W = 1024, 2048
OUTPUTS = ('color', 'compose', 'diff', 'ids')
ALPHA = 0.5

ap = argparse.ArgumentParser()
ap.add_argument('--groups', type=int, default=50)
ap.add_argument('--group', type=int, default=4)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--host-repeats', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
lines = []


def say(text):
    print(text)
    lines.append(text)


def timed(variants, nbytes):
    import torch
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
    med = {}
    for nm, _ in variants:
        v = times[nm]
        med[nm] = statistics.median(v)
        say('  %-58s %10.1f us   %10.1f .. %10.1f   %8.1f GB/s' % (nm, med[nm], min(v), max(v), nbytes / med[nm] / 1e3))
    return med


def host_reference(pred, image, gt, palette, id_to_trainid):
    """eval.py:674-692 on numpy arrays, as written there, up to the point where the files would be saved."""
    import numpy as np
    from PIL import Image, ImageChops, ImageOps
    prediction = pred.astype(np.int64)
    img = Image.fromarray(image)
    colorized = Image.fromarray(prediction.astype(np.uint8)).convert('P')
    colorized.putpalette(palette)
    blend = Image.blend(img.convert('RGBA'), colorized.convert('RGBA'), ALPHA)
    diff = (prediction != gt)
    diff[gt == 255] = 0
    lighter = ImageChops.lighter(blend, ImageOps.invert(Image.fromarray(diff.astype('uint8') * 255)).convert('RGBA'))
    label_out = np.zeros_like(prediction)
    for label_id, train_id in id_to_trainid.items():
        label_out[np.where(prediction == train_id)] = label_id
    return dict(color=np.asarray(colorized.convert('RGB')), compose=np.asarray(blend)[..., :3], diff=np.asarray(lighter)[..., :3], ids=label_out.astype(np.uint8))


def main():
    import torch
    from pinthememory_amd import build
    from pinthememory_amd.hip import kernels as K
    import eval_dump_cases as EC
    if not torch.cuda.is_available():
        sys.exit('eval_dump_probe: needs a GPU')
    build.build()
    with open(build.STAMP) as f:
        stamp = f.read().strip()[:16]
    calls = a.groups * a.group
    assert calls >= 50, 'at least 50 timed calls'
    say('eval_dump_probe: %s, library build %s; device times per call: median of %d groups of %d calls (%d timed calls, HIP events, us), min .. max; GB/s of '
        'algorithmic bytes' % (torch.cuda.get_device_name(0), stamp, a.groups, a.group, calls))
    g = torch.Generator(device='cuda').manual_seed(3)
    pred = torch.randint(0, 19, (H, W), generator=g, device='cuda').to(torch.uint8)
    gt = torch.where(torch.rand((H, W), generator=g, device='cuda') < 0.5, pred.long(), torch.randint(0, 19, (H, W), generator=g, device='cuda'))
    gt[torch.rand((H, W), generator=g, device='cuda') < 0.2] = 255
    image = torch.randint(0, 256, (H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
    palette = torch.from_numpy(EC.PALETTE).cuda()
    table = K.trainid_table(EC.ID_TO_TRAINID).cuda()

    def new():
        return K.eval_dump(pred, palette=palette, image=image, labels=gt, id_table=table, alpha=ALPHA, want=OUTPUTS)

    def stock():
        idx = pred.long()
        color = palette[idx]
        im = image.float()
        compose = (im + ALPHA * (color.float() - im)).to(torch.uint8)
        differs = (gt != 255) & (gt != idx)
        return dict(color=color, compose=compose, diff=torch.where(differs.unsqueeze(-1), compose, torch.full_like(compose, 255)), ids=table[idx])

    got, old = new(), stock()
    unequal = {k: int((got[k] != old[k]).sum()) for k in OUTPUTS}
    nbytes = H * W * (1 + 3 + 8 + 10)
    say('eval_dump: class map %d x %d uint8, image uint8, labels int64 -> color + compose + diff + ids, algorithmic bytes %.2f MB' % (H, W, nbytes / 1e6))
    med = timed([('(new) eval_dump, one launch', new), ('(stock) gather + float blend + where + gather in torch', stock)], nbytes)
    ratio = med['(new) eval_dump, one launch'] / med['(stock) gather + float blend + where + gather in torch']
    say('  (new) / (stock): %.4f%s' % (ratio, '' if ratio < 1 else '   -- the kernel is NOT faster here'))
    say('  bytes differing between (new) and (stock): %s' % ', '.join('%s %d' % (k, unequal[k]) for k in OUTPUTS))
    try:
        import PIL
        np_in = (pred.cpu().numpy(), image.cpu().numpy(), gt.cpu().numpy(), EC.PALETTE.reshape(-1).tolist(), EC.ID_TO_TRAINID)
        ref = host_reference(*np_in)
        same = all(bool((got[k].cpu().numpy() == ref[k]).all()) for k in OUTPUTS)
        host = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            host_reference(*np_in)
            host.append((time.perf_counter() - t0) * 1e6)
        say('  %-58s %10.1f us   %10.1f .. %10.1f   (host clock, %d repeats; Pillow %s)' % ('(host) the reference\'s PIL / numpy sequence', statistics.median(host), min(host),
                                                                                      max(host), a.host_repeats, PIL.__version__))
        say('  (new) equals (host) on every byte of the four images: %s' % same)
    except ImportError:
        say('  (host) Pillow is not importable here: not measured')
    try:
        with open(os.path.join(ROOT, 'profiles', 'ablation_probe.txt')) as f:
            m = re.search(r'\(new\) mem_actmap.*?([0-9.]+) GB/s', f.read())
        say('  for comparison, pm_mem_actmap in profiles/ablation_probe.txt: %s GB/s of its algorithmic bytes (125.61 MB per call)' % (m.group(1) if m else 'no figure found'))
    except OSError:
        say('  profiles/ablation_probe.txt is not here: no figure of pm_mem_actmap to compare with')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
