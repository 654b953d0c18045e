"""GPU: the ablation sweep's kernels (csrc/ablation.hip) at the shape of the reference's ablation scripts -- one 1280 x 720 image, features [256, 45, 80] in fp32 and
bf16, memory scores [19, 45, 80] -- against the stock formulation on the same device:
  sums    (new)   K.label_splat once + K.class_sums twice (features and refined features share the splat);
          (stock) tsnelib.py:48-65 twice: F.normalize -> F.interpolate(bilinear, align_corners=True) to 720 x 1280 -> one-hot of the labels (int64 -> float) -> matmul;
  actmap  (new)   K.mem_actmap, bytes + rgb + blend for 19 slots in one launch;
          (stock) ablation.py:375-399 in torch: F.interpolate -> per-pixel min / max over the slots -> divide -> clip -> * 255 -> uint8 -> palette gather -> blend.
HIP events around groups of GROUP calls, warm-up first, the variants visited alternately so that drift hits both alike; per call: the median over the groups,
min .. max. GB/s are ALGORITHMIC bytes over that time: what the fused form has to move (sums: the int64 labels once, both feature maps once, splat and sums; actmap: the
scores, the image and the three byte outputs) -- the same figure for both variants whatever they really move. Before anything is timed the variants' results are
compared and reported. Every case runs in a child process of its own under its own time limit; after a child that did not end cleanly nothing more is started.

    python tools/ablation_probe.py [--out profiles/ablation_probe.txt] [--groups 8] [--group 3] [--limit 240]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, h, w, C, M, CLASSES = 720, 1280, 45, 80, 256, 19, 19
CASES = ['sums_f32', 'sums_bf16', 'actmap']

ap = argparse.ArgumentParser()
ap.add_argument('--groups', type=int, default=8)
ap.add_argument('--group', type=int, default=3)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--limit', type=int, default=240, help='seconds a child may take')
ap.add_argument('--case', default=None, choices=CASES, help='(child) which case to time')
ap.add_argument('--out', default=None)
a = ap.parse_args()


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
    med = []
    for nm, _ in variants:
        v = times[nm]
        med.append(statistics.median(v))
        print('  %-58s %10.1f us   %10.1f .. %10.1f   %8.1f GB/s' % (nm, med[-1], min(v), max(v), nbytes / med[-1] / 1e3))
    print('  (new) / (stock): %.4f%s' % (med[0] / med[1], '' if med[0] < med[1] else '   -- the fused path is NOT faster here'))


def sums_case(dt):
    import torch
    import torch.nn.functional as F
    from pinthememory_amd.hip import kernels as K
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    g = torch.Generator(device='cuda').manual_seed(1)
    feats = [torch.randn((1, h, w, C), generator=g, device='cuda').to(dtype).permute(0, 3, 1, 2) for _ in range(2)]      # logical NCHW, channels-last memory
    lab = torch.randint(0, CLASSES, (1, H, W), generator=g, device='cuda')
    lab[torch.rand((1, H, W), generator=g, device='cuda') < 0.1] = 255

    def new():
        splat, counts = K.label_splat(lab, (h, w), CLASSES)
        return [K.class_sums(f, splat) for f in feats], counts

    def stock():
        out = []
        for f in feats:      # tsnelib.py:50-65, as written: the one-hot is rebuilt by every call
            fn = F.normalize(f.clone(), dim=1)
            gt = lab.clone()
            gt[gt == 255] = CLASSES
            oh = F.one_hot(gt, num_classes=CLASSES + 1).view(1, -1, CLASSES + 1)
            den = oh.sum(1)
            up = F.interpolate(fn, [H, W], mode='bilinear', align_corners=True).reshape(1, C, -1)
            out.append(torch.matmul(up, oh.type(up.dtype)).transpose(1, 2))
        return out, den

    (s_new, c_new), (s_old, c_old) = new(), stock()
    assert torch.equal(c_new, c_old), 'counts differ'
    cnt = c_new.clamp(min=1).double().unsqueeze(-1)
    diff = max(float(((p.double() - q.double()) / cnt).abs().max()) for p, q in zip(s_new, s_old))
    # fp64 on the device for both class-mean sets: how far each formulation is from it
    truth = [torch.matmul(F.interpolate(F.normalize(f.double(), dim=1), [H, W], mode='bilinear', align_corners=True).reshape(1, C, -1),
                          F.one_hot(torch.where(lab == 255, CLASSES, lab), CLASSES + 1).view(1, -1, CLASSES + 1).double()).transpose(1, 2) for f in feats]
    e_new = max(float(((p.double() - t) / cnt).abs().max()) for p, t in zip(s_new, truth))
    e_old = max(float(((q.double() - t) / cnt).abs().max()) for q, t in zip(s_old, truth))
    assert e_new < (1e-5 if dt == 'f32' else 1e-5), (e_new, e_old)
    del truth, s_old
    nbytes = lab.numel() * 8 + 2 * feats[0].numel() * feats[0].element_size() + h * w * (CLASSES + 1) * 4 * 3 + 2 * (CLASSES + 1) * C * 4
    print('sums %s: labels %d x %d int64, two feature maps [%d, %d, %d] %s, algorithmic bytes %.2f MB' % (dt, H, W, C, h, w, dt, nbytes / 1e6))
    timed([('(new) label_splat + 2 x class_sums', new), ('(stock) 2 x normalize + interpolate + one_hot + matmul', stock)], nbytes)
    print('  largest class-mean difference (new) against (stock): %.2e; against fp64 on the device: (new) %.2e, (stock) %.2e' % (diff, e_new, e_old))


def actmap_case():
    import torch
    import torch.nn.functional as F
    from pinthememory_amd.hip import kernels as K
    g = torch.Generator(device='cuda').manual_seed(2)
    sc = torch.softmax(3 * torch.randn((1, h, w, M), generator=g, device='cuda'), dim=-1)
    palette = torch.randint(0, 256, (256, 3), generator=g, device='cuda', dtype=torch.uint8)
    image = torch.randint(0, 256, (1, H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
    slots = list(range(M))
    alpha = 0.65

    def new():
        return K.mem_actmap(sc, (1, h, w), (H, W), slots, palette=palette, image=image, alpha=alpha, want=('bytes', 'rgb', 'blend'))

    def stock():
        up = F.interpolate(sc.permute(0, 3, 1, 2), [H, W], mode='bilinear', align_corners=True)
        up = up - up.min(1, keepdim=True)[0]
        up = up / up.max(1, keepdim=True)[0]
        byts = (up.clamp(0, 1) * 255).to(torch.uint8)
        rgb = palette[byts.long()]
        im = image.unsqueeze(1).float()
        blend = (im + alpha * (rgb.float() - im)).to(torch.uint8)
        return dict(bytes=byts, rgb=rgb, blend=blend)

    got, old = new(), stock()
    d = (got['bytes'].int() - old['bytes'].int()).abs()
    db = (got['blend'].int() - old['blend'].int()).abs()
    assert int(d.max()) <= 1, int(d.max())
    share, bshare = float((d != 0).double().mean()), float((db != 0).double().mean())
    del old, d, db
    nbytes = sc.numel() * 4 + image.numel() + M * H * W * 7
    print('actmap: scores [%d, %d, %d] fp32 -> %d slots at %d x %d, bytes + rgb + blend, algorithmic bytes %.2f MB' % (M, h, w, M, H, W, nbytes / 1e6))
    timed([('(new) mem_actmap, one launch', new), ('(stock) interpolate + min / max + clip + byte + gather + blend', stock)], nbytes)
    print('  bytes differing between (new) and (stock): %.4f %% (by one level, none by more); blend bytes differing: %.4f %%' % (100 * share, 100 * bshare))


def main():
    import torch
    from pinthememory_amd import build
    if not torch.cuda.is_available():
        sys.exit('ablation_probe: needs a GPU')
    build.build()
    with open(build.STAMP) as f:
        stamp = f.read().strip()[:16]
    lines = ['ablation_probe: %s, library build %s; device times per call: median of %d groups of %d calls (HIP events, us), min .. max; GB/s of algorithmic bytes'
             % (torch.cuda.get_device_name(0), stamp, a.groups, a.group)]
    common = ['--groups', str(a.groups), '--group', str(a.group), '--warmup', str(a.warmup)]
    for case in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', case] + common, capture_output=True, text=True, timeout=a.limit)
            rc, out, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, (e.stdout or b'').decode() if isinstance(e.stdout, bytes) else (e.stdout or ''), 'time limit of %d s' % a.limit
        lines += [ln for ln in out.splitlines() if ln.startswith(('sums', 'actmap', '  '))]
        if rc != 0:
            lines.append('child %s ended with status %d: %s -- nothing more was started' % (case, rc, ' | '.join(err.strip().splitlines()[-3:])))
            break
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0 if not lines[-1].startswith('child') else 1


if __name__ == '__main__':
    if a.case is None:
        sys.exit(main())
    elif a.case == 'actmap':
        actmap_case()
    else:
        sums_case(a.case.split('_')[1])
