"""Inputs and CPU references shared by tests/test_ablation_cpu.py and tests/test_ablation.py: torch restatements of tsnelib.py:48-74 (the class sums) and of
ablation.py:309-315,375-399 (the memory activation map), evaluated in the precision the caller asks for. The reference's own files need .cuda() and cv2 and cannot be
imported; nothing here reads them."""
import torch
import torch.nn.functional as F

CLASSES = 19
ULP = 2.0 ** -23
ACT_K = 32.0      # the activation rule: |act - act64| <= ACT_K * 2^-23 / range_p

# (n, C, h, w, H, W)
SUM_SHAPES = [(1, 16, 5, 7, 33, 50), (2, 256, 12, 20, 90, 157), (1, 8, 1, 1, 9, 4), (1, 8, 3, 1, 3, 6)]
# (n, m, h, w, H, W)
ACT_SHAPES = [(1, 19, 5, 7, 33, 50), (1, 19, 9, 13, 67, 131), (2, 19, 12, 20, 90, 157), (1, 7, 3, 2, 17, 9)]
ABSENT = 7        # the class no 'mixed' label image holds


def gen(seed):
    return torch.Generator().manual_seed(seed)


def features(n, C, h, w, seed=11):
    """fp32 [n, C, h, w] (contiguous NCHW values; the tests lay them out as they need)"""
    return torch.randn((n, C, h, w), generator=gen(seed))


def labels(n, H, W, kind='mixed', seed=23):
    """int64 [n, H, W]. mixed: uniform over the classes without ABSENT, 10 % set to 255, a few values of 19..254 (skipped by the kernels); every image differs.
    all255 / single: what the names say."""
    if kind == 'all255':
        return torch.full((n, H, W), 255, dtype=torch.int64)
    if kind == 'single':
        return torch.full((n, H, W), 4, dtype=torch.int64)
    g = gen(seed)
    lab = torch.randint(0, CLASSES - 1, (n, H, W), generator=g)
    lab = lab + (lab >= ABSENT).long()
    lab[torch.rand((n, H, W), generator=g) < 0.10] = 255
    odd = torch.rand((n, H, W), generator=g) < 0.02
    lab[odd] = torch.randint(CLASSES, 255, (int(odd.sum()),), generator=g)
    return lab


def one_hot(lab, dtype):
    """[n, H W, CLASSES + 1]: 255 -> row CLASSES (tsnelib.py:54), values of 19..254 in no row (F.one_hot would raise)"""
    row = torch.where(lab == 255, torch.full_like(lab, CLASSES), torch.where((lab >= 0) & (lab < CLASSES), lab, torch.full_like(lab, -1)))      # a raw 19 is skipped too
    return (row.reshape(lab.shape[0], -1).unsqueeze(-1) == torch.arange(CLASSES + 1)).to(dtype)


def class_sums_ref(feat, lab, dtype):
    """tsnelib.py:51-65 per image in `dtype`: normalise -> up-sample -> matmul with the one-hot. -> (sums [n, CLASSES + 1, C], counts int64 [n, CLASSES + 1])"""
    n, C = feat.shape[:2]
    oh = one_hot(lab, dtype)
    up = F.interpolate(F.normalize(feat.to(dtype), dim=1), list(lab.shape[1:]), mode='bilinear', align_corners=True)
    return torch.matmul(up.reshape(n, C, -1), oh).transpose(1, 2).contiguous(), oh.sum(1).long()


def means(sums, counts):
    """-> (means of the present classes [rows, C], presence mask [n, CLASSES + 1])"""
    present = counts > 0
    return (sums.double() / counts.clamp(min=1).double().unsqueeze(-1))[present], present


def scores(n, m, h, w, seed=31, constant_block=False):
    """softmax(3 randn) over the slots, fp32 [n, h, w, m]; constant_block: the top-left 2 x 2 low-res pixels hold 1 / m in every slot (hi == lo where only they enter)"""
    s = torch.softmax(3.0 * torch.randn((n, h, w, m), generator=gen(seed)), dim=-1)
    if constant_block:
        s[:, :2, :2, :] = 1.0 / m
    return s


def act_ref(sc, H, W, dtype):
    """ablation.py:375-378 in `dtype`: up-sample, per-pixel min-max over the slots. -> (a [n, m, H, W] (0 where hi == lo), range [n, H, W])"""
    up = F.interpolate(sc.permute(0, 3, 1, 2).to(dtype), [H, W], mode='bilinear', align_corners=True)
    lo, hi = up.min(1, keepdim=True)[0], up.max(1, keepdim=True)[0]
    rng = hi - lo
    a = torch.where(rng > 0, (up - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(up))
    return a, rng[:, 0]


def act_bytes(a):
    """np.uint8(np.clip(a, 0, 1) * 255) in a's own precision"""
    return (a.clamp(0, 1) * 255).to(torch.uint8)


def screen(a64, rng64):
    """-> (band half-width of the float map per pixel [n, 1, H, W], bytes whose fp64 value * 255 lies inside the band around an integer [n, m, H, W])"""
    tol = (ACT_K * ULP / rng64.clamp(min=1e-300)).unsqueeze(1)
    x = a64 * 255
    return tol, (x - x.round()).abs() < 255 * tol


def check_act_rule(act, byts, a64, rng64):
    """The activation rule of the issue for one float map / byte map against the fp64 reference -> dict of figures; raises where the rule is broken.
    act may be None (a byte map alone)."""
    tol, band = screen(a64, rng64)
    fig = {}
    if act is not None:
        err = ((act.double() - a64).abs() / (ULP / rng64.clamp(min=1e-300)).unsqueeze(1))
        fig['act_err_units'] = float(err.max())
        assert fig['act_err_units'] <= ACT_K, fig
    b64 = act_bytes(a64).int()
    d = (byts.int() - b64).abs()
    # the share counts the bytes the rule leaves open: a pixel's arg-min / arg-max slot sits ON an integer (0 and 255 exactly) and has the exact rule below instead
    fig['band_share'] = float((band & (a64 > 0) & (a64 < 1)).double().mean())
    fig['bytes_differing'] = int((d != 0).sum())
    assert int(d.max()) <= 1, fig
    assert not bool(((d != 0) & ~band).any()), fig
    live = (rng64 > 0).unsqueeze(1)
    amin, amax = a64.argmin(1, keepdim=True), a64.argmax(1, keepdim=True)
    assert bool((byts.gather(1, amin)[live] == 0).all()) and bool((byts.gather(1, amax)[live] == 255).all()), fig
    return fig
