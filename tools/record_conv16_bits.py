"""Records the output bits of the bf16 tier's LDS-DMA convolution kernels (csrc/conv16.hip, conv16w.hip, wgrad16.hip) into tests/golden/conv16_bits.json;
tests/test_conv16_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_conv16_bits.py [--out FILE]

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. Every kernel is deterministic
(the split-K reduce has a fixed order), so a digest (sha256 of the output's bytes) either matches or the change altered a bit.

The calls go through pm_conv_fwd / pm_conv_bwd_data / pm_conv_bwd_weight (hip/kernels.py) on the bf16 tier under pm_set_conv16 routes 2 (narrow tiles), 3 (persistent
ring), 8 (ring, one block per tile) and 7 (256 x 256), with pm_set_wgrad16(1). Inputs come from CPU generators with fixed seeds. Beside the digests the in-library
profile's record of each call is kept ('reach': tile form, K-split), and check_reach holds it to the form the case is named for -- the planner rules the cases were
laid out by are proven by that, not assumed."""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv16_bits.json')

ROUTES = {2: 'narrow', 3: 'persistent', 8: 'ring', 7: '256x256'}


def fwd(name, route, x, cout, k=1, pad=0, dil=1, ep='plain', padded=False, expect=None):
    """x = (n, cin, h, w). ep: plain | affine (scale / shift + residual + ReLU) | stats (bn_partials) | logits (fp32 out + bias). padded: through a K.new buffer."""
    return dict(name=name, kind='fwd', route=route, x=x, cout=cout, k=k, pad=pad, dil=dil, ep=ep, padded=padded, expect=expect)


def dgrad(name, route, x, cout, k=3, stride=1, pad=1, dil=1, expect=None):
    return dict(name=name, kind='dgrad', route=route, x=x, cout=cout, k=k, stride=stride, pad=pad, dil=dil, expect=expect)


def wgrad(name, case, expect):
    n, cin, h, w, cout, k, s, p, d = case
    return dict(name=name, kind='wgrad', route=2, x=(n, cin, h, w), cout=cout, k=k, stride=s, pad=p, dil=d, expect=expect)


def T(bm, bn, nst, ks=1):      # a narrow tile form: LDS stages, K-splits
    return dict(mode=4, bm=bm, bn=bn, km=0, nst=nst, ksplit=ks)


def W(route, bm, bn, ks=1):    # a wide form; km = 1: the persistent kernel
    return dict(mode=5, bm=bm, bn=bn, km=1 if route == 3 else 0, nst=3, ksplit=ks)


def G(bm, bn):                 # the weight gradient's ring
    return dict(mode=2, bm=bm, bn=bn, km=2, nst=3)


# pm_conv_fwd hands the LDS-DMA kernels calls of at least 256 output pixels (C16_MIN_M, csrc/conv_igemm.hip): the small shapes sit just above it
S = (2, 64, 13, 11)            # 286 output pixels: five 64-row tiles, the last ragged
CASES = [
    # ---- narrow, 64-row tiles ----
    fwd('n64-1x1', 2, S, 64, expect=T(64, 64, 1)),                                      # one stage
    fwd('n64-1x1-affine', 2, S, 64, ep='affine', expect=T(64, 64, 1)),
    fwd('n64-1x1-stats', 2, S, 64, ep='stats', expect=T(64, 64, 1)),
    fwd('n64-3x3', 2, S, 64, k=3, pad=1, expect=T(64, 64, 2)),                          # two stages, 9 K-steps, no split
    fwd('n64-3x3-affine', 2, S, 64, k=3, pad=1, ep='affine', expect=T(64, 64, 2)),
    fwd('n64-3x3-stats', 2, S, 64, k=3, pad=1, ep='stats', expect=T(64, 64, 2)),
    fwd('n64-3x3-c128', 2, S, 128, k=3, pad=1, expect=T(64, 128, 2)),
    fwd('n64-3x3-c128-stats', 2, S, 128, k=3, pad=1, ep='stats', expect=T(64, 128, 2)),
    fwd('n64-3x3-c200', 2, S, 200, k=3, pad=1, ep='affine', expect=T(64, 128, 2)),       # ragged second column tile
    fwd('n64-1x1-c19-logits', 2, S, 19, ep='logits', expect=T(64, 64, 1)),
    fwd('n64-3x3-cin48', 2, (2, 48, 13, 11), 64, k=3, pad=1, padded=True, expect=T(64, 64, 2)),
    fwd('n64-1x1-cin304', 2, (2, 304, 13, 11), 64, padded=True, expect=T(64, 64, 2)),
    # ---- narrow, 128-row tiles: 512 tiles of 128 rows ----
    fwd('n128x64-1stage', 2, (1, 64, 255, 257), 64, expect=T(128, 64, 1)),              # last tile ragged by one row
    fwd('n128x64-2stage', 2, (1, 128, 255, 257), 64, ep='affine', expect=T(128, 64, 2)),
    fwd('n128x128-1stage', 2, (1, 64, 127, 129), 512, ep='affine', expect=T(128, 128, 1)),
    fwd('n128x128-2stage', 2, (1, 128, 127, 129), 512, expect=T(128, 128, 2)),
    fwd('n128x128-2stage-stats', 2, (1, 128, 127, 129), 512, ep='stats', expect=T(128, 128, 2)),
]
# ---- split-K and invisible filter rows, every route: 18 K-steps in 2 splits on the narrow tiles (the second starts mid-tap); 27 K-steps in 3 splits of which the first
# and the last see only invisible taps (units of ZERO K-steps: a zero slab); the same over two images (a tile spans both: no skipping) ----
for r in (2, 3, 8, 7):
    wide = (lambda ks: W(r, 256, 256, ks)) if r == 7 else (lambda ks: W(r, 256, 128, ks))
    CASES += [
        fwd('split-midtap/%s' % ROUTES[r], r, (1, 128, 20, 15), 64, k=3, pad=1, expect=T(64, 64, 2, 2) if r == 2 else wide(9)),
        fwd('split-invisible/%s' % ROUTES[r], r, (1, 192, 12, 24), 128, k=3, pad=12, dil=12, expect=T(64, 128, 2, 3) if r == 2 else wide(None)),
        fwd('split-two-images/%s' % ROUTES[r], r, (2, 192, 12, 12), 128, k=3, pad=12, dil=12, expect=T(64, 128, 2, 3) if r == 2 else wide(None)),
    ]
# ---- wide forms (forced routes take every shape; with few tiles the cost model splits K from 4 K-steps up): 260 rows are two ragged 256-row tiles under 128 columns
# and three 128-row tiles under 256 ----
for r in (3, 8, 7):
    bm_a, bn_a = (256, 256) if r == 7 else (256, 128)
    bm_b, bn_b = (256, 256) if r == 7 else (128, 256)
    CASES += [
        fwd('w260x128-3k/%s' % ROUTES[r], r, (2, 192, 10, 13), 128, ep='affine', expect=W(r, bm_a, bn_a)),            # bf16 epilogue
        fwd('w260x128-18k/%s' % ROUTES[r], r, (2, 128, 10, 13), 128, k=3, pad=1, expect=W(r, bm_a, bn_a, 9)),          # fp32 slabs
        fwd('w260x256-3k/%s' % ROUTES[r], r, (2, 192, 10, 13), 256, ep='affine', expect=W(r, bm_b, bn_b)),
        fwd('w260x256-18k/%s' % ROUTES[r], r, (2, 128, 10, 13), 256, k=3, pad=1, expect=W(r, bm_b, bn_b, 9)),
        fwd('w-logits/%s' % ROUTES[r], r, (2, 192, 10, 13), 19, ep='logits', expect=W(r, bm_a, bn_a)),
        fwd('w-256tiles/%s' % ROUTES[r], r, (1, 64, 255, 257), 128, k=3, pad=1, expect=W(r, bm_a, bn_a)),             # 256 tiles, unsplit, 9 K-steps
    ]
# 512 tiles on at most 256 blocks: a persistent block walks at least two tiles, and the ring runs across a tile boundary
CASES.append(fwd('w-512tiles/persistent', 3, (1, 64, 255, 257), 256, k=3, pad=1, ep='affine', expect=W(3, 256, 128)))
# ---- data gradient (+ add) on one 3x3 per route; the stride-2 native form (four parity classes) ----
CASES += [dgrad('dgrad-3x3/%s' % ROUTES[r], r, (2, 128, 10, 13), 128, expect=T(64, 128, 2, 2) if r == 2 else W(r, *((256, 256) if r == 7 else (256, 128)), 9))
          for r in (2, 3, 8, 7)]
CASES.append(dgrad('dgrad-stride2', 2, (2, 128, 16, 16), 128, stride=2, expect=dict(mode=4)))
# ---- weight gradient: four of the cases of tests/test_hip_kernels.py WGRAD16_CASES ----
CASES += [
    wgrad('wgrad-dilated-480px', (1, 512, 24, 20, 512, 3, 1, 2, 2), G(256, 128)),        # a partial last 64-pixel step
    wgrad('wgrad-cin304', (1, 304, 40, 36, 256, 3, 1, 1, 1), G(256, 128)),               # the last channel block half empty
    wgrad('wgrad-cout384', (1, 256, 40, 40, 384, 1, 1, 0, 1), G(128, 256)),
    wgrad('wgrad-wide-1x1-144px', (1, 1024, 12, 12, 2048, 1, 1, 0, 1), G(256, 128)),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PERSISTENT = [c['name'] for c in CASES if c['route'] == 3 or c['kind'] == 'wgrad']      # the producer / consumer kernels: run as a step of their own


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def _randn(shape, seed, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _b16(t):
    import torch
    return t.to(torch.bfloat16).cuda()


def _profile(K):
    """The launches recorded since the last clear -> ['mode/bm/bn/km/nst/prec/ksplit', ...] of the LDS-DMA kernels (prec 5: conv16; mode 2, nst 3, prec 4: wgrad16)."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'profile.csv')
        K.profile_dump(path)
        with open(path) as f:
            rows = [line.strip().split(',') for line in f.readlines()[1:]]
    out = []
    for mode, bm, bn, km, nst, prec, m, n, k, batch, ksplit, ms, gflop in rows:
        if int(prec) == 5 or (int(mode) == 2 and int(nst) == 3 and int(prec) == 4):
            out.append('/'.join((mode, bm, bn, km, nst, prec, ksplit)))
    return out


def run_case(K, c):
    """-> ({output: sha256}, reach)."""
    import torch
    n, cin, h, w = c['x']
    cout, k = c['cout'], c['k']
    x = _randn((n, h, w, cin), 1)
    wt = _randn((cout, k, k, cin), 2, (2.0 / (cin * k * k)) ** 0.5).cuda()
    was16, was_prec, was_route = K.BN_EPILOGUE16, (K.CONV_PREC, K.ACT_DTYPE), K.routing()      # put back what was found, whatever it was
    K.set_conv_precision('bf16')
    K.set_conv16(c['route'])
    K.set_wgrad16(True)
    K.profile_enable(True)
    K.profile_read(clear=True)
    out = {}
    try:
        if c['kind'] == 'fwd':
            if c['padded']:
                xg = K.new((n, h, w, cin), wt, dtype=torch.bfloat16)      # zero-padded to a multiple of 64 channels and registered: gathered in place
                xg.copy_(_b16(x))
            else:
                xg = _b16(x)
            ho, wo = K.conv_out_hw(h, w, k, 1, c['pad'], c['dil'])
            kw = {}
            if c['ep'] == 'affine':
                kw = dict(scale=(_randn((cout,), 6).abs() + 0.5).cuda(), shift=_randn((cout,), 7).cuda(), residual=_b16(_randn((n, ho, wo, cout), 8)), relu=True)
            elif c['ep'] == 'logits':
                kw = dict(bias=_randn((cout,), 3).cuda(), out_dtype=torch.float32)
            elif c['ep'] == 'stats':
                K.BN_EPILOGUE16 = True
                kw = dict(bn_partials=[])
            out['y'] = digest(K.conv_fwd(xg, wt, 1, c['pad'], c['dil'], **kw))
            if c['ep'] == 'stats':
                assert kw['bn_partials'][0] is not None, 'the statistics epilogue did not take %s' % c['name']
                out['bn_partials'] = digest(kw['bn_partials'][0])
        elif c['kind'] == 'dgrad':
            ho, wo = K.conv_out_hw(h, w, k, c['stride'], c['pad'], c['dil'])
            dy, skip = _b16(_randn((n, ho, wo, cout), 4)), _b16(_randn((n, h, w, cin), 5))
            out['dx'] = digest(K.conv_bwd_data(dy, wt, (n, h, w, cin), c['stride'], c['pad'], c['dil'], add=skip))
        else:
            ho, wo = K.conv_out_hw(h, w, k, c['stride'], c['pad'], c['dil'])
            dy = _b16(_randn((n, ho, wo, cout), 4))
            out['dw'] = digest(K.conv_bwd_weight(_b16(x), dy, (cout, k, k, cin), c['stride'], c['pad'], c['dil'])[0])
        torch.cuda.synchronize()
        reach = _profile(K)
    finally:
        K.BN_EPILOGUE16 = was16
        K.profile_read(clear=True)
        K.profile_enable(False)      # (the library has no getter for it; every user switches it on for its own calls, as here)
        K.routing(**was_route)
        K.CONV_PREC, K.ACT_DTYPE = was_prec
        K.clear_filters()
    return out, reach


def check_reach(fixture):
    """Every case is recorded, and the profile shows the launch it is named for: every key the case's `expect` gives equals the recorded one (a K-split of None: any
    above 1); a parity-class data gradient has four launches, every other case one."""
    assert sorted(fixture['digests']) == sorted(BY_NAME), sorted(set(fixture['digests']) ^ set(BY_NAME))
    wrong = {}
    for name, c in BY_NAME.items():
        got = [dict(zip(('mode', 'bm', 'bn', 'km', 'nst', 'prec', 'ksplit'), map(int, r.split('/')))) for r in fixture['reach'][name]]
        ok = len(got) == (4 if name == 'dgrad-stride2' else 1)
        for g in got:
            ok = ok and all(g[k] == v if v is not None else g[k] > 1 for k, v in c['expect'].items())
        if not ok:
            wrong[name] = (fixture['reach'][name], c['expect'])
    assert not wrong, wrong


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    assert torch.cuda.is_available(), 'the digests need the GPU'
    from pinthememory_amd.hip import kernels as K
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else FIXTURE
    only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None      # 'persistent' / 'rest': the producer / consumer kernels as a step of their own
    fixture = {'digests': {}, 'reach': {}}
    if os.path.exists(out):
        with open(out) as f:
            fixture = json.load(f)
    for c in CASES:
        if only and (c['name'] in PERSISTENT) != (only == 'persistent'):
            continue
        fixture['digests'][c['name']], fixture['reach'][c['name']] = run_case(K, c)
        print(c['name'], fixture['reach'][c['name']], flush=True)
    with open(out, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    if len(fixture['digests']) == len(CASES):
        check_reach(fixture)
    print('%d case digests -> %s' % (len(fixture['digests']), out))


if __name__ == '__main__':
    main()
