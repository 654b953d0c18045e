"""Records the output bits of the implicit-GEMM convolution kernel (csrc/conv_igemm_kernel.h: every fp32 convolution, every Winograd point product, and what the
LDS-DMA kernels leave of the bf16 tier), of the streaming pointwise kernel (csrc/pwstream.hip) and of the split-K reduce into tests/golden/igemm_bits.json;
tests/test_igemm_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_igemm_bits.py [--out FILE] [--only NAME,NAME...]

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. Every kernel is deterministic
(the split-K reduce has a fixed order), so a digest (sha256 of the output's bytes) either matches or the change altered a bit.

The calls go through conv_fwd / conv_bwd_data / conv_bwd_weight (hip/kernels.py) under five configurations (CONFIGS below): the fp32 tier with default routing
(operands split into three bf16 pieces where the reduction allows: PREC 5) and with routing(split=0) (fp32 MFMA: PREC 0), fp32 tensors rounded per fragment
('bf16_staged': PREC 1), bf16 operands over fp32 activations ('bf16_operands': PREC 2, weight gradient PREC 3) and the bf16 tier with the LDS-DMA kernels
switched off (PREC 2 with bf16 output, weight gradients PREC 4 / 3, the parity-class data gradient on a widened dy). Two more take the fp32 tier through the Winograd
transforms (csrc/winograd.hip) on maps that do not tile: 'wino2' (routing(winograd=2): F(2 x 2) where the default takes F(4 x 4)) and 'fused' (routing(winograd_fused=1):
wino_fused_f4_kernel, recorded as mode 3) -- their digests hold every transform's bits, epilogue, ragged edges, K padding and slab sum included. Inputs come from CPU generators with fixed
seeds. Beside the digests the in-library profile's record of each call is kept ('reach': mode/bm/bn/km/nst/prec/batch/ksplit per launch) and check_reach holds
it to the form the case is named for -- the planner rules the cases were laid out by are proven by that, not assumed."""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'igemm_bits.json')

# name -> (set_conv_precision, routing fields replaced for the case)
CONFIGS = {
    'split': ('f32', dict(split=1)),
    'fp32': ('f32', dict(split=0)),
    'staged': ('bf16_staged', dict()),
    'operands': ('bf16_operands', dict(conv16=0)),
    'bf16': ('bf16', dict(conv16=0)),
    'bf16-small': ('bf16', dict()),      # default routing: fewer than 256 output pixels stay with the register-staged kernel
    'wino2': ('f32', dict(winograd=2)),      # F(2 x 2) wherever the Winograd route is taken
    'fused': ('f32', dict(winograd_fused=1)),      # F(4 x 4): point products and output transform in one kernel (wino_fused_f4_kernel)
}
REACH_KEYS = ('mode', 'bm', 'bn', 'km', 'nst', 'prec', 'batch', 'ksplit')
FAST, MID, SMALL, PW, STREAM = 0, 1, 2, 3, 4      # the km column (K_FAST ... K_PW of the kernel; 4: the streaming pointwise kernel's records)

CASES = []


def case(kind, name, cfg, x, cout, k=1, stride=1, pad=0, dil=1, expect=None, launches=1, **kw):
    """x = (n, cin, h, w) of the convolution's input. expect: keys of REACH_KEYS every recorded launch must show; launches: how many (None: at least one)."""
    CASES.append(dict(kind=kind, name='%s/%s/%s' % (cfg, kind, name), cfg=cfg, x=x, cout=cout, k=k, stride=stride, pad=pad, dil=dil, expect=expect or {}, launches=launches, **kw))


def fwd(name, cfg, x, cout, ep='plain', **kw):
    """ep: plain | bias | affine (scale / shift + residual + ReLU) | stats (bn_partials) | affine-odd (bf16: the residual is a channel slice that starts 8 bytes
    off a 16-byte boundary)."""
    case('fwd', name if ep == 'plain' else '%s-%s' % (name, ep), cfg, x, cout, ep=ep, **kw)


def dgrad(name, cfg, x, cout, add='add', **kw):
    """add: none | add | mask (pm_conv_bwd_data_masked)."""
    case('dgrad', name if add == 'add' else '%s-%s' % (name, add), cfg, x, cout, add=add, **kw)


def wgrad(name, cfg, x, cout, dbias=False, **kw):
    case('wgrad', name, cfg, x, cout, dbias=dbias, **kw)


def E(mode, bm=None, bn=None, km=None, nst=None, prec=None, batch=1, ksplit=None):
    return {k: v for k, v in dict(mode=mode, bm=bm, bn=bn, km=km, nst=nst, prec=prec, batch=batch, ksplit=ksplit).items() if v is not None}


def S(c):
    return (2, c, 13, 11)       # 286 pixels: ragged in every tile size


def MIDDLE(c):
    return (1, c, 127, 129)


def L(c):
    return (1, c, 255, 257)     # 65535 pixels: one below the streaming kernel's threshold


C3 = dict(k=3, pad=1)
STEM = dict(k=7, stride=2, pad=3)

# ---- the small and middle shapes, under default routing (split operands, PREC 5, one LDS stage) and under routing(split=0) (fp32 MFMA, PREC 0) ----
for cfg in ('split', 'fp32'):
    sp = cfg == 'split'
    P = 5 if sp else 0

    def T(mode, bm, bn, km, ksplit=None, nst=1, prec=P, **kw):
        return E(mode, bm, bn, km, nst if not sp or prec == 0 else 1, prec, ksplit=ksplit, **kw)

    for ep in ('plain', 'bias', 'affine', 'stats'):
        fwd('1x1-160-64', cfg, S(160), 64, ep, expect=T(0, 64, 64, PW if sp else FAST, 1))
        fwd('1x1-160-200', cfg, S(160), 200, ep, expect=T(0, 64, 128 if sp else 64, PW if sp else FAST, 1))      # ragged column tile
    fwd('1x1-64-64', cfg, S(64), 64, expect=E(0, 64, 64, FAST, 1, 0, ksplit=1))                                  # K = 64 < 129: fp32 MFMA either way
    fwd('3x3-64-64', cfg, S(64), 64, 'affine', expect=T(0, 64, 64, FAST, 4), **C3)                                 # four K-splits: the vector reduce applies the epilogue
    fwd('3x3-64-64-d2', cfg, S(64), 64, 'affine', expect=T(0, 64, 64, FAST, 4), k=3, pad=2, dil=2)
    fwd('3x3-64-1100', cfg, S(64), 1100, expect=T(0, 64, 128 if sp else 64, FAST), **C3)                         # nine (eighteen) column tiles: the n_group walk
    fwd('3x3-256-64', cfg, MIDDLE(256), 64, expect=T(0, 64, 64, FAST, 1, nst=2), **C3)                           # 72 K-steps: two LDS stages on the fp32-MFMA form
    fwd('3x3-256-64', cfg, MIDDLE(256), 64, 'stats', expect=T(0, 64, 64, FAST, 1, nst=2), **C3)
    fwd('3x3-48-64', cfg, S(48), 64, expect=T(0, 64, 64, MID, 1, nst=2), **C3)
    fwd('stem', cfg, (2, 4, 13, 11), 64, expect=T(0, 64, 64, SMALL, 1, nst=2), **STEM)
    fwd('1x1-64-19', cfg, S(64), 19, 'bias', expect=E(0, 128, 32, FAST, 2, 0, ksplit=1))                          # pitch 20, 19 columns: the per-element edge epilogue
    fwd('1x1-64-20', cfg, S(64), 20, 'bias', expect=E(0, 128, 32, FAST, 2, 0, ksplit=1))                          # the staged one
    dgrad('3x3-64-64', cfg, S(64), 64, expect=T(1, 64, 64, FAST, 4), **C3)
    dgrad('1x1-64-160', cfg, S(64), 160, expect=T(1, 64, 64, PW if sp else FAST, 1))
    dgrad('1x1-64-160', cfg, S(64), 160, 'mask', expect=T(1, 64, 64, PW if sp else FAST, 1))
    dgrad('3x3-48-48', cfg, S(48), 48, expect=T(1, 64, 64, MID, 1, nst=2), **C3)
    dgrad('3x3-64-16', cfg, S(64), 16, expect=T(1, 64, 64, SMALL, 1, nst=2), **C3)
    dgrad('s2-8-8', cfg, (1, 8, 9, 9), 8, expect=E(1, 128, 32, SMALL, 2, 0), launches=4, k=3, stride=2, pad=1)      # parity classes
    dgrad('s2-64-64', cfg, (2, 64, 12, 12), 64, expect=E(1, 64, 64, MID), launches=4, k=3, stride=2, pad=1)
    wgrad('3x3-64-64-w20', cfg, (2, 64, 24, 20), 64, expect=T(2, 64, 128, SMALL, nst=2), **C3)
    wgrad('3x3-64-64-w36', cfg, (1, 64, 40, 36), 64, expect=T(2, 64, 128, MID, nst=2), **C3)
    wgrad('3x3-64-128', cfg, S(64), 128, expect=T(2, 128, 128, SMALL, nst=2), **C3)
    wgrad('stem', cfg, (2, 4, 40, 36), 64, dbias=True, expect=T(2, 64, 128, SMALL, nst=2), **STEM)
    wgrad('1x1-64-19', cfg, S(64), 19, expect=T(2, 64, 64, SMALL, nst=2))                                          # 19 ragged rows
    wgrad('1x1-8-8', cfg, S(8), 8, expect=E(2, 128, 32, SMALL, 2, 0))
    # batched launches, the unstaged epilogue: Winograd F(4 x 4) (36 point products; with 256 channels: two column tiles, the XCD dealing with a remainder of four
    # units) and F(2 x 2) at dilation 6 (16: whole units per XCD). The weight gradient takes the route from 256 x 256 channels up.
    WB = dict(bm=128 if sp else 64, bn=128, prec=P, nst=1)
    for c, hw in ((128, 16), (256, 16)):
        fwd('wino4-%d' % c, cfg, (1, c, hw, hw), c, expect=dict(mode=0, batch=36, km=PW if sp else FAST, **WB), **C3)
        dgrad('wino4-%d' % c, cfg, (1, c, hw, hw), c, expect=dict(mode=0, batch=36, km=PW if sp else FAST, **WB), **C3)
    wgrad('wino4-256', cfg, (1, 256, 16, 16), 256, expect=dict(mode=2, batch=36, bm=128, bn=128, prec=P), **C3)
    fwd('wino2-d6', cfg, (1, 128, 12, 12), 128, expect=dict(mode=0, batch=16, km=PW if sp else FAST, **WB), k=3, pad=6, dil=6)
    dgrad('wino2-d6', cfg, (1, 128, 12, 12), 128, expect=dict(mode=0, batch=16, km=PW if sp else FAST, **WB), k=3, pad=6, dil=6)

# ---- default routing only: the large shape (128-row tiles, unsplit) and the streaming pointwise kernel ----
for cout, bn in ((64, 64), (128, 128), (200, 128)):
    for ep in ('plain', 'affine'):
        fwd('3x3-L-64-%d' % cout, 'split', L(64), cout, ep, expect=E(0, 128, bn, FAST, 1, 5, ksplit=1), **C3)
fwd('3x3-L-64-128', 'split', L(64), 128, 'stats', expect=E(0, 128, 128, FAST, 1, 5, ksplit=1), **C3)
PWS = dict(bm=32, bn=64, km=STREAM, nst=0, prec=5, batch=1, ksplit=1)
fwd('stream-64-64', 'split', (1, 64, 256, 256), 64, expect=dict(mode=0, **PWS))
fwd('stream-128-256', 'split', (1, 128, 256, 256), 256, 'affine', expect=dict(mode=0, **PWS))
dgrad('stream-64-64', 'split', (1, 64, 256, 256), 64, 'mask', expect=dict(mode=1, **PWS))

# ---- the Winograd transforms (csrc/winograd.hip) where a map does not tile: F(4 x 4) under default routing, F(2 x 2) under routing(winograd=2) ----
# 132 -> 140 channels on 13 x 15: ragged edge tiles in both axes, K padded 132 -> 160 (zero-filled in V and U), a ragged column tile, output rows beyond H / W
# skipped. Dilation 2: sub-lattices of 7 / 6 rows and 8 / 7 columns, so the edge tiles differ per sub-lattice (multiplies ratio 0.328 for F(4 x 4), 0.583 for F(2 x 2)).
# The weight gradient takes the route from 256 x 256 channels up (260 -> Kp 288): one slab on 13 x 15, and on 63 x 65 the fixed-order slab sum of wino_dw_kernel
# (F(4 x 4): 544 tiles, 17 K-steps, two slabs; F(2 x 2): 2112 tiles, 66 K-steps, five).
WX = (2, 132, 13, 15)
D2 = dict(k=3, pad=2, dil=2)
for cfg, batch, ks in (('split', 36, 2), ('wino2', 16, 5)):
    for ep in ('plain', 'bias', 'affine'):
        fwd('wino-132-140', cfg, WX, 140, ep, expect=E(0, batch=batch), **C3)
    for add in ('none', 'add'):
        dgrad('wino-132-140', cfg, WX, 140, add, expect=E(0, batch=batch), **C3)
    fwd('wino-132-140-d2', cfg, WX, 140, 'affine', expect=E(0, batch=batch), **D2)
    dgrad('wino-132-140-d2', cfg, WX, 140, expect=E(0, batch=batch), **D2)
    wgrad('wino-260-256', cfg, (1, 260, 13, 15), 256, dbias=True, expect=E(2, batch=batch, ksplit=1), **C3)
    wgrad('wino-260-256-slabs', cfg, (2, 260, 63, 65), 256, expect=E(2, batch=batch, ksplit=ks), **C3)
# the fused kernel (recorded as mode 3): 48 tiles are one full and one half tile block; 140 channels are five channel blocks, the last 12 wide, the data gradient's 132
# leave it 4 wide
fwd('wino-132-140', 'fused', (3, 132, 13, 15), 140, 'affine', expect=E(3, batch=36), **C3)
dgrad('wino-132-140', 'fused', (3, 132, 13, 15), 140, expect=E(3, batch=36), **C3)

# ---- fp32 tiles rounded to bf16 per fragment (PREC 1) ----
fwd('3x3-64-64', 'staged', S(64), 64, 'affine', expect=E(0, prec=1), **C3)
fwd('1x1-64-19', 'staged', S(64), 19, 'bias', expect=E(0, prec=1))
dgrad('3x3-64-64', 'staged', S(64), 64, expect=E(1, prec=1), **C3)
wgrad('3x3-64-64-w20', 'staged', (2, 64, 24, 20), 64, expect=E(2, prec=1), **C3)

# ---- bf16 operands over fp32 activations: PREC 2 in forward form (the data gradient too), the transpose-read weight gradient PREC 3 ----
fwd('3x3-64-64', 'operands', S(64), 64, 'affine', expect=E(0, km=FAST, prec=2), **C3)
dgrad('3x3-64-64', 'operands', S(64), 64, expect=E(0, km=FAST, prec=2), **C3)
wgrad('3x3-64-64', 'operands', S(64), 64, expect=E(2, prec=3), **C3)

# ---- the bf16 tier without the LDS-DMA kernels ----
for ep in ('plain', 'affine', 'stats', 'affine-odd'):      # affine-odd: the per-element bf16 epilogue
    fwd('3x3-64-64', 'bf16', S(64), 64, ep, expect=E(0, km=FAST, prec=2, ksplit=1), **C3)
fwd('3x3-64-64', 'bf16-small', (1, 64, 13, 11), 64, expect=E(0, km=FAST, prec=2), **C3)
fwd('stem', 'bf16', (2, 4, 13, 11), 64, expect=E(0, km=SMALL, prec=1), **STEM)                     # fp32 image in, bf16 out
wgrad('3x3-128-64', 'bf16', (1, 128, 16, 16), 64, expect=E(2, prec=4), **C3)                       # both operands bf16: gathered as they are
wgrad('stem', 'bf16', (2, 4, 40, 36), 64, dbias=True, expect=E(2, prec=3), **STEM)                 # fp32 image x bf16 dy: dy widened
dgrad('s2-64-32', 'bf16', (2, 64, 12, 12), 32, expect=E(1, km=MID, prec=1), launches=4, k=3, stride=2, pad=1)      # parity classes on a widened dy

BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes()).hexdigest()


def _randn(shape, seed, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _profile(K):
    """The launches recorded since the last clear -> ['mode/bm/bn/km/nst/prec/batch/ksplit', ...]."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'profile.csv')
        K.profile_dump(path)
        with open(path) as f:
            rows = [line.strip().split(',') for line in f.readlines()[1:]]
    return ['/'.join((mode, bm, bn, km, nst, prec, batch, ksplit)) for mode, bm, bn, km, nst, prec, m, n, k, batch, ksplit, ms, gflop in rows]


def run_case(K, c):
    """-> ({output: sha256}, reach)."""
    import torch
    n, cin, h, w = c['x']
    cout, k, stride, pad, dil = c['cout'], c['k'], c['stride'], c['pad'], c['dil']
    ho, wo = K.conv_out_hw(h, w, k, stride, pad, dil)
    prec_name, route = CONFIGS[c['cfg']]
    was_ep, was_prec, was_route = (K.BN_EPILOGUE, K.BN_EPILOGUE16), (K.CONV_PREC, K.ACT_DTYPE), K.routing()      # put back what was found, whatever it was
    K.set_conv_precision(prec_name)
    K.routing(**route)
    act = K.ACT_DTYPE

    def dev(t, dtype=None):
        return t.to(dtype or act).cuda()

    wt = _randn((cout, k, k, cin), 2, (2.0 / (cin * k * k)) ** 0.5).cuda()
    K.profile_enable(True)
    K.profile_read(clear=True)
    out = {}
    try:
        if c['kind'] == 'fwd':
            x = dev(_randn((n, h, w, cin), 1), torch.float32 if cin < 32 else None)      # the stem reads the fp32 image on either tier
            ep, kw = c['ep'], {}
            if ep == 'bias':
                kw = dict(bias=_randn((cout,), 3).cuda())
            elif ep in ('affine', 'affine-odd'):
                res = dev(_randn((n, ho, wo, cout + (8 if ep == 'affine-odd' else 0)), 8))
                kw = dict(scale=(_randn((cout,), 6).abs() + 0.5).cuda(), shift=_randn((cout,), 7).cuda(), residual=res[..., 4:4 + cout] if ep == 'affine-odd' else res, relu=True)
            elif ep == 'stats':
                K.BN_EPILOGUE = K.BN_EPILOGUE16 = True
                kw = dict(bn_partials=[])
            out['y'] = digest(K.conv_fwd(x, wt, stride, pad, dil, **kw))
            if ep == 'stats':
                assert kw['bn_partials'][0] is not None, 'the statistics epilogue did not take %s' % c['name']
                # (mean, M2) per 32-row slab and channel: the buffer is sized up to a multiple of 256 bytes and nothing writes the tail (200 channels: 48 floats)
                out['bn_partials'] = digest(kw['bn_partials'][0][:(n * ho * wo + 31) // 32 * cout * 2])
        elif c['kind'] == 'dgrad':
            dy = dev(_randn((n, ho, wo, cout), 4))
            kw = {}
            if c['add'] != 'none':
                kw['add'] = dev(_randn((n, h, w, cin), 5))
            if c['add'] == 'mask':
                kw['add_mask'] = torch.randint(0, 16, (n * h * w, cin // 4), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).cuda()
            out['dx'] = digest(K.conv_bwd_data(dy, wt, (n, h, w, cin), stride, pad, dil, **kw))
        else:
            x = dev(_randn((n, h, w, cin), 1), torch.float32 if cin < 32 else None)
            dy = dev(_randn((n, ho, wo, cout), 4))
            if cout % 4:      # the 19 class logits: rows padded to 16 bytes, as every producer leaves them
                dy = K.new(dy.shape, dy, pitch_pad=True).copy_(dy)
            dw, db = K.conv_bwd_weight(x, dy, (cout, k, k, cin), stride, pad, dil, want_bias=c['dbias'])
            out['dw'] = digest(dw)
            if c['dbias']:
                out['dbias'] = digest(db)
        torch.cuda.synchronize()
        reach = _profile(K)
    finally:
        K.BN_EPILOGUE, K.BN_EPILOGUE16 = was_ep
        K.profile_read(clear=True)
        K.profile_enable(False)      # (the library has no getter for it; every user switches it on for its own calls, as here)
        K.routing(**was_route)
        K.CONV_PREC, K.ACT_DTYPE = was_prec
        K.clear_filters()
    return out, reach


def reach_errors(fixture):
    """{case: (recorded, expected)} of the cases whose recorded launches are not the ones they are named for."""
    wrong = {}
    for name, c in BY_NAME.items():
        if name not in fixture['reach']:
            continue
        got = [dict(zip(REACH_KEYS, map(int, r.split('/')))) for r in fixture['reach'][name]]
        ok = len(got) == c['launches'] if c['launches'] else len(got) >= 1
        for g in got:
            ok = ok and all(g[k] == v for k, v in c['expect'].items())
        if not ok:
            wrong[name] = (fixture['reach'][name], c['expect'], c['launches'])
    return wrong


# every instantiation family of the kernel: (mode, km, prec) of a recorded launch -- what the cases together have to cover
FORMS = [(m, km, p) for m in (0, 1) for km, p in ((FAST, 0), (MID, 0), (SMALL, 0), (FAST, 5), (MID, 5), (SMALL, 5), (PW, 5), (STREAM, 5), (FAST, 1))] + \
        [(2, km, p) for km in (MID, SMALL) for p in (0, 5)] + [(0, SMALL, 1), (1, MID, 1), (2, SMALL, 1), (0, FAST, 2), (2, None, 3), (2, None, 4)]


def check_reach(fixture):
    """Every case is recorded and the profile shows the launches it is named for: every key the case's `expect` gives equals the recorded one in every launch, and
    there are as many launches as the case says (a parity-class data gradient: four). Together the cases reach every form of FORMS, both LDS stage counts of the
    fp32-MFMA kernel and every tile. What a launch record does not carry -- the n_group walk (more than eight column tiles), the batch_xcd dealing and its remainder
    path (36 units over one / two tiles), the STATS instantiation (bn_partials handed out), the bf16 per-element epilogue (affine-odd) -- is reached by the way the
    cases are laid out, not proven here; a wrong result there shows in the digests."""
    assert sorted(fixture['digests']) == sorted(BY_NAME), sorted(set(fixture['digests']) ^ set(BY_NAME))
    wrong = reach_errors(fixture)
    assert not wrong, wrong
    rows = [dict(zip(REACH_KEYS, map(int, r.split('/')))) for rs in fixture['reach'].values() for r in rs]
    seen = {(g['mode'], g['km'], g['prec']) for g in rows} | {(g['mode'], None, g['prec']) for g in rows}
    assert not [f for f in FORMS if f not in seen], [f for f in FORMS if f not in seen]
    assert {(g['bm'], g['bn']) for g in rows if g['prec'] == 0} >= {(64, 64), (64, 128), (128, 128), (128, 32)}
    assert {(g['bm'], g['bn']) for g in rows if g['prec'] == 5 and g['km'] != STREAM} >= {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {g['nst'] for g in rows if g['prec'] == 0 and g['mode'] == 0 and g['km'] == FAST and g['bn'] >= 64} == {1, 2}


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    assert torch.cuda.is_available(), 'the digests need the GPU'
    from pinthememory_amd.hip import kernels as K
    from pinthememory_amd.hip.lib import PinmemError
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else FIXTURE
    only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else None
    fixture = {'digests': {}, 'reach': {}}
    if os.path.exists(out):
        with open(out) as f:
            fixture = json.load(f)
    for key in ('digests', 'reach'):      # cases that left the list
        fixture[key] = {n: v for n, v in fixture[key].items() if n in BY_NAME}
    for c in CASES:
        if only and c['name'] not in only:
            continue
        try:
            fixture['digests'][c['name']], fixture['reach'][c['name']] = run_case(K, c)
        except (AssertionError, PinmemError) as e:      # a call the library refused: reported, the other cases are still recorded (anything else ends the run)
            print('ERROR', c['name'], e, flush=True)
            continue
        print(c['name'], fixture['reach'][c['name']], flush=True)
    with open(out, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    for name, w in reach_errors(fixture).items():
        print('REACH', name, w, flush=True)
    if len(fixture['digests']) == len(CASES):
        check_reach(fixture)
    print('%d case digests -> %s' % (len(fixture['digests']), out))


if __name__ == '__main__':
    main()
