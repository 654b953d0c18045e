"""Every instantiation of the split-path convolution kernel (csrc/conv_split.hip: the fp32 tier on the bf16 matrix pipe, PREC 5) against an fp64 convolution at fp32
accuracy. conv_split.hip instantiates 2 modes (forward, data gradient) x 4 block tiles x 4 K-state modes and the weight gradient x 4 tiles x 2 K-state modes; register
arrays, LDS plane strides and the ragged-edge predication depend on the tile, so each one is reached here by a shape of its own, the launch record (pm_profile_*) proves
that it ran, and the error bar is the one that tells fp32 from a 16-bit mantissa: within 2 x the fp32-MFMA kernel's error + 2e-7 on the same operands
(test_hip_kernels.test_split_path_accuracy_vs_fp64 holds seven small shapes to the same bar; they reach the 64-row tiles and the K_SMALL weight gradient only)."""
import csv

import pytest
import torch
import torch.nn.functional as F

from test_hip_kernels import K, nchw, nhwc, rel, rnd, SPLIT_CASES      # noqa: F401  (K: the module-scoped fixture)

BK = 32
FWD, DGRAD, WGRAD = 0, 1, 2
K_FAST, K_MID, K_SMALL, K_PW = 0, 1, 2, 3
SPLIT_MIN_K = 129

# (n, cin, h, w, cout, k, stride, pad, dil) -> the instantiation (mode, bm, bn, km) each pass must reach under default routing with the Winograd route off, None where
# the pass is not on the split path (a column tile below 64 or a forward / data-gradient reduction below 129). Forward GEMM: M = output pixels, N = cout, K = k^2 cin,
# K-state by cin; data gradient: M = input pixels (stride 2: one GEMM per parity class), N = cin, K = taps x cout, K-state by cout; weight gradient: M = cout,
# N = k^2 cin, K = output pixels, K-state by the output width. Every shape is ragged: rows no multiple of the row tile, columns no multiple of the column tile (the
# stem's 64 columns excepted), K_MID channel counts no multiple of 32. Shapes come from the port of make_plan below; the record on the GPU decides.
SPLIT_MATRIX = [
    # 64-row tiles: fewer than ~150 row tiles
    ((1, 160, 13, 15, 40, 3, 1, 2, 2), (FWD, 64, 64, K_FAST), (DGRAD, 64, 128, K_MID), (WGRAD, 64, 128, K_SMALL)),        # dilated 3x3
    ((1, 36, 13, 15, 40, 3, 1, 1, 1), (FWD, 64, 64, K_MID), (DGRAD, 64, 64, K_MID), (WGRAD, 64, 128, K_SMALL)),
    ((1, 20, 13, 15, 40, 3, 2, 1, 1), (FWD, 64, 64, K_SMALL), None, (WGRAD, 64, 128, K_SMALL)),
    ((1, 160, 13, 15, 40, 1, 1, 0, 1), (FWD, 64, 64, K_PW), None, (WGRAD, 64, 128, K_SMALL)),
    ((2, 4, 40, 36, 64, 7, 2, 3, 1), (FWD, 64, 64, K_SMALL), None, (WGRAD, 64, 128, K_SMALL)),                           # the stem: 7x7 taps, N = 64 exactly
    ((1, 160, 13, 15, 96, 3, 1, 1, 1), (FWD, 64, 128, K_FAST), (DGRAD, 64, 128, K_FAST), (WGRAD, 128, 128, K_SMALL)),
    ((1, 36, 13, 15, 96, 3, 1, 1, 1), (FWD, 64, 128, K_MID), (DGRAD, 64, 64, K_FAST), (WGRAD, 128, 128, K_SMALL)),
    ((1, 20, 13, 15, 72, 3, 2, 1, 1), (FWD, 64, 128, K_SMALL), None, (WGRAD, 128, 128, K_SMALL)),
    ((1, 160, 13, 15, 160, 1, 1, 0, 1), (FWD, 64, 128, K_PW), (DGRAD, 64, 128, K_PW), (WGRAD, 128, 128, K_SMALL)),
    ((1, 36, 13, 15, 160, 1, 1, 0, 1), None, (DGRAD, 64, 64, K_PW), (WGRAD, 128, 64, K_SMALL)),
    ((1, 36, 13, 15, 20, 3, 1, 1, 1), None, (DGRAD, 64, 64, K_SMALL), (WGRAD, 64, 128, K_SMALL)),
    ((1, 72, 13, 15, 20, 3, 1, 1, 1), None, (DGRAD, 64, 128, K_SMALL), (WGRAD, 64, 128, K_SMALL)),
    ((1, 36, 13, 15, 40, 1, 1, 0, 1), None, None, (WGRAD, 64, 64, K_SMALL)),
    ((1, 36, 33, 40, 40, 1, 1, 0, 1), None, None, (WGRAD, 64, 64, K_MID)),
    # 128-row tiles: the production maps' row counts (two rounds of the 256 CUs and more)
    ((2, 160, 97, 95, 40, 3, 1, 1, 1), (FWD, 128, 64, K_FAST), (DGRAD, 64, 128, K_MID), (WGRAD, 64, 128, K_MID)),
    ((6, 144, 97, 95, 40, 1, 1, 0, 1), (FWD, 128, 64, K_MID), None, (WGRAD, 64, 128, K_MID)),
    ((6, 20, 97, 95, 40, 3, 1, 1, 1), (FWD, 128, 64, K_SMALL), None, (WGRAD, 64, 128, K_MID)),
    ((6, 160, 97, 95, 40, 1, 1, 0, 1), (FWD, 128, 64, K_PW), None, (WGRAD, 64, 128, K_MID)),
    ((5, 160, 66, 63, 136, 3, 2, 1, 1), (FWD, 64, 128, K_FAST), (DGRAD, 64, 128, K_MID), (WGRAD, 128, 128, K_MID)),      # stride 2: four parity-class data gradients, K = 136 ... 544
    ((3, 32, 97, 95, 136, 3, 1, 1, 1), (FWD, 128, 128, K_FAST), None, (WGRAD, 128, 128, K_MID)),                         # one K split: the kernel's own epilogue
    ((3, 144, 97, 95, 160, 1, 1, 0, 1), (FWD, 128, 128, K_MID), (DGRAD, 128, 128, K_PW), (WGRAD, 128, 128, K_MID)),
    ((3, 20, 97, 95, 136, 3, 1, 1, 1), (FWD, 128, 128, K_SMALL), None, (WGRAD, 128, 128, K_MID)),
    ((3, 160, 97, 95, 136, 1, 1, 0, 1), (FWD, 128, 128, K_PW), (DGRAD, 128, 128, K_MID), (WGRAD, 128, 128, K_MID)),
    ((2, 36, 97, 95, 160, 3, 1, 1, 1), (FWD, 64, 128, K_MID), (DGRAD, 128, 64, K_FAST), (WGRAD, 128, 128, K_MID)),
    ((6, 36, 97, 95, 136, 1, 1, 0, 1), None, (DGRAD, 128, 64, K_MID), (WGRAD, 128, 64, K_MID)),
    ((6, 36, 97, 95, 20, 3, 1, 1, 1), None, (DGRAD, 128, 64, K_SMALL), (WGRAD, 64, 128, K_MID)),
    ((6, 36, 97, 95, 160, 1, 1, 0, 1), None, (DGRAD, 128, 64, K_PW), (WGRAD, 128, 64, K_MID)),
    ((1, 144, 97, 95, 96, 3, 1, 1, 1), (FWD, 64, 128, K_MID), (DGRAD, 128, 128, K_FAST), (WGRAD, 128, 128, K_MID)),
    ((3, 144, 97, 95, 20, 3, 1, 1, 1), None, (DGRAD, 128, 128, K_SMALL), (WGRAD, 64, 128, K_MID)),
]

# (case, mode) -> whether that pass splits K (ksplit > 1 in the record): one launch of either kind per mode
KSPLIT_WITNESS = {
    ((1, 160, 13, 15, 40, 3, 1, 2, 2), FWD): True, ((3, 32, 97, 95, 136, 3, 1, 1, 1), FWD): False,
    ((1, 160, 13, 15, 96, 3, 1, 1, 1), DGRAD): True, ((3, 144, 97, 95, 160, 1, 1, 0, 1), DGRAD): False,
    ((3, 144, 97, 95, 160, 1, 1, 0, 1), WGRAD): True, ((1, 36, 13, 15, 40, 1, 1, 0, 1), WGRAD): False,
}

FWD_128x128 = (3, 32, 97, 95, 136, 3, 1, 1, 1)       # forward 128 x 128 K_FAST, one K split
FWD_128x64 = (6, 160, 97, 95, 40, 1, 1, 0, 1)        # forward 128 x 64 K_PW, one K split
DGRAD_128x64 = (6, 36, 97, 95, 160, 1, 1, 0, 1)      # data gradient 128 x 64 K_PW, one K split (neither forward case above has a data gradient on the split path)


# ---- a port of the planner (conv_igemm.hip: make_plan, split_takes, the K-state rules of conv_direct / dgrad_s2_parity / conv_wgrad_direct) -------------------
def _cdiv(a, b):
    return -(-a // b)


def make_plan(mode, M, Nn, K):
    """-> (bm, bn, ksplit) of the fp32 tier under pm_routing.split = 1."""
    bn = 128 if Nn > 64 else (64 if Nn > 32 else 32)
    big = mode == WGRAD or K >= SPLIT_MIN_K
    if mode != WGRAD and not big and bn == 128:
        bn = 64
    ksteps = _cdiv(K, BK)
    best, plan = 1e30, None
    for bm in (128, 64):
        if (bm == 64 and bn < 64) or (not big and mode != WGRAD and bn >= 64 and bm == 128):
            continue
        if mode == WGRAD and ((bm == 64 and M > 64) or (bm == 128 and M <= 64 and bn >= 64)):
            continue
        tiles = _cdiv(M, bm) * _cdiv(Nn, bn)
        unit = 2.0 * (bm / 128.0) * (bn / 128.0) * (1.08 if bm == 64 else 1.0)
        for ks in range(1, max(1, min(ksteps // 4, 512)) + 1):
            per = _cdiv(ksteps, ks)
            if _cdiv(ksteps, per) != ks:
                continue
            per_cu = _cdiv(tiles * ks, 256)
            t = per_cu * (per + 2) * unit * (1.25 if per_cu == 1 else 1.0)
            if ks > 1:
                t += 2.0 * ks * M * Nn * 4.0 / 3.0e6 + 6.0
            if t < best:
                best, plan = t, (bm, bn, ks)
    return plan


def _out_hw(h, w, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


def _s2_taps(c, pad, dil, k):
    if dil & 1:
        k0 = (c + pad) & 1
        return (k - k0 + 1) // 2 if k0 < k else 0
    return 0 if (c + pad) & 1 else k


def predict(case):
    """-> per mode the list of (mode, bm, bn, km, ksplit, on the split path) launches the direct route makes."""
    n, cin, h, w, cout, k, s, p, d = case
    ho, wo = _out_hw(h, w, k, s, p, d)

    def kstate(c, pointwise):
        km = K_FAST if c % BK == 0 else (K_MID if c >= BK else K_SMALL)
        return K_PW if km == K_FAST and pointwise else km

    def one(mode, M, Nn, K, km):
        bm, bn, ks = make_plan(mode, M, Nn, K)
        taken = bn >= 64 and (mode == WGRAD or K >= SPLIT_MIN_K)
        return (mode, bm, bn, km if taken or km != K_PW else K_FAST, ks, taken)

    out = {FWD: [one(FWD, n * ho * wo, cout, k * k * cin, kstate(cin, k == 1 and s == 1 and p == 0))]}
    if s == 2:
        out[DGRAD] = []
        for cls in range(4):
            cy, cx = cls >> 1, cls & 1
            rows, taps = n * ((h - cy + 1) >> 1) * ((w - cx + 1) >> 1), _s2_taps(cy, p, d, k) * _s2_taps(cx, p, d, k)
            if rows > 0 and taps > 0:
                out[DGRAD].append(one(DGRAD, rows, cin, taps * cout, K_MID if cout >= BK else K_SMALL))
    else:
        out[DGRAD] = [one(DGRAD, n * h * w, cin, k * k * cout, kstate(cout, k == 1 and p == 0))]
    out[WGRAD] = [one(WGRAD, cout, k * k * cin, n * ho * wo, K_MID if wo >= BK else K_SMALL)]
    return out


def every_instantiation():
    tiles = [(128, 128), (128, 64), (64, 128), (64, 64)]
    return ({(m, bm, bn, km) for m in (FWD, DGRAD) for bm, bn in tiles for km in (K_FAST, K_MID, K_SMALL, K_PW)} |
            {(WGRAD, bm, bn, km) for bm, bn in tiles for km in (K_MID, K_SMALL)})


def test_split_matrix_declares_every_instantiation():
    """The union of the declared instantiations is the full list conv_split.hip instantiates (2 x 4 x 4 + 4 x 2 = 40), no entry left out; the table holds the cases the
    issue of this test asks for (either kind of K split per mode, a dilated 3x3, a stride-2 data gradient whose four parity classes are all on the split path)."""
    assert len(SPLIT_MATRIX) <= 30 and len({e[0] for e in SPLIT_MATRIX}) == len(SPLIT_MATRIX)
    declared = {inst for e in SPLIT_MATRIX for inst in e[1:] if inst is not None}
    assert all(e[1 + m] is None or e[1 + m][0] == m for e in SPLIT_MATRIX for m in (FWD, DGRAD, WGRAD))
    assert declared == every_instantiation() and len(declared) == 40
    cases = [e[0] for e in SPLIT_MATRIX]
    for m in (FWD, DGRAD, WGRAD):
        assert {v for (c, mode), v in KSPLIT_WITNESS.items() if mode == m and c in cases} == {True, False}, m
    assert any(k == 3 and p == 2 and d == 2 for (_, _, _, _, _, k, _, p, d) in cases)
    assert any(s == 2 and cout >= 64 and e[2] is not None for e in SPLIT_MATRIX for (_, _, _, _, cout, _, s, _, _) in [e[0]])
    assert (2, 4, 40, 36, 64, 7, 2, 3, 1) in cases
    for c in (FWD_128x128, FWD_128x64, DGRAD_128x64):
        assert c in cases


@pytest.mark.parametrize('entry', SPLIT_MATRIX, ids=lambda e: 'x'.join(map(str, e[0])))
def test_split_matrix_agrees_with_the_planner_port(entry):
    """The port of make_plan / split_takes above predicts what the table declares (and the K splits of KSPLIT_WITNESS): every launch of a declared pass is that
    instantiation on the split path, no launch of an undeclared pass is on it; and the shape is ragged in every declared GEMM."""
    case = entry[0]
    n, cin, h, w, cout, k, s, p, d = case
    pred = predict(case)
    for m in (FWD, DGRAD, WGRAD):
        if entry[1 + m] is None:
            assert not any(r[5] for r in pred[m]), (m, pred[m])
            continue
        assert pred[m] and all(r[5] and r[:4] == entry[1 + m] for r in pred[m]), (m, pred[m])
        if (case, m) in KSPLIT_WITNESS:
            assert (max(r[4] for r in pred[m]) > 1) == KSPLIT_WITNESS[(case, m)]
        _, bm, bn, km = entry[1 + m]
        ho, wo = _out_hw(h, w, k, s, p, d)
        rows = [n * ho * wo] if m == FWD else ([cout] if m == WGRAD else
                                               ([n * h * w] if s == 1 else [n * ((h - c // 2 + 1) >> 1) * ((w - c % 2 + 1) >> 1) for c in range(4)]))
        cols = cout if m == FWD else (cin if m == DGRAD else k * k * cin)
        if case != (2, 4, 40, 36, 64, 7, 2, 3, 1):      # the stem is in the table for its 7x7 taps and its 64 output channels: exactly one column tile
            assert all(r % bm for r in rows) and cols % bn, (m, rows, cols)
        if km == K_MID and m != WGRAD:
            assert (cin if m == FWD else cout) % BK


# ---- the GPU tests ------------------------------------------------------------------------------------------------------------------------------------------
def operands_no_oracle(case):
    """As test_split_path_accuracy_vs_fp64: a post-ReLU-like x (mostly one sign, large sums), a He-scaled w, a normal dy."""
    n, cin, h, w, cout, k, s, p, d = case
    ho, wo = _out_hw(h, w, k, s, p, d)
    x = torch.relu(rnd(n, cin, h, w, seed=1)) + 0.01 * rnd(n, cin, h, w, seed=7)
    return x, rnd(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5), rnd(n, cout, ho, wo, seed=4)


def operands(case):
    """The same with the oracle: the fp64 convolution on the CPU and its two gradients."""
    n, cin, h, w, cout, k, s, p, d = case
    x, wt, dy = operands_no_oracle(case)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, stride=s, padding=p, dilation=d)
    y_ref.backward(dy.double())
    return x, wt, dy, y_ref.detach(), xr.grad, wr.grad


def records(K, path):
    """The launch records filed since profile_enable(True), as dicts of ints (mode, bm, bn, km, nst, prec, M, N, K, batch, ksplit); the store is cleared."""
    torch.cuda.synchronize()
    K.profile_dump(path)
    K.profile_read(clear=True)
    with open(path) as f:
        return [{k: int(v) for k, v in row.items() if k not in ('ms', 'gflop')} for row in csv.DictReader(f)]


@pytest.mark.gpu
@pytest.mark.parametrize('entry', SPLIT_MATRIX, ids=lambda e: 'x'.join(map(str, e[0])))
def test_split_instantiation_vs_fp64(K, entry, tmp_path, capsys):
    """One table entry: forward, data gradient and weight gradient with the split path on and off (Winograd route off). The record shows the declared instantiation
    with prec 5 and no other operand form in that mode (split on), no prec 5 launch at all (split off). Each of rel(y), rel(dx), rel(dw) against fp64 with the split
    on is within 2 x the fp32-MFMA kernel's + 2e-7 (one product of the six lost: ~1.5e-5), and the fp32 kernel itself is inside the bars of test_conv_fwd_bwd."""
    case = entry[0]
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt, dy, y_ref, dx_ref, dw_ref = operands(case)
    xg, wg, dyg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy)
    errs, recs = {}, {}
    K.profile_read(clear=True)
    try:
        K.set_winograd(0)
        for split in (True, False):
            K.set_split(split)
            K.profile_enable(True)
            y = K.conv_fwd(xg, wg, s_, p, d)
            dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s_, p, d)
            dw, _ = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s_, p, d)
            recs[split] = records(K, str(tmp_path / ('split%d.csv' % split)))
            K.profile_enable(False)
            errs[split] = (rel(nchw(y), y_ref), rel(nchw(dx), dx_ref), rel(dw.permute(0, 3, 1, 2), dw_ref))
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_split(True)
        K.set_winograd(4)
    with capsys.disabled():
        print('\n[split matrix %s] ' % (case,) + ' '.join('(%d,%d,%d,%d,ks%d,p%d)' % (r['mode'], r['bm'], r['bn'], r['km'], r['ksplit'], r['prec']) for r in recs[True]) +
              '; ' + '; '.join('%s: y %.2e dx %.2e dw %.2e' % (('split' if sp else 'fp32 ',) + e) for sp, e in errs.items()))
    for m in (FWD, DGRAD, WGRAD):
        mine = [r for r in recs[True] if r['mode'] == m]
        assert mine, (m, recs[True])
        if entry[1 + m] is None:
            assert all(r['prec'] != 5 for r in mine), (m, mine)
            continue
        assert any((r['mode'], r['bm'], r['bn'], r['km']) == entry[1 + m] and r['prec'] == 5 for r in mine), (m, mine)
        assert all(r['prec'] == 5 for r in mine), (m, mine)
        if (case, m) in KSPLIT_WITNESS:
            assert (max(r['ksplit'] for r in mine) > 1) == KSPLIT_WITNESS[(case, m)], (m, mine)
    assert recs[False] and all(r['prec'] != 5 for r in recs[False]), recs[False]
    assert errs[False][0] < 2e-5 and errs[False][1] < 2e-5 and errs[False][2] < 5e-5, errs
    for es, e0 in zip(errs[True], errs[False]):
        assert es <= 2.0 * e0 + 2e-7, errs


@pytest.mark.gpu
@pytest.mark.parametrize('case', [FWD_128x128, FWD_128x64])
def test_split_epilogue_and_channel_slices_on_the_large_tiles(K, case, tmp_path):
    """The kernel's own epilogue (one K split) on the 128-row tiles: bias, scale / shift, residual and ReLU, read from a channel slice of a wider input and written into
    the channel slice [32, 32 + cout) of a wider zeroed buffer. Order as in the kernel: relu((conv + bias) * scale + shift + residual)."""
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt, _, y_ref, _, _ = operands(case)
    b, sc, sh, res = rnd(cout, seed=3), rnd(cout, seed=5).abs() + 0.5, rnd(cout, seed=6), rnd(*y_ref.shape, seed=8)
    ref = torch.relu((y_ref + b.double()[None, :, None, None]) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None] + res.double())
    xwide = torch.zeros(n, h, w, cin + 48, device='cuda')
    xwide[..., :16] = 1e3      # the neighbours of the slice: large values a gather that ignored the pitch would pick up
    xwide[..., 16 + cin:] = -1e3
    xwide[..., 16:16 + cin] = nhwc(x)
    rwide = torch.full((n, y_ref.shape[2], y_ref.shape[3], cout + 16), 1e3, device='cuda')
    rwide[..., 8:8 + cout] = nhwc(res)
    wg = wt.permute(0, 2, 3, 1).contiguous().cuda()
    buf = torch.zeros(n, y_ref.shape[2], y_ref.shape[3], cout + 64, device='cuda')
    errs = {}
    K.profile_read(clear=True)
    try:
        K.set_winograd(0)
        for split in (True, False):
            K.set_split(split)
            buf.zero_()
            K.profile_enable(True)
            out = K.conv_fwd(xwide[..., 16:16 + cin], wg, s_, p, d, bias=b.cuda(), scale=sc.cuda(), shift=sh.cuda(), residual=rwide[..., 8:8 + cout], relu=True,
                             out=buf[..., 32:32 + cout])
            rec = records(K, str(tmp_path / 'ep.csv'))
            K.profile_enable(False)
            assert len(rec) == 1 and rec[0]['ksplit'] == 1 and (rec[0]['prec'] == 5) == split, rec
            if split:
                assert (rec[0]['mode'], rec[0]['bm'], rec[0]['bn'], rec[0]['km']) == [e for e in SPLIT_MATRIX if e[0] == case][0][1], rec
            errs[split] = rel(nchw(out), ref)
            assert buf[..., :32].abs().max().item() == 0 and buf[..., 32 + cout:].abs().max().item() == 0
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_split(True)
        K.set_winograd(4)
    print('[split epilogue %s] split %.2e fp32 %.2e' % (case, errs[True], errs[False]))
    assert errs[False] < 2e-5 and errs[True] <= 2.0 * errs[False] + 2e-7, errs


@pytest.mark.gpu
def test_split_data_gradient_fused_add_on_the_large_tile(K, tmp_path):
    """The data gradient's fused skip add (dx = conv_bwd_data(dy) + add in the kernel's epilogue) on the 128 x 64 tile, one K split."""
    case = DGRAD_128x64
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt, dy, _, dx_ref, _ = operands(case)
    add = rnd(n, cin, h, w, seed=5)
    wg, dyg, addg = wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy), nhwc(add)
    errs = {}
    K.profile_read(clear=True)
    try:
        K.set_winograd(0)
        for split in (True, False):
            K.set_split(split)
            K.profile_enable(True)
            dx = K.conv_bwd_data(dyg, wg, (n, h, w, cin), s_, p, d, add=addg)
            rec = records(K, str(tmp_path / 'add.csv'))
            K.profile_enable(False)
            assert len(rec) == 1 and rec[0]['ksplit'] == 1 and (rec[0]['prec'] == 5) == split, rec
            if split:
                assert (rec[0]['mode'], rec[0]['bm'], rec[0]['bn'], rec[0]['km']) == (DGRAD, 128, 64, K_PW), rec
            errs[split] = rel(nchw(dx), dx_ref + add.double())
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_split(True)
        K.set_winograd(4)
    print('[split dgrad add %s] split %.2e fp32 %.2e' % (case, errs[True], errs[False]))
    assert errs[False] < 2e-5 and errs[True] <= 2.0 * errs[False] + 2e-7, errs


@pytest.mark.gpu
@pytest.mark.parametrize('case', [FWD_128x128, FWD_128x64])
def test_split_statistics_twin_on_the_large_tiles(K, case, tmp_path):
    """The STATS = true twins of the split forward kernel (BatchNorm statistics out of the convolution's epilogue, as test_conv_epilogue_bn_statistics requests them):
    y is bit-identical to the run without the request, mean and inverse standard deviation match fp64 statistics of that y to 1e-6."""
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt = operands_no_oracle(case)[:2]
    b = rnd(cout, seed=3)
    xg, wg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda()
    ps = []
    prev = K.BN_EPILOGUE
    K.profile_read(clear=True)
    try:
        K.set_winograd(0)
        K.BN_EPILOGUE = True
        K.profile_enable(True)
        y = K.conv_fwd(xg, wg, s_, p, d, bias=b.cuda(), bn_partials=ps)
        rec = records(K, str(tmp_path / 'stats.csv'))
        K.profile_enable(False)
        K.BN_EPILOGUE = prev
        y_plain = K.conv_fwd(xg, wg, s_, p, d, bias=b.cuda())
    finally:
        K.BN_EPILOGUE = prev
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_winograd(4)
    assert ps[0] is not None, 'pm_conv_bn_partials_bytes must be non-zero here: one K split, a column tile of 64 or more'
    assert len(rec) == 1 and rec[0]['prec'] == 5 and rec[0]['ksplit'] == 1 and (rec[0]['bm'], rec[0]['bn']) == [e for e in SPLIT_MATRIX if e[0] == case][0][1][1:3], rec
    assert torch.equal(y, y_plain)
    pixels = y.shape[0] * y.shape[1] * y.shape[2]
    mean, inv = K.bn_partials_finalize(ps[0], pixels, cout, 1e-5)
    yr = nchw(y).double()
    assert rel(mean, yr.mean((0, 2, 3))) < 1e-6 and rel(inv, 1.0 / torch.sqrt(yr.var((0, 2, 3), unbiased=False) + 1e-5)) < 1e-6


@pytest.mark.gpu
def test_split_winograd_f2_point_gemms_vs_fp64(K, tmp_path):
    """F(2x2,3x3) on the split path: sixteen batched point GEMMs per pass (batch > 1: on the split path at every reduction length), forward and data gradient,
    against fp64 at the split bar (test_split_path_accuracy_vs_fp64 holds routes 4 and 0 to it)."""
    case = SPLIT_CASES[2]
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt, dy, y_ref, dx_ref, dw_ref = operands(case)
    xg, wg, dyg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy)
    errs = {}
    K.profile_read(clear=True)
    try:
        K.set_winograd(2)
        for split in (True, False):
            K.set_split(split)
            K.profile_enable(True)
            y = K.conv_fwd(xg, wg, s_, p, d)
            dx = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s_, p, d)
            dw, _ = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s_, p, d)
            rec = records(K, str(tmp_path / 'wino.csv'))
            K.profile_enable(False)
            batched = [r for r in rec if r['batch'] > 1]
            assert len(batched) == 2 and all(r['batch'] == 16 and (r['prec'] == 5) == split for r in batched), rec      # forward and data gradient: F(2x2) is taken
            assert all((r['prec'] == 5) == split for r in rec), rec
            errs[split] = (rel(nchw(y), y_ref), rel(nchw(dx), dx_ref), rel(dw.permute(0, 3, 1, 2), dw_ref))
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_split(True)
        K.set_winograd(4)
    print('[split wino 2 %s] ' % (case,) + '; '.join('%s: y %.2e dx %.2e dw %.2e' % (('split' if sp else 'fp32 ',) + e) for sp, e in errs.items()))
    assert errs[False][0] < 2e-5 and errs[False][1] < 2e-5 and errs[False][2] < 5e-5, errs
    for es, e0 in zip(errs[True], errs[False]):
        assert es <= 2.0 * e0 + 2e-7, errs


@pytest.mark.gpu
@pytest.mark.parametrize('mode,case', [(FWD, FWD_128x128), (DGRAD, (3, 144, 97, 95, 160, 1, 1, 0, 1)), (WGRAD, (2, 36, 97, 95, 160, 3, 1, 1, 1))])
def test_split_power_of_two_scale_invariance(K, mode, case, tmp_path):
    """Every step of the split kernel commutes with a power of two (truncation split, exact remainders, products, fp32 accumulation, the split-K sum): scaling x
    (forward) or dy (both gradients: the cross-entropy gradient is divided by millions of pixels) by 2^-24 scales the result by exactly 2^-24. No bias."""
    n, cin, h, w, cout, k, s_, p, d = case
    x, wt, dy = operands_no_oracle(case)
    xg, wg, dyg = nhwc(x), wt.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(dy)
    sc = 2.0 ** -24
    K.profile_read(clear=True)
    try:
        K.set_winograd(0)
        K.profile_enable(True)
        if mode == FWD:
            a, b = K.conv_fwd(xg, wg, s_, p, d), K.conv_fwd(xg * sc, wg, s_, p, d)
        elif mode == DGRAD:
            a, b = K.conv_bwd_data(dyg, wg, tuple(xg.shape), s_, p, d), K.conv_bwd_data(dyg * sc, wg, tuple(xg.shape), s_, p, d)
        else:
            a, b = K.conv_bwd_weight(xg, dyg, tuple(wg.shape), s_, p, d)[0], K.conv_bwd_weight(xg, dyg * sc, tuple(wg.shape), s_, p, d)[0]
        rec = records(K, str(tmp_path / 'pow2.csv'))
    finally:
        K.profile_enable(False)
        K.profile_read(clear=True)
        K.set_winograd(4)
    want = [e for e in SPLIT_MATRIX if e[0] == case][0][1 + mode]
    assert len(rec) == 2 and all((r['mode'], r['bm'], r['bn'], r['km']) == want and r['prec'] == 5 for r in rec), rec
    assert a.abs().max().item() > 0
    assert torch.equal(b, a * sc), ((b - a * sc).abs().max().item(), a.abs().max().item())
