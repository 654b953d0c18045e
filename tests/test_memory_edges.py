"""The memory kernels (memory.hip) at the slot counts, row counts and noise ranges that neither tests/test_hip_kernels.py nor the memory block of
tests/test_tensor_views.py reaches: more than one row per wave in the row kernels, more column partials than the apply kernel keeps in registers, the generic
(32 padded slots) instantiations at slots 8..31, softmax arguments that overflow fp32 without the max subtraction, and labels the write kernels must drop.

Every reference is the plain formulation in fp64 torch on the CPU (read_ref / write_ref below); gradients are autograd of that formulation. p_mem and p_query are
compared with the fp64 softmax of the kernel's OWN score plus the noise (the score is checked against the fp64 score separately): the score's 4e-7 would otherwise be
amplified by the exponentials. Bars (rel() = max |a - b| / max |b|): qr, score, p_mem, p_query 2e-6; p_query column sums within 1e-5 of 1; nominator, denominator
3e-6; dx, dmem, dz, dnom 2e-5. The launcher constants the shapes are computed from: row_blocks() = min(ceil(rows / 4), 2048) blocks of four waves (row kernels),
min(ceil(rows / 32), 3072) blocks of one 32-row tile (MFMA read kernels), CSA_PER = 24 partials per thread in registers (32 ranges: 768 partials)."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_kernels import rel, rnd

pytestmark = pytest.mark.gpu
D = 256


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pinthememory_amd.hip import kernels
    return kernels


def read_ref(x, mem, noise=None, dqr=None, dsx=None):
    """The read in fp64: F.normalize -> matmul -> softmax over the slots -> matmul -> cat. x (..., 256) channels-last fp32 on the CPU. Returns qr, score, p_mem and,
    when dqr is given, the autograd gradients of sum(qr dqr) + sum(score dsx) with respect to x (as rows) and the memory."""
    rows = x.numel() // D
    xr = x.double().reshape(rows, D).requires_grad_(dqr is not None)
    mr = mem.double().requires_grad_(dqr is not None)
    q = F.normalize(xr, dim=1)
    s = torch.matmul(q, mr.t())
    pm = F.softmax(s if noise is None else s + noise.double(), 1)
    qr = torch.cat((q, torch.matmul(pm, mr)), 1)
    if dqr is None:
        return qr, s, pm, None, None
    ((qr * dqr.double().reshape(rows, 2 * D)).sum() + (s * dsx.double()).sum()).backward()
    return qr.detach(), s.detach(), pm.detach(), xr.grad, mr.grad


def write_ref(z, lab, m, normalize, dnom=None):
    """The write accumulation in fp64: one-hot -> F.interpolate(bilinear, align_corners=True) -> matmul. 255 and the literal m are the ignore class (channel m); every
    other label outside [0, m) goes to an extra channel m + 1 that is cut off after the interpolation: the pixel keeps its bilinear weight but feeds no class, which
    is what the kernels' `cls = -1` does. Returns nominator [m + 1][256], denominator [m + 1] and, when dnom is given, the gradient of sum(nominator dnom) wrt z."""
    n, h, w, _ = z.shape
    t = lab.clone()
    t[((lab < 0) | (lab > m)) & (lab != 255)] = m + 1
    t[lab == 255] = m
    y = F.interpolate(F.one_hot(t, m + 2).permute(0, 3, 1, 2).double(), [h, w], mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(n * h * w, m + 2)
    y = y[:, :m + 1]
    zr = z.double().reshape(n * h * w, D).requires_grad_(dnom is not None)
    nom = torch.matmul(y.t(), F.normalize(zr, dim=1) if normalize else zr)
    if dnom is None:
        return nom, y.sum(0), None
    (nom * dnom.double()).sum().backward()
    return nom.detach(), y.sum(0), zr.grad


def gumbel(rows, m, seed):
    return -torch.empty(rows, m).exponential_(generator=torch.Generator().manual_seed(seed)).log()


def read_case(n, h, w, m, seed=40):
    """relu(randn) features with ONE all-zero row (the eps clamp), a normalised memory, dqr and a non-zero dsx."""
    x = torch.relu(rnd(n, h, w, D, seed=seed))
    x[0, 0, 0, :] = 0
    mem = F.normalize(rnd(m, D, seed=seed + 1), dim=1)
    return x, mem, rnd(n, h, w, 2 * D, seed=seed + 2), rnd(n * h * w, m, seed=seed + 3) * 0.1


def read_bwd_both(K, xg, memg, pmem, dqr, dsx, dx_ref, dmem_ref):
    """Both backward kernels on one p_mem: the row kernel (dx + dmem) and the dx-only MFMA kernel against autograd at 2e-5 (the one all-zero row, row 0, left out: torch
    takes another sub-gradient at the clamp), and against each other at 1e-5 with that row included (scaled by 1 / eps in both). Returns the errors and dmem."""
    rows = dx_ref.shape[0]
    dqg, dsg = dqr.cuda(), dsx.cuda()
    dx, dmem = K.mem_read_bwd(xg, memg, pmem, dqg, dsg, want_dmem=True)
    dx2, none = K.mem_read_bwd(xg, memg, pmem, dqg, dsg)
    assert none is None
    e = (rel(dx.view(rows, D)[1:], dx_ref[1:]), rel(dx2.view(rows, D)[1:], dx_ref[1:]), rel(dmem, dmem_ref), rel(dx2, dx))
    assert e[0] < 2e-5 and e[1] < 2e-5 and e[2] < 2e-5 and e[3] < 1e-5, e
    return e, dmem


@pytest.mark.parametrize('n,h,w,m', [(1, 91, 91, 19), (8, 48, 48, 19), (1, 91, 91, 32), (1, 91, 91, 20)])
def test_read_bwd_dmem_accumulates_over_several_rows_per_wave(K, n, h, w, m, capsys):
    """Gap 1: the per-wave `dm[j] += ...` of mem_read_bwd_kernel<*, true>, its grid-stride loop and the 2 048-slab fixed-order reduce behind them. row_blocks() caps
    the launch at 2 048 blocks x 4 waves = 8 192 waves, and every other test stays at or below 4 608 rows (one row per wave at most). 8 281 rows (1 x 91 x 91): 89
    waves take two rows; 18 432 rows (8 x 48 x 48, the flagship batch): two or three rows per wave. m = 19 is the specialised instantiation, 20 and 32 the generic
    one (32: no padding slot). p_mem comes from a forward with Gumbel noise, dsx is non-zero. dmem and dx against fp64 autograd at 2e-5, dx of the two kernels
    against each other at 1e-5 (zero row included), dmem bit-identical over two calls, and dmem must be more than 1e-3 away from the fp64 dmem of the first 8 192
    rows alone: a kernel that kept one row per wave is wrong by that much, not merely close.
    Measured on the MI355X, worst of the four cases: dx of the row kernel 4.1e-7, dx of the MFMA kernel 1.5e-7, dmem 3.1e-7, row against MFMA kernel 3.1e-7; dmem
    is 0.10 (8 281 rows, m = 19) to 1.04 (18 432 rows) away from the dmem of the first 8 192 rows."""
    rows = n * h * w
    assert rows > 8192
    x, mem, dqr, dsx = read_case(n, h, w, m)
    noise = gumbel(rows, m, 5)
    _, _, _, dx_ref, dmem_ref = read_ref(x, mem, noise, dqr, dsx)
    head = read_ref(x.view(rows, D)[:8192], mem, noise[:8192], dqr.view(rows, 2 * D)[:8192], dsx[:8192])[4]
    assert rel(dmem_ref, head) > 1e-3                                   # the rows past the first 8 192 matter ...
    xg, memg = x.cuda(), mem.cuda()
    _, _, pmem = K.mem_read_fwd(xg, memg, noise.cuda())
    e, dmem = read_bwd_both(K, xg, memg, pmem, dqr, dsx, dx_ref, dmem_ref)
    with capsys.disabled():
        print('\n[dmem rows=%d m=%d] dx row %.2e  dx mfma %.2e  dmem %.2e  row vs mfma %.2e  (dmem vs first 8 192 rows alone %.2e)' % ((rows, m) + e + (rel(dmem, head),)))
    assert rel(dmem, head) > 1e-3                                       # ... and the kernel has them
    _, again = K.mem_read_bwd(xg, memg, pmem, dqr.cuda(), dsx.cuda(), want_dmem=True)
    assert torch.equal(dmem, again)                                     # fixed-order reduction


@pytest.mark.parametrize('m', [1, 8, 9, 20, 31, 32])
def test_read_slot_counts(K, m, capsys):
    """Gap 4, read side: the generic instantiations (M_ = 0, 32 padded slots) were only run at m <= 7, i.e. register quad 0 of the MFMA result layout. Slot of
    register q is (q & 3) + 8 (q >> 2) + 4 half, the column partials use w + 8 qq + 4 half: m = 8 fills the first quad of both half-waves exactly, 9 starts the second
    quad, 20 and 31 reach the third and fourth, 32 (MAXM) has no padding lane (mz always 1), 1 is a softmax over one slot (p_mem exactly 1.0). 126 rows (2 x 9 x 7):
    three full 32-row tiles and a ragged one of 30. Plain read and read + p_query (bit-equal q / score / p_mem) without noise and with two independent Gumbel draws,
    mem_colsoftmax, and both backward kernels (dx of both, dmem of the row kernel)."""
    n, h, w = 2, 9, 7
    rows = n * h * w
    x, mem, dqr, dsx = read_case(n, h, w, m, seed=50)
    noise, noise_q = gumbel(rows, m, 5), gumbel(rows, m, 7)
    xg, memg = x.cuda(), mem.cuda()
    worst = [0.0] * 5
    for nz, nq in ((None, None), (noise, noise_q)):
        qr_ref, s_ref, pm_ref, dx_ref, dmem_ref = read_ref(x, mem, nz, dqr, dsx)
        nzg, nqg = (nz.cuda(), nq.cuda()) if nz is not None else (None, None)
        qr, score, pmem = K.mem_read_fwd(xg, memg, nzg)
        qa, sa, pa, pq = K.mem_read_fwd_pq(xg, memg, nzg, nqg)
        assert torch.equal(qa, qr) and torch.equal(sa, score) and torch.equal(pa, pmem)
        sk = score.double().cpu()
        pm_own = F.softmax(sk + (nz.double() if nz is not None else 0.0), 1)
        pq_own = F.softmax(sk + (nq.double() if nq is not None else 0.0), 0)
        e = (rel(qr.view(rows, 2 * D), qr_ref), rel(score, s_ref), rel(pmem, pm_own), rel(pq, pq_own), rel(K.mem_colsoftmax(score, nqg), pq_own))
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert max(e) < 2e-6, e
        assert rel(pmem, pm_ref) < 2e-6                                 # 126 rows, unscaled noise: also within the bar of the end-to-end fp64 p_mem
        assert (pq.double().sum(0) - 1).abs().max().item() < 1e-5
        if m == 1:
            assert (pmem == 1.0).all().item()
        eb, _ = read_bwd_both(K, xg, memg, pmem, dqr, dsx, dx_ref, dmem_ref)
    with capsys.disabled():
        print('\n[read m=%d] qr %.2e score %.2e p_mem %.2e p_query %.2e colsoftmax %.2e | gumbel: dx row %.2e dx mfma %.2e dmem %.2e row vs mfma %.2e' % ((m,) + tuple(worst) + eb))


def edge_labels(m, n, H, W, seed):
    """Labels from [0, m) with class m - 2 folded into class 0 (an absent class, m >= 3), ~10 % 255, ~5 % values the kernels must DROP (from {-1, m + 1 .. 254}, with
    -1, m + 1, 254 and 2^32 -- class 0 after a truncation to 32 bits -- planted so that each occurs), ~2 % the literal m (the ignore class, exactly like 255)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, m, (n, H, W), generator=g)
    if m >= 3:
        lab[lab == m - 2] = 0
    u = torch.rand(n, H, W, generator=g)
    lab[u < 0.10] = 255
    pool = torch.tensor([-1] + list(range(m + 1, 255)))
    sel = (u >= 0.10) & (u < 0.15)
    picks = pool[torch.randint(0, len(pool), (int(sel.sum()),), generator=g)]
    picks[:4] = torch.tensor([-1, m + 1, 254, 1 << 32])
    lab[sel] = picks
    lab[(u >= 0.15) & (u < 0.17)] = m
    return lab


@pytest.mark.parametrize('normalize', [True, False], ids=['normalized', 'raw'])
@pytest.mark.parametrize('m', [1, 3, 20, 31])
def test_write_slot_counts_and_dropped_labels(K, m, normalize, capsys):
    """Gaps 4 (write side) and 7. Writes ran at m = 19 and 6 only: m = 31 is the largest (m + 1 == 32 = MAXM classes, every lane of the A operand a class, the
    exchange tile full), 20 leaves a partial slab that is not 16-byte sized beyond register quad 1, 1 and 3 are the smallest. soft_label_taps gives `cls = -1` to
    every label outside [0, m] other than 255: such a pixel feeds neither a nominator nor a denominator -- one_hot would raise there, so the reference sends them to
    an extra channel that is cut off. z (1, 9, 7): one ragged chunk of 63 rows, labels (30, 20). Nominator and denominator at 3e-6 (an all-zero row included), dz of
    mem_write_accum_bwd at 2e-5 on a z without the zero row."""
    n, h, w, H, W = 1, 9, 7, 30, 20
    zb = torch.relu(rnd(n, h, w, D, seed=61))
    z = zb.clone()
    z[0, 0, 0, :] = 0
    lab = edge_labels(m, n, H, W, 62)
    dropped = ((lab < 0) | (lab > m)) & (lab != 255)
    assert dropped.sum().item() >= 4 and (lab == m).any().item() and (lab == 255).any().item()
    nom_ref, den_ref, _ = write_ref(z, lab, m, normalize)
    labg = lab.cuda()
    nomden = K.mem_write_accum(z.cuda(), labg, m, normalize=normalize)
    e_nom, e_den = rel(nomden[:(m + 1) * D].view(m + 1, D), nom_ref), rel(nomden[(m + 1) * D:], den_ref)
    dnom = rnd(m + 1, D, seed=63)
    _, _, dz_ref = write_ref(zb, lab, m, normalize, dnom)
    dz = K.mem_write_accum_bwd(zb.cuda(), labg, m, dnom.cuda(), normalize=normalize)
    e_dz = rel(dz.view(-1, D), dz_ref)
    with capsys.disabled():
        print('\n[write m=%d normalize=%d] nominator %.2e denominator %.2e dz %.2e' % (m, normalize, e_nom, e_den, e_dz))
    assert e_nom < 3e-6 and e_den < 3e-6
    assert e_dz < 2e-5
    if m >= 3:
        assert nomden[(m + 1) * D + m - 2].item() == 0.0 and nomden[(m - 2) * D:(m - 1) * D].abs().max().item() == 0.0      # the absent class


@pytest.mark.parametrize('m', [1, 31])
def test_write_update_on_the_accumulated_nomden(K, m, capsys):
    """Gap 4, update side: mem_write_update / mem_write_update_bwd on the nominator / denominator that mem_write_accum left for the labels of the test above, at
    m = 1 (one block) and m = 31 (dnom has m + 1 = 32 rows). U = den != 0 ? mu M + (1 - mu) nom / den : M, M' = U / |U| and dnom against fp64 autograd on the same
    nomden (outputs 2e-6, dnom 2e-5); at m = 31 class 29 is absent and keeps its slot (m = 1 has no class that could be absent next to a present one)."""
    n, h, w, H, W, mu = 1, 9, 7, 30, 20, 0.8
    z = torch.relu(rnd(n, h, w, D, seed=61))
    z[0, 0, 0, :] = 0
    lab = edge_labels(m, n, H, W, 62)
    mem, dout = F.normalize(rnd(m, D, seed=64), dim=1), rnd(m, D, seed=65)
    nomden = K.mem_write_accum(z.cuda(), lab.cuda(), m)
    nd = nomden.double().cpu()
    nom, den = nd[:(m + 1) * D].view(m + 1, D).clone().requires_grad_(True), nd[(m + 1) * D:]
    mr = mem.double()
    present = den[:m] != 0
    safe = torch.where(present, den[:m], torch.ones(m, dtype=torch.float64))[:, None]
    upd = torch.where(present[:, None], mu * mr + (1 - mu) * nom[:m] / safe, mr)
    new = F.normalize(upd, dim=1)
    (new * dout.double()).sum().backward()
    out, u = K.mem_write_update(mem.cuda(), nomden, mu, want_u=True)
    dnom = K.mem_write_update_bwd(u, nomden, mu, dout.cuda())
    e = (rel(out, new.detach()), rel(u, upd.detach()), rel(dnom, nom.grad))
    with capsys.disabled():
        print('\n[update m=%d] out %.2e u %.2e dnom %.2e' % ((m,) + e))
    assert e[0] < 2e-6 and e[1] < 2e-6 and e[2] < 2e-5
    assert dnom[m].abs().max().item() == 0.0                             # the ignore class never reaches the memory
    if m == 31:
        assert not present[29].item() and present.sum().item() == m - 1
        assert rel(out[29], mem[29]) < 1e-6 and dnom[29].abs().max().item() == 0.0


def softmax_fp32_error(v32, dim, ref64):
    """e_ref: the error against fp64 of a well-summed fp32 softmax of the same fp32 argument (torch.sum is cascaded)."""
    e = torch.exp(v32 - v32.max(dim, keepdim=True).values)
    return rel(e / e.sum(dim, keepdim=True), ref64)


@pytest.mark.parametrize('m', [8, 32])
def test_softmax_arguments_that_need_the_max_subtraction(K, m, capsys):
    """Gap 5: scores are cosines and the Gumbel draws of every other test stay in about [-2.5, 13], where exp() is harmless in fp32 with or without the max
    subtraction. -log(Exp(1)) has no upper bound: both draws are multiplied by 8 here (arguments in about [-20, 105]) and the test asserts that exp(score + noise)
    does overflow fp32, so a row softmax, a column partial, a partial merge or an apply pass that skipped or misplaced its max would produce inf / nan. 8 281 rows
    (1 x 91 x 91): 259 tiles / 65 partials. Bar for p_mem and p_query: max(2e-6, 4 e_ref), e_ref the error against fp64 of exp(v - max) / sum in fp32 torch on the
    same fp32 score and noise (the fp32 sum score + noise alone is rounded to 4e-6 at 100); the 4 covers expf against exp and another, still tree-shaped, summation
    order. Column sums within 1e-5, score at 2e-6, every output finite, and the backward through these p_mem (both kernels) at 2e-5.
    Measured on the MI355X. m = 8, arguments in [-18.9, 98.8]: p_mem 4.8e-7 (e_ref 4.8e-7, bar 2e-6), p_query 8.0e-7 from the read's partials and from
    mem_colsoftmax (e_ref 8.6e-7, bar 3.4e-6). m = 32, arguments in [-20.0, 104.6]: p_mem 8.1e-7 (e_ref 8.1e-7, bar 3.2e-6), p_query 1.41e-6 from both (e_ref
    1.41e-6, bar 5.6e-6). The kernels sit at the reference-side error: what is left is the rounding of score + noise. Backward: dx 3.8e-7, dmem 2.5e-7."""
    n, h, w = 1, 91, 91
    rows = n * h * w
    x, mem, dqr, dsx = read_case(n, h, w, m, seed=70)
    noise, noise_q = 8 * gumbel(rows, m, 5), 8 * gumbel(rows, m, 7)
    _, s_ref, _, dx_ref, dmem_ref = read_ref(x, mem, noise, dqr, dsx)
    assert torch.isinf(torch.exp((s_ref + noise).float())).any().item()          # without the max subtraction the row softmax overflows ...
    assert torch.isinf(torch.exp((s_ref + noise_q).float())).any().item()        # ... and so does the softmax over the queries
    xg, memg, nzg, nqg = x.cuda(), mem.cuda(), noise.cuda(), noise_q.cuda()
    qr, score, pmem = K.mem_read_fwd(xg, memg, nzg)
    qa, sa, pa, pq = K.mem_read_fwd_pq(xg, memg, nzg, nqg)
    pc = K.mem_colsoftmax(score, nqg)
    for t in (qr, score, pmem, pq, pc):
        assert torch.isfinite(t).all().item()
    assert torch.equal(qa, qr) and torch.equal(sa, score) and torch.equal(pa, pmem)
    assert rel(score, s_ref) < 2e-6
    sk = score.cpu()
    pm_own, pq_own = F.softmax(sk.double() + noise.double(), 1), F.softmax(sk.double() + noise_q.double(), 0)
    er_m, er_q = softmax_fp32_error(sk + noise, 1, pm_own), softmax_fp32_error(sk + noise_q, 0, pq_own)
    bar_m, bar_q = max(2e-6, 4 * er_m), max(2e-6, 4 * er_q)
    e_m, e_q, e_c = rel(pmem, pm_own), rel(pq, pq_own), rel(pc, pq_own)
    with capsys.disabled():
        print('\n[softmax range m=%d, arguments in [%.1f, %.1f]] p_mem %.2e (e_ref %.2e, bar %.2e)  p_query %.2e  colsoftmax %.2e (e_ref %.2e, bar %.2e)'
              % (m, (sk + noise).min().item(), (sk + noise).max().item(), e_m, er_m, bar_m, e_q, e_c, er_q, bar_q))
    assert e_m < bar_m and e_q < bar_q and e_c < bar_q
    assert (pq.double().sum(0) - 1).abs().max().item() < 1e-5 and (pc.double().sum(0) - 1).abs().max().item() < 1e-5
    eb, _ = read_bwd_both(K, xg, memg, pmem, dqr, dsx, dx_ref, dmem_ref)
    with capsys.disabled():
        print('[softmax range m=%d] dx row %.2e dx mfma %.2e dmem %.2e row vs mfma %.2e' % ((m,) + eb))


def test_read_pq_with_more_partials_than_the_apply_kernel_keeps_in_registers(K, capsys):
    """Gap 2 through pm_mem_read_fwd_pq: a thread of mem_colsoftmax_apply_kernel keeps ceil(nb / 32) <= CSA_PER = 24 partials in registers, nb <= 768; beyond that
    it takes the branch that re-reads its partials twice. The read kernel leaves one partial per 32-row tile, so the branch starts at 24 577 rows; the largest
    p_query of the other tests has 576. 24 649 rows (1 x 157 x 157) = 771 tiles, per = 25, the last tile ragged with 9 rows; m = 20 (generic instantiation, third
    register quad). With and without noise_q: p_query against the fp64 softmax of the kernel's score (+ noise) at 2e-6, columns sum to 1 within 1e-5, q / score /
    p_mem bit-equal to the plain read, score against fp64 at 2e-6, a second call gives the same bits."""
    n, h, w, m = 1, 157, 157, 20
    rows = n * h * w
    assert (rows + 31) // 32 == 771 and rows % 32 == 9
    x, mem, _, _ = read_case(n, h, w, m, seed=80)
    _, s_ref, _, _, _ = read_ref(x, mem)
    xg, memg = x.cuda(), mem.cuda()
    qr, score, pmem = K.mem_read_fwd(xg, memg)
    assert rel(score, s_ref) < 2e-6
    sk = score.double().cpu()
    for nq in (None, gumbel(rows, m, 7)):
        nqg = nq.cuda() if nq is not None else None
        qa, sa, pa, pq = K.mem_read_fwd_pq(xg, memg, None, nqg)
        assert torch.equal(qa, qr) and torch.equal(sa, score) and torch.equal(pa, pmem)
        ref = F.softmax(sk + (nq.double() if nq is not None else 0.0), 0)
        e, cs = rel(pq, ref), (pq.double().sum(0) - 1).abs().max().item()
        with capsys.disabled():
            print('\n[771 partials, noise_q %s] p_query %.2e  column sums off by %.2e' % (nq is not None, e, cs))
        assert e < 2e-6 and cs < 1e-5
        assert torch.equal(pq, K.mem_read_fwd_pq(xg, memg, None, nqg)[3])


@pytest.mark.parametrize('m', [19, 32])
def test_colsoftmax_either_side_of_the_register_edge(K, m, capsys):
    """Gap 2 through pm_mem_colsoftmax (128-row partials): 98 304 rows = 768 partials, per = 24, the last size that stays in registers; 98 305 rows = 769 partials,
    per = 25, the first that takes the re-reading branch (its 769th partial holds one row). A flat score with cosine-ranged values plus Gumbel noise, no read;
    m = 19 and 32 (every column of the 32-wide thread layout live). p_query against fp64 at 2e-6, columns sum to 1 within 1e-5, a second call gives the same bits.
    The two sizes share their first 98 304 rows and must agree there to 1e-5 of the column maxima: the extra row is planted at the bottom of the range (score -1,
    the smallest noise drawn), so that it moves every normaliser by less than 1e-7 and the two branches are compared on what is the same softmax."""
    g = torch.Generator().manual_seed(90 + m)
    score = torch.rand(98305, m, generator=g) * 2 - 1
    noise = gumbel(98305, m, 91 + m)
    score[-1], noise[-1] = -1.0, noise.min()
    got = {}
    for rows in (98304, 98305):
        assert (rows + 127) // 128 == (768 if rows == 98304 else 769)
        sg, ng = score[:rows].contiguous().cuda(), noise[:rows].contiguous().cuda()
        pq = K.mem_colsoftmax(sg, ng)
        ref = F.softmax(score[:rows].double() + noise[:rows].double(), 0)
        e, cs = rel(pq, ref), (pq.double().sum(0) - 1).abs().max().item()
        with capsys.disabled():
            print('\n[colsoftmax rows=%d m=%d] p_query %.2e  column sums off by %.2e' % (rows, m, e, cs))
        assert e < 2e-6 and cs < 1e-5
        assert torch.equal(pq, K.mem_colsoftmax(sg, ng))
        got[rows] = pq.double().cpu()
    a, b = got[98304], got[98305][:98304]
    assert ((a - b).abs().max(0).values / a.max(0).values).max().item() < 1e-5


@pytest.mark.parametrize('normalize', [True, False], ids=['normalized', 'raw'])
def test_write_accum_bwd_past_one_row_per_wave(K, normalize, capsys):
    """Gap 6: mem_write_accum_bwd_kernel launches row_blocks() = min(ceil(rows / 4), 2 048) blocks of four waves and had only run on <= 63 rows: one row per wave,
    its grid-stride loop never taken. z (4, 96, 100) = 38 400 rows on 8 192 waves: four or five rows per wave; labels (200, 333), m = 19 -- the shape
    test_memory_write_accum_on_the_matrix_cores uses for the forward. dz against fp64 autograd at 2e-5; the planted all-zero row (torch: another sub-gradient at the
    clamp) is left out when the rows are normalised. Measured on the MI355X: 7.4e-6 normalised, 8.5e-6 raw -- twenty times the 4e-7 of the 63-row cases, and not
    from the loop: the bilinear weights are formed in fp32 from source coordinates of up to 332, whose fraction carries 332 x 2^-24 = 2e-5, and dz is linear in them."""
    n, h, w, H, W, m = 4, 96, 100, 200, 333, 19
    z = torch.relu(rnd(n, h, w, D, seed=21))
    z[0, 0, 0, :] = 0
    g = torch.Generator().manual_seed(22)
    lab = torch.randint(0, m - 3, (n, H, W), generator=g)
    lab[torch.rand(n, H, W, generator=g) < 0.1] = 255
    dnom = rnd(m + 1, D, seed=23)
    _, _, dz_ref = write_ref(z, lab, m, normalize, dnom)
    dz = K.mem_write_accum_bwd(z.cuda(), lab.cuda(), m, dnom.cuda(), normalize=normalize).view(-1, D)
    skip = 1 if normalize else 0
    e = rel(dz[skip:], dz_ref[skip:])
    with capsys.disabled():
        print('\n[write bwd 38 400 rows normalize=%d] dz %.2e' % (normalize, e))
    assert e < 2e-5
