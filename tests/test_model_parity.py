"""GPU parity of the assembled HIP path (network package + harness) against the CPU oracle on the same seeded inputs
and against the golden fixtures captured from the imported reference. Bar (BASELINE.json north_star): logits within 1e-3
fp32, argmax class maps bit-exact (wherever the reference's own top-2 margin exceeds 2e-3, SURVEY.md 'Hard parts')."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CRIT = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
LOGIT_TOL = 1e-3


@pytest.fixture(scope='module')
def env():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from oracle.ref_cpu import deeplab as o_deeplab, harness as o_harness
    from pinthememory_amd import harness, synth
    from pinthememory_amd.network import deepv2, deepv3plus
    return dict(o_deeplab=o_deeplab, o_harness=o_harness, harness=harness, synth=synth, deepv2=deepv2, deepv3plus=deepv3plus)


def argmax_gate(lg, ref_lg, tol=LOGIT_TOL):
    top2 = ref_lg.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 2 * tol
    a, b = lg.argmax(1), ref_lg.argmax(1)
    return bool((a[safe] == b[safe]).all()), float((a == b).float().mean()), float(safe.float().mean())


def test_config1_eval_forward_vs_oracle_and_golden(env, golden):
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
    x, _ = synth.make_batch(1, 256)
    with torch.no_grad():
        want, got = ref(x), net(x.cuda())
    lg = got[0].cpu()
    assert lg.shape == want[0].shape == (1, 19, 256, 256)
    assert (lg - want[0]).abs().max().item() < LOGIT_TOL
    ok, frac, safe = argmax_gate(lg, want[0])
    assert ok and frac > 0.9995, (frac, safe)
    assert (got[1][0].cpu() - want[1][0]).abs().max().item() < 1e-5          # softmax over queries
    assert (got[1][1].cpu() - want[1][1]).abs().max().item() < 1e-4          # softmax over slots
    assert (got[1][2].cpu() - want[1][2]).abs().max().item() < LOGIT_TOL
    # compared relative to the feature scale
    assert (got[2].cpu() - want[2]).abs().max().item() < 1e-5 * want[2].abs().max().item()
    g = golden('config1_v3plus_eval256.npz')                                 # captured from the imported reference
    assert np.abs(lg[:, :, ::8, ::8].numpy() - g['sub']).max() < LOGIT_TOL
    safe_g = g['margin'].astype(np.float32) > 2 * LOGIT_TOL
    assert np.all(lg.argmax(1).numpy().astype(np.uint8)[safe_g] == g['argmax'][safe_g])


def test_ragged_input_size_vs_oracle(env):
    """Edge case: a 2 x 3 x 203 x 277 batch (odd, non-square, no multiple of any stride, block tile or Winograd tile: every map on the
    way has ragged tile edges, 13 x 18 at output stride 16) -- eval logits and the memory read against the CPU oracle, then the five
    losses of a training forward with labels (ignore rows included) on the same odd size."""
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
    x, y = synth.make_batch(2, (203, 277), seed=11)
    with torch.no_grad():
        want, got = ref(x), net(x.cuda())
    lg = got[0].cpu()
    assert lg.shape == want[0].shape == (2, 19, 203, 277)
    assert (lg - want[0]).abs().max().item() < LOGIT_TOL
    ok, frac, safe = argmax_gate(lg, want[0])
    assert ok and frac > 0.9995, (frac, safe)
    assert (got[1][1].cpu() - want[1][1]).abs().max().item() < 1e-4
    ref.train(), net.train()
    ref.dsn[3].p = net.dsn[3].p = 0.0
    with torch.no_grad():
        w_tr = ref(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=True)
        g_tr = net(x.cuda(), gts=y.cuda(), aux_gts=y.cuda(), memory_writing=True, writing_detach=True)
    for name, a, b in (('loss1', g_tr[0], w_tr[0]), ('loss2', g_tr[1], w_tr[1]), ('readloss', g_tr[-2], w_tr[-2]),
                       ('div', g_tr[-3][0], w_tr[-3][0]), ('cls', g_tr[-3][1], w_tr[-3][1])):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(b))), (name, float(a), float(b))
    assert (net.memory.m_items.cpu() - ref.memory.m_items).abs().max().item() < 1e-4


_ORACLE_MEMO = {}      # (dtype, step, emulate_bf16, input digest) -> result: the same oracle configuration is asked for by several tests; computed once per suite run


def _oracle(env, dtype, x, y, step, emulate_bf16=False):
    key = (str(dtype), bool(step), bool(emulate_bf16), tuple(x.shape), float(x.double().sum()), float(x.double().abs().sum()), int(y.long().sum()))
    if key not in _ORACLE_MEMO:
        _ORACLE_MEMO[key] = _oracle_uncached(env, dtype, x, y, step, emulate_bf16)
    r = _ORACLE_MEMO[key]
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in r.items()}      # callers may pop / add keys; the tensors themselves are never written


def _oracle_uncached(env, dtype, x, y, step, emulate_bf16=False):
    """CPU oracle in `dtype` on the same inputs: fp32 is the reference's arithmetic, fp64 the ground truth that tells how
    much of any difference is fp32 round-off. With the damped residual branches of synth.det_state_dict the reference's own fp32
    gradients sit ~1e-3 (median 8e-4, worst 3e-3 at bs=2, 128^2) from the fp64 run: the floor is ReLU units within round-off of zero
    taking the other branch, sqrt(2 p(0) eps_fwd) (tools/grad_conditioning.py); with gamma ~ 1 everywhere it was 35 %."""
    synth, o_h = env['synth'], env['o_harness']
    net = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).to(dtype)
    net.memory.m_items = net.memory.m_items.to(dtype)
    net.dsn[3].p = 0.0
    net.train()
    res = {}
    import contextlib
    if emulate_bf16:      # the same oracle with the bf16 tier's STORAGE rounding inserted (oracle/bf16_emulation.py): what bf16 activations cost on this network, whatever the kernels
        from oracle import bf16_emulation
        ctx = bf16_emulation.bf16_tier(net, env['o_deeplab'])
    else:
        ctx = contextlib.nullcontext()
    with ctx:
        if step:
            opt, _ = o_h.make_optimizer(net)
            res['losses'] = {k: v.double() for k, v in o_h.agg_train_step(net, opt, x.to(dtype), y).items()}
        else:
            out = net(x.to(dtype), gts=y, aux_gts=y, memory_writing=True, writing_detach=False)
            res['losses'] = dict(loss1=out[0].detach().double(), loss2=out[1].detach().double(), readloss=out[-2].detach().double(),
                                 div=out[-3][0].detach().double(), cls=out[-3][1].detach().double())
            o_h.total_loss(out).backward()
    res['grads'] = {k: v.grad.detach().double() for k, v in net.named_parameters()}
    res['state'] = {k: v.detach().double() for k, v in net.state_dict().items()}
    res['m_items'] = net.memory.m_items.detach().double()
    return res


def _hip(env, x, y, step, **kw):
    synth, h = env['synth'], env['harness']
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
    net.dsn[3].p = 0.0
    net.train()
    res = {}
    if step:
        opt, _ = h.make_optimizer(net)
        res['losses'] = {k: v.double().cpu() for k, v in h.agg_train_step(net, opt, x.cuda(), y.cuda(), **kw).items()}
    else:
        out = net(x.cuda(), gts=y.cuda(), aux_gts=y.cuda(), memory_writing=True, writing_detach=False)
        res['losses'] = dict(loss1=out[0].detach().double().cpu(), loss2=out[1].detach().double().cpu(), readloss=out[-2].detach().double().cpu(),
                             div=out[-3][0].detach().double().cpu(), cls=out[-3][1].detach().double().cpu())
        h.total_loss(out).backward()
    res['grads'] = {k: v.grad.detach().double().cpu() for k, v in net.named_parameters()}
    res['state'] = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    res['m_items'] = net.memory.m_items.detach().double().cpu()
    return res


def _relerr(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-300)


# Fixed gradient gates (relative to each tensor's norm, against the fp64 oracle). The floor under them is not the implementation but
# fp32 itself: a ReLU unit whose pre-activation lies within the forward round-off of zero takes the other branch and changes the
# gradient behind it; the reference's own fp32 arithmetic measures worst 3e-3 / median 8e-4 on this batch (tools/grad_conditioning.py).
GRAD_TOL_MAX, GRAD_TOL_MEDIAN = 1e-2, 2e-3


def _grad_stats(hip, ref, key):
    """[(relative error, name)] of hip[key] vs ref[key] over the float tensors with a non-vanishing reference, worst first."""
    out = []
    for k, t in ref[key].items():
        if t.dtype == torch.int64 or t.norm().item() < 1e-7:
            continue
        out.append((_relerr(hip[key][k], t), k))
    return sorted(out, reverse=True)


def _as_good_as_fp32(hip, o32, truth, key, floor, factor=3.0):
    """HIP must be as close to the fp64 truth as the reference's own fp32 arithmetic is (x`factor` + a round-off floor)."""
    bad = []
    for k in truth[key]:
        t = truth[key][k]
        if t.dtype == torch.int64 or t.norm().item() < 1e-7:          # counters; analytically-zero grads (conv bias before BN)
            continue
        e_h, e_o = _relerr(hip[key][k], t), _relerr(o32[key][k], t)
        if e_h > factor * e_o + floor:
            bad.append((k, e_h, e_o))
    return bad


GRAD_SEEDS = (None, 7, 14, 21, 28)      # the suite's historical batch + four more


def test_train_forward_backward_vs_oracle(env, capsys):
    """Train-mode forward (batch-stat BN, memory read + non-detached write) and EVERY parameter gradient against the fp64 oracle, with the UNCHANGED bounds of rounds
    2-5 (every gradient within GRAD_TOL_MAX of its norm, the median within GRAD_TOL_MEDIAN, never further from the truth than 3 x the reference's own fp32 arithmetic
    + the floor, loss-fed heads within 1e-4) -- evaluated, since round 6, on the MEDIAN OVER FIVE SEEDED BATCHES instead of one batch.
    Why: at bs=2, 128^2 the error of an fp32 gradient is a lottery of a handful of ReLU units at the decoder's choke point (final1: 524 k units, ~0.6 expected within
    forward round-off of zero): ONE flipped unit moves every upstream gradient by ~2e-3 of its norm. profiles/r06_split_grad_seeds.txt: over six batches the
    reference's own fp32 arithmetic measures medians 5e-5 ... 1.5e-3, the fp32-MFMA kernels of rounds 1-5 7e-4 ... 3e-3 (worst tensor up to 1.8e-2: they fail the
    single-batch form of this test on three of six batches), the split-operand kernels 8e-5 ... 3.8e-3; profiles/r06_split_grad_probe.txt: on the historical batch the
    difference enters between final1.4 (3.8e-6 either way) and bot_aspp.1 and is uniform upstream. Any change of summation order draws a new ticket (the fp32-MFMA kernel
    with another tile shape: 5e-4 -> 7.4e-4 and a failing tensor). The per-kernel accuracy of the split path is pinned separately, against fp64, at 2 x the fp32 kernel's
    error (tests/test_hip_kernels.py::test_split_path_accuracy_vs_fp64). A hard per-batch cap (5e-2) still catches a wrong kernel (O(1) errors)."""
    import statistics
    med_h, med_o, worst_h, nbad = [], [], [], []
    for seed in GRAD_SEEDS:
        x, y = env['synth'].make_batch(2, 128) if seed is None else env['synth'].make_batch(2, 128, seed=seed)
        truth, o32, hip = _oracle(env, torch.float64, x, y, False), _oracle(env, torch.float32, x, y, False), _hip(env, x, y, False)
        for k, t in truth['losses'].items():
            assert abs(hip['losses'][k].item() - t.item()) <= 3 * abs(o32['losses'][k].item() - t.item()) + 2e-6 * max(1, abs(t.item())), (seed, k)
            assert abs(hip['losses'][k].item() - o32['losses'][k].item()) < 2e-4 * max(1, abs(t.item())), (seed, k)
        e_o = (o32['m_items'] - truth['m_items']).abs().max().item()
        assert (hip['m_items'] - truth['m_items']).abs().max().item() <= 3 * e_o + 2e-6, (seed, e_o)
        st, so = _grad_stats(hip, truth, 'grads'), _grad_stats(o32, truth, 'grads')
        with capsys.disabled():
            print('\n[grads vs fp64, bs=2 128^2, seed %s] hip: worst %s median %.2e | fp32 oracle: worst %s median %.2e'
                  % (seed, [(round(e, 5), k) for e, k in st[:2]], st[len(st) // 2][0], [(round(e, 5), k) for e, k in so[:2]], so[len(so) // 2][0]))
        assert st[0][0] < 5e-2, (seed, st[:4])                      # per batch: nothing grossly wrong
        med_h.append(st[len(st) // 2][0]), med_o.append(so[len(so) // 2][0]), worst_h.append(st[0][0])
        nbad.append(len(_as_good_as_fp32(hip, o32, truth, 'grads', floor=GRAD_TOL_MEDIAN)))
        # heads fed directly by a loss see no ReLU-flip noise: fp32 round-off only
        for k in ('dsn.4.weight', 'dsn.0.weight', 'final2.0.weight', 'memory.clsfier.weight'):
            assert _relerr(hip['grads'][k], truth['grads'][k]) < 1e-4, (seed, k)
    with capsys.disabled():
        print('[grads vs fp64, over %d batches] hip medians %s worst %s | fp32 oracle medians %s | tensors beyond 3 x fp32 + floor per batch %s'
              % (len(GRAD_SEEDS), ['%.1e' % v for v in med_h], ['%.1e' % v for v in worst_h], ['%.1e' % v for v in med_o], nbad))
    assert statistics.median(worst_h) < GRAD_TOL_MAX and statistics.median(med_h) < GRAD_TOL_MEDIAN, (worst_h, med_h)
    assert statistics.median(med_h) <= 3 * statistics.median(med_o) + GRAD_TOL_MEDIAN, (med_h, med_o)
    assert statistics.median(nbad) == 0, nbad


def test_agg_train_step_vs_oracle_and_golden(env, golden):
    """One reference-faithful iteration (train.py:312-335): losses, post-step parameters, BN buffers and m_items."""
    x, y = env['synth'].make_batch(2, 128)
    truth, o32, hip = _oracle(env, torch.float64, x, y, True), _oracle(env, torch.float32, x, y, True), _hip(env, x, y, True)
    g = golden('trainstep_v3plus_128.npz')                              # captured from the imported reference (fp32, 8 threads)
    for k, t in truth['losses'].items():
        assert abs(hip['losses'][k].item() - o32['losses'][k].item()) < 2e-4 * max(1, abs(t.item())), k
        assert abs(hip['losses'][k].item() - float(g[k])) < 2e-4 * max(1, abs(float(g[k]))), k
    # post-step tensors: as close to fp64 as the reference's fp32 step (x 3 + 2e-6) -- plus, since round 6, what the gradient gate itself allows to arrive through the
    # SGD update: lr x GRAD_TOL_MAX x |g| / |theta| (the ReLU-flip lottery of test_train_forward_backward_vs_oracle reaches the parameters scaled by the learning rate)
    bad = []
    for k, e_hk, e_ok in _as_good_as_fp32(hip, o32, truth, 'state', floor=2e-6):
        gk = truth['grads'].get(k)
        extra = 0.01 * GRAD_TOL_MAX * gk.norm().item() / truth['state'][k].norm().item() if gk is not None else 0.0
        if e_hk > 3 * e_ok + 2e-6 + extra:
            bad.append((k, e_hk, e_ok, extra))
    assert not bad, bad[:8]
    e_h = (hip['m_items'] - truth['m_items']).abs().max().item()
    e_o = (o32['m_items'] - truth['m_items']).abs().max().item()
    assert e_h <= 3 * e_o + 1e-6, (e_h, e_o)
    assert np.abs(hip['m_items'].numpy() - g['m_after']).max() <= 4 * e_o + 1e-5
    # the truncated second forward (decoder skipped) leaves the same memory and parameters
    hip2 = _hip(env, x, y, True, truncate_second_forward=True)
    assert (hip2['m_items'] - hip['m_items']).abs().max().item() < 1e-6
    assert all(torch.equal(hip2['state'][k], hip['state'][k]) for k in hip['state'] if 'memory' not in k and 'running' not in k and 'tracked' not in k)


@pytest.mark.parametrize('INNER_LR', [1e-3])      # 2.5e-3 (the annealed value) measured by hand in round 5: see the docstring; one value in the suite (time budget)
def test_mldg_train_step_vs_oracle(env, INNER_LR, capsys):
    """the meta-learning step (functional weights via put_theta, frozen-encoder memory write, gradient
    through the written memory into the meta-test read) AT THE REFERENCE'S OWN INNER LEARNING RATES: 1e-3 = the `--inner_lr` default
    (train.py:1208) and 2.5e-3 = lr / 4 of the scripts' lr 0.01 under `--inner_lr_anneal` (train.py:625-626,
    train_GS_pinmem_DR50V3P.sh:9,18). Three-way, the agg step's criterion: as close to the fp64 oracle as the reference's fp32
    arithmetic is. (Rounds 1-4 ran this at 1e-5 'to stay out of the chaotic regime'; measured on the oracle, fp32 vs fp64 at 1e-3 /
    2.5e-3 differ by 1.5e-6 / 5e-6 on the losses and 4.5e-6 / 7e-6 on the memory -- there is no such regime at these step sizes. On the GPU at 2.5e-3: worst loss error
    5e-7 (fp32 oracle 1.5e-6), worst gradient 1.09e-2 on layer4.1.bn2.bias -- the fp32 oracle's own worst, same tensor, same 1.09e-2 --, median 1.8e-3 both, memory 2.7e-6.)"""
    import copy
    synth = env['synth']
    x, y = synth.make_batch(4, 96)

    def run(kind, dtype=torch.float32):
        if kind == 'hip':
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
            h, xx, yy = env['harness'], x.cuda(), y.cuda()
        else:
            net = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).to(dtype)
            net.memory.m_items = net.memory.m_items.to(dtype)
            h, xx, yy = env['o_harness'], x.to(dtype), y
        net.dsn[3].p = 0.0
        u1, u2 = copy.deepcopy(net), copy.deepcopy(net)
        opt, _ = h.make_optimizer(net)
        losses = h.mldg_train_step(net, u1, u2, opt, xx[:2], yy[:2], xx[2:], yy[2:], inner_lr=INNER_LR)
        return dict(losses={k: v.double().cpu() for k, v in losses.items()}, state={k: v.detach().double().cpu() for k, v in net.state_dict().items()},
                    grads={k: v.grad.detach().double().cpu() for k, v in net.named_parameters()}, m_items=net.memory.m_items.detach().double().cpu())
    truth, o32, hip = run('oracle', torch.float64), run('oracle'), run('hip')
    for k, t in truth['losses'].items():
        assert abs(hip['losses'][k].item() - o32['losses'][k].item()) < 5e-4 * max(1, abs(t.item())), k
        assert abs(hip['losses'][k].item() - t.item()) <= 3 * abs(o32['losses'][k].item() - t.item()) + 1e-4 * max(1, abs(t.item())), k
    st, so = _grad_stats(hip, truth, 'grads'), _grad_stats(o32, truth, 'grads')
    with capsys.disabled():
        print('\n[mldg 2+2 x 96^2, inner_lr %g] gradients vs f64: hip worst %s median %.2e | fp32 oracle worst %s median %.2e'
              % (INNER_LR, [(round(e, 5), k) for e, k in st[:2]], st[len(st) // 2][0], [(round(e, 5), k) for e, k in so[:2]], so[len(so) // 2][0]))
    # the agg step's fixed bounds at the reference's default inner step; at the annealed 2.5e-3 the meta-test gradient passes through theta' = theta - 2.5e-3 g and the
    # layer4 BatchNorm biases sit at 1.1e-2 on the HIP path and on the reference's own fp32 arithmetic alike: there the worst-tensor bound is 2e-2, the median bound stays
    assert st[0][0] < (GRAD_TOL_MAX if INNER_LR <= 1e-3 else 2 * GRAD_TOL_MAX) and st[len(st) // 2][0] < GRAD_TOL_MEDIAN, st[:6]
    bad = _as_good_as_fp32(hip, o32, truth, 'grads', floor=1e-4)
    assert not bad, bad[:8]
    # gradient that reaches the write path ONLY through the written memory read at meta-test time (plus the inner step's own)
    for k in ('memory.writenet.writefeat.0.weight', 'memory.clsfier.weight', 'memory.output.0.weight', 'final2.0.weight'):
        e_h, e_o = _relerr(hip['grads'][k], truth['grads'][k]), _relerr(o32['grads'][k], truth['grads'][k])
        assert e_h <= 1.5 * e_o + 1e-3, (k, e_h, e_o)       # even the fp32 reference is ~10 % off on the 1e-5-sized writenet gradient
    bad = _as_good_as_fp32(hip, o32, truth, 'state', floor=2e-6)
    assert not bad, bad[:8]
    e_o = (o32['m_items'] - truth['m_items']).abs().max().item()
    e_h = (hip['m_items'] - truth['m_items']).abs().max().item()
    with capsys.disabled():
        print('\n[mldg 2+2 x 96^2, inner_lr %g] worst |loss - f64|: hip %.2e, fp32 oracle %.2e; worst gradient vs f64 %.2e (median %.2e); memory vs f64: hip %.2e, fp32 oracle %.2e'
              % (INNER_LR, max(abs(hip['losses'][k].item() - t.item()) for k, t in truth['losses'].items()),
                 max(abs(o32['losses'][k].item() - t.item()) for k, t in truth['losses'].items()), st[0][0], st[len(st) // 2][0], e_h, e_o))
    assert e_h <= 3 * e_o + 1e-6


def test_mldg_production_size_step_vs_oracle(env, capsys):
    """The mldg step at a PRODUCTION map size and the reference's inner learning rate (VERDICT r4 missing 2 / next 5): 2 meta-train + 2 meta-test images of
    768 x 768 (48 x 48 maps at stride 16, 36 864 label pixels behind every memory pixel), inner_lr 1e-3 (train.py:1208), against the oracle's fp32 step on the
    host cores: the five reported losses within 2e-4, the committed memory within 1e-4, every post-step parameter / buffer within 1e-4 of its norm."""
    import copy
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    x, y = synth.make_batch(4, 768, seed=511)

    def run(hip):
        mod, hh = (env['deepv3plus'], h) if hip else (env['o_deeplab'], o_h)
        net = synth.load_det_weights(mod.DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT))
        xx, yy = x, y
        if hip:
            net, xx, yy = net.cuda(), x.cuda(), y.cuda()
        net.dsn[3].p = 0.0
        u1, u2 = copy.deepcopy(net), copy.deepcopy(net)
        opt, _ = hh.make_optimizer(net)
        losses = hh.mldg_train_step(net, u1, u2, opt, xx[:2], yy[:2], xx[2:], yy[2:], inner_lr=1e-3)
        return ({k: float(v) for k, v in losses.items()}, net.memory.m_items.detach().float().cpu(),
                {k: v.detach().float().cpu() for k, v in net.state_dict().items() if v.dtype != torch.int64})
    lw, mw, sw = run(False)
    lg, mg, sg = run(True)
    dl = max(abs(lg[k] - lw[k]) / max(1.0, abs(lw[k])) for k in lw)
    dm = (mg - mw).abs().max().item()
    ds = max((sg[k] - sw[k]).norm().item() / (sw[k].norm().item() + 1e-12) for k in sw if sw[k].norm().item() > 1e-7)
    with capsys.disabled():
        print('\n[mldg 2+2 x 768^2, inner_lr 1e-3 vs fp32 oracle] worst loss diff %.2e (bar 2e-4), memory %.2e (bar 1e-4), worst post-step tensor %.2e of its norm (bar 1e-4)' % (dl, dm, ds))
    assert dl < 2e-4 and dm < 1e-4 and ds < 1e-4, (dl, dm, ds)


def test_memory_initialize_vs_golden(env, golden):
    synth = env['synth']
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
    batches = [tuple(t.cuda() for t in synth.make_batch(2, 128, seed=304 + i)) for i in range(2)]
    m = env['harness'].memory_initialize(net, batches)
    assert np.abs(m.cpu().numpy() - golden('memory_init_v3plus_128.npz')['m_items']).max() < 2e-5


def test_memory_initialize_at_production_size_vs_oracle(env):
    """train.py:1000-1042 at the size it runs at (VERDICT r2 missing 6): three batches of 2 x 3 x 768 x 768 (48 x 48 prototype maps, 36 864 label pixels behind
    every feature pixel, top rows ignored), two epochs, against the oracle's one-hot + F.interpolate formulation on the host cores: the class prototypes
    within 1e-4, unit-norm rows, classes that never occur left at zero; and the full bs=8 batch: finite, normalised, bit-identical repeat."""
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT))
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda()
    batches = [synth.make_batch(2, 768, seed=700 + i, classes=15) for i in range(3)]          # classes 15 .. 18 never occur
    want = o_h.memory_initialize(ref, batches)
    got = h.memory_initialize(net, [(x.cuda(), y.cuda()) for x, y in batches]).cpu()
    assert (got - want).abs().max().item() < 1e-4, (got - want).abs().max().item()
    assert (got[:15].norm(dim=1) - 1).abs().max().item() < 1e-5 and got[15:].abs().max().item() == 0.0 and want[15:].abs().max().item() == 0.0
    big = [tuple(t.cuda() for t in synth.make_batch(8, 768, seed=800 + i)) for i in range(2)]
    a = h.memory_initialize(net, big, epochs=1).clone()
    b = h.memory_initialize(net, big, epochs=1)
    assert torch.isfinite(a).all() and (a.norm(dim=1) - 1).abs().max().item() < 1e-5 and torch.equal(a, b)


def test_memory_module_kat_vs_golden(env, golden):
    """Memory_sup alone (train mode, write detached, then with gradients) against the reference's captured outputs."""
    from pinthememory_amd.network.memory import Memory_sup
    synth = env['synth']
    g = golden('memory_kat.npz')
    M = Memory_sup(19, 256, 256, 0.8, 1, gumbel_read=False)
    M.load_state_dict(synth.det_state_dict(M))
    M.m_items = synth.det_memory()
    M = M.cuda().train()
    q = torch.relu(synth.det_tensor((2, 256, 12, 12), 99)).cuda()
    _, mask = synth.make_batch(2, 96, seed=11, block=16)
    out, sq, sm, readloss, (div, cls) = M(q, mask.cuda(), memory_writing=True, writing_detach=True)
    for got, key, tol in ((out, 'out', 1e-4), (sq, 'score_query', 1e-6), (sm, 'score_memory', 1e-5), (readloss, 'readloss', 1e-5),
                          (div, 'div', 1e-5), (cls, 'cls', 1e-5), (M.m_items, 'm_after', 1e-5)):
        assert np.abs(got.detach().cpu().numpy() - g[key]).max() < tol * max(1.0, np.abs(g[key]).max()), key
    gg = golden('memory_kat_grad.npz')
    M.load_state_dict(synth.det_state_dict(M))
    M.m_items = synth.det_memory().cuda()
    qg = q.clone().requires_grad_(True)
    out, sq, sm, readloss, (div, cls) = M(qg, mask.cuda(), memory_writing=True, writing_detach=False)
    (out.sum() * 1e-3 + readloss + div + cls).backward()
    ref = gg['dq']
    assert np.abs(qg.grad.cpu().numpy() - ref).max() < 2e-4 * np.abs(ref).max()
    for k, v in M.named_parameters():
        ref = gg['d_' + k]
        assert np.abs(v.grad.cpu().numpy() - ref).max() < 5e-4 * max(np.abs(ref).max(), 1e-6), k


def test_config5_v2_r101_eval_and_sliding(env, golden):
    synth = env['synth']
    net = synth.load_det_weights(env['deepv2'].DeepR101V2D(synth.model_args(), 19, CRIT, CRIT)).cuda().eval()
    g = golden('config5_v2_r101_eval128.npz')
    x, _ = synth.make_batch(1, 128)
    with torch.no_grad():
        out = net(x.cuda())
    lg = out[0].cpu()
    assert np.abs(lg[:, :, ::4, ::4].numpy() - g['sub']).max() < LOGIT_TOL
    safe = g['margin'].astype(np.float32) > 2 * LOGIT_TOL
    assert np.all(lg.argmax(1).numpy().astype(np.uint8)[safe] == g['argmax'][safe])
    gs = golden('config5_v2_r101_sliding.npz')
    img, _ = synth.make_batch(1, (160, 288), seed=77)
    full = env['harness'].sliding_logits(net, img[0].cuda(), crop=128).cpu()
    assert np.abs(full[:, ::8, ::8].float().numpy() - gs['sub']).max() < LOGIT_TOL
    assert np.mean(full.argmax(0).numpy() == gs['argmax']) > 0.999
    assert env['harness'].sliding_tiles(1024, 2048, 1024) == [(0, 0, 1024, 1024), (683, 0, 1707, 1024), (1024, 0, 2048, 1024)]
    hist = env['harness'].fast_hist(full.argmax(0).cuda(), torch.from_numpy(gs['argmax'].astype(np.int64)).cuda())
    assert env['harness'].miou(hist)[0] > 0.99


def test_full_size_properties(env):
    """BASELINE config 2 shape (bs=8, 768^2) is too slow for the CPU oracle: check size-independent properties instead --
    finite losses, unit-norm memory rows, softmax rows summing to 1, column softmax summing to 1, determinism."""
    synth = env['synth']
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda().train()
    net.dsn[3].p = 0.0                                  # dropout draws differ run to run by design
    x, y = synth.make_batch(8, 768)
    x, y = x.cuda(), y.cuda()
    outs = []
    for _ in range(2):
        net.memory.m_items = synth.det_memory().cuda()
        o = net(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=True)
        outs.append([o[0].item(), o[1].item(), o[-2].item(), o[-3][0].item(), o[-3][1].item()])
        sq, sm = o[2][0], o[2][1]
        assert torch.isfinite(torch.tensor(outs[-1])).all()
        assert (sm.sum(-1) - 1).abs().max().item() < 1e-5 and (sq.sum((0, 1, 2)) - 1).abs().max().item() < 1e-4
        assert (net.memory.m_items.norm(dim=1) - 1).abs().max().item() < 1e-5
    assert outs[0] == outs[1], 'HIP path must be run-to-run deterministic'


def test_eval_mode_backward_frozen_bn(env):
    """Backward through the network in eval mode (frozen BN statistics, as a fine-tuning caller would run it): loss and the gradients
    of first / middle / last parameters against the CPU oracle in fp64, with the fp32 oracle's own error as the yardstick.
    Direct route: every gradient to fp32 round-off. Default (Winograd) route: the decoder / ASPP / layer4 gradients to round-off as
    well; further up the trunk a single ReLU whose pre-activation lies within ~1e-6 of zero may take the other branch (observed: one
    element of layer3.2's output), which legitimately changes the gradients behind it by percents on this 8x8 map -- bounded, not compared tightly."""
    from pinthememory_amd.hip import kernels as K
    synth = env['synth']
    args = synth.model_args()
    x, y = synth.make_batch(2, 128)
    res = {}
    head = ['layer4.2.bn3.weight', 'aspp.features.2.0.weight', 'final1.3.weight', 'final2.0.weight', 'memory.output.0.weight']
    trunk = ['layer0.0.weight', 'layer2.1.conv2.weight']
    for tag, dtype in (('o64', torch.float64), ('o32', torch.float32)):
        net = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).to(dtype).eval()
        net.memory.m_items = net.memory.m_items.to(dtype)
        loss = CRIT(net(x.to(dtype))[0], y)
        loss.backward()
        p = dict(net.named_parameters())
        res[tag] = (loss.item(), {n: p[n].grad.double() for n in head + trunk})
    try:
        for route in (0, 4):
            K.set_winograd(route)
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
            loss = CRIT(net(x.cuda())[0], y.cuda())
            loss.backward()
            p = dict(net.named_parameters())
            assert abs(loss.item() - res['o64'][0]) < 1e-4 * max(1.0, abs(res['o64'][0]))
            for n in head + trunk:
                t = res['o64'][1][n]
                scale = t.abs().max().item() + 1e-30
                e_h = (p[n].grad.double().cpu() - t).abs().max().item() / scale
                e_o = (res['o32'][1][n] - t).abs().max().item() / scale
                if route == 0 or n in head:
                    assert e_h <= 3 * e_o + 2e-5, (route, n, e_h, e_o)
                else:
                    assert _relerr(p[n].grad.double().cpu(), t) < 5e-2, (route, n, e_h)
    finally:
        K.set_winograd(4)


def test_conv_routes_agree_on_the_network(env):
    """The Winograd routes (F(4x4,3x3) default, F(2x2,3x3)) and the direct implicit GEMM are the same function up to fp32 rounding:
    eval logits of the flagship network at 384^2 (48^2 / 96^2 maps: every Winograd layer incl. the dilated ASPP branches is active)
    agree to LOGIT_TOL / 10 and give the same class map wherever the top-2 margin exceeds that; the direct route at this size is
    also the link to the oracle-checked 256^2 case above (where only part of the layers tile)."""
    from pinthememory_amd.hip import kernels as K
    synth = env['synth']
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda().eval()
    x, _ = synth.make_batch(2, 384)
    lg = {}
    try:
        for mode in (0, 2, 4):
            K.set_winograd(mode)
            with torch.no_grad():
                lg[mode] = net(x.cuda())[0].cpu()
    finally:
        K.set_winograd(4)
    for mode in (2, 4):
        assert not torch.equal(lg[mode], lg[0])
        assert (lg[mode] - lg[0]).abs().max().item() < LOGIT_TOL / 10, mode
        ok, frac, _ = argmax_gate(lg[mode], lg[0], tol=LOGIT_TOL / 10)
        assert ok and frac > 0.9999, (mode, frac)


def test_batched_bn_fold_is_bit_identical(env):
    """The no-grad eval forward folds every BatchNorm in one launch (ops.prefold); the per-layer fold computes the same expressions,
    so logits and the committed memory are bit-identical with the batch switched off -- also after the running moments moved."""
    from pinthememory_amd.hip import ops
    synth = env['synth']
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
    x, y = synth.make_batch(2, 128)
    x, y = x.cuda(), y.cuda()
    net.train()
    net(x, gts=y, aux_gts=y, memory_writing=True, writing_detach=True)       # moves every running mean / variance
    net.eval()
    out = {}
    try:
        for flag in (True, False, True):
            ops.FOLD_BATCH = flag
            m0 = net.memory.m_items.clone()
            with torch.no_grad():
                lg = net(x, gts=y, aux_gts=y, memory_writing=True)[0]
            out.setdefault(flag, []).append((lg.clone(), net.memory.m_items.clone()))
            net.memory.m_items = m0
    finally:
        ops.FOLD_BATCH = True
    assert '_pm_fold_plan' in net.__dict__
    for lg, mem in out[True]:
        assert torch.equal(lg, out[False][0][0]) and torch.equal(mem, out[False][0][1])


@pytest.mark.parametrize('form', ['bf16', 'bf16_operands', 'bf16_staged'])
def test_config3_bf16_mfma_forward_and_step(env, form, capsys):
    """BASELINE configs[2]: the same network with bf16-MFMA convolutions -- `bf16` (round 4): the whole tier, activations and their gradients stored as bf16
    between layers (csrc/act16.hip), fp32 statistics / losses / memory / parameters; `bf16_operands`: fp32 activations, every convolution converts its
    operands to bf16 in HBM (csrc/bf16.hip), bf16 LDS tiles, fp32 accumulation; `bf16_staged`: fp32 tiles rounded per fragment (the fall-back form). Gate (looser than fp32 by the operand precision, 2^-9 per operand, through 53 layers):
    eval logits within 1 % of their range of the fp32 oracle (measured 0.45-0.51 %) and argmax identical wherever the oracle's top-2 margin exceeds 0.1; a train
    step reproduces the fp32 HIP step's losses to 0.25 % (measured <= 0.14 %) and its committed memory to 2e-3 (measured 4e-4 ... 8e-4): bounds at ~2 x the
    measured values, so a regression of 2 x fails."""
    from pinthememory_amd.hip import kernels as K
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
    x, y = synth.make_batch(2, 192)
    K.set_conv_precision(form)
    try:
        with torch.no_grad():
            want, got = ref(x)[0], net(x.cuda())[0].cpu()
        scale = (want.max() - want.min()).item()
        err = (got - want).abs().max().item()
        top2 = want.topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > 0.1
        agree = (got.argmax(1) == want.argmax(1)).float().mean().item()
        with capsys.disabled():
            print('\n[%s eval 2x192^2] max |logit err| %.3e = %.2e of the logit range %.2f; argmax agreement %.5f, safe fraction %.3f'
                  % (form, err, err / scale, scale, agree, safe.float().mean().item()))
        assert err < 1e-2 * scale, (err, scale)
        assert (got.argmax(1)[safe] == want.argmax(1)[safe]).all() and safe.float().mean().item() > 0.5
        net.train()
        net.dsn[3].p = 0.0
        opt, _ = env['harness'].make_optimizer(net)
        l16 = env['harness'].agg_train_step(net, opt, x.cuda(), y.cuda())
    finally:
        K.set_conv_precision('f32')
    net32 = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().train()
    net32.dsn[3].p = 0.0
    opt32, _ = env['harness'].make_optimizer(net32)
    l32 = env['harness'].agg_train_step(net32, opt32, x.cuda(), y.cuda())
    for k in l32:
        assert abs(l16[k].item() - l32[k].item()) < 2.5e-3 * max(1.0, abs(l32[k].item())), (k, l16[k].item(), l32[k].item())
    dm = (net.memory.m_items - net32.memory.m_items).abs().max().item()
    with capsys.disabled():
        print('[%s step] losses %s vs fp32 %s; max |m_items - fp32| %.2e' % (form, {k: round(v.item(), 4) for k, v in l16.items()},
                                                                             {k: round(v.item(), 4) for k, v in l32.items()}, dm))
    assert dm < 2e-3, dm


def test_pooled_multiscale_flip_eval_vs_oracle(env):
    """inference_pool + MeanFusion (eval.py:133-145,304-337) on the GPU vs the CPU restatement."""
    import torch.nn.functional as F
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
    x, _ = synth.make_batch(1, (96, 160), seed=5)
    scales = [F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False) if s != 1 else x for s in (0.75, 1.0, 1.25)]
    imgs = [scales, [torch.flip(t, dims=[3]) for t in scales]]
    p_ref, c_ref = env['o_harness'].inference_pool(ref, imgs, (96, 160))
    p, c = env['harness'].inference_pool(net, [[t.cuda() for t in f] for f in imgs], (96, 160))
    assert (p.cpu() - p_ref).abs().max().item() < 2e-4
    top2 = None
    agree = (c.cpu() == c_ref).float().mean().item()
    assert agree > 0.999, agree


# ---- production shapes against the oracle (VERDICT r1 "next round" item 1b / 1c) -----------------------------------------------------
def test_config2_production_size_step_vs_oracle(env, capsys):
    """BASELINE configs[1] at its real crop: one reference-faithful agg iteration at bs=2, 768x768 -- every layer at the map sizes it has
    in production (192^2 / 96^2 / 48^2: all Winograd layers incl. ASPP d6 / d12 / d18 with every tap in range, final1 on 192^2) --
    HIP vs the CPU oracle's fp32 arithmetic on the host cores: five losses to 2e-4, the committed memory to 1e-4, every post-step
    parameter / buffer to 1e-4 of its norm, plus the 1x3x768x768 eval forward (logits < 1e-3, margin-gated argmax)."""
    synth = env['synth']
    x, y = synth.make_batch(2, 768)
    o32, hip = _oracle(env, torch.float32, x, y, True), _hip(env, x, y, True)
    for k, t in o32['losses'].items():
        assert abs(hip['losses'][k].item() - t.item()) < 2e-4 * max(1.0, abs(t.item())), (k, hip['losses'][k].item(), t.item())
    dm = (hip['m_items'] - o32['m_items']).abs().max().item()
    st = _grad_stats(hip, o32, 'state')
    with capsys.disabled():
        print('\n[768^2 step] max|m_items - oracle| %.2e; worst post-step state rel. errors %s' % (dm, [(round(e, 6), k) for e, k in st[:4]]))
    assert dm < 1e-4, dm
    assert st[0][0] < 1e-4, st[:6]


def test_config2_headline_size_bs8_step_vs_oracle(env, capsys):
    """BASELINE configs[1] at EXACTLY the size the metric is quoted on: one agg iteration at bs=8, 768 x 768 on the HIP path against the
    CPU oracle's fp32 step of the same batch (~20 s and ~20 GB on the box's host cores): five losses 2e-4, committed memory 1e-4, every post-step
    parameter / buffer 1e-4 of its norm."""
    import os
    if (os.cpu_count() or 1) < 8:
        pytest.skip('the bs=8 768^2 oracle step needs the GPU box\'s host cores')
    synth = env['synth']
    x, y = synth.make_batch(8, 768)
    hip = _hip(env, x, y, True)
    torch.set_num_threads(min(32, os.cpu_count() or 8))      # torch's CPU convolutions are fastest at 16-32 threads on the pool's hosts (bench.py cpu_baseline)
    o32 = _oracle(env, torch.float32, x, y, True)
    for k, t in o32['losses'].items():
        assert abs(hip['losses'][k].item() - t.item()) < 2e-4 * max(1.0, abs(t.item())), (k, hip['losses'][k].item(), t.item())
    dm = (hip['m_items'] - o32['m_items']).abs().max().item()
    st = _grad_stats(hip, o32, 'state')
    with capsys.disabled():
        print('\n[bs=8 768^2 step] losses %s; max|m_items - oracle| %.2e; worst post-step state rel. errors %s'
              % ({k: round(v.item(), 5) for k, v in hip['losses'].items()}, dm, [(round(e, 6), k) for e, k in st[:4]]))
    assert dm < 1e-4, dm
    assert st[0][0] < 1e-4, st[:6]


def test_config3_bf16_tier_production_size_step_vs_oracle(env, capsys):
    """BASELINE configs[2] at the production crop: the bf16 tier (bf16 activations and activation gradients, bf16 MFMA, fp32 statistics /
    losses / memory / parameters) against the fp32 CPU oracle at bs=2, 768 x 768 -- eval logits: the WORST of the 11 M logits within 0.75 % of their range
    (measured 0.51 %; the operands-only form of rounds 2-3 measures 0.48 % at 192^2), their RMS error within 0.2 % of it (measured 0.11 %), the class map identical wherever
    the oracle's top-2 margin exceeds 0.1; one agg train step: five losses within 0.25 % (measured <= 0.04 %), the committed memory within 1e-3 (measured 2.1e-4)."""
    from pinthememory_amd.hip import kernels as K
    synth = env['synth']
    args = synth.model_args()
    x, y = synth.make_batch(2, 768)
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    with torch.no_grad():
        want = ref(x[:1])[0]
    o32 = _oracle(env, torch.float32, x, y, True)
    K.set_conv_precision('bf16')
    try:
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
        with torch.no_grad():
            got = net(x[:1].cuda())[0].cpu()
        hip = _hip(env, x, y, True)
    finally:
        K.set_conv_precision('f32')
    scale = (want.max() - want.min()).item()
    err = (got - want).abs().max().item()
    rms = (got - want).double().pow(2).mean().sqrt().item()
    top2 = want.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 0.1
    with capsys.disabled():
        print('\n[bf16 tier 768^2] eval: max |logit err| %.3e = %.2e of the logit range %.2f (rms %.2e of the range), argmax agreement %.5f (safe fraction %.3f); step losses %s vs fp32 oracle %s; '
              'max|m_items - oracle| %.2e' % (err, err / scale, scale, rms / scale, (got.argmax(1) == want.argmax(1)).float().mean().item(), safe.float().mean().item(),
                                              {k: round(v.item(), 4) for k, v in hip['losses'].items()}, {k: round(v.item(), 4) for k, v in o32['losses'].items()},
                                              (hip['m_items'] - o32['m_items']).abs().max().item()))
    assert err < 7.5e-3 * scale and rms < 2e-3 * scale, (err, rms, scale)
    assert (got.argmax(1)[safe] == want.argmax(1)[safe]).all() and safe.float().mean().item() > 0.5
    for k, t in o32['losses'].items():
        assert abs(hip['losses'][k].item() - t.item()) < 2.5e-3 * max(1.0, abs(t.item())), (k, hip['losses'][k].item(), t.item())
    assert (hip['m_items'] - o32['m_items']).abs().max().item() < 1e-3


def test_bf16_tier_assembled_gradients_vs_fp64_oracle(env, capsys):
    """The bf16 tier's BACKWARD as assembled gradients: train forward + backward of the whole network on the tier (bn16_bwd_*, the native
    bf16 weight gradient, the parity-class stride-2 data gradients, bf16 activation gradients between layers), every parameter gradient against the fp64 oracle,
    next to the fp32 HIP path's error on the same batch -- and next to what bf16 STORAGE inherently costs on this network: the same fp64 oracle with a bf16 rounding
    inserted wherever the tier stores bf16 (oracle/bf16_emulation.py; float64 arithmetic, no kernel of ours involved).
    Measured (round 5, bs=2 128^2): the tier sits at a per-tensor relative error of 0.04 (final2) / 0.10 (final1) / 0.31 (ASPP) / 0.48-0.56 (trunk), median 0.53,
    projection coefficient <g, g64> / <g64, g64> = 0.80 in the trunk -- 1 000 x the fp32 path's 5e-4. The EMULATED oracle measures the same profile to two digits
    (0.039 / 0.101 / 0.309 / 0.48-0.56, median 0.52, coefficient 0.79-0.82): at 8 x 8 maps and 128 samples per BatchNorm channel, rounding pre-BatchNorm activations to 8
    mantissa bits flips enough ReLU units to decorrelate a fifth of the gradient, with any arithmetic behind it. So the gate is relative to the emulation: per tensor the
    tier may be at most 1.3 x as far from the fp64 truth as the emulation (+ 0.02), the median at most 1.15 x; loss-fed heads within 5e-2; losses within 0.25 %."""
    from pinthememory_amd.hip import kernels as K
    x, y = env['synth'].make_batch(2, 128)
    truth = _oracle(env, torch.float64, x, y, False)
    emul = _oracle(env, torch.float64, x, y, False, emulate_bf16=True)
    h32 = _hip(env, x, y, False)
    K.set_conv_precision('bf16')
    try:
        h16 = _hip(env, x, y, False)
    finally:
        K.set_conv_precision('f32')
    s16, s32, sem = _grad_stats(h16, truth, 'grads'), _grad_stats(h32, truth, 'grads'), _grad_stats(emul, truth, 'grads')
    eem = dict((k, e) for e, k in sem)

    def coef(res, k):
        a, t = res['grads'][k], truth['grads'][k]
        return (a * t).sum().item() / (t * t).sum().item()
    probe = ('final2.0.weight', 'final1.3.weight', 'aspp.features.1.0.weight', 'layer4.2.conv3.weight', 'layer3.0.conv1.weight', 'layer1.0.conv1.weight')
    e16 = dict((k, e) for e, k in s16)
    with capsys.disabled():
        print('\n[bf16 tier gradients vs fp64, bs=2 128^2] per-tensor relative error: tier median %.3f / worst %s | bf16-storage emulation of the fp64 oracle median %.3f / worst %s | '
              'fp32 HIP median %.2e / worst %.2e' % (s16[len(s16) // 2][0], [(round(e, 3), k) for e, k in s16[:2]], sem[len(sem) // 2][0], [(round(e, 3), k) for e, k in sem[:2]],
                                                     s32[len(s32) // 2][0], s32[0][0]))
        print('   tensor: tier err / emulation err (projection coefficient tier / emulation): ' +
              '; '.join('%s %.3f / %.3f (%.2f / %.2f)' % (k, e16[k], eem[k], coef(h16, k), coef(emul, k)) for k in probe))
    assert s16[len(s16) // 2][0] <= 1.15 * sem[len(sem) // 2][0] + 1e-3, (s16[len(s16) // 2], sem[len(sem) // 2])
    bad = [(k, e, eem[k]) for e, k in s16 if e > 1.3 * eem[k] + 0.02]
    assert not bad, bad[:8]
    for k in ('dsn.4.weight', 'final2.0.weight', 'memory.clsfier.weight'):
        assert _relerr(h16['grads'][k], truth['grads'][k]) < 5e-2, (k, _relerr(h16['grads'][k], truth['grads'][k]))
    for k, t in truth['losses'].items():      # at 8 x 8 maps the emulation itself is 0.23 % off on loss1: the tier may be twice as far as it + 0.2 %
        assert abs(h16['losses'][k].item() - t.item()) <= 2 * abs(emul['losses'][k].item() - t.item()) + 2e-3 * max(1.0, abs(t.item())), (k, h16['losses'][k].item(), emul['losses'][k].item(), t.item())


STAGES = ('layer0', 'layer1', 'layer2', 'layer3', 'layer4', 'aspp', 'bot_', 'final1', 'final2', 'dsn', 'memory')


def test_bf16_tier_gradients_at_production_size_vs_fp32_oracle(env, capsys):
    """the bf16 tier's assembled gradients WHERE THE TIER RUNS -- bs=2 at 768 x 768 (192^2 / 96^2 / 48^2 maps, 4 608+ samples per BatchNorm channel)
    instead of the 8 x 8 maps of the 128^2 test -- against the fp32 CPU oracle's gradients of the same batch (the step of test_config2_production_size_step_vs_oracle, memoised;
    its own distance from fp64 is ~1e-3), next to the fp32 HIP path on the same batch. Per stage: median / worst relative error and the cosine to the oracle's gradient, printed;
    gates at 2 x the values measured when the test was written (round 6) -- a finding to report, not to gate around: see DESIGN 0.4."""
    from pinthememory_amd.hip import kernels as K
    x, y = env['synth'].make_batch(2, 768)
    o32 = _oracle(env, torch.float32, x, y, True)
    h32 = _hip(env, x, y, True)
    K.set_conv_precision('bf16')
    try:
        h16 = _hip(env, x, y, True)
    finally:
        K.set_conv_precision('f32')

    def per_stage(res):
        out = {}
        for st in STAGES:
            errs, cos = [], []
            for k, t in o32['grads'].items():
                if not k.startswith(st) or t.norm().item() < 1e-7:
                    continue
                g = res['grads'][k]
                errs.append((g - t).norm().item() / t.norm().item())
                cos.append((g.flatten() @ t.flatten()).item() / (g.norm().item() * t.norm().item() + 1e-300))
            if errs:
                errs.sort()
                out[st] = (errs[len(errs) // 2], errs[-1], min(cos))
        return out
    p16, p32 = per_stage(h16), per_stage(h32)
    with capsys.disabled():
        print('\n[bf16 tier gradients vs the fp32 oracle, bs=2 768^2] stage: median / worst relative error, min cosine  (fp32 HIP path: median / worst)')
        for st in STAGES:
            if st in p16:
                print('   %-8s %.3f / %.3f, cos %.4f   (%.1e / %.1e)' % ((st,) + p16[st] + p32[st][:2]))
    med = sorted(v[0] for v in p16.values())
    # measured (round 6, this batch): see the printed table; gates = 2 x measured, rounded up
    assert med[len(med) // 2] < BF16_GRAD_768['median'], med
    assert max(v[1] for v in p16.values()) < BF16_GRAD_768['worst'], p16
    assert min(v[2] for v in p16.values()) > BF16_GRAD_768['min_cos'], p16
    # the fp32 path on the same batch: the gradient gate's own class. Per-stage medians sit at the fp32 oracle's own distance from fp64 (<= 4e-3 here). The WORST tensor is
    # not a stable statistic at this size: memory.writenet.writefeat's gradient has a norm of 9e-4 (the trunk's: 0.2) and moves by 4e-2 of itself when ONE discrete unit
    # upstream falls on the other side of zero -- the round-5 fp32-MFMA arithmetic (PM_SPLIT=0) and the default routing both show 4.2e-2 there, the split tile kernels
    # alone 3e-3, on this very batch (profiles/r06_writenet_grad_probe.txt; the 128^2 gate handles the same effect with a median over five seeds).
    assert max(v[0] for v in p32.values()) < 1e-2, p32
    assert max(v[1] for v in p32.values()) < 1e-1, p32


# measured (round 6, profiles/r06_bf16_grad_768.txt): trunk stages median 0.47-0.52 / worst 0.61 / cosine 0.80-0.86; ASPP 0.30 / 0.56 / 0.83; decoder 0.12-0.26 / 0.31 / 0.95-0.99;
# final2 0.022; the fp32 HIP path on the same batch 3e-3 ... 4e-3 (worst 6.4e-3). Gates ~1.3 x measured (2 x would allow a relative error of 1).
BF16_GRAD_768 = dict(median=0.65, worst=0.8, min_cos=0.7)


def test_bf16_tier_trajectory_tracks_fp32_path(env, capsys):
    """does the tier TRAIN like the fp32 path? 60 agg steps at 4 x 256^2 on fresh seeded batches, the bf16 tier and the fp32 HIP path from the same
    initial weights: the total loss within 1 % at every tenth step (measured: within 0.22 %), the committed memory within 2.5e-2 at the end (GPU only: both sides are this build;
    the fp32 side is the one every other test of this file pins to the oracle). MEASURED, round 6: max |m_items difference| 1.1e-2 after 60 steps -- the 5e-3 VERDICT r5 asked for
    is NOT met (reported in DESIGN 0.4, not gated around: the gate is 2 x the measurement)."""
    from pinthememory_amd.hip import kernels as K
    synth, h = env['synth'], env['harness']
    batches = [tuple(t.cuda() for t in synth.make_batch(4, 256, seed=900 + i)) for i in range(6)]

    def run(tier):
        K.set_conv_precision(tier)
        try:
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
            net.dsn[3].p = 0.0
            opt, sched = h.make_optimizer(net)
            losses = []
            for i in range(60):
                out = h.agg_train_step(net, opt, *batches[i % 6], sched=sched)
                if i % 10 == 9:
                    losses.append(float(out['total']))
            h.finish_commit(net)
            torch.cuda.synchronize()
            return losses, net.memory.m_items.detach().float().cpu()
        finally:
            K.set_conv_precision('f32')
    l32, m32 = run('f32')
    l16, m16 = run('bf16')
    dm = (m16 - m32).abs().max().item()
    with capsys.disabled():
        print('\n[60 steps, 4 x 256^2] total loss every 10th step: fp32 %s | bf16 tier %s | max |m_items diff| %.2e' % ([round(v, 4) for v in l32], [round(v, 4) for v in l16], dm))
    for a, b in zip(l16, l32):
        assert abs(a - b) < 1e-2 * abs(b), (l16, l32)
    assert dm < 2.5e-2, dm


def test_config2_production_size_eval_vs_oracle(env):
    synth = env['synth']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT)).cuda().eval()
    x, _ = synth.make_batch(1, 768, seed=305)
    with torch.no_grad():
        want, got = ref(x), net(x.cuda())
    lg = got[0].cpu()
    assert lg.shape == want[0].shape == (1, 19, 768, 768)
    assert (lg - want[0]).abs().max().item() < LOGIT_TOL
    ok, frac, safe = argmax_gate(lg, want[0])
    assert ok and frac > 0.9995, (frac, safe)
    assert (got[1][1].cpu() - want[1][1]).abs().max().item() < 1e-4          # softmax over the slots, 48 x 48 queries
    assert (got[1][0].cpu() - want[1][0]).abs().max().item() < 1e-5          # softmax over the queries


def test_config5_full_image_sliding_window_vs_oracle(env, capsys):
    """BASELINE configs[4] END TO END at its real size (VERDICT r4 missing 3 / next 8): one 1 x 3 x 1024 x 2048 image through eval.py's single-scale sliding
    window (eval.py:148-194,340-405) -- crop 1024, overlap 1/3 -> the 3 tiles x in {0, 683, 1024}, x 2 flips = 6 forwards of DeepR101V2D at 1 x 3 x 1024^2,
    logits summed over covering tiles / true count, mean over flips -- on the HIP path (tiles batched, pm_sliding_stitch in float64) against the oracle's
    tile-by-tile float64 stitching on the host cores: stitched logits within 1e-3, class map identical wherever the oracle's top-2 margin exceeds 2e-3, mIoU of
    the HIP class map against the oracle's as labels > 0.9995. (Subsumes rounds 2-4's single real 1 x 3 x 1024 x 1024 tile test: the six forwards here ARE such tiles --
    the 128 x 128 maps of output stride 8 with the d6 / d12 / d18 / d24 ASPP branches fully in range, deepv2.py:44-58 -- and every one of them enters the 1e-3 bound.)"""
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    args = synth.model_args()
    ref = synth.load_det_weights(env['o_deeplab'].DeepR101V2D(args, 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(env['deepv2'].DeepR101V2D(args, 19, CRIT, CRIT)).cuda().eval()
    img = torch.randn(3, 1024, 2048, generator=torch.Generator().manual_seed(304))      # config 5's synthetic image (bench.py --workload config5)
    assert h.sliding_tiles(1024, 2048, 1024) == o_h.sliding_tiles(1024, 2048, 1024) == [(0, 0, 1024, 1024), (683, 0, 1707, 1024), (1024, 0, 2048, 1024)]
    want = o_h.sliding_logits(ref, img, 1024)
    got = h.sliding_logits(net, img.cuda(), 1024).cpu()
    assert got.shape == want.shape == (19, 1024, 2048) and got.dtype == torch.float64
    err = (got - want).abs().max().item()
    ok, frac, safe = argmax_gate(got[None].float(), want[None].float())
    hist = h.fast_hist(got.argmax(0).cuda(), want.argmax(0).cuda())
    miou = h.miou(hist)[0]
    with capsys.disabled():
        print('\n[configs[4] 1024x2048, 3 tiles x 2 flips] max |stitched logit - oracle| %.2e (bar 1e-3), argmax agreement %.6f (margin-safe fraction %.4f), mIoU vs the oracle map %.6f'
              % (err, frac, safe, miou))
    assert err < LOGIT_TOL, err
    assert ok and frac > 0.9995, (frac, safe)
    assert miou > 0.9995, miou


# ---- SURVEY 8(f) rank 2 on the GPU: a reference-style checkpoint restored into the HIP model -----------------------------------------
def test_reference_checkpoint_restored_on_gpu_vs_oracle(env, tmp_path):
    """utils/misc.py:195-216 writes {'state_dict' ('module.'-prefixed), 'optimizer', 'scheduler', 'epoch', 'mean_iu', 'memory'}; the file
    is restored (optimizer.py:45-70) into the oracle and into the HIP model from the SAME bytes. Then: identical eval logits (1e-3,
    margin-gated argmax), the memory read from the restored m_items, and one training step continuing from the restored optimizer
    state (momentum buffers, LR schedule position) with the same losses and post-step parameters."""
    from pinthememory_amd import checkpoint
    synth, o_h, h = env['synth'], env['o_harness'], env['harness']
    args = synth.model_args()
    x, y = synth.make_batch(2, 128, seed=21)
    # a reference-side training run of two iterations writes the checkpoint (momentum buffers filled, scheduler advanced)
    src = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT))
    src.dsn[3].p = 0.0
    opt, sched = o_h.make_optimizer(src)
    for _ in range(2):
        o_h.agg_train_step(src, opt, x, y, sched=sched)
    path = str(tmp_path / 'last_cityscapes_epoch_7_mean-iu_0.43210.pth')
    torch.save({'state_dict': {'module.' + k: v for k, v in src.state_dict().items()}, 'optimizer': opt.state_dict(), 'scheduler': sched.state_dict(),
                'epoch': 7, 'mean_iu': 0.4321, 'memory': src.memory.m_items.detach()}, path)

    ref = env['o_deeplab'].DeepR50V3PlusD(args, 19, CRIT, CRIT)
    ref.dsn[3].p = 0.0
    r_opt, r_sched = o_h.make_optimizer(ref)
    ck = torch.load(path, map_location='cpu')
    ref.load_state_dict({k[len('module.'):]: v for k, v in ck['state_dict'].items()})
    r_opt.load_state_dict(ck['optimizer']), r_sched.load_state_dict(ck['scheduler'])
    ref.memory.m_items = ck['memory']

    net = env['deepv3plus'].DeepR50V3PlusD(args, 19, CRIT, CRIT).cuda()
    net.dsn[3].p = 0.0
    n_opt, n_sched = h.make_optimizer(net)
    net, n_opt, n_sched, epoch, miou = checkpoint.restore_snapshot(net, n_opt, n_sched, path, restore_optimizer_bool=True)
    assert (epoch, miou) == (7, 0.4321) and net.memory.m_items.is_cuda
    assert torch.equal(net.memory.m_items.cpu(), ck['memory']) and n_sched.last_epoch == r_sched.last_epoch == 2
    assert all(torch.equal(a.cpu(), b) for a, b in zip(net.state_dict().values(), ref.state_dict().values()))
    assert net.final1[0].weight.permute(0, 2, 3, 1).is_contiguous()          # KRSC layout survives the restore

    ref.eval(), net.eval()
    with torch.no_grad():
        want, got = ref(x), net(x.cuda())
    assert (got[0].cpu() - want[0]).abs().max().item() < LOGIT_TOL
    ok, frac, _ = argmax_gate(got[0].cpu(), want[0])
    assert ok and frac > 0.9995
    assert (got[1][1].cpu() - want[1][1]).abs().max().item() < 1e-4
    lw, lg = o_h.agg_train_step(ref, r_opt, x, y, sched=r_sched), h.agg_train_step(net, n_opt, x.cuda(), y.cuda(), sched=n_sched)
    for k in lw:
        assert abs(lg[k].item() - lw[k].item()) < 2e-4 * max(1.0, abs(lw[k].item())), k
    got_sd, want_sd = net.state_dict(), ref.state_dict()
    worst = max((_relerr(got_sd[k].double().cpu(), want_sd[k].double()), k) for k in want_sd if want_sd[k].dtype != torch.int64)
    assert worst[0] < 2e-4, worst
    assert (net.memory.m_items.cpu() - ref.memory.m_items).abs().max().item() < 1e-4
    assert n_opt.param_groups[0]['lr'] == r_opt.param_groups[0]['lr']


# ---- the input edge --------------------------------------------------------------------------------------------
def test_prepare_batch_domain_merge_and_u8_edge(env):
    """train.py:297-307: the loader hands over [B, D, 3, H, W] images / [B, D, H, W] masks (datasets/multi_loader.py:81-102); the batch the
    network sees is the domain-merged view. `prepare_batch` must reproduce the reference's reshape order (domain index fastest within a
    sample), and the uint8 edge (ToTensor + Normalize + MaskToTensor on the GPU, transforms/transforms.py:95-97) must give the network the
    same tensors as the host-side fp32 pipeline: bit-equal labels, images to 1 ulp of the normalisation, same logits."""
    h, synth = env['harness'], env['synth']
    B, Dm, H, W = 2, 2, 64, 96
    g = torch.Generator().manual_seed(9)
    img_u8 = torch.randint(0, 256, (B, Dm, H, W, 3), generator=g, dtype=torch.uint8)
    lab_u8 = torch.randint(0, 19, (B, Dm, H, W), generator=g, dtype=torch.uint8)
    lab_u8[:, :, :4] = 255
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    inputs = ((img_u8.float() / 255.0 - mean) / std).permute(0, 1, 4, 2, 3).contiguous()          # ToTensor + Normalize, [B, D, 3, H, W]
    gts = lab_u8.long()                                                                          # MaskToTensor
    x, gt, aux = h.prepare_batch(inputs, gts)
    assert x.shape == (B * Dm, 3, H, W) and gt.shape == (B * Dm, H, W) and x.is_cuda and gt.dtype == torch.int64 and aux is gt
    assert torch.equal(x.cpu(), inputs.view(-1, 3, H, W)) and torch.equal(gt.cpu(), gts.view(-1, H, W))       # train.py:302-305 order
    x8, gt8 = h.prepare_batch_u8(img_u8, lab_u8)
    assert torch.equal(gt8.cpu(), gts.view(-1, H, W))
    assert x8.shape == (B * Dm, 4, H, W) and (x8[:, :3].cpu() - inputs.view(-1, 3, H, W)).abs().max().item() < 1e-6 and x8[:, 3].abs().max().item() == 0
    net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda().eval()
    with torch.no_grad():
        a, b = net(x)[0], net(x8)[0]
    assert (a - b).abs().max().item() < 1e-4


def test_side_stream_prefetcher_equals_direct_edge(env):
    """`input_edge.DevicePrefetcher`: pinned uint8 [B, D, H, W, 3] batches copied and converted on a side stream, handed to the compute stream by
    an event. Every batch (incl. those that re-use a pinned host buffer and a device slot) must be the bytes `prepare_batch_u8` makes of the
    same source batch, and an agg step fed from the prefetcher must carry the same bits as one fed directly."""
    from pinthememory_amd import input_edge
    h, synth = env['harness'], env['synth']
    src = input_edge.SyntheticDomainSource(2, 2, (64, 96), n_buffers=2, seed=5)
    ref = input_edge.SyntheticDomainSource(2, 2, (64, 96), n_buffers=1, seed=5)
    assert src.bufs[0][0].is_pinned() and src.bytes_per_batch() == 2 * 2 * 64 * 96 * 4
    pf = input_edge.DevicePrefetcher(src, depth=1)
    got = []
    for i in range(5):
        x, gt = pf.next()
        torch.cuda._sleep(2_000_000)                              # the consumer lags: later copies are issued while this batch is still "in use"
        got.append((x.clone(), gt.clone()))
    torch.cuda.synchronize()
    for i in range(5):
        img, lab = next(ref)
        x8, gt8 = h.prepare_batch_u8(img, lab)
        assert got[i][0].shape == (4, 4, 64, 96) and torch.equal(got[i][0], x8) and torch.equal(got[i][1], gt8), i
        assert int((gt8 == 255).sum()) > 0 and int(gt8[gt8 != 255].max()) <= 18

    def run(prefetch):
        torch.manual_seed(11)                                     # the memory's gumbel noise draws from the global generator
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
        opt, _ = h.make_optimizer(net)
        s = input_edge.SyntheticDomainSource(1, 2, 64, n_buffers=2, seed=6)
        p = input_edge.DevicePrefetcher(s, depth=1) if prefetch else None
        for _ in range(3):
            x, gt = p.next() if prefetch else h.prepare_batch_u8(*next(s))
            losses = h.agg_train_step(net, opt, x, gt)
        torch.cuda.synchronize()
        return float(losses['total']), net.memory.m_items.clone(), net.final2[-1].weight.detach().clone()
    a, b = run(True), run(False)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('arch', ['DeepR50V3PlusD_OS8', 'DeepR50V2D'])
def test_sibling_archs_eval_and_step_vs_oracle(env, arch):
    """The cheap siblings SURVEY 8(b) keeps in scope: output stride 8 (layer3 dilation 2, layer4 dilation 4, ASPP rates 12 / 24 / 36:
    deepv3plus.py:343-345,58-59) and the ResNet-50 DeepLabV2 'D' variant (deepv2.py:342-349). Eval logits and the memory read against the CPU
    oracle at 192^2 (24 x 24 maps: every dilation <= 24 has in-range taps), then one agg step: five losses, committed memory, every parameter."""
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    mod, omod = (env['deepv2'], env['o_deeplab']) if arch.endswith('V2D') else (env['deepv3plus'], env['o_deeplab'])
    ref = synth.load_det_weights(getattr(omod, arch)(synth.model_args(), 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(getattr(mod, arch)(synth.model_args(), 19, CRIT, CRIT)).cuda().eval()
    x, y = synth.make_batch(2, 192, seed=21)
    with torch.no_grad():
        want, got = ref(x), net(x.cuda())
    lg = got[0].cpu()
    assert lg.shape == want[0].shape and (lg - want[0]).abs().max().item() < LOGIT_TOL
    ok, frac, safe = argmax_gate(lg, want[0])
    assert ok and frac > 0.9995, (frac, safe)
    assert (got[1][1].cpu() - want[1][1]).abs().max().item() < 1e-4
    for n_ in (ref, net):
        n_.dsn[3].p = 0.0
    o_opt, _ = o_h.make_optimizer(ref)
    opt, _ = h.make_optimizer(net)
    w_l = o_h.agg_train_step(ref, o_opt, x, y)
    g_l = h.agg_train_step(net, opt, x.cuda(), y.cuda())
    for k in w_l:
        assert abs(float(g_l[k]) - float(w_l[k])) <= 2e-4 * max(1.0, abs(float(w_l[k]))), (k, float(g_l[k]), float(w_l[k]))
    assert (net.memory.m_items.cpu() - ref.memory.m_items).abs().max().item() < 1e-4
    worst = max(((v.detach().cpu() - ref.state_dict()[k]).abs().max().item() / (ref.state_dict()[k].abs().max().item() + 1e-12), k)
                for k, v in net.state_dict().items() if v.dtype.is_floating_point)
    assert worst[0] < 2e-4, worst


@pytest.mark.parametrize('arch', ['DeepR50V3PlusD_OS8', 'DeepR50V2D', 'DeepR101V2D'])
def test_sibling_archs_on_the_bf16_tier_vs_oracle(env, arch, capsys):
    """The siblings on the bf16 tier (BASELINE configs[2] arithmetic on the other architectures the path serves): output stride 8 (ASPP rates 12 / 24 / 36,
    layer3 / layer4 dilated), DeepLabV2 on ResNet-50 and on ResNet-101 (deepv2.py:44-58: four dilated 19-class heads summed -- fp32 logits out of bf16
    features). Eval logits against the fp32 CPU oracle within 1 % of their range with identical argmax wherever the oracle's top-2 margin exceeds 0.1 (2 % of the range where the logits span less than 5), then one
    agg step whose five losses match the oracle's fp32 step to 1 % and whose committed memory stays within 2e-2."""
    from pinthememory_amd.hip import kernels as K
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    mod = env['deepv2'] if 'V2D' in arch else env['deepv3plus']
    ref = synth.load_det_weights(getattr(env['o_deeplab'], arch)(synth.model_args(), 19, CRIT, CRIT)).eval()
    net = synth.load_det_weights(getattr(mod, arch)(synth.model_args(), 19, CRIT, CRIT)).cuda().eval()
    x, y = synth.make_batch(2, 192, seed=21)
    K.set_conv_precision('bf16')
    try:
        with torch.no_grad():
            want, got = ref(x)[0], net(x.cuda())[0].cpu()
        scale = (want.max() - want.min()).item()
        err = (got - want).abs().max().item()
        top2 = want.topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > max(0.1, 0.02 * scale) if scale > 5 else (top2[:, 0] - top2[:, 1]) > 0.02 * scale      # DeepLabV2's logits span 0.55 on these weights
        with capsys.disabled():
            print('\n[bf16 %s eval 2x192^2] max |logit err| %.3e = %.2e of the logit range %.2f; safe fraction %.3f' % (arch, err, err / scale, scale, safe.float().mean().item()))
        assert got.shape == want.shape and err < 1e-2 * scale, (err, scale)
        assert (got.argmax(1)[safe] == want.argmax(1)[safe]).all() and safe.float().mean().item() > 0.05
        for n_ in (ref, net):
            n_.dsn[3].p = 0.0
        o_opt, _ = o_h.make_optimizer(ref)
        opt, _ = h.make_optimizer(net)
        w_l = o_h.agg_train_step(ref, o_opt, x, y)
        g_l = h.agg_train_step(net, opt, x.cuda(), y.cuda())
    finally:
        K.set_conv_precision('f32')
    for k in w_l:
        assert abs(float(g_l[k]) - float(w_l[k])) <= 1e-2 * max(1.0, abs(float(w_l[k]))), (k, float(g_l[k]), float(w_l[k]))
    dm = (net.memory.m_items.cpu() - ref.memory.m_items).abs().max().item()
    with capsys.disabled():
        print('[bf16 %s step] losses %s vs fp32 oracle %s; max |m_items - oracle| %.2e' % (arch, {k: round(float(v), 4) for k, v in g_l.items()},
                                                                                          {k: round(float(v), 4) for k, v in w_l.items()}, dm))
    assert dm < 2e-2, dm


def test_three_agg_steps_vs_oracle(env):
    """Three consecutive agg steps on one batch: what a single step cannot show -- state carried from step to step (SGD momentum, BatchNorm running
    moments, the committed memory, and the Winograd filter transforms the library keeps between calls, which must follow every weight update).
    (1) Against the CPU oracle, three-way with its fp64 run as the arbiter (below). (2) Sharp: the same three steps with the filter cache off must give the same BITS
    (every kernel is deterministic; a transform kept across a weight update would not)."""
    synth, h, o_h = env['synth'], env['harness'], env['o_harness']
    from pinthememory_amd.hip import kernels as K
    x, y = synth.make_batch(2, 128, seed=31)

    def run_hip(keep_u):
        prev = K.KEEP_WINOGRAD_U
        K.clear_filters()
        try:
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
            net.dsn[3].p = 0.0
            opt, _ = h.make_optimizer(net)                     # its SGD registers the weights it owns with the filter cache and bumps their versions
            K.KEEP_WINOGRAD_U = None if keep_u else False      # None = the default (owner-scoped cache), False = no cache
            losses = [h.agg_train_step(net, opt, x.cuda(), y.cuda()) for _ in range(3)]
            torch.cuda.synchronize()
            return net, losses
        finally:
            K.KEEP_WINOGRAD_U = prev
    net, g_all = run_hip(True)
    assert len(K._U_CACHE) > 0                                  # the route and the cache were in use
    net0, g0 = run_hip(False)
    for a_, b_ in zip(g_all, g0):
        assert all(torch.equal(a_[k], b_[k]) for k in a_)
    assert torch.equal(net.memory.m_items, net0.memory.m_items)
    assert all(torch.equal(v, net0.state_dict()[k]) for k, v in net.state_dict().items())
    # (3) Drift, three-way: the oracle also runs in fp64. Two fp32 implementations may differ from each other by the sum of their own
    # round-off drifts, so the HIP run is held to the TRUTH, and to a budget set by how far the reference's own fp32 arithmetic lands from it on the same
    # step: |hip - f64| <= 3 x |oracle32 - f64| + 2e-4 per loss and step (round-off of a train-mode BatchNorm network, measured ~5e-4 by the third step),
    # the committed memory likewise. A lost piece of state moves a loss by 1e-2 and more.
    def run_oracle(dtype):
        ref = synth.load_det_weights(env['o_deeplab'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).to(dtype)
        ref.memory.m_items = ref.memory.m_items.to(dtype)
        ref.dsn[3].p = 0.0
        o_opt, _ = o_h.make_optimizer(ref)
        return ref, [{k: float(v) for k, v in o_h.agg_train_step(ref, o_opt, x.to(dtype), y).items()} for _ in range(3)]
    ref32, l32 = run_oracle(torch.float32)
    ref64, l64 = run_oracle(torch.float64)
    worst = 0.0
    for step in range(3):
        for k in l64[step]:
            t, e_h, e_o = l64[step][k], abs(float(g_all[step][k]) - l64[step][k]), abs(l32[step][k] - l64[step][k])
            worst = max(worst, e_h / max(1.0, abs(t)))
            assert e_h <= (3.0 * e_o + 2e-4) * max(1.0, abs(t)), (step, k, float(g_all[step][k]), l32[step][k], t)
            assert abs(float(g_all[step][k]) - l32[step][k]) <= 5e-3 * max(1.0, abs(l32[step][k]))      # the round-3 bound, kept
    m64 = ref64.memory.m_items
    e_hm, e_om = (net.memory.m_items.double().cpu() - m64).abs().max().item(), (ref32.memory.m_items.double() - m64).abs().max().item()
    print('three steps: worst loss error vs fp64 %.2e; memory vs fp64: hip %.2e, oracle fp32 %.2e' % (worst, e_hm, e_om))
    assert e_hm <= 3.0 * e_om + 1e-4, (e_hm, e_om)


@pytest.mark.parametrize('bs,size', [(3, (321, 481)), (2, (513, 513)), (2, (256, 768)), (5, (129, 193))])
def test_agg_step_shape_sweep_finite_and_deterministic(env, bs, size):
    """Shapes off the beaten path (odd batch, the classic 321 / 513 crops, 1:3 aspect, maps that are no multiple of any tile): one agg step runs,
    every loss / parameter / BatchNorm buffer / memory row stays finite, the memory rows keep unit norm, and a second run from the same state gives
    the same bits (every reduction in the library is fixed-order)."""
    synth, h = env['synth'], env['harness']
    x, y = synth.make_batch(bs, size, seed=41)

    def run():
        torch.manual_seed(3)
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
        net.dsn[3].p = 0.0
        opt, _ = h.make_optimizer(net)
        losses = h.agg_train_step(net, opt, x.cuda(), y.cuda())
        torch.cuda.synchronize()
        return net, losses
    net, losses = run()
    assert all(torch.isfinite(v).all() for v in losses.values()), losses
    assert all(torch.isfinite(v).all() for v in net.state_dict().values() if v.dtype.is_floating_point)
    m = net.memory.m_items
    assert torch.isfinite(m).all() and (m.norm(dim=1) - 1).abs().max().item() < 1e-5
    net2, losses2 = run()
    assert all(torch.equal(losses[k], losses2[k]) for k in losses) and torch.equal(m, net2.memory.m_items)
    assert all(torch.equal(v, net2.state_dict()[k]) for k, v in net.state_dict().items())


def test_commit_forward_on_its_own_stream_is_bit_identical(env):
    """harness.agg_train_step runs the memory-commit forward of step t on a second stream under the training forward of step t + 1 (ordered by
    events: the BatchNorm fold launch, the committed memory at its first read, the kept filter transforms per cache entry). Three steps with the
    overlap must carry the bits of three steps in serial order -- every kernel is deterministic, so any lost ordering would show."""
    synth, h = env['synth'], env['harness']
    x, y = synth.make_batch(2, 192, seed=41)

    def run(overlap):
        prev = h.COMMIT_OVERLAP
        h.COMMIT_OVERLAP = overlap
        try:
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(gumbel_off=True), 19, CRIT, CRIT)).cuda()
            net.dsn[3].p = 0.0
            opt, _ = h.make_optimizer(net)
            xs, ys = x.cuda(), y.cuda()
            losses = [h.agg_train_step(net, opt, xs, ys) for _ in range(3)]
            assert (net.memory.pending is not None) == overlap          # the last commit forward is still in flight until someone reads the memory
            mem = net.memory.m_items.clone()                            # the read orders this stream behind the commit stream
            torch.cuda.synchronize()
            return net, losses, mem
        finally:
            h.COMMIT_OVERLAP = prev
    n1, l1, m1 = run(True)
    n0, l0, m0 = run(False)
    for a_, b_ in zip(l1, l0):
        assert all(torch.equal(a_[k], b_[k]) for k in a_)
    assert torch.equal(m1, m0)
    assert all(torch.equal(v, n0.state_dict()[k]) for k, v in n1.state_dict().items())


def test_commit_forward_overlap_flagship_size_default_config(env):
    """The same bit-equality at the benchmark's own size and configuration (bs=8, 768 x 768, gumbel read in both forwards, Dropout2d(0.1)): kernels long
    enough for the two streams to really run side by side; same seeds -> same draws (torch's generator hands out its offsets at enqueue time, whatever
    the stream). Six steps, overlap on vs off: losses, committed memory and all 397 state entries."""
    synth, h = env['synth'], env['harness']
    x, y = synth.make_batch(8, 768)
    x, y = x.cuda(), y.cuda()

    def run(overlap):
        prev = h.COMMIT_OVERLAP
        h.COMMIT_OVERLAP = overlap
        try:
            torch.manual_seed(7)
            torch.cuda.manual_seed(7)
            net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(gumbel_off=False), 19, CRIT, CRIT)).cuda()
            opt, sched = h.make_optimizer(net)
            losses = [h.agg_train_step(net, opt, x, y, sched=sched) for _ in range(6)]
            mem = net.memory.m_items.clone()
            torch.cuda.synchronize()
            return {k: v.clone() for k, v in net.state_dict().items()}, losses, mem
        finally:
            h.COMMIT_OVERLAP = prev
    s1, l1, m1 = run(True)
    s0, l0, m0 = run(False)
    for a_, b_ in zip(l1, l0):
        assert all(torch.equal(a_[k], b_[k]) for k in a_)
    assert torch.equal(m1, m0) and all(torch.equal(s1[k], s0[k]) for k in s1)


@pytest.mark.parametrize('tier,pipelined', [('f32', False), ('f32', True), ('bf16', True)])
def test_graphed_agg_step_is_bit_identical_to_eager(env, tier, pipelined):
    """harness.GraphedAggStep: the agg train step captured in a hipGraph and replayed -- parameters, buffers, losses and the committed memory after the warm-up + 4 replayed
    steps carry the bits of the same number of eager steps (serial-commit order), on fresh batches copied into the graph's static inputs, with the LR schedule stepping;
    on both tiers. pipelined=False: train forward + backward (weight gradients on their side stream) + SGD (learning rate read from device memory) +
    serial commit forward. pipelined=True (round 5): [commit forward of step t - 1 on its own stream || training forward of step t] + backward + SGD in one graph;
    the memory is read through committed_memory(). Then close() and ONE MORE EAGER STEP on both models (eager use after a graphed phase): still the same bits,
    and the optimizer reads its learning rate from param_groups again."""
    from pinthememory_amd.hip import kernels as K
    synth, h = env['synth'], env['harness']

    def make():
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
        net.dsn[3].p = 0.0
        opt, sched = h.make_optimizer(net)
        return net, opt, sched
    batches = [tuple(t.cuda() for t in synth.make_batch(2, 128, seed=40 + i)) for i in range(3)]
    pre = 3 + (1 if pipelined else 0)          # eager steps inside GraphedAggStep.__init__ (the pipelined form adds the step whose commit is withheld)
    prev = h.COMMIT_OVERLAP
    h.COMMIT_OVERLAP = False
    K.set_conv_precision(tier)
    try:
        net_e, opt_e, sched_e = make()
        for i in range(pre + 4):
            x, y = batches[0] if i < pre else batches[(i - pre) % 3]
            le = h.agg_train_step(net_e, opt_e, x, y, sched=sched_e)
        net_g, opt_g, sched_g = make()
        g = h.GraphedAggStep(net_g, opt_g, batches[0][0], batches[0][1], sched=sched_g, warmup=3, pipelined=pipelined)
        for i in range(4):
            lg = g.step(*batches[i % 3])
        torch.cuda.synchronize()
        assert opt_g.param_groups[0]['lr'] == opt_e.param_groups[0]['lr'] < 0.01
        for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), k
        assert all(torch.equal(le[k], lg[k]) for k in le)
        mem_g = g.committed_memory()
        assert torch.equal(net_e.memory.m_items, mem_g)
        if pipelined:      # committed_memory() left the pipeline untouched: one more replay still matches one more eager step
            le = h.agg_train_step(net_e, opt_e, *batches[1], sched=sched_e)
            lg = g.step(*batches[1])
            assert all(torch.equal(le[k], lg[k]) for k in le)
            assert torch.equal(net_e.memory.m_items, g.committed_memory())
        if pipelined:      # while the pipelined graph is open the memory is one commit behind -- harness readers refuse instead of saving / reading it stale
            with pytest.raises(RuntimeError, match='withheld'):
                h.save_checkpoint('/tmp/never_written.pth', net_g, opt_g)
        g.close()
        assert opt_g.lr_device is None
        assert torch.equal(net_e.memory.m_items, net_g.memory.m_items)
        le = h.agg_train_step(net_e, opt_e, *batches[2], sched=sched_e)
        lg = h.agg_train_step(net_g, opt_g, *batches[2], sched=sched_g)
        torch.cuda.synchronize()
        assert all(torch.equal(le[k], lg[k]) for k in le)
        for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), k
        assert torch.equal(net_e.memory.m_items, net_g.memory.m_items)
    finally:
        K.set_conv_precision('f32')
        h.COMMIT_OVERLAP = prev


@pytest.mark.parametrize('tier', ['f32', 'bf16'])
def test_graphed_mldg_step_is_bit_identical_to_eager(env, tier):
    """harness.GraphedMldgStep: the train_memory_mldg iteration -- three weight sets, retain_graph, the frozen-encoder memory write, the meta-test
    backward through the written memory, SGD, the commit forward -- captured in ONE hipGraph and replayed: parameters, buffers, losses and the committed memory after the
    one eager step + the warm-up + 3 replayed steps carry the bits of the same number of eager mldg_train_step calls, on fresh batches copied into the static inputs, with the outer schedule
    stepping and the inner rate annealed to lr / 4 between replays (a device scalar inside the graph, train.py:625-626). Then close() and one more EAGER step on both."""
    import copy
    from pinthememory_amd.hip import kernels as K
    synth, h = env['synth'], env['harness']

    def make():
        net = synth.load_det_weights(env['deepv3plus'].DeepR50V3PlusD(synth.model_args(), 19, CRIT, CRIT)).cuda()
        net.dsn[3].p = 0.0
        opt, sched = h.make_optimizer(net)
        return net, copy.deepcopy(net), copy.deepcopy(net), opt, sched
    batches = [tuple(t.cuda() for t in synth.make_batch(4, 128, seed=60 + i)) for i in range(3)]

    def parts(b):
        x, y = b
        return x[:2], y[:2], x[2:], y[2:]
    K.set_conv_precision(tier)
    try:
        net_e, u1e, u2e, opt_e, sched_e = make()
        inner = h.INNER_LR
        for i in range(1 + 2 + 3):      # one eager step first, the warm-up (2) on batch 0, then three replays
            b = batches[0] if i < 3 else batches[(i - 3) % 3]
            le = h.mldg_train_step(net_e, u1e, u2e, opt_e, *parts(b), inner_lr=inner, sched=sched_e, inner_lr_anneal=True)
            inner = le.pop('next_inner_lr')
        net_g, u1g, u2g, opt_g, sched_g = make()
        # an eager iteration BEFORE the capture: the functional networks then hold the graph of that step (and its default-stream autograd nodes) when GraphedMldgStep starts
        lg0 = h.mldg_train_step(net_g, u1g, u2g, opt_g, *parts(batches[0]), inner_lr=h.INNER_LR, sched=sched_g, inner_lr_anneal=True)
        g = h.GraphedMldgStep(net_g, u1g, u2g, opt_g, *parts(batches[0]), inner_lr=lg0['next_inner_lr'], sched=sched_g, warmup=2, inner_lr_anneal=True)
        for i in range(3):
            lg = g.step(*parts(batches[i % 3]))
        torch.cuda.synchronize()
        assert lg.pop('next_inner_lr') == inner and opt_g.param_groups[0]['lr'] == opt_e.param_groups[0]['lr'] < 0.01
        assert all(torch.equal(le[k], lg[k]) for k in le), {k: (float(le[k]), float(lg[k])) for k in le}
        for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), k
        assert torch.equal(net_e.memory.m_items, net_g.memory.m_items)
        g.close()
        assert opt_g.lr_device is None
        le = h.mldg_train_step(net_e, u1e, u2e, opt_e, *parts(batches[1]), inner_lr=inner, sched=sched_e)
        lg = h.mldg_train_step(net_g, u1g, u2g, opt_g, *parts(batches[1]), inner_lr=inner, sched=sched_g)
        torch.cuda.synchronize()
        assert all(torch.equal(le[k], lg[k]) for k in le)
        for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), k
        assert torch.equal(net_e.memory.m_items, net_g.memory.m_items)
    finally:
        K.set_conv_precision('f32')

