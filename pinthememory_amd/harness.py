"""Callers either side of the hot path, on the GPU: the aggregation train step, memory initialisation, sliding-window
evaluation and mIoU -- the build's counterparts of /root/reference/train.py:284-374 (+ calculate_loss :213-244),
train.py:1000-1042, eval.py:148-274,340-405 and utils/misc.py:65-73."""
import contextlib
import math

import torch
import torch.nn.functional as F

from . import dist as D
from .hip import kernels as K
from .hip import ops

LOSS_W = dict(aux=0.4, read=0.02, div=0.4, cls=0.2)    # train.py:1213-1215 defaults


def make_optimizer(net, lr=0.01, momentum=0.9, poly_exp=9):
    """optimizer.py:11-32: SGD over all named parameters, weight decay hard-coded 5e-4, lr * exp(-poly_exp*it/120000).
    The optimizer is torch.optim.SGD (same state_dict) whose step() is one multi-tensor launch of the HIP library (optim.py);
    it registers the weights it owns with the transformed-filter cache (hip/kernels.py) and bumps their versions when it updates them."""
    from .optim import SGD
    opt = SGD([p for _, p in net.named_parameters()], lr=lr, weight_decay=5e-4, momentum=momentum, nesterov=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: math.exp(-1 * poly_exp * it / 120000))
    return opt, sched


def total_loss(outputs, w=LOSS_W):
    main, aux, readloss, writeloss = outputs[0], outputs[1], outputs[-2], outputs[-3]
    return main + w['aux'] * aux + w['read'] * readloss + w['div'] * writeloss[0] + w['cls'] * writeloss[1]


def memory_only_forward(net, x, gts):
    """What the reference's second forward (train.py:330-335) is for: eval-mode features -> memory.write(); the decoder
    and losses it also computes are discarded there, so skipping them leaves every result identical."""
    m = net.module if hasattr(net, 'module') else net
    _, _, feat = m._trunk(x)
    feat = m.aspp(feat)
    if hasattr(m, 'bot_aspp'):
        from .network.deepv3plus import run_cbr
        feat = run_cbr(m.bot_aspp, feat)
    m.memory._mem(feat)
    m.memory.m_items = m.memory.m_items.detach()
    m.memory.write(feat, gts, True)
    from .hip import ops
    ops.flush_bn_counters()


# The memory-commit forward of step t (eval mode, no graph, post-SGD weights) and the training forward of step t + 1 are independent up to the
# memory read of the latter: the commit forward runs on its own stream, and the next step's HBM-bound BatchNorm / transform passes run under its
# GEMMs (and vice versa). Ordering: (1) it starts after the SGD launches; (2) the main stream continues once the commit forward's ONE fold launch has
# read every BatchNorm running moment (ops.last_prefold_event) -- the next training forward updates them; (3) Memory_sup waits for the committed memory
# where it is first read (Memory_sup.pending); (4) transformed filters the commit forward wrote are event-ordered per cache entry (hip/kernels.py);
# (5) the next SGD is behind (3) on the main stream, so the weights are not written under it. Results are bit-identical to the serial order.
# With more than one rank every collective of a step stays on the MAIN stream (dist.py: one communicator, program order): the commit forward's only
# exchange -- the memory-slot sum of its write -- is deferred (Memory_sup.defer_sync) to the next point EVERY rank passes: the next training forward's
# memory read, or an explicit harness.finish_commit(net) -- never to an attribute read (a rank-0-only save would pair it with another rank's
# collective; `m_items` raises while the sum is owed); eval-mode BatchNorm has no exchange. Under the reference's DDP wrapper the commit forward calls
# the bare module (see agg_train_step). PM_COMMIT_OVERLAP=0 disables the overlap.
COMMIT_OVERLAP = __import__('os').environ.get('PM_COMMIT_OVERLAP', '1') == '1'
_commit_streams = {}


COMMIT_CUS = int(__import__('os').environ.get('PM_COMMIT_CUS', '0'))      # A/B knob: confine the commit forward's stream to n CUs (ops.masked_stream)


def _commit_stream(device):
    if device.index not in _commit_streams:
        _commit_streams[device.index] = ops.masked_stream(COMMIT_CUS, device.index, first=1) if COMMIT_CUS > 0 else torch.cuda.Stream(device=device)
    return _commit_streams[device.index]


def finish_commit(net):
    """Finish the memory write of the last commit forward where it was left to the next reader (more than one rank, commit forward on its own
    stream: Memory_sup.defer_sync). COLLECTIVE in that case -- call it on EVERY rank, at the same point of the program, before anything reads
    `m_items` between steps on a subset of ranks (validation, the rank-0-only save of train.py:188-191). The next training forward does it by
    itself (Memory_sup.read). A no-op with one rank or when nothing is pending."""
    m = net.module if hasattr(net, 'module') else net
    if getattr(m, 'memory', None) is not None:
        m.memory.finish_commit()


def sync_commit(net=None):
    """Order the CURRENT stream behind the commit forward of the last agg_train_step (it reads every weight on its own stream). Needed before
    anything WRITES weights outside agg_train_step / mldg_train_step / optim.SGD.step / checkpoint.restore_snapshot, which wait by themselves:
    a foreign optimizer, an EMA update, in-place edits. No collective, no host synchronisation."""
    ops.wait_commit()


_WITHHELD = {}      # id(Memory_sup) -> weakref to the open GraphedAggStep(pipelined=True) whose last commit is withheld (m_items is one commit behind between replays)


def _check_not_withheld(net, what):
    """with GraphedAggStep(pipelined=True) open, `m_items` is one commit behind between replays -- a checkpoint, a validation pass or an mldg step that read it
    would silently see stale memory. Raise instead (as restore_snapshot does for an owed cross-rank commit): read g.committed_memory(), or g.close() first."""
    m = net.module if hasattr(net, 'module') else net
    ref = _WITHHELD.get(id(getattr(m, 'memory', None)))
    g = ref() if ref is not None else None
    if g is not None and not g.closed:
        raise RuntimeError('%s: a GraphedAggStep(pipelined=True) is open on this model -- its last memory commit is withheld until the next replay, so net.memory.m_items is '
                           'one commit behind. Use g.committed_memory() for the up-to-date memory, or g.close() before handing the model to eager code.' % what)


def save_checkpoint(path, net, optimizer=None, scheduler=None, epoch=0, mean_iu=0.0):
    """utils/misc.py:195-216 for the harness: EVERY rank calls it (it finishes a pending memory commit collectively), rank 0 writes the file."""
    from . import checkpoint
    _check_not_withheld(net, 'save_checkpoint')
    finish_commit(net)
    if not D.is_dist() or torch.distributed.get_rank() == 0:
        checkpoint.save_snapshot(path, net, optimizer, scheduler, epoch, mean_iu)


_TRAIN_OVERRIDES = {}      # frozenset of module classes -> does any of them override nn.Module.train()?


def set_mode(net, training):
    """net.train(training) without nn.Module.__setattr__ on each of the ~600 modules (0.5 ms per step over the three toggles of an agg step): the flag lives in
    each module's __dict__. The module tree is walked every time (modules may have been swapped: convert_sync_batchnorm). A tree in which some class overrides
    train() (frozen-BatchNorm variants, user wrappers that hook the mode switch) gets the real net.train(training): checked once per set of classes."""
    mods = list(net.modules())
    classes = frozenset(type(m) for m in mods)
    over = _TRAIN_OVERRIDES.get(classes)
    if over is None:
        over = _TRAIN_OVERRIDES[classes] = any(c.train is not torch.nn.Module.train for c in classes)
    if over:
        return net.train(training)
    for m in mods:
        m.__dict__['training'] = training
    return net


def _all_syncbn(m):
    """Every BatchNorm of the tree is a SyncBatchNorm (train.py:95)? Walked on every call -- only multi-rank steps under the DDP wrapper ask, and a conversion or a
    module swap after the first step must not be answered from a stale cache."""
    bns = [b for b in m.modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]
    return all(isinstance(b, torch.nn.SyncBatchNorm) for b in bns)


def _commit_forward(net, m, x, gts, aux_gts, mem_t, overlap, dist_on, truncate_second_forward=False, main=None):
    """The memory-commit forward of train.py:330-335: eval mode, no graph, post-SGD weights, starting from the memory `mem_t` the training forward read;
    on its own stream when `overlap` (the caller's stream otherwise). Returns the event recorded at its end (overlap) or None."""
    wrapped = hasattr(net, 'module')
    fwd_net = m if (overlap and wrapped) else net
    main = (torch.cuda.current_stream() if x.is_cuda else None) if main is None else main
    side = _commit_stream(x.device) if overlap else None
    done = None
    if overlap:
        side.wait_stream(main)
        for t in (x, gts, aux_gts, mem_t):
            t.record_stream(side)
    with torch.no_grad(), (torch.cuda.stream(side) if overlap else contextlib.nullcontext()):
        set_mode(net, False)
        m.memory.m_items = mem_t
        m.memory.defer_sync = overlap and dist_on
        ops.last_prefold_event, ops.fold_misses = None, 0
        try:
            if truncate_second_forward:
                memory_only_forward(net, x, gts)
            else:
                fwd_net(x, gts=gts, aux_gts=aux_gts, memory_writing=True)
        finally:
            m.memory.defer_sync = False
        set_mode(net, True)
        if overlap:
            done = side.record_event()
            m.memory.pending = done
            ops.commit_done[x.device.index] = done      # whoever writes weights next waits for it (optim.SGD.step, checkpoint restore, sync_commit)
    if overlap:
        # the next training forward rewrites the BatchNorm running moments: wait for the fold launch that read them (or, without one, for everything)
        main.wait_event(ops.last_prefold_event if (ops.last_prefold_event is not None and ops.fold_misses == 0) else done)
    return done


def agg_train_step(net, opt, x, gts, aux_gts=None, sched=None, buckets=None, truncate_second_forward=False, commit=True):
    """One iteration of train_memory_agg. `buckets` (dist.GradBuckets) replaces DDP's reducer for N > 1.
    commit=False withholds the memory-commit forward (GraphedAggStep(pipelined=True) runs it at the head of the next captured step, beside that step's
    training forward): the returned dict then carries `mem_t`, the memory the commit forward has to start from."""
    aux_gts = gts if aux_gts is None else aux_gts
    m = net.module if hasattr(net, 'module') else net
    set_mode(net, True)
    if x.is_cuda and x.shape[1] == 3:
        # both forward passes of the step read the same batch: lay it out once as the stem's NHWC / 4-channel input
        x = ops.nchw(K.nchw_to_nhwc(x.float(), c_pad=4))
    if buckets is not None:
        buckets.zero()
    else:
        opt.zero_grad()
    outputs = net(x, gts=gts, aux_gts=aux_gts, memory_writing=True, writing_detach=False)
    # train.py:312 clones the memory before the forward; it is re-assigned, never written in place (memory.py:253,256; Memory_sup.write here), so the
    # tensor the read just used IS that clone -- taken after the forward, because with an overlapped commit forward it only becomes final at that read
    mem_t = m.memory.last_read
    loss = total_loss(outputs)
    loss.backward()
    if buckets is not None:
        buckets.finish()
    opt.step()
    out = dict(loss1=outputs[0].detach(), loss2=outputs[1].detach(), readloss=outputs[-2].detach(), div=outputs[-3][0].detach(),
               cls=outputs[-3][1].detach(), total=loss.detach())
    if not commit:
        out['mem_t'] = mem_t
        if sched is not None:
            sched.step()
        return out
    dist_on = D.is_dist()
    # Under the reference's DDP wrapper (network/__init__.py:25-33) the commit forward goes through the bare module: DDP's forward would broadcast the
    # buffers on its own communicator, from a second stream. With every BatchNorm converted to SyncBatchNorm (train.py:95) the running moments are
    # already identical on all ranks, so that broadcast changes nothing; with local BatchNorms it does (rank 0's moments win) and the overlap stays off.
    wrapped = hasattr(net, 'module')
    overlap = COMMIT_OVERLAP and x.is_cuda and (not dist_on or (D.SYNC_MEMORY and (not wrapped or _all_syncbn(m))))
    _commit_forward(net, m, x, gts, aux_gts, mem_t, overlap, dist_on, truncate_second_forward)
    if sched is not None:
        sched.step()
    return out


def plain_train_step(net, opt, x, gts, aux_gts=None, sched=None, buckets=None):
    """One iteration of train_agg (train.py:634-700, calculate_loss :213-244) for a network WITHOUT memory (the IBN-Net baseline, or the plain trunk): zero_grad,
    the training forward, loss1 + 0.4 * loss2, backward, step. `buckets` (dist.GradBuckets) replaces DDP's reducer for N > 1. -> dict(loss1, loss2, total)."""
    aux_gts = gts if aux_gts is None else aux_gts
    m = net.module if hasattr(net, 'module') else net
    assert not m.args.memory, 'plain_train_step serves networks without memory; agg_train_step runs the others'
    set_mode(net, True)
    if x.is_cuda and x.shape[1] == 3:
        x = ops.nchw(K.nchw_to_nhwc(x.float(), c_pad=4))
    if buckets is not None:
        buckets.zero()
    else:
        opt.zero_grad()
    outputs = net(x, gts=gts, aux_gts=aux_gts)
    loss = outputs[0] + LOSS_W['aux'] * outputs[1]
    loss.backward()
    if buckets is not None:
        buckets.finish()
    opt.step()
    if sched is not None:
        sched.step()
    return dict(loss1=outputs[0].detach(), loss2=outputs[1].detach(), total=loss.detach())


class GraphedAggStep:
    """One agg train step (train forward + backward + SGD + memory-commit forward) captured in a hipGraph and replayed: ~1 300 kernel launches, their stream forks /
    joins and allocations become ONE graph launch per step. For the regime where the step is launch-bound -- the bf16 tier: 20 ms of Python + HIP enqueue per step
    against 26 ms of GPU time (DESIGN section 7 "Round 4"), i.e. host-bound as soon as the kernels get 20 % faster.

    What makes the step replayable: static input buffers (`x`, `gts` are copied in before each replay), the committed memory lives in one static buffer
    (`Memory_sup.m_items` points at it; the captured step reads it first and writes it last), weights / BatchNorm buffers / momentum buffers are updated in place, the
    learning rate is read from device memory (`optim.SGD.lr_device`, pm_sgd_momentum_multi_dev), random draws (gumbel noise, Dropout2d) go through torch's graph-safe
    generator, and the kept filter transforms are recomputed INSIDE the captured step exactly where an eager step recomputes them (after the SGD), so the
    cache stays consistent with the weights across replays. Single process only.

    pipelined=False: the commit forward runs serially at the END of the captured step (no cross-step overlap: a graph boundary is a join).
    pipelined=True (round 5): the captured unit is [commit forward of step t - 1 on its own stream  ||  training forward of step t] -> backward -> SGD, i.e. the eager
    path's cross-step overlap (worth 1.0-1.8 ms on the bf16 tier) INSIDE one graph: the commit forward of the previous batch (static copies `x_prev`, `gts_prev`, kept by
    the replay itself) forks off at the head of the graph, the training forward joins it where it reads the memory -- the same dependencies the eager overlapped step has
    (BatchNorm running moments: the training forward waits for the commit forward's one fold launch). Every step performs exactly the reference's operations in the
    reference's dependency order; what shifts is only WHEN the commit of step t is executed: at the head of replay t + 1. Hence `Memory_sup.m_items` is one commit
    behind between replays; `committed_memory()` returns the up-to-date memory (it runs the withheld commit forward eagerly into a scratch tensor, leaving the pipeline
    untouched) and `close()` folds it in and hands the model back to eager use.

        g = GraphedAggStep(net, opt, x, gts, sched=sched, pipelined=True)      # warms up eagerly, then captures
        losses = g.step(x, gts)                                  # every further step; tensors of the returned dict are overwritten by the next replay
        g.close()                                                # model, optimizer and memory are consistent for eager code again
    """

    def __init__(self, net, opt, x, gts, sched=None, warmup=3, pipelined=False, buckets=None):
        global COMMIT_OVERLAP
        assert x.is_cuda, 'GraphedAggStep: GPU training only'
        if D.is_dist():
            # N > 1 (round 6): the serial form only, with the build's GradBuckets, and only while EVERY exchange of the step (SyncBN moments / backward sums, the
            # memory-slot sum, the gradient buckets) is an RCCL call enqueued on the capturing stream through the direct communicator (rccl.py): those are
            # ordinary kernel nodes of the graph, replayed in the captured order on every rank. torch.distributed's own process group hops to an internal
            # stream and keeps host-side work objects -- not something to bake into a graph -- so dist.py raises if a capture would reach it.
            assert not pipelined, 'GraphedAggStep: pipelined=True is single-process (the withheld commit would defer a collective across a graph boundary)'
            assert buckets is not None and not hasattr(net, 'module'), 'GraphedAggStep under torch.distributed: pass the bare module and a dist.GradBuckets'
            assert D.direct_ready(x.device), 'GraphedAggStep under torch.distributed needs the direct RCCL communicator: ' + D.direct_fallback_reason()
        self.buckets = buckets
        assert len(opt.param_groups) == 1, 'GraphedAggStep: one parameter group (optimizer.py:21-25)'
        self.net, self.opt, self.sched, self.pipelined, self.closed = net, opt, sched, pipelined, False
        m = self.m = net.module if hasattr(net, 'module') else net
        self.x = ops.nchw(K.nchw_to_nhwc(x.float(), c_pad=4)) if x.shape[1] == 3 else x.clone()      # the stem's NHWC4 layout, converted once per step outside the graph
        self.gts = gts.clone()
        self.lr = torch.zeros(1, dtype=torch.float32, device=x.device)
        prev_overlap, COMMIT_OVERLAP = COMMIT_OVERLAP, False
        ok = False
        try:
            opt.lr_device = self.lr
            for _ in range(warmup):      # allocates workspaces, momentum buffers, filter caches, sets every kernel's LDS attribute
                self.lr.fill_(float(opt.param_groups[0]['lr']))
                agg_train_step(net, opt, self.x, self.gts, sched=sched, buckets=buckets)
            finish_commit(net)
            self.mem = m.memory.m_items.detach().clone()
            m.memory.m_items = self.mem
            if pipelined:
                import weakref
                _WITHHELD[id(m.memory)] = weakref.ref(self)
                # one more eager step whose commit is withheld: the state every replay starts from (weights after SGD t, memory committed through t - 1, batch t in x_prev)
                self.x_prev, self.gts_prev = self.x.clone(), self.gts.clone()
                self.lr.fill_(float(opt.param_groups[0]['lr']))
                agg_train_step(net, opt, self.x, self.gts, sched=sched, commit=False)
                m.memory.m_items = self.mem
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            self.lr.fill_(float(opt.param_groups[0]['lr']))
            with torch.cuda.graph(self.graph):
                if pipelined:
                    main = torch.cuda.current_stream()
                    side = _commit_stream(x.device)
                    self._commit(main, overlap=True)
                    self.out = agg_train_step(net, opt, self.x, self.gts, sched=None, commit=False)
                    self.out.pop('mem_t')
                    main.wait_stream(side)
                    self.x_prev.copy_(self.x)
                    self.gts_prev.copy_(self.gts)
                else:
                    self.out = agg_train_step(net, opt, self.x, self.gts, sched=None, buckets=buckets)
                    self.mem.copy_(m.memory.m_items)
                if ops.overlap_wgrad():      # every stream forked into the capture rejoins it (the weight-gradient stream's last event record trails its last join)
                    torch.cuda.current_stream().wait_stream(ops._side_stream())
            torch.cuda.synchronize()
            # events recorded inside the capture mean nothing to eager code (waiting for one from a non-capturing stream is an error): everything they ordered is complete
            m.memory.pending = None
            m.memory.m_items = self.mem
            ops.commit_done.pop(x.device.index, None)
            ops.last_prefold_event = None
            K.forget_filter_events()
            ok = True
        finally:
            COMMIT_OVERLAP = prev_overlap
            if not ok:      # a failed warm-up / capture must not leave the optimizer reading a dead device scalar or the memory pointing into the capture
                opt.lr_device = None
                m.memory.m_items = (self.mem if getattr(self, 'mem', None) is not None else m.memory._m_items).detach().clone()
                m.memory.pending = None
                ops.commit_done.pop(x.device.index, None)

    def _commit(self, main, overlap, into=None):
        """The withheld commit forward of the previous batch: from the static memory buffer, result copied back into it (or into `into`)."""
        m = self.m
        _commit_forward(self.net, m, self.x_prev, self.gts_prev, self.gts_prev, self.mem, overlap, False, main=main)
        m.memory.pending = None            # dropped, not waited for: the event below (after the copy-back) replaces it
        side = _commit_stream(self.x.device) if overlap else None
        done = None
        with torch.no_grad(), (torch.cuda.stream(side) if overlap else contextlib.nullcontext()):
            (self.mem if into is None else into).copy_(m.memory._m_items)
            if overlap:
                done = side.record_event()
        m.memory.m_items = self.mem
        if overlap:
            m.memory.pending = done       # the training forward's memory read (and the SGD: ops.commit_done) wait for the copy-back
            ops.commit_done[self.x.device.index] = done

    def step(self, x=None, gts=None):
        assert not self.closed, 'GraphedAggStep.step() after close()'
        if x is not None and x.data_ptr() != self.x.data_ptr():
            if x.shape[1] == 3:
                self.x.copy_(ops.nchw(K.nchw_to_nhwc(x.float(), c_pad=4)))
            else:
                self.x.copy_(x)
        if gts is not None and gts.data_ptr() != self.gts.data_ptr():
            self.gts.copy_(gts)
        self.lr.fill_(float(self.opt.param_groups[0]['lr']))
        self.graph.replay()
        if self.sched is not None:
            self.sched.step()
        return self.out

    def committed_memory(self):
        """The memory as of the last step INCLUDING its commit. pipelined: the withheld commit forward is run eagerly into a scratch tensor (the pipeline state --
        static memory buffer, x_prev -- is left as it is, so replays may continue); otherwise the static buffer itself."""
        if not self.pipelined or self.closed:
            return self.m.memory.m_items
        out = torch.empty_like(self.mem)
        self._commit(torch.cuda.current_stream(), overlap=False, into=out)      # reads the static buffer, writes `out`; m_items points at the static buffer again
        return out

    def close(self):
        """Hand model and optimizer back to eager code: the withheld commit (pipelined) is folded into `m_items`, the optimizer forgets the device-side learning
        rate of the capture (an eager opt.step() after a graphed phase silently used the LR of the last replay), graph-internal events are dropped."""
        if self.closed:
            return
        torch.cuda.synchronize()
        if self.pipelined:
            self._commit(torch.cuda.current_stream(), overlap=False)
            _WITHHELD.pop(id(self.m.memory), None)
        self.m.memory.m_items = self.mem.clone()
        self.m.memory.pending = None
        ops.commit_done.pop(self.x.device.index, None)
        if getattr(self.opt, 'lr_device', None) is self.lr:
            self.opt.lr_device = None
        self.closed = True
        torch.cuda.synchronize()


def memory_initialize(net, batches, epochs=2):
    """Class-prototype initialisation: sum of normalised bot_aspp features per soft class / count (no writenet).
    The reference builds a one-hot + F.interpolate per batch (train.py:1020-1030); here it is the write kernel's
    4-tap gather with normalize=1, summed across batches (and ranks) before the division."""
    m = net.module if hasattr(net, 'module') else net
    mem = m.memory
    net.eval()
    acc = None
    with torch.no_grad():
        for _ in range(epochs):
            for x, gt in batches:
                feat = net(x, gts=gt, aux_gts=gt)[-1]
                nomden = K.mem_write_accum(K.cast(ops.nhwc(feat), torch.float32), gt.contiguous(), mem.memory_size, normalize=True)
                acc = nomden if acc is None else acc + nomden
        acc = D.all_reduce_sum(acc)
        s, d = mem.memory_size, mem.feature_dim
        basket = acc[:(s + 1) * d].view(s + 1, d)[:s]
        count = acc[(s + 1) * d:][:s].clone().unsqueeze(1)
        count[count == 0] = 1
        mem.m_items = F.normalize(basket / count, dim=1)
    net.train()
    return mem.m_items


def sliding_tiles(h, w, crop, overlap=1.0 / 3, scale=1.0):
    """eval.py:158-182: [(x1,y1,x2,y2)] in the reference's order."""
    tile = int(crop * max(scale, 1.0))
    stride = math.ceil(tile * (1 - overlap))
    rows = int(math.ceil((w - tile) / stride) + 1)
    cols = int(math.ceil((h - tile) / stride) + 1)
    out = []
    for r in range(rows):
        for c in range(cols):
            x2, y2 = min(int(r * stride) + tile, w), min(int(c * stride) + tile, h)
            out.append((max(int(x2 - tile), 0), max(int(y2 - tile), 0), x2, y2))
    return out


def sliding_logits(net, img, crop, overlap=1.0 / 3, flips=(False, True), batch_tiles=True):
    """Single-scale sliding-window logits for one CHW image, stitched on the GPU in float64 (the reference stitches
    per class in numpy threads, eval.py:210-274). Logits (not probabilities) are averaged (eval.py:380-392); the count
    divides by the true per-pixel tile count (the reference's count array is mis-indexed but class-uniform)."""
    c, h, w = img.shape
    tiles = sliding_tiles(h, w, crop, overlap)
    net.eval()
    acc = None
    with torch.no_grad():
        for flip in flips:
            src = torch.flip(img, dims=[2]) if flip else img
            crops = torch.stack([src[:, y1:y2, x1:x2] for (x1, y1, x2, y2) in tiles])
            outs = net(crops)[0] if batch_tiles else torch.cat([net(cr[None])[0] for cr in crops])   # eval.py:379-390 (--faster batches)
            if len(tiles) <= STITCH_MAX_TILES and outs.is_cuda:
                # one kernel per flip: float64 sum of the covering tiles (tile order) / count, written un-flipped into the accumulator
                acc = K.sliding_stitch(ops.nhwc(outs), tiles, h, w, flip, acc)
            else:
                acc = _stitch_torch(outs, tiles, h, w, flip, acc)
    return acc / len(flips)


STITCH_MAX_TILES = 64      # pm_sliding_stitch takes the tile table by value in its kernel arguments


def _stitch_torch(outs, tiles, h, w, flip, acc):
    """The same stitching in stock float64 torch ops for what the kernel does not take: more than 64 tiles per image (a 1024 x 2048 image at
    crop 256 has 72) -- same sums in the same tile order, the same division by the true count, the same un-flip."""
    full = torch.zeros(outs.shape[1], h, w, dtype=torch.float64, device=outs.device)
    cnt = torch.zeros(1, h, w, dtype=torch.float64, device=outs.device)
    for lg, (x1, y1, x2, y2) in zip(outs, tiles):
        full[:, y1:y2, x1:x2] += lg.to(torch.float64)
        cnt[:, y1:y2, x1:x2] += 1
    full = full / cnt
    if flip:
        full = torch.flip(full, dims=[2])
    return full if acc is None else acc + full


def fast_hist(pred, gt, n=19):
    """utils/misc.py:65-70 as one device bincount."""
    pred, gt = pred.reshape(-1), gt.reshape(-1)
    k = (gt >= 0) & (gt < n)
    return torch.bincount(n * gt[k].long() + pred[k].long(), minlength=n * n).view(n, n)


def miou(hist):
    hist = hist.double()
    iu = torch.diag(hist) / (hist.sum(1) + hist.sum(0) - torch.diag(hist))
    return float(torch.nanmean(iu)), iu


# ---- the validation loop every training script runs after each epoch (train.py:847-939) ---------------------------------------
def validate(net, batches, criterion=None, classes=19, dump=10, decode=None, tables=None):
    """train.py:847-939 without the logging, the checkpointing and the distributed reduce (the caller sums `hist` across ranks where the reference
    all-reduces iou_acc). Per batch: one eval forward that returns the head's LOW-RES logits, then one kernel that up-samples them, evaluates the
    criterion, takes output.max(1)[1] and adds fast_hist into the running histogram (K.upsample_eval) -- the [n,19,H,W] logits are never written and
    nothing is copied to the host before the last batch. `batches` yields (inputs, gt, ...); a [B,D,C,H,W] input is flattened (:872-875). A criterion
    other than the plain CrossEntropyLoss(ignore_index=255), or a shape the kernel does not take, goes through resize + criterion + argmax + fast_hist
    on the device (correct, not tuned). The loss means carry the reference's AverageMeter weighting: each batch's mean by n*H*W, ignored pixels
    included (:880,903). The class maps of the first `dump` batches are kept (the reference's image dumps). Leaves the net in eval mode.
    decode (an input_edge.LabelDecode; None = gt holds train ids) with tables (one table index of `decode` for every image, or one entry per image of a batch after
    the leading axes merged; -1 / None = pass-through): gt is the dataset's raw uint8 mask, [.., H, W] ids or [.., H, W, 3] colours, decoded on the device first.
    -> dict(val_loss, read_loss (None without the memory), hist int64 [C,C] on the device, mean_iu, iu, predictions: list of uint8 [n,H,W])."""
    from .network.deepv3plus import fused_ce_ok
    m = net.module if hasattr(net, 'module') else net
    device = next(m.parameters()).device
    with_memory = bool(getattr(m.args, 'memory', False))
    fused = criterion is None or fused_ce_ok(criterion)
    net.eval()
    hist = torch.zeros((classes, classes), dtype=torch.int64, device=device)
    sums = torch.zeros(3, dtype=torch.float64, device=device)      # sum of loss * pixels, of read loss * pixels, of pixels
    predictions = []
    was = m.eval_logits_lowres
    m.eval_logits_lowres = True
    try:
        with torch.no_grad():
            for idx, data in enumerate(batches):
                inputs, gt = data[0], data[1]
                if decode is not None:                                     # raw masks: decoded on the device before anything else
                    h, w = inputs.shape[-2:]
                    raw = gt.to(device).reshape(-1, *((h, w, 3) if gt.dim() == inputs.dim() else (h, w))).contiguous()
                    entries = [tables] * raw.shape[0] if tables is None or isinstance(tables, int) else tables
                    gt = K.labels_u8_to_i64(decode.decode(raw, entries))
                if inputs.dim() == 5:
                    inputs = inputs.reshape(-1, *inputs.shape[2:])
                    gt = gt.reshape(-1, *inputs.shape[2:])
                assert inputs.dim() == 4 and gt.dim() == 3 and inputs.shape[2:] == gt.shape[1:]
                pixels = inputs.shape[0] * inputs.shape[2] * inputs.shape[3]
                inputs, gt = inputs.to(device), gt.to(device).contiguous()
                outputs = net(inputs)
                low = outputs[0]
                assert low.shape[1] == classes
                lv = ops.nhwc(low)
                if fused and K.upsample_eval_ok(lv, tuple(gt.shape[1:])):
                    loss_out, _, pred = K.upsample_eval(lv, gt, 1.0, hist=hist, want_pred=idx < dump)
                    loss = loss_out[0]
                else:
                    full = ops.resize(low, tuple(gt.shape[1:]))
                    loss = F.cross_entropy(full, gt, ignore_index=255) if criterion is None else criterion(full, gt)
                    pred = full.argmax(1)
                    hist += fast_hist(pred, gt, classes)
                    pred = pred.to(torch.uint8)
                if idx < dump:
                    predictions.append(pred)
                sums[0] += loss.double() * pixels
                sums[2] += pixels
                if with_memory:
                    query = F.normalize(outputs[-1], dim=1).permute(0, 2, 3, 1).contiguous()
                    sums[1] += m.memory.get_score(query, gt, m.memory.m_items)[-1].double() * pixels
    finally:
        m.eval_logits_lowres = was
    sums = sums.cpu()
    mean_iu, iu = miou(hist)
    return dict(val_loss=float(sums[0] / sums[2]), read_loss=float(sums[1] / sums[2]) if with_memory else None, hist=hist, mean_iu=mean_iu, iu=iu,
                predictions=predictions)


# ---- sliding-window evaluation: what every eval_*.sh runs (eval.py --inference_mode sliding; :340-405, :630-653, :695-702) ----------------------------
def _scaled_u8(img, scale):
    """eval.py:357-358: img.resize((int(w * scale), int(h * scale)), Image.BILINEAR) of a HOST uint8 [H, W, 3] image."""
    import numpy as np
    from PIL import Image
    if img.is_cuda:
        raise ValueError('evaluate_sliding: a scale other than 1 is resized by PIL on the host -- pass the image as a host tensor')
    h, w = img.shape[:2]
    pil = Image.fromarray(img.contiguous().numpy()).resize((int(w * scale), int(h * scale)), Image.BILINEAR)
    return torch.from_numpy(np.array(pil))


def tile_stack(parts):
    """The heads' low-res logits of every forward of one (image, scale), NHWC views [n_i, h, w, C] in the order K.sliding_eval reads them -> ONE [sum n_i, h, w, C] view
    whose pixels keep the heads' 16-byte pitch (K.new(pitch_pad=True): 20 floats for 19 classes), which the kernels' 16-byte loads need. torch.cat would pack the
    pixels to C floats and send every launch to the 4-byte loads (profiles/sliding_eval_probe.txt). A single part that has that pitch is handed on as it is."""
    if len(parts) == 1 and parts[0].stride(2) % 4 == 0 and parts[0].data_ptr() % 16 == 0:
        return parts[0]
    _, h, w, c = parts[0].shape
    low = K.new((sum(p.shape[0] for p in parts), h, w, c), parts[0], pitch_pad=True, dtype=torch.float32)
    at = 0
    for p in parts:
        low[at:at + p.shape[0]].copy_(p)
        at += p.shape[0]
    return low


def evaluate_sliding(net, img, gt=None, crop=768, scales=(1.0,), overlap=1.0 / 3, flips=(False, True), hist=None, want_logits=False, batch_tiles=True,
                     device_tiles=False):
    """eval.py:340-405 (inference_sliding) and :647-653 (mean over the scales, argmax, fast_hist) for ONE image. Per scale: the image is scaled (PIL on the host; scale 1
    is sliced on the device as it is), normalised (K.image_u8_to_nhwc4), cut into sliding_tiles and forwarded -- mirrored too unless flips=(False,) -- with the heads
    returning their LOW-RES logits; one K.sliding_eval launch sequence then up-samples, stitches, un-flips and averages them without writing the up-sampled tiles or
    a stitched map. At scales=(1.0,) the same launch takes the argmax and adds fast_hist(pred, gt) into `hist`; with more scales each one is resampled to the image's
    size (cv2.resize INTER_LINEAR) into a float64 accumulator and K.sliding_eval_finish yields the class map and the histogram. Nothing is copied to the host.
    img: uint8 [H, W, 3], host or device; a normalised float [3, H, W] is taken when every scale is 1. gt: [H, W] train ids (255 = ignore) or None. hist: int64
    [C, C] on the device to add into (None: a fresh one when gt is given). batch_tiles=False forwards tile by tile (eval.py:383-390, without --faster).
    device_tiles=True: the uint8 image, host or device, goes to the device once and every scale, 1.0 included, takes its crops of both flips from ONE
    K.eval_tiles_u8 launch (PIL's bilinear bytes, the mirror image, the normalisation and the cropping; the tables come from K.eval_tile_plan's cache) instead of
    PIL on the host + K.image_u8_to_nhwc4 + torch.flip + slices + torch.stack: the same bits, so the same result. A float image raises ValueError with it; a scale
    the library's tables do not hold raises its PinmemError.
    -> dict(pred uint8 [H, W], hist, logits float64 [C, H, W] with want_logits else None). Leaves the net in eval mode."""
    m = net.module if hasattr(net, 'module') else net
    device = next(m.parameters()).device
    scales, flips = tuple(float(s) for s in scales), tuple(bool(f) for f in flips)
    assert len(scales) >= 1 and flips in ((False,), (False, True)), 'flips: (False,) or (False, True) -- the image, then its mirror (eval.py:362-370)'
    as_u8 = img.dtype == torch.uint8
    if as_u8:
        assert img.dim() == 3 and img.shape[2] == 3, 'uint8 images are [H, W, 3]'
        H, W = img.shape[:2]
    else:
        if any(s != 1.0 for s in scales):
            raise ValueError('evaluate_sliding: a normalised float image cannot be re-scaled as the reference scales its uint8 image; pass uint8 [H, W, 3]')
        assert img.dim() == 3 and img.shape[0] == 3 and img.is_floating_point(), 'float images are normalised [3, H, W]'
        H, W = img.shape[1:]
    if device_tiles:
        if not as_u8:
            raise ValueError('evaluate_sliding: device_tiles=True scales and normalises the uint8 [H, W, 3] image itself; a normalised float image has no bytes to scale')
        img = img.to(device).contiguous()
    if gt is not None:
        gt = gt.to(device=device, dtype=torch.int64).reshape(H, W).contiguous()
    single = scales == (1.0,)
    net.eval()
    acc = None
    was = m.eval_logits_lowres
    m.eval_logits_lowres = True
    try:
        with torch.no_grad():
            for i, s in enumerate(scales):
                if device_tiles:
                    plan = K.eval_tile_plan(H, W, s, crop, overlap, device)
                    Hs, Ws, tiles = plan.Hs, plan.Ws, plan.tiles
                    x = K.eval_tiles_u8(img, plan, len(flips))      # [F * T, th, tw, 4]
                elif as_u8:
                    x = K.image_u8_to_nhwc4((img if s == 1.0 else _scaled_u8(img, s)).to(device)[None].contiguous())[0]      # [Hs, Ws, 4]
                    Hs, Ws = x.shape[:2]
                else:
                    x, Hs, Ws = img.to(device), H, W
                if not device_tiles:
                    tiles = sliding_tiles(Hs, Ws, crop, overlap, s)
                lows = []
                for k, flip in enumerate(flips):
                    if device_tiles:
                        crops = ops.nchw(x[k * len(tiles):(k + 1) * len(tiles)])
                    elif as_u8:
                        src = torch.flip(x, dims=[1]) if flip else x
                        crops = ops.nchw(torch.stack([src[y1:y2, x1:x2] for (x1, y1, x2, y2) in tiles]))
                    else:
                        src = torch.flip(x, dims=[2]) if flip else x
                        crops = torch.stack([src[:, y1:y2, x1:x2] for (x1, y1, x2, y2) in tiles])
                    lows += [ops.nhwc(net(crops)[0])] if batch_tiles else [ops.nhwc(net(cr[None])[0]) for cr in crops]
                low = tile_stack(lows)
                assert low.stride(2) % 4 == 0, 'evaluate_sliding: the logits handed to K.sliding_eval lost the 16-byte pixel pitch of the heads (%d floats)' % low.stride(2)
                if single:
                    pred, hist, logits = K.sliding_eval(low, tiles, (Hs, Ws), (H, W), len(flips), labels=gt, hist=hist, want_pred=True, want_logits=want_logits)
                else:
                    if acc is None:
                        acc = torch.empty((low.shape[3], H, W), dtype=torch.float64, device=device)
                    K.sliding_eval(low, tiles, (Hs, Ws), (H, W), len(flips), acc=acc, acc_add=i > 0)
            if not single:
                pred, hist, logits = K.sliding_eval_finish(acc, len(scales), labels=gt, hist=hist, want_pred=True, logits_out=acc if want_logits else None)
    finally:
        m.eval_logits_lowres = was
    return dict(pred=pred, hist=hist, logits=logits)


def eval_metrics(hist):
    """utils/misc.py:132-148 evaluate_eval_for_inference on the device, in float64: (acc, acc_cls, mean_iu, fwavacc) as a [4] tensor."""
    h = hist.double()
    diag, rows, total = torch.diag(h), h.sum(1), h.sum()
    iu = diag / (rows + h.sum(0) - diag)
    freq = rows / total
    return torch.stack([diag.sum() / total, torch.nanmean(diag / rows), torch.nanmean(iu), torch.where(freq > 0, freq * iu, torch.zeros_like(iu)).sum()])


def _dump_tables(who, palette, id_to_trainid):
    """The host halves of what K.eval_dump reads per call: the checked palette and the label-id table (None without id_to_trainid). No device involved."""
    if palette is None:
        raise ValueError('%s: on_images needs the palette (uint8 [256, 3] RGB) -- the library ships no colour table' % who)
    palette = torch.as_tensor(palette)
    if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3):
        raise ValueError('%s: the palette is uint8 [256, 3] (got %s %s)' % (who, palette.dtype, tuple(palette.shape)))
    return palette, None if id_to_trainid is None else K.trainid_table(id_to_trainid)


def _dump_source(who, img):
    """One loader image -> uint8 [H, W, 3]: the bytes the composed image blends with."""
    img = img[0] if img.dim() == 4 else img
    if img.dtype != torch.uint8:
        raise ValueError('%s: image dumps blend the uint8 [H, W, 3] source image; a normalised float image has no bytes to blend' % who)
    assert img.dim() == 3 and img.shape[2] == 3, 'uint8 images are [H, W, 3]'
    return img


def evaluate(net, loader, crop=768, scales=(1.0,), overlap=1.0 / 3, no_flip=False, classes=19, dump=0, device_tiles=False, on_images=None, palette=None,
             id_to_trainid=None, alpha=0.5):
    """The loop of eval.py:756-779 over RunEval.inf (:630-653) and final_dump (:695-702); the image files of --dump_images are the caller's, from what on_images hands out: `loader` yields (image, gt, ...) with the image
    uint8 [H, W, 3] (or [1, H, W, 3]) and gt [H, W] (or [1, H, W]); every image goes through evaluate_sliding into ONE histogram on the device, and nothing is
    copied to the host before the last image. -> dict(hist int64 [classes, classes] on the device, acc, acc_cls, mean_iu, fwavacc as evaluate_eval_for_inference
    computes them, predictions: the uint8 class maps of the first `dump` images). device_tiles: as evaluate_sliding takes it.
    on_images (--dump_images, eval.py:664-693): called as on_images(idx, data, images) per image, `data` the loader's item and `images` K.eval_dump's dict of device
    tensors for the image's class map, source image and gt -- 'color', 'compose', 'diff' [H, W, 3] and, with id_to_trainid (the dataset's dict), 'ids' [H, W].
    palette: uint8 [256, 3] RGB, required with on_images; alpha: the blend's. Palette and id table go to the device once; the harness copies nothing to the host,
    encoding and files stay with the caller. A float image raises ValueError with on_images."""
    if on_images is not None:
        palette, id_table = _dump_tables('evaluate', palette, id_to_trainid)
    m = net.module if hasattr(net, 'module') else net
    device = next(m.parameters()).device
    if on_images is not None:
        palette, id_table = palette.to(device).contiguous(), None if id_table is None else id_table.to(device)
    hist = torch.zeros((classes, classes), dtype=torch.int64, device=device)
    predictions = []
    for idx, data in enumerate(loader):
        img, gt = data[0], data[1]
        img = img[0] if img.dim() == 4 else img
        if on_images is not None:
            src = _dump_source('evaluate', img).to(device).contiguous()
            if device_tiles:
                img = src      # one upload serves the tiles and the blend
        res = evaluate_sliding(net, img, gt, crop, scales, overlap, (False,) if no_flip else (False, True), hist=hist, device_tiles=device_tiles)
        if idx < dump:
            predictions.append(res['pred'])
        if on_images is not None:
            labels = gt.to(device=device, dtype=torch.int64).reshape(src.shape[:2]).contiguous()
            want = ('color', 'compose', 'diff') + (('ids',) if id_table is not None else ())
            on_images(idx, data, K.eval_dump(res['pred'], palette=palette, image=src, labels=labels, id_table=id_table, alpha=alpha, want=want))
    acc, acc_cls, mean_iu, fwavacc = eval_metrics(hist).tolist()
    return dict(hist=hist, acc=acc, acc_cls=acc_cls, mean_iu=mean_iu, fwavacc=fwavacc, predictions=predictions)


def segment_folder(net, loader, on_images, palette, id_to_trainid=None, crop=768, scales=(1.0,), overlap=1.0 / 3, no_flip=False, alpha=0.5, device_tiles=False):
    """The `video_folder` loop of eval.py:757-779 (eval_custumfolder_pinmem_DR50V3P.sh): images without ground truth, so no histogram, no metrics and no diff image --
    the colourised frames and overlays are the whole product. `loader` yields a uint8 [H, W, 3] (or [1, H, W, 3]) image, or a tuple / list whose first item is one
    (the reference's (imgs, img_names)). Every image goes through evaluate_sliding(gt=None) and K.eval_dump, and on_images(idx, data, images) receives the loader's
    item and the device tensors 'color', 'compose' [H, W, 3] and, with id_to_trainid, 'ids' [H, W]. palette, alpha, device_tiles: as evaluate takes them.
    -> the number of images."""
    palette, id_table = _dump_tables('segment_folder', palette, id_to_trainid)
    if on_images is None:
        raise ValueError('segment_folder: on_images is the only product of this loop')
    m = net.module if hasattr(net, 'module') else net
    device = next(m.parameters()).device
    palette, id_table = palette.to(device).contiguous(), None if id_table is None else id_table.to(device)
    want = ('color', 'compose') + (('ids',) if id_table is not None else ())
    count = 0
    for idx, data in enumerate(loader):
        img = _dump_source('segment_folder', data[0] if isinstance(data, (tuple, list)) else data)
        src = img.to(device).contiguous()
        res = evaluate_sliding(net, src if device_tiles else img, None, crop, scales, overlap, (False,) if no_flip else (False, True), device_tiles=device_tiles)
        on_images(idx, data, K.eval_dump(res['pred'], palette=palette, image=src, id_table=id_table, alpha=alpha, want=want))
        count += 1
    return count


# ---- the ablation sweep: ablation.py RunAbla.tsne_memact (:317-399) with tsnelib.py RunTsne (:48-96), without t-SNE, figures and files ------------------------
class FeatureBasket:
    """RunTsne's basket (tsnelib.py:48-96) without the plotting: per image and per selected class with at least one pixel, the mean L2-normalised feature vector of
    the class, with its class and domain labels -- image-major, then in the order of selected_clsid; absent classes are dropped. Nothing is copied to the host while the
    basket fills (the reference reads 19 counts per image back): the rows of an image are kept with a presence mask and compacted once, when they are read."""

    def __init__(self, selected_clsid, classes=19):
        self.selected_clsid = [int(c) for c in selected_clsid]
        assert all(0 <= c < classes for c in self.selected_clsid), 'selected classes lie in [0, %d)' % classes
        self.classes = classes
        self.init_basket()

    def init_basket(self):
        self._means, self._present, self._domains = [], [], []
        self.mem_vecs = self.mem_vec_labels = None

    def add_sums(self, sums, counts, domain_id):
        """sums [n, classes + 1, C] and counts [n, classes + 1] of K.class_sums / K.label_splat (any device): the kernel-free half of add()."""
        assert sums.dim() == 3 and tuple(counts.shape) == tuple(sums.shape[:2]) and sums.shape[1] == self.classes + 1
        sel = torch.as_tensor(self.selected_clsid, dtype=torch.int64, device=sums.device)
        cnt = counts.index_select(1, sel)
        self._means.append(sums.index_select(1, sel) / cnt.clamp(min=1).to(sums.dtype).unsqueeze(-1))      # tsnelib.py:69 nominator[slot] / denominator[slot]
        self._present.append(cnt != 0)
        self._domains.append(int(domain_id))

    def add(self, features, labels, domain_id, splat=None):
        """features: logical-NCHW [n, C, h, w] (fp32 / bf16, channels-last memory), labels int64 [n, H, W]; splat: (splat, counts) of K.label_splat for these labels
        and this feature size, when the caller already has it (one splat serves both baskets of the sweep)."""
        splat, counts = splat if splat is not None else K.label_splat(labels, tuple(features.shape[2:]), self.classes)
        self.add_sums(K.class_sums(features, splat), counts, domain_id)

    def input_memory_item(self, m_items):
        sel = torch.as_tensor(self.selected_clsid, dtype=torch.int64, device=m_items.device)
        self.mem_vecs = m_items.detach().index_select(0, sel)
        self.mem_vec_labels = sel

    def vectors(self):
        """-> (vectors [rows, C], class labels int64 [rows], domain labels int64 [rows]) as draw_tsne takes them (tsnelib.py:90-92): the rows normalised with
        F.normalize(dim=1). If memory items were given, the selected items follow the feature rows as they are (draw_tsne(plot_memory=True), :145-147), with their
        slot as class label and domain -1. The one host synchronisation of the basket happens here (the boolean compaction)."""
        if not self._means:
            dev = self.mem_vecs.device if self.mem_vecs is not None else 'cpu'
            vecs, labels, domains = torch.zeros((0, 0), device=dev), torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
        else:
            means, present = torch.cat(self._means), torch.cat(self._present)
            dev, S = means.device, len(self.selected_clsid)
            keep = present.reshape(-1)
            vecs = F.normalize(means.reshape(-1, means.shape[-1])[keep].float(), dim=1)
            labels = torch.as_tensor(self.selected_clsid, dtype=torch.int64, device=dev).repeat(present.shape[0])[keep]
            per_image = torch.as_tensor([d for d, p in zip(self._domains, self._present) for _ in range(p.shape[0])], dtype=torch.int64, device=dev)
            domains = per_image.repeat_interleave(S)[keep]
        if self.mem_vecs is not None:
            mv = self.mem_vecs.to(vecs.device).float()
            vecs = torch.cat([vecs, mv]) if vecs.numel() else mv
            labels = torch.cat([labels, self.mem_vec_labels.to(labels.device)])
            domains = torch.cat([domains, torch.full((mv.shape[0],), -1, dtype=torch.int64, device=domains.device)])
        return vecs, labels, domains


def memory_activation(mem_output, size, slots, palette=None, image=None, alpha=0.65):
    """ablation.py:371-399 for one batch: mem_output is the memory entry of a net's eval outputs ([p_query, p_mem, refined features]); its soft-max over the slots,
    mem_output[1] [n, h, w, m], is up-sampled to size = (H, W), min-max normalised per pixel over the slots and mapped for every slot of `slots` -- in one kernel
    (K.mem_actmap). -> dict: 'bytes', plus 'rgb' with a palette (uint8 [256, 3] RGB on the device) and 'blend' with palette and image (uint8 [n, H, W, 3])."""
    pm = mem_output[1]
    n, h, w, _ = pm.shape
    want = ('bytes',) + (('rgb',) if palette is not None else ()) + (('blend',) if palette is not None and image is not None else ())
    return K.mem_actmap(pm, (n, h, w), size, slots, palette=palette, image=image, alpha=alpha, want=want)


def ablation_sweep(net, loader, selected_clsid, domain_id, max_images=600, on_maps=None, palette=None):
    """RunAbla.tsne_memact's loop (ablation.py:317-399) over one domain's loader, on the device. `loader` yields (inputs, gt, ...): inputs either the normalised fp32
    [b, 3, H, W] batch the net takes, or uint8 [b, H, W, 3] images, which are normalised on the device and are then also the background of the blended maps; gt
    [b, H, W] train ids. Per batch: one eval forward under no_grad (low-res logits: they are not used), one label splat, the class sums of inter_feature (the last
    output) into the first basket and, for a memory net, of the refined features (mem_output[-1]) into the second. on_maps (memory nets): called as
    on_maps(first image index, maps) with memory_activation's dict for the batch, slots = selected_clsid. At most max_images images are taken (--imagenum_dom).
    -> (basket, basket of the refined features or None). t-SNE, figures and files stay with the caller."""
    m = net.module if hasattr(net, 'module') else net
    device = next(m.parameters()).device
    with_memory = bool(getattr(m.args, 'memory', False))
    basket = FeatureBasket(selected_clsid)
    updated = FeatureBasket(selected_clsid) if with_memory else None
    net.eval()
    was = m.eval_logits_lowres
    m.eval_logits_lowres = True
    count = 0
    try:
        with torch.no_grad():
            for data in loader:
                if count >= max_images:
                    break
                inputs, gt = data[0], data[1]
                image = None
                if inputs.dtype == torch.uint8:
                    image = inputs.reshape(-1, *inputs.shape[-3:])[:max_images - count].to(device).contiguous()
                    inputs = ops.nchw(K.image_u8_to_nhwc4(image))
                else:
                    inputs = inputs.reshape(-1, *inputs.shape[-3:])[:max_images - count].to(device)
                H, W = inputs.shape[2:]
                gt = gt.reshape(-1, H, W)[:inputs.shape[0]].to(device).contiguous()
                outputs = net(inputs)
                features = outputs[-1]
                splat = K.label_splat(gt, tuple(features.shape[2:]))
                basket.add(features, gt, domain_id, splat)
                if with_memory:
                    mem_output = outputs[-2]
                    updated.add(mem_output[-1], gt, domain_id, splat)
                    if on_maps is not None:
                        on_maps(count, memory_activation(mem_output, (H, W), selected_clsid, palette=palette, image=image))
                count += inputs.shape[0]
    finally:
        m.eval_logits_lowres = was
    if with_memory:
        items = m.memory.m_items.clone().detach()
        basket.input_memory_item(items), updated.input_memory_item(items)
    return basket, updated


# ---- the meta-learning regime every pinmem script runs: train_memory_mldg (train.py:493-632) ----------------------------
def put_theta(model, theta):
    """train.py:262-277: rewire every leaf module's _parameters with (non-leaf) tensors; the HIP ops take weights as
    autograd inputs at call time, so functional parameters work without touching the modules."""
    def walk(mod, name=None):
        if len(mod._modules) != 0:
            for k, v in mod._modules.items():
                walk(v, str(k) if name is None else str(name + '.' + k))
        else:
            for k, v in mod._parameters.items():
                if isinstance(v, torch.Tensor):
                    mod._parameters[k] = theta[str(name + '.' + k)]
    walk(model)
    return model


def functional_theta(old, lr):
    """train.py:246-260: theta' = theta - lr * grad (first order) for every parameter that has a gradient, the detached value otherwise (the reference takes the
    state_dict entry there). The ~160 multiply / subtract pairs are two multi-tensor launches (same arithmetic, same bits as `p - lr * p.grad` one by one): 640 tiny
    launches and ~6 ms of host time per mldg step less. Only parameters: put_theta rewires nothing else."""
    names, ps = [], []
    for k, p in old.named_parameters():
        names.append(k)
        ps.append(p)
    idx = [i for i, p in enumerate(ps) if p.grad is not None]
    # lr: a python float, or a 0-dim fp32 device tensor (GraphedMldgStep: the annealed inner rate changes between replays) -- the same fp32 multiply either way
    upd = torch._foreach_sub([ps[i] for i in idx], torch._foreach_mul([ps[i].grad for i in idx], lr)) if idx else []
    theta = {k: p.detach() for k, p in zip(names, ps)}
    for i, u in zip(idx, upd):
        theta[names[i]] = u
    return theta


def get_updated_network(old, new, lr, theta=None):
    """train.py:246-260: `new` rewired with theta' = theta - lr * grad of `old` (first order)."""
    return put_theta(new, functional_theta(old, lr) if theta is None else theta)


INNER_LR = 0.001      # train.py:1208 `--inner_lr` default


def annealed_inner_lr(opt):
    """train.py:625-626 (`--inner_lr_anneal`, passed by every pinmem script: train_GS_pinmem_DR50V3P.sh:18): after each scheduler step the inner
    learning rate of the NEXT iteration is a quarter of the outer one."""
    return opt.param_groups[-1]['lr'] / 4


def mldg_train_step(net, updated_net, updated_net2, opt, x_tr, y_tr, x_te, y_te, inner_lr=INNER_LR, sched=None, inner_lr_anneal=False):
    """One iteration of train_memory_mldg (memory configuration, whitening off): inner step on the meta-train domains,
    frozen-encoder memory write with the stepped weights, read-only meta-test forward whose loss back-propagates through the
    WRITTEN memory into the write graph (memory.py:323-324 only detaches when writing), outer step, memory commit.
    inner_lr: the reference's default 1e-3 (train.py:1208); with inner_lr_anneal the returned dict carries `next_inner_lr` = lr / 4 of the
    outer schedule after this step (train.py:625-626) for the caller to pass into the next iteration."""
    _check_not_withheld(net, 'mldg_train_step')
    set_mode(net, True)
    finish_commit(net)          # every rank is here: a memory commit deferred by a preceding agg step is finished before m_items is read
    mem_t = net.memory.m_items.clone().detach()
    opt.zero_grad()
    out_in = net(x_tr, gts=y_tr, aux_gts=y_tr, memory_writing=True, writing_detach=False)
    inner = total_loss(out_in)
    inner.backward(retain_graph=True)
    # both functional networks carry the same theta' (train.py:543,546 build it twice from the same gradients); the second one's encoder is frozen (train.py:549-552):
    # its non-memory entries are the detached values
    theta = functional_theta(net, inner_lr)
    updated_net = set_mode(get_updated_network(net, updated_net, inner_lr, theta), True)
    theta2 = {k: (v if k.split('.')[0] == 'memory' else v.detach()) for k, v in theta.items()}
    updated_net2 = set_mode(get_updated_network(net, updated_net2, inner_lr, theta2), True)
    updated_net2.memory.m_items = mem_t
    updated_net2(x_tr, gts=y_tr, aux_gts=y_tr, memory_writing=True, writing_detach=False)
    updated_net.memory.m_items = updated_net2.memory.m_items.clone()
    out_te = updated_net(x_te, gts=y_te, aux_gts=y_te, memory_writing=False)
    outer = out_te[0] + LOSS_W['aux'] * out_te[1] + LOSS_W['read'] * out_te[-2]
    outer.backward()
    opt.step()
    with torch.no_grad():
        set_mode(net, False)
        net.memory.m_items = mem_t
        net(x_tr, gts=y_tr, aux_gts=y_tr, memory_writing=True)
        set_mode(net, True)
    if sched is not None:
        sched.step()
    out = dict(inner=inner.detach(), outer=outer.detach(), inner_loss1=out_in[0].detach(), outer_loss1=out_te[0].detach(),
               outer_read=out_te[-2].detach())
    if inner_lr_anneal:
        out['next_inner_lr'] = annealed_inner_lr(opt)
    return out


def release_functional_state(net, *functional_nets):
    """Drop every reference the harness objects hold into the autograd graph of an earlier iteration: the functional networks' theta' (rewired to detached views of
    `net`'s parameters), the memories written without detaching, the deferred weight proxies of the last forward. See GraphedMldgStep.__init__ for why a capture needs it."""
    import gc
    plain = {k: p.detach() for k, p in net.named_parameters()}
    for u in functional_nets:
        put_theta(u, plain)
    for m in (net,) + tuple(functional_nets):
        mem = getattr(m, 'memory', None)
        if mem is not None:
            mem._m_items = mem._m_items.detach()
            mem.last_read = None
    ops._proxy.clear()
    gc.collect()


class GraphedMldgStep:
    """One train_memory_mldg iteration (train.py:493-632: inner forward + backward with retain_graph, the two functional weight sets theta' = theta - inner_lr g,
    frozen-encoder memory write, meta-test forward + backward through the written memory, SGD, eval-mode memory-commit forward) captured in ONE hipGraph and
    replayed. The regime every pinmem script runs (train_GS_pinmem_DR50V3P.sh:9-10,18) enqueues ~2 400 launches per step: on the bf16 tier 33-35 ms of host time
    against 30 ms of GPU time -- host-bound as eager launches. What makes it replayable on top of GraphedAggStep's list: the inner learning rate is a device
    scalar (`--inner_lr_anneal` changes it every iteration: train.py:625-626), the functional networks are rewired once at capture (their theta' tensors live in
    the graph's memory pool and are recomputed by every replay), the committed memory lives in one static buffer that the captured step reads first and writes last.
    Bit-identical to eager mldg_train_step calls (tests/test_model_parity.py::test_graphed_mldg_step_is_bit_identical_to_eager). Single process only.

        g = GraphedMldgStep(net, u1, u2, opt, x_tr, y_tr, x_te, y_te, sched=sched, inner_lr_anneal=True)      # warms up eagerly, then captures
        out = g.step(x_tr, y_tr, x_te, y_te)      # tensors of the returned dict are overwritten by the next replay; out['next_inner_lr'] as mldg_train_step
        g.close()
    """

    def __init__(self, net, updated_net, updated_net2, opt, x_tr, y_tr, x_te, y_te, inner_lr=INNER_LR, sched=None, warmup=2, inner_lr_anneal=False):
        assert x_tr.is_cuda and not D.is_dist(), 'GraphedMldgStep: single-process GPU training only'
        assert len(opt.param_groups) == 1, 'GraphedMldgStep: one parameter group (optimizer.py:21-25)'
        self.net, self.u1, self.u2, self.opt, self.sched, self.anneal, self.closed = net, updated_net, updated_net2, opt, sched, inner_lr_anneal, False
        self.x_tr, self.y_tr, self.x_te, self.y_te = x_tr.clone(), y_tr.clone(), x_te.clone(), y_te.clone()
        dev = x_tr.device
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.inner = torch.zeros((), dtype=torch.float32, device=dev)      # 0-dim: torch._foreach_mul's tensor-scalar overload
        self.inner_lr = float(inner_lr)
        # Warm-up and capture run on ONE side stream, after every reference into an earlier autograd graph has been dropped. An autograd AccumulateGrad node remembers the
        # stream it was created on and lives as long as any graph refers to it; the functional networks keep theta' -- hence the graph of the inner step, hence every
        # parameter's node -- alive BETWEEN iterations. A node born in eager code on the default stream would be reused inside the capture and enqueue its accumulation on
        # that (non-capturing) stream: hipStreamEndCapture crashes (tools/mldg_graph_probe.py: the bisection). GraphedAggStep never meets this: its graphs die with each step.
        self.stream = torch.cuda.Stream(device=dev)
        ok = False
        try:
            opt.lr_device = self.lr
            finish_commit(net)
            release_functional_state(net, updated_net, updated_net2)
            torch.cuda.synchronize()
            with torch.cuda.stream(self.stream):
                for _ in range(max(1, warmup)):      # allocates workspaces, momentum buffers, filter caches, sets every kernel's LDS attribute; >= 1: the nodes are reborn on this stream
                    self._eager()
                self.mem = net.memory.m_items.detach().clone()
                net.memory.m_items = self.mem
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            self._fill()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.out = mldg_train_step(net, updated_net, updated_net2, opt, self.x_tr, self.y_tr, self.x_te, self.y_te, inner_lr=self.inner, sched=None)
                self.mem.copy_(net.memory.m_items)
                if ops.overlap_wgrad():      # every stream forked into the capture rejoins it
                    torch.cuda.current_stream().wait_stream(ops._side_stream())
            torch.cuda.synchronize()
            net.memory.pending = None
            net.memory.m_items = self.mem
            ops.commit_done.pop(dev.index, None)
            ops.last_prefold_event = None
            K.forget_filter_events()
            ok = True      # (a capture records, it does not execute: the model is where the warm-up left it)
        finally:
            if not ok:      # a failed warm-up / capture must not leave the optimizer reading a dead device scalar
                opt.lr_device = None
                if getattr(self, 'mem', None) is not None:
                    net.memory.m_items = self.mem.clone()
                net.memory.pending = None

    def _fill(self):
        self.lr.fill_(float(self.opt.param_groups[0]['lr']))
        self.inner.fill_(self.inner_lr)

    def _after(self):
        if self.sched is not None:
            self.sched.step()
        if self.anneal:
            self.inner_lr = annealed_inner_lr(self.opt)

    def _eager(self):
        self._fill()
        mldg_train_step(self.net, self.u1, self.u2, self.opt, self.x_tr, self.y_tr, self.x_te, self.y_te, inner_lr=self.inner, sched=None)
        self._after()

    def step(self, x_tr=None, y_tr=None, x_te=None, y_te=None):
        assert not self.closed, 'GraphedMldgStep.step() after close()'
        for dst, src in ((self.x_tr, x_tr), (self.y_tr, y_tr), (self.x_te, x_te), (self.y_te, y_te)):
            if src is not None and src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        self._fill()
        self.graph.replay()
        self._after()
        out = dict(self.out)
        if self.anneal:
            out['next_inner_lr'] = self.inner_lr
        return out

    def close(self):
        """Hand model and optimizer back to eager code (the memory becomes a private tensor again, the optimizer forgets the capture's device-side learning rate)."""
        if self.closed:
            return
        torch.cuda.synchronize()
        self.net.memory.m_items = self.mem.clone()
        self.net.memory.pending = None
        ops.commit_done.pop(self.x_tr.device.index, None)
        if getattr(self.opt, 'lr_device', None) is self.lr:
            self.opt.lr_device = None
        release_functional_state(self.net, self.u1, self.u2)      # eager code gets fresh autograd nodes on ITS stream (the captured ones were born on the capture stream)
        self.closed = True
        torch.cuda.synchronize()


# ---- pooled multi-scale / flip evaluation: inference_pool + MeanFusion (eval.py:133-145,277-337) -------------------------
def inference_pool(net, imgs, orisize, no_flip=False):
    """imgs[flip][scale]: pre-scaled (and pre-flipped for flip = 1) NCHW image batches as the reference's loader provides them.
    Per entry: logits -> half-pixel bilinear to `orisize` (un-flipping flipped inputs) -> softmax -> float64 running mean;
    returns (probs, preds) = max over classes of the fused buffer. All of it stays on the GPU (the reference moves every
    map to the CPU, eval.py:328-330)."""
    net.eval()
    n = imgs[0][0].shape[0]
    buf, cnt = None, 0
    with torch.no_grad():
        for flip in range(1 if no_flip else 2):
            for img in imgs[flip]:
                lg = ops.nhwc(net(img)[0])
                up = K.resize_hp_fwd(lg, orisize, flip_w=(flip == 1))
                if buf is None:
                    buf = torch.zeros((n, orisize[0], orisize[1], up.shape[3]), dtype=torch.float64, device=up.device)
                cnt += 1
                K.softmax_mean_update(up, buf, cnt)
    return K.argmax_f64(buf)


# ---- input edge -----------------------------------------------------------------------------------
def prepare_batch(inputs, gts, aux_gts=None):
    """train.py:297-307: DomainUniformConcatDataset batches arrive as [B, D, 3, H, W] / [B, D, H, W]; merge the domain axis."""
    c, h, w = inputs.shape[-3:]
    x = inputs.reshape(-1, c, h, w).cuda(non_blocking=True)
    gt = gts.reshape(-1, h, w).cuda(non_blocking=True)
    aux = gt if aux_gts is None else aux_gts.reshape(-1, h, w).cuda(non_blocking=True)
    return x, gt, aux


def prepare_batch_u8(images_u8, labels_u8, augment=None, hard=None, geometry=None, sizes=None, centroids=None, decode=None, tables=None):
    """GPU-side ToTensor + Normalize(ImageNet) + MaskToTensor for uint8 [.., H, W, 3] images and uint8 [.., H, W] label maps:
    4x / 8x less host->device traffic than the fp32 / int64 tensors the reference's loader ships. Returns the image as a
    logical-NCHW view of NHWC4 memory (what the stem consumes without another conversion) and int64 labels.
    augment (an input_edge.PhotometricAugment; None = the plain conversion): colour jitter, blur and flip on the device first (image and labels flipped alike);
    hard: one bool per image after the leading axes merged -- those get the hard augmentation of the meta-test domains.
    geometry (an input_edge.GeometricAugment; None = none): RandomSizeAndCrop on the device before all of that -- resize, pad and crop of image and labels; sizes
    ((H, W) per image, the image in the top-left corner of its slab; None: every image fills it) and centroids go to its sampler.
    decode (an input_edge.LabelDecode; None = the masks hold train ids) with tables (one entry per image after the leading axes merged: a table index of `decode`,
    -1 or None for the pass-through): labels_u8 is raw, [.., H, W] ids or [.., H, W, 3] colours, and is decoded on the device first -- inside the geometry's mask
    gather where there is one, else in a pass of its own."""
    h, w = images_u8.shape[-3:-1]
    img_d = images_u8.reshape(-1, h, w, 3).cuda(non_blocking=True).contiguous()
    if decode is None:
        assert tables is None, 'tables without a LabelDecode'
        lab_d = labels_u8.reshape(-1, h, w).cuda(non_blocking=True).contiguous()
    else:
        lab_tail = (h, w, 3) if labels_u8.dim() == images_u8.dim() else (h, w)
        table = decode.image_table([None] * img_d.shape[0] if tables is None else tables, img_d.shape[0], 3 if len(lab_tail) == 3 else 1)
        lab_d = labels_u8.reshape(-1, *lab_tail).cuda(non_blocking=True).contiguous()
        if geometry is None:
            lab_d = K.labels_decode_u8(lab_d, decode.device_tables(lab_d.device), table)
    if geometry is not None:
        from .input_edge import sample_geometry
        geo = sample_geometry(geometry, img_d.shape, dict(sizes=sizes, centroids=centroids))
        if decode is None:
            img_d, lab_d = K.resample_crop_u8(img_d, lab_d, geo)
        else:
            img_d, lab_d = K.resample_crop_decode_u8(img_d, lab_d, geo, decode.device_tables(lab_d.device), table)
    if augment is None:
        return ops.nchw(K.image_u8_to_nhwc4(img_d)), K.labels_u8_to_i64(lab_d)
    params = K.upload_aug_params(augment.sample(img_d.shape[0], hard), img_d.device)
    return ops.nchw(K.augment_u8(img_d, params)), K.labels_u8_to_i64(lab_d, params)
