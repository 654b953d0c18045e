"""Golden vectors of the IBN trunks (wt_layer values 3 / 4: nn.InstanceNorm2d in the stem and behind the last block of a stage), captured FROM THE IMPORTED
REFERENCE on CPU (oracle.import_reference: its classes are imported where they lie, nothing of them is copied) with the RNG-free weights and inputs of
pinthememory_amd/synth.py and the packers of oracle/make_golden.py. Needs the reference tree.

    python tools/make_ibn_golden.py

tests/golden/state_dict_v3plus_r50_ibn.json   [name, shape, dtype] of DeepR50V3PlusD(wt_layer=WT, memory=True).state_dict(), in order
tests/golden/ibn_v3plus_128.npz               wt_layer=WT, 2 x 3 x 128 x 128, det_state_dict weights, dropout p = 0, gumbel off:
    argmax / sub / margin / sha256            eval logits of the memory=True net (logits_pack);  plain_*: the same of the memory=False net
    plain_loss1 / plain_loss2 / plain_total   the memory-less training forward (train.py:213-244: total = loss1 + 0.4 loss2)
    plain_grad_sums / plain_grad_sample       fingerprint of its parameter gradients (named_parameters order, plain_grad_names)
    loss1 / loss2 / readloss / div / cls / total, grad_sums / grad_sample / grad_names: one agg train step of the memory=True net"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import import_reference as IR                     # noqa: E402
from oracle.make_golden import fingerprint, logits_pack       # noqa: E402
from oracle.ref_cpu import harness                            # noqa: E402
from pinthememory_amd import synth                            # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
WT = [0, 0, 4, 4, 4, 0, 0]
SIZE, BATCH = 128, 2


def reference_net(memory, wt=WT):
    rv3, _, _ = IR.load()
    crit = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    net = synth.load_det_weights(rv3.DeepR50V3PlusD(synth.model_args(wt_layer=list(wt), memory=memory), 19, crit, crit))
    net.dsn[3].p = 0.0
    return net


def eval_logits(net, x):
    net.eval()
    with torch.no_grad():
        return net(x)[0]


def plain_forward_backward(net, x, y):
    """-> (loss1, loss2, total) of the memory-less training forward; gradients are left on the parameters"""
    net.train()
    net.zero_grad()
    out = net(x, gts=y, aux_gts=y)
    total = out[0] + harness.LOSS_W['aux'] * out[1]
    total.backward()
    return out[0].detach(), out[1].detach(), total.detach()


def main():
    torch.set_num_threads(8)
    g = {}
    x, y = synth.make_batch(BATCH, SIZE)
    net = reference_net(True)
    keys = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in net.state_dict().items()]
    json.dump(keys, open(os.path.join(OUT, 'state_dict_v3plus_r50_ibn.json'), 'w'))
    g.update(logits_pack(eval_logits(net, x)))
    opt, _ = harness.make_optimizer(net)
    losses = harness.agg_train_step(net, opt, x, y)
    for k, v in losses.items():
        g[k] = v.numpy()
    named = [(k, p) for k, p in net.named_parameters() if p.grad is not None]
    g['grad_names'] = np.array([k for k, _ in named])
    g['grad_sums'], g['grad_sample'] = fingerprint([p.grad for _, p in named])

    net = reference_net(False)
    g.update({'plain_' + k: v for k, v in logits_pack(eval_logits(net, x)).items()})
    l1, l2, tot = plain_forward_backward(net, x, y)
    g['plain_loss1'], g['plain_loss2'], g['plain_total'] = l1.numpy(), l2.numpy(), tot.numpy()
    named = [(k, p) for k, p in net.named_parameters() if p.grad is not None]
    g['plain_grad_names'] = np.array([k for k, _ in named])
    g['plain_grad_sums'], g['plain_grad_sample'] = fingerprint([p.grad for _, p in named])
    g['wt_layer'] = np.array(WT)
    np.savez_compressed(os.path.join(OUT, 'ibn_v3plus_128.npz'), **g)
    print('%d state_dict entries; fixtures written to %s' % (len(keys), OUT))


if __name__ == '__main__':
    main()
