"""Records what the convolution size queries answer into tests/golden/conv_size_queries.json (tests/test_abi.py holds every later build to it).

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_conv_sizes.py        # re-record the rows; signatures are read from the fixture itself
    python tools/record_conv_sizes.py --collect keys.json                                     # GPU: the call signatures of the networks, as keys of kernels._SIZES
    PM_LIB=... python tools/record_conv_sizes.py --import-keys keys.json                      # replace the fixture's network signatures by those keys, then record

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test: the queries are pure host code
and answer for fake, aligned, non-null tensor pointers, so recording needs no GPU.

A signature is one convolution layer: x and y as (n, h, w, c, pitch, dtype, flags), then kh, stride, pad, dil, prec. A row is [signature, routing name, the seven
integers pm_conv_workspace(x, y, p, 0 | 1 | 2), pm_conv_winograd_v_bytes(x, y, p), pm_conv_wxf_bytes(x, y, p), pm_conv_wxf_bytes_dgrad(y, x, p),
pm_conv_bn_partials_bytes(x, y, p)]."""
import argparse
import ctypes
import json
import os
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_size_queries.json')
F32, BF16, ZERO_PAD64 = 0, 1, 1
X_PTR, Y_PTR = 0x10000, 0x4000000      # fake device pointers, 256-byte aligned: the queries never dereference them

DEFAULT = {'winograd': 4, 'winograd_fused': 0, 'conv16': 1, 'conv16_wide': 1, 'conv16_persistent': 1, 'wgrad16': 1, 'bf16_wgrad': 0, 'split': 1}      # include/pinmem_hip.h pm_routing
# single-field departures from it, and the tier of the rows each can affect
ROUTINGS = [('default', {}, 'both'), ('split=0', {'split': 0}, 'f32'), ('winograd=0', {'winograd': 0}, 'f32'), ('winograd=2', {'winograd': 2}, 'f32'),
            ('winograd_fused=1', {'winograd_fused': 1}, 'f32'), ('conv16=0', {'conv16': 0}, 'bf16'), ('conv16=2', {'conv16': 2}, 'bf16'),
            ('conv16_wide=0', {'conv16_wide': 0}, 'bf16'), ('conv16_wide=2', {'conv16_wide': 2}, 'bf16'), ('conv16_wide=3', {'conv16_wide': 3}, 'bf16'),
            ('conv16_persistent=0', {'conv16_persistent': 0}, 'bf16'), ('wgrad16=0', {'wgrad16': 0}, 'bf16'), ('bf16_wgrad=1', {'bf16_wgrad': 1}, 'bf16')]


def sig(n, h, w, cin, cout, k, stride=1, pad=None, dil=1, prec=0, xdt=F32, ydt=F32, xpitch=None, ypitch=None, xflags=0):
    pad = dil * (k - 1) // 2 if pad is None else pad
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return [n, h, w, cin, xpitch or cin, xdt, xflags, n, ho, wo, cout, ypitch or cout, ydt, 0, k, stride, pad, dil, prec]


def edge_signatures():
    """Hand-written edges, each as small as it stays on its route."""
    b = dict(xdt=BF16, ydt=BF16, prec=2)
    s = [sig(2, 97, 131, 128, 128, 3), sig(2, 97, 131, 64, 64, 3, **b), sig(2, 97, 131, 64, 64, 1),                         # a ragged map
         sig(1, 32, 32, 4, 64, 7, stride=2, pad=3, prec=2, ydt=BF16), sig(1, 32, 32, 4, 64, 7, stride=2, pad=3),          # the 4-channel stem
         sig(1, 16, 16, 256, 19, 1, prec=2, xdt=BF16, ypitch=20), sig(1, 16, 16, 256, 19, 1, ypitch=20),                   # the class head
         sig(1, 16, 16, 48, 64, 3, **b), sig(1, 16, 16, 48, 64, 1, **b),                                                    # 48 channels bf16: padded copy
         sig(1, 16, 16, 304, 256, 3, xpitch=320, **b), sig(1, 16, 16, 304, 256, 3, xpitch=320, xflags=ZERO_PAD64, **b)]    # 304 channels at pitch 320
    for k in (3, 1):                                                                                                       # stride 2
        s += [sig(1, 9, 9, 8, 8, k, stride=2), sig(1, 10, 10, 64, 64, k, stride=2), sig(1, 10, 10, 64, 64, k, stride=2, **b),
              sig(1, 10, 10, 64, 32, k, stride=2, **b)]
    s += [sig(1, 16, 16, 256, 255 - 3, 3), sig(1, 16, 16, 256, 256, 3), sig(1, 16, 16, 128, 128, 3), sig(1, 16, 16, 128, 128, 3, dil=2),      # Winograd weight gradient from 256 x 256
          sig(1, 15, 17, 64, 64, 3, **b), sig(1, 16, 16, 64, 64, 3, **b), sig(1, 8, 8, 64, 64, 3, **b),                    # M = 255 / 256 / 64: the LDS-DMA threshold
          sig(1, 4, 4, 2048, 256, 3), sig(1, 4, 4, 2048, 256, 3, **b), sig(1, 16, 16, 128, 64, 3, **b), sig(1, 16, 16, 128, 128, 3, **b),
          sig(1, 16, 16, 64, 64, 3, prec=2), sig(1, 16, 16, 64, 64, 3, prec=1)]                                              # long K, small M: split-K; the older tiers
    return s


def tier(s):
    return 'bf16' if (s[5] == BF16 or s[12] == BF16 or s[18] != 0) else 'f32'


def signatures_from_keys(keys):
    """keys of pinthememory_amd.hip.kernels._SIZES (conv_fwd / conv_bwd_data / conv_bwd_weight entries) -> sorted distinct signatures."""
    dt = {'torch.float32': F32, 'torch.bfloat16': BF16}

    def desc(shape, stride, dtype, flags=0):
        n, h, w, c = shape
        sn, sh, sw, _ = stride
        return [n, h, w, c, sw if w > 1 else (sh if h > 1 else (sn if n > 1 else c)), dt[dtype], flags]      # hip/lib.py tdesc

    out = set()
    for k in keys:
        if k[0] == 'f':
            _, xs, xst, xdt, xfl, ws, yst, ydt, stride, pad, dil, prec, _ = k
            ho, wo = [(v + 2 * pad - dil * (ws[1] - 1) - 1) // stride + 1 for v in xs[1:3]]
            x, y = desc(xs, xst, xdt, xfl), desc([xs[0], ho, wo, ws[0]], yst, ydt)
        elif k[0] == 'd':
            _, ys, yst, ydt, yfl, ws, xs, xst, xdt, stride, pad, dil, prec, _ = k
            x, y = desc(xs, xst, xdt), desc(ys, yst, ydt, yfl)
        elif k[0] == 'w':
            _, xs, xst, xdt, ys, yst, ydt, ws, stride, pad, dil, prec, _, _ = k
            x, y = desc(xs, xst, xdt), desc(ys, yst, ydt)
        else:
            continue
        out.add(tuple(x + y + [ws[1], stride, pad, dil, prec]))
    return [list(s) for s in sorted(out)]


def collect(path):
    """GPU: one DeepV3Plus-R50 training step at 2 x 128^2 and 8 x 768^2 on both tiers and one DeepV2 eval tile; writes the keys of kernels._SIZES."""
    import torch
    from pinthememory_amd import harness, synth
    from pinthememory_amd.hip import kernels as K
    from pinthememory_amd.network import deepv2, deepv3plus
    crit = torch.nn.CrossEntropyLoss(reduction='mean', ignore_index=255)
    keys = set()
    for dtype in ('f32', 'bf16'):
        K.set_conv_precision(dtype)
        for batch, size in ((2, 128), (8, 768)):
            net = synth.load_det_weights(deepv3plus.DeepR50V3PlusD(synth.model_args(gumbel_off=False), 19, crit, crit)).cuda()
            opt, sched = harness.make_optimizer(net)
            x, y = synth.make_batch(batch, size)
            harness.agg_train_step(net, opt, x.cuda(), y.cuda(), sched=sched)
            harness.finish_commit(net)
            torch.cuda.synchronize()
            keys |= set(K._SIZES)
            del net, opt
    K.set_conv_precision('f32')
    net = synth.load_det_weights(deepv2.DeepR101V2D(synth.model_args(), 19, crit, crit)).cuda()
    harness.sliding_logits(net, torch.randn(3, 1024, 1024).cuda(), 1024, flips=(False,))
    torch.cuda.synchronize()
    keys |= set(K._SIZES)
    plain = lambda v: [plain(e) for e in v] if isinstance(v, (tuple, list)) else (v if isinstance(v, (int, bool, str)) else str(v))
    with open(path, 'w') as f:
        json.dump(sorted((plain(k) for k in keys if k[0] in 'fdw'), key=repr), f)
    print('wrote %d keys to %s' % (len(keys), path))


def query(lib, L, s):
    x, y = L.PmTensor(X_PTR, *s[0:7]), L.PmTensor(Y_PTR, *s[7:14])
    p = L.conv_params(s[14], s[14], s[15], s[16], s[17], s[18])
    return [lib.pm_conv_workspace(byref(x), byref(y), byref(p), 0), lib.pm_conv_workspace(byref(x), byref(y), byref(p), 1),
            lib.pm_conv_workspace(byref(x), byref(y), byref(p), 2), lib.pm_conv_winograd_v_bytes(byref(x), byref(y), byref(p)),
            lib.pm_conv_wxf_bytes(byref(x), byref(y), byref(p)), lib.pm_conv_wxf_bytes_dgrad(byref(y), byref(x), byref(p)),
            lib.pm_conv_bn_partials_bytes(byref(x), byref(y), byref(p))]


class routing:
    """with routing(lib, L, {'split': 0}): the default routing (not whatever PM_* variables the library was loaded under) with those fields replaced; the previous routing comes back on exit."""

    def __init__(self, lib, L, fields):
        self.lib, self.L, self.fields = lib, L, fields

    def __enter__(self):
        self.before = self.L.PmRouting(ctypes.sizeof(self.L.PmRouting))
        assert self.lib.pm_routing_get(byref(self.before)) == 0
        r = self.L.PmRouting(ctypes.sizeof(self.L.PmRouting), **dict(DEFAULT, **self.fields))
        assert self.lib.pm_routing_set(byref(r)) == 0, self.fields

    def __exit__(self, *exc):
        assert self.lib.pm_routing_set(byref(self.before)) == 0


def rows(lib, L, signatures):
    out = []
    for name, fields, which in ROUTINGS:
        with routing(lib, L, fields):
            out += [[s, name, query(lib, L, s)] for s in signatures if which in ('both', tier(s))]
    return out


def dumps(network, edge, table):
    line = lambda v: json.dumps(v, separators=(',', ':'))
    block = lambda vs: '[\n' + ',\n'.join(line(v) for v in vs) + '\n]'
    return ('{"signature": "x: n h w c pitch dtype flags, y: the same, kh stride pad dil prec",\n"values": "workspace fwd dgrad wgrad, winograd_v, wxf, wxf_dgrad, bn_partials",\n'
            '"routings": %s,\n"network_signatures": %s,\n"edge_signatures": %s,\n"rows": %s}\n' % (line({n: f for n, f, _ in ROUTINGS}), block(network), block(edge), block(table)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--collect', metavar='KEYS.json')
    ap.add_argument('--import-keys', metavar='KEYS.json')
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args()
    if a.collect:
        return collect(a.collect)
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    if a.import_keys:
        with open(a.import_keys) as f:
            network = signatures_from_keys(json.load(f))
    else:
        with open(FIXTURE) as f:
            network = json.load(f)['network_signatures']
    edge = edge_signatures()
    table = rows(lib, L, network + [s for s in edge if s not in network])
    with open(a.out, 'w') as f:
        f.write(dumps(network, edge, table))
    print('%d signatures, %d rows -> %s' % (len(network) + len(edge), len(table), a.out))


if __name__ == '__main__':
    main()
