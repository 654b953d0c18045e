"""Records the output bits of every loss entry point (csrc/loss.hip) into tests/golden/loss_bits.json; tests/test_loss_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_loss_bits.py

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. The size queries are pure host
code and are recorded on any machine; the digests need the GPU and are kept as they are when there is none. Every output is fixed-order and deterministic, so a
digest (sha256 of the output's bytes) either matches or the change altered a bit.

A case is (name, n, (h, w), (H, W), inv_temp, C). Inputs come from CPU generators with fixed seeds; the logits sit in a pitch-padded buffer as in
tests/test_hip_kernels.py::test_upsample_ce. Labels: about 1 % are no class (in [C, 254]), 10 % are 255 and the first two rows are all 255."""
import hashlib
import json
import os
import subprocess
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'loss_bits.json')
MAX_REFUSED = 2      # cases a call family may refuse (upsample_ce_fused_ok / upsample_eval_ok / upsample_relax_ok), of all of CASES
GSCALE = 1.7

CASES = [
    ('flat-forward', 2, (5, 7), (33, 29), 0.5, 19),                # W < 32: the flat forward; interval field
    ('row-staged', 2, (12, 12), (48, 48), 1.0, 19),
    ('parts', 2, (6, 6), (96, 96), 2.0, 19),                       # 16-fold: PARTS > 1
    ('generic-classes', 2, (7, 5), (30, 41), 1.0, 8),              # the select-not-branch form of the weighted generic kernel
    ('two-rounds', 2, (3, 300), (7, 611), 1.0, 19),                # rows wider than one round: the carry
    ('interval-wave-edges', 2, (33, 65), (65, 129), 1.0, 19),
    ('three-segments', 2, (20, 256), (41, 520), 1.0, 19),          # column segments with a left-neighbour lane
    ('identity', 2, (16, 16), (16, 16), 1.0, 19),
    ('wide-labels', 1, (4, 230), (9, 900), 1.0, 19),               # W > 768: past the three label registers
    ('down-sampling', 2, (9, 9), (4, 6), 1.0, 19),
    ('single-tap', 2, (1, 1), (8, 8), 1.0, 19),
    ('eval-row-walk', 2, (64, 8), (512, 20), 1.0, 19),             # the validation kernel walks several rows and swaps its LDS slots
    ('wide-generic', 2, (4, 4), (4, 700), 1.0, 5),
]
SIZE_ONLY = [('main-loss', 8, (192, 192), (768, 768), 1.0, 19), ('eval-image', 1, (256, 512), (1024, 2048), 1.0, 19)]
SIZE_NAMES = ['pm_upsample_ce_workspace', 'pm_upsample_ce_field_bytes', 'pm_upsample_ce_bwd_workspace', 'pm_upsample_wce_workspace', 'pm_upsample_wce_loss_floats',
              'pm_upsample_eval_workspace', 'pm_label_class_weights_workspace']
RELAX_SIZE_NAMES = ['pm_upsample_relax_workspace', 'pm_upsample_relax_loss_floats', 'pm_upsample_relax_field_bytes', 'pm_relax_class_weights_workspace']
STRICT_MASK = 0b101      # classes 0 and 2 keep their one-hot in the border-2 sets


def sizes(lib, L, case):
    """The seven size queries for a case's shape (fake, aligned, non-null logits pointer: the queries never dereference it)."""
    _, n, (h, w), (H, W), _, C = case
    t = L.PmTensor(0x10000, n, h, w, C, (C + 3) // 4 * 4, L.PM_F32, 0)
    return [lib.pm_upsample_ce_workspace(n, H, W), lib.pm_upsample_ce_field_bytes(byref(t), H, W), lib.pm_upsample_ce_bwd_workspace(byref(t), H, W),
            lib.pm_upsample_wce_workspace(n, H, W), lib.pm_upsample_wce_loss_floats(n), lib.pm_upsample_eval_workspace(byref(t), H, W),
            lib.pm_label_class_weights_workspace(n)]


def relax_sizes(lib, case):
    """The four size queries of the relaxed-border family (RELAX_SIZE_NAMES) for a case's shape."""
    _, n, (h, w), (H, W), _, C = case
    return [lib.pm_upsample_relax_workspace(n, H, W), lib.pm_upsample_relax_loss_floats(n), lib.pm_upsample_relax_field_bytes(n, h, w, C, H, W),
            lib.pm_relax_class_weights_workspace(n)]


def inputs(K, case):
    """-> (logits [n, h, w, C] on the device, pitch-padded; int64 labels [n, H, W] on the device; [C] class weights on the device)."""
    import torch
    _, n, (h, w), (H, W), _, C = case
    g = torch.Generator().manual_seed(1)
    lg = torch.randn(n, h, w, C, generator=g) * 3
    g = torch.Generator().manual_seed(2)
    lab = torch.randint(0, C, (n, H, W), generator=g)
    other = torch.randint(C, 255, (n, H, W), generator=g)
    u = torch.rand(n, H, W, generator=g)
    lab = torch.where(u < 0.01, other, lab)
    lab[(u >= 0.01) & (u < 0.11)] = 255
    lab[:, :2] = 255
    vec = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3))
    dev = torch.zeros(1, device='cuda')
    lgg = K.new((n, h, w, C), dev, pitch_pad=True)
    lgg.copy_(lg)
    return lgg, lab.cuda(), vec.cuda()


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(K, case):
    """Every call of every family on the case's inputs -> {call: {output: sha256} or 'refused'}."""
    import torch
    _, n, _, HW, inv_temp, C = case
    lg, lab, vec = inputs(K, case)
    gs = torch.tensor([GSCALE], device='cuda')
    fused, out = K.upsample_ce_fused_ok(lg, HW), {}
    rows = {(norm, per_batch): K.label_class_weights(lab, C, norm=norm, per_batch=per_batch) for norm in (False, True) for per_batch in (False, True)}
    out['label_class_weights'] = {'norm=%d,per_batch=%d' % k: digest(v) for k, v in rows.items()}

    loss = K.upsample_ce_fwd(lg, lab, inv_temp)
    out['ce_fwd'] = {'loss_out': digest(loss)}
    if fused:
        lf, field = K.upsample_ce_fwd_field(lg, lab, inv_temp)
        out['ce_fwd_field'] = {'loss_out': digest(lf), 'field': digest(field)}
        out['ce_bwd_field'] = {'dlogits': digest(K.upsample_ce_bwd_field(lg, HW, lf, field, gs, inv_temp))}
        out['ce_bwd'] = {'dlogits': digest(K.upsample_ce_bwd(lg, lab, loss, None, inv_temp))}
    else:
        out['ce_fwd_field'] = out['ce_bwd_field'] = out['ce_bwd'] = 'refused'

    for tag, wts, per_image in (('vector', vec, False), ('rows', rows[(False, False)], False), ('rows,per_image', rows[(False, False)], True)):
        out['wce_fwd[%s]' % tag] = {'loss_out': digest(K.upsample_wce_fwd(lg, lab, wts, per_image, inv_temp))}
        if fused:
            lf, field = K.upsample_wce_fwd_field(lg, lab, wts, per_image, inv_temp)
            out['wce_fwd_field[%s]' % tag] = {'loss_out': digest(lf), 'field': digest(field)}
            out['wce_bwd_field[%s]' % tag] = {'dlogits': digest(K.upsample_wce_bwd_field(lg, HW, lf, field, gs, per_image, inv_temp))}
        else:
            out['wce_fwd_field[%s]' % tag] = out['wce_bwd_field[%s]' % tag] = 'refused'

    if K.upsample_eval_ok(lg, HW):
        _, hist, _ = K.upsample_eval(lg, lab, inv_temp, want_pred=True)
        le, hist, pred = K.upsample_eval(lg, lab, inv_temp, hist=hist, want_pred=True)      # twice into one histogram
        out['eval'] = {'loss_out': digest(le), 'hist': digest(hist), 'pred': digest(pred)}
    else:
        out['eval'] = 'refused'
    torch.cuda.synchronize()
    return out


def run_relax_case(K, case):
    """Every call of the relaxed-border families on the case's inputs -> {call: {output: sha256} or 'refused'}. The sets come from the case's own labels."""
    import torch
    _, n, _, HW, inv_temp, C = case
    lg, lab, vec = inputs(K, case)
    gs = torch.tensor([GSCALE], device='cuda')
    out = {}
    sets = {'border=0': K.relax_border_bits(lab, C, 0), 'border=1': K.relax_border_bits(lab, C, 1), 'border=2,strict': K.relax_border_bits(lab, C, 2, STRICT_MASK)}
    out['relax_border_bits'] = {k: digest(v) for k, v in sets.items()}
    bits = sets['border=1']
    planes = ((bits.unsqueeze(1) >> torch.arange(C + 1, device='cuda').view(1, -1, 1, 1)) & 1).to(torch.uint8)
    out['multihot_to_bits'] = {'bits': digest(K.multihot_to_bits(planes))}
    rrows = {(norm, per_batch): K.relax_class_weights(bits, C, norm=norm, per_batch=per_batch) for norm in (False, True) for per_batch in (False, True)}
    out['relax_class_weights'] = {'norm=%d,per_batch=%d' % k: digest(v) for k, v in rrows.items()}
    relax = K.upsample_relax_ok(lg, HW)
    for tag, wts in (('vector', vec), ('rows', rrows[(False, False)])):
        out['relax_fwd[%s]' % tag] = {'loss_out': digest(K.upsample_relax_fwd(lg, bits, wts, inv_temp))}
        if relax:
            lf, field = K.upsample_relax_fwd_field(lg, bits, wts, inv_temp)
            out['relax_fwd_field[%s]' % tag] = {'loss_out': digest(lf), 'field': digest(field)}
            out['relax_bwd_field[%s]' % tag] = {'dlogits': digest(K.upsample_relax_bwd_field(lg, HW, lf, field, gs, inv_temp))}
        else:
            out['relax_fwd_field[%s]' % tag] = out['relax_bwd_field[%s]' % tag] = 'refused'
    torch.cuda.synchronize()
    return out


def merge(old, new, what):
    """Recording only ever adds: a value the fixture already holds has to come out of the parent build again."""
    if not isinstance(old, dict) or not isinstance(new, dict):
        assert old == new, 'the parent build no longer reproduces its own record: %s was %r, is %r' % (what, old, new)
        return old
    return {k: merge(old[k], new[k], '%s/%s' % (what, k)) if k in old else new[k] for k in list(old) + [k for k in new if k not in old]}


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    fixture = {'digests': {}}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            fixture = json.load(f)
    fixture['size_queries'], fixture['relax_size_queries'] = SIZE_NAMES, RELAX_SIZE_NAMES
    fixture['sizes'] = merge(fixture.get('sizes', {}), {c[0]: sizes(lib, L, c) for c in CASES + SIZE_ONLY}, 'sizes')
    fixture['relax_sizes'] = merge(fixture.get('relax_sizes', {}), {c[0]: relax_sizes(lib, c) for c in CASES + SIZE_ONLY}, 'relax_sizes')
    if torch.cuda.is_available():
        from pinthememory_amd.hip import kernels as K
        version = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--version'], capture_output=True, text=True).stdout
        fixture['hipcc'] = next((l.strip() for l in version.splitlines() if 'version' in l.lower()), '')      # for information only
        fixture['digests'] = merge(fixture['digests'], {c[0]: run_case(K, c) for c in CASES}, 'digests')
        fixture['relax_digests'] = merge(fixture.get('relax_digests', {}), {c[0]: run_relax_case(K, c) for c in CASES}, 'relax_digests')
        for group in ('digests', 'relax_digests'):
            for k in sorted({k for d in fixture[group].values() for k in d}):
                refused = [name for name, d in fixture[group].items() if d[k] == 'refused']
                assert len(refused) <= MAX_REFUSED, 'replace a case: %s is refused for %s' % (k, refused)
    else:
        print('no GPU: size queries recorded, digests kept as they were')
    with open(FIXTURE, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d cases, %d shapes of size queries -> %s' % (len(fixture['digests']), len(fixture['sizes']), FIXTURE))


if __name__ == '__main__':
    main()
