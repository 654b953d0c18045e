"""Records the output bits of the memory entry points (csrc/memory.hip: K.mem_read_fwd, K.mem_read_fwd_pq, K.mem_colsoftmax, K.mem_read_bwd, K.mem_write_accum,
K.mem_write_accum_bwd, K.mem_write_update, K.mem_write_update_bwd) and the answers of their four workspace queries into tests/golden/memory_bits.json;
tests/test_memory_bits.py holds every later build to them.

    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/record_memory_bits.py

Record against a library built from the PARENT of the change under test (tools/build_base_lib.sh), never from the code under test. The workspace answers are pure
host code and are recorded on any machine; the digests need the GPU and are kept as they are when there is none. Every output is fixed-order and deterministic, so a
digest (sha256 of the output's bytes) either matches or the change altered a bit.

The cases are the smallest that reach every arm of the kernels (the two large ones are sizes the suite already runs):
  slots         126 rows (three full 32-row tiles and a ragged one of 30) at every slot count that changes a register quad or the instantiation, noise off and on
  views         the same at m = 19 and 20 with x and dqr as channel slices of wider slabs
  tile-loop     98 344 rows > 3072 tiles x 32: every read block walks several tiles, the column softmax merges 3074 / 769 partials out of registers, the row
                backward runs 12 to 13 rows per wave
  write-small   63 rows under 30 x 20 labels at m = 6 (scalar stores, scalar reduce), 19 and 31 (the widest), normalised or not; empty classes, ignored and
                out-of-range labels, an all-zero row
  write-chunks  33 024 rows > 512 blocks x 64: blocks take a second chunk, the backward is grid-strided
Inputs come from CPU generators with fixed seeds; what is not elementwise (the memory's normalisation, the logarithm of the noise) is computed in fp64 and rounded."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'memory_bits.json')
D = 256
MU = 0.8

# (name, x shape, slot counts, noise settings, (pitch of x's slab, pitch of dqr's slab) or None)
READ_CASES = [
    ('slots', (2, 9, 7, D), (1, 8, 9, 19, 20, 31, 32), (0, 1), None),
    ('views', (2, 9, 7, D), (19, 20), (0, 1), (272, 528)),
    ('tile-loop', (1, 8, 12293, D), (19, 20), (1,), None),
]
# (name, z shape, label shape, slot counts, normalize settings)
WRITE_CASES = [
    ('write-small', (1, 9, 7, D), (1, 30, 20), (6, 19, 31), (0, 1)),
    ('write-chunks', (2, 129, 128, D), (2, 516, 512), (19,), (1,)),
]
FLAGSHIP = ('flagship', (8, 48, 48, D), (19,))
READ_RUNS = [(c, m, noise) for c in READ_CASES for m in c[2] for noise in c[3]]
WRITE_RUNS = [(c, m, nz) for c in WRITE_CASES for m in c[3] for nz in c[4]]
BWD_MODES = [(dmem, dsx) for dmem in (0, 1) for dsx in (0, 1)]


def run_id(case, m, flag):
    return '%s/m=%d/%s=%d' % (case[0], m, 'noise' if case in READ_CASES else 'normalize', flag)


def workspaces(lib, shape, m):
    """The four size queries for an fp32 [n, h, w, 256] tensor and m slots: read_fwd_pq, colsoftmax, read_bwd, write_accum. Host code only."""
    from pinthememory_amd.hip import lib as L
    n, h, w, c = shape
    z = L.PmTensor(None, n, h, w, c, c, L.PM_F32, 0)
    rows = n * h * w
    return [lib.pm_mem_read_fwd_pq_workspace(rows, m), lib.pm_mem_colsoftmax_workspace(rows, m), lib.pm_mem_read_bwd_workspace(rows, m, c),
            lib.pm_mem_write_accum_workspace(z, m)]


def workspace_shapes():
    return [(c[0], c[1], c[2]) for c in READ_CASES] + [(c[0], c[1], c[3]) for c in WRITE_CASES] + [FLAGSHIP]


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _slice_of_slab(cpu, pitch, off=8):
    import torch
    n, h, w, c = cpu.shape
    v = torch.zeros((n, h, w, pitch), dtype=torch.float32, device='cuda')[..., off:off + c]
    v.copy_(cpu)
    return v


def _memory(m, g):
    import torch
    v = torch.randn(m, D, generator=g).double()
    return (v / v.norm(dim=1, keepdim=True)).float().cuda()


def _gumbel(shape, g):
    import torch
    return (-torch.empty(shape, dtype=torch.float64).exponential_(generator=g).log()).float().cuda()


def read_inputs(case, m, noise):
    """-> x, mem, noise, noise_q, dqr, dsx on the device. relu(randn) features with one all-zero row, a normalised memory, Gumbel noise, non-zero dsx."""
    import torch
    name, shape, _, _, pitches = case
    rows = shape[0] * shape[1] * shape[2]
    g = torch.Generator().manual_seed(1000 + 37 * m + rows % 997)
    x = torch.relu(torch.randn(shape, generator=g))
    x.view(-1, D)[5] = 0
    dqr = torch.randn(shape[:3] + (2 * D,), generator=g)
    dsx = torch.randn(rows, m, generator=g).cuda()
    mem = _memory(m, g)
    nz, nq = (_gumbel((rows, m), g), _gumbel((rows, m), g)) if noise else (None, None)
    if pitches:
        return _slice_of_slab(x, pitches[0]), mem, nz, nq, _slice_of_slab(dqr, pitches[1]), dsx
    return x.cuda(), mem, nz, nq, dqr.cuda(), dsx


def run_read(K, case, m, noise):
    """Every read entry point on the case's inputs -> {call: {output: sha256}}."""
    import torch
    x, mem, nz, nq, dqr, dsx = read_inputs(case, m, noise)
    out = {}
    qr, score, pmem = K.mem_read_fwd(x, mem, nz)
    out['mem_read_fwd'] = dict(qr=digest(qr), score=digest(score), p_mem=digest(pmem))
    qr2, score2, pmem2, pq = K.mem_read_fwd_pq(x, mem, nz, nq)
    out['mem_read_fwd_pq'] = dict(qr=digest(qr2), score=digest(score2), p_mem=digest(pmem2), p_query=digest(pq))
    out['mem_colsoftmax'] = dict(p_query=digest(K.mem_colsoftmax(score, nq)))
    for want_dmem, with_dsx in BWD_MODES:
        dx, dmem = K.mem_read_bwd(x, mem, pmem, dqr, dsx if with_dsx else None, want_dmem=bool(want_dmem))
        outs = dict(dx=digest(dx))
        if want_dmem:
            outs['dmem'] = digest(dmem)
        out['mem_read_bwd[dmem=%d,dsx=%d]' % (want_dmem, with_dsx)] = outs
    torch.cuda.synchronize()
    return out


def write_inputs(case, m):
    """-> z, labels, mem, dnom, dout on the device. Labels from [0, m - 3): the classes m - 3, m - 2, m - 1 stay empty; 10 % are 255 (ignored); m, -1 and 200 are
    planted (m is the ignore row's own index, the other two belong to no class). One row of z is all zero."""
    import torch
    name, zshape, lshape, _, _ = case
    g = torch.Generator().manual_seed(2000 + 41 * m + zshape[1])
    z = torch.relu(torch.randn(zshape, generator=g))
    z.view(-1, D)[7] = 0
    lab = torch.randint(0, m - 3, lshape, generator=g)
    lab[torch.rand(lshape, generator=g) < 0.1] = 255
    flat = lab.view(-1)
    flat[3], flat[lshape[2] + 1], flat[flat.numel() // 2] = m, -1, 200
    dnom = torch.randn(m + 1, D, generator=g)
    dout = torch.randn(m, D, generator=g)
    return z.cuda(), lab.cuda(), _memory(m, g), dnom.cuda(), dout.cuda()


def run_write(K, case, m, normalize):
    """Every write entry point on the case's inputs -> {call: {output: sha256}}."""
    import torch
    from pinthememory_amd.hip import lib as L
    z, lab, mem, dnom, dout = write_inputs(case, m)
    out = {}
    nomden = K.mem_write_accum(z, lab, m, normalize=bool(normalize))
    out['mem_write_accum'] = dict(nomden=digest(nomden))
    out['mem_write_accum_bwd'] = dict(dz=digest(K.mem_write_accum_bwd(z, lab, m, dnom, normalize=bool(normalize))))
    new, u = K.mem_write_update(mem, nomden, MU, want_u=True)
    out['mem_write_update'] = dict(mem=digest(new), u=digest(u))
    out['mem_write_update_bwd'] = dict(dnom=digest(K.mem_write_update_bwd(u, nomden, MU, dout)))
    dn2, dmem_in = torch.empty((m + 1, D), dtype=torch.float32, device='cuda'), torch.empty((m, D), dtype=torch.float32, device='cuda')
    L.check(L.load().pm_mem_write_update_bwd(u.data_ptr(), nomden.data_ptr(), m, D, MU, dout.data_ptr(), dn2.data_ptr(), dmem_in.data_ptr(), L.stream()),
            'pm_mem_write_update_bwd')
    out['mem_write_update_bwd[dmem_in]'] = dict(dnom=digest(dn2), dmem_in=digest(dmem_in))
    torch.cuda.synchronize()
    return out


def main():
    assert os.environ.get('PM_LIB'), 'set PM_LIB to a library built from the parent commit (tools/build_base_lib.sh)'
    import torch
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    fixture = {'digests': {}}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            fixture = json.load(f)
    fixture['workspaces'] = {name: {str(m): workspaces(lib, shape, m) for m in ms} for name, shape, ms in workspace_shapes()}
    if torch.cuda.is_available():
        from pinthememory_amd.hip import kernels as K
        version = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--version'], capture_output=True, text=True).stdout
        fixture['hipcc'] = next((l.strip() for l in version.splitlines() if 'version' in l.lower()), '')      # for information only
        fixture['digests'] = {run_id(*r): run_read(K, *r) for r in READ_RUNS}
        fixture['digests'].update({run_id(*r): run_write(K, *r) for r in WRITE_RUNS})
    else:
        print('no GPU: workspace answers recorded, digests kept as they were')
    with open(FIXTURE, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d run digests, %d workspace shapes -> %s' % (len(fixture['digests']), len(fixture['workspaces']), FIXTURE))


if __name__ == '__main__':
    main()
