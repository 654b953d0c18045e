"""Pooling, resize and elementwise passes at the workload's shapes, both tiers: median of 30 calls (HIP events, us) per line.

    python tools/pool_probe.py                      # the in-tree library
    PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so python tools/pool_probe.py

Lines: the stem max pool 8x384x384x64 (forward, backward), the average pool 8x48x48x2048 (forward, backward), the decoder resize 8x48x48x256 -> 192x192 (forward,
separable backward, gather backward), the ASPP image feature 8x1x1x256 -> 48x48 (forward, backward), add_n of five 8x48x48x2048 tensors and the copy of one, as fp32
and as bf16. The outputs are allocated once and the library is called directly, so a line times the kernels and the launch. profiles/pool_refactor_ab.txt holds a
parent / tree / parent / tree series of it."""
import os
import sys
from ctypes import POINTER, byref, pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CALLS = 30


def median_us(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    from pinthememory_amd.hip import lib as L
    lib = L.load()
    st = L.stream()
    print('pool_probe: %s, library %s, median of %d calls (HIP events, us)' % (torch.cuda.get_device_name(0), L.LIB_PATH, CALLS))
    g = torch.Generator().manual_seed(7)

    def rnd(*shape, dtype):
        return torch.randn(shape, generator=g).to('cuda', dtype)

    def T(t):
        return byref(L.tdesc(t))

    def ok(code):
        assert code == 0, lib.pm_last_error()

    for dtype, tag in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
        lines = []
        x, y, dy = rnd(8, 384, 384, 64, dtype=dtype), rnd(8, 192, 192, 64, dtype=dtype), rnd(8, 192, 192, 64, dtype=dtype)
        dx, arg = torch.empty_like(x), torch.empty((8, 192, 192, 64), dtype=torch.uint8, device='cuda')
        lines.append(('max pool 8x384x384x64', 'forward', lambda: ok(lib.pm_maxpool3x3s2_fwd(T(x), T(y), arg.data_ptr(), st))))
        lines.append(('max pool 8x384x384x64', 'backward', lambda: ok(lib.pm_maxpool3x3s2_bwd(T(dy), arg.data_ptr(), T(dx), st))))
        a, pa, da = rnd(8, 48, 48, 2048, dtype=dtype), rnd(8, 1, 1, 2048, dtype=dtype), rnd(8, 48, 48, 2048, dtype=dtype)
        lines.append(('average pool 8x48x48x2048', 'forward', lambda: ok(lib.pm_global_avgpool_fwd(T(a), T(pa), st))))
        lines.append(('average pool 8x48x48x2048', 'backward', lambda: ok(lib.pm_global_avgpool_bwd(T(pa), T(da), 0, st))))
        lo, hi = rnd(8, 48, 48, 256, dtype=dtype), rnd(8, 192, 192, 256, dtype=dtype)
        nb = lib.pm_resize_bilinear_bwd_workspace(T(hi), T(lo))
        ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
        lines.append(('resize 8x48x48x256 -> 192x192', 'forward', lambda: ok(lib.pm_resize_bilinear_fwd(T(lo), T(hi), st))))
        lines.append(('resize 8x48x48x256 -> 192x192', 'backward, separable', lambda: ok(lib.pm_resize_bilinear_bwd_separable(T(hi), T(lo), 0, ws.data_ptr(), nb, st))))
        lines.append(('resize 8x48x48x256 -> 192x192', 'backward, gather', lambda: ok(lib.pm_resize_bilinear_bwd(T(hi), T(lo), 0, st))))
        one, up = rnd(8, 1, 1, 256, dtype=dtype), rnd(8, 48, 48, 256, dtype=dtype)
        lines.append(('resize 8x1x1x256 -> 48x48', 'forward', lambda: ok(lib.pm_resize_bilinear_fwd(T(one), T(up), st))))
        lines.append(('resize 8x1x1x256 -> 48x48', 'backward', lambda: ok(lib.pm_resize_bilinear_bwd(T(up), T(one), 0, st))))
        xs = [a, da] + [rnd(8, 48, 48, 2048, dtype=dtype) for _ in range(3)]
        descs = [L.tdesc(t) for t in xs]
        arr = (POINTER(L.PmTensor) * 5)(*[pointer(d) for d in descs])
        out = torch.empty_like(a)
        lines.append(('add_n of five 8x48x48x2048', 'one pass', lambda: ok(lib.pm_add_n(arr, 5, T(out), st))))
        lines.append(('copy of 8x48x48x2048', 'one pass', lambda: ok(lib.pm_copy(T(a), T(out), st))))
        for name, line, fn in lines:
            print('%-36s | %-22s %10.1f' % (tag + ' ' + name, line, median_us(fn)))
        del x, y, dy, dx, arg, a, pa, da, lo, hi, ws, one, up, xs, out


if __name__ == '__main__':
    main()
