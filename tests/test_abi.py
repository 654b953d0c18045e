"""CPU: the C-ABI shared library loads and exports exactly the entry points include/pinmem_hip.h declares
(no compute calls here -- there is no GPU in the build container)."""
import os
import re
import subprocess
import sys

from pinthememory_amd import build
from pinthememory_amd.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, 'include', 'pinmem_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(pm_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_and_exports_every_declared_symbol():
    build.build()
    lib = L.load()
    names = declared()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), 'missing export ' + n
    assert sorted(L.SIGNATURES) == names, 'ctypes table and header drifted apart'
    hdr = int(re.search(r'#define PM_ABI_VERSION (\d+)', open(os.path.join(ROOT, 'include', 'pinmem_hip.h')).read()).group(1))
    assert lib.pm_version() == hdr == L.ABI_VERSION          # library, header and ctypes binding agree on the struct layouts
    assert lib.pm_last_error() is not None


def test_struct_size_guards_reject_a_caller_built_against_another_header():
    """pm_conv_params / pm_conv_epilogue grew in rounds 2 and 3; their first member is their own size, and an entry point that receives another size
    (a consumer compiled against an older header) refuses the call instead of reading past the caller's object."""
    import ctypes
    from ctypes import byref
    lib = L.load()
    assert ctypes.sizeof(L.PmConvParams) == L.conv_params(3, 3, 1, 1, 1).struct_size
    buf = (ctypes.c_float * 64)()
    x = L.PmTensor(ctypes.addressof(buf), 1, 2, 2, 4, 4)
    y = L.PmTensor(ctypes.addressof(buf), 1, 2, 2, 4, 4)
    p = L.conv_params(1, 1, 1, 0, 1)
    p.struct_size -= 8                                     # "older header"
    assert lib.pm_conv_fwd(byref(x), ctypes.addressof(buf), byref(y), byref(p), None, None, 0, None) == -1
    assert b'struct_size' in lib.pm_last_error()
    p = L.conv_params(1, 1, 1, 0, 1)
    ep = L.conv_epilogue(None, None, None, None, 0, 0, None, 0)
    ep.struct_size = 48
    assert lib.pm_conv_fwd(byref(x), ctypes.addressof(buf), byref(y), byref(p), byref(ep), None, 0, None) == -1
    assert b'pm_conv_epilogue.struct_size' in lib.pm_last_error()


def test_argument_validation_without_gpu():
    """Entry points reject bad arguments before touching the device (error convention of the boundary)."""
    lib = L.load()
    assert lib.pm_mem_colsoftmax(None, None, 0, 19, None, None, 0, None) == -1
    assert b'mem_colsoftmax' in lib.pm_last_error()
    assert lib.pm_sgd_momentum(None, None, None, 10, 0.1, 0.9, 0.0, 1, None) == -1


def test_routing_is_one_struct_with_single_field_wrappers():
    """Round 6: the library's only mutable global state is ONE pm_routing value -- struct_size-guarded, read and replaced as a whole; the pm_set_*
    entry points change one field of it. No compute: which kernel WOULD take a call."""
    import ctypes
    from ctypes import byref
    lib = L.load()
    r = L.PmRouting()
    r.struct_size = ctypes.sizeof(L.PmRouting)
    assert lib.pm_routing_get(byref(r)) == 0
    before = {k: getattr(r, k) for k, _ in L.PmRouting._fields_}
    assert before['winograd'] in (0, 2, 4) and before['split'] in (0, 1) and before['conv16'] in (0, 1, 2)
    bad = L.PmRouting()
    bad.struct_size = ctypes.sizeof(L.PmRouting) - 4                 # "another header"
    assert lib.pm_routing_get(byref(bad)) == -1 and b'struct_size' in lib.pm_last_error()
    assert lib.pm_routing_set(byref(bad)) == -1
    try:
        assert lib.pm_set_split(0) == 0 and lib.pm_set_winograd(2) == 0 and lib.pm_set_conv16(8) == 0
        assert lib.pm_routing_get(byref(r)) == 0
        assert (r.split, r.winograd, r.conv16, r.conv16_wide, r.conv16_persistent) == (0, 2, 2, 2, 0)
        assert lib.pm_set_conv16(5) == 0 and lib.pm_routing_get(byref(r)) == 0 and r.conv16 == 1      # the streaming 1x1 kernel left the library: 5 / 6 mean 1
        r.winograd = 3
        assert lib.pm_routing_set(byref(r)) == -1 and b'winograd' in lib.pm_last_error()              # validated as a whole, nothing applied
        assert lib.pm_routing_get(byref(r)) == 0 and r.winograd == 2
    finally:
        for k, v in before.items():
            setattr(r, k, v)
        assert lib.pm_routing_set(byref(r)) == 0
    assert lib.pm_routing_get(byref(r)) == 0 and {k: getattr(r, k) for k, _ in L.PmRouting._fields_} == before


def test_set_conv16_restores_the_routing_read_at_load():
    """pm_set_conv16(1) puts conv16_wide / conv16_persistent back to the values the library read from its environment when it was loaded, not to whatever
    the routing held at the first pm_set_conv16 call. A fresh process with no PM_* variable set (the library is loaded once per process): both defaults are 1."""
    L.load()
    code = '''
import ctypes, sys
from ctypes import byref
from pinthememory_amd.hip.lib import PmRouting
lib = ctypes.CDLL(sys.argv[1])
r = PmRouting(ctypes.sizeof(PmRouting))
assert lib.pm_routing_get(byref(r)) == 0
r.conv16_wide = r.conv16_persistent = 0
assert lib.pm_routing_set(byref(r)) == 0 and lib.pm_set_conv16(1) == 0 and lib.pm_routing_get(byref(r)) == 0
print(r.conv16_wide, r.conv16_persistent)
'''
    env = {k: v for k, v in os.environ.items() if not k.startswith('PM_')}
    out = subprocess.run([sys.executable, '-c', code, L.LIB_PATH], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ['1', '1']


def _size_table():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('record_conv_sizes', os.path.join(ROOT, 'tools', 'record_conv_sizes.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.FIXTURE) as f:
        return tool, json.load(f)


def test_conv_size_queries_answer_what_the_recorded_table_holds():
    """tests/golden/conv_size_queries.json: the seven size queries of every convolution call signature of the networks (one training step of DeepV3Plus-R50 at 2 x 128^2 and
    8 x 768^2 on both tiers, one DeepV2 eval tile) and of a hand-written edge list, under the default routing and every single-field departure from it, recorded from the
    library BEFORE the queries became field reads of route_conv (tools/record_conv_sizes.py against the parent commit's build). Every row is held exactly: pure host code,
    fake aligned pointers, no GPU."""
    import ctypes
    from ctypes import byref
    tool, table = _size_table()
    lib = L.load()
    before = L.PmRouting(ctypes.sizeof(L.PmRouting))
    assert lib.pm_routing_get(byref(before)) == 0
    assert 1000 <= len(table['rows']) <= 5000 and {r[1] for r in table['rows']} == {n for n, _, _ in tool.ROUTINGS}
    try:
        for name, fields, _ in tool.ROUTINGS:
            with tool.routing(lib, L, fields):
                for s, rname, want in table['rows']:
                    if rname == name:
                        assert tool.query(lib, L, s) == want, (s, name)
        # the recorder itself, run against this build, writes the committed file byte for byte
        sigs = table['network_signatures'] + [s for s in tool.edge_signatures() if s not in table['network_signatures']]
        with open(tool.FIXTURE) as f:
            assert tool.dumps(table['network_signatures'], tool.edge_signatures(), tool.rows(lib, L, sigs)) == f.read()
    finally:
        assert lib.pm_routing_set(byref(before)) == 0


def test_conv_entry_points_require_exactly_the_queried_workspace():
    """A query and the call it sizes share one plan: with one byte less than pm_conv_workspace answered, every entry point refuses the call before any launch
    (PM_EWORKSPACE; there is no device here, so the calls are made with need - 1 only). Every recorded row with a workspace, fake aligned pointers."""
    import ctypes
    from ctypes import byref
    tool, table = _size_table()
    lib = L.load()
    before = L.PmRouting(ctypes.sizeof(L.PmRouting))
    assert lib.pm_routing_get(byref(before)) == 0
    W, DW, WS = 0x8000000, 0x9000000, 0xC000000
    calls = 0
    try:
        for name, fields, _ in tool.ROUTINGS:
            with tool.routing(lib, L, fields):
                for s, rname, want in table['rows']:
                    if rname != name:
                        continue
                    x, y = L.PmTensor(tool.X_PTR, *s[0:7]), L.PmTensor(tool.Y_PTR, *s[7:14])
                    p = L.conv_params(s[14], s[14], s[15], s[16], s[17], s[18])
                    for which, need in enumerate(want[:3]):
                        if need == 0:
                            continue
                        if which == 0:
                            rc = lib.pm_conv_fwd(byref(x), W, byref(y), byref(p), None, WS, need - 1, None)
                        elif which == 1:
                            rc = lib.pm_conv_bwd_data(byref(y), W, byref(x), byref(p), None, WS, need - 1, None)
                        else:
                            rc = lib.pm_conv_bwd_weight(byref(x), byref(y), DW, None, byref(p), WS, need - 1, None)
                        calls += 1
                        assert rc == -2 and b'workspace' in lib.pm_last_error(), (s, name, which, need, rc, lib.pm_last_error())      # PM_EWORKSPACE
    finally:
        assert lib.pm_routing_set(byref(before)) == 0
    assert calls >= 2000
