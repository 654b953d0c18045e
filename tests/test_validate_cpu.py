"""CPU: the validation sweep's entry points (pm_upsample_eval, pm_upsample_eval_workspace) are exported, reject bad arguments before touching the device, and
the workspace query tells a shape the kernel takes from one it does not (no compute calls here: there is no GPU in the build container)."""
import ctypes
from ctypes import byref

from pinthememory_amd.hip import lib as L


def desc(n, h, w, c, dtype=L.PM_F32):
    """A pm_tensor with a pitch-padded row and a pointer that is never read (size queries and argument checks only)."""
    buf = (ctypes.c_float * 4)()
    return L.PmTensor(ctypes.addressof(buf), n, h, w, c, (c + 3) // 4 * 4, dtype, 0), buf


def test_library_exports_the_validation_entry_points():
    lib = L.load()
    for name in ('pm_upsample_eval', 'pm_upsample_eval_workspace'):
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_null_arguments_are_rejected_without_a_gpu():
    lib = L.load()
    assert lib.pm_upsample_eval(None, 1.0, None, 8, 8, None, None, 0, None, None, 0, None) == -1
    assert b'upsample_eval' in lib.pm_last_error()
    t, keep = desc(1, 4, 4, 19)
    lab = (ctypes.c_int64 * 64)()
    out, hist = (ctypes.c_float * 2)(), (ctypes.c_int64 * 361)()
    assert lib.pm_upsample_eval(byref(t), 1.0, None, 8, 8, out, hist, 0, None, None, 0, None) == -1                      # labels
    assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, None, hist, 0, None, None, 0, None) == -1                      # loss_out
    assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, out, None, 0, None, None, 0, None) == -1                       # hist
    assert b'upsample_eval' in lib.pm_last_error()
    assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, out, hist, 2, None, None, 0, None) == -1                       # accumulate is 0 or 1
    assert b'accumulate' in lib.pm_last_error()
    assert lib.pm_upsample_eval_workspace(None, 8, 8) == 0


def test_class_count_workspace_and_shape_checks_come_before_any_launch():
    lib = L.load()
    lab = (ctypes.c_int64 * 64)()
    out, hist = (ctypes.c_float * 2)(), (ctypes.c_int64 * 4096)()
    for c in (0, 33):
        t, keep = desc(1, 4, 4, c)
        assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, out, hist, 0, None, None, 0, None) == -4       # PM_EUNSUPPORTED
        assert b'upsample_eval' in lib.pm_last_error()
        assert lib.pm_upsample_eval_workspace(byref(t), 8, 8) == 0
    t, keep = desc(1, 4, 4, 19)
    need = lib.pm_upsample_eval_workspace(byref(t), 8, 8)
    assert need > 0
    ws = (ctypes.c_char * need)()
    assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, out, hist, 0, None, ws, need - 1, None) == -2       # PM_EWORKSPACE
    assert b'workspace' in lib.pm_last_error()
    assert lib.pm_upsample_eval(byref(t), 1.0, lab, 8, 8, out, hist, 0, None, None, need, None) == -2
    bf, keep = desc(1, 4, 4, 19, L.PM_BF16)                                                                  # fp32 logits only
    assert lib.pm_upsample_eval_workspace(byref(bf), 8, 8) == 0
    assert lib.pm_upsample_eval(byref(bf), 1.0, lab, 8, 8, out, hist, 0, None, ws, need, None) == -4


def test_workspace_query_for_one_cityscapes_image():
    lib = L.load()
    t, keep = desc(1, 256, 512, 19)
    need = lib.pm_upsample_eval_workspace(byref(t), 1024, 2048)
    assert need > 0 and need % 256 == 0
    # at least the per-row loss partials and one block's C x C counters
    assert need >= 1024 * 2 * 4 + 361 * 4


def test_workspace_query_answers_zero_for_a_row_too_wide_for_lds():
    """The width comes from pm_upsample_ce_field_bytes' own limit: two low-res logit rows of w x 19 floats in 159 KB of LDS, w <= ~1000. 1100 columns are refused
    by both queries (and by the call, before any launch); 1000 columns are taken by both."""
    lib = L.load()
    wide, keep = desc(1, 16, 1100, 19)
    assert lib.pm_upsample_ce_field_bytes(byref(wide), 64, 4400) == 0
    assert lib.pm_upsample_eval_workspace(byref(wide), 64, 4400) == 0
    lab = (ctypes.c_int64 * 8)()
    out, hist, ws = (ctypes.c_float * 2)(), (ctypes.c_int64 * 361)(), (ctypes.c_char * 256)()
    assert lib.pm_upsample_eval(byref(wide), 1.0, lab, 64, 4400, out, hist, 0, None, ws, 256, None) == -4     # PM_EUNSUPPORTED
    assert b'LDS' in lib.pm_last_error()
    ok, keep = desc(1, 16, 1000, 19)
    assert lib.pm_upsample_ce_field_bytes(byref(ok), 64, 4000) != 0
    assert lib.pm_upsample_eval_workspace(byref(ok), 64, 4000) % 256 == 0 and lib.pm_upsample_eval_workspace(byref(ok), 64, 4000) > 0
