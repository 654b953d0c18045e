"""Poisoned slabs around the tensors a kernel test hands to the library (tests/test_tensor_views.py, tests/test_tensor_views_cpu.py).

A test that allocates every tensor on its own cannot see a kernel that indexes with `c` where it should use `pitch`, stores one row too many from a ragged tile, or
folds rows behind the tensor into a reduction: the stray access lands in the allocator's pool. Here every tensor lives inside memory the test owns:

    buf, view = slab((n, h, w, c), dtype, layout, role, data)      # NHWC view inside a wider, longer buffer
    buf, arr = flat(numel, dtype, role, data)                      # dense array between two margins
    before = snapshot(bufs); <call>; check(before, bufs)

Plain torch with a device argument, so the harness itself is tested on the CPU. What it can show: every write outside a view, every write into an input, every output
element left unwritten, and every read outside a view WHOSE VALUE REACHES A RESULT (the surroundings hold NaN, so does 0 * them). A stray load that a select discards
is not observable this way."""
import torch

GUARD_ROWS = 256      # pixels of the slab's full width before and after the view: the tallest row tile of any kernel
FLAT_MARGIN = 64      # elements on both sides of a flat array
LAYOUTS = ('dense', 'slice', 'odd', 'ownpad')
ROLES = ('in', 'out', 'inout')
LABEL_FILL = 1        # margins of a label array hold a VALID class: an over-read changes counts and sums
BYTE_FILL = 0xA5


def _round_up(v, a):
    return (v + a - 1) // a * a


def geometry(c, dtype, layout):
    """-> (channel offset of the view, pitch, number of pad lanes behind c that belong to the view)"""
    assert layout in LAYOUTS, layout
    bf16 = dtype == torch.bfloat16
    if layout == 'dense':
        return 0, c, 0
    if layout == 'slice':
        return (64, c + 128, 0) if bf16 else (32, c + 64, 0)
    if layout == 'odd':
        assert not bf16, 'the bf16 tier has no scalar form: no odd layout'
        assert c % 4 != 1, 'pitch c + 3 would be a multiple of 4'
        return 1, c + 3, 0
    if bf16:          # own pad up to a multiple of 64 (zeros), inside a wider pitch whose other lanes are poison
        assert c % 64 != 0
        return 64, _round_up(c, 64) + 128, _round_up(c, 64) - c
    assert c % 4 != 0
    return 0, _round_up(c, 4), _round_up(c, 4) - c


def _poison(mem):
    if mem.dtype.is_floating_point:
        mem.fill_(float('nan'))
    elif mem.dtype == torch.uint8:
        mem.fill_(BYTE_FILL)
    else:
        mem.fill_(LABEL_FILL)


class Buffer:
    """One owned allocation: `mem` (1-D), the view or array inside it, and which elements are the interior / the view's own pad lanes."""

    def __init__(self, mem, view, role, inside, pad, pitch=None, layout=None):
        self.mem, self.view, self.role, self.inside, self.pad, self.pitch, self.layout = mem, view, role, inside, pad, pitch, layout

    def bytes(self):
        return self.mem.view(torch.uint8)

    def byte_mask(self, elems):
        return elems.repeat_interleave(self.mem.element_size())


def slab(shape_nhwc, dtype, layout, role, data=None, device='cpu'):
    """-> (Buffer, NHWC view of shape_nhwc). data: the interior of an 'in' / 'inout' tensor (any device, converted to dtype)."""
    assert role in ROLES, role
    n, h, w, c = shape_nhwc
    off, pitch, npad = geometry(c, dtype, layout)
    pixels = n * h * w
    rows = GUARD_ROWS + pixels + GUARD_ROWS
    mem = torch.empty(rows * pitch + 4, dtype=dtype, device=device)      # + 4: the odd layout starts one element in
    _poison(mem)
    first = GUARD_ROWS * pitch + off
    view = mem.as_strided((n, h, w, c), (h * w * pitch, w * pitch, pitch, 1), first)
    idx = torch.arange(mem.numel(), device=device) - first
    lane = torch.remainder(idx, pitch)
    row_ok = (idx >= 0) & (torch.div(idx, pitch, rounding_mode='floor') < pixels)
    inside = row_ok & (lane < c)
    pad = row_ok & (lane >= c) & (lane < c + npad)
    if npad:
        mem[pad] = 0
    if role in ('in', 'inout'):
        assert data is not None and tuple(data.shape) == tuple(shape_nhwc), 'an %s slab needs its data' % role
        view.copy_(data.to(device))
    else:
        assert data is None
    return Buffer(mem, view, role, inside, pad, pitch, layout), view


def flat(numel, dtype, role, data=None, device='cpu'):
    """-> (Buffer, 1-D array of numel elements) with FLAT_MARGIN poisoned elements on both sides."""
    assert role in ROLES, role
    mem = torch.empty(numel + 2 * FLAT_MARGIN, dtype=dtype, device=device)
    _poison(mem)
    arr = mem[FLAT_MARGIN:FLAT_MARGIN + numel]
    inside = torch.zeros(mem.numel(), dtype=torch.bool, device=device)
    inside[FLAT_MARGIN:FLAT_MARGIN + numel] = True
    if role in ('in', 'inout'):
        assert data is not None and data.numel() == numel, 'an %s array needs its data' % role
        arr.copy_(data.reshape(-1).to(device))
    elif not dtype.is_floating_point:
        arr.fill_(BYTE_FILL if dtype == torch.uint8 else torch.iinfo(dtype).min + 0x5A)      # no NaN here: a value no kernel of the library produces by itself
    return Buffer(mem, arr, role, inside, torch.zeros_like(inside)), arr


def snapshot(buffers):
    """The bytes of every buffer, to be handed to check() after the call."""
    return [b.bytes().clone() for b in buffers]


def problems(before, buffers):
    """-> list of findings (empty: the call kept to its views). before: snapshot(buffers) taken ahead of the call.
    1. every byte outside every interior is unchanged (raw bytes: NaN payloads do not compare by value); own pad lanes hold zero;
    2. every byte of every 'in' buffer is unchanged, interior included;
    3. the interior of every 'out' / 'inout' buffer of a floating type is finite."""
    out = []
    assert len(before) == len(buffers)
    for i, (old, b) in enumerate(zip(before, buffers)):
        new = b.bytes()
        changed = old != new
        if b.role == 'in':
            if bool(changed.any()):
                out.append('buffer %d (in): %d bytes of an input changed' % (i, int(changed.sum())))
            continue
        outside = b.byte_mask(~(b.inside | b.pad))
        if bool((changed & outside).any()):
            at = int(torch.nonzero(changed & outside)[0]) // b.mem.element_size()
            out.append('buffer %d (%s): %d bytes outside the view changed, first at element %d' % (i, b.role, int((changed & outside).sum()), at))
        if bool(b.pad.any()) and bool((b.mem[b.pad] != 0).any()):
            out.append('buffer %d (%s): a pad lane of the view is not zero' % (i, b.role))
        if b.mem.dtype.is_floating_point:
            bad = ~torch.isfinite(b.mem[b.inside].float() if b.mem.dtype == torch.bfloat16 else b.mem[b.inside])
            if bool(bad.any()):
                out.append('buffer %d (%s): %d interior elements are not finite' % (i, b.role, int(bad.sum())))
    return out


def check(before, buffers):
    found = problems(before, buffers)
    assert not found, '; '.join(found)
