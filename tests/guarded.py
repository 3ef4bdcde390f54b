"""A guarded arena for the tests of where the library writes (tests/test_gpu_caller_memory_*.py): ONE uint8 tensor filled with a
poison byte, out of which outputs and inputs are carved at a chosen pointer residue with at least GUARD poisoned bytes on either
side.  check() compares the whole arena with a snapshot taken just before the call under test: every byte outside the extents
the call was allowed to write -- the guard bands, the gaps between carvings, every input -- must be as it was.

The comparison itself (first_change, describe) works on numpy byte arrays and is tested on the CPU by tests/test_guarded_host.py;
carve's arithmetic only needs data_ptr(), so a CPU arena (device='cpu') tests that too."""
import collections

import numpy as np

GUARD = 4096
Carving = collections.namedtuple('Carving', 'name start end')  # byte offsets into the arena, [start, end)


def first_change(before, after, written):
    """before, after: uint8 arrays of one length; written: (start, end) byte ranges that MAY differ.  Returns the offset of the
    first byte outside every range that differs, or None"""
    before, after = np.asarray(before, np.uint8).reshape(-1), np.asarray(after, np.uint8).reshape(-1)
    assert before.shape == after.shape
    changed = before != after
    for start, end in written:
        assert 0 <= start <= end <= len(changed), (start, end, len(changed))
        changed[start:end] = False
    at = np.flatnonzero(changed)
    return int(at[0]) if len(at) else None


def describe(offset, carvings, before, after):
    """the report of a changed byte: the carving it lies nearest to, its signed distance from that carving's start (negative: in
    front of it), from its end (>= 0: behind it) or its offset inside it, and the old and new byte"""
    def dist(c):
        return c.start - offset if offset < c.start else offset - (c.end - 1) if offset >= c.end else 0
    if not carvings:
        return 'byte %d changed: 0x%02X -> 0x%02X (no carvings)' % (offset, before[offset], after[offset])
    c = min(carvings, key=dist)
    if offset < c.start:
        where = '%d from the start of' % (offset - c.start)
    elif offset >= c.end:
        where = '+%d from the end of' % (offset - c.end)
    else:
        where = 'at byte %d inside' % (offset - c.start)
    return 'byte %d changed, %s %r [%d, %d): 0x%02X -> 0x%02X' % (offset, where, c.name, c.start, c.end, before[offset], after[offset])


def place_offset(base, cursor, align, residue, itemsize, guard=GUARD):
    """the smallest offset >= cursor + guard with (base + offset) % align == residue"""
    if align <= 0 or align & (align - 1):
        raise ValueError('align must be a power of two, not %r' % (align,))
    if not 0 <= residue < align:
        raise ValueError('residue %r is not below align %r' % (residue, align))
    if residue % itemsize or align % itemsize:
        raise ValueError('a pointer to %d-byte elements cannot be at %d mod %d' % (itemsize, residue, align))
    start = cursor + guard
    return start + (residue - (base + start)) % align


class Arena:
    def __init__(self, nbytes, poison, device='cuda'):
        import torch
        self.torch = torch
        self.poison = int(poison)
        self.bytes = torch.full((int(nbytes),), self.poison, dtype=torch.uint8, device=device)
        self.base = self.bytes.data_ptr()
        self.cursor = 0
        self.carvings = []
        self.before = None

    def carve(self, shape, dtype, align=16, residue=0, name=None):
        """a contiguous view of `dtype` (a torch dtype) and `shape` whose data_ptr() % align == residue, poison on both sides"""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        itemsize = self.torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        start = place_offset(self.base, self.cursor, align, residue, itemsize)
        if start + nbytes + GUARD > self.bytes.numel():
            raise ValueError('the arena (%d bytes) has no room for %d bytes at %d and a guard band' % (self.bytes.numel(), nbytes, start))
        view = self.bytes[start:start + nbytes].view(dtype).view(shape)
        assert view.data_ptr() == self.base + start and view.data_ptr() % align == residue and view.is_contiguous()
        self.carvings.append(Carving(name or '#%d %s%s' % (len(self.carvings), str(dtype).replace('torch.', ''), list(shape)), start,
                                     start + nbytes))
        self.cursor = start + nbytes
        return view

    def place(self, array, align=16, residue=0, name=None, dtype=None):
        """carve room for the host array and copy it in.  dtype: the torch dtype of the view, of the array's shape and item size;
        None: the array's bytes as one flat uint8 view, what the wrappers take for records"""
        a = np.ascontiguousarray(array)
        raw = a.reshape(-1).view(np.uint8).copy()
        if dtype is None:
            view = self.carve(raw.shape, self.torch.uint8, align, residue, name)
        else:
            view = self.carve(a.shape, dtype, align, residue, name)
            assert view.element_size() == a.itemsize, (dtype, a.dtype)
        view.view(self.torch.uint8).reshape(-1).copy_(self.torch.from_numpy(raw))
        return view

    def refill(self, view, value=None):
        """poison (or `value`) into a carving again, between two calls that write it"""
        view.view(self.torch.uint8).fill_(self.poison if value is None else value)

    def host(self):
        if self.bytes.device.type == 'cuda':
            self.torch.cuda.synchronize()
        return self.bytes.cpu().numpy().copy()

    def snapshot(self):
        self.before = self.host()

    def span(self, view):
        """(start, end) of a contiguous view into the arena"""
        assert view.is_contiguous()
        if view.numel() == 0:  # (nothing may be written: an empty view has no address to speak of)
            return 0, 0
        start = view.data_ptr() - self.base
        end = start + view.numel() * view.element_size()
        assert 0 <= start <= end <= self.bytes.numel(), 'not a view of this arena'
        return start, end

    def check(self, written=(), what=''):
        """every byte outside the views in `written` equals the last snapshot()"""
        assert self.before is not None, 'snapshot() first'
        after = self.host()
        at = first_change(self.before, after, [self.span(v) for v in written])
        assert at is None, '%s: %s' % (what, describe(at, self.carvings, self.before, after))
        return after


def bits_of(a):
    """a host array as unsigned words of its item size: what host_of gives for the device's"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.itemsize])


def run_guarded(nbytes, setup, what, poisons=(0xFF, 0x00)):
    """One case at every poison.  setup(arena) carves and places what the call takes and returns (call, outputs): call() is the
    entry point under test, outputs a list of (name, view, want) -- the extents it may write and the expected values there (want
    None: only the extent is checked).  After call() every byte of the arena outside the outputs must equal the snapshot taken just
    before it, every output must equal `want` bit for bit, and the outputs of the runs must equal each other."""
    runs = []
    for poison in poisons:
        arena = Arena(nbytes, poison)
        call, outputs = setup(arena)
        arena.snapshot()
        call()
        tag = '%s, poison 0x%02X' % (what, poison)
        arena.check(written=[view for _, view, _ in outputs], what=tag)
        got = [host_of(view) for _, view, _ in outputs]
        for (name, view, want), g in zip(outputs, got):
            if want is not None:
                w = bits_of(want)
                if g.dtype != w.dtype:  # (records in a byte view: compared as bytes)
                    g, w = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
                assert g.size == w.size, (tag, name, g.shape, w.shape)
                w = w.reshape(g.shape)
                bad = g != w
                assert not bad.any(), '%s: %s differs from the reference at %d elements, first at %s: 0x%X, expected 0x%X' % (
                    tag, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), g[bad][0], w[bad][0])
        runs.append([g for (_, _, want), g in zip(outputs, got) if want is not None])
    for first, other in zip(runs[0], runs[-1]):
        assert np.array_equal(first, other), '%s: the outputs depend on the poison' % what


def host_of(view):
    """a carving's bytes on the host, as a numpy array of the view's shape (uint8 views) or its dtype's bits"""
    import torch
    names = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.int32: np.uint32, torch.float32: np.uint32}
    for n in ('uint16', 'uint32'):
        if hasattr(torch, n):
            names[getattr(torch, n)] = getattr(np, n)
    return view.contiguous().view(torch.uint8).cpu().numpy().view(names[view.dtype]).reshape(tuple(view.shape)).copy()
