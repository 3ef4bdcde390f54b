"""CPU: the guarded arena of tests/guarded.py does what the caller-memory GPU tests rely on -- a byte changed just before an
output, just after it or inside an input is reported at its offset with the right distance; a byte inside an output is not --
and carve() places views at the residue asked for, with a guard band on either side."""
import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

import guarded

needs_torch = pytest.mark.skipif(torch is None, reason='the arena is a torch tensor')

CARVINGS = [guarded.Carving('input', 4096, 4096 + 100), guarded.Carving('output', 8300, 8300 + 77)]
SIZE = 8300 + 77 + 4096


def changed_at(offset, written):
    before = np.full(SIZE, 0xFF, np.uint8)
    after = before.copy()
    after[offset] = 0x12
    at = guarded.first_change(before, after, written)
    return at, (None if at is None else guarded.describe(at, CARVINGS, before, after))


def test_a_byte_just_before_an_output_is_reported():
    out = CARVINGS[1]
    at, text = changed_at(out.start - 1, [(out.start, out.end)])
    assert at == out.start - 1
    assert "-1 from the start of 'output'" in text and '0xFF -> 0x12' in text, text


def test_a_byte_just_after_an_output_is_reported():
    out = CARVINGS[1]
    at, text = changed_at(out.end, [(out.start, out.end)])
    assert at == out.end
    assert "+0 from the end of 'output'" in text and '0xFF -> 0x12' in text, text
    at, text = changed_at(out.end + 5, [(out.start, out.end)])
    assert at == out.end + 5 and "+5 from the end of 'output'" in text, text


def test_a_byte_inside_an_input_is_reported():
    inp, out = CARVINGS
    at, text = changed_at(inp.start + 40, [(out.start, out.end)])
    assert at == inp.start + 40
    assert "at byte 40 inside 'input'" in text, text


def test_a_byte_inside_an_output_is_not_reported():
    out = CARVINGS[1]
    for offset in (out.start, out.start + 33, out.end - 1):
        assert changed_at(offset, [(out.start, out.end)]) == (None, None)
    # ... and is, when the call was allowed a sub-range only
    at, text = changed_at(out.start + 33, [(out.start, out.start + 33)])
    assert at == out.start + 33 and "at byte 33 inside 'output'" in text, text


def test_the_first_of_several_changes_is_the_one_reported():
    before = np.zeros(SIZE, np.uint8)
    after = before.copy()
    after[[9000, 5000, 8290]] = 1
    assert guarded.first_change(before, after, [(8300, 8377)]) == 5000
    assert guarded.first_change(before, after, [(4096, 8377)]) == 9000
    assert guarded.first_change(before, before.copy(), []) is None


def test_place_offset_arithmetic():
    for base in (0, 512, 7, 4099):
        for cursor in (0, 1, 4095, 10000):
            for align, residue, item in ((16, 1, 1), (16, 2, 1), (16, 3, 1), (16, 2, 2), (16, 6, 2), (16, 4, 4), (16, 12, 4), (32, 16, 4),
                                         (4, 1, 1), (4, 2, 2)):
                off = guarded.place_offset(base, cursor, align, residue, item)
                assert (base + off) % align == residue and cursor + guarded.GUARD <= off < cursor + guarded.GUARD + align
    for align, residue, item in ((16, 1, 2), (16, 2, 4), (16, 6, 4), (16, 16, 1), (12, 4, 4), (2, 0, 4), (16, -4, 4)):
        with pytest.raises(ValueError):
            guarded.place_offset(0, 0, align, residue, item)


@needs_torch
def test_carve_on_a_cpu_tensor():
    arena = guarded.Arena(64 * 1024, 0xFF, device='cpu')
    a = arena.carve((3, 5), torch.uint8, 16, 3, name='a')
    b = arena.carve((7,), torch.int16, 16, 6, name='b')
    c = arena.carve((2, 2), torch.float32, 16, 12, name='c')
    d = arena.place(np.arange(10, dtype=np.int32), 32, 16, name='d', dtype=torch.int32)
    e = arena.place(np.arange(6, dtype=np.float32), 16, 4, name='e')
    assert [v.data_ptr() % 16 for v in (a, b, c, e)] == [3, 6, 12, 4] and d.data_ptr() % 32 == 16
    assert a.shape == (3, 5) and b.dtype == torch.int16 and c.is_contiguous() and e.dtype == torch.uint8 and e.numel() == 24
    assert d.tolist() == list(range(10)) and np.array_equal(guarded.host_of(e).view(np.float32), np.arange(6, dtype=np.float32))
    assert torch.isnan(c).all() and (b == -1).all()  # 0xFF: a NaN as float32, -1 as an integer
    spans = [arena.span(v) for v in (a, b, c, d, e)]
    assert spans == [(k.start, k.end) for k in arena.carvings] and [k.name for k in arena.carvings] == list('abcde')
    assert spans[0][0] >= guarded.GUARD and spans[-1][1] + guarded.GUARD <= arena.bytes.numel()
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert start - end >= guarded.GUARD
    with pytest.raises(ValueError):  # a residue the dtype cannot have
        arena.carve((4,), torch.float32, 16, 2)
    with pytest.raises(ValueError):  # no room left for the carving and its guard band
        arena.carve((64 * 1024,), torch.uint8, 16, 1)
    assert len(arena.carvings) == 5

    # check(): against the snapshot, outside the written views
    arena.snapshot()
    a.fill_(7)
    c[0, 0] = 1.0
    arena.check(written=[a, c], what='both written')
    arena.check(written=[a, c[:1]], what='the first row of c')
    with pytest.raises(AssertionError) as err:
        arena.check(written=[a], what='c changed')
    assert "at byte 0 inside 'c'" in str(err.value)
    arena.snapshot()
    arena.bytes[spans[1][1]] = 0  # the byte behind b
    with pytest.raises(AssertionError) as err:
        arena.check(written=[b], what='behind b')
    assert "+0 from the end of 'b'" in str(err.value) and '0xFF -> 0x00' in str(err.value)
    arena.snapshot()
    arena.bytes[spans[3][0] - 1] = 0  # the byte in front of d
    with pytest.raises(AssertionError) as err:
        arena.check(written=[d], what='in front of d')
    assert "-1 from the start of 'd'" in str(err.value)
    arena.snapshot()
    d[3] = 99  # an input
    with pytest.raises(AssertionError) as err:
        arena.check(written=[a, b, c], what='input d')
    assert "at byte 12 inside 'd'" in str(err.value)
