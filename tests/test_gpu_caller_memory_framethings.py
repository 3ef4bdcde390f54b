"""GPU: WHERE rdoom_frame_things writes.  The ids, the depth, the table and the bit rows are carvings of a guarded arena
(tests/guarded.py) at the least alignment the header allows, 4 and 12 mod 16.  After the call every byte outside the table and the
bit rows, the inputs included, must be what it was, and the outputs must equal tests/framethings_ref.py's reduction bit for bit, with
the arena poisoned 0xFF and 0x00.  Widths with and without a tail of ids, 33 records (two words, one bit in the second), rows of
bits two words wider than the records need, and the call without depth and without bits."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import framethings_ref as fr
import rust_doom_amd as rd
from guarded import GUARD, run_guarded

pytestmark = pytest.mark.gpu
N, H, MAX_THINGS, MIN_PIXELS = 2, 33, 33, 2


@functools.lru_cache(maxsize=None)
def case(width, stride):
    """computed once and left unchanged: ids in [-2, MAX_THINGS + 2], a depth plane with +inf, -1, NaN and 0, and the reduction"""
    rng = np.random.default_rng(340 + width)
    ids = rng.integers(-2, MAX_THINGS + 3, (N, H, width)).astype(np.int32)
    depth = fr.synthetic_depth(rng, (N, H, width))
    with_depth = fr.reduce(ids, depth, MAX_THINGS, MIN_PIXELS, stride)
    without = fr.reduce(ids, None, MAX_THINGS, MIN_PIXELS, stride)
    return dict(ids=ids, depth=depth, with_depth=with_depth, without=without)


@pytest.mark.parametrize('use_depth,use_bits', [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize('width,stride', [(64, 2), (65, 4), (3, 2)])
@pytest.mark.parametrize('residue', [4, 12])
def test_frame_things(residue, width, stride, use_depth, use_bits):
    rd.set_device(0)
    c = case(width, stride)
    want_t, want_b = c['with_depth'] if use_depth else c['without']
    assert (want_t['count'] > 0).all() or width == 3

    def setup(arena):
        at, other = residue, 16 - residue
        ids = arena.place(c['ids'], 16, at, 'ids', torch.int32)
        depth = arena.place(c['depth'], 16, other, 'depth', torch.float32)
        table = arena.carve((N, MAX_THINGS, 6), torch.int32, 16, other, 'table')
        bits = arena.carve((N, stride), torch.int32, 16, at, 'bits')
        assert {t.data_ptr() % 16 for t in (ids, depth, table, bits)} == {4, 12}
        call = lambda: rd.frame_things(ids, depth if use_depth else None, max_things=MAX_THINGS, min_pixels=MIN_PIXELS, table_out=table,
                                       bits_out=bits if use_bits else False)
        outputs = [('table', table, fr.as_words(want_t))]
        if use_bits:
            outputs.append(('bits', bits, want_b))
        return call, outputs
    run_guarded(8 * (2 * GUARD + 4096) + 4 * N * H * width * 4, setup,
                'frame_things %d wide at %d mod 16, depth=%s, bits=%s' % (width, residue, use_depth, use_bits))
