"""GPU: WHAT a render reads of the rows given to rdoom_batch_set_hidden_things, and that it writes none of it.  The rows are a
carving of a guarded arena (tests/guarded.py) at the least alignment the header allows, 4 and 12 mod 16, with the arena poisoned
0xFF and 0x00: a word read in front of the rows, behind them or beyond a row's stride would hide everything under one poison and
nothing under the other, so the frames -- held against the oracle on the twins of tests/hidden_ref.py -- must be what the rows
alone say under both, and every byte of the arena, the rows included, must be what it was."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import hidden_ref
import rust_doom_amd as rd
from guarded import GUARD, Arena
from oracle import raster
from util import META_PATH, ensure_wad

pytestmark = pytest.mark.gpu
U = np.uint32
W, H, N = 320, 200, 5


@functools.lru_cache(maxsize=None)
def case(stride):
    """computed once and left unchanged: E1M1, five poses that face things, rows of `stride` words, and the oracle's frames of the
    twins.  One word: the quads of things 32 and above are beyond the row, where the arena's poison lies"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    arrays, table, lights = built.arrays(), built.decor_things(), built.lights_at(0.0)
    things = wad.build_world(0, device=False).map_things()
    late = [int(i) for i in table if i >= 32]
    assert late
    poses = np.zeros(N, rd.POSE)
    for p in range(N):
        t = things[late[p % len(late)] if p % 2 else int(table[3 * p])]
        a = 1.3 * p
        eye = np.array([t['x'] + 0.9 * np.cos(a), t['base'] + 0.45, t['z'] + 0.9 * np.sin(a)])
        d = np.array([t['x'], t['base'] + 0.2, t['z']]) - eye
        poses[p] = rd.pose_look(tuple(float(x) for x in eye), float(np.arctan2(-d[0], -d[2])), float(np.arctan2(d[1], np.hypot(d[0], d[2]))), W, H, 0.0)
    rows = np.random.default_rng(41 + stride).integers(0, 1 << 32, (N, stride), dtype=np.uint64).astype(U)
    fbs, prims = [], []
    for p in range(N):
        tw = hidden_ref.twin(arrays, hidden_ref.hidden_quads(rows[p], table))
        fb, prim = raster.RasterOracle(tw).render(poses[p]['modelview'], poses[p]['projection'], 0.0, lights, W, H, want_prim=True)
        fbs.append(fb), prims.append(prim)
    base = [raster.RasterOracle(arrays).render(poses[p]['modelview'], poses[p]['projection'], 0.0, lights, W, H) for p in range(N)]
    assert sum((b != f).any() for b, f in zip(base, fbs)) >= 2  # the rows matter
    return dict(built=built, poses=poses, lights=lights, rows=rows, fb=np.stack(fbs), prim=np.stack(prims))


@pytest.mark.parametrize('stride', [1, 2, 3])
@pytest.mark.parametrize('residue', [4, 12])
def test_a_render_reads_the_rows_and_nothing_around_them(stride, residue):
    rd.set_device(0)
    c = case(stride)
    level = rd.DeviceLevel(c['built'])
    batch = rd.Batch(level, W, H, N)
    batch.enable_primitive_ids()
    for poison in (0xFF, 0x00):
        arena = Arena(4 * (GUARD + 256), poison)
        rows = arena.place(c['rows'].view(np.int32), 16, residue, 'hidden rows', torch.int32)
        assert rows.data_ptr() % 16 == residue and tuple(rows.shape) == (N, stride)
        arena.snapshot()
        batch.set_hidden_things(rows)
        batch.render(c['poses'], c['lights'])
        fb, prim = batch.read_framebuffer(), batch.read_primitive_ids()
        batch.set_hidden_things(None)
        arena.check(written=[], what='hidden rows of %d words at %d, poison 0x%02X' % (stride, residue, poison))  # nothing is written
        assert np.array_equal(fb, c['fb']) and np.array_equal(prim, c['prim']), (stride, residue, poison)
