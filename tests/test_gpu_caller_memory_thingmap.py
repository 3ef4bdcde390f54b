"""GPU: WHERE rdoom_thingset_draw_maps writes.  Every array -- states, level slots and the hidden and known rows going in, the byte
plane and the index plane coming out -- is a carving of a guarded arena (tests/guarded.py) at the least alignment the header allows:
the bytes at 1 and 3 mod 16, everything else at 4 and 12 mod 16.  After the call every byte outside the outputs, the inputs
included, must be what it was, and the outputs must equal tests/thingmap_ref.py byte for byte and index for index, with the arena
poisoned 0xFF and 0x00.  Tables of 33 things (two words, one bit in the second) and 257 (a second stride of one thing), three
players a launch at 77 x 53 (three tiles by two, the last column 13 pixels wide), with and without RDOOM_THING_MARKS_OVER."""
import functools

import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import rust_doom_amd as rd
import things_ref
import thingmap_ref
from guarded import GUARD, run_guarded
from util import META_PATH, ensure_wad

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
N = 3
VIEW = thingmap_ref.view_of(77, 53, 0.12, rotate=True)
SHAPE = (N, 53, 77)


@functools.lru_cache(maxsize=None)
def case(size):
    """computed once and left unchanged: the tables of two levels, three players next to things of theirs in slots 1, 0 and 5, rows
    in which a quarter of the things are hidden and three quarters known, the bytes an overlay finds, and the reference's results"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    hosts = [wad.build_world(i, device=False) for i in (0, 2)]
    rng = np.random.default_rng(900 + size)
    tables = [things_ref.make_table(rng, size if k == 0 else 40, things_ref.bounds_of(h.map_lines()),
                                    np.stack([h.map_things()['x'], h.map_things()['z']], 1)) for k, h in enumerate(hosts)]
    words = things_ref.set_words(tables)
    rand = lambda: rng.integers(0, 1 << 32, (N, words), dtype=np.uint64).astype(U)
    hidden, known = rand() & rand(), rand() | rand()
    lv = np.array([1, 0, 5], U)
    st = np.concatenate([things_ref.players_near(tables[min(int(s), 1)], 1, rng, spread=0.25) for s in lv])
    before = rng.integers(0, 16, SHAPE).astype(np.uint8)
    want = {over: thingmap_ref.draw(tables, st, VIEW, levels=lv, hidden=hidden, known=known, over=before if over else None)
            for over in (False, True)}
    return dict(tables=tables, words=words, hidden=hidden, known=known, levels=lv, states=st, before=before, want=want)


@pytest.mark.parametrize('over', [False, True])
@pytest.mark.parametrize('size', [33, 257])
@pytest.mark.parametrize('residue', [(1, 4), (3, 12)])
def test_thingset_draw_maps(residue, size, over):
    rd.set_device(0)
    c = case(size)
    out_want, index_want, _ = c['want'][over]
    assert (index_want[:2].reshape(2, -1).max(1) >= 0).all() and (index_want[2] == -1).all()  # slot 5 is outside the set
    assert (out_want[2] == (c['before'][2] if over else 0)).all()
    things = rd.DeviceThings(c['tables'])
    assert things.words() == c['words'] == (size + 31) // 32

    def setup(arena):
        at, other = residue[1], 16 - residue[1]
        s = arena.place(c['states'], 16, at, 'states')
        lv = arena.place(c['levels'].view(np.int32), 16, other, 'levels', torch.int32)
        hid = arena.place(c['hidden'].view(np.int32), 16, at, 'hidden', torch.int32)
        kno = arena.place(c['known'].view(np.int32), 16, other, 'known', torch.int32)
        out = arena.place(c['before'], 16, residue[0], 'out', torch.uint8)  # what an overlay finds; written whole without OVER
        index = arena.carve(SHAPE, torch.int32, 16, at, 'index_out')
        assert {t.data_ptr() % 16 for t in (s, lv, hid, kno, index)} == {4, 12} and out.data_ptr() % 16 == residue[0]
        call = lambda: things.draw_maps(s, 77, 53, 0.12, levels=lv, hidden=hid, known=kno, rotate=True, over=over, out=out, index_out=index)
        return call, [('out', out, out_want), ('index', index, index_want)]
    run_guarded(16 * (GUARD + 4096), setup, 'thing maps of %d at %s, over=%s' % (size, residue, over))
    things.close()
