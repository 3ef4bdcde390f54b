"""GPU: WHERE the batch resolves write (rdoom_batch_resolve_rgb / _plane / _observation).  Every output is a carving of a guarded
arena (tests/guarded.py) at a pointer the header allows and an ordinary allocation never has -- bytes at 1, 2, 3 mod 16, 16-bit
elements at 2 and 6, 32-bit ones at 4 and 12 (and at 0, the other side of every alignment branch) -- holding exactly the two
frames of first=1, count=2.  After the call every byte of the arena outside the carving must be what it was, and the carving must
hold the ORACLE's frames bit for bit (test_gpu_rgb.compose, planes_ref, observe_ref), with the arena poisoned 0xFF and again 0x00.
E1M1, three poses (the last from outside the level), rendered after util.dirtying_poses, plain path and id path."""
import numpy as np
import pytest

try:  # before the library is loaded: torch and the library then share one HIP runtime, as in bench.py
    import torch
except ImportError:
    torch = None

import observe_ref as oref
import planes_ref
import rust_doom_amd as rd
from guarded import GUARD, run_guarded
from test_gpu_rgb import compose, oracle_frames, outside_pose
from util import dirtying_poses

pytestmark = pytest.mark.gpu
# 96 x 40: three quadrants across (the workgroup's fourth wave is idle), a second quadrant row of 8 rows, a width that is a
# multiple of 4 and of 16; 77 x 53: tails both ways, rows that change their alignment
SIZES = [(96, 40), (77, 53)]
FIRST, COUNT = 1, 2
_scenes = {}


def scene(oracle_levels, size, ids):
    """the rendered batch and the oracle's frames of it, once per size and path"""
    rd.set_device(0)
    w, h = size
    if size not in _scenes:
        from test_gpu_raster_parity import sweep_poses
        lv = oracle_levels(0)
        poses = sweep_poses(lv, 2, w, h, seed=31, time=0.7)
        poses = np.concatenate([poses, outside_pose(lv, w, h, float(poses[0]['time']))])
        lights = np.array([lv.lights.fill_buffer_at(float(p['time'])) for p in poses])
        fb, prim = oracle_frames(lv, poses, lights, w, h)
        assert (prim[FIRST:] == 0xFFFFFFFF).any() and (prim[FIRST:] != 0xFFFFFFFF).any()  # drawn and undrawn pixels
        planes = planes_ref.expected_batch(lv, poses, lights, w, h)
        _scenes[size] = {'lv': lv, 'poses': poses, 'lights': lights, 'fb': fb, 'prim': prim, 'planes': planes,
                         'rgb': compose(fb, prim, lv.palette), 'batches': {}}
    s = _scenes[size]
    if ids not in s['batches']:
        batch = rd.Batch(rd.DeviceLevel(s['lv']), w, h, len(s['poses']))
        if ids:
            batch.enable_primitive_ids()
        batch.render(dirtying_poses(s['poses']), np.roll(s['lights'], 1, axis=0))
        batch.render(s['poses'], s['lights'])
        batch.finish()
        s['batches'][ids] = batch
    return s, s['batches'][ids]


def guarded_call(shape, dtype, residue, want, call, what):
    """`call(out)` into a carving of `shape` at `residue` mod 16, at both poisons: nothing outside it changes, it holds `want`"""
    def setup(arena):
        out = arena.carve(shape, dtype, 16, residue, name='device_out')
        assert out.data_ptr() % 16 == residue and out.numel() * out.element_size() == want.nbytes
        return (lambda: call(out)), [('device_out', out, want)]
    run_guarded(want.nbytes + 2 * GUARD + 64, setup, what)


@pytest.mark.parametrize('ids', [False, True], ids=['plain', 'ids'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_resolve_rgb(oracle_levels, size, ids):
    """resolve.hip's `dword` both ways: RGBA8 off a dword boundary is store_run<4>'s per-pixel path, RGB8 of a width that is a
    multiple of 4 takes the per-pixel path only when the pointer does"""
    s, batch = scene(oracle_levels, size, ids)
    w, h = size
    seen = set()
    for alpha in (False, True):
        for residue in (0, 1, 2, 3):
            for td in (False, True):
                want = np.ascontiguousarray(compose(s['fb'][FIRST:], s['prim'][FIRST:], s['lv'].palette, alpha, td))
                shape = (COUNT, h, w, 4 if alpha else 3)

                def call(out):
                    dword = out.data_ptr() % 4 == 0 and (alpha or w % 4 == 0)  # the kernel's own condition, on the host
                    assert dword == (residue == 0 and (alpha or w % 4 == 0))
                    seen.add((alpha, dword))
                    batch.resolve_rgb(out, FIRST, COUNT, alpha=alpha, top_down=td)
                guarded_call(shape, torch.uint8, residue, want, call, 'rgb %dx%d alpha=%s residue %d top_down=%s' % (w, h, alpha, residue, td))
    assert (True, True) in seen and (True, False) in seen and (False, False) in seen  # RGBA both ways, RGB8 per pixel
    assert ((False, True) in seen) == (w % 4 == 0)                                   # RGB8 packed, and at 96 wide unpacked by the pointer alone


@pytest.mark.parametrize('ids', [False, True], ids=['plain', 'ids'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_resolve_plane(oracle_levels, size, ids):
    """planes.hip's `dword` for the 16-bit label plane both ways at an even width (0 against 2 and 6 mod 16); depth and primitive
    rows at 4 and 12 mod 16, never 16-byte aligned"""
    s, batch = scene(oracle_levels, size, ids)
    w, h = size
    seen = set()
    cases = [('label', rd.PLANE_LABEL, torch.int16, (0, 2, 6)), ('depth', rd.PLANE_DEPTH, torch.float32, (4, 12)),
             ('primitive', rd.PLANE_PRIMITIVE, torch.int32, (4, 12))]
    for name, plane, dtype, residues in cases:
        for residue in residues:
            for td in (False, True):
                want = s['planes'][name][FIRST:]
                want = np.ascontiguousarray(want[:, ::-1] if td else want)

                def call(out):
                    if name == 'label':
                        dword = out.data_ptr() % 4 == 0 and w % 2 == 0
                        assert dword == (residue == 0 and w % 2 == 0)
                        seen.add(dword)
                    else:
                        assert out.data_ptr() % 4 == 0 and out.data_ptr() % 16 != 0
                    batch.resolve_plane(out, plane, FIRST, COUNT, top_down=td)
                guarded_call((COUNT, h, w), dtype, residue, want, call, '%s %dx%d residue %d top_down=%s' % (name, w, h, residue, td))
    assert False in seen and ((True in seen) == (w % 2 == 0))


@pytest.mark.parametrize('ids', [False, True], ids=['plain', 'ids'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_resolve_observation(oracle_levels, size, ids):
    """observe.hip's store_bytes packs a run into dwords when its address is dword aligned: with the base at 1, 2 or 3 mod 4 the
    rows that packed at an aligned base no longer do, and the other way round; store_words' 8- and 16-byte stores at 4 and 12"""
    s, batch = scene(oracle_levels, size, ids)
    w, h = size
    rgb, depth = s['rgb'][FIRST:], s['planes']['depth'][FIRST:]
    row_starts = set()
    for factor in ((4, 4), (8, 2), (1, 4)):
        for fmt in (rd.OBS_GRAY8, rd.OBS_RGB8, rd.OBS_RGB8_PLANAR, rd.OBS_DEPTH_MIN):
            shape = (COUNT,) + rd.observation_shape(fmt, w, h, factor)
            ow = w // factor[0]
            row_bytes = ow * (3 if fmt == rd.OBS_RGB8 else 1)
            for residue in ((4, 12) if fmt == rd.OBS_DEPTH_MIN else (0, 1, 2, 3)):
                for td in (False, True):
                    want = oref.observation(fmt, factor, rgb, depth, td)
                    assert want.shape == shape

                    def call(out):
                        if fmt == rd.OBS_DEPTH_MIN:
                            assert out.data_ptr() % 4 == 0 and out.data_ptr() % 16 != 0
                        else:  # the alignments the rows of this output start at
                            starts = {(out.data_ptr() + r * row_bytes) % 4 for r in range(out.numel() // row_bytes)}
                            assert residue in starts and (residue == 0 or starts != {0})
                            row_starts.update(starts)
                        batch.resolve_observation(out, fmt, factor, FIRST, COUNT, top_down=td)
                    guarded_call(shape, torch.float32 if fmt == rd.OBS_DEPTH_MIN else torch.uint8, residue, want, call,
                                 'observation %d %r %dx%d residue %d top_down=%s' % (fmt, factor, w, h, residue, td))
    assert row_starts == {0, 1, 2, 3}  # store_bytes' condition was met and missed
