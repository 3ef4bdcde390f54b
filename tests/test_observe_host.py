"""CPU: the observation contract (include/rdoom.h: rdoom_batch_resolve_observation) as tests/observe_ref.py restates it, pinned on
hand-made arrays, and the surface the feature adds -- header, exported symbols, the Python mirror's constants and shapes."""
import ctypes
import os
import re

import numpy as np
import pytest

import observe_ref as oref
import rust_doom_amd as rd
from util import ROOT

HEADER = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
CLEAR = (15, 18, 23)


def frame(h, w, value=0):
    return np.full((1, h, w, 3), value, np.uint8)


def test_a_mean_of_exactly_one_half_rounds_up():
    rgb = frame(8, 8)
    rgb[0, 0:2, 0:2, 0] = [[1, 2], [1, 2]]         # sum 6 of 4: 1.5 -> 2
    rgb[0, 0:2, 0:2, 1] = [[1, 1], [1, 2]]         # sum 5 of 4: 1.25 -> 1
    rgb[0, 0:2, 0:2, 2] = [[255, 255], [255, 254]]  # sum 1019 of 4: 254.75 -> 255
    rgb[0, 0, 2:4, 0] = [7, 0]                     # cell (1, 0) at (2, 1): sum 7 of 2: 3.5 -> 4
    got = oref.mean_rgb(rgb, 2)
    assert got.shape == (1, 4, 4, 3) and got.dtype == np.uint8
    assert got[0, 0, 0].tolist() == [2, 1, 255]
    assert oref.mean_rgb(rgb, (2, 1))[0, 0, 1, 0] == 4
    assert oref.mean_rgb(rgb, 1).tolist() == rgb.tolist()  # factor 1 is the frame itself
    full = oref.mean_rgb(frame(8, 8, 255), 8)
    assert full.shape == (1, 1, 1, 3) and (full == 255).all()  # 64 * 255: no overflow, no rounding past 255


def test_grey_of_white_and_of_the_clear_colour():
    assert (oref.gray(frame(8, 8, 255), 4) == 255).all()
    clear = frame(8, 8)
    clear[...] = CLEAR
    want = (77 * 15 + 150 * 18 + 29 * 23 + 128) // 256
    assert want == 18
    for f in (1, 2, 8, (4, 2)):
        assert (oref.gray(clear, f) == want).all(), f
    # the sums are weighted, not the rounded means: (3, 0, 0) and (0, 0, 0) side by side
    two = frame(8, 8)
    two[0, 0, 0] = (3, 0, 0)
    assert oref.gray(two, (2, 1))[0, 0, 0] == (77 * 3 + 128 * 2) // 512


def test_depth_takes_the_smallest_finite_value_and_never_a_nan():
    d = np.full((1, 8, 8), np.inf, np.float32)
    d[0, 1, 1] = 5.0                       # one finite depth in a sky cell
    d[0, 0, 4], d[0, 1, 4] = np.nan, 7.0   # a NaN beside a finite depth
    d[0, 4, 0] = np.nan                    # a NaN beside +inf only
    got = oref.depth_min(d, 2)
    assert got.dtype == np.float32 and got.shape == (1, 4, 4)
    assert got[0, 0, 0] == 5.0 and got[0, 0, 2] == 7.0
    assert np.isposinf(got[0, 2, 0]) and np.isposinf(got[0, 3, 3])  # never a NaN; an all-sky cell stays +inf
    assert not np.isnan(got).any()
    d[0, 0, 0] = 2.5
    assert oref.depth_min(d, 8)[0, 0, 0] == 2.5


def test_leftover_columns_and_rows_belong_to_no_cell():
    rgb = np.arange(7 * 5 * 3, dtype=np.uint8).reshape(1, 5, 7, 3)
    got = oref.mean_rgb(rgb, (2, 4))
    assert got.shape == (1, 1, 3, 3)
    loud = rgb.copy()
    loud[0, 4, :] = 255  # the top row
    loud[0, :, 6] = 255  # the right column
    assert np.array_equal(oref.mean_rgb(loud, (2, 4)), got)
    s = rgb[0, 0:4, 2:4].astype(np.uint32).sum((0, 1))
    assert got[0, 0, 1].tolist() == ((2 * s + 8) // 16).tolist()
    d = np.arange(35, dtype=np.float32).reshape(1, 5, 7)
    assert oref.depth_min(d, (2, 4)).tolist() == [[[0.0, 2.0, 4.0]]]


def test_top_down_reverses_the_rows_only():
    rng = np.random.RandomState(1)
    rgb = rng.randint(0, 256, (2, 8, 8, 3)).astype(np.uint8)
    d = rng.rand(2, 8, 8).astype(np.float32)
    for fmt in (oref.OBS_RGB8, oref.OBS_GRAY8, oref.OBS_DEPTH_MIN):
        up = oref.observation(fmt, (4, 2), rgb, d)
        down = oref.observation(fmt, (4, 2), rgb, d, top_down=True)
        assert np.array_equal(down, up[:, ::-1]) and not np.array_equal(down, up)
    # the cells stay where they are: flipping the INPUT of 7 rows is something else (row 6 is the leftover, not row 0)
    odd = rng.randint(0, 256, (1, 7, 8, 3)).astype(np.uint8)
    assert not np.array_equal(oref.mean_rgb(odd, 2)[:, ::-1], oref.mean_rgb(odd[:, ::-1], 2))
    planar = oref.observation(oref.OBS_RGB8_PLANAR, 2, rgb, top_down=True)
    assert planar.shape == (2, 3, 4, 4)
    assert np.array_equal(planar, np.moveaxis(oref.observation(oref.OBS_RGB8, 2, rgb, top_down=True), 3, 1))


# ---- the surface: these fail without the feature -----------------------------------------------------------------------------
def header_value(name):
    m = re.search(r'^#define\s+RDOOM_%s\s+(\d+)u' % name, HEADER, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_declares_the_entry_points_and_formats():
    text = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
    for fn in ('rdoom_batch_resolve_observation', 'rdoom_batch_read_observation'):
        m = re.search(r'rdoom_status\s+%s\s*\(([^)]*)\)' % fn, text)
        assert m, fn
        args = ' '.join(m.group(1).split())
        assert args.startswith('rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t format, uint32_t fx, uint32_t fy, void *'), args
    values = [header_value(n) for n in ('OBS_RGB8', 'OBS_RGB8_PLANAR', 'OBS_GRAY8', 'OBS_DEPTH_MIN')]
    assert len(set(values)) == 4 and all(0 < v < 0x100 for v in values)  # (RDOOM_RGB_TOP_DOWN is or-ed in above the low byte)


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(rd.LIB_PATH)
    for fn in ('rdoom_batch_resolve_observation', 'rdoom_batch_read_observation'):
        assert hasattr(lib, fn) and fn in rd.API_SYMBOLS, fn


def test_python_constants_equal_the_headers():
    for name in ('OBS_RGB8', 'OBS_RGB8_PLANAR', 'OBS_GRAY8', 'OBS_DEPTH_MIN'):
        assert getattr(rd, name) == header_value(name) == getattr(oref, name), name


def test_observation_shape_follows_the_contract():
    assert rd.observation_shape(rd.OBS_RGB8, 640, 400, 4) == (100, 160, 3)
    assert rd.observation_shape(rd.OBS_RGB8_PLANAR, 640, 400, 4) == (3, 100, 160)
    assert rd.observation_shape(rd.OBS_GRAY8, 321, 200, 8) == (25, 40)
    assert rd.observation_shape(rd.OBS_DEPTH_MIN, 321, 200, (4, 8)) == (25, 80)
    assert rd.observation_shape(rd.OBS_RGB8_PLANAR, 77, 53, (1, 4)) == (3, 13, 77)
    assert rd.observation_shape(rd.OBS_GRAY8, 1920, 1080, 1) == (1080, 1920)
    for fmt in (rd.OBS_RGB8, rd.OBS_RGB8_PLANAR, rd.OBS_GRAY8, rd.OBS_DEPTH_MIN):
        for factor in (1, 2, (8, 2), (1, 4)):
            assert rd.observation_shape(fmt, 77, 53, factor) == oref.shape(fmt, 77, 53, factor)
    for bad in (3, 16, 0, (4, 3), (16, 1)):
        with pytest.raises(ValueError):
            rd.observation_shape(rd.OBS_RGB8, 640, 400, bad)
    with pytest.raises(ValueError):
        rd.observation_shape(7, 640, 400, 4)
    with pytest.raises(ValueError):
        rd.observation_shape(rd.OBS_GRAY8, 7, 400, 8)  # ow == 0
