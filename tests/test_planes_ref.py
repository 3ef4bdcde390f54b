"""tests/planes_ref.py (the oracle composition the GPU tests compare the planes with) against itself, on the CPU."""
import json
import os

import numpy as np

import planes_ref
from oracle import raster
from util import GOLDEN


def test_the_composition_is_consistent_on_a_golden_pose(oracle_levels):
    lv = oracle_levels(0)
    g = json.load(open(os.path.join(GOLDEN, 'digests.json')))
    row = np.load(os.path.join(GOLDEN, 'poses.npy'))[0][0]
    pose = {'modelview': row[:16], 'projection': row[16:32], 'time': row[32]}
    w, h = g['width'], g['height']
    ro = raster.RasterOracle(lv)
    want = planes_ref.expected_planes(ro, lv, pose, lv.lights.fill_buffer_at(float(row[32])), w, h)
    prim, depth, label = want['primitive'], want['depth'], want['label']
    assert prim.dtype == np.uint32 and depth.dtype == np.float32 and label.dtype == np.uint16 and depth.shape == (h, w)
    kind, obj, owner = planes_ref.draw_tables(lv)
    draws = np.asarray(lv.draws).reshape(-1, 4)
    drawn = prim != planes_ref.NO_PRIM
    assert drawn.any()
    pk = np.where(drawn, kind[np.where(drawn, prim, 0)], 99)
    solid = drawn & (pk != planes_ref.KIND_SKY)
    assert solid.any()
    # every pixel with a non-sky winner has a finite positive depth, every other pixel +inf
    assert np.isfinite(depth[solid]).all() and (depth[solid] > 0).all()
    assert np.isposinf(depth[~solid]).all()
    # the label's kind is the kind of the draw that owns the oracle's primitive id, its object that draw's object
    own = owner[prim[drawn]]
    assert np.array_equal(label[drawn] & 0xF, draws[own, 0]) and np.array_equal(label[drawn] >> 4, draws[own, 1])
    assert (label[~drawn] == planes_ref.LABEL_NONE).all() and (label[drawn] != planes_ref.LABEL_NONE).all()
    # primitive ids are positions in draw order
    assert int(prim[drawn].max()) < int(draws[:, 3].sum()) // 3 == len(kind)
