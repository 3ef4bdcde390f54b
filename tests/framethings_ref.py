"""Things in the frame (include/rdoom_frame_things.h) restated for the tests, composed from the ORACLE only (never from the
product's own output): the thing plane from the oracle's winners (RasterOracle.render(..., want_prim=True)), the level's draws
(planes_ref.draw_tables gives the kind) and its decor index list (the winner's quad is decor_indices // 4, as
tests/test_hidden_things_host.py's decor_ids derives it); the reduction in plain numpy, pinned by a triple loop over pixels on small
arrays.  A helper, not a test."""
import numpy as np

import planes_ref

NO_THING = 0xFFFFFFFF
KIND_DECOR = 2
INT32_MAX = 0x7FFFFFFF
INF_BITS = 0x7F800000
FRAME_THING = np.dtype([('count', '<u4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('depth_min', '<f4')])


def quad_of_primitive(lv):
    """per primitive id (position in draw order): the decor quad the triangle belongs to, -1 for every triangle that is no decor"""
    arrays = lv if isinstance(lv, dict) else lv.arrays()
    kind, _obj, owner = planes_ref.draw_tables(arrays)
    draws = np.asarray(arrays['draws'], np.uint32).reshape(-1, 4)
    di = np.asarray(arrays['decor_indices'], np.uint32)
    quad = np.full(len(kind), -1, np.int64)
    at = 0
    for k, _o, start, count in draws.tolist():
        nt = count // 3
        if k == KIND_DECOR:
            quad[at:at + nt] = di[start:start + 3 * nt:3].astype(np.int64) // 4
        at += nt
    assert ((quad >= 0) == (kind == KIND_DECOR)).all() and len(owner) == len(quad)
    return quad


def thing_plane(built_or_arrays, table, prim):
    """(.., H, W) winners of the oracle -> (.., H, W) int32: the thing of the winning decor quad by `table` (one word per quad,
    BuiltLevel.decor_things() or a hand-made one; None: a handle without a table), -1 elsewhere"""
    prim = np.asarray(prim, np.uint32)
    out = np.full(prim.shape, -1, np.int32)
    if table is None:
        return out
    table = np.asarray(table, np.uint32)
    quad = quad_of_primitive(built_or_arrays)
    drawn = prim != planes_ref.NO_PRIM
    q = np.where(drawn, quad[np.where(drawn, prim, 0).astype(np.int64)], -1)
    some = q >= 0
    words = table[q[some]]
    out[some] = np.where(words == NO_THING, -1, words.astype(np.int64)).astype(np.int32)
    return out


def empty_table(n, max_things):
    t = np.zeros((n, max_things), FRAME_THING)
    t['x0'] = t['y0'] = INT32_MAX
    t['x1'] = t['y1'] = -1
    t['depth_min'] = np.inf
    return t


def bits_of(count, min_pixels, stride):
    """(n, max_things) counts -> (n, stride) uint32 words"""
    n, max_things = count.shape
    out = np.zeros((n, stride), np.uint32)
    for i in range(min(max_things, 32 * stride)):
        out[:, i // 32] |= (count[:, i] >= min_pixels).astype(np.uint32) << np.uint32(i % 32)
    return out


def reduce(ids, depth, max_things, min_pixels, stride):
    """(table, bits): (n, max_things) FRAME_THING records and (n, stride) uint32 words (None with stride None) of an (n, H, W)
    int32 id plane and an optional float32 depth plane of the same shape"""
    ids = np.asarray(ids, np.int32)
    n, _h, _w = ids.shape
    t = empty_table(n, max_things)
    dbits = None if depth is None else np.ascontiguousarray(depth, np.float32).view(np.uint32)
    for f in range(n):
        for i in np.unique(ids[f]).tolist():
            if not 0 <= i < max_things:
                continue
            ys, xs = np.nonzero(ids[f] == i)
            r = t[f, i]
            r['count'], r['x0'], r['x1'], r['y0'], r['y1'] = len(xs), xs.min(), xs.max(), ys.min(), ys.max()
            if dbits is not None:
                d = dbits[f][ys, xs]
                d = d[d < INF_BITS]
                if len(d):
                    r['depth_min'] = np.array([d.min()], np.uint32).view(np.float32)[0]
    return t, (None if stride is None else bits_of(t['count'], min_pixels, stride))


def reduce_loop(ids, depth, max_things, min_pixels, stride):
    """the same by a triple loop over the pixels, for arrays of at most 8 x 8: the contract read word for word"""
    ids = np.asarray(ids, np.int32)
    n, h, w = ids.shape
    assert h <= 8 and w <= 8
    t = empty_table(n, max_things)
    for f in range(n):
        for y in range(h):
            for x in range(w):
                i = int(ids[f, y, x])
                if i < 0 or i >= max_things:
                    continue
                r = t[f, i]
                r['count'] += 1
                r['x0'], r['y0'] = min(int(r['x0']), x), min(int(r['y0']), y)
                r['x1'], r['y1'] = max(int(r['x1']), x), max(int(r['y1']), y)
                if depth is not None:
                    d = np.float32(depth[f, y, x])
                    if int(d.view(np.uint32)) < INF_BITS and d < r['depth_min']:
                        r['depth_min'] = d
    bits = None
    if stride is not None:
        bits = np.zeros((n, stride), np.uint32)
        for f in range(n):
            for i in range(max_things):
                if i < 32 * stride and t[f, i]['count'] >= min_pixels:
                    bits[f, i // 32] |= np.uint32(1 << (i % 32))
    return t, bits


def as_words(table):
    """FRAME_THING records as the (.., 6) int32 words rd.frame_things returns"""
    return np.ascontiguousarray(table).view(np.int32).reshape(table.shape + (6,))


def synthetic_depth(rng, shape):
    """a depth plane with +inf, -1.0, a NaN, 0.0 and -0.0 among positive values"""
    d = rng.uniform(0.1, 50.0, shape).astype(np.float32)
    flat = d.reshape(-1)
    pick = rng.integers(0, 6, flat.shape)
    flat[pick == 0] = np.inf
    flat[pick == 1] = -1.0
    flat[pick == 2] = np.nan
    flat[(pick == 3) & (rng.integers(0, 4, flat.shape) == 0)] = 0.0
    flat[(pick == 3) & (rng.integers(0, 16, flat.shape) == 0)] = -0.0
    return d
