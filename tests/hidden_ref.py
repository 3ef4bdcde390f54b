"""Hidden things (include/rdoom.h "hidden things") restated on level arrays, for tests/test_hidden_things_host.py and the GPU tests.

The yardstick is a TWIN level: the same arrays with the six indices of every hidden quad q replaced by 4q.  Such a triangle has
three equal vertices: every pair of products in the edge coefficients (S3) cancels exactly, the determinant (S4) is exactly 0, and
`det > 0` culls it, in the oracle and in the kernels.  Draw ranges and primitive ids are those of the level itself, so frames,
primitive ids, depth and labels of a render with hidden rows compare bit for bit with a render of the twin without rows."""
import numpy as np

NO_THING = 0xFFFFFFFF


def hidden_quads(row, table):
    """the decor quads a row of thing bits hides: quad q of thing table[q] when that is not NO_THING, lies below 32 * len(row), and
    has its bit set"""
    row = np.ascontiguousarray(row).reshape(-1).view(np.uint32)  # (uint32 or int32 words)
    out = []
    for q, thing in enumerate(np.asarray(table, np.uint32).tolist()):
        if thing != NO_THING and thing < 32 * len(row) and (int(row[thing >> 5]) >> (thing & 31)) & 1:
            out.append(q)
    return np.array(out, np.int64)


def row_of(things, stride):
    """a row of `stride` words with the bits of `things` set (all of them must fit)"""
    row = np.zeros(stride, np.uint32)
    for t in things:
        assert 0 <= int(t) < 32 * stride, (t, stride)
        row[int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
    return row


def twin(arrays, quads):
    """the level's arrays with every decor triangle of `quads` collapsed to the quad's first vertex"""
    out = dict(arrays)
    di = np.array(arrays['decor_indices'], np.uint32, copy=True)
    hit = np.isin(di // 4, np.asarray(quads, np.int64))
    di[hit] = (di[hit] // 4) * 4
    out['decor_indices'] = di
    return out


def deleted(arrays, quads):
    """(arrays, old_id): the level's arrays without the decor triangles of `quads` -- index list and draw ranges rebuilt -- and, per
    primitive id of the new level, the id the triangle has in the old one"""
    out = dict(arrays)
    draws = np.asarray(arrays['draws'], np.uint32).reshape(-1, 4)
    di = np.asarray(arrays['decor_indices'], np.uint32)
    quads = np.asarray(quads, np.int64)
    new_di, new_draws, old_id, at = [], [], [], 0
    for kind, obj, first, count in draws.tolist():
        if kind != 2:
            new_draws.append((kind, obj, first, count))
            old_id.extend(range(at, at + count // 3))
        else:
            tris = di[first:first + count].reshape(-1, 3)
            keep = ~np.isin(tris[:, 0] // 4, quads)
            if keep.any():
                new_draws.append((kind, obj, sum(len(t) for t in new_di), 3 * int(keep.sum())))
                new_di.append(tris[keep].reshape(-1))
            old_id.extend((at + np.flatnonzero(keep)).tolist())
        at += count // 3
    out['decor_indices'] = np.concatenate(new_di).astype(np.uint32) if new_di else np.zeros(0, np.uint32)
    out['draws'] = np.array(new_draws, np.uint32).reshape(-1, 4)
    return out, np.array(old_id, np.uint32)


def remap(prim, old_id):
    """primitive ids of a `deleted` level as ids of the level it came from (no primitive stays no primitive)"""
    prim = np.asarray(prim, np.uint32)
    out = np.full(prim.shape, NO_THING, np.uint32)
    some = prim != NO_THING
    out[some] = old_id[prim[some]]
    return out
