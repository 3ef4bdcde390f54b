"""Things in the frame on the host, with no GPU: the header include/rdoom_frame_things.h (prototypes, the record, the third symbol
list), every argument error that is found before a device is touched, and the yardstick of the GPU tests, tests/framethings_ref.py:
the thing plane of the oracle's winners on E1M1's two facing poses, the numpy reduction against a triple loop over the pixels, and
its bit rows against rd.pack_things."""
import ctypes
import os
import re

import numpy as np
import pytest

import framethings_ref as fr
import rust_doom_amd as rd
from oracle import raster
from test_hidden_things_host import decor_ids, facing_poses
from util import META_PATH, ensure_wad

BAD = -1  # RDOOM_BAD_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rdoom_frame_things.h')
W, H = 320, 200


def declared(path):
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(rdoom_[a-z0-9_]+)\s*\(', text)))


def prototype(name):
    m = re.search(r'^(\w[\w \*]*?)\s*\b%s\(([^;]*)\);' % name, open(HEADER).read(), flags=re.M)
    assert m, name
    return m.group(1).strip(), [' '.join(a.split()) for a in m.group(2).split(',')]


# ---- the interface ----
def test_the_prototypes_argument_by_argument():
    assert prototype('rdoom_batch_resolve_thing_plane') == \
        ('rdoom_status', ['rdoom_batch *batch', 'uint32_t first', 'uint32_t count', 'uint32_t flags', 'int32_t *d_out', 'void *stream'])
    assert prototype('rdoom_batch_read_thing_plane') == \
        ('rdoom_status', ['rdoom_batch *batch', 'uint32_t first', 'uint32_t count', 'uint32_t flags', 'int32_t *out'])
    assert prototype('rdoom_frame_things') == \
        ('rdoom_status', ['const int32_t *d_ids', 'const float *d_depth', 'uint32_t n', 'uint32_t width', 'uint32_t height', 'uint32_t max_things',
                          'uint32_t min_pixels', 'rdoom_frame_thing *d_table', 'uint32_t *d_bits', 'uint32_t stride', 'void *stream'])
    assert '#include "rdoom.h"' in open(HEADER).read()


def test_the_record_is_24_bytes_of_six_words():
    text = open(HEADER).read()
    m = re.search(r'typedef struct rdoom_frame_thing \{(.*?)\} rdoom_frame_thing;', text, flags=re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    fields = [(' '.join(t.split()), [n.strip() for n in names.split(',')]) for t, names in re.findall(r'(\w+)\s+([\w, ]+);', body)]
    assert fields == [('uint32_t', ['count']), ('int32_t', ['x0', 'y0', 'x1', 'y1']), ('float', ['depth_min'])]
    dt = rd.FRAME_THING
    assert dt.itemsize == 24 and dt.names == ('count', 'x0', 'y0', 'x1', 'y1', 'depth_min') and dt == fr.FRAME_THING
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20]
    assert [dt.fields[n][0].str for n in dt.names] == ['<u4', '<i4', '<i4', '<i4', '<i4', '<f4']
    empty = fr.empty_table(1, 1)
    assert fr.as_words(empty).reshape(-1).tolist() == [0, 0x7FFFFFFF, 0x7FFFFFFF, -1, -1, 0x7F800000]
    assert rd.frame_things_depth(fr.as_words(empty)).tolist() == [[np.inf]]


def test_the_third_symbol_list_is_the_new_header_and_the_other_two_are_untouched():
    assert declared(HEADER) == sorted(rd.FRAME_THINGS_API_SYMBOLS) and len(set(rd.FRAME_THINGS_API_SYMBOLS)) == 3
    assert not set(rd.FRAME_THINGS_API_SYMBOLS) & (set(rd.API_SYMBOLS) | set(rd.RAY_API_SYMBOLS))
    lib = ctypes.CDLL(rd.LIB_PATH)
    assert all(hasattr(lib, n) for n in rd.FRAME_THINGS_API_SYMBOLS)
    assert all(getattr(rd.lib(), n).restype is ctypes.c_int32 for n in rd.FRAME_THINGS_API_SYMBOLS)
    main = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
    assert len(rd.API_SYMBOLS) == len(re.findall(r'^(?:rdoom_status|void|const char \*)\s*rdoom_\w+\(', main, flags=re.M)) == 135
    assert 'thing_plane' not in main and 'rdoom_frame_things' not in main
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    outside = text[:text.index('<!-- BEGIN GENERATED')] + text[text.index('<!-- END GENERATED'):]
    assert 'rdoom_frame_things.h' in outside
    for name in rd.FRAME_THINGS_API_SYMBOLS:
        assert re.search(r'pub fn %s\(' % name, outside), name


def test_the_calls_check_their_arguments_before_they_touch_a_device():
    """device pointers that are never followed: every call below is refused on the host, or (n == 0) queues nothing"""
    L = rd.lib()
    v = ctypes.c_void_p
    fake, fake2, fake3, fake4 = v(0x1000), v(0x2000), v(0x3000), v(0x4000)
    for fn, tail in ((L.rdoom_batch_resolve_thing_plane, (fake, None)), (L.rdoom_batch_read_thing_plane, (fake,))):
        assert fn(None, 0, 1, 0, *tail) == BAD and 'null' in L.rdoom_last_error().decode()
        assert fn(None, 0, 1, rd.RGB_TOP_DOWN, *tail) == BAD and 'null' in L.rdoom_last_error().decode()
        for flags in (1, 4, rd.PLANE_PRIMITIVE, rd.RGB_TOP_DOWN | 1, 0x200, 0x80000000):  # stray bits, found before the null batch
            assert fn(None, 0, 1, flags, *tail) == BAD and 'flag' in L.rdoom_last_error().decode(), flags

    def call(n=1, w=4, h=4, max_things=8, min_pixels=1, ids=fake, depth=fake2, table=fake3, bits=fake4, stride=1):
        return L.rdoom_frame_things(ids, depth, n, w, h, max_things, min_pixels, table, bits, stride, None)

    assert call(n=0) == 0 and call(n=0, ids=None, depth=None, table=None, bits=None, stride=0) == 0  # a null launch
    for n in (0, 1):  # the limits hold for a null launch too
        assert call(n=n, min_pixels=0) == BAD and 'min_pixels' in L.rdoom_last_error().decode()
        assert call(n=n, max_things=0) == BAD and 'max_things' in L.rdoom_last_error().decode()
        assert call(n=n, max_things=(1 << 20) + 1) == BAD and 'max_things' in L.rdoom_last_error().decode()
        assert call(n=n, w=0) == BAD and call(n=n, h=0) == BAD
        assert call(n=n, w=1 << 16, h=1 << 15) == BAD and '2^31' in L.rdoom_last_error().decode()
        assert call(n=n, w=0x7FFFFFFF, h=2) == BAD
        assert call(n=n, stride=0) == BAD and 'stride' in L.rdoom_last_error().decode()
        for k in ('ids', 'depth', 'table', 'bits'):
            assert call(n=n, **{k: v(0x1002)}) == BAD and 'aligned' in L.rdoom_last_error().decode(), k
    assert call(ids=None) == BAD and 'null' in L.rdoom_last_error().decode()
    assert call(table=None) == BAD and 'null' in L.rdoom_last_error().decode()
    assert call(n=1 << 12, max_things=1 << 20) == BAD  # n * max_things records at 2^32
    assert call(n=0, max_things=1 << 20, w=46340, h=46340, bits=None, stride=0) == 0  # the limits themselves are inside


# ---- the yardstick ----
@pytest.fixture(scope='module')
def e1m1():
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(0)
    arrays = built.arrays()
    poses, lights = facing_poses(built, arrays)
    ro = raster.RasterOracle(arrays)
    prims = np.stack([ro.render(p['modelview'], p['projection'], 0.0, lights, W, H, want_prim=True)[1] for p, _seen in poses])
    return dict(built=built, arrays=arrays, table=built.decor_things(), poses=poses, prims=prims)


def test_the_thing_plane_of_the_two_facing_poses(e1m1):
    arrays, table = e1m1['arrays'], e1m1['table']
    ids = decor_ids(arrays)
    quad_of = fr.quad_of_primitive(arrays)
    for q, t in ids.items():  # the map of test_hidden_things_host.py: a quad's two triangles follow each other
        assert quad_of[t] == quad_of[t + 1] == q
    assert (quad_of >= 0).sum() == 2 * len(table)
    plane = fr.thing_plane(arrays, table, e1m1['prims'])
    assert plane.dtype == np.int32 and plane.shape == (2, H, W)
    for f, (_pose, seen) in enumerate(e1m1['poses']):
        shown = sorted(set(plane[f][plane[f] >= 0].tolist()))
        assert len(shown) >= 2 and shown == sorted(table[seen].tolist()), (shown, seen)
        # a pixel names a thing exactly where the winner is one of the quad's two triangles
        for q in seen:
            assert np.array_equal(plane[f] == table[q], (e1m1['prims'][f] == ids[q]) | (e1m1['prims'][f] == ids[q] + 1))
    assert (plane == -1).mean() > 0.9  # most of a frame shows no thing
    assert (fr.thing_plane(arrays, None, e1m1['prims']) == -1).all()
    # a table of its own: NO_THING and an index that repeats
    other = np.array(table, np.uint32, copy=True)
    a, b = e1m1['poses'][0][1][:2]
    other[a], other[b] = fr.NO_THING, 77
    p2 = fr.thing_plane(arrays, other, e1m1['prims'][0])
    assert not (p2 == table[a]).any() and np.array_equal(p2 == 77, plane[0] == table[b]) and ((p2 == -1) == ((plane[0] == -1) | (plane[0] == table[a]))).all()


def test_reduce_on_the_facing_poses_counts_every_thing_pixel(e1m1):
    plane = fr.thing_plane(e1m1['arrays'], e1m1['table'], e1m1['prims'])
    t, bits = fr.reduce(plane, None, 64, 12, 2)
    assert int(t['count'].sum()) == int((plane >= 0).sum()) and np.isinf(t['depth_min']).all()
    for f in range(2):
        for i in np.flatnonzero(t[f]['count']).tolist():
            r = t[f, i]
            box = plane[f, r['y0']:r['y1'] + 1, r['x0']:r['x1'] + 1]
            assert (box == i).sum() == r['count'] == (plane[f] == i).sum()
            assert (box[0] == i).any() and (box[-1] == i).any() and (box[:, 0] == i).any() and (box[:, -1] == i).any()
    assert np.array_equal(bits.view(np.int32), np.stack([rd.pack_things(t[f]['count'] >= 12, 2) for f in range(2)]))


@pytest.mark.parametrize('seed', range(6))
def test_reduce_against_the_triple_loop(seed):
    rng = np.random.default_rng(seed)
    n, h, w = int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
    max_things = (1, 5, 31, 32, 33, 65)[seed]
    ids = rng.integers(-2, min(max_things, 6) + 3, (n, h, w)).astype(np.int32)
    if seed == 2:
        ids[0] = 3  # one id throughout
    depth = fr.synthetic_depth(rng, (n, h, w))
    words = (max_things + 31) // 32
    for d in (None, depth):
        for min_pixels in (1, 2, h * w + 1):
            for stride in (None, 1, words, words + 2):
                a, ab = fr.reduce(ids, d, max_things, min_pixels, stride)
                b, bb = fr.reduce_loop(ids, d, max_things, min_pixels, stride)
                assert np.array_equal(fr.as_words(a), fr.as_words(b)), (seed, min_pixels, stride)
                assert (ab is None and bb is None) or np.array_equal(ab, bb)
                if stride is not None and stride >= words:
                    assert np.array_equal(ab.view(np.int32), np.stack([rd.pack_things(a[f]['count'] >= min_pixels, stride) for f in range(n)]))
                if min_pixels == h * w + 1 and stride is not None:
                    assert not ab.any()


def test_reduce_hand_cases():
    ids = np.array([[[0, 0, -1, 2], [7, 0, 2, 2], [-5, 8, 2, 1]]], np.int32)
    depth = np.array([[[2.0, -1.0, 1.0, np.inf], [0.5, np.nan, 3.0, 0.0], [0.1, 0.1, -0.0, 4.0]]], np.float32)
    t, bits = fr.reduce(ids, depth, 8, 2, 3)
    rows = fr.as_words(t)[0]
    inf = 0x7F800000
    assert rows[0].tolist() == [3, 0, 0, 1, 1, int(np.float32(2.0).view(np.uint32))]  # -1.0 and the NaN never count
    assert rows[1].tolist() == [1, 3, 2, 3, 2, int(np.float32(4.0).view(np.uint32))]
    assert rows[2].tolist() == [4, 2, 0, 3, 2, 0]  # +0.0 is the smallest; -0.0 (bits 0x80000000) does not count
    assert rows[7].tolist() == [1, 0, 1, 0, 1, int(np.float32(0.5).view(np.uint32))]
    assert rows[3].tolist() == [0, 0x7FFFFFFF, 0x7FFFFFFF, -1, -1, inf]  # id 8 == max_things is ignored
    assert bits.tolist() == [[0b101, 0, 0]]
