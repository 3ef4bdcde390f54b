"""Depth / label / primitive planes (rdoom_batch_resolve_plane / rdoom_batch_read_plane) at the C-ABI boundary, without a GPU:
the header declares the entry points and the constants, the library exports and validates, the Python wrapper exposes the API.
The errors that need a batch are checked in tests/test_gpu_planes.py."""
import ctypes
import inspect
import os
import re

import numpy as np

import rust_doom_amd as rd
from util import ROOT

HEADER = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()
PLANES = ('DEPTH', 'LABEL', 'PRIMITIVE')


def header_define(name):
    m = re.search(r'^#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b' % name, HEADER, flags=re.M)
    assert m, name
    return int(m.group(1), 0)


def test_header_declares_the_entry_points_and_constants():
    code = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
    assert re.search(r'rdoom_status rdoom_batch_resolve_plane\(rdoom_batch \*batch, uint32_t first, uint32_t count, uint32_t plane,'
                     r'\s*void \*device_out,\s*void \*stream\);', code)
    assert re.search(r'rdoom_status rdoom_batch_read_plane\(rdoom_batch \*batch, uint32_t first, uint32_t count, uint32_t plane,'
                     r'\s*void \*host_out\);', code)
    values = [header_define('RDOOM_PLANE_' + p) for p in PLANES]
    assert values == [rd.PLANE_DEPTH, rd.PLANE_LABEL, rd.PLANE_PRIMITIVE] and len(set(values)) == 3
    assert all(0 < v <= 0xFF and not v & rd.RGB_TOP_DOWN for v in values)  # (the row-order flag sits above the plane field)
    assert header_define('RDOOM_LABEL_NONE') == rd.LABEL_NONE == 0xFFFF
    # no label of a drawn pixel is RDOOM_LABEL_NONE: kind 0..3, object id 12 bits, and kind 15 does not exist
    assert max(header_define('RDOOM_KIND_' + k) for k in ('FLAT', 'WALL', 'DECOR', 'SKY')) == 3
    assert {p: np.dtype(rd.PLANE_DTYPES[getattr(rd, 'PLANE_' + p)]).name for p in PLANES} == \
        {'DEPTH': 'float32', 'LABEL': 'uint16', 'PRIMITIVE': 'uint32'}


def test_header_states_the_contract():
    """the planes' definitions are the header comment's: depth formula, sky at infinity, the none values, row order"""
    doc = HEADER[HEADER.index('Per-pixel planes of the batch'):HEADER.index('#define RDOOM_PLANE_DEPTH')]
    for needle in ('1.0f / fmaf(wp[0], x + 0.5f, fmaf(wp[1], y + 0.5f, wp[2]))', '+inf', 'kind | object_id << 4', 'RDOOM_LABEL_NONE',
                   '0xFFFFFFFF', 'RDOOM_RGB_TOP_DOWN', 'rdoom_batch_read_primitive_ids', 'playpal'):
        assert needle in doc, needle
    prim_doc = HEADER[HEADER.index('Debug / test facility'):HEADER.index('rdoom_status rdoom_batch_enable_primitive_ids')]
    assert 'RDOOM_PLANE_PRIMITIVE' in prim_doc


def test_library_exports_the_entry_points():
    L = rd.lib()
    for name in ('rdoom_batch_resolve_plane', 'rdoom_batch_read_plane'):
        assert name in rd.API_SYMBOLS and hasattr(L, name)


def test_bad_arguments_are_rejected_without_a_device():
    L = rd.lib()
    out = np.zeros(64, np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    good = [rd.PLANE_DEPTH, rd.PLANE_LABEL, rd.PLANE_PRIMITIVE]
    for plane in good + [v | rd.RGB_TOP_DOWN for v in good]:
        assert L.rdoom_batch_read_plane(None, 0, 1, plane, p) == -1
        assert b'null' in L.rdoom_last_error()
        assert L.rdoom_batch_resolve_plane(None, 0, 1, plane, p, None) == -1
        assert b'null' in L.rdoom_last_error()
    # an unknown plane or a stray flag bit: rejected before the batch is looked at (a null batch is not what is reported)
    for plane in (0, 4, 0xFF, rd.RGB_TOP_DOWN, 0x200 | rd.PLANE_DEPTH, 0x80000000 | rd.PLANE_LABEL, 0x1000 | rd.PLANE_PRIMITIVE):
        assert L.rdoom_batch_read_plane(None, 0, 1, plane, p) == -1
        assert b'plane' in L.rdoom_last_error() and b'null' not in L.rdoom_last_error(), plane
        assert L.rdoom_batch_resolve_plane(None, 0, 1, plane, p, None) == -1
        assert b'plane' in L.rdoom_last_error() and b'null' not in L.rdoom_last_error(), plane


def test_python_wrapper_exposes_the_api():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(rd.Batch.resolve_plane) == ['self', 'out', 'plane', 'first', 'count', 'top_down', 'stream']
    assert sig(rd.Batch.read_plane) == ['self', 'plane', 'first', 'count', 'top_down']
    assert sig(rd.Batch.resolve_depth) == ['self', 'out', 'first', 'count', 'top_down', 'stream']
    assert sig(rd.Batch.read_depth) == ['self', 'first', 'count', 'top_down']
    p = inspect.signature(rd.Batch.resolve_plane).parameters
    assert (p['first'].default, p['count'].default, p['top_down'].default, p['stream'].default) == (0, None, False, None)
