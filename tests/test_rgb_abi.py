"""RGB frames (rdoom_batch_resolve_rgb / rdoom_batch_read_rgb) at the C-ABI boundary, without a GPU: the header declares the
entry points and the formats, the clear colour is the reference window's, the library exports and validates, the Python
wrapper exposes the API, and the shipped resolve kernels use no scratch memory."""
import ctypes
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

import gl_readback
import rust_doom_amd as rd
from util import ROOT

HEADER = open(os.path.join(ROOT, 'include', 'rdoom.h')).read()


def header_define(name):
    m = re.search(r'^#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b' % name, HEADER, flags=re.M)
    assert m, name
    return int(m.group(1), 0)


def test_header_declares_the_entry_points_and_formats():
    code = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
    assert re.search(r'rdoom_status rdoom_batch_resolve_rgb\(rdoom_batch \*batch, uint32_t first, uint32_t count, uint32_t format,'
                     r'\s*void \*device_out,\s*void \*stream\);', code)
    assert re.search(r'rdoom_status rdoom_batch_read_rgb\(rdoom_batch \*batch, uint32_t first, uint32_t count, uint32_t format,'
                     r'\s*uint8_t \*host_out\);', code)
    assert header_define('RDOOM_RGB8') == rd.RGB8 == 3
    assert header_define('RDOOM_RGBA8') == rd.RGBA8 == 4
    assert header_define('RDOOM_RGB_TOP_DOWN') == rd.RGB_TOP_DOWN
    assert rd.RGB_TOP_DOWN & 0xFF == 0  # (a flag above the bytes-per-pixel field)


def test_clear_colour_is_the_reference_windows():
    """window.rs:40-44 clears to (0.06, 0.07, 0.09): the colour the GL readbacks show where nothing was drawn"""
    clear = tuple(header_define('RDOOM_CLEAR_' + c) for c in 'RGB')
    assert clear == tuple(gl_readback.CLEAR_RGB) == tuple(rd.CLEAR_RGB)
    assert clear == tuple(int(round(v * 255)) for v in (0.06, 0.07, 0.09))


def test_library_exports_the_entry_points():
    L = rd.lib()
    assert 'rdoom_batch_resolve_rgb' in rd.API_SYMBOLS and 'rdoom_batch_read_rgb' in rd.API_SYMBOLS
    assert hasattr(L, 'rdoom_batch_resolve_rgb') and hasattr(L, 'rdoom_batch_read_rgb')


def test_bad_arguments_are_rejected_without_a_device():
    L = rd.lib()
    out = np.zeros(64, np.uint8)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for fmt in (rd.RGB8, rd.RGBA8, rd.RGB8 | rd.RGB_TOP_DOWN, rd.RGBA8 | rd.RGB_TOP_DOWN):
        assert L.rdoom_batch_read_rgb(None, 0, 1, fmt, p) == -1
        assert b'null' in L.rdoom_last_error()
        assert L.rdoom_batch_resolve_rgb(None, 0, 1, fmt, p, None) == -1
        assert b'null' in L.rdoom_last_error()
    for fmt in (0, 1, 2, 5, 0x200 | rd.RGB8, 0x80000000 | rd.RGBA8, rd.RGB_TOP_DOWN):
        assert L.rdoom_batch_read_rgb(None, 0, 1, fmt, p) == -1
        assert b'format' in L.rdoom_last_error(), fmt
        assert L.rdoom_batch_resolve_rgb(None, 0, 1, fmt, p, None) == -1
        assert b'format' in L.rdoom_last_error(), fmt


def test_python_wrapper_exposes_the_api():
    assert callable(rd.Batch.read_rgb) and callable(rd.Batch.resolve_rgb)
    import inspect
    assert list(inspect.signature(rd.Batch.read_rgb).parameters) == ['self', 'first', 'count', 'alpha', 'top_down']
    assert list(inspect.signature(rd.Batch.resolve_rgb).parameters) == ['self', 'out', 'first', 'count', 'alpha', 'top_down', 'stream']


_spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


@pytest.mark.skipif(not (os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump')) and shutil.which('c++filt')), reason='needs the ROCm LLVM tools')
def test_resolve_kernels_are_shipped_without_scratch():
    res = {kr.short(k): v for k, v in kr.kernel_resources().items()}
    names = ['%s<%d, %s>' % (k, bpp, v16) for k in ('resolve_kernel', 'resolve_fix_kernel') for bpp in (3, 4) for v16 in ('false', 'true')]
    for k in names:
        assert k in res, (k, sorted(res))
        r = res[k]
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, (k, r)
    # the palette is the only LDS: 256 words
    assert all(res[k]['group_segment_fixed_size'] <= 1024 for k in names)
