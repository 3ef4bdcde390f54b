"""GPU: things in the frame (include/rdoom_frame_things.h; rust-doom_amd/csrc/hip/framethings.hip).  The thing plane of a render
against tests/framethings_ref.py's composition of the ORACLE's winners, and rdoom_frame_things against its numpy reduction, bit for
bit everywhere.  The cases run in tests/gpu_framethings_child.py, a process of their own per group (the debug hooks are
process-wide); frames of at most 321 x 200 and at most 16 poses."""
import os
import subprocess
import sys

import pytest

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(mode):
    """tests/gpu_framethings_child.py MODE in a process of its own, under a time limit: a child that dies by a signal or times out fails"""
    p = subprocess.run([sys.executable, os.path.join(HERE, 'gpu_framethings_child.py'), mode], cwd=HERE, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode >= 0, 'child killed by signal %d:\n%s%s' % (-p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    out = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT')]
    assert out and p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return {k: int(v) for k, v in (kv.split('=') for kv in out[-1].split()[1:])}


@gpu
def test_the_facing_poses_under_every_debug_path():
    """320 x 200 and 321 x 200; plain and id path; both row orders; a sub-range; vis32, no_qtab, keep_vis, leak_mod, no_bins, entry_cap"""
    fields = run_child('hooks')
    assert fields['bad'] == 0 and fields['checks'] == 2 * 7 * 2 * 7


@gpu
def test_a_level_set_names_things_per_level():
    fields = run_child('levels')
    assert fields['bad'] == 0 and fields['checks'] == 2 * 7


@gpu
def test_the_hand_made_level_hidden_rows_a_described_quadrant_and_no_table():
    """indices at and above 32, two quads of one thing, NO_THING; random hidden rows against the twin level; from so close that whole
    quadrants are one decor triangle's; and the handle before a table is attached: all -1"""
    fields = run_child('handmade')
    assert fields['bad'] == 0 and fields['checks'] == 2 + 3 * 2 * 7 and fields['whole'] >= 8


@gpu
def test_frame_things_on_synthetic_tensors():
    """widths 1 .. 321, heights 1, 2, 33, one to three frames, max_things 1 .. 65, strides at the minimum and wider, min_pixels 1, 2
    and 64001, depth with +inf, -1, NaN and 0; one id throughout 320 x 200; 200 ids in 2 x 2 blocks; ids far out of range"""
    fields = run_child('synthetic')
    assert fields['bad'] == 0 and fields['checks'] == 2 * (11 * 3 * 2 * 3 + 5 + 3 + 2 + 1)


@gpu
def test_frame_things_alone_captured_into_a_graph():
    fields = run_child('graph')
    assert fields['bad'] == 0 and fields['checks'] == 4


@gpu
def test_a_thing_on_a_lift_through_render_players():
    fields = run_child('lift')
    assert fields['bad'] == 0 and fields['checks'] == 4


@gpu
def test_the_errors_that_need_a_device_and_raw_pointers():
    """nothing rendered, frame ranges, a host pointer, a misaligned pointer, stray flags, plane value 4 still refused by
    resolve_plane, tensors that do not fit; then the plane and the reduction through raw device pointers on a raw stream handle"""
    fields = run_child('errors')
    assert fields['bad'] == 0 and fields['checks'] == 7 + 7 + 4


@gpu
def test_the_tick_on_one_stream_without_a_host_wait():
    fields = run_child('tick')
    assert fields['bad'] == 0 and fields['checks'] == 6
