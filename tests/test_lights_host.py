"""The light infos leave the host builder (rdoom_built_light_infos), and the device light tables' contract -- restated in numpy,
tests/lights_ref.py -- against the host's Lights::fill_buffer_at: every byte equal, except Random entries at arguments where glibc
sinf is not the correctly rounded sine.  CPU only."""
import ctypes
import importlib

import numpy as np
import pytest

import lights_ref
import rust_doom_amd as rd
from oracle import wad_oracle
from util import META_PATH, ensure_big_wad

synthetic = importlib.import_module('rust-doom_amd.synthetic')
# every synthetic level: E1M1..E1M9, the level ten times E1M1, the texture-rich level
LEVELS = [('synth', i) for i in range(9)] + [('big', 0), ('rich', 0)]


def wad_of(which, wad_path):
    return {'synth': lambda: wad_path, 'big': ensure_big_wad, 'rich': synthetic.ensure_rich_wad}[which]()


@pytest.fixture(scope='module')
def built_levels(wad_path):
    out = {}
    for which, index in LEVELS:
        out[which, index] = rd.Wad(wad_of(which, wad_path), META_PATH).build_level(index)
    return out


@pytest.mark.parametrize('which,index', LEVELS)
def test_light_infos_equal_the_oracles_list(built_levels, wad_path, oracle_levels, which, index):
    infos = built_levels[which, index].light_infos()
    want = (oracle_levels(index) if which == 'synth' else wad_oracle.build_level(wad_of(which, wad_path), META_PATH, index)).lights.lights
    assert infos.dtype == rd.LIGHT_INFO and len(infos) == len(want) == built_levels[which, index].counters()['num_lights']
    for got, w in zip(infos, want):
        assert np.float32(got['level']).tobytes() == np.float32(w.level).tobytes()
        assert bool(got['has_effect']) == (w.effect is not None)
        if w.effect is None:
            assert got.tobytes()[4:] == bytes(24)  # the effect fields are zero
            continue
        alt, speed, dur, sync, kind = w.effect
        assert int(got['effect_kind']) == int(kind)
        for name, v in (('alt_level', alt), ('speed', speed), ('duration', dur), ('sync', sync)):
            assert np.float32(got[name]).tobytes() == np.float32(v).tobytes(), name


def kind_counts(infos, n_times):
    fx = infos['has_effect'] != 0
    return np.array([int((fx & (infos['effect_kind'] == k)).sum()) * n_times for k in range(3)])


def test_restatement_equals_the_host_but_for_sinf(built_levels):
    times = lights_ref.host_times()
    evaluations = np.zeros(3, np.int64)
    differing = 0
    for key, built in built_levels.items():
        infos = built.light_infos()
        host = np.stack([built.lights_at(float(t)) for t in times])
        want = lights_ref.tables(infos, times)
        n_diff, bad = lights_ref.explained(infos, times, host, want)
        assert not bad, (key, bad[:8])
        differing += n_diff
        evaluations += kind_counts(infos, len(times))
    print('levels: evaluations of Glow / Random / Alternate %s, %d bytes differ (all explained by sinf)' % (evaluations, differing))
    # the hand-written table goes through the same rule against the oracle's Lights (the host builder takes no table from outside)
    infos = lights_ref.handwritten_infos()
    lights = wad_oracle.Lights()
    for i in infos:
        lights.lights.append(wad_oracle.LightInfo(np.float32(i['level']), (np.float32(i['alt_level']), np.float32(i['speed']),
                             np.float32(i['duration']), np.float32(i['sync']), int(i['effect_kind'])) if i['has_effect'] else None))
    hw_times = times[::4]
    got = np.stack([lights.fill_buffer_at(float(t)) for t in hw_times])
    n_diff, bad = lights_ref.explained(infos, hw_times, got, lights_ref.tables(infos, hw_times))
    assert not bad, bad[:8]
    evaluations += kind_counts(infos, len(hw_times))
    print('with the hand-written table: %s, %d more bytes differ' % (evaluations, n_diff))
    assert (evaluations >= 1000).all(), evaluations  # not vacuous: each kind was compared a thousand times and more


def test_degenerate_glow_is_rusts():
    """Pins the RESTATEMENT (tests/lights_ref.py), not the library: it passes without the feature.  The device is held to the
    restatement on this table by the GPU `tables` case; this test fixes what the restatement must say there, from Rust's rules:
    level == alt_level: phase = t * speed / 0 is +-inf or NaN, fract of it NaN, and `NaN as u8` is 0 in Rust -- at every time"""
    times = np.array([0.0, 0.5, 1.0, 77.7, 1e5], np.float32)
    got = lights_ref.tables(lights_ref.degenerate_glow(), times)
    assert got.shape == (5, 256) and not got.any()
    assert np.isnan(lights_ref.levels_at(lights_ref.degenerate_glow(), times)).all()


def test_rust_cast():
    """Pins the restatement's `as u8` (truncate, saturate, NaN -> 0), not the library: it passes without the feature"""
    v = np.array([np.nan, -1.0, -0.0, 0.0, 0.999, 1.0, 254.999, 255.0, 256.0, np.inf, -np.inf], np.float32)
    assert lights_ref.rust_u8(v).tolist() == [0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 0]


def test_light_infos_argument_errors(built_levels):
    L = rd.lib()
    h = built_levels['synth', 0]._h
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    assert L.rdoom_built_light_infos(None, ctypes.byref(p), ctypes.byref(n)) == -1
    assert L.rdoom_built_light_infos(h, None, ctypes.byref(n)) == -1
    assert L.rdoom_built_light_infos(h, ctypes.byref(p), None) == -1
    assert b'null' in L.rdoom_last_error()
    assert L.rdoom_built_light_infos(h, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == len(built_levels['synth', 0].light_infos())
