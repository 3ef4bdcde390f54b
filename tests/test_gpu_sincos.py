"""GPU: the project's sincos (csrc/hip/sincos_rd.hpp) over every binary32 argument.  rdoom_selftest_sincos evaluates all 2^32 on
the device and sums them per binade; tests/sincos_sweep.c does the same on the host with the restatements' one definition
(tests/sincos_restatement.h): the 512 sums must be equal, and eight binades are compared result by result.  The selftest proves its
own translation unit only -- every consumer inlines its own copy -- so two consumers are driven over the whole stated domain as
well: the player cameras (frames.hip) and one tick of the player step (world.hip), bit for bit against their restatements."""
import numpy as np
import pytest

import frames_ref
import rust_doom_amd as rd
import sincos_ref
import world_ref
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
F = np.float32


def _device_raw(b):
    """binade b's (s, c) pairs from the device: float32 (2^23, 2)"""
    out = torch.empty(2 * sincos_ref.BINADE, dtype=torch.float32, device='cuda')
    rd.selftest_sincos(raw_binade=b, raw_out=out)
    return out.cpu().numpy().reshape(-1, 2)


def _first_differences(b, got, want, limit=3):
    """the first arguments of binade b at which the device's and the host's results differ, with both"""
    bad = np.nonzero(~sincos_ref.same_bits(got, want).all(1))[0][:limit]
    x = ((np.uint32(b) << np.uint32(23)) | bad.astype(np.uint32)).view(F)
    return [dict(x=float(x[i]), bits=hex(int(x[i:i + 1].view(np.uint32)[0])), device=got[m].tolist(), host=want[m].tolist()) for i, m in enumerate(bad)]


def test_every_argument_has_the_hosts_bits():
    """(f) all 512 sums; exponent 255 (inf, NaN: every result a NaN) goes through the canonical NaN of the sum.  On a mismatch the
    first differing binade is dumped and its first three differing arguments are reported."""
    rd.set_device(0)
    got, want = rd.selftest_sincos(), sincos_ref.sums()
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape == (512,)
    differing = np.nonzero(got != want)[0]
    if len(differing):
        b = int(differing[0])
        pytest.fail('binades %s differ; binade %d (exponent %d, %s): %s' % (
            differing.tolist(), b, (b & 255) - 127, 'negative' if b >> 8 else 'positive', _first_differences(b, _device_raw(b), sincos_ref.raw(b))))
    assert len(set(got.tolist())) == 512  # (no two binades share a sum: each sum is its own binade's)


@pytest.mark.parametrize('exponent,negative', [(-1, False), (8, False), (12, False), (31, False), (32, False), (-127, False),
                                               (31, True), (32, True)])
def test_raw_results_of_a_binade(exponent, negative):
    """(f) without the hash: 2^-1, 2^8 (the last binade of the two-ulp domain), 2^12 (the last of the curve described), 2^31 and
    2^32 (where the quadrant's conversion saturates at INT_MAX: quadrant 3), zero with the denormals, and -2^31 and -2^32 (the other
    saturation, at INT_MIN: quadrant 0)"""
    rd.set_device(0)
    b = sincos_ref.binade(exponent, negative)
    got, want = _device_raw(b), sincos_ref.raw(b)
    assert sincos_ref.same_bits(got, want).all(), _first_differences(b, got, want)
    if exponent < 31:
        assert np.isfinite(want).all() and (np.abs(want) <= 1.0 + 2.0 ** -22).all()


def test_selftest_rejects_bad_arguments():
    rd.set_device(0)
    out = torch.empty(2 * sincos_ref.BINADE, dtype=torch.float32, device='cuda')
    with pytest.raises(rd.RdoomError) as e:
        rd.selftest_sincos(raw_binade=512, raw_out=out)
    assert e.value.status == -1
    with pytest.raises(rd.RdoomError):
        rd.selftest_sincos(raw_binade=0, raw_out=out.data_ptr() + 4)
    with pytest.raises(ValueError):
        rd.selftest_sincos(raw_binade=0, raw_out=out[:1024])


# ---- (h) two consumers over the stated domain ---------------------------------------------------------------------------------
PITCH_LIMIT = F(1.57079637) - F(1e-2)  # world.hip's clamp (player.rs:196-201)


def _domain_states():
    """players at E1M1's start: 4096 yaws spread over +-512 and every multiple of pi / 4 in that range with both float neighbours,
    each at 9 pitches from clamp end to clamp end"""
    wad = rd.Wad(ensure_wad(), META_PATH)
    pos, _ = wad.build_level(0).start()
    yaws = [np.linspace(-512.0, 512.0, 4096).astype(F)]
    k = np.arange(-651, 652)
    mult = (k * (np.pi / 4)).astype(F)
    assert np.abs(mult).max() < 512 and abs(652 * np.pi / 4) > 512
    yaws += [mult, np.nextafter(mult, F(np.inf)), np.nextafter(mult, F(-np.inf))]
    yaws = np.concatenate(yaws)
    pitches = np.linspace(-float(PITCH_LIMIT), float(PITCH_LIMIT), 9).astype(F)
    pitches[0], pitches[-1] = -PITCH_LIMIT, PITCH_LIMIT
    st = rd.player_states(np.broadcast_to(pos, (len(yaws) * 9, 3)), np.repeat(yaws, 9), pitch=np.tile(pitches, len(yaws)))
    return wad, st


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def test_cameras_over_the_domain():
    """poses_from_players_device (frames.hip) against tests/frames_ref.py, bit for bit (elsewhere compared at |yaw| < 60 pi)"""
    rd.set_device(0)
    _, st = _domain_states()
    poses, _ = rd.poses_from_players_device(st, 320, 200, 0.5)
    torch.cuda.synchronize()
    want, _ = frames_ref.cameras(st, 320, 200, 0.5)
    got = _u32(poses.cpu().numpy())
    bad = np.nonzero((got != _u32(want)).any(1))[0]
    assert len(bad) == 0, (len(bad), st[bad[:3]])
    assert np.isfinite(got.view(F)).all()


def test_one_step_over_the_domain():
    """one tick of step_players (world.hip) with a look and a movement input against tests/world_ref.py, bit for bit (elsewhere
    compared at |yaw| < ~10); every third player flies, so both of the step's uses of the pitch's sine and cosine are taken"""
    rd.set_device(0)
    wad, st = _domain_states()
    st['flags'][::3] |= rd.PLAYER_FLY
    world, ref = wad.build_world(0), world_ref.RefWorld(wad, 0)
    inp = np.zeros((1, len(st)), rd.PLAYER_INPUT)
    inp['look'][0, :, 0], inp['look'][0, :, 1] = 0.015, -0.01
    inp['movement'][0, :, 0], inp['movement'][0, :, 1] = 0.5, -1.0
    inp['jump'][0, ::2] = 1
    got, want = world.step(st, inp), ref.step(st, inp)
    bad = np.nonzero((_u32(got) != _u32(want)).any(1))[0]
    assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
    assert (got['yaw'] != st['yaw']).all() and (np.linalg.norm(got['vel'], axis=1) > 0).all()  # (they turned and were pushed)
    assert (got['pitch'][8::9] == PITCH_LIMIT).all() and (got['pitch'][0::9] > -PITCH_LIMIT).all()  # (look.y up: one end clamps)
