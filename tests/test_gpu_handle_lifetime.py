"""GPU: every handle created, used and destroyed twenty times over (csrc/hip/device_memory.hpp: a handle's members own its device
memory, pinned memory, events and stream, and its destroy function is `delete`).  A cycle allocates every member a handle can
have, the ones allocated on first use included; the frames of the last cycle must be the first cycle's, byte for byte, and the
first cycle's the oracle's.  E1M2, 128 x 80 x 4 poses, 64 players.  The free device memory the cycles cost is printed, not asserted
(other users of the card move it): run with -s."""
import numpy as np
import pytest

import rust_doom_amd as rd
from oracle import raster
from util import META_PATH, ensure_wad

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
W, H, N, PLAYERS, CYCLES = 128, 80, 4, 64, 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_twenty_cycles_of_every_handle():
    rd.set_device(0)
    wad = rd.Wad(ensure_wad(), META_PATH)
    built = wad.build_level(1)
    pos, yaw = built.start()
    poses = np.zeros(N, rd.POSE)
    for i in range(N):
        poses[i] = rd.pose_look((pos[0], pos[1] + 0.12, pos[2]), float(yaw) + 0.7 * i, 0.05 * i, W, H, 0.0)
    lights = built.lights_at(0.0)
    table = built.decor_things()
    things_table = wad.build_world(1, device=False).map_things()
    words = (len(things_table) + 31) // 32
    hidden = np.zeros((N, max(1, words)), np.uint32)
    hidden[0] = 0xFFFFFFFF  # pose 0 sees no thing at all, the others every one
    states = _dev(rd.player_states(np.tile(np.asarray(pos, np.float32), (PLAYERS, 1)), np.linspace(0.0, 6.0, PLAYERS, dtype=np.float32)))
    slots = torch.from_numpy((np.arange(PLAYERS) % 2).astype(np.int32)).cuda()
    times = torch.linspace(0.0, 9.0, PLAYERS, device='cuda')
    fan = torch.from_numpy(rd.ray_fan(16, 2.0)).cuda()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle(measure):
        before = free_bytes() if measure else 0
        level = rd.DeviceLevel(built.desc)  # (from the descriptor: no thing table yet)
        om = np.ascontiguousarray(np.broadcast_to(poses['modelview'].reshape(N, 1, 16), (N, level.num_objects(), 16)), np.float32)
        batch = rd.Batch(level, W, H, N)
        batch.render(poses, lights, object_modelviews=om)
        out = {'frame': batch.read_framebuffer(), 'om': om}
        batch.enable_primitive_ids()
        batch.render(poses, lights, object_modelviews=om)
        out['rgb'], out['prim'] = batch.read_rgb(), batch.read_primitive_ids()
        level.set_decor_things(table)
        rows = torch.from_numpy(hidden.view(np.int32).copy()).cuda()
        batch.set_hidden_things(rows)
        batch.render(poses, lights)
        out['hidden'] = batch.read_framebuffer()
        world, ws = rd.World(wad, 1), rd.WorldSet(wad, [0, 1])
        dev_lights, dev_things = rd.DeviceLights(built), rd.DeviceThings(things_table)
        out['frac'] = world.cast_rays(states, fan, 30.0).cpu().numpy()
        out['set_frac'] = ws.cast_rays(states, slots, fan, 30.0).cpu().numpy()
        out['tables'] = dev_lights.tables(times).cpu().numpy()
        out['visible'] = world.sense_things(states, dev_things, 30.0).visible.cpu().numpy()
        held = before - free_bytes() if measure else 0
        for handle in (dev_things, dev_lights, ws, world, batch, level):
            handle.close()
        return out, held

    first, _ = cycle(False)
    ro = raster.RasterOracle(built.arrays())
    for i in range(N):
        want = ro.render(poses[i]['modelview'], poses[i]['projection'], 0.0, lights, W, H, object_modelviews=first['om'][i])
        assert np.array_equal(want, first['frame'][i]), ('pose %d differs from the oracle' % i, int((want != first['frame'][i]).sum()))
    _, held = cycle(True)
    after_two = free_bytes()
    for _ in range(CYCLES - 3):
        cycle(False)
    last, _ = cycle(False)
    print('\nhandle lifetime: one cycle holds %d bytes of device memory; free memory fell by %d bytes between the end of cycle 2 and '
          'the end of cycle %d' % (held, after_two - free_bytes(), CYCLES))
    assert sorted(last) == sorted(first)
    for name in first:
        assert first[name].dtype == last[name].dtype and first[name].tobytes() == last[name].tobytes(), name
