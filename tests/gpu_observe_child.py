"""Child process of tests/test_gpu_observe.py (one mode per process, prints one RESULT line):
  hooks  every test hook of tests/gpu_rgb_child.py (HOOKS, SIZES: they are process-wide), each time a dirtied batch rendered
         without and with primitive ids; the observations of both renders must equal tests/observe_ref.py applied to THIS
         process's id-path frames (the composition of read_framebuffer / read_primitive_ids, and read_depth), bit for bit.
         Reports bad (differing cells), cases, fixups (pixels that went through fixup_kernel and the fix-list pass) and changed:
         on the REFERENCE, the output cells that differ when the pixels leak_mod sends through the fix list (drawn pixels whose
         row * pitch + column is a multiple of leak_mod, fragment.hip) are left out of the full-size frames -- clear colour,
         +inf -- so a pass that lost the fix pixels' share of a cell could not pass;
  torch  resolve_observation into torch tensors and raw device pointers on a side stream, a sub-range, tensors that do not fit,
         and a captured graph of render_players + resolve_observation replayed.  torch is initialised BEFORE the library is loaded, as
         bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import observe_ref as oref
import rust_doom_amd as rd
from gpu_rgb_child import HOOKS, SIZES, compose
from oracle import wad_oracle
from test_gpu_raster_parity import sweep_poses
from util import META_PATH, ensure_wad

CASES = [(rd.OBS_RGB8, (4, 4)), (rd.OBS_GRAY8, (4, 4)), (rd.OBS_DEPTH_MIN, (4, 4)), (rd.OBS_RGB8, (2, 8))]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def observations(batch):
    return [batch.read_observation(fmt, factor, top_down=(i % 2 == 1)) for i, (fmt, factor) in enumerate(CASES)]


def hooks_case():
    lv = wad_oracle.build_level(ensure_wad(), META_PATH, 0)
    level = rd.DeviceLevel(lv)
    bad, fixups, cases, changed = 0, 0, 0, 0
    for hooks in HOOKS:
        rd.debug_set('reset')
        for name, value in hooks.items():
            rd.debug_set(name, value)
        for w, h, n in SIZES:
            poses = sweep_poses(lv, n, w, h, seed=11, time=0.4)
            other = sweep_poses(lv, n, w, h, seed=12, time=0.4)
            lights = lv.lights.fill_buffer_at(0.4)
            batch = rd.Batch(level, w, h, n)  # (vis32 / entry_cap are read here)
            batch.render(other, lights)
            batch.render(poses, lights)
            plain = observations(batch)
            batch.enable_primitive_ids()
            batch.render(other, lights)
            t = batch.render(poses, lights, timed=True)
            fixups += t['fixup_pixels']
            fb, prim = batch.read_framebuffer(), batch.read_primitive_ids()
            rgb, depth = compose(fb, prim, lv.palette), batch.read_depth()
            ids = observations(batch)
            for i, (fmt, factor) in enumerate(CASES):
                want = oref.observation(fmt, factor, rgb, depth, top_down=(i % 2 == 1))
                diff = int((bits(plain[i]) != bits(want)).sum()) + int((bits(ids[i]) != bits(want)).sum())
                if diff:
                    print('MISMATCH hooks=%r size=%dx%d format=%d factor=%r cells=%d' % (hooks, w, h, fmt, factor, diff))
                bad += diff
            if 'leak_mod' in hooks:  # the reference without the pixels of the fix list
                pitch = batch.framebuffer_pitch()
                yy, xx = np.mgrid[0:h, 0:w]
                forced = ((yy * pitch + xx) % hooks['leak_mod'] == 0)[None] & (prim != 0xFFFFFFFF)
                assert t['fixup_pixels'] >= int(forced.sum()) > 0
                rgb0, depth0 = rgb.copy(), depth.copy()
                rgb0[forced], depth0[forced] = rd.CLEAR_RGB, np.inf
                for fmt, factor in CASES:
                    changed += int((bits(oref.observation(fmt, factor, rgb0, depth0)) != bits(oref.observation(fmt, factor, rgb, depth))).sum())
            cases += 1
            batch.close()
    rd.debug_set('reset')
    print('RESULT bad=%d fixups=%d cases=%d changed=%d' % (bad, fixups, cases, changed))
    return bad == 0


def torch_case():
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    rd.set_device(0)
    lv = wad_oracle.build_level(ensure_wad(), META_PATH, 1)
    w, h, n = 160, 96, 3
    poses = sweep_poses(lv, n, w, h, seed=3, time=0.2)
    lights = lv.lights.fill_buffer_at(0.2)
    batch = rd.Batch(rd.DeviceLevel(lv), w, h, n)
    s = torch.cuda.Stream()
    batch.render(poses, lights, stream=s.cuda_stream)
    for fmt in (rd.OBS_RGB8, rd.OBS_RGB8_PLANAR, rd.OBS_GRAY8, rd.OBS_DEPTH_MIN):
        dtype = torch.float32 if fmt == rd.OBS_DEPTH_MIN else torch.uint8
        for factor, top_down in ((4, False), ((2, 8), True)):
            shape = (n,) + rd.observation_shape(fmt, w, h, factor)
            out = torch.full(shape, 7, dtype=dtype, device='cuda')
            torch.cuda.synchronize()  # (the fill ran on torch's stream)
            assert batch.resolve_observation(out, fmt, factor, top_down=top_down, stream=s) is out
            s.synchronize()
            want = batch.read_observation(fmt, factor, top_down=top_down)
            assert want.shape == shape and np.array_equal(bits(out.cpu().numpy()), bits(want)), (fmt, factor, top_down)
    # a sub-range, into a raw device pointer
    out = torch.zeros((2,) + rd.observation_shape(rd.OBS_RGB8_PLANAR, w, h, 2), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    batch.resolve_observation(out.data_ptr(), rd.OBS_RGB8_PLANAR, 2, first=1, count=2, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), batch.read_observation(rd.OBS_RGB8_PLANAR, 2)[1:3])
    assert np.array_equal(batch.read_observation(rd.OBS_DEPTH_MIN, (8, 4), first=1, count=2), batch.read_observation(rd.OBS_DEPTH_MIN, (8, 4))[1:3])
    # against the full-size frames of the same render
    assert np.array_equal(batch.read_observation(rd.OBS_GRAY8, 4, first=1, count=2, top_down=True),
                          oref.observation(rd.OBS_GRAY8, 4, batch.read_rgb(), top_down=True)[1:3])
    # tensors that do not fit are refused before anything is written
    oh, ow = h // 4, w // 4
    for bad in (torch.zeros((n, oh, ow, 3), dtype=torch.uint8),                  # host memory
                torch.zeros((n, oh, ow, 3), dtype=torch.int32, device='cuda'),   # not bytes
                torch.zeros((n, oh, ow), dtype=torch.uint8, device='cuda'),      # the grey size for RGB8
                torch.zeros((n, oh, ow * 3 + 1), dtype=torch.uint8, device='cuda')[..., :ow * 3]):  # not contiguous
        try:
            batch.resolve_observation(bad, rd.OBS_RGB8, 4)
        except ValueError:
            continue
        raise AssertionError('accepted %s %s %s' % (bad.dtype, bad.device, tuple(bad.shape)))
    try:
        batch.resolve_observation(torch.zeros((n, oh, ow), dtype=torch.uint8, device='cuda'), rd.OBS_DEPTH_MIN, 4)
        raise AssertionError('accepted bytes for depth')
    except ValueError:
        pass
    # a render from device state and its observations captured into one graph (nothing in them allocates or waits), replayed
    built = rd.Wad(ensure_wad(), META_PATH).build_level(0)
    pos, yaw = built.start()
    st = rd.player_states([[pos[0], pos[1], pos[2]]] * n, [float(yaw) + 0.3 * i for i in range(n)])
    states = torch.from_numpy(st.view(np.uint8).copy()).cuda()
    times = torch.full((n,), 0.3, dtype=torch.float32, device='cuda')
    dl = rd.DeviceLights(built)
    pbatch = rd.Batch(rd.DeviceLevel(built), w, h, n)
    pbatch.render_players(states, dl, times=times)
    want_rgb, want_dep = pbatch.read_observation(rd.OBS_RGB8, 4), pbatch.read_observation(rd.OBS_DEPTH_MIN, 4, top_down=True)
    assert np.isfinite(want_dep).any() and len(np.unique(want_rgb)) > 8
    rgb = torch.zeros((n,) + rd.observation_shape(rd.OBS_RGB8, w, h, 4), dtype=torch.uint8, device='cuda')
    dep = torch.zeros((n,) + rd.observation_shape(rd.OBS_DEPTH_MIN, w, h, 4), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cur = torch.cuda.current_stream()
        pbatch.render_players(states, dl, times=times, stream=cur)
        pbatch.resolve_observation(rgb, rd.OBS_RGB8, 4, stream=cur)
        pbatch.resolve_observation(dep, rd.OBS_DEPTH_MIN, 4, top_down=True, stream=cur)
    rgb.zero_()
    dep.zero_()
    graph.replay()
    torch.cuda.synchronize()
    pbatch.finish()
    assert np.array_equal(rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(bits(dep.cpu().numpy()), bits(want_dep))
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if {'hooks': hooks_case, 'torch': torch_case}[sys.argv[1]]() else 1)
