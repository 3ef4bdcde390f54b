"""Child process of tests/test_gpu_rgb.py (one mode per process, prints one RESULT line):
  hooks  every test hook of tests/test_gpu_debug_paths.py in turn (they are process-wide), each time a dirtied batch rendered
         without and with primitive ids; the RGB frames of both renders must equal the composition of THIS process's id-path
         frames: PLAYPAL[fb], CLEAR_RGB where the id is 0xFFFFFFFF, alpha, optional flip;
  torch  resolve_rgb into torch tensors and raw device pointers on the render's stream.  torch is initialised BEFORE the library
         is loaded, as bench.py does: torch and the library then use one HIP runtime."""
import sys

import numpy as np

import conftest  # noqa: F401  (sys.path)
import rust_doom_amd as rd
from oracle import raster, wad_oracle
from test_gpu_raster_parity import sweep_poses
from util import META_PATH, ensure_wad

HOOKS = [{}, {'leak_mod': 97}, {'no_bins': 1}, {'entry_cap': 300}, {'frag_nq': 1}, {'vis32': 1}, {'vis32': 1, 'leak_mod': 101},
         {'no_cover': 1}, {'frag_bw': 3}, {'frag_bw': 5}, {'no_qtab': 1}, {'keep_vis': 1}, {'qpath': 1}, {'no_split': 1}]
SIZES = [(320, 200, 4), (1366, 768, 2)]


def compose(fb, prim, playpal, alpha=False, top_down=False):
    rgb = np.asarray(playpal, np.uint8).reshape(256, 3)[fb]
    clear = prim == 0xFFFFFFFF
    rgb[clear] = rd.CLEAR_RGB
    if alpha:
        rgb = np.concatenate([rgb, np.where(clear, 0, 255).astype(np.uint8)[..., None]], -1)
    return rgb[:, ::-1] if top_down else rgb


def all_formats(batch):
    return {(a, t): batch.read_rgb(alpha=a, top_down=t) for a in (False, True) for t in (False, True)}


def hooks_case():
    lv = wad_oracle.build_level(ensure_wad(), META_PATH, 0)
    level = rd.DeviceLevel(lv)
    bad, fixups, cases = 0, 0, 0
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
            plain = all_formats(batch)
            batch.enable_primitive_ids()
            batch.render(other, lights)
            t = batch.render(poses, lights, timed=True)
            fixups += t['fixup_pixels']
            fb, prim = batch.read_framebuffer(), batch.read_primitive_ids()
            ids = all_formats(batch)
            for (a, td), got in plain.items():
                want = compose(fb, prim, lv.palette, a, td)
                diff = int((got != want).any(-1).sum()) + int((ids[(a, td)] != want).any(-1).sum())
                if diff:
                    print('MISMATCH hooks=%r size=%dx%d alpha=%s top_down=%s pixels=%d' % (hooks, w, h, a, td, diff))
                bad += diff
            cases += 1
            batch.close()
    rd.debug_set('reset')
    print('RESULT bad=%d fixups=%d cases=%d' % (bad, fixups, cases))
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
    for alpha in (False, True):
        for top_down in (False, True):
            out = torch.full((n, h, w, 4 if alpha else 3), 7, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()  # (the fill ran on torch's stream)
            assert batch.resolve_rgb(out, alpha=alpha, top_down=top_down, stream=s) is out
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), batch.read_rgb(alpha=alpha, top_down=top_down)), (alpha, top_down)
    # a sub-range, into a raw device pointer
    out = torch.zeros((2, h, w, 4), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    batch.resolve_rgb(out.data_ptr(), first=1, count=2, alpha=True, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), batch.read_rgb(alpha=True)[1:3])
    # against the oracle's frames
    ro = raster.RasterOracle(lv)
    fb, prim = zip(*[ro.render(p['modelview'], p['projection'], 0.2, lights, w, h, want_prim=True) for p in poses])
    assert np.array_equal(batch.read_rgb(first=1, count=2, top_down=True), compose(np.array(fb), np.array(prim), lv.palette, top_down=True)[1:3])
    # tensors that do not fit are refused before anything is written
    for bad in (torch.zeros((n, h, w, 3), dtype=torch.uint8),                 # host memory
                torch.zeros((n, h, w, 3), dtype=torch.int32, device='cuda'),  # not bytes
                torch.zeros((n, h, w, 4), dtype=torch.uint8, device='cuda'),  # the RGBA size for RGB8
                torch.zeros((n, h, w * 3 + 1), dtype=torch.uint8, device='cuda')[..., :w * 3]):  # not contiguous
        try:
            batch.resolve_rgb(bad)
        except ValueError:
            continue
        raise AssertionError('accepted %s %s %s' % (bad.dtype, bad.device, tuple(bad.shape)))
    print('RESULT ok=1')
    return True


if __name__ == '__main__':
    sys.exit(0 if {'hooks': hooks_case, 'torch': torch_case}[sys.argv[1]]() else 1)
