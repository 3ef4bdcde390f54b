"""What rdoom_batch_resolve_plane / rdoom_batch_read_plane must return, composed from the ORACLE only (never from the product's
own output): depth from RasterOracle.render_varyings' v_dist where the oracle's winner is not sky and +inf elsewhere; label and
primitive from render(..., want_prim=True) and the level's draws (running triangle count per draw -> kind and object id).
A helper, not a test."""
import numpy as np

NO_PRIM = 0xFFFFFFFF
LABEL_NONE = 0xFFFF
KIND_SKY = 3


def draw_tables(lv):
    """per primitive id (position in draw order): (kind, object id, index of the draw that owns it)"""
    draws = np.asarray(lv['draws'] if isinstance(lv, dict) else lv.draws, np.uint32).reshape(-1, 4)
    ntri = draws[:, 3].astype(np.int64) // 3
    owner = np.repeat(np.arange(len(draws)), ntri)
    return draws[owner, 0].astype(np.uint32), draws[owner, 1].astype(np.uint32), owner


def labels_of(lv, prim):
    """(.., H, W) winners -> (.., H, W) uint16 labels: kind | object id << 4, LABEL_NONE where nothing was drawn"""
    kind, obj, _ = draw_tables(lv)
    drawn = prim != NO_PRIM
    safe = np.where(drawn, prim, 0).astype(np.int64)
    assert int(obj.max(initial=0)) < 4096
    label = (kind[safe] | (obj[safe] << 4)).astype(np.uint16)
    return np.where(drawn, label, np.uint16(LABEL_NONE)).astype(np.uint16)


def kinds_of(lv, prim):
    """(.., H, W) winners -> kind per pixel (-1 where nothing was drawn)"""
    kind, _, _ = draw_tables(lv)
    drawn = prim != NO_PRIM
    return np.where(drawn, kind[np.where(drawn, prim, 0).astype(np.int64)].astype(np.int64), -1)


def expected_planes(ro, lv, pose, lights, w, h, object_modelviews=None):
    """one frame, bottom-up rows: {'depth': float32 (None with moved objects: render_varyings takes no per-object matrices),
    'label': uint16, 'primitive': uint32}"""
    mv, pr, t = pose['modelview'], pose['projection'], float(pose['time'])
    _, prim = ro.render(mv, pr, t, lights, w, h, want_prim=True, object_modelviews=object_modelviews)
    depth = None
    if object_modelviews is None:
        _, vprim, var = ro.render_varyings(mv, pr, t, lights, w, h)
        assert np.array_equal(vprim, prim)  # (one oracle: both entry points name the same winners)
        solid = (prim != NO_PRIM) & (kinds_of(lv, prim) != KIND_SKY)
        depth = np.where(solid, var[..., 2], np.float32(np.inf)).astype(np.float32)
    return {'depth': depth, 'label': labels_of(lv, prim), 'primitive': prim.astype(np.uint32)}


def expected_batch(lv, poses, lights, w, h, object_modelviews=None, ro=None):
    """all frames of a batch: dict of (n, H, W) arrays"""
    from oracle import raster
    ro = ro or raster.RasterOracle(lv)
    frames = [expected_planes(ro, lv, poses[i], lights[i], w, h, None if object_modelviews is None else object_modelviews[i])
              for i in range(len(poses))]
    return {k: (None if frames[0][k] is None else np.array([f[k] for f in frames])) for k in ('depth', 'label', 'primitive')}
