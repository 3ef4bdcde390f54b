"""rust-doom_amd -- MI355X-native pose-batch renderer for Doom WAD levels.

Thin Python mirror of the C ABI in include/rdoom.h (ctypes over librdoom_hip.so).  Names follow the
reference: `Wad` ~ wad::Archive + TextureDirectory (wad/src/archive.rs, tex.rs), `BuiltLevel` ~ what
game::level::Builder + GameShaders::load_level hand to glium (game/src/level.rs:424-496),
`DeviceLevel` / `Batch` ~ the GL buffers/textures and Renderer::update's draw loop
(engine/src/renderer.rs:98-157) -- executed by hand-written HIP kernels.

There is NO CPU fallback: if librdoom_hip.so is missing or a HIP call fails, this raises.
(The directory name contains '-', so import it with importlib.import_module('rust-doom_amd') or via
the `rust_doom_amd` shim at the repository root.)
"""
import collections
import ctypes
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'librdoom_hip.so')

KIND_FLAT, KIND_WALL, KIND_DECOR, KIND_SKY = 0, 1, 2, 3
ALL_KINDS = 0xF
NO_PRIMITIVE = 0xFFFFFFFF
# rdoom_batch_resolve_rgb / rdoom_batch_read_rgb formats (include/rdoom.h); CLEAR_RGB: the GL clear colour (window.rs:40-44)
RGB8, RGBA8, RGB_TOP_DOWN = 3, 4, 0x100
CLEAR_RGB = (15, 18, 23)
# rdoom_batch_resolve_plane / rdoom_batch_read_plane: per-pixel planes of the last render (include/rdoom.h has the contract)
PLANE_DEPTH, PLANE_LABEL, PLANE_PRIMITIVE = 1, 2, 3
LABEL_NONE = 0xFFFF
PLANE_DTYPES = {PLANE_DEPTH: np.float32, PLANE_LABEL: np.uint16, PLANE_PRIMITIVE: np.uint32}
# rdoom_batch_resolve_observation / rdoom_batch_read_observation: reduced-size observations (include/rdoom.h has the contract)
OBS_RGB8, OBS_RGB8_PLANAR, OBS_GRAY8, OBS_DEPTH_MIN = 1, 2, 3, 4
OBS_DTYPES = {OBS_RGB8: np.uint8, OBS_RGB8_PLANAR: np.uint8, OBS_GRAY8: np.uint8, OBS_DEPTH_MIN: np.float32}

STATIC_VERTEX = np.dtype([('a_pos', '<f4', 3), ('a_atlas_uv', '<f4', 2), ('a_tile_uv', '<f4', 2),
                          ('a_tile_size', '<f4', 2), ('a_scroll_rate', '<f4'), ('a_row_height', '<f4'),
                          ('a_num_frames', 'u1'), ('a_light', 'u1'), ('_pad', 'u1', 2)])
SPRITE_VERTEX = np.dtype([('a_pos', '<f4', 3), ('a_atlas_uv', '<f4', 2), ('a_tile_uv', '<f4', 2),
                          ('a_tile_size', '<f4', 2), ('a_local_x', '<f4'), ('a_num_frames', 'u1'),
                          ('a_light', 'u1'), ('_pad', 'u1', 2)])
POSE = np.dtype([('modelview', '<f4', 16), ('projection', '<f4', 16), ('time', '<f4'), ('_pad', '<f4')])
assert STATIC_VERTEX.itemsize == 48 and SPRITE_VERTEX.itemsize == 44 and POSE.itemsize == 136
# the collision world + player physics (include/rdoom.h): Player's state with the entity's position and (yaw, pitch), one tick's
# input as Input::poll_analog2d / poll_gesture return it (game/src/player.rs:107-113, 190-192), Config's physics half (:56-92)
PLAYER_STATE = np.dtype([('pos', '<f4', 3), ('vel', '<f4', 3), ('yaw', '<f4'), ('pitch', '<f4'), ('last_height_diff', '<f4'),
                         ('flags', '<u4')])
PLAYER_INPUT = np.dtype([('movement', '<f4', 2), ('look', '<f4', 2), ('jump', '<u4')])
PLAYER_CONFIG = np.dtype([(n, '<f4') for n in ('move_force', 'spring_const_p', 'spring_const_d', 'radius', 'height', 'air_drag',
                                               'ground_drag', 'friction')])
PLAYER_FLY, PLAYER_CLIP, PLAYER_DIVERGED = 1, 2, 0x100
WORLD_HOST_ONLY = 1
# doors, lifts and exits (include/rdoom.h rdoom_world_triggers / rdoom_world_step_game)
PLAYER_EXITED = 0x200
ACTION_NONE, ACTION_PUSH, ACTION_SHOOT = 0, 1, 2
TRIGGER_WALK_OVER, TRIGGER_PUSH, TRIGGER_SWITCH, TRIGGER_GUN, TRIGGER_ANY = 0, 1, 2, 3, 4
TRIGGER_ONLY_ONCE, TRIGGER_EXIT, TRIGGER_UNIMPLEMENTED = 1, 2, 4
TRIGGER = np.dtype([('origin', '<f4', 2), ('displace', '<f4', 2), ('length', '<f4'), ('trigger_type', '<u4'), ('flags', '<u4'),
                    ('special_type', '<u4'), ('effect_start', '<u4'), ('effect_end', '<u4')])
MOVE_EFFECT = np.dtype([('object_id', '<u4'), ('first_height_offset', '<f4'), ('second_height_offset', '<f4'), ('speed', '<f4'),
                        ('wait', '<f4'), ('has_second', '<u4'), ('repeat', '<u4')])
assert TRIGGER.itemsize == 40 and MOVE_EFFECT.itemsize == 28
# world sets (include/rdoom.h rdoom_worldset_*): one slot per level, and the level each exit leads to
WORLDSET_NO_DESTINATION = 0xFFFFFFFF
WORLDSET_LEVEL = np.dtype([('archive_index', '<u4'), ('destination', '<u4'), ('start_pos', '<f4', 3), ('start_yaw', '<f4'),
                           ('n_triggers', '<u4'), ('n_objects', '<u4'), ('node_depth', '<u4')])
assert PLAYER_STATE.itemsize == 40 and PLAYER_INPUT.itemsize == 20 and PLAYER_CONFIG.itemsize == 32
RAY_NO_HIT = 0xFFFFFFFF  # rdoom_world_cast_rays' hit index where nothing is within range
# rdoom_map_line: one linedef of a level's line table (World.map_lines), and the class codes of a map pixel (World.draw_maps)
MAP_SIDE = np.dtype([('present', '<u4'), ('floor', '<f4'), ('ceiling', '<f4'), ('floor_id', '<u4'), ('ceiling_id', '<u4')])
MAP_LINE = np.dtype([('linedef', '<u4'), ('a', '<f4', 2), ('b', '<f4', 2), ('flags', '<u4'), ('special_type', '<u4'),
                     ('front', MAP_SIDE), ('back', MAP_SIDE)])
MAP_NONE, MAP_FLAT, MAP_CEILING_STEP, MAP_FLOOR_STEP, MAP_CLOSED, MAP_ONE_SIDED, MAP_PLAYER = 0, 1, 2, 3, 4, 5, 8
MAP_ROTATE, MAP_SHOW_FLAT, MAP_SHOW_HIDDEN, MAP_TOP_DOWN = 1, 2, 4, 8
LINE_SECRET, LINE_HIDDEN = 0x20, 0x80  # the linedef flags the map reads: drawn as one-sided; never on the map
MAP_SECTOR = np.dtype([('floor', '<f4'), ('ceiling', '<f4'), ('floor_id', '<u4'), ('ceiling_id', '<u4'), ('light_level', '<u4'),
                       ('sector_type', '<u4'), ('tag', '<u4')])  # rdoom_map_sector
MAP_EDGE = np.dtype([('a', '<f4', 2), ('d', '<f4', 2)])  # rdoom_map_edge
SECTOR_NONE, SECTOR_NONE16 = 0xFFFFFFFF, 0xFFFF
FLOOD_UNREACHED = 0xFFFF  # RDOOM_FLOOD_UNREACHED: flood_maps' distance of a cell no allowed path leads to
FLOOD_GRID_UNREACHED = 0xFFFFFFFF  # RDOOM_FLOOD_GRID_UNREACHED: flood_grids' distance of such a cell (-1 as int32)
FLOOD_TOWARDS = 1  # RDOOM_FLOOD_TOWARDS: flood_grids counts the moves from a cell to the seed, not from the seed to the cell
LINE_REVERSED = 1  # RDOOM_LINE_REVERSED: walk_lines tests every move of a line from its far cell back to its near one
STRAIGHTEN_MAX_LOOK = 1024  # RDOOM_STRAIGHTEN_MAX_LOOK: the most cells of a path straighten_paths looks ahead from a corner
WALL_FAR = 0xFFFF  # RDOOM_WALL_FAR: wall_distances' value of a cell with no blocking cell within the radius
WALL_MAX_RADIUS = 32  # RDOOM_WALL_MAX_RADIUS: the largest radius, in cells, of wall_distances and inflate_grids
WALL_EDGE_OPEN = 1  # RDOOM_WALL_EDGE_OPEN: cells outside the grid do not block
WALL_TILE = (64, 32)  # the cells (across, down) of the tile one workgroup of the wall-distance kernel takes (kernels.hpp)
SPAWN_TRIES = 8  # RDOOM_SPAWN_TRIES: the candidates spawn_players draws for a player before it falls back to the level's start
SPAWN_RISE = 0.5  # RDOOM_SPAWN_RISE: a spawned player's height above the live floor, the start's above the floor at the start marker
SPAWN_ENTRY = np.dtype([('a', '<f4', 3), ('b', '<f4', 3), ('c', '<f4', 3), ('cumulative', '<f4')])  # rdoom_spawn_entry
# rdoom_thing: one thing of a level's thing table (World.map_things, DeviceThings), its categories (the low byte of `category`), and
# rdoom_thing_nearest: sense_things' record of the nearest visible thing of a category
THING = np.dtype([('x', '<f4'), ('z', '<f4'), ('base', '<f4'), ('radius', '<f4'), ('object_id', '<u4'), ('sector', '<u4'),
                  ('thing_type', '<u2'), ('flags', '<u2'), ('category', '<u2'), ('angle', '<u2')])
THING_NEAREST = np.dtype([('index', '<i4'), ('d2', '<f4'), ('right', '<f4'), ('forward', '<f4')])
assert THING.itemsize == 32 and THING_NEAREST.itemsize == 16
THING_DECORATION, THING_WEAPON, THING_POWERUP, THING_ARTIFACT, THING_AMMO, THING_KEY, THING_MONSTER, THING_UNKNOWN = range(8)
THING_HANGING = 0x100  # RDOOM_THING_HANGING, above the category's low byte
THING_CATEGORIES = 8
LINE_MAPPED = 0x100  # RDOOM_LINE_MAPPED, Doom's "already on the map": drawn through a seen set whether seen or not
AREA_UNKNOWN, AREA_FREE, AREA_WALL = 0, 1, 2  # RDOOM_AREA_*: draw_area_maps' bytes (3: a cell that carries both bits)
AREA_MAX_STEPS = 4096  # RDOOM_AREA_MAX_STEPS
# (3, 3) uint8, unknown / free / wall: torch.from_numpy(AREA_COLORS).cuda()[maps.clamp(max=2).long()] is an RGB map (both bits: wall)
AREA_COLORS = np.array([(0, 0, 0), (72, 72, 88), (252, 0, 0)], np.uint8)


def _map_colors():
    t = np.zeros((256, 3), np.uint8)
    t[MAP_FLAT] = (96, 96, 96)            # grey: no height differs
    t[MAP_CEILING_STEP] = (252, 252, 0)   # yellow
    t[MAP_FLOOR_STEP] = (188, 120, 72)    # brown
    t[MAP_CLOSED] = (0, 200, 200)         # a shut door: cyan, not one of Doom's
    t[MAP_ONE_SIDED] = (252, 0, 0)        # red
    t[MAP_PLAYER] = (255, 255, 255)
    return t


MAP_COLORS = _map_colors()  # (256, 3) uint8: torch.from_numpy(MAP_COLORS).cuda()[maps.long()] is an RGB map
# rdoom_thingset_draw_maps (DeviceThings.draw_maps): the default code of a thing of category c is MAP_THING + c, above every MAP_*
# line class; THING_MARKS_OVER: only the covered bytes are written; THING_MARKS: rdoom_thing_marks as a numpy record
MAP_THING = 16
THING_MARKS_OVER = 1
THING_MARKS = np.dtype([('min_radius', '<f4'), ('codes', 'u1', 8), ('flags', '<u4')])
# rdoom_world_stamp_things (World.stamp_things): its parameters, and the cells (across, down) of the tile one workgroup takes (kernels.hpp)
STAMP_PARAMS = np.dtype([('grow', '<f4'), ('block_below', '<f4'), ('block_above', '<f4'), ('flags', '<u4')])
STAMP_TILE = (64, 16)
# rdoom_ray_things (include/rdoom_rays.h; World.cast_rays_things): its parameters
RAY_THINGS = np.dtype([('height', '<f4', 8), ('grow', '<f4'), ('category_mask', '<u4'), ('flags', '<u4')])
assert THING_MARKS.itemsize == 16 and RAY_THINGS.itemsize == 44
# rdoom_frame_thing (include/rdoom_frame_things.h; frame_things): what one frame shows of one thing
FRAME_THING = np.dtype([('count', '<u4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('depth_min', '<f4')])
assert FRAME_THING.itemsize == 24


def _thing_map_colors():
    t = np.zeros((MAP_THING + THING_CATEGORIES, 3), np.uint8)
    t[:MAP_THING] = MAP_COLORS[:MAP_THING]
    t[MAP_THING + THING_DECORATION] = (120, 120, 140)  # grey-blue: scenery
    t[MAP_THING + THING_WEAPON] = (255, 128, 0)        # orange
    t[MAP_THING + THING_POWERUP] = (0, 255, 0)         # green
    t[MAP_THING + THING_ARTIFACT] = (200, 0, 255)      # violet
    t[MAP_THING + THING_AMMO] = (255, 220, 120)        # sand
    t[MAP_THING + THING_KEY] = (64, 128, 255)          # blue
    t[MAP_THING + THING_MONSTER] = (255, 0, 128)       # pink
    t[MAP_THING + THING_UNKNOWN] = (160, 160, 160)     # grey
    return t


# (24, 3) uint8: MAP_COLORS' first 16 rows, then one colour per thing category, so that
# torch.from_numpy(THING_MAP_COLORS).cuda()[maps.long()] colours a line map with the default thing marks overlaid
THING_MAP_COLORS = _thing_map_colors()
# rdoom_light_info (wad/src/light.rs:8-25 LightInfo): what BuiltLevel.light_infos returns and DeviceLights takes
LIGHT_INFO = np.dtype([('level', '<f4'), ('has_effect', '<i4'), ('effect_kind', '<i4'), ('alt_level', '<f4'), ('speed', '<f4'),
                       ('duration', '<f4'), ('sync', '<f4')])
LIGHT_GLOW, LIGHT_RANDOM, LIGHT_ALTERNATE = 0, 1, 2
assert LIGHT_INFO.itemsize == 28


class RdoomError(RuntimeError):
    def __init__(self, status, message):
        super().__init__('rdoom status %d: %s' % (status, message))
        self.status = status


class LevelDesc(ctypes.Structure):
    _fields_ = [
        ('static_verts', ctypes.c_void_p), ('n_static_verts', ctypes.c_uint32),
        ('static_indices', ctypes.c_void_p), ('n_static_indices', ctypes.c_uint32),
        ('sky_verts', ctypes.c_void_p), ('n_sky_verts', ctypes.c_uint32),
        ('sky_indices', ctypes.c_void_p), ('n_sky_indices', ctypes.c_uint32),
        ('decor_verts', ctypes.c_void_p), ('n_decor_verts', ctypes.c_uint32),
        ('decor_indices', ctypes.c_void_p), ('n_decor_indices', ctypes.c_uint32),
        ('draws', ctypes.c_void_p), ('n_draws', ctypes.c_uint32),
        ('flat_atlas', ctypes.c_void_p), ('flat_w', ctypes.c_uint32), ('flat_h', ctypes.c_uint32),
        ('wall_atlas', ctypes.c_void_p), ('wall_w', ctypes.c_uint32), ('wall_h', ctypes.c_uint32),
        ('decor_atlas', ctypes.c_void_p), ('decor_w', ctypes.c_uint32), ('decor_h', ctypes.c_uint32),
        ('sky_texture', ctypes.c_void_p), ('sky_w', ctypes.c_uint32), ('sky_h', ctypes.c_uint32),
        ('sky_tiled_band_size', ctypes.c_float),
        ('playpal', ctypes.c_void_p), ('colormap', ctypes.c_void_p)]


class Timings(ctypes.Structure):
    _fields_ = [('setup_ms', ctypes.c_float), ('raster_ms', ctypes.c_float), ('fragment_ms', ctypes.c_float),
                ('total_ms', ctypes.c_float), ('pixels', ctypes.c_uint64), ('visible_triangles', ctypes.c_uint64),
                ('fixup_pixels', ctypes.c_uint64)]


class PathStats(ctypes.Structure):
    _fields_ = [('poses', ctypes.c_uint32), ('bins_overflowed_poses', ctypes.c_uint32), ('tiles', ctypes.c_uint64), ('split_tiles', ctypes.c_uint64),
                ('tile_entries', ctypes.c_uint64), ('quadrants', ctypes.c_uint64), ('described_quadrants', ctypes.c_uint64),
                ('half_runs', ctypes.c_uint64), ('half_fallbacks', ctypes.c_uint64), ('listed_quads', ctypes.c_uint64),
                ('masked_fast_bodies', ctypes.c_uint64), ('masked_fast_pixels', ctypes.c_uint64), ('masked_fast_replays', ctypes.c_uint64),
                ('masked_general_bodies', ctypes.c_uint64), ('settled_pairs', ctypes.c_uint64), ('raster_pairs', ctypes.c_uint64)]


class HostTimings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ('open_ms', 'textures_ms', 'level_lumps_ms', 'atlases_ms', 'analysis_ms', 'walk_ms')]


class Counters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in
                ('num_wall_quads', 'num_floor_polys', 'num_ceil_polys', 'num_sky_wall_quads', 'num_sky_floor_polys',
                 'num_sky_ceil_polys', 'num_decors', 'num_static_tris', 'num_sky_tris', 'num_sprite_tris',
                 'num_objects', 'num_lights')]


# every symbol include/rdoom.h declares (tests check the library exports all of them)
API_SYMBOLS = [
    'rdoom_last_error', 'rdoom_device_count', 'rdoom_set_device', 'rdoom_level_create', 'rdoom_level_destroy',
    'rdoom_batch_create', 'rdoom_batch_destroy', 'rdoom_batch_render', 'rdoom_batch_render_timed', 'rdoom_batch_render_profiled', 'rdoom_batch_collect_timings',
    'rdoom_batch_framebuffer_device', 'rdoom_batch_finish', 'rdoom_batch_read_framebuffer', 'rdoom_batch_read_primitive_ids',
    'rdoom_wad_open', 'rdoom_wad_close', 'rdoom_wad_num_levels', 'rdoom_wad_level_name',
    'rdoom_wad_name_from_bytes', 'rdoom_wad_build_level', 'rdoom_built_destroy', 'rdoom_built_desc',
    'rdoom_built_counters', 'rdoom_built_lights_at', 'rdoom_built_start', 'rdoom_built_floor_centroids',
    'rdoom_pose_look', 'rdoom_selftest_fastmath', 'rdoom_debug_set', 'rdoom_wad_walk', 'rdoom_wad_build_level_chained', 'rdoom_batch_render_objects', 'rdoom_level_num_objects', 'rdoom_batch_enable_primitive_ids',
    'rdoom_wad_timings', 'rdoom_built_timings', 'rdoom_pose_from_player', 'rdoom_batch_framebuffer_pitch', 'rdoom_batch_path_stats',
    'rdoom_levelset_create', 'rdoom_level_num_levels', 'rdoom_batch_render_levels', 'rdoom_batch_resolve_rgb', 'rdoom_batch_read_rgb',
    'rdoom_world_create', 'rdoom_world_destroy', 'rdoom_world_host_arrays', 'rdoom_world_sweep', 'rdoom_world_step_players',
    'rdoom_player_config_default', 'rdoom_world_triggers', 'rdoom_world_game_bytes', 'rdoom_world_game_reset', 'rdoom_world_step_game',
    'rdoom_object_modelviews_from_player', 'rdoom_worldset_create', 'rdoom_worldset_destroy', 'rdoom_worldset_info',
    'rdoom_worldset_level', 'rdoom_worldset_game_bytes', 'rdoom_worldset_game_reset', 'rdoom_worldset_step_game',
    'rdoom_poses_from_players_device', 'rdoom_batch_render_players', 'rdoom_batch_resolve_plane', 'rdoom_batch_read_plane',
    'rdoom_world_cast_rays', 'rdoom_worldset_cast_rays', 'rdoom_built_light_infos', 'rdoom_lightset_create', 'rdoom_lightset_destroy',
    'rdoom_lightset_tables', 'rdoom_poses_from_players_device_clocked', 'rdoom_batch_render_players_clocked',
    'rdoom_world_map_lines', 'rdoom_worldset_level_map_lines', 'rdoom_world_draw_maps', 'rdoom_worldset_draw_maps',
    'rdoom_world_reveal_lines', 'rdoom_worldset_reveal_lines', 'rdoom_world_draw_maps_seen', 'rdoom_worldset_draw_maps_seen',
    'rdoom_world_map_sectors', 'rdoom_worldset_level_map_sectors', 'rdoom_world_locate_players', 'rdoom_worldset_locate_players',
    'rdoom_world_draw_sector_maps', 'rdoom_worldset_draw_sector_maps', 'rdoom_batch_resolve_observation',
    'rdoom_batch_read_observation', 'rdoom_flood_max_cells', 'rdoom_flood_maps',
    'rdoom_world_spawn_table', 'rdoom_worldset_level_spawn_table', 'rdoom_world_spawn_players', 'rdoom_worldset_spawn_players',
    'rdoom_world_area_grid', 'rdoom_worldset_level_area_grid', 'rdoom_world_area_words', 'rdoom_worldset_area_words',
    'rdoom_world_reveal_area', 'rdoom_worldset_reveal_area', 'rdoom_world_draw_area_maps', 'rdoom_worldset_draw_area_maps',
    'rdoom_world_draw_area_planes', 'rdoom_worldset_draw_area_planes', 'rdoom_flood_grid_max_cells', 'rdoom_flood_grids',
    'rdoom_world_area_cells', 'rdoom_worldset_area_cells', 'rdoom_flood_descend', 'rdoom_world_area_frontiers',
    'rdoom_worldset_area_frontiers', 'rdoom_wall_distance', 'rdoom_selftest_sincos', 'rdoom_flood_grids_octile',
    'rdoom_flood_descend_octile', 'rdoom_grid_walk_lines', 'rdoom_path_straighten',
    'rdoom_world_map_things', 'rdoom_worldset_level_map_things', 'rdoom_thingset_create', 'rdoom_thingset_destroy', 'rdoom_thingset_info',
    'rdoom_world_sense_things', 'rdoom_worldset_sense_things',
    'rdoom_built_decor_things', 'rdoom_level_set_decor_things', 'rdoom_batch_set_hidden_things', 'rdoom_thingset_draw_maps',
    'rdoom_world_thing_obstacles', 'rdoom_worldset_level_thing_obstacles',
    'rdoom_world_stamp_things', 'rdoom_worldset_stamp_things']
# every symbol include/rdoom_rays.h declares: the same library exports them
RAY_API_SYMBOLS = ['rdoom_world_cast_rays_things', 'rdoom_worldset_cast_rays_things']
# every symbol include/rdoom_frame_things.h declares: the same library exports them
FRAME_THINGS_API_SYMBOLS = ['rdoom_batch_resolve_thing_plane', 'rdoom_batch_read_thing_plane', 'rdoom_frame_things']

_lib = None


def lib():
    """Loads librdoom_hip.so (built by rust-doom_amd/build.py).  Raises if it is missing: no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError('%s is missing: run `python rust-doom_amd/build.py` (hipcc, gfx950). '
                              'There is no CPU fallback.' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.rdoom_last_error.restype = ctypes.c_char_p
        for name in API_SYMBOLS:
            fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
            if name not in ('rdoom_last_error', 'rdoom_level_destroy', 'rdoom_batch_destroy', 'rdoom_wad_close',
                            'rdoom_built_destroy', 'rdoom_world_destroy', 'rdoom_worldset_destroy', 'rdoom_lightset_destroy',
                            'rdoom_thingset_destroy'):
                fn.restype = ctypes.c_int32
            elif name != 'rdoom_last_error':
                fn.restype = None
        for name in RAY_API_SYMBOLS + FRAME_THINGS_API_SYMBOLS:
            getattr(L, name).restype = ctypes.c_int32
        _lib = L
    return _lib


def _check(status):
    if status != 0:
        raise RdoomError(status, lib().rdoom_last_error().decode('utf-8', 'replace'))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def _factors(factor):
    fx, fy = (factor, factor) if isinstance(factor, (int, np.integer)) else factor
    fx, fy = int(fx), int(fy)
    if fx not in (1, 2, 4, 8) or fy not in (1, 2, 4, 8):
        raise ValueError('factor must be 1, 2, 4 or 8, or a pair (fx, fy) of them, not %r' % (factor,))
    return fx, fy


def observation_shape(format, width, height, factor):
    """shape of ONE frame's observation: (oh, ow, 3) OBS_RGB8, (3, oh, ow) OBS_RGB8_PLANAR, (oh, ow) OBS_GRAY8 (uint8) and
    OBS_DEPTH_MIN (float32), with ow = width // fx, oh = height // fy; factor: an int or (fx, fy), each 1, 2, 4 or 8"""
    if format not in OBS_DTYPES:
        raise ValueError('format must be OBS_RGB8, OBS_RGB8_PLANAR, OBS_GRAY8 or OBS_DEPTH_MIN, not %r' % (format,))
    fx, fy = _factors(factor)
    ow, oh = int(width) // fx, int(height) // fy
    if ow == 0 or oh == 0:
        raise ValueError('factors %d x %d leave no cell of a %d x %d frame' % (fx, fy, width, height))
    return {OBS_RGB8: (oh, ow, 3), OBS_RGB8_PLANAR: (3, oh, ow)}.get(format, (oh, ow))


def device_count():
    n = ctypes.c_int32(0)
    _check(lib().rdoom_device_count(ctypes.byref(n)))
    return n.value


def set_device(i):
    _check(lib().rdoom_set_device(int(i)))


def debug_set(name, value=1):
    """rdoom_debug_set: test hooks selecting equivalent kernel paths (include/rdoom.h); 'reset' restores the defaults."""
    _check(lib().rdoom_debug_set(name.encode('ascii'), int(value)))


def selftest_fastmath():
    """rdoom_selftest_fastmath: exhaustive on-device check of the fragment kernel's exact division forms."""
    out = (ctypes.c_uint64 * 8)()
    _check(lib().rdoom_selftest_fastmath(out))
    keys = ('rcp_mismatches', 'div09_mismatches', 'inputs_swept', 'mod_violations', 'mod_samples', 'mod_certified',
            'mod_floor_differs', 'packed_mismatches')
    return dict(zip(keys, [int(x) for x in out]))


def selftest_sincos(raw_binade=None, raw_out=None):
    """rdoom_selftest_sincos: the device's sincos over all 2^32 binary32 arguments.  Returns the 512 per-binade sums (uint64; a
    binade is bits >> 23; include/rdoom.h states the sum).  With raw_binade and raw_out -- a contiguous float32 torch tensor of
    2^24 elements on the current device, or a device pointer -- binade raw_binade's (s, c) pairs are written there as well."""
    sums = np.zeros(512, np.uint64)
    if (raw_binade is None) != (raw_out is None):
        raise ValueError('raw_binade and raw_out go together')
    ptr = None
    if raw_out is not None:
        if hasattr(raw_out, 'data_ptr'):
            if not (raw_out.is_cuda and raw_out.is_contiguous() and raw_out.element_size() == 4 and raw_out.numel() >= 1 << 24):
                raise ValueError('raw_out must be a contiguous device tensor of at least 2^24 float32')
            ptr = ctypes.c_void_p(raw_out.data_ptr())
        else:
            ptr = ctypes.c_void_p(int(raw_out))
    _check(lib().rdoom_selftest_sincos(sums.ctypes.data_as(ctypes.c_void_p), int(raw_binade or 0), ptr))
    return sums


def wad_name(value):
    """WadName::from_bytes (wad/src/name.rs:41-75) -> 8 bytes; raises RdoomError on invalid names."""
    if isinstance(value, str):
        value = value.encode('utf-8')
    out = (ctypes.c_uint8 * 8)()
    _check(lib().rdoom_wad_name_from_bytes(bytes(value), len(value), out))
    return bytes(out)


def pose_look(eye, yaw, pitch, width, height, time=0.0):
    """rdoom_pose_look: the reference camera (player.rs:84-89,325-345) as one POSE record."""
    pose = np.zeros(1, POSE)
    e = (ctypes.c_float * 3)(*[float(x) for x in eye])
    _check(lib().rdoom_pose_look(e, ctypes.c_float(yaw), ctypes.c_float(pitch), int(width), int(height),
                                 ctypes.c_float(time), pose.ctypes.data_as(ctypes.c_void_p)))
    return pose[0]


def pose_from_player(pos, yaw, pitch, width, height, time=0.0):
    """rdoom_pose_from_player: the same camera in the reference's own binary32 arithmetic (Decomposed / Quaternion of cgmath);
    `pos` is the player's position -- the camera height (0.12) is added by the helper."""
    pose = np.zeros(1, POSE)
    e = (ctypes.c_float * 3)(*[float(x) for x in pos])
    _check(lib().rdoom_pose_from_player(e, ctypes.c_float(yaw), ctypes.c_float(pitch), int(width), int(height),
                                        ctypes.c_float(time), pose.ctypes.data_as(ctypes.c_void_p)))
    return pose[0]


def make_desc(arrays):
    """Builds a LevelDesc from a dict/object of numpy arrays (same field names as oracle BuiltLevel).
    Returns (desc, keepalive)."""
    g = (lambda k, d=None: arrays.get(k, d)) if isinstance(arrays, dict) else (lambda k, d=None: getattr(arrays, k, d))
    c = np.ascontiguousarray
    keep = dict(
        sv=c(g('static_vertices')), si=c(g('static_indices'), np.uint32),
        kv=c(g('sky_vertices'), np.float32).reshape(-1, 3), ki=c(g('sky_indices'), np.uint32),
        dv=c(g('decor_vertices', np.zeros(0, SPRITE_VERTEX))), di=c(g('decor_indices', np.zeros(0, np.uint32)), np.uint32),
        dr=c(g('draws'), np.uint32).reshape(-1, 4), fa=c(g('flat_atlas'), np.uint8), wa=c(g('wall_atlas'), np.uint16),
        da=c(g('decor_atlas', np.zeros((0, 0), np.uint16)), np.uint16),
        st=c(g('sky_texture'), np.uint16), pp=c(g('palette'), np.uint8), cm=c(g('colormap'), np.uint8))
    k = keep
    assert k['sv'].dtype.itemsize == 48, 'static vertices must be 48-byte StaticVertex records'
    assert k['dv'].dtype.itemsize == 44 or k['dv'].size == 0
    h2 = lambda a: (a.shape[1], a.shape[0]) if a.ndim == 2 and a.size else (0, 0)
    d = LevelDesc()
    d.static_verts, d.n_static_verts = _ptr(k['sv']), len(k['sv'])
    d.static_indices, d.n_static_indices = _ptr(k['si']), len(k['si'])
    d.sky_verts, d.n_sky_verts = _ptr(k['kv']), len(k['kv'])
    d.sky_indices, d.n_sky_indices = _ptr(k['ki']), len(k['ki'])
    d.decor_verts, d.n_decor_verts = _ptr(k['dv']), len(k['dv'])
    d.decor_indices, d.n_decor_indices = _ptr(k['di']), len(k['di'])
    d.draws, d.n_draws = _ptr(k['dr']), len(k['dr'])
    d.flat_atlas = _ptr(k['fa'])
    d.flat_w, d.flat_h = h2(k['fa'])
    d.wall_atlas = _ptr(k['wa'])
    d.wall_w, d.wall_h = h2(k['wa'])
    d.decor_atlas = _ptr(k['da'])
    d.decor_w, d.decor_h = h2(k['da'])
    d.sky_texture = _ptr(k['st'])
    d.sky_w, d.sky_h = h2(k['st'])
    d.sky_tiled_band_size = float(g('sky_band', 0.0))
    d.playpal, d.colormap = _ptr(k['pp']), _ptr(k['cm'])
    return d, keep


# ---- trait wad::LevelVisitor over the C ABI (include/rdoom.h: rdoom_visitor_vtbl) -----------------------------------
class LightInfo(ctypes.Structure):
    _fields_ = [('level', ctypes.c_float), ('has_effect', ctypes.c_int32), ('effect_kind', ctypes.c_int32),
                ('alt_level', ctypes.c_float), ('speed', ctypes.c_float), ('duration', ctypes.c_float), ('sync', ctypes.c_float)]


class StaticQuad(ctypes.Structure):
    _fields_ = [('object_id', ctypes.c_uint32), ('v1', ctypes.c_float * 2), ('v2', ctypes.c_float * 2),
                ('tex_start', ctypes.c_float * 2), ('tex_end', ctypes.c_float * 2), ('height_range', ctypes.c_float * 2),
                ('light_info', ctypes.POINTER(LightInfo)), ('scroll', ctypes.c_float), ('has_tex_name', ctypes.c_int32),
                ('tex_name', ctypes.c_uint8 * 8), ('blocker', ctypes.c_int32)]


class StaticPoly(ctypes.Structure):
    _fields_ = [('object_id', ctypes.c_uint32), ('vertices', ctypes.POINTER(ctypes.c_float)), ('n_vertices', ctypes.c_uint32),
                ('height', ctypes.c_float), ('light_info', ctypes.POINTER(LightInfo)), ('tex_name', ctypes.c_uint8 * 8)]


class SkyQuad(ctypes.Structure):
    _fields_ = [('object_id', ctypes.c_uint32), ('v1', ctypes.c_float * 2), ('v2', ctypes.c_float * 2),
                ('height_range', ctypes.c_float * 2)]


class SkyPoly(ctypes.Structure):
    _fields_ = [('object_id', ctypes.c_uint32), ('vertices', ctypes.POINTER(ctypes.c_float)), ('n_vertices', ctypes.c_uint32),
                ('height', ctypes.c_float)]


class Decor(ctypes.Structure):
    _fields_ = [('object_id', ctypes.c_uint32), ('low', ctypes.c_float * 3), ('high', ctypes.c_float * 3),
                ('half_width', ctypes.c_float), ('light_info', ctypes.POINTER(LightInfo)), ('tex_name', ctypes.c_uint8 * 8)]


class Line2f(ctypes.Structure):
    _fields_ = [('origin', ctypes.c_float * 2), ('displace', ctypes.c_float * 2), ('length', ctypes.c_float)]


_VP = ctypes.c_void_p
_VISITOR_SIGNATURES = [
    ('visit_wall_quad', (ctypes.POINTER(StaticQuad),)), ('visit_floor_poly', (ctypes.POINTER(StaticPoly),)),
    ('visit_ceil_poly', (ctypes.POINTER(StaticPoly),)), ('visit_floor_sky_poly', (ctypes.POINTER(SkyPoly),)),
    ('visit_ceil_sky_poly', (ctypes.POINTER(SkyPoly),)), ('visit_sky_quad', (ctypes.POINTER(SkyQuad),)),
    ('visit_marker', (ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.c_int32, ctypes.c_uint32)),
    ('visit_decor', (ctypes.POINTER(Decor),)), ('visit_bsp_root', (ctypes.POINTER(Line2f),)),
    ('visit_bsp_node', (ctypes.POINTER(Line2f), ctypes.c_int32)), ('visit_bsp_leaf', (ctypes.c_int32,)),
    ('visit_bsp_leaf_end', ()), ('visit_bsp_node_end', ())]
_VISITOR_TYPES = {name: ctypes.CFUNCTYPE(None, _VP, *args) for name, args in _VISITOR_SIGNATURES}


class VisitorVtbl(ctypes.Structure):
    _fields_ = [(name, _VISITOR_TYPES[name]) for name, _ in _VISITOR_SIGNATURES]


def make_visitor(obj):
    """rdoom_visitor_vtbl from any object: a method named like a callback of trait LevelVisitor (visitor.rs:65-116)
    receives the payload (ctypes structure pointers are dereferenced); missing methods stay NULL = the trait's default.
    Returns (vtbl, keepalive)."""
    vt, keep = VisitorVtbl(), []
    for name, args in _VISITOR_SIGNATURES:
        fn = getattr(obj, name, None)
        if fn is None:
            continue

        def thunk(_user, *a, _fn=fn):
            _fn(*[x.contents if hasattr(x, 'contents') and not isinstance(x, ctypes.POINTER(ctypes.c_float)) else x for x in a])
        cb = _VISITOR_TYPES[name](thunk)
        keep.append(cb)
        setattr(vt, name, cb)
    return vt, keep


def _close_quietly(obj):
    """__del__ of the handle classes: at interpreter shutdown the module's globals may already be gone"""
    try:
        obj.close()
    except Exception:
        pass


class Wad:
    """wad::Archive + TextureDirectory behind rdoom_wad_open (wad/src/archive.rs:36-60, tex.rs:53-107)."""

    def __init__(self, wad_path, metadata_path):
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_wad_open(os.fsencode(wad_path), os.fsencode(metadata_path), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().rdoom_wad_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def timings(self):
        """open_ms, textures_ms of rdoom_wad_open (single thread, steady clock inside the library)"""
        t = HostTimings()
        _check(lib().rdoom_wad_timings(self._h, ctypes.byref(t)))
        return {n: getattr(t, n) for n, _ in HostTimings._fields_}

    def num_levels(self):
        n = ctypes.c_uint32()
        _check(lib().rdoom_wad_num_levels(self._h, ctypes.byref(n)))
        return n.value

    def level_name(self, index):
        buf = ctypes.create_string_buffer(9)
        _check(lib().rdoom_wad_level_name(self._h, int(index), buf))
        return buf.value.decode('ascii')

    def build_level(self, index, gpu_tessellation=False, visitor=None):
        """visitor: an object with LevelVisitor methods, chained after the Builder (game/src/level.rs:378-382)"""
        return BuiltLevel(self, index, gpu_tessellation, visitor)

    def build_world(self, index, device=True):
        """game::world::WorldBuilder over level `index` (game/src/world.rs:211-409) -> World; device=False keeps it on the host"""
        return World(self, index, device)

    def build_world_set(self, indices, device=True):
        """a WorldSet of these archive levels (rdoom_worldset_create): slot s holds level indices[s]"""
        return WorldSet(self, indices, device)

    def walk(self, index, visitor):
        """WadSystem::walk (game/src/wad_system.rs:47-56) with the caller's visitor only"""
        vt, keep = make_visitor(visitor)
        _check(lib().rdoom_wad_walk(self._h, int(index), ctypes.byref(vt), None))
        del keep


class BuiltLevel:
    """Result of game::level::Builder::build + GameShaders::load_level."""

    def __init__(self, wad, index, gpu_tessellation=False, visitor=None):
        self._h = ctypes.c_void_p()
        self._wad = wad
        if visitor is None:
            _check(lib().rdoom_wad_build_level(wad._h, int(index), int(bool(gpu_tessellation)), ctypes.byref(self._h)))
        else:
            vt, keep = make_visitor(visitor)
            _check(lib().rdoom_wad_build_level_chained(wad._h, int(index), int(bool(gpu_tessellation)), ctypes.byref(vt), None,
                                                       ctypes.byref(self._h)))
            del keep
        self.desc = LevelDesc()
        _check(lib().rdoom_built_desc(self._h, ctypes.byref(self.desc)))

    def close(self):
        if self._h:
            lib().rdoom_built_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def _view(self, ptr, count, dtype):
        if not ptr or count == 0:
            return np.zeros(0, dtype)
        dt = np.dtype(dtype)
        buf = (ctypes.c_uint8 * (count * dt.itemsize)).from_address(ptr)
        return np.frombuffer(buf, dt, count).copy()

    def arrays(self):
        """Copies of every array of the descriptor, keyed like the oracle's BuiltLevel fields."""
        d = self.desc
        return dict(
            static_vertices=self._view(d.static_verts, d.n_static_verts, STATIC_VERTEX),
            static_indices=self._view(d.static_indices, d.n_static_indices, np.uint32),
            sky_vertices=self._view(d.sky_verts, d.n_sky_verts * 3, np.float32).reshape(-1, 3),
            sky_indices=self._view(d.sky_indices, d.n_sky_indices, np.uint32),
            decor_vertices=self._view(d.decor_verts, d.n_decor_verts, SPRITE_VERTEX),
            decor_indices=self._view(d.decor_indices, d.n_decor_indices, np.uint32),
            draws=self._view(d.draws, d.n_draws * 4, np.uint32).reshape(-1, 4),
            flat_atlas=self._view(d.flat_atlas, d.flat_w * d.flat_h, np.uint8).reshape(d.flat_h, d.flat_w),
            wall_atlas=self._view(d.wall_atlas, d.wall_w * d.wall_h, np.uint16).reshape(d.wall_h, d.wall_w),
            decor_atlas=self._view(d.decor_atlas, d.decor_w * d.decor_h, np.uint16).reshape(d.decor_h, d.decor_w),
            sky_texture=self._view(d.sky_texture, d.sky_w * d.sky_h, np.uint16).reshape(d.sky_h, d.sky_w),
            sky_band=np.float32(d.sky_tiled_band_size),
            palette=self._view(d.playpal, 768, np.uint8), colormap=self._view(d.colormap, 32 * 256, np.uint8))

    def counters(self):
        c = Counters()
        _check(lib().rdoom_built_counters(self._h, ctypes.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def timings(self):
        """level_lumps_ms, atlases_ms, analysis_ms, walk_ms of this build"""
        t = HostTimings()
        _check(lib().rdoom_built_timings(self._h, ctypes.byref(t)))
        return {n: getattr(t, n) for n, _ in HostTimings._fields_}

    def lights_at(self, time):
        out = np.zeros(256, np.uint8)
        _check(lib().rdoom_built_lights_at(self._h, ctypes.c_float(time), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def light_infos(self):
        """rdoom_built_light_infos: the level's Lights list in push order, as LIGHT_INFO records (entry i = light index i)"""
        p = ctypes.c_void_p()
        n = ctypes.c_uint32()
        _check(lib().rdoom_built_light_infos(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value, LIGHT_INFO)

    def start(self):
        pos = (ctypes.c_float * 3)()
        yaw = ctypes.c_float()
        _check(lib().rdoom_built_start(self._h, pos, ctypes.byref(yaw)))
        return np.array(pos[:], np.float32), np.float32(yaw.value)

    def floor_centroids(self):
        p = ctypes.c_void_p()
        n = ctypes.c_uint32()
        _check(lib().rdoom_built_floor_centroids(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value * 3, np.float32).reshape(-1, 3)

    def decor_things(self):
        """rdoom_built_decor_things: per decor quad q (decor vertices 4q .. 4q + 3), the index of its thing in the level's thing
        table (World.map_things of the same level); uint32, strictly increasing"""
        p = ctypes.c_void_p()
        n = ctypes.c_uint32()
        _check(lib().rdoom_built_decor_things(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self._view(p.value, n.value, np.uint32)


NO_THING = 0xFFFFFFFF  # RDOOM_NO_THING: a decor quad that no row of hidden things hides


def _set_decor_things(level, slot, table):
    table = np.ascontiguousarray(table, np.uint32).reshape(-1)
    _check(lib().rdoom_level_set_decor_things(level._h, int(slot), _ptr(table), len(table)))


class DeviceLevel:
    """Level arrays resident in HBM (replaces the GL vertex/index buffers and textures).  A BuiltLevel's decor_things() are
    attached at once, so that a Batch on it can hide things per pose (Batch.set_hidden_things); any other source attaches its
    own table with set_decor_things."""

    def __init__(self, source):
        if isinstance(source, BuiltLevel):
            desc, self._keep = source.desc, source
        elif isinstance(source, LevelDesc):
            desc, self._keep = source, None
        else:
            desc, self._keep = make_desc(source)
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_level_create(ctypes.byref(desc), ctypes.byref(self._h)))
        if isinstance(source, BuiltLevel):
            self.set_decor_things(source.decor_things())

    def set_decor_things(self, table):
        """rdoom_level_set_decor_things: table[q] is the thing-table index of decor quad q (decor vertices 4q .. 4q + 3), or
        NO_THING for a quad that is never hidden; one entry per quad.  Synchronous; replaces an earlier table."""
        _set_decor_things(self, 0, table)

    def num_objects(self):
        n = ctypes.c_uint32()
        _check(lib().rdoom_level_num_objects(self._h, ctypes.byref(n)))
        return n.value

    def close(self):
        if self._h:
            lib().rdoom_level_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)


class DeviceLevelSet(DeviceLevel):
    """Several levels resident in HBM as ONE handle (rdoom_levelset_create): a Batch created on it renders poses of different
    levels in one launch set (Batch.render(..., level_of_pose=...)).  `sources`: BuiltLevel / LevelDesc / array dicts."""

    def __init__(self, sources):
        descs, self._keep = [], []
        sources = list(sources)
        for source in sources:
            if isinstance(source, BuiltLevel):
                desc, keep = source.desc, source
            elif isinstance(source, LevelDesc):
                desc, keep = source, None
            else:
                desc, keep = make_desc(source)
            descs.append(desc)
            self._keep.append((desc, keep))
        arr = (ctypes.POINTER(LevelDesc) * len(descs))(*[ctypes.pointer(d) for d in descs])
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_levelset_create(arr, len(descs), ctypes.byref(self._h)))
        for slot, source in enumerate(sources):
            if isinstance(source, BuiltLevel):
                self.set_decor_things(slot, source.decor_things())

    def set_decor_things(self, slot, table):
        """rdoom_level_set_decor_things for level `slot` of the set (DeviceLevel.set_decor_things has the table)"""
        _set_decor_things(self, slot, table)

    def num_levels(self):
        n = ctypes.c_uint32()
        _check(lib().rdoom_level_num_levels(self._h, ctypes.byref(n)))
        return n.value


class DeviceLights:
    """The light infos of one or more levels resident on the device (rdoom_lightset_create): slot l holds levels[l], a BuiltLevel
    (its light_infos()) or an array of LIGHT_INFO records.  tables() evaluates every player's 256-byte light table at that
    player's own time on the GPU; Batch.render_players(states, device_lights, ..., times=...) renders with them."""

    def __init__(self, levels):
        if isinstance(levels, (BuiltLevel, np.ndarray)):
            levels = [levels]
        arrays = [np.ascontiguousarray(lv.light_infos() if isinstance(lv, BuiltLevel) else lv, LIGHT_INFO).reshape(-1) for lv in levels]
        self.n_levels = len(arrays)
        ptrs = (ctypes.c_void_p * max(1, len(arrays)))(*[_ptr(a) for a in arrays])
        counts = (ctypes.c_uint32 * max(1, len(arrays)))(*[len(a) for a in arrays])
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_lightset_create(ptrs, counts, len(arrays), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().rdoom_lightset_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def tables(self, times, levels=None, out=None, stream=None):
        """rdoom_lightset_tables: times a float32 GPU tensor of n entries; levels None (slot 0) or a GPU tensor of n 32-bit slots;
        out None or a contiguous uint8 GPU tensor of n * 256 entries.  Returns the (n, 256) uint8 tensor: row p is level
        levels[p]'s light table at times[p], zeros for a slot outside the set.  Asynchronous on `stream`."""
        import torch
        n = int(times.numel())
        pt = _times_tensor(times, n)
        pv = None
        if levels is not None:
            if not isinstance(levels, torch.Tensor) or levels.device.type != 'cuda' or not levels.is_contiguous() or \
                    levels.numel() != n or levels.element_size() != 4:
                raise ValueError('levels must be a contiguous GPU tensor of one 32-bit slot per player (%d)' % n)
            pv = levels.data_ptr()
        if out is None:
            out = torch.empty((n, 256), dtype=torch.uint8, device=times.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device.type != 'cuda' or not out.is_contiguous() \
                or out.numel() != n * 256:
            raise ValueError('out must be a contiguous uint8 GPU tensor of %d x 256 entries' % n)
        _check(lib().rdoom_lightset_tables(self._h, ctypes.c_void_p(pv), ctypes.c_void_p(pt), n,
                                           ctypes.c_void_p(out.data_ptr() if n else None), ctypes.c_void_p(_stream_handle(stream))))
        return out


class Batch:
    """A pose batch: device scratch + the three kernels (setup, tiled raster, fragment)."""

    def __init__(self, level, width, height, max_poses):
        self.level, self.width, self.height, self.max_poses = level, int(width), int(height), int(max_poses)
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_batch_create(level._h, self.width, self.height, self.max_poses, ctypes.byref(self._h)))
        self.last_n = 0
        self._hidden = None

    def close(self):
        if self._h:
            lib().rdoom_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    @staticmethod
    def _prep(poses, lights):
        poses = np.ascontiguousarray(poses, POSE).reshape(-1)
        lights = np.ascontiguousarray(lights, np.uint8)
        if lights.size == 256:
            stride = 0
        else:
            assert lights.size == 256 * len(poses), 'lights must be (256,) or (n_poses, 256)'
            stride = 256
        return poses, lights, stride

    def _render_levels(self, poses, lights, stride, kinds, stream, level_of_pose, object_modelviews, profiled):
        lop = np.ascontiguousarray(level_of_pose, np.uint32).reshape(-1)
        assert len(lop) == len(poses), 'level_of_pose: one level index per pose'
        om, n_obj = None, 0
        if object_modelviews is not None:
            om = np.ascontiguousarray(object_modelviews, np.float32).reshape(len(poses), -1, 16)
            n_obj = om.shape[1]
        _check(lib().rdoom_batch_render_levels(
            self._h, poses.ctypes.data_as(ctypes.c_void_p), lop.ctypes.data_as(ctypes.c_void_p), lights.ctypes.data_as(ctypes.c_void_p),
            stride, len(poses), int(kinds), ctypes.c_void_p(stream or 0), om.ctypes.data_as(ctypes.c_void_p) if om is not None else None,
            n_obj, 1 if profiled else 0))

    def render_profiled(self, poses, lights, kinds=ALL_KINDS, stream=None, level_of_pose=None):
        """rdoom_batch_render_profiled: asynchronous, the per-kernel events stay pending (at most 64 renders)"""
        poses, lights, stride = self._prep(poses, lights)
        self.last_n = self._rows_for(len(poses))
        if level_of_pose is not None:
            return self._render_levels(poses, lights, stride, kinds, stream, level_of_pose, None, True)
        _check(lib().rdoom_batch_render_profiled(self._h, poses.ctypes.data_as(ctypes.c_void_p), lights.ctypes.data_as(ctypes.c_void_p),
                                                 stride, len(poses), int(kinds), ctypes.c_void_p(stream or 0)))

    def collect_timings(self):
        """rdoom_batch_collect_timings: sums over the pending profiled renders + their number"""
        t, n = Timings(), ctypes.c_uint32()
        _check(lib().rdoom_batch_collect_timings(self._h, ctypes.byref(t), ctypes.byref(n)))
        out = {k: getattr(t, k) for k, _ in Timings._fields_}
        out['renders'] = n.value
        return out

    def render(self, poses, lights, kinds=ALL_KINDS, stream=None, timed=False, object_modelviews=None, level_of_pose=None):
        """rdoom_batch_render(_timed): asynchronous unless timed; returns Timings fields when timed.
        object_modelviews: optional (n_poses, n_objects, 16) u_modelview per object -> rdoom_batch_render_objects.
        level_of_pose: (n_poses,) level index of every pose, for a batch on a DeviceLevelSet -> rdoom_batch_render_levels."""
        poses, lights, stride = self._prep(poses, lights)
        self.last_n = self._rows_for(len(poses))
        if level_of_pose is not None:
            assert not timed, 'timed renders of a level set: use render_profiled + collect_timings'
            return self._render_levels(poses, lights, stride, kinds, stream, level_of_pose, object_modelviews, False)
        if object_modelviews is not None:
            om = np.ascontiguousarray(object_modelviews, np.float32).reshape(len(poses), -1, 16)
            _check(lib().rdoom_batch_render_objects(
                self._h, poses.ctypes.data_as(ctypes.c_void_p), lights.ctypes.data_as(ctypes.c_void_p), stride,
                len(poses), int(kinds), ctypes.c_void_p(stream or 0), om.ctypes.data_as(ctypes.c_void_p), om.shape[1]))
            return None
        args = (self._h, poses.ctypes.data_as(ctypes.c_void_p), lights.ctypes.data_as(ctypes.c_void_p), stride,
                len(poses), int(kinds), ctypes.c_void_p(stream or 0))
        if not timed:
            _check(lib().rdoom_batch_render(*args))
            return None
        t = Timings()
        _check(lib().rdoom_batch_render_timed(*args, ctypes.byref(t)))
        return {n: getattr(t, n) for n, _ in Timings._fields_}

    def render_players(self, states, lights, levels=None, offsets=None, time=0.0, kinds=ALL_KINDS, stream=None, poses_out=None,
                       modelviews_out=None, profiled=False, times=None):
        """rdoom_batch_render_players: render every player of a device states tensor (World.step_game / WorldSet.step_game's) from its
        own camera, without a host round trip.  levels: the players' level slots (WorldSet.game_state's int32 tensor; None on a
        batch of one level); offsets: the (n, n_objects, 3) float32 tensor of game_state (None: every object at rest); lights: a
        uint8 (256,) table shared by every level, or (n_levels, 256), one per level of the batch's set.  Tensors on the GPU are used
        as they are; numpy arrays are uploaded (and waited for).  poses_out / modelviews_out: optional tensors from
        poses_from_players_device's shapes, filled with what was rendered.  Asynchronous on `stream`; profiled as render_profiled.
        The clocked render (rdoom_batch_render_players_clocked): times, a float32 GPU tensor of n entries, with lights a
        DeviceLights -- player p is rendered at times[p] with its level's light table at that time, computed on the device; `time`
        is not used.  times without a DeviceLights, or a DeviceLights without times, is a ValueError."""
        if (times is not None) != isinstance(lights, DeviceLights):
            raise ValueError('the clocked render takes times and a DeviceLights together (times: %s, lights: %s)'
                             % ('given' if times is not None else 'None', type(lights).__name__))
        keep = []

        def dev(a, what):
            if a is None:
                return None
            ptr, k, uploaded = _device_tensor(a, what)
            keep.append((k, uploaded))
            return ptr
        ps, n = dev(states, 'states'), _n_players(states)
        if times is None:
            lights_n = lights.numel() if not isinstance(lights, np.ndarray) else lights.size
            n_levels = ctypes.c_uint32()
            _check(lib().rdoom_level_num_levels(self.level._h, ctypes.byref(n_levels)))
            if lights_n == 256:
                stride = 0
            elif lights_n == 256 * n_levels.value:
                stride = 256
            else:
                raise ValueError('lights must be (256,) or one 256-byte table per level of the set (%d), got %d bytes'
                                 % (n_levels.value, lights_n))
            pl = dev(np.ascontiguousarray(lights, np.uint8) if isinstance(lights, np.ndarray) else lights, 'lights')
        else:
            pt = _times_tensor(times, n)
        n_obj = 0
        if offsets is not None:
            if isinstance(offsets, np.ndarray):
                offsets = np.ascontiguousarray(offsets, np.float32)
            if tuple(offsets.shape[::2]) != (n, 3) or len(offsets.shape) != 3:
                raise ValueError('offsets must be (n, n_objects, 3) for %d players, got %s' % (n, tuple(offsets.shape)))
            n_obj = int(offsets.shape[1])
        if levels is not None:
            if isinstance(levels, np.ndarray):
                levels = np.ascontiguousarray(levels, np.int64).astype(np.uint32)
            size = levels.size if isinstance(levels, np.ndarray) else levels.numel()
            item = levels.itemsize if isinstance(levels, np.ndarray) else levels.element_size()
            if size != n or item != 4:
                raise ValueError('levels must hold one 32-bit slot per player (%d)' % n)
        po, pm = _out_tensor(poses_out, n * POSE.itemsize, 'poses_out'), _out_tensor(modelviews_out, n * n_obj * 64, 'modelviews_out')
        pv, po_ = dev(levels, 'levels'), dev(offsets, 'offsets')
        self.last_n = self._rows_for(n)
        if times is None:
            _check(lib().rdoom_batch_render_players(self._h, ctypes.c_void_p(ps), ctypes.c_void_p(pv), ctypes.c_void_p(po_), n_obj,
                                                    ctypes.c_void_p(pl), stride, ctypes.c_float(time), n, int(kinds),
                                                    1 if profiled else 0, ctypes.c_void_p(_stream_handle(stream)), ctypes.c_void_p(po),
                                                    ctypes.c_void_p(pm)))
        else:
            _check(lib().rdoom_batch_render_players_clocked(self._h, ctypes.c_void_p(ps), ctypes.c_void_p(pv), ctypes.c_void_p(po_),
                                                            n_obj, lights._h, ctypes.c_void_p(pt), n, int(kinds), 1 if profiled else 0,
                                                            ctypes.c_void_p(_stream_handle(stream)), ctypes.c_void_p(po),
                                                            ctypes.c_void_p(pm)))
        if any(uploaded for _, uploaded in keep):
            import torch
            torch.cuda.synchronize()

    def _rows_for(self, n):
        """n, once the tensor given to set_hidden_things is known to hold a row for each of a render's n poses"""
        rows = self._hidden
        if rows is not None and not isinstance(rows, (int, np.integer)) and int(rows.shape[0]) < n:
            raise ValueError('the hidden-things tensor has %d rows, the render %d poses' % (int(rows.shape[0]), n))
        return n

    def set_hidden_things(self, rows, stride=None):
        """rdoom_batch_set_hidden_things: every following render of this batch leaves out, for pose or player p, the decor
        triangles of the things whose bit is set in row p of `rows` -- sense_things' `collected` tensor as it stands: a 32-bit
        integer (n, words) GPU tensor, read on the render's stream when the render runs, so a sense_things queued before the
        render on that stream is seen without a wait.  Or a raw device pointer (an int) with `stride`, the words of a row.  The
        batch keeps a reference to the tensor.  None switches it off.  The level needs its decor things attached
        (DeviceLevel.set_decor_things; a BuiltLevel's are)."""
        if rows is None:
            _check(lib().rdoom_batch_set_hidden_things(self._h, None, 0))
            self._hidden = None
            return
        if isinstance(rows, (int, np.integer)):
            if stride is None:
                raise ValueError('stride is needed with a raw pointer')
            ptr = int(rows)
        else:
            if rows.device.type != 'cuda' or not rows.is_contiguous() or rows.element_size() != 4 or rows.dtype.is_floating_point \
                    or rows.dim() != 2:
                raise ValueError('rows must be a contiguous 32-bit integer (n, words) tensor on the GPU')
            if stride is None:
                stride = int(rows.shape[1])
            elif int(stride) != int(rows.shape[1]):
                raise ValueError('stride %d, but the rows are %d words long' % (int(stride), int(rows.shape[1])))
            ptr = rows.data_ptr()
        _check(lib().rdoom_batch_set_hidden_things(self._h, ctypes.c_void_p(ptr), int(stride)))
        self._hidden = rows

    def finish(self):
        """rdoom_batch_finish: wait for the last render and raise if the device found a problem"""
        _check(lib().rdoom_batch_finish(self._h))

    def framebuffer_device_ptr(self):
        p = ctypes.c_void_p()
        _check(lib().rdoom_batch_framebuffer_device(self._h, ctypes.byref(p)))
        return p.value

    def path_stats(self):
        """rdoom_batch_path_stats: which paths the last render took (overflowed poses, split tile lists, described quadrants)"""
        s = PathStats()
        _check(lib().rdoom_batch_path_stats(self._h, ctypes.byref(s)))
        return {n: getattr(s, n) for n, _ in PathStats._fields_}

    def framebuffer_pitch(self):
        """bytes between rows of the device framebuffer (the width, or the next multiple of 8 when width % 4 != 0)"""
        n = ctypes.c_uint32()
        _check(lib().rdoom_batch_framebuffer_pitch(self._h, ctypes.byref(n)))
        return n.value

    def read_framebuffer(self, first=0, count=None):
        count = self.last_n - first if count is None else count
        out = np.zeros((count, self.height, self.width), np.uint8)
        _check(lib().rdoom_batch_read_framebuffer(self._h, int(first), int(count), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def _rgb_args(self, first, count, alpha, top_down):
        count = self.last_n - first if count is None else count
        fmt = (RGBA8 if alpha else RGB8) | (RGB_TOP_DOWN if top_down else 0)
        return int(first), int(count), fmt, (int(count), self.height, self.width, 4 if alpha else 3)

    def read_rgb(self, first=0, count=None, alpha=False, top_down=False):
        """rdoom_batch_read_rgb: frames [first, first+count) of the last render as (count, H, W, 3) RGB8 -- (.., 4) RGBA8 with
        alpha=True (255 drawn, 0 clear) -- PLAYPAL 0 where a primitive was drawn, CLEAR_RGB elsewhere; row 0 = the bottom row
        (glReadPixels order) unless top_down"""
        first, count, fmt, shape = self._rgb_args(first, count, alpha, top_down)
        out = np.zeros(shape, np.uint8)
        _check(lib().rdoom_batch_read_rgb(self._h, first, count, fmt, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def resolve_rgb(self, out, first=0, count=None, alpha=False, top_down=False, stream=None):
        """rdoom_batch_resolve_rgb: the same frames written to device memory, asynchronously on `stream` (a hipStream_t handle,
        or a torch stream; None = the null stream).  out: a raw device pointer (int) of count*H*W*(3|4) bytes, or a contiguous
        uint8 torch tensor of that many elements on the batch's device.  Returns out."""
        first, count, fmt, shape = self._rgb_args(first, count, alpha, top_down)
        ptr = _resolve_out(out, ('uint8',), shape, first, count)
        _check(lib().rdoom_batch_resolve_rgb(self._h, first, count, fmt, ctypes.c_void_p(ptr or None), ctypes.c_void_p(_stream_handle(stream))))
        return out

    def _plane_args(self, plane, first, count, top_down):
        if plane not in PLANE_DTYPES:
            raise ValueError('plane must be PLANE_DEPTH, PLANE_LABEL or PLANE_PRIMITIVE, not %r' % (plane,))
        count = self.last_n - first if count is None else count
        return int(first), int(count), int(plane) | (RGB_TOP_DOWN if top_down else 0), (int(count), self.height, self.width)

    def read_plane(self, plane, first=0, count=None, top_down=False):
        """rdoom_batch_read_plane: one per-pixel plane of frames [first, first+count) of the last render as (count, H, W) --
        PLANE_DEPTH float32 (the winning fragment's view-space depth in world units, +inf for sky and where nothing was drawn),
        PLANE_LABEL uint16 (kind | object id << 4, LABEL_NONE where nothing was drawn), PLANE_PRIMITIVE uint32 (what
        read_primitive_ids reports, without enable_primitive_ids); row 0 = the bottom row unless top_down"""
        first, count, arg, shape = self._plane_args(plane, first, count, top_down)
        out = np.zeros(shape, PLANE_DTYPES[plane])
        _check(lib().rdoom_batch_read_plane(self._h, first, count, arg, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def resolve_plane(self, out, plane, first=0, count=None, top_down=False, stream=None):
        """rdoom_batch_resolve_plane: the same plane written to device memory, asynchronously on `stream` (a hipStream_t handle,
        or a torch stream; None = the null stream).  out: a raw device pointer (int) of count*H*W elements, or a contiguous torch
        tensor of the plane's dtype (float32 / uint16 / uint32; int16 / int32 are taken as their bits) with that many elements
        on the batch's device.  Returns out."""
        first, count, arg, shape = self._plane_args(plane, first, count, top_down)
        names = {PLANE_DEPTH: ('float32',), PLANE_LABEL: ('uint16', 'int16'), PLANE_PRIMITIVE: ('uint32', 'int32')}[plane]
        ptr = _resolve_out(out, names, shape, first, count)
        _check(lib().rdoom_batch_resolve_plane(self._h, first, count, arg, ctypes.c_void_p(ptr or None), ctypes.c_void_p(_stream_handle(stream))))
        return out

    def read_thing_plane(self, first=0, count=None, top_down=False):
        """rdoom_batch_read_thing_plane (include/rdoom_frame_things.h): per pixel of frames [first, first+count) of the last render
        the index, in the thing table of the pose's level, of the thing whose decor quad shows there, -1 everywhere else (flats,
        walls, sky, nothing drawn, decor of NO_THING, a level handle without set_decor_things) as (count, H, W) int32; row 0 =
        the bottom row unless top_down.  Things hidden by set_hidden_things were not drawn and do not appear."""
        count = self.last_n - first if count is None else count
        out = np.zeros((int(count), self.height, self.width), np.int32)
        _check(lib().rdoom_batch_read_thing_plane(self._h, int(first), int(count), RGB_TOP_DOWN if top_down else 0,
                                                  out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def resolve_thing_plane(self, out, first=0, count=None, top_down=False, stream=None):
        """rdoom_batch_resolve_thing_plane: the same plane written to device memory, asynchronously on `stream` (a hipStream_t
        handle, or a torch stream; None = the null stream).  out: a raw device pointer (int) of count*H*W int32, or a contiguous
        torch.int32 tensor with that many elements on the batch's device.  Returns out; frame_things reduces it."""
        count = self.last_n - first if count is None else count
        first, count = int(first), int(count)
        ptr = _resolve_out(out, ('int32',), (count, self.height, self.width), first, count)
        _check(lib().rdoom_batch_resolve_thing_plane(self._h, first, count, RGB_TOP_DOWN if top_down else 0, ctypes.c_void_p(ptr or None),
                                                     ctypes.c_void_p(_stream_handle(stream))))
        return out

    def read_depth(self, first=0, count=None, top_down=False):
        """read_plane(PLANE_DEPTH, ...): (count, H, W) float32"""
        return self.read_plane(PLANE_DEPTH, first, count, top_down)

    def resolve_depth(self, out, first=0, count=None, top_down=False, stream=None):
        """resolve_plane(out, PLANE_DEPTH, ...): out a float32 tensor (or device pointer) of count*H*W elements"""
        return self.resolve_plane(out, PLANE_DEPTH, first, count, top_down, stream)

    def _observation_args(self, format, factor, first, count, top_down):
        shape = observation_shape(format, self.width, self.height, factor)
        fx, fy = _factors(factor)
        count = self.last_n - first if count is None else count
        return int(first), int(count), int(format) | (RGB_TOP_DOWN if top_down else 0), fx, fy, (int(count),) + shape

    def read_observation(self, format=OBS_RGB8, factor=4, first=0, count=None, top_down=False):
        """rdoom_batch_read_observation: frames [first, first+count) of the last render reduced by `factor` (an int or (fx, fy),
        each 1, 2, 4 or 8) as (count,) + observation_shape(format, W, H, factor): the exact mean colour of every cell (OBS_RGB8,
        OBS_RGB8_PLANAR), its grey value (OBS_GRAY8) or its smallest depth (OBS_DEPTH_MIN, float32); row 0 = the bottom row of
        cells unless top_down"""
        first, count, fmt, fx, fy, shape = self._observation_args(format, factor, first, count, top_down)
        out = np.zeros(shape, OBS_DTYPES[format])
        _check(lib().rdoom_batch_read_observation(self._h, first, count, fmt, fx, fy, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def resolve_observation(self, out, format=OBS_RGB8, factor=4, first=0, count=None, top_down=False, stream=None):
        """rdoom_batch_resolve_observation: the same observations written to device memory, asynchronously on `stream` (a
        hipStream_t handle, or a torch stream; None = the null stream).  out: a raw device pointer (int), or a contiguous torch
        tensor on the batch's device with count * prod(observation_shape(...)) elements -- uint8 for the colour formats, float32
        for OBS_DEPTH_MIN.  Returns out."""
        first, count, fmt, fx, fy, shape = self._observation_args(format, factor, first, count, top_down)
        ptr = _resolve_out(out, ('float32',) if format == OBS_DEPTH_MIN else ('uint8',), shape, first, count)
        _check(lib().rdoom_batch_resolve_observation(self._h, first, count, fmt, fx, fy, ctypes.c_void_p(ptr or None),
                                                     ctypes.c_void_p(_stream_handle(stream))))
        return out

    def enable_primitive_ids(self):
        _check(lib().rdoom_batch_enable_primitive_ids(self._h))

    def read_primitive_ids(self, first=0, count=None):
        count = self.last_n - first if count is None else count
        out = np.zeros((count, self.height, self.width), np.uint32)
        _check(lib().rdoom_batch_read_primitive_ids(self._h, int(first), int(count),
                                                    out.ctypes.data_as(ctypes.c_void_p)))
        return out


# ---- the collision world + player physics (include/rdoom.h: rdoom_world_*, rdoom_player_*) ----------------------------------
class WorldArrays(ctypes.Structure):
    _fields_ = [('nodes', ctypes.c_void_p), ('n_nodes', ctypes.c_uint32), ('chunks', ctypes.c_void_p), ('n_chunks', ctypes.c_uint32),
                ('triangles', ctypes.c_void_p), ('n_triangles', ctypes.c_uint32), ('n_static_triangles', ctypes.c_uint32),
                ('verts', ctypes.c_void_p), ('n_verts', ctypes.c_uint32), ('dynamics', ctypes.c_void_p), ('n_dynamics', ctypes.c_uint32),
                ('n_objects', ctypes.c_uint32), ('node_depth', ctypes.c_uint32)]


class WorldTriggerArrays(ctypes.Structure):
    _fields_ = [('triggers', ctypes.c_void_p), ('n_triggers', ctypes.c_uint32), ('effects', ctypes.c_void_p), ('n_effects', ctypes.c_uint32),
                ('n_objects', ctypes.c_uint32)]


WORLD_NODE = np.dtype([('origin', '<f4', 2), ('displace', '<f4', 2), ('length', '<f4'), ('positive', '<i4'), ('negative', '<i4')])


def _world_arrays(a):
    """World.arrays and WorldSet.arrays: copies of a WorldArrays' arrays"""
    v = BuiltLevel._view
    return dict(nodes=v(None, a.nodes, a.n_nodes, WORLD_NODE), chunks=v(None, a.chunks, a.n_chunks * 2, np.uint32).reshape(-1, 2),
                triangles=v(None, a.triangles, a.n_triangles * 4, np.uint32).reshape(-1, 4),
                verts=v(None, a.verts, a.n_verts * 3, np.float32).reshape(-1, 3),
                dynamics=v(None, a.dynamics, a.n_dynamics * 3, np.uint32).reshape(-1, 3),
                n_static_triangles=a.n_static_triangles, n_objects=a.n_objects, node_depth=a.node_depth)


def _trigger_arrays(a):
    """World.triggers and WorldSet.triggers: copies of a WorldTriggerArrays' arrays"""
    v = BuiltLevel._view
    return dict(triggers=v(None, a.triggers, a.n_triggers, TRIGGER), effects=v(None, a.effects, a.n_effects, MOVE_EFFECT),
                n_objects=a.n_objects)


def player_config_default():
    """rdoom_player_config_default: Config::default's physics half (game/src/player.rs:73-92) as a PLAYER_CONFIG record"""
    cfg = np.zeros(1, PLAYER_CONFIG)
    _check(lib().rdoom_player_config_default(cfg.ctypes.data_as(ctypes.c_void_p)))
    return cfg[0]


def player_states(positions, yaws, pitch=1e-8, flags=PLAYER_CLIP):
    """PLAYER_STATE records at rest, as Player::reset leaves them (player.rs:118-133: pitch 1e-8, no velocity); flags: PLAYER_CLIP
    (the reference's default) and / or PLAYER_FLY, a scalar or one per player"""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.zeros(len(pos), PLAYER_STATE)
    out['pos'] = pos
    out['yaw'] = np.broadcast_to(np.asarray(yaws, np.float32), len(pos))
    out['pitch'] = np.broadcast_to(np.asarray(pitch, np.float32), len(pos))
    out['flags'] = np.broadcast_to(np.asarray(flags, np.uint32), len(pos))
    return out


def poses_from_players(states, width, height, time=0.0):
    """the camera of every player (rdoom_pose_from_player: the head at pos + 0.12, rotated by (yaw, pitch)) as a POSE array --
    step, then this, then Batch.render"""
    states = np.asarray(states, PLAYER_STATE).reshape(-1)
    return np.array([pose_from_player(s['pos'], float(s['yaw']), float(s['pitch']), width, height, time) for s in states], POSE)


def object_modelviews_from_players(states, offsets):
    """the u_modelview of every object in every player's frame (rdoom_object_modelviews_from_player): states PLAYER_STATE records,
    offsets (n, n_objects, 3) (numpy or a torch tensor, e.g. World.step_game's) -> (n, n_objects, 16) float32, ready for
    Batch.render(object_modelviews=...)"""
    states = np.asarray(states, PLAYER_STATE).reshape(-1)
    if not isinstance(offsets, np.ndarray):
        offsets = offsets.detach().cpu().numpy()
    offsets = np.ascontiguousarray(offsets, np.float32)
    if offsets.ndim != 3 or offsets.shape[0] != len(states) or offsets.shape[2] != 3:
        raise ValueError('offsets must be (n, n_objects, 3) for %d players, got %s' % (len(states), offsets.shape))
    n_obj = offsets.shape[1]
    out = np.zeros((len(states), n_obj, 16), np.float32)
    for i, s in enumerate(states):
        pos = np.ascontiguousarray(s['pos'], np.float32)
        _check(lib().rdoom_object_modelviews_from_player(pos.ctypes.data_as(ctypes.c_void_p), ctypes.c_float(s['yaw']),
                                                         ctypes.c_float(s['pitch']), offsets[i].ctypes.data_as(ctypes.c_void_p), n_obj,
                                                         out[i].ctypes.data_as(ctypes.c_void_p)))
    return out


def _n_players(states):
    size = states.nbytes if isinstance(states, np.ndarray) else states.numel() * states.element_size()
    if size == 0 or size % PLAYER_STATE.itemsize:
        raise ValueError('states must hold n >= 1 records of %d bytes' % PLAYER_STATE.itemsize)
    return size // PLAYER_STATE.itemsize


def _out_tensor(t, nbytes, what):
    """the device pointer of an optional output tensor of exactly nbytes"""
    if t is None:
        return None
    if t.device.type != 'cuda' or not t.is_contiguous() or t.numel() * t.element_size() != nbytes:
        raise ValueError('%s must be a contiguous GPU tensor of %d bytes' % (what, nbytes))
    return t.data_ptr()


def _times_tensor(times, n):
    """the device pointer of a clocked call's times: a contiguous float32 GPU tensor of n entries"""
    import torch
    if not isinstance(times, torch.Tensor) or times.dtype != torch.float32 or times.device.type != 'cuda' or \
            not times.is_contiguous() or times.numel() != n:
        raise ValueError('times must be a contiguous float32 tensor of %d entries on the GPU' % n)
    return times.data_ptr()


def poses_from_players_device(states, width, height, time=0.0, offsets=None, stream=None, times=None):
    """rdoom_poses_from_players_device: the camera of every player, on the device.  states: a GPU tensor of PLAYER_STATE records
    (numpy: uploaded); offsets: None or the (n, n_objects, 3) float32 tensor of game_state.  Returns (poses, modelviews): poses a
    float32 (n, 34) tensor of POSE records (.cpu().numpy().view(POSE)), modelviews None or a float32 (n, n_objects, 16) tensor --
    what poses_from_players / object_modelviews_from_players compute on the host, with the project's sincos.
    times: None, or a float32 GPU tensor of n entries -- pose p's time is times[p] instead of `time`
    (rdoom_poses_from_players_device_clocked).  Asynchronous on `stream`."""
    import torch
    n = _n_players(states)
    ps, ks, uploaded = _device_tensor(states, 'states')
    dev = ks.device
    poses = torch.empty((n, POSE.itemsize // 4), dtype=torch.float32, device=dev)
    mvs, po, n_obj, ko = None, None, 0, None
    if offsets is not None:
        if isinstance(offsets, np.ndarray):
            offsets = np.ascontiguousarray(offsets, np.float32)
        if len(offsets.shape) != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be (n, n_objects, 3) for %d players, got %s' % (n, tuple(offsets.shape)))
        po, ko, up2 = _device_tensor(offsets, 'offsets')
        uploaded = uploaded or up2
        n_obj = int(offsets.shape[1])
        mvs = torch.empty((n, n_obj, 16), dtype=torch.float32, device=dev)
    tail = (ctypes.c_void_p(po), n_obj, ctypes.c_void_p(poses.data_ptr()), ctypes.c_void_p(mvs.data_ptr() if mvs is not None else None),
            ctypes.c_void_p(_stream_handle(stream)))
    if times is None:
        _check(lib().rdoom_poses_from_players_device(ctypes.c_void_p(ps), n, int(width), int(height), ctypes.c_float(time), *tail))
    else:
        _check(lib().rdoom_poses_from_players_device_clocked(ctypes.c_void_p(ps), n, int(width), int(height),
                                                             ctypes.c_void_p(_times_tensor(times, n)), *tail))
    if uploaded:
        torch.cuda.synchronize(dev)
    return poses, mvs


def _stream_handle(stream):
    """a hipStream_t handle (int), a torch stream, or None: the null stream"""
    if stream is None or isinstance(stream, int):
        return stream or 0
    return stream.cuda_stream


def _resolve_out(out, names, shape, first, count):
    """The `out` of Batch.resolve_*, as a device pointer: an int as it stands, or a contiguous GPU tensor of one of the torch dtypes
    `names` with prod(shape) elements -- what frames [first, first+count) need"""
    if isinstance(out, int):
        return out
    import torch  # (only here: the package imports without torch)
    if not isinstance(out, torch.Tensor):
        raise TypeError('out must be a device pointer (int) or a torch tensor, not %s' % type(out).__name__)
    ok = [getattr(torch, n) for n in names if hasattr(torch, n)]
    if out.dtype not in ok or not out.is_contiguous() or out.device.type != 'cuda':
        raise ValueError('out must be a contiguous %s tensor on the GPU (got %s, %s, contiguous=%s)'
                         % (' / '.join('torch.' + n for n in names), out.dtype, out.device, out.is_contiguous()))
    need = int(np.prod(shape))
    if out.numel() != need:
        raise ValueError('out has %d elements, frames %d..%d need %s = %d' % (out.numel(), first, first + count, shape, need))
    return out.data_ptr()  # (the library checks that it lives on the batch's device)


def _device_tensor(a, what):
    """(device pointer, keepalive, is_numpy): a torch tensor on the GPU is used as it is; a numpy array is copied to the current one"""
    import torch  # (only here: the package imports without torch)
    if isinstance(a, torch.Tensor):
        if a.device.type != 'cuda' or not a.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU (got %s, contiguous=%s)' % (what, a.device, a.is_contiguous()))
        return a.data_ptr(), a, False
    raw = np.ascontiguousarray(a)
    t = torch.from_numpy(raw.view(np.uint8).reshape(-1).copy()).cuda()
    return t.data_ptr(), t, True


class _GameStepArgs:
    """the arguments of a step (World.step, World.step_game, WorldSet.step_game), checked and on the device: states
    PLAYER_STATE records (numpy: a stepped copy is returned) or a GPU tensor of n * 40 bytes (stepped in place); inputs
    (n_ticks, n) PLAYER_INPUT records, or a GPU tensor with n_ticks given; actions None or (n_ticks, n) ACTION_* bytes; config a
    PLAYER_CONFIG or None"""

    def __init__(self, states, inputs, actions, n_ticks, config):
        if isinstance(actions, np.ndarray):
            actions = np.ascontiguousarray(actions)
            if actions.size and int(actions.max()) > ACTION_SHOOT:
                raise RdoomError(-1, 'action %d is not ACTION_NONE / ACTION_PUSH / ACTION_SHOOT' % int(actions.max()))
            actions = actions.astype(np.uint8)
        self.is_np = isinstance(states, np.ndarray)
        if self.is_np:
            states = np.ascontiguousarray(states, PLAYER_STATE).reshape(-1)
            n = len(states)
        else:
            if states.numel() * states.element_size() % PLAYER_STATE.itemsize:
                raise ValueError('a states tensor must hold n * %d bytes' % PLAYER_STATE.itemsize)
            n = states.numel() * states.element_size() // PLAYER_STATE.itemsize
        if isinstance(inputs, np.ndarray):
            inputs = np.ascontiguousarray(inputs, PLAYER_INPUT)
            inputs = inputs.reshape(-1, n) if inputs.size else inputs.reshape(0, n)
            if n_ticks is not None and n_ticks != inputs.shape[0]:
                raise ValueError('n_ticks %d, but inputs for %d ticks' % (n_ticks, inputs.shape[0]))
            n_ticks = inputs.shape[0]
        elif n_ticks is None:
            raise ValueError('n_ticks is needed with an input tensor')
        if actions is not None:
            size = actions.size if isinstance(actions, np.ndarray) else actions.numel() * actions.element_size()
            if size != n_ticks * n:
                raise ValueError('actions must be (n_ticks, n) = (%d, %d) bytes, got %d' % (n_ticks, n, size))
        self.states, self.n, self.n_ticks, self.actions = states, n, n_ticks, actions
        self.ps, self.ks, _ = _device_tensor(states, 'states')
        self.pi, self.ki, _ = _device_tensor(inputs, 'inputs')
        self.pa, self.ka = None, None
        if actions is not None:
            self.pa, self.ka, _ = _device_tensor(actions, 'actions')
        self.cfg = None
        if config is not None:
            self.cfg = np.ascontiguousarray(np.asarray(config, PLAYER_CONFIG).reshape(1))

    def cfg_ptr(self):
        return self.cfg.ctypes.data_as(ctypes.c_void_p) if self.cfg is not None else None

    def result(self):
        """after the launch: the states tensor, or a stepped numpy copy"""
        if self.is_np or isinstance(self.actions, np.ndarray):  # (numpy actions: their upload is freed on return)
            import torch
            torch.cuda.synchronize(self.ks.device)
        return self.ks.cpu().numpy().view(PLAYER_STATE).copy() if self.is_np else self.states


def _game_args(game_bytes, game, offsets, *levels, players=None):
    """(n, n_objects) of a game's device tensors, checked: game (n * game_bytes bytes), offsets and a world set's levels (a world
    passes none); n must be `players` when given (a step's)"""
    import torch
    for t, what in zip((game, offsets) + levels, ('game', 'offsets', 'levels')):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[2] != 3:
        raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor, got %s %s' % (offsets.dtype, tuple(offsets.shape)))
    n = int(offsets.shape[0])
    if game.numel() * game.element_size() != n * game_bytes:
        raise ValueError('the game state must hold %d players x %d bytes' % (n, game_bytes))
    for lv in levels:
        if lv.element_size() != 4 or lv.numel() != n:
            raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, lv.dtype, tuple(lv.shape)))
    if players is not None and n != players:
        raise ValueError('%d players, but game state and offsets for %d' % (players, n))
    return n, int(offsets.shape[1])


def _reset_masked(mask, reset):
    """reset_game's call reset(mask pointer): mask None (every player), or n bools / bytes, numpy (copied to the device) or a GPU
    tensor; returns once the launch no longer reads the mask's memory"""
    pm, km = None, None
    if mask is not None:
        if isinstance(mask, np.ndarray):
            mask = np.ascontiguousarray(mask).astype(np.uint8)
        pm, km, _ = _device_tensor(mask, 'mask')
    _check(reset(ctypes.c_void_p(pm)))
    if km is not None:
        import torch
        torch.cuda.synchronize(km.device)


def ray_fan(n_rays, fov, pitch=0.0):
    """a direction table for cast_rays: n_rays unit directions in the camera frame (-z forward), evenly spaced in yaw across `fov`
    radians and centred on -z (ray 0 is the leftmost, at +fov / 2; an odd n_rays has a ray straight ahead), all raised by `pitch` radians"""
    n_rays = int(n_rays)
    if n_rays < 1:
        raise ValueError('n_rays must be at least 1')
    yaw = np.linspace(0.5 * fov, -0.5 * fov, n_rays) if n_rays > 1 else np.zeros(1)
    cp, sp = np.cos(float(pitch)), np.sin(float(pitch))
    return np.stack([-np.sin(yaw) * cp, np.full(n_rays, sp), -np.cos(yaw) * cp], 1).astype(np.float32)


def _triangle_objects(arrays):
    """the object id of every triangle of a World.arrays dict: 0 for the statics, a dynamic chunk's object id for its triangles"""
    out = np.zeros(len(arrays['triangles']), np.uint32)
    for obj, start, end in arrays['dynamics']:
        out[start:end] = obj
    return out


def _cast_rays(call, states, levels, dirs, max_range, offsets, frac_out, hit_out, origin_out, vel_out, stream):
    """World.cast_rays / WorldSet.cast_rays: the checks and the launch; call(states, levels, n, dirs, n_rays, max_range, offsets,
    n_objects, frac, hit, origin, vel, stream) is the C entry point with its handle bound"""
    import torch
    for t, what in ((states, 'states'), (dirs, 'dirs')) + (((levels, 'levels'),) if levels is not None else ()) + \
            (((offsets, 'offsets'),) if offsets is not None else ()):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    n = _n_players(states)
    if dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.shape[0] == 0:
        raise ValueError('dirs must be a float32 (n_rays, 3) tensor with n_rays >= 1, got %s %s' % (dirs.dtype, tuple(dirs.shape)))
    n_rays = int(dirs.shape[0])
    if levels is not None and (levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    n_obj = 0
    if offsets is not None:
        if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s %s'
                             % (n, offsets.dtype, tuple(offsets.shape)))
        n_obj = int(offsets.shape[1])
    want_hit = hit_out is not None
    if hit_out is True:
        hit_out = torch.empty((n, n_rays), dtype=torch.int32, device=states.device)
    if frac_out is None:
        frac_out = torch.empty((n, n_rays), dtype=torch.float32, device=states.device)
    elif frac_out.dtype != torch.float32:
        raise ValueError('frac_out must be float32')
    pf = _out_tensor(frac_out, n * n_rays * 4, 'frac_out')
    ph = _out_tensor(hit_out, n * n_rays * 4, 'hit_out') if want_hit else None
    po, pv = _out_tensor(origin_out, n * n_rays * 12, 'origin_out'), _out_tensor(vel_out, n * n_rays * 12, 'vel_out')
    for t, what in ((origin_out, 'origin_out'), (vel_out, 'vel_out')):
        if t is not None and t.dtype != torch.float32:
            raise ValueError('%s must be float32' % what)
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n, v(dirs.data_ptr()), n_rays,
                ctypes.c_float(max_range), v(offsets.data_ptr()) if offsets is not None else None, n_obj, v(pf), v(ph), v(po), v(pv),
                v(_stream_handle(stream))))
    return (frac_out, hit_out) if want_hit else frac_out


class MapLines(ctypes.Structure):
    _fields_ = [('lines', ctypes.c_void_p), ('n_lines', ctypes.c_uint32)]


class MapView(ctypes.Structure):
    _fields_ = [('width', ctypes.c_uint32), ('height', ctypes.c_uint32), ('scale', ctypes.c_float), ('half_width', ctypes.c_float),
                ('marker', ctypes.c_float), ('flags', ctypes.c_uint32)]


def _map_lines(get):
    """World.map_lines / WorldSet.map_lines: a copy of the table get(&rdoom_map_lines) lends"""
    a = MapLines()
    _check(get(ctypes.byref(a)))
    return BuiltLevel._view(None, a.lines, a.n_lines, MAP_LINE)


def _seen_rows(seen, n, words):
    """(pointer, stride in words) of a caller's rows of seen bits: a contiguous 32-bit (n, stride) GPU tensor with stride >= words"""
    import torch
    if not isinstance(seen, torch.Tensor) or seen.device.type != 'cuda' or not seen.is_contiguous() or seen.dim() != 2 or \
            seen.element_size() != 4 or seen.dtype.is_floating_point or seen.shape[0] != n or seen.shape[1] < words:
        raise ValueError('seen must be a contiguous 32-bit integer (n, words) tensor on the GPU for %d players with words >= %d' % (n, words))
    return seen.data_ptr(), int(seen.shape[1])


def _draw_maps(call, states, levels, width, height, scale, offsets, half_width, marker, rotate, show_flat, show_hidden, top_down, out,
               stream, seen=None, words=0):
    """World.draw_maps / WorldSet.draw_maps: the checks and the launch; call(states, levels, n, offsets, n_objects, view, seen,
    stride, out, stream) is the C entry point with its handle bound"""
    import torch
    for t, what in ((states, 'states'),) + (((levels, 'levels'),) if levels is not None else ()) + \
            (((offsets, 'offsets'),) if offsets is not None else ()):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    n = _n_players(states)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError('a map needs at least 1 x 1 pixels, got %d x %d' % (width, height))
    if levels is not None and (levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    n_obj = 0
    if offsets is not None:
        if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s %s'
                             % (n, offsets.dtype, tuple(offsets.shape)))
        n_obj = int(offsets.shape[1])
    if out is None:
        out = torch.empty((n, height, width), dtype=torch.uint8, device=states.device)
    elif out.dtype != torch.uint8:
        raise ValueError('out must be uint8')
    po = _out_tensor(out, n * height * width, 'out')
    view = MapView(width, height, scale, half_width, marker, (MAP_ROTATE if rotate else 0) | (MAP_SHOW_FLAT if show_flat else 0) |
                   (MAP_SHOW_HIDDEN if show_hidden else 0) | (MAP_TOP_DOWN if top_down else 0))
    ps, stride = _seen_rows(seen, n, words) if seen is not None else (None, 0)
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n,
                v(offsets.data_ptr()) if offsets is not None else None, n_obj, ctypes.byref(view), v(ps), stride, v(po),
                v(_stream_handle(stream))))
    return out


def map_fan(n_rays, fov):
    """a direction table for reveal_lines: n_rays unit directions (right, forward) in the player's map frame, a float32 (n_rays, 2)
    array, evenly spaced across `fov` radians and centred on straight ahead (ray 0 is the leftmost, at fov / 2 to the left; an odd
    n_rays has the ray (0, 1))"""
    n_rays = int(n_rays)
    if n_rays < 1:
        raise ValueError('n_rays must be at least 1')
    angle = np.linspace(-0.5 * fov, 0.5 * fov, n_rays) if n_rays > 1 else np.zeros(1)
    return np.stack([np.sin(angle), np.cos(angle)], 1).astype(np.float32)


def unpack_seen(row, n_lines):
    """a row of reveal_lines' bits (a numpy array or tensor of 32-bit words) as a bool array of n_lines: [l] = line l is seen"""
    if not isinstance(row, np.ndarray):
        row = row.cpu().numpy()
    words = np.ascontiguousarray(row).reshape(-1).view(np.uint32)
    n_lines = int(n_lines)
    if len(words) * 32 < n_lines:
        raise ValueError('%d words hold fewer than %d lines' % (len(words), n_lines))
    l = np.arange(n_lines)
    return ((words[l >> 5] >> (l & 31).astype(np.uint32)) & 1).astype(bool)


def _reveal_lines(call, words, states, levels, fan, max_range, offsets, seen, new_out, stream):
    """World.reveal_lines / WorldSet.reveal_lines: the checks and the launch; call(states, levels, n, dirs, n_rays, max_range,
    offsets, n_objects, seen, stride, new_out, stream) is the C entry point with its handle bound"""
    import torch
    for t, what in ((states, 'states'), (fan, 'fan')) + (((levels, 'levels'),) if levels is not None else ()) + \
            (((offsets, 'offsets'),) if offsets is not None else ()):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    n = _n_players(states)
    if fan.dtype != torch.float32 or fan.dim() != 2 or fan.shape[1] != 2 or fan.shape[0] == 0:
        raise ValueError('fan must be a float32 (n_rays, 2) tensor with n_rays >= 1, got %s %s' % (fan.dtype, tuple(fan.shape)))
    if levels is not None and (levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    n_obj = 0
    if offsets is not None:
        if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s %s'
                             % (n, offsets.dtype, tuple(offsets.shape)))
        n_obj = int(offsets.shape[1])
    if seen is None:
        seen = torch.zeros((n, words), dtype=torch.int32, device=states.device)
    ps, stride = _seen_rows(seen, n, words)
    if new_out is not None and (new_out.element_size() != 4 or new_out.dtype.is_floating_point):
        raise ValueError('new_out must hold 32-bit integers')
    pn = _out_tensor(new_out, n * 4, 'new_out')
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n, v(fan.data_ptr()), int(fan.shape[0]),
                ctypes.c_float(max_range), v(offsets.data_ptr()) if offsets is not None else None, n_obj, v(ps), stride, v(pn),
                v(_stream_handle(stream))))
    return seen


class MapThings(ctypes.Structure):
    _fields_ = [('things', ctypes.c_void_p), ('n_things', ctypes.c_uint32)]


class ThingSense(ctypes.Structure):
    """rdoom_thing_sense"""
    _fields_ = [('max_range', ctypes.c_float), ('cos_half_fov', ctypes.c_float), ('touch_radius', ctypes.c_float),
                ('touch_below', ctypes.c_float), ('touch_above', ctypes.c_float), ('collect_mask', ctypes.c_uint32),
                ('flags', ctypes.c_uint32)]


class ThingMarks(ctypes.Structure):
    """rdoom_thing_marks (THING_MARKS is the same record for numpy)"""
    _fields_ = [('min_radius', ctypes.c_float), ('codes', ctypes.c_uint8 * 8), ('flags', ctypes.c_uint32)]


def _map_things(get):
    """World.map_things / WorldSet.map_things: a copy of the table get(&rdoom_map_things) lends"""
    a = MapThings()
    _check(get(ctypes.byref(a)))
    return BuiltLevel._view(None, a.things, a.n_things, THING)


class DeviceThings:
    """The thing tables of one or more levels resident on the device (rdoom_thingset_create): slot l holds tables[l], an array of
    THING records -- a level's own (World.map_things()) or any other, so that a consumer can scatter items of its own per run.
    A single array is a set of one level.  World.sense_things / WorldSet.sense_things sense them."""

    def __init__(self, tables):
        if isinstance(tables, np.ndarray):
            tables = [tables]
        arrays = [np.ascontiguousarray(t, THING).reshape(-1) for t in tables]
        self.n_levels, self.counts = len(arrays), [len(a) for a in arrays]
        ptrs = (ctypes.c_void_p * max(1, len(arrays)))(*[_ptr(a) for a in arrays])
        counts = (ctypes.c_uint32 * max(1, len(arrays)))(*self.counts)
        self._h = ctypes.c_void_p()
        _check(lib().rdoom_thingset_create(ptrs, counts, len(arrays), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().rdoom_thingset_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def info(self):
        """rdoom_thingset_info: (levels, words, largest object_id)"""
        n, w, o = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().rdoom_thingset_info(self._h, ctypes.byref(n), ctypes.byref(w), ctypes.byref(o)))
        return n.value, w.value, o.value

    def words(self):
        """the 32-bit words a row of thing bits takes at least: max(1, ceil(largest table / 32))"""
        return self.info()[1]

    def draw_maps(self, states, width, height, scale, levels=None, min_radius=2.0, codes=None, hidden=None, known=None, rotate=False,
                  top_down=False, over=False, out=None, index_out=None, stream=None, n=None, stride=None):
        """rdoom_thingset_draw_maps: every player's thing marks on the pixels of World.draw_maps(states, width, height, scale,
        rotate=, top_down=), one launch.  A thing is a disc of its own radius, at least min_radius pixels; its byte is
        codes[category] (a sequence of eight, 0: that category is not drawn; None: MAP_THING + category), and where discs overlap the
        larger code wins, the lower index among equal codes.  levels: None (every player in slot 0; a set of one level) or one
        32-bit slot per player.  hidden: None or sense_things' `collected` (n, words) tensor as it stands: player p's map leaves
        out the things whose bit is set in row p.  known: None (every thing) or such a tensor of the things a player may see on
        its map, for instance `known |= visible` after every sense_things.  out: a uint8 (n, height, width) tensor, allocated when
        None, or False for no byte plane; over: only the covered bytes of `out` are written, so that a call on the tensor draw_maps
        filled overlays the marks on the lines (THING_MAP_COLORS colours the result).  index_out: None / False, True (allocated) or
        an int32 (n, height, width) tensor: the index of the thing at each pixel, -1 where there is none; always written whole.
        Every tensor may instead be a raw device pointer (an int; then n, and with hidden or known stride, must be given).  Returns
        what was asked for: out, index_out, or (out, index_out).  Asynchronous on `stream`; nothing is copied to the host."""
        raw = isinstance(states, (int, np.integer))
        if raw:
            if n is None:
                raise ValueError('n is needed with raw pointers')
            n = int(n)
        else:
            n = _n_players(states)
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError('a map needs at least 1 x 1 pixels, got %d x %d' % (width, height))
        if codes is None:
            codes = [MAP_THING + c for c in range(THING_CATEGORIES)]
        codes = [int(c) for c in codes]
        if len(codes) != THING_CATEGORIES or not all(0 <= c <= 255 for c in codes):
            raise ValueError('codes must be eight bytes, one per category, got %r' % (codes,))
        for r, what in ((hidden, 'hidden'), (known, 'known')):
            if r is None or isinstance(r, (int, np.integer)):
                if r is not None and stride is None:
                    raise ValueError('stride is needed with a raw %s pointer' % what)
                continue
            if r.element_size() != 4 or r.dtype.is_floating_point or r.dim() != 2:
                raise ValueError('%s must be a 32-bit integer (n, words) tensor' % what)
            if int(r.shape[0]) < n:
                raise ValueError('the %s tensor has %d rows, the call %d players' % (what, int(r.shape[0]), n))
            if stride is not None and int(stride) != int(r.shape[1]):
                raise ValueError('stride %d, but the %s rows are %d words long' % (int(stride), what, int(r.shape[1])))
            stride = int(r.shape[1])
        stride = 0 if stride is None else int(stride)
        if levels is not None and not isinstance(levels, (int, np.integer)) and (levels.element_size() != 4 or levels.numel() != n):
            raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
        wants_index = index_out is not None and index_out is not False
        if out is False:
            out = None
        elif out is None:
            if over:
                raise ValueError('over=True writes only the covered bytes: it needs the tensor to draw over as out')
            if raw:
                raise ValueError('out is needed with raw pointers')
            import torch
            out = torch.empty((n, height, width), dtype=torch.uint8, device=states.device)
        elif not isinstance(out, (int, np.integer)) and out.element_size() != 1:
            raise ValueError('out must hold bytes')
        if index_out is True:
            if raw:
                raise ValueError('index_out must be a tensor or a pointer with raw pointers')
            import torch
            index_out = torch.empty((n, height, width), dtype=torch.int32, device=states.device)
        elif not wants_index:
            index_out = None
        elif not isinstance(index_out, (int, np.integer)) and (index_out.element_size() != 4 or index_out.dtype.is_floating_point):
            raise ValueError('index_out must hold 32-bit integers')
        view = MapView(width, height, scale, 0.0, 0.0, (MAP_ROTATE if rotate else 0) | (MAP_TOP_DOWN if top_down else 0))
        marks = ThingMarks(min_radius, (ctypes.c_uint8 * 8)(*codes), THING_MARKS_OVER if over else 0)
        v = ctypes.c_void_p
        pixels = n * height * width
        _check(lib().rdoom_thingset_draw_maps(self._h, v(_pointer(states, n * PLAYER_STATE.itemsize, 'states')),
                                              v(_pointer(levels, n * 4, 'levels')), n, ctypes.byref(view), ctypes.byref(marks),
                                              v(_pointer(hidden, n * stride * 4, 'hidden')), v(_pointer(known, n * stride * 4, 'known')),
                                              stride, v(_pointer(out, pixels, 'out')), v(_pointer(index_out, pixels * 4, 'index_out')),
                                              v(_stream_handle(stream))))
        if out is None:
            return index_out
        return (out, index_out) if index_out is not None else out


def unpack_things(row, n):
    """a row of sense_things' bits (a numpy array or tensor of 32-bit words) as a bool array of n: [i] = thing i's bit is set"""
    return unpack_seen(row, n)


def pack_things(bools, words=None):
    """the inverse of unpack_things: a bool array of n things as a row of `words` 32-bit words (None: max(1, ceil(n / 32))), bit
    i % 32 of word i // 32 for thing i, an int32 array.  A list of arrays gives a (levels, words) array, one row a level: for
    instance pack_things([ws.thing_obstacles(s) for s in range(ws.n_levels)]), the obstacle bits of a set"""
    if isinstance(bools, (list, tuple)) and len(bools) and not np.isscalar(bools[0]):
        rows = [np.asarray(b, bool).reshape(-1) for b in bools]
        if words is None:
            words = max(1, max((len(r) + 31) // 32 for r in rows))
        return np.stack([pack_things(r, words) for r in rows])
    bits = np.asarray(bools, bool).reshape(-1)
    need = max(1, (len(bits) + 31) // 32)
    words = need if words is None else int(words)
    if words < need:
        raise ValueError('%d words hold fewer than %d things' % (words, len(bits)))
    padded = np.zeros(words * 32, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded.reshape(words, 32), axis=1, bitorder='little').view('<u4').reshape(words).astype(np.uint32).view(np.int32)


def frame_things(ids, depth=None, max_things=None, min_pixels=1, table_out=None, bits_out=None, stream=None, shape=None):
    """rdoom_frame_things (include/rdoom_frame_things.h): what each frame of an id plane shows of each thing.  ids: a contiguous
    int32 (n, H, W) GPU tensor -- Batch.resolve_thing_plane's, or any other plane of ids -- or a raw device pointer with shape =
    (n, H, W); depth: None, or the float32 plane of the same shape and row order (Batch.resolve_depth's), tensor or pointer.
    Returns (table, bits).  table: an int32 (n, max_things, 6) GPU tensor of FRAME_THING records -- count, x0, y0, x1, y1 (the
    inclusive box in columns and rows of the plane as given) and the bits of depth_min (frame_things_depth(table) views them),
    the smallest finite non-negative depth of the thing's pixels; a thing with no pixel has count 0, x0 = y0 = INT32_MAX, x1 = y1
    = -1 and depth_min = +inf; ids below 0 or at or above max_things are ignored.  bits: an int32 (n, words) tensor, words =
    ceil(max_things / 32), bit i % 32 of word i // 32 set exactly when thing i has at least min_pixels pixels -- the layout of
    sense_things' rows, so `known |= bits` works as it stands -- or None with bits_out=False.  table_out, bits_out: tensors (32-bit
    integer; bits_out (n, stride) with any stride >= 1) or raw device pointers (bits_out then with the stride `words`) to write
    instead of new ones.  Three launches, asynchronous on `stream` (None, a torch stream or a raw handle); it can be captured into
    a graph."""
    import torch
    if max_things is None:
        raise ValueError('max_things must be given: the number of records per frame, for instance 32 * things.words()')
    max_things, min_pixels = int(max_things), int(min_pixels)
    raw = isinstance(ids, int) and not isinstance(ids, bool)
    if raw:
        if shape is None or len(shape) != 3:
            raise ValueError('a raw ids pointer needs shape=(n, H, W)')
        pi, device = ids, None
    else:
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.device.type != 'cuda' or not ids.is_contiguous() or ids.dim() != 3:
            raise ValueError('ids must be a contiguous int32 (n, H, W) tensor on the GPU, or a device pointer with shape=')
        if shape is not None and tuple(shape) != tuple(ids.shape):
            raise ValueError('shape %r, but ids is %r' % (tuple(shape), tuple(ids.shape)))
        shape, pi, device = tuple(ids.shape), ids.data_ptr(), ids.device
    n, height, width = (int(s) for s in shape)
    if depth is None or (isinstance(depth, int) and not isinstance(depth, bool)):
        pd = depth
    elif not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32:
        raise ValueError('depth must be None, a float32 tensor of the shape of ids, or a device pointer')
    else:
        pd = _out_tensor(depth, n * height * width * 4, 'depth')
    if device is None and (table_out is None or bits_out is None or bits_out is True):
        raise ValueError('with a raw ids pointer give table_out, and bits_out or bits_out=False')
    table, pt = _int32_out(table_out, (n, max_things, 6), device, 'table_out')
    words = (max_things + 31) // 32
    if bits_out is False:
        bits, pb, stride = None, None, 0
    elif isinstance(bits_out, torch.Tensor):
        if bits_out.dim() != 2 or bits_out.shape[0] != n or bits_out.shape[1] < 1:
            raise ValueError('bits_out must be an (n, stride) tensor with stride >= 1')
        stride = int(bits_out.shape[1])
        bits, pb = _int32_out(bits_out, (n, stride), device, 'bits_out')
    else:
        stride = words
        bits, pb = _int32_out(bits_out, (n, stride), device, 'bits_out')
    v = ctypes.c_void_p
    _check(lib().rdoom_frame_things(v(pi or None), v(pd or None), n, width, height, max_things, min_pixels, v(pt or None), v(pb or None), stride,
                                    v(_stream_handle(stream))))
    return table, bits


def frame_things_depth(table):
    """column 5 of frame_things' table, depth_min, viewed as float32: (n, max_things)"""
    import torch
    return table[..., 5].view(torch.float32) if isinstance(table, torch.Tensor) else np.asarray(table)[..., 5].view(np.float32)


def _thing_obstacles(get, n_things):
    """World.thing_obstacles / WorldSet.thing_obstacles: the bits get(&words, &n_words) lends, as a bool array of n_things"""
    p, n = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_uint32(0)
    _check(get(ctypes.byref(p), ctypes.byref(n)))
    return unpack_things(np.ctypeslib.as_array(p, shape=(n.value,)).copy(), n_things)


ThingsSensed = collections.namedtuple('ThingsSensed', 'collected visible touched nearest new')


def _pointer(t, nbytes, what):
    """the device pointer of an optional argument: None, a raw device pointer (an int, taken as it is), or a contiguous GPU tensor
    of at least nbytes"""
    if t is None or isinstance(t, (int, np.integer)):
        return int(t) if t else None
    if t.device.type != 'cuda' or not t.is_contiguous() or t.numel() * t.element_size() < nbytes:
        raise ValueError('%s must be a contiguous GPU tensor of at least %d bytes' % (what, nbytes))
    return t.data_ptr()


def _sense_things(call, states, levels, things, max_range, fov, touch_radius, touch_below, touch_above, collect, offsets, collected,
                  visible_out, touched_out, nearest_out, new_out, stream, n, n_objects, stride):
    """World.sense_things / WorldSet.sense_things: the checks and the launch; call(states, levels, n, offsets, n_objects, params,
    collected, visible, touched, stride, nearest, new, stream) is the C entry point with its handle and the thing set bound"""
    if not isinstance(things, DeviceThings):
        raise ValueError('things must be a DeviceThings')
    raw = isinstance(states, (int, np.integer))
    if raw:
        if n is None:
            raise ValueError('n is needed with raw pointers')
        n = int(n)
    else:
        n = _n_players(states)
    words = things.words()
    rows = (collected, visible_out, touched_out)
    if all(o is None for o in rows + (nearest_out, new_out)):
        import torch
        visible_out = torch.empty((n, words), dtype=torch.int32, device=states.device)
        touched_out = torch.empty((n, words), dtype=torch.int32, device=states.device)
        nearest_out = torch.empty((n, THING_CATEGORIES, 4), dtype=torch.float32, device=states.device)
        new_out = torch.empty((n, THING_CATEGORIES), dtype=torch.int32, device=states.device)
        rows = (collected, visible_out, touched_out)
    if stride is None:
        strides = {int(r.shape[-1]) for r in rows if r is not None and not isinstance(r, (int, np.integer))}
        if len(strides) > 1:
            raise ValueError('collected, visible_out and touched_out must have rows of one length, got %s' % sorted(strides))
        stride = strides.pop() if strides else words
    stride = int(stride)
    for r, what in zip(rows, ('collected', 'visible_out', 'touched_out')):
        if r is not None and not isinstance(r, (int, np.integer)) and (r.element_size() != 4 or r.dtype.is_floating_point or r.dim() != 2
                                                                       or r.shape[0] != n):
            raise ValueError('%s must be a 32-bit integer (n, words) tensor for %d players' % (what, n))
    n_obj = 0
    if offsets is not None:
        if isinstance(offsets, (int, np.integer)):
            if n_objects is None:
                raise ValueError('n_objects is needed with a raw offsets pointer')
            n_obj = int(n_objects)
        else:
            if offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3 or offsets.element_size() != 4:
                raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s' % (n, tuple(offsets.shape)))
            n_obj = int(offsets.shape[1])
    mask = 0
    for c in ((collect,) if isinstance(collect, (int, np.integer)) else collect):
        if not 0 <= int(c) < THING_CATEGORIES:
            raise ValueError('collect names categories 0 .. 7, not %r' % (c,))
        mask |= 1 << int(c)
    params = ThingSense(max_range, -1.0 if fov is None else math.cos(0.5 * float(fov)), touch_radius, touch_below, touch_above, mask, 0)
    v = ctypes.c_void_p
    _check(call(v(_pointer(states, n * PLAYER_STATE.itemsize, 'states')), v(_pointer(levels, n * 4, 'levels')), n,
                v(_pointer(offsets, n * n_obj * 12, 'offsets')), n_obj, ctypes.byref(params),
                v(_pointer(collected, n * stride * 4, 'collected')), v(_pointer(visible_out, n * stride * 4, 'visible_out')),
                v(_pointer(touched_out, n * stride * 4, 'touched_out')), stride,
                v(_pointer(nearest_out, n * THING_CATEGORIES * 16, 'nearest_out')), v(_pointer(new_out, n * THING_CATEGORIES * 4, 'new_out')),
                v(_stream_handle(stream))))
    return ThingsSensed(collected, visible_out, touched_out, nearest_out, new_out)


_SENSE_DOC = """marks the things of `things` (a DeviceThings) every player sees and touches, finds the nearest visible
        thing of each category and collects what the player walks over, in one launch.  states: the tensor a step leaves; offsets:
        None or step_game's tensor, so that a shut door hides a thing until that player opens it and a candle on a lift rides it.
        max_range: how far a player sees; fov: None (all round) or the full opening angle in radians; touch_radius: the body's;
        touch_below / touch_above: how far the thing's base may lie above / below the player's position to be touched; collect: the
        categories (THING_*) whose touched things are collected.  collected: an int32 (n, words >= things.words()) tensor -- a
        collected thing is neither seen nor touched any more; its bits are OR-ed into after the call's evaluation and never
        cleared, so zero a row to start an episode.  visible_out / touched_out: int32 (n, words) tensors, bit i % 32 of word i // 32
        of row p for thing i (unpack_things unpacks a row); nearest_out: n x 8 THING_NEAREST records (any tensor of n * 128 bytes,
        for instance float32 (n, 8, 4): index as bits, d2, right, forward); new_out: int32 (n, 8), what this call collected per
        category.  With every output None, visible, touched, nearest and new are allocated.  Every tensor may instead be a raw
        device pointer (an int; then n, and with offsets n_objects, and stride must be given).  Returns a ThingsSensed of the five.
        Asynchronous on `stream`."""


class AreaGridStruct(ctypes.Structure):
    _fields_ = [('ix0', ctypes.c_int32), ('iz0', ctypes.c_int32), ('gw', ctypes.c_uint32), ('gh', ctypes.c_uint32),
                ('pitch', ctypes.c_uint32), ('words', ctypes.c_uint32)]


class AreaGrid(collections.namedtuple('AreaGrid', 'ix0 iz0 gw gh pitch words')):
    """rdoom_area_grid: the explored-area grid of a level at one cell size.  Cell (ix, iz) covers world x in [(ix0 + ix) * cell,
    (ix0 + ix + 1) * cell) and z alike; it is bit ix % 32 of word iz * pitch + ix // 32 of a plane of `words` words"""


def _area_grid(get):
    """World.area_grid / WorldSet.area_grid: get(&rdoom_area_grid) as an AreaGrid"""
    g = AreaGridStruct()
    _check(get(ctypes.byref(g)))
    return AreaGrid(g.ix0, g.iz0, g.gw, g.gh, g.pitch, g.words)


def _area_words(get):
    words = ctypes.c_uint32(0)
    _check(get(ctypes.byref(words)))
    return words.value


def area_steps(max_range, cell):
    """the n_steps of reveal_area that puts samples half a cell apart along a ray of unit direction: ceil(2 * max_range / cell)"""
    if not (max_range > 0 and cell > 0):
        raise ValueError('max_range and cell must be positive')
    return max(1, int(math.ceil(2.0 * float(max_range) / float(cell))))


def unpack_area(rows, grid):
    """one player's rows of reveal_area's bits (a numpy array or tensor, (2, stride) 32-bit words with stride >= grid.words) as a
    (2, gh, gw) bool array: [0, iz, ix] = cell (ix, iz) is free, [1, iz, ix] = it is a wall"""
    if not isinstance(rows, np.ndarray):
        rows = rows.cpu().numpy()
    words = np.ascontiguousarray(rows).view(np.uint32)
    if words.ndim != 2 or words.shape[0] != 2 or words.shape[1] < grid.words:
        raise ValueError('rows must be (2, stride) words with stride >= %d, got %s' % (grid.words, tuple(words.shape)))
    planes = words[:, :grid.words].reshape(2, grid.gh, grid.pitch)
    ix = np.arange(grid.gw)
    return ((planes[:, :, ix >> 5] >> (ix & 31).astype(np.uint32)) & 1).astype(bool)


def _area_rows(area, n, words):
    """(pointer, stride in words) of a caller's area rows: a contiguous 32-bit (n, 2, stride) GPU tensor with stride >= words"""
    import torch
    if not isinstance(area, torch.Tensor) or area.device.type != 'cuda' or not area.is_contiguous() or area.dim() != 3 or \
            area.element_size() != 4 or area.dtype.is_floating_point or area.shape[0] != n or area.shape[1] != 2 or area.shape[2] < words:
        raise ValueError('area must be a contiguous 32-bit integer (n, 2, words) tensor on the GPU for %d players with words >= %d' % (n, words))
    return area.data_ptr(), int(area.shape[2])


def _reveal_area(call, words, states, levels, fan, max_range, cell, n_steps, offsets, area, new_out, stream):
    """World.reveal_area / WorldSet.reveal_area: the checks and the launch; call(states, levels, n, dirs, n_rays, max_range,
    offsets, n_objects, cell, n_steps, area, stride, new_out, stream) is the C entry point with its handle bound"""
    import torch
    if not isinstance(fan, torch.Tensor) or fan.device.type != 'cuda' or not fan.is_contiguous():
        raise ValueError('fan must be a contiguous tensor on the GPU')
    n, n_obj = _player_tensors(states, levels, offsets)
    if fan.dtype != torch.float32 or fan.dim() != 2 or fan.shape[1] != 2 or fan.shape[0] == 0:
        raise ValueError('fan must be a float32 (n_rays, 2) tensor with n_rays >= 1, got %s %s' % (fan.dtype, tuple(fan.shape)))
    if n_steps is None:
        n_steps = area_steps(max_range, cell)
    if area is None:
        area = torch.zeros((n, 2, words), dtype=torch.int32, device=states.device)
    pa, stride = _area_rows(area, n, words)
    if new_out is not None and (new_out.element_size() != 4 or new_out.dtype.is_floating_point):
        raise ValueError('new_out must hold 32-bit integers')
    pn = _out_tensor(new_out, n * 8, 'new_out')
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n, v(fan.data_ptr()), int(fan.shape[0]),
                ctypes.c_float(max_range), v(offsets.data_ptr()) if offsets is not None else None, n_obj, ctypes.c_float(cell), int(n_steps),
                v(pa), stride, v(pn), v(_stream_handle(stream))))
    return area


def _draw_area_maps(call, words, states, levels, width, height, scale, area, cell, rotate, top_down, out, stream):
    """World.draw_area_maps / WorldSet.draw_area_maps: the checks and the launch; call(states, levels, n, view, area, stride, cell,
    out, stream) is the C entry point with its handle bound"""
    import torch
    n, _ = _player_tensors(states, levels, None)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError('a map needs at least 1 x 1 pixels, got %d x %d' % (width, height))
    pa, stride = _area_rows(area, n, words)
    if out is None:
        out = torch.empty((n, height, width), dtype=torch.uint8, device=states.device)
    elif out.dtype != torch.uint8:
        raise ValueError('out must be uint8')
    po = _out_tensor(out, n * height * width, 'out')
    view = MapView(width, height, scale, 0.0, 0.0, (MAP_ROTATE if rotate else 0) | (MAP_TOP_DOWN if top_down else 0))
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n, ctypes.byref(view), v(pa), stride,
                ctypes.c_float(cell), v(po), v(_stream_handle(stream))))
    return out


class MapSectorArrays(ctypes.Structure):
    _fields_ = [('sectors', ctypes.c_void_p), ('leaf_sector', ctypes.c_void_p), ('leaf_edges', ctypes.c_void_p), ('edges', ctypes.c_void_p),
                ('n_sectors', ctypes.c_uint32), ('n_leaves', ctypes.c_uint32), ('n_edges', ctypes.c_uint32)]


class MapSectors(collections.namedtuple('MapSectors', 'sectors leaf_sector leaf_edges edges')):
    """copies of a level's sector table (rdoom_map_sectors): sectors, a MAP_SECTOR record per SECTORS entry; leaf_sector, per chunk
    of the collision BSP its sector or SECTOR_NONE; leaf_edges, per chunk (first, count) into edges; edges, MAP_EDGE records (a, d) of
    the solid segs, the sub-sector where (q - a) x d <= 0"""


def _map_sectors(get):
    """World.map_sectors / WorldSet.map_sectors: copies of the tables get(&rdoom_map_sectors) lends"""
    a = MapSectorArrays()
    _check(get(ctypes.byref(a)))
    view = lambda ptr, n, dtype: BuiltLevel._view(None, ptr, n, dtype)
    return MapSectors(view(a.sectors, a.n_sectors, MAP_SECTOR), view(a.leaf_sector, a.n_leaves, np.uint32),
                      view(a.leaf_edges, a.n_leaves * 2, np.uint32).reshape(-1, 2), view(a.edges, a.n_edges, MAP_EDGE))


def _player_tensors(states, levels, offsets):
    """what the sector calls check of states, levels and offsets: (n, n_objects)"""
    import torch
    for t, what in ((states, 'states'),) + (((levels, 'levels'),) if levels is not None else ()) + \
            (((offsets, 'offsets'),) if offsets is not None else ()):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    n = _n_players(states)
    if levels is not None and (levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    n_obj = 0
    if offsets is not None:
        if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s %s'
                             % (n, offsets.dtype, tuple(offsets.shape)))
        n_obj = int(offsets.shape[1])
    return n, n_obj


def _locate_players(call, words, states, levels, offsets, heights_out, visited, new_out, out, stream):
    """World.locate_players / WorldSet.locate_players: the checks and the launch; call(states, levels, n, offsets, n_objects,
    sector_out, heights_out, visited, stride, new_out, stream) is the C entry point with its handle bound"""
    import torch
    n, n_obj = _player_tensors(states, levels, offsets)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=states.device)
    elif out.element_size() != 4 or out.dtype.is_floating_point:
        raise ValueError('out must hold 32-bit integers')
    po = _out_tensor(out, n * 4, 'out')
    if heights_out is not None and heights_out.dtype != torch.float32:
        raise ValueError('heights_out must be float32')
    ph = _out_tensor(heights_out, n * 8, 'heights_out')
    pv, stride = _seen_rows(visited, n, words) if visited is not None else (None, 0)
    if new_out is not None and (new_out.element_size() != 4 or new_out.dtype.is_floating_point):
        raise ValueError('new_out must hold 32-bit integers')
    pn = _out_tensor(new_out, n * 4, 'new_out')
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n,
                v(offsets.data_ptr()) if offsets is not None else None, n_obj, v(po), v(ph), v(pv), stride, v(pn), v(_stream_handle(stream))))
    return out


def _draw_sector_maps(call, words, states, levels, width, height, scale, offsets, rotate, top_down, sector_out, floor, ceiling, visited,
                      stream):
    """World.draw_sector_maps / WorldSet.draw_sector_maps: the checks and the launch; call(states, levels, n, offsets, n_objects,
    view, visited, stride, sector_out, floor_out, ceiling_out, stream) is the C entry point with its handle bound.  Returns the
    planes asked for, in the order sector, floor, ceiling: one tensor, or a tuple of them"""
    import torch
    n, n_obj = _player_tensors(states, levels, offsets)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError('a map needs at least 1 x 1 pixels, got %d x %d' % (width, height))
    planes = []
    for want, dtype, what in ((sector_out, torch.int16, 'sector_out'), (floor, torch.float32, 'floor'), (ceiling, torch.float32, 'ceiling')):
        if want is None or want is False:
            planes.append(None)
            continue
        if want is True:
            want = torch.empty((n, height, width), dtype=dtype, device=states.device)
        elif not isinstance(want, torch.Tensor) or want.element_size() != (2 if dtype == torch.int16 else 4) or \
                want.dtype.is_floating_point != (dtype == torch.float32):
            raise ValueError('%s must be True or a %s tensor' % (what, '16-bit integer' if dtype == torch.int16 else 'float32'))
        _out_tensor(want, n * height * width * want.element_size(), what)
        planes.append(want)
    if all(t is None for t in planes):
        raise ValueError('no plane asked for: sector_out, floor and ceiling are all off')
    view = MapView(width, height, scale, 0.0, 0.0, (MAP_ROTATE if rotate else 0) | (MAP_TOP_DOWN if top_down else 0))
    pv, stride = _seen_rows(visited, n, words) if visited is not None else (None, 0)
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n,
                v(offsets.data_ptr()) if offsets is not None else None, n_obj, ctypes.byref(view), v(pv), stride,
                *[v(t.data_ptr()) if t is not None else None for t in planes], v(_stream_handle(stream))))
    given = tuple(t for t in planes if t is not None)
    return given[0] if len(given) == 1 else given


class FloodParams(ctypes.Structure):
    """rdoom_flood_params"""
    _fields_ = [('max_step', ctypes.c_float), ('max_drop', ctypes.c_float), ('clearance', ctypes.c_float), ('flags', ctypes.c_uint32)]


def flood_max_cells():
    """rdoom_flood_max_cells: the most cells (width * height) of a map flood_maps takes, a constant of the library"""
    cells = ctypes.c_uint32(0)
    _check(lib().rdoom_flood_max_cells(ctypes.byref(cells)))
    return cells.value


def flood_maps(floor, ceiling, seeds=None, max_step=0.24, max_drop=float('inf'), clearance=0.56, dist_out=None, count_out=None, stream=None):
    """rdoom_flood_maps: every player's filled map flooded from a seed cell.  floor, ceiling: the float32 (n, H, W) GPU tensors
    draw_sector_maps(floor=True, ceiling=True) returns, in either row order (the flood works on stored rows); H * W is at most
    flood_max_cells().  A cell is open when its floor is finite and ceiling - floor >= clearance; a move to a 4-neighbour is allowed
    when both are open, the floor rises by at most max_step and falls by at most max_drop, and the opening the two share
    (min ceiling - max floor) is at least clearance -- so moves are directed, a ledge is dropped from and not climbed, and a door a
    player has not opened blocks that player's flood.  seeds: None -- the cell (W // 2, H // 2), the player's own -- or an int32
    (n, 2) tensor of (column, row) in stored order.  Returns the (n, H, W) uint16 tensor of distances in moves, 0 at the seed and
    FLOOD_UNREACHED where no path leads, where the cell is closed, and everywhere when the seed is closed or outside the grid
    (dist_out: a 16-bit integer tensor, or a raw device pointer, to write instead of a new one); with count_out True, an (n,)
    32-bit integer tensor or a raw device pointer, returns (distances, counts), counts[p] the number of cells player p reaches.  The defaults are Doom's 24-unit step and 56-unit
    body at this project's 1/100 scale: a model of walking, which nothing ties to the sphere-and-spring physics of World.step.
    One launch, asynchronous on `stream` (None, a torch stream or a raw handle); it can be captured into a graph."""
    n, height, width = _flood_inputs(floor, ceiling, seeds)
    dist_out, pd, count_out, pc = _flood_outputs(n, height, width, floor.device, dist_out, count_out, 2)
    params = FloodParams(max_step, max_drop, clearance, 0)
    v = ctypes.c_void_p
    _check(lib().rdoom_flood_maps(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height, v(seeds.data_ptr()) if seeds is not None else None,
                                  ctypes.byref(params), v(pd), v(pc), v(_stream_handle(stream))))
    return dist_out if count_out is None else (dist_out, count_out)


def _flood_outputs(n, height, width, device, dist_out, count_out, dist_bytes):
    """flood_maps' and flood_grids' outputs, checked: (dist_out, its pointer, count_out or None, its pointer)"""
    import torch
    bits = '%d-bit' % (8 * dist_bytes)
    if dist_out is None:
        dist_out = torch.empty((n, height, width), dtype=torch.uint16 if dist_bytes == 2 else torch.int32, device=device)
    if isinstance(dist_out, int) and not isinstance(dist_out, bool):
        pd = dist_out  # a raw device pointer to n * height * width distances
    elif not isinstance(dist_out, torch.Tensor) or dist_out.element_size() != dist_bytes or dist_out.dtype.is_floating_point:
        raise ValueError('dist_out must be a %s integer tensor or a device pointer' % bits)
    else:
        pd = _out_tensor(dist_out, n * height * width * dist_bytes, 'dist_out')
    if count_out is None or count_out is False:
        count_out = None
    elif count_out is True:
        count_out = torch.empty(n, dtype=torch.int32, device=device)
    if isinstance(count_out, int) and not isinstance(count_out, bool):
        pc = count_out  # a raw device pointer to n uint32
    elif count_out is not None and (not isinstance(count_out, torch.Tensor) or count_out.element_size() != 4 or count_out.dtype.is_floating_point):
        raise ValueError('count_out must be True, a 32-bit integer tensor or a device pointer')
    else:
        pc = _out_tensor(count_out, n * 4, 'count_out')
    return dist_out, pd, count_out, pc


def _flood_inputs(floor, ceiling, seeds):
    """flood_maps' and flood_grids' inputs, checked: (n, height, width)"""
    import torch
    for t, what in ((floor, 'floor'), (ceiling, 'ceiling')):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous() or t.dtype != torch.float32 or t.dim() != 3:
            raise ValueError('%s must be a contiguous float32 (n, height, width) tensor on the GPU' % what)
    if floor.shape != ceiling.shape:
        raise ValueError('floor %s and ceiling %s differ in shape' % (tuple(floor.shape), tuple(ceiling.shape)))
    n, height, width = (int(x) for x in floor.shape)
    if seeds is not None and (not isinstance(seeds, torch.Tensor) or seeds.device.type != 'cuda' or not seeds.is_contiguous() or
                              seeds.dtype != torch.int32 or tuple(seeds.shape) != (n, 2)):
        raise ValueError('seeds must be a contiguous int32 (%d, 2) tensor of (column, row) on the GPU' % n)
    return n, height, width


def flood_grid_max_cells():
    """rdoom_flood_grid_max_cells: the most cells (width * height) of a grid flood_grids takes, a constant of the library: 2 ** 22"""
    cells = ctypes.c_uint32(0)
    _check(lib().rdoom_flood_grid_max_cells(ctypes.byref(cells)))
    return cells.value


def flood_grids(floor, ceiling, seeds=None, towards=False, max_step=0.24, max_drop=float('inf'), clearance=0.56, dist_out=None, count_out=None,
                stream=None):
    """rdoom_flood_grids: flood_maps for grids of any size up to flood_grid_max_cells() cells and AREA_MAX_SIDE a side -- the planes
    World.draw_area_planes(floor=True, ceiling=True) returns of a whole level -- from the seed or towards it.  floor, ceiling,
    seeds, max_step, max_drop, clearance: as flood_maps takes them; seeds may be area_cells' output, whose (-1, -1) of a player in no
    cell gives an all-unreached row.  towards False: the moves from the seed to each cell, as flood_maps counts them; True: the moves
    from each cell to the seed, the same directed moves followed backwards -- with a goal's cell as the seed, the walking distance
    to the goal from everywhere, which across a ledge differs from the distance from the goal.  Returns the (n, H, W) int32 tensor of
    distances, 0 at the seed and FLOOD_GRID_UNREACHED (-1 as int32) where no path leads, where the cell is closed, and everywhere
    when the seed is closed or outside the grid (dist_out: a 32-bit integer tensor, or a raw device pointer, to write instead of a
    new one); with count_out True, an (n,) 32-bit integer tensor or a raw device pointer, returns (distances, counts).  For a grid
    flood_maps takes and towards False the two give the same distances.  One launch, asynchronous on `stream` (None, a torch stream
    or a raw handle); it can be captured into a graph."""
    n, height, width = _flood_inputs(floor, ceiling, seeds)
    dist_out, pd, count_out, pc = _flood_outputs(n, height, width, floor.device, dist_out, count_out, 4)
    params = FloodParams(max_step, max_drop, clearance, FLOOD_TOWARDS if towards else 0)
    v = ctypes.c_void_p
    _check(lib().rdoom_flood_grids(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height, v(seeds.data_ptr()) if seeds is not None else None,
                                   ctypes.byref(params), v(pd), v(pc), v(_stream_handle(stream))))
    return dist_out if count_out is None else (dist_out, count_out)


def _int32_out(t, shape, device, what):
    """an int32 output of `shape`: None allocates, a 32-bit integer tensor of that many elements or a raw device pointer is used as
    given.  Returns (tensor or the pointer, pointer)"""
    import torch
    if t is None or t is True:
        t = torch.empty(shape, dtype=torch.int32, device=device)
    if isinstance(t, int) and not isinstance(t, bool):
        return t, t
    if not isinstance(t, torch.Tensor) or t.element_size() != 4 or t.dtype.is_floating_point:
        raise ValueError('%s must be a 32-bit integer tensor or a device pointer' % what)
    return t, _out_tensor(t, int(np.prod(shape)) * 4, what)


def _descend(entry, params, floor, ceiling, dist, starts, max_moves, stop_dist, cells_out, moves_out, path_out, stream):
    """descend_grids' and descend_grids_octile's arguments, checked, and the call of `entry` (rdoom_flood_descend's signature) with
    `params`; what they return"""
    import torch
    n, height, width = _flood_inputs(floor, ceiling, None)
    if not isinstance(starts, torch.Tensor) or starts.device.type != 'cuda' or not starts.is_contiguous() or starts.dtype != torch.int32 or \
            tuple(starts.shape) != (n, 2):
        raise ValueError('starts must be a contiguous int32 (%d, 2) tensor of (column, row) on the GPU' % n)
    if not isinstance(dist, torch.Tensor) or dist.device.type != 'cuda' or not dist.is_contiguous() or dist.element_size() != 4 or \
            dist.dtype.is_floating_point or tuple(dist.shape) != (n, height, width):
        raise ValueError('dist must be a contiguous 32-bit integer (%d, %d, %d) tensor on the GPU' % (n, height, width))
    cells_out, pc = _int32_out(cells_out, (n, 2), floor.device, 'cells_out')
    moves_out, pm = _int32_out(moves_out, (n,), floor.device, 'moves_out')
    pp, path_len = None, 0
    if path_out is not None:
        if isinstance(path_out, int) and not isinstance(path_out, bool):
            path_out = torch.empty((n, path_out, 2), dtype=torch.int32, device=floor.device)
        if not isinstance(path_out, torch.Tensor) or path_out.dim() != 3 or path_out.shape[0] != n or path_out.shape[2] != 2:
            raise ValueError('path_out must be a length or a 32-bit integer (%d, length, 2) tensor' % n)
        path_len = int(path_out.shape[1])
        path_out, pp = _int32_out(path_out, (n, path_len, 2), floor.device, 'path_out')
    v = ctypes.c_void_p
    _check(entry(v(floor.data_ptr()), v(ceiling.data_ptr()), v(dist.data_ptr()), n, width, height, v(starts.data_ptr()), ctypes.byref(params),
                 ctypes.c_uint32(0xFFFFFFFF if max_moves is None else int(max_moves)), ctypes.c_uint32(int(stop_dist)), v(pc), v(pm), v(pp),
                 path_len, v(_stream_handle(stream))))
    return (cells_out, moves_out) if path_out is None else (cells_out, moves_out, path_out)


def descend_grids(floor, ceiling, dist, starts, towards=False, max_moves=None, stop_dist=0, max_step=0.24, max_drop=float('inf'), clearance=0.56,
                  cells_out=None, moves_out=None, path_out=None, stream=None):
    """rdoom_flood_descend: walk flood_grids' field downhill.  floor, ceiling: the planes that flood took; dist: the (n, H, W)
    distances it returned with the same towards, max_step, max_drop and clearance; starts: an int32 (n, 2) tensor of (column, row),
    area_cells' or area_frontiers' layout.  From its start every row steps to the first 4-neighbour (left, right, up, down) whose
    distance is one less and which the field's directed moves connect -- a ledge is dropped from and not climbed, which the
    distances alone do not say -- until the distance is stop_dist or max_moves (None: no limit) moves are made.  Returns (cells,
    moves): the int32 (n, 2) cell reached, (-1, -1) for a start outside the grid or on an unreached cell, and the int32 (n,) moves
    made.  With towards=True and max_moves=K the cell is the waypoint K moves ahead on a shortest path to the goal (the goal itself
    if nearer); on a forward field, from a frontier cell with stop_dist=K, it is the cell K moves from the player on the way
    there.  path_out: an int (the length to allocate) or a 32-bit integer (n, length, 2) tensor: entry k is the cell after move
    k + 1, (-1, -1) past the walk's end; then (cells, moves, path) is returned.  cells_out, moves_out: tensors or raw device
    pointers to write instead of new ones.  One launch, asynchronous on `stream` (None, a torch stream or a raw handle); it can be
    captured into a graph."""
    params = FloodParams(max_step, max_drop, clearance, FLOOD_TOWARDS if towards else 0)
    return _descend(lib().rdoom_flood_descend, params, floor, ceiling, dist, starts, max_moves, stop_dist, cells_out, moves_out, path_out, stream)


class FloodOctileParams(ctypes.Structure):
    """rdoom_flood_octile_params"""
    _fields_ = [('max_step', ctypes.c_float), ('max_drop', ctypes.c_float), ('clearance', ctypes.c_float), ('flags', ctypes.c_uint32),
                ('axial_cost', ctypes.c_uint32), ('diagonal_cost', ctypes.c_uint32)]


def flood_grids_octile(floor, ceiling, seeds=None, towards=False, axial_cost=5, diagonal_cost=7, max_step=0.24, max_drop=float('inf'),
                       clearance=0.56, dist_out=None, count_out=None, stream=None):
    """rdoom_flood_grids_octile: flood_grids over moves to the eight neighbours.  floor, ceiling, seeds, towards, max_step, max_drop,
    clearance, dist_out, count_out: as flood_grids takes them.  A move to a 4-neighbour costs axial_cost; a diagonal move costs
    diagonal_cost and is allowed exactly when the four axial moves round both sides of it are, so it never cuts the corner of a
    closed cell, a ledge or a door.  1 <= axial_cost <= diagonal_cost <= 2 * axial_cost, and axial_cost * H * W is at most
    0xFFFFFF.  Returns the (n, H, W) int32 tensor of smallest total costs, 0 at the seed and FLOOD_GRID_UNREACHED (-1 as int32)
    exactly where flood_grids has it (with count_out: (costs, counts)); cost * cell / axial_cost is the length in world units,
    with the default (5, 7) within -1 % and +8 % of the straight line in free space.  With diagonal_cost == 2 * axial_cost the
    result is axial_cost * flood_grids'.  One launch, asynchronous on `stream` (None, a torch stream or a raw handle); it can be
    captured into a graph."""
    n, height, width = _flood_inputs(floor, ceiling, seeds)
    dist_out, pd, count_out, pc = _flood_outputs(n, height, width, floor.device, dist_out, count_out, 4)
    params = FloodOctileParams(max_step, max_drop, clearance, FLOOD_TOWARDS if towards else 0, int(axial_cost), int(diagonal_cost))
    v = ctypes.c_void_p
    _check(lib().rdoom_flood_grids_octile(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height,
                                          v(seeds.data_ptr()) if seeds is not None else None, ctypes.byref(params), v(pd), v(pc),
                                          v(_stream_handle(stream))))
    return dist_out if count_out is None else (dist_out, count_out)


def descend_grids_octile(floor, ceiling, dist, starts, towards=False, axial_cost=5, diagonal_cost=7, max_moves=None, stop_dist=0, max_step=0.24,
                         max_drop=float('inf'), clearance=0.56, cells_out=None, moves_out=None, path_out=None, stream=None):
    """rdoom_flood_descend_octile: descend_grids down flood_grids_octile's field.  dist: the costs that call returned with the same
    towards, costs and limits.  Every row steps to the first of its eight neighbours -- left, right, up, down, then the (column,
    row) offsets (-1, -1), (+1, -1), (-1, +1), (+1, +1) -- whose cost plus the move's equals the cell's and which the field's
    directed moves connect, until the cost is at most stop_dist (in cost units) or max_moves (None: no limit) moves are made.
    starts, cells_out, moves_out, path_out, the return value and a start outside the grid or on an unreached cell: as
    descend_grids has them; moves count moves, not cost.  One launch, asynchronous on `stream`; it can be captured into a graph."""
    params = FloodOctileParams(max_step, max_drop, clearance, FLOOD_TOWARDS if towards else 0, int(axial_cost), int(diagonal_cost))
    return _descend(lib().rdoom_flood_descend_octile, params, floor, ceiling, dist, starts, max_moves, stop_dist, cells_out, moves_out, path_out,
                    stream)


def _cells_in(t, shape, what):
    """an int32 input of (column, row) cells of `shape` on the GPU, checked"""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous() or t.dtype != torch.int32 or tuple(t.shape) != shape:
        raise ValueError('%s must be a contiguous int32 %s tensor of (column, row) on the GPU' % (what, shape))


def walk_lines(floor, ceiling, starts, targets, reversed=False, max_step=0.24, max_drop=float('inf'), clearance=0.56, clear_out=None,
               stop_out=None, stream=None):
    """rdoom_grid_walk_lines: can each target be walked to in a straight line?  floor, ceiling: the (n, H, W) planes flood_grids
    takes; starts: an int32 (n, 2) tensor of (column, row), area_cells' layout; targets: an int32 (n, q, 2) tensor.  Line (p, k)
    is the chain of grid moves the segment from the centre of starts[p] to the centre of targets[p, k] makes -- a column or row
    move at every boundary it crosses, a diagonal move where it passes exactly through a cell corner -- and it is clear when both
    cells are inside the grid, the start is open and every move is allowed by flood_grids' rules with max_step, max_drop and
    clearance, a diagonal by flood_grids_octile's: no corner of a closed cell, a ledge or a door is cut.  reversed: every move is
    tested from its far cell back to its near one, the walk from the target to the start over the same cells.  Returns the (n, q)
    uint8 tensor, 1 for clear (clear_out: a one-byte tensor or a raw device pointer to write instead); with stop_out True, a 32-bit
    integer (n, q, 2) tensor or a raw device pointer, returns (clear, stop): the last cell reached from the start -- the target
    when clear, else the cell the first refused move starts from, (-1, -1) when either end is outside the grid.  One launch,
    asynchronous on `stream` (None, a torch stream or a raw handle); it can be captured into a graph."""
    import torch
    n, height, width = _flood_inputs(floor, ceiling, None)
    _cells_in(starts, (n, 2), 'starts')
    if not isinstance(targets, torch.Tensor) or targets.dim() != 3:
        raise ValueError('targets must be a contiguous int32 (%d, q, 2) tensor of (column, row) on the GPU' % n)
    q = int(targets.shape[1])
    _cells_in(targets, (n, q, 2), 'targets')
    if clear_out is None:
        clear_out = torch.empty((n, q), dtype=torch.uint8, device=floor.device)
    if isinstance(clear_out, int) and not isinstance(clear_out, bool):
        pc = clear_out  # a raw device pointer to n * q bytes
    elif not isinstance(clear_out, torch.Tensor) or clear_out.element_size() != 1:
        raise ValueError('clear_out must be a one-byte tensor or a device pointer')
    else:
        pc = _out_tensor(clear_out, n * q, 'clear_out')
    ps = None
    if stop_out is not None and stop_out is not False:
        stop_out, ps = _int32_out(stop_out, (n, q, 2), floor.device, 'stop_out')
    else:
        stop_out = None
    params = FloodParams(max_step, max_drop, clearance, LINE_REVERSED if reversed else 0)
    v = ctypes.c_void_p
    _check(lib().rdoom_grid_walk_lines(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height, v(starts.data_ptr()), v(targets.data_ptr()),
                                       q, ctypes.byref(params), v(pc), v(ps), v(_stream_handle(stream))))
    return clear_out if stop_out is None else (clear_out, stop_out)


def straighten_paths(floor, ceiling, starts, path, towards=False, max_look=64, corners=8, max_step=0.24, max_drop=float('inf'), clearance=0.56,
                     count_out=None, length_out=None, stream=None):
    """rdoom_path_straighten: pull a descent's staircase straight.  floor, ceiling, starts: as descend_grids took them; path: the
    int32 (n, length, 2) path it or descend_grids_octile wrote, or any list of cells ended by (-1, -1); towards, max_step, max_drop,
    clearance: the descent's -- with towards the lines are walked in the listed direction, without it from the listed cell back,
    because a forward field's path is listed from the far end to the player.  From its start every row takes as its next corner
    the farthest of the next max_look (at most STRAIGHTEN_MAX_LOOK) cells of the path that walk_lines calls clear from the last
    corner, and goes on behind it, until the path ends, no cell ahead is clear or `corners` are found.  corners: an int (the
    number to allocate) or a 32-bit integer (n, number, 2) tensor.  Returns (corners, count): the int32 corners, (-1, -1) past the
    last, and the int32 (n,) number found -- corners[:, 0] is the any-angle waypoint, the cell to head for; with length_out True, a
    float32 (n,) tensor or a raw device pointer, returns (corners, count, length): the summed Euclidean length of the straight
    walks in cells, times the cell size in world units.  count_out: a tensor or a raw device pointer to write instead of a new
    one.  One launch, asynchronous on `stream` (None, a torch stream or a raw handle); it can be captured into a graph."""
    import torch
    n, height, width = _flood_inputs(floor, ceiling, None)
    _cells_in(starts, (n, 2), 'starts')
    if not isinstance(path, torch.Tensor) or path.dim() != 3:
        raise ValueError('path must be a contiguous int32 (%d, length, 2) tensor of (column, row) on the GPU' % n)
    path_len = int(path.shape[1])
    _cells_in(path, (n, path_len, 2), 'path')
    if isinstance(corners, int) and not isinstance(corners, bool):
        corners = torch.empty((n, corners, 2), dtype=torch.int32, device=floor.device)
    if not isinstance(corners, torch.Tensor) or corners.dim() != 3 or corners.shape[0] != n or corners.shape[2] != 2:
        raise ValueError('corners must be a number or a 32-bit integer (%d, number, 2) tensor' % n)
    corner_len = int(corners.shape[1])
    corners, pk = _int32_out(corners, (n, corner_len, 2), floor.device, 'corners')
    count_out, pc = _int32_out(count_out, (n,), floor.device, 'count_out')
    pl = None
    if length_out is None or length_out is False:
        length_out = None
    elif isinstance(length_out, int) and not isinstance(length_out, bool):
        pl = length_out  # a raw device pointer to n floats
    else:
        if length_out is True:
            length_out = torch.empty(n, dtype=torch.float32, device=floor.device)
        if not isinstance(length_out, torch.Tensor) or length_out.dtype != torch.float32:
            raise ValueError('length_out must be True, a float32 tensor or a device pointer')
        pl = _out_tensor(length_out, n * 4, 'length_out')
    params = FloodParams(max_step, max_drop, clearance, FLOOD_TOWARDS if towards else 0)
    v = ctypes.c_void_p
    _check(lib().rdoom_path_straighten(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height, v(starts.data_ptr()), v(path.data_ptr()),
                                       path_len, ctypes.byref(params), ctypes.c_uint32(int(max_look)), v(pk), corner_len, v(pc), v(pl),
                                       v(_stream_handle(stream))))
    return (corners, count_out) if length_out is None else (corners, count_out, length_out)


class WallParams(ctypes.Structure):
    """rdoom_wall_params"""
    _fields_ = [('clearance', ctypes.c_float), ('radius', ctypes.c_uint32), ('close_d2', ctypes.c_uint32), ('flags', ctypes.c_uint32)]


def wall_close_d2(radius, cell):
    """the close_d2 of a body of `radius` on a grid of `cell`: a blocked centre within radius of a cell's centre is D2 <= (radius / cell) ** 2"""
    return int(math.floor((float(radius) / float(cell)) ** 2))


def _wall_radius(close_d2):
    """the smallest R >= 1 with R * R >= close_d2; ValueError above WALL_MAX_RADIUS"""
    r = max(1, math.isqrt(close_d2 - 1) + 1) if close_d2 > 0 else 1
    if r > WALL_MAX_RADIUS:
        raise ValueError('close_d2 %d needs a radius of %d cells: at most %d (a coarser cell, or a smaller body)' % (close_d2, r, WALL_MAX_RADIUS))
    return r


def _plane_out(t, like, what):
    """an output plane shaped like `like`: None allocates, a float32 tensor of that many bytes or a raw device pointer is used as
    given.  Returns (tensor or the pointer, pointer)"""
    import torch
    if t is None:
        t = torch.empty_like(like)
    if isinstance(t, int) and not isinstance(t, bool):
        return t, t
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError('%s must be a float32 tensor or a device pointer' % what)
    return t, _out_tensor(t, like.numel() * 4, what)


def _wall_distance(floor, ceiling, radius, close_d2, clearance, edge_open, pd, pf, pc, stream):
    n, height, width = (int(x) for x in floor.shape)
    params = WallParams(clearance, radius, close_d2, WALL_EDGE_OPEN if edge_open else 0)
    v = ctypes.c_void_p
    _check(lib().rdoom_wall_distance(v(floor.data_ptr()), v(ceiling.data_ptr()), n, width, height, ctypes.byref(params), v(pd), v(pf), v(pc),
                                     v(_stream_handle(stream))))


def wall_distances(floor, ceiling, radius_cells, clearance=0.56, edge_open=False, dist2_out=None, stream=None):
    """rdoom_wall_distance, the distances alone: how far the nearest wall is from every cell.  floor, ceiling: the float32 (n, H, W)
    GPU tensors flood_maps or flood_grids take; a cell blocks when it is not open (floor finite and ceiling - floor >= clearance),
    and so does every position outside the grid unless edge_open -- True for draw_sector_maps' window, whose edge is unknown and
    not a wall.  Returns the (n, H, W) uint16 tensor of D2, the squared distance in cells to the nearest blocking cell: exact where
    D2 <= radius_cells ** 2 (1 .. WALL_MAX_RADIUS), 0 on a closed cell, WALL_FAR beyond (dist2_out: a 16-bit integer tensor, or a
    raw device pointer, to write instead of a new one).  One launch, asynchronous on `stream` (None, a torch stream or a raw handle);
    it can be captured into a graph."""
    n, height, width = _flood_inputs(floor, ceiling, None)
    dist2_out, pd, _, _ = _flood_outputs(n, height, width, floor.device, dist2_out, None, 2)
    _wall_distance(floor, ceiling, int(radius_cells), 0, clearance, edge_open, pd, None, None, stream)
    return dist2_out


def inflate_grids(floor, ceiling, radius, cell, clearance=0.56, edge_open=False, floor_out=None, ceiling_out=None, dist2_out=None, stream=None):
    """rdoom_wall_distance, the planes: floor and ceiling with every cell a body of `radius` cannot stand in made void (+inf / -inf)
    -- the cells with a blocking cell's centre within `radius` of their own, D2 <= wall_close_d2(radius, cell) -- and every other
    word as it was.  radius and cell are in the level's units (World.step's body: 0.19).  The result goes through flood_maps,
    flood_grids, descend_grids and area_frontiers as it is.  Returns (floor, ceiling), new tensors or floor_out / ceiling_out (float32
    tensors or raw device pointers, not the inputs: there is no in-place form); with dist2_out True, a 16-bit integer tensor or a raw
    device pointer, (floor, ceiling, dist2) with wall_distances' D2 up to the launch's radius, the smallest R with R * R >= close_d2.
    ValueError when that R is above WALL_MAX_RADIUS.  A radius below the cell's size (0.19 at cell 0.25) gives close_d2 0: only
    closed cells are touched.  One launch, asynchronous on `stream`; it can be captured into a graph."""
    n, height, width = _flood_inputs(floor, ceiling, None)
    close_d2 = wall_close_d2(radius, cell)
    r = _wall_radius(close_d2)
    floor_out, pf = _plane_out(floor_out, floor, 'floor_out')
    ceiling_out, pc = _plane_out(ceiling_out, ceiling, 'ceiling_out')
    pd = None
    if dist2_out is not None and dist2_out is not False:
        dist2_out, pd, _, _ = _flood_outputs(n, height, width, floor.device, None if dist2_out is True else dist2_out, None, 2)
    _wall_distance(floor, ceiling, r, close_d2, clearance, edge_open, pd, pf, pc, stream)
    return (floor_out, ceiling_out) if pd is None else (floor_out, ceiling_out, dist2_out)


class StampParams(ctypes.Structure):
    """rdoom_stamp_params (STAMP_PARAMS is the same record for numpy)"""
    _fields_ = [('grow', ctypes.c_float), ('block_below', ctypes.c_float), ('block_above', ctypes.c_float), ('flags', ctypes.c_uint32)]


def _stamp_things(call, levels, floor, ceiling, things, cell, solid, hidden, offsets, grow, block_below, block_above, floor_out, ceiling_out,
                  index_out, stream, n, n_objects, stride):
    """World.stamp_things / WorldSet.stamp_things: the checks and the launch; call(levels, n, offsets, n_objects, cell, width, height,
    solid, hidden, stride, params, floor, ceiling, floor_out, ceiling_out, index_out, stream) is the C entry point with its handle and
    the thing set bound"""
    import torch
    if not isinstance(things, DeviceThings):
        raise ValueError('things must be a DeviceThings')
    rows, height, width = _flood_inputs(floor, ceiling, None)
    n = rows if n is None else int(n)
    if not 0 <= n <= rows:
        raise ValueError('n = %d, but the planes have %d rows' % (n, rows))
    raw = lambda t: isinstance(t, (int, np.integer)) and not isinstance(t, bool)
    if levels is not None and not raw(levels) and (levels.element_size() != 4 or levels.numel() < n):
        raise ValueError('levels must hold one 32-bit slot per row (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    if solid is not None and not raw(solid) and solid.dim() == 1:
        solid = solid.reshape(1, -1)
    for r, what, need in ((solid, 'solid', things.n_levels), (hidden, 'hidden', n)):
        if r is None:
            continue
        if raw(r):
            if stride is None:
                raise ValueError('stride is needed with a raw %s pointer' % what)
            continue
        if r.element_size() != 4 or r.dtype.is_floating_point or r.dim() != 2:
            raise ValueError('%s must be a 32-bit integer (rows, words) tensor' % what)
        if int(r.shape[0]) < need:
            raise ValueError('the %s tensor has %d rows, the call needs %d' % (what, int(r.shape[0]), need))
        if stride is not None and int(stride) != int(r.shape[1]):
            raise ValueError('stride %d, but the %s rows are %d words long' % (int(stride), what, int(r.shape[1])))
        stride = int(r.shape[1])
    stride = 0 if stride is None else int(stride)
    n_obj = 0
    if offsets is not None:
        if raw(offsets):
            if n_objects is None:
                raise ValueError('n_objects is needed with a raw offsets pointer')
            n_obj = int(n_objects)
        else:
            if offsets.dim() != 3 or int(offsets.shape[0]) < n or offsets.shape[2] != 3 or offsets.dtype != torch.float32:
                raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d rows, got %s' % (n, tuple(offsets.shape)))
            n_obj = int(offsets.shape[1])
    wants_index = index_out is not None and index_out is not False
    if (floor_out is False) != (ceiling_out is False) or (floor_out is None) != (ceiling_out is None):
        raise ValueError('floor_out and ceiling_out go together: both given, both None (allocated) or both False (no planes)')
    if floor_out is False:
        if not wants_index:
            raise ValueError('nothing asked for: no planes and no index_out')
        floor_out = ceiling_out = pf = pc = None
    else:
        floor_out, pf = _plane_out(floor_out, floor, 'floor_out')
        ceiling_out, pc = _plane_out(ceiling_out, ceiling, 'ceiling_out')
    if index_out is True:
        index_out = torch.empty((rows, height, width), dtype=torch.int32, device=floor.device)
    elif not wants_index:
        index_out = None
    elif not raw(index_out) and (not isinstance(index_out, torch.Tensor) or index_out.dtype != torch.int32):
        raise ValueError('index_out must be True, an int32 (n, height, width) tensor or a device pointer')
    cells = n * height * width
    params = StampParams(grow, block_below, block_above, 0)
    v = ctypes.c_void_p
    _check(call(v(_pointer(levels, n * 4, 'levels')), n, v(_pointer(offsets, n * n_obj * 12, 'offsets')), n_obj, ctypes.c_float(cell), width, height,
                v(_pointer(solid, things.n_levels * stride * 4, 'solid')), v(_pointer(hidden, n * stride * 4, 'hidden')), stride, ctypes.byref(params),
                v(floor.data_ptr()), v(ceiling.data_ptr()), v(pf), v(pc), v(_pointer(index_out, cells * 4, 'index_out')), v(_stream_handle(stream))))
    if floor_out is None:
        return index_out
    return (floor_out, ceiling_out, index_out) if index_out is not None else (floor_out, ceiling_out)


_STAMP_DOC = """makes void (+inf / -inf) the cells of floor and ceiling -- draw_area_planes' float32 (n, H, W) tensors at
        this `cell` -- that a solid thing of `things` (a DeviceThings) stands on, per row and in the row's own game, so that
        inflate_grids, flood_grids, flood_grids_octile, descend_grids, walk_lines, straighten_paths and area_frontiers route round
        them.  A thing covers the cells whose centre lies within radius + grow of it, and always the cell it stands in.  solid: None
        (every thing) or an int32 (levels, words >= things.words()) GPU tensor of obstacle bits, one row a level of the set --
        torch.from_numpy(pack_things(world.thing_obstacles())).cuda(); hidden: None or sense_things' `collected` (n, words) tensor as it
        stands: a thing row p has collected no longer blocks row p, and only row p.  offsets: None (at rest) or step_game's tensor:
        a thing on a lift rides it.  block_below / block_above: how far the cell's floor may lie below / above the thing's live
        height for the thing to block it (inf: no vertical test).  floor_out / ceiling_out: None allocates; the inputs themselves
        stamp in place (no other overlap is allowed); False for both: no planes, the index alone.  index_out: None / False, True
        (allocated) or an int32 (n, H, W) tensor: the lowest blocking thing of each cell, -1 where none blocks.  Every other word
        passes through untouched.  solid, hidden, offsets and the outputs may instead be raw device pointers (ints; then stride,
        and with offsets n_objects, must be given); n: the rows to stamp when fewer than the planes'.  Stamp with grow=0 before
        inflate_grids, or with grow=0.19 (the body's radius) without it.  Returns what was asked for: (floor, ceiling),
        (floor, ceiling, index) or index.  One launch, asynchronous on `stream`; it can be captured into a graph."""


class RayThings(ctypes.Structure):
    """rdoom_ray_things (RAY_THINGS is the same record for numpy)"""
    _fields_ = [('height', ctypes.c_float * 8), ('grow', ctypes.c_float), ('category_mask', ctypes.c_uint32), ('flags', ctypes.c_uint32)]


def _cast_rays_things(call, states, levels, things, dirs, max_range, heights, grow, categories, select, hidden, offsets, frac, frac_out,
                      thing_out, stream, n, n_objects, stride):
    """World.cast_rays_things / WorldSet.cast_rays_things: the checks and the launch; call(states, levels, n, dirs, n_rays, max_range,
    offsets, n_objects, params, select, hidden, stride, frac_in, frac_out, thing_out, stream) is the C entry point with its handle and
    the thing set bound"""
    import torch
    if not isinstance(things, DeviceThings):
        raise ValueError('things must be a DeviceThings')
    raw = lambda t: isinstance(t, (int, np.integer)) and not isinstance(t, bool)
    if not isinstance(dirs, torch.Tensor) or dirs.device.type != 'cuda' or not dirs.is_contiguous() or dirs.dtype != torch.float32 or \
            dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.shape[0] == 0:
        raise ValueError('dirs must be a contiguous float32 (n_rays, 3) tensor on the GPU with n_rays >= 1')
    n_rays = int(dirs.shape[0])
    if raw(states):
        if n is None:
            raise ValueError('n is needed with raw pointers')
        n = int(n)
    else:
        n = _n_players(states) if n is None else int(n)
    if levels is not None and not raw(levels) and (levels.element_size() != 4 or levels.numel() < n):
        raise ValueError('levels must hold one 32-bit slot per player (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    if select is not None and not raw(select) and select.dim() == 1:
        select = select.reshape(1, -1)
    for r, what, need in ((select, 'select', things.n_levels), (hidden, 'hidden', n)):
        if r is None:
            continue
        if raw(r):
            if stride is None:
                raise ValueError('stride is needed with a raw %s pointer' % what)
            continue
        if r.element_size() != 4 or r.dtype.is_floating_point or r.dim() != 2:
            raise ValueError('%s must be a 32-bit integer (rows, words) tensor' % what)
        if int(r.shape[0]) < need:
            raise ValueError('the %s tensor has %d rows, the call needs %d' % (what, int(r.shape[0]), need))
        if stride is not None and int(stride) != int(r.shape[1]):
            raise ValueError('stride %d, but the %s rows are %d words long' % (int(stride), what, int(r.shape[1])))
        stride = int(r.shape[1])
    stride = 0 if stride is None else int(stride)
    n_obj = 0
    if offsets is not None:
        if raw(offsets):
            if n_objects is None:
                raise ValueError('n_objects is needed with a raw offsets pointer')
            n_obj = int(n_objects)
        else:
            if offsets.dim() != 3 or int(offsets.shape[0]) < n or offsets.shape[2] != 3 or offsets.dtype != torch.float32:
                raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d players, got %s' % (n, tuple(offsets.shape)))
            n_obj = int(offsets.shape[1])
    heights = [float(heights)] * THING_CATEGORIES if np.isscalar(heights) else [float(h) for h in heights]
    if len(heights) != THING_CATEGORIES:
        raise ValueError('heights must be a number or eight, one per category, got %d' % len(heights))
    mask = 0
    for c in (range(THING_CATEGORIES) if categories is None else ((categories,) if isinstance(categories, (int, np.integer)) else categories)):
        if not 0 <= int(c) < THING_CATEGORIES:
            raise ValueError('categories names categories 0 .. 7, not %r' % (c,))
        mask |= 1 << int(c)
    for t, what in ((frac, 'frac'), (frac_out, 'frac_out')):
        if t is not None and not raw(t) and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise ValueError('%s must be a float32 tensor or a device pointer' % what)
    rays = n * n_rays
    if frac_out is None:
        if raw(states):
            raise ValueError('frac_out is needed with raw pointers')
        frac_out = torch.empty((n, n_rays), dtype=torch.float32, device=dirs.device)
    if thing_out is True:
        thing_out = torch.empty((n, n_rays), dtype=torch.int32, device=dirs.device)
    elif thing_out is None or thing_out is False:
        thing_out = None
    elif not raw(thing_out) and (not isinstance(thing_out, torch.Tensor) or thing_out.dtype != torch.int32):
        raise ValueError('thing_out must be True, an int32 (n, n_rays) tensor or a device pointer')
    params = RayThings((ctypes.c_float * 8)(*heights), grow, mask, 0)
    v = ctypes.c_void_p
    _check(call(v(_pointer(states, n * PLAYER_STATE.itemsize, 'states')), v(_pointer(levels, n * 4, 'levels')), n, v(dirs.data_ptr()), n_rays,
                ctypes.c_float(max_range), v(_pointer(offsets, n * n_obj * 12, 'offsets')), n_obj, ctypes.byref(params),
                v(_pointer(select, things.n_levels * stride * 4, 'select')), v(_pointer(hidden, n * stride * 4, 'hidden')), stride,
                v(_pointer(frac, rays * 4, 'frac')), v(_pointer(frac_out, rays * 4, 'frac_out')), v(_pointer(thing_out, rays * 4, 'thing_out')),
                v(_stream_handle(stream))))
    return frac_out, thing_out


_RAY_THINGS_DOC = """shortens the rays of cast_rays(states, dirs, max_range) that meet a thing of `things` (a
        DeviceThings) before they meet the world, per player and in that player's own game: a second pass after cast_rays, one
        launch.  A thing is a vertical cylinder of its radius + grow, heights[category] tall (a number, or eight; inf: no top),
        standing on its live base, or hanging from it.  categories: None (all) or an iterable of THING_*; select: None (every thing)
        or an int32 (levels, words >= things.words()) GPU tensor of bits, one row a level of the set --
        torch.from_numpy(pack_things(world.thing_obstacles())).cuda() gives the obstacles only; hidden: None or sense_things'
        `collected` (n, words) tensor as it stands: a thing player p has collected is passed by p's rays, and only p's.  offsets:
        None (at rest) or step_game's tensor: a barrel on a lift rides it.  frac: None (every ray starts at +inf) or the float32
        (n, n_rays) fractions cast_rays wrote; the thing wins only when strictly nearer.  frac_out: None allocates; frac itself runs
        in place (no other overlap is allowed).  thing_out: None / False, True (allocated) or an int32 (n, n_rays) tensor: the index
        of the thing each ray ends on, -1 where it ends on the world or on nothing.  states, levels, select, hidden, offsets, frac and
        the outputs may instead be raw device pointers (ints; then n, stride, and with offsets n_objects, must be given).  Returns
        (frac_out, thing_out).  Asynchronous on `stream`; it can be captured into a graph."""


def _area_frontiers(call, words, levels, area, dist, cell, cell_out, dist_out, count_out, mask_out, stream):
    """World.area_frontiers / WorldSet.area_frontiers: the checks and the launch; call(levels, n, cell, width, height, area, stride,
    dist, cell_out, dist_out, count_out, mask_out, stream) is the C entry point with its handle bound.  Returns cell_out, or a tuple
    of it and the optional outputs asked for, in the order dist, count, mask"""
    import torch
    if not isinstance(dist, torch.Tensor) or dist.device.type != 'cuda' or not dist.is_contiguous() or dist.element_size() != 4 or \
            dist.dtype.is_floating_point or dist.dim() != 3:
        raise ValueError('dist must be a contiguous 32-bit integer (n, height, width) tensor on the GPU')
    n, height, width = (int(x) for x in dist.shape)
    if levels is not None and (not isinstance(levels, torch.Tensor) or levels.device.type != 'cuda' or not levels.is_contiguous() or
                               levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per row (%d) in a contiguous tensor on the GPU' % n)
    pa, stride = _area_rows(area, n, words)
    cell_out, pc = _int32_out(cell_out, (n, 2), dist.device, 'cell_out')
    optional = []
    for want, what in ((dist_out, 'dist_out'), (count_out, 'count_out')):
        optional.append((None, None) if want is None or want is False else _int32_out(want, (n,), dist.device, what))
    if mask_out is None or mask_out is False:
        optional.append((None, None))
    else:
        if mask_out is True:
            mask_out = torch.empty((n, height, width), dtype=torch.uint8, device=dist.device)
        elif not isinstance(mask_out, torch.Tensor) or mask_out.element_size() != 1:
            raise ValueError('mask_out must be True or a one-byte (n, height, width) tensor')
        optional.append((mask_out, _out_tensor(mask_out, n * height * width, 'mask_out')))
    v = ctypes.c_void_p
    _check(call(v(levels.data_ptr()) if levels is not None else None, n, ctypes.c_float(cell), width, height, v(pa), stride, v(dist.data_ptr()),
                v(pc), *[v(ptr) for _, ptr in optional], v(_stream_handle(stream))))
    out = (cell_out,) + tuple(t for t, _ in optional if t is not None)
    return out[0] if len(out) == 1 else out


def _draw_area_planes(call, shape, words, levels, cell, n, offsets, area, sector_out, floor, ceiling, stream):
    """World.draw_area_planes / WorldSet.draw_area_planes: the checks and the launch; call(levels, n, offsets, n_objects, cell,
    width, height, area, stride, sector_out, floor_out, ceiling_out, stream) is the C entry point with its handle bound.  Returns
    the planes asked for, in the order sector, floor, ceiling: one tensor, or a tuple of them"""
    import torch
    given = [t for t in (levels, offsets, area, sector_out, floor, ceiling) if isinstance(t, torch.Tensor)]
    for t, what in ((levels, 'levels'), (offsets, 'offsets')):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or not t.is_contiguous()):
            raise ValueError('%s must be a contiguous tensor on the GPU' % what)
    if n is None:  # the rows of the first tensor given, else 1
        n = int(given[0].numel()) if levels is not None else (int(given[0].shape[0]) if given else 1)
    n = int(n)
    if levels is not None and (levels.element_size() != 4 or levels.numel() != n):
        raise ValueError('levels must hold one 32-bit slot per row (%d), got %s %s' % (n, levels.dtype, tuple(levels.shape)))
    n_obj = 0
    if offsets is not None:
        if offsets.dtype != torch.float32 or offsets.dim() != 3 or offsets.shape[0] != n or offsets.shape[2] != 3:
            raise ValueError('offsets must be a float32 (n, n_objects, 3) tensor for %d rows, got %s %s' % (n, offsets.dtype, tuple(offsets.shape)))
        n_obj = int(offsets.shape[1])
    pa, stride = _area_rows(area, n, words) if area is not None else (None, 0)
    height, width = shape
    device = given[0].device if given else torch.device('cuda', torch.cuda.current_device())
    asked = ((sector_out, torch.int16, 'sector_out'), (floor, torch.float32, 'floor'), (ceiling, torch.float32, 'ceiling'))
    # the caller's tensors first: they set the (padded) extent of every plane, those allocated here too
    mine = []
    for want, dtype, what in asked:
        if want is None or want is False or want is True:
            continue
        if not isinstance(want, torch.Tensor) or want.element_size() != (2 if dtype == torch.int16 else 4) or \
                want.dtype.is_floating_point != (dtype == torch.float32) or want.dim() != 3 or want.shape[0] != n:
            raise ValueError('%s must be True or a %s (n, height, width) tensor' % (what, '16-bit integer' if dtype == torch.int16 else 'float32'))
        mine.append(want)
    if mine:
        height, width = int(mine[0].shape[1]), int(mine[0].shape[2])
        if any(tuple(t.shape) != (n, height, width) for t in mine):
            raise ValueError('the planes differ in shape: %s' % [tuple(t.shape) for t in mine])
    planes = []
    for want, dtype, what in asked:
        if want is None or want is False:
            planes.append(None)
            continue
        if want is True:
            want = torch.empty((n, height, width), dtype=dtype, device=device)
        _out_tensor(want, n * height * width * want.element_size(), what)
        planes.append(want)
    if all(t is None for t in planes):
        raise ValueError('no plane asked for: sector_out, floor and ceiling are all off')
    v = ctypes.c_void_p
    _check(call(v(levels.data_ptr()) if levels is not None else None, n, v(offsets.data_ptr()) if offsets is not None else None, n_obj,
                ctypes.c_float(cell), width, height, v(pa), stride, *[v(t.data_ptr()) if t is not None else None for t in planes],
                v(_stream_handle(stream))))
    out = tuple(t for t in planes if t is not None)
    return out[0] if len(out) == 1 else out


def _area_cells(call, states, levels, cell, out, stream):
    """World.area_cells / WorldSet.area_cells: the checks and the launch; call(states, levels, n, cell, out, stream) is the C entry
    point with its handle bound"""
    import torch
    n, _ = _player_tensors(states, levels, None)
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=states.device)
    elif out.dtype != torch.int32:
        raise ValueError('out must be int32')
    po = _out_tensor(out, n * 8, 'out')
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n, ctypes.c_float(cell), v(po), v(_stream_handle(stream))))
    return out


class SpawnTableArrays(ctypes.Structure):
    """rdoom_spawn_table"""
    _fields_ = [('entries', ctypes.c_void_p), ('n_entries', ctypes.c_uint32), ('start_pos', ctypes.c_float * 3), ('start_yaw', ctypes.c_float)]


class SpawnParams(ctypes.Structure):
    """rdoom_spawn_params"""
    _fields_ = [('margin', ctypes.c_float), ('clearance', ctypes.c_float), ('max_step', ctypes.c_float), ('flags', ctypes.c_uint32)]


class SpawnTable(collections.namedtuple('SpawnTable', 'entries start_pos start_yaw')):
    """a copy of a level's spawn table (rdoom_spawn_table): entries, a SPAWN_ENTRY record per floor triangle with an area (its corners
    a, b, c and the cumulative area up to and including it), in the order of arrays()['triangles']; start_pos (3,) float32 and
    start_yaw float32, the level's start, which a player without a valid candidate gets"""


def _spawn_table(get):
    """World.spawn_table / WorldSet.spawn_table: a copy of the table get(&rdoom_spawn_table) lends"""
    a = SpawnTableArrays()
    _check(get(ctypes.byref(a)))
    return SpawnTable(BuiltLevel._view(None, a.entries, a.n_entries, SPAWN_ENTRY), np.array(tuple(a.start_pos), np.float32), np.float32(a.start_yaw))


def _spawn_players(call, states, levels, seed, mask, episode, offsets, margin, clearance, max_step, flags, tries_out, stream):
    """World.spawn_players / WorldSet.spawn_players: the checks and the launch; call(states, levels, n, offsets, n_objects, mask, seed,
    episode, params, tries_out, stream) is the C entry point with its handle bound"""
    n, n_obj = _player_tensors(states, levels, offsets)
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError('seed must fit 64 bits without a sign, got %d' % seed)
    pointers = []
    for t, size, what in ((mask, 1, 'mask'), (episode, 4, 'episode'), (tries_out, 4, 'tries_out')):
        if t is None or (isinstance(t, int) and not isinstance(t, bool)):
            pointers.append(t)  # nothing, or a raw device pointer to n elements
            continue
        if not hasattr(t, 'element_size') or t.element_size() != size or t.dtype.is_floating_point:
            raise ValueError('%s must hold one %d-bit integer per player, or be a device pointer' % (what, 8 * size))
        pointers.append(_out_tensor(t, n * size, what))
    if margin is None:
        margin = float(player_config_default()['radius'])
    params = SpawnParams(margin, clearance, max_step, int(flags))
    v = ctypes.c_void_p
    _check(call(v(states.data_ptr()), v(levels.data_ptr()) if levels is not None else None, n,
                v(offsets.data_ptr()) if offsets is not None else None, n_obj, v(pointers[0]), ctypes.c_uint64(seed), v(pointers[1]),
                ctypes.byref(params), v(pointers[2]), v(_stream_handle(stream))))
    return states


class World:
    """game::world::World on the host and the current device (rdoom_world_create): World::sweep_sphere for a batch of queries,
    Player::update for a batch of players."""

    def __init__(self, wad, index, device=True):
        self._h = ctypes.c_void_p()
        self._wad = wad
        _check(lib().rdoom_world_create(wad._h, int(index), 0 if device else WORLD_HOST_ONLY, ctypes.byref(self._h)))
        a = WorldArrays()
        _check(lib().rdoom_world_host_arrays(self._h, ctypes.byref(a)))
        self.n_objects, self.node_depth = a.n_objects, a.node_depth
        self.game_objects = self.triggers()['n_objects']

    def close(self):
        if self._h:
            lib().rdoom_world_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def arrays(self):
        """copies of rdoom_world_host_arrays: nodes (WORLD_NODE), chunks (n, 2), triangles (n, 4), verts (n, 3), dynamics (n, 3:
        object id, first triangle, end), n_static_triangles, n_objects, node_depth"""
        a = WorldArrays()
        _check(lib().rdoom_world_host_arrays(self._h, ctypes.byref(a)))
        return _world_arrays(a)

    def _offsets(self, offsets, n):
        if offsets is None:
            return None, None, 0
        shape = tuple(offsets.shape)
        if len(shape) != 3 or shape[0] != n or shape[2] != 3:
            raise ValueError('object offsets must be (n, n_objects, 3), got %s' % (shape,))
        ptr, keep, _ = _device_tensor(offsets if not isinstance(offsets, np.ndarray) else np.asarray(offsets, np.float32), 'object offsets')
        return ptr, keep, shape[1]

    def sweep(self, spheres, vels, object_offsets=None, stream=None):
        """rdoom_world_sweep: spheres (n, 4) = centre xyz + radius, vels (n, 3), object_offsets None or (n, n_objects, 3)
        -> (n, 4) = time (+inf: no contact), normal xyz.  torch tensors on the GPU stay there (asynchronous on `stream`, the
        result is a new tensor); numpy arrays are copied there and back (synchronous)."""
        n = int(spheres.shape[0])
        if tuple(spheres.shape) != (n, 4) or tuple(vels.shape) != (n, 3):
            raise ValueError('spheres must be (n, 4) and vels (n, 3), got %s and %s' % (tuple(spheres.shape), tuple(vels.shape)))
        conv = (lambda a: np.asarray(a, np.float32)) if isinstance(spheres, np.ndarray) else (lambda a: a)
        ps, ks, host = _device_tensor(conv(spheres), 'spheres')
        pv, kv, _ = _device_tensor(conv(vels), 'vels')
        po, ko, n_obj = self._offsets(object_offsets, n)
        import torch
        out = torch.empty((n, 4), dtype=torch.float32, device=ks.device)
        _check(lib().rdoom_world_sweep(self._h, ctypes.c_void_p(ps), ctypes.c_void_p(pv), n, ctypes.c_void_p(po), n_obj,
                                       ctypes.c_void_p(_stream_handle(stream)), ctypes.c_void_p(out.data_ptr())))
        if host:
            torch.cuda.synchronize(ks.device)
            return out.cpu().numpy()
        return out

    def step(self, states, inputs, n_ticks=None, config=None, dt=1.0 / 60.0, object_offsets=None, stream=None):
        """rdoom_world_step_players: n_ticks ticks of Player::update for every player.  states: PLAYER_STATE records (numpy: a
        stepped copy is returned) or a contiguous GPU tensor of n * 40 bytes (stepped in place, asynchronously on `stream`).
        inputs: (n_ticks, n) PLAYER_INPUT records, or a GPU tensor of n_ticks * n * 20 bytes with n_ticks given.
        config: a PLAYER_CONFIG record or None (the defaults); object_offsets None or (n, n_objects, 3)."""
        a = _GameStepArgs(states, inputs, None, n_ticks, config)
        po, ko, n_obj = self._offsets(object_offsets, a.n)
        _check(lib().rdoom_world_step_players(self._h, ctypes.c_void_p(a.ps), ctypes.c_void_p(a.pi), a.n, int(a.n_ticks), a.cfg_ptr(),
                                              ctypes.c_float(dt), ctypes.c_void_p(po), n_obj, ctypes.c_void_p(_stream_handle(stream))))
        return a.result()

    # ---- doors, lifts and exits --------------------------------------------------------------------------------------------
    def triggers(self):
        """copies of rdoom_world_triggers: triggers (TRIGGER records, linedef order), effects (MOVE_EFFECT records), n_objects
        (the game's object count, the least n_objects of every game call)"""
        a = WorldTriggerArrays()
        _check(lib().rdoom_world_triggers(self._h, ctypes.byref(a)))
        return _trigger_arrays(a)

    def game_bytes(self):
        """rdoom_world_game_bytes: the bytes of one player's game state"""
        b = ctypes.c_uint64()
        _check(lib().rdoom_world_game_bytes(self._h, ctypes.byref(b)))
        return b.value

    def game_state(self, n, stream=None):
        """(game, offsets) for n players on the current device, reset: game an int32 tensor of n * game_bytes / 4 words, offsets a
        float32 (n, n_objects, 3) tensor"""
        import torch
        game = torch.zeros(n * self.game_bytes() // 4, dtype=torch.int32, device='cuda')
        offsets = torch.zeros((n, self.game_objects, 3), dtype=torch.float32, device='cuda')
        self.reset_game(game, offsets, stream=stream)
        return game, offsets

    def reset_game(self, game, offsets, mask=None, stream=None):
        """rdoom_world_game_reset: a fresh level (all triggers live, no effect, zero offsets) for every player, or for those whose
        mask entry is true (mask: n bools / bytes, numpy or a GPU tensor)"""
        n, n_obj = _game_args(self.game_bytes(), game, offsets)
        _reset_masked(mask, lambda pm: lib().rdoom_world_game_reset(self._h, ctypes.c_void_p(game.data_ptr()),
                                                                    ctypes.c_void_p(offsets.data_ptr()), n_obj, n, pm,
                                                                    ctypes.c_void_p(_stream_handle(stream))))

    def step_game(self, states, inputs, game, offsets, actions=None, n_ticks=None, config=None, dt=1.0 / 60.0, stream=None):
        """rdoom_world_step_game: n_ticks game ticks (physics, effects, triggers) for every player.  states / inputs / config / dt as
        for step (numpy states: a stepped copy is returned; a GPU tensor is stepped in place, asynchronously).  game, offsets: from
        game_state, on the GPU, read and written in place.  actions: None or (n_ticks, n) ACTION_* bytes (numpy or a GPU tensor)."""
        a = _GameStepArgs(states, inputs, actions, n_ticks, config)
        _, n_obj = _game_args(self.game_bytes(), game, offsets, players=a.n)
        _check(lib().rdoom_world_step_game(self._h, ctypes.c_void_p(a.ps), ctypes.c_void_p(a.pi), ctypes.c_void_p(a.pa),
                                           ctypes.c_void_p(game.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), n_obj, a.n,
                                           int(a.n_ticks), a.cfg_ptr(), ctypes.c_float(dt), ctypes.c_void_p(_stream_handle(stream))))
        return a.result()

    # ---- range-sensor rays -------------------------------------------------------------------------------------------------
    def cast_rays(self, states, dirs, max_range, offsets=None, frac_out=None, hit_out=None, origin_out=None, vel_out=None, stream=None):
        """rdoom_world_cast_rays: n_rays rays from every player's camera eye, along the player's rotation of the shared (n_rays, 3)
        float32 direction table `dirs` (ray_fan), for `max_range`.  Tensors in, tensors out, all on the GPU; asynchronous on
        `stream`, nothing is copied to the host.  states: the tensor a step leaves (n * 40 bytes); offsets: None or step_game's
        (n, n_objects, 3) tensor.  Returns frac, a float32 (n, n_rays) tensor of fractions of max_range (+inf: nothing within
        range), or (frac, hit) when hit_out is given (True: a new int32 (n, n_rays) tensor; RAY_NO_HIT as -1): the triangle hit, an
        index into arrays()['triangles'] and triangle_objects().  frac_out / origin_out / vel_out: optional preallocated outputs
        ((n, n_rays) and (n, n_rays, 3) float32); origin and vel are the rays as World.sweep takes them."""
        L = lib()
        return _cast_rays(lambda st, lv, *rest: L.rdoom_world_cast_rays(self._h, st, *rest), states, None, dirs, max_range, offsets,
                          frac_out, hit_out, origin_out, vel_out, stream)

    def triangle_objects(self):
        """a host uint32 array with the object id of each triangle of arrays()['triangles']: 0 for the statics, the dynamic chunk's
        object id for a door's or lift's -- triangle_objects()[hit] names what a ray of cast_rays ended on"""
        return _triangle_objects(self.arrays())

    # ---- top-down maps -----------------------------------------------------------------------------------------------------
    def map_lines(self):
        """a copy of rdoom_world_map_lines: the level's line table, a MAP_LINE record per linedef with both vertices, in linedef
        order (end points in world xz, flags, special, and per side the sector's heights and its floor and ceiling object ids)"""
        return _map_lines(lambda a: lib().rdoom_world_map_lines(self._h, a))

    def draw_maps(self, states, width, height, scale, offsets=None, half_width=0.75, marker=3.0, rotate=False, show_flat=False,
                  show_hidden=False, top_down=False, out=None, stream=None, seen=None):
        """rdoom_world_draw_maps: every player's top-down map, a uint8 (n, height, width) GPU tensor of MAP_* class codes, centred
        on the player, `scale` world units per pixel.  states: the tensor a step leaves (n * 40 bytes); offsets: None or
        step_game's (n, n_objects, 3) tensor, so that a door a player opened shows open in that player's map.  half_width: half
        a line's thickness in pixels; marker: the player marker's size in pixels (0: none); rotate: the player's view direction is
        up (else map north); show_flat / show_hidden: draw lines between equal sectors / linedefs flagged never-on-the-map;
        top_down: row 0 is the top row (else the bottom row, as Batch frames).  out: an optional preallocated tensor.  Asynchronous
        on `stream`; nothing is copied to the host.  torch.from_numpy(MAP_COLORS).cuda()[maps.long()] colours the maps.
        seen: None (every line of the level: the cheat map) or reveal_lines' (n, words) tensor: player p's map then shows only
        the lines whose bit is set in row p and the linedefs flagged LINE_MAPPED (rdoom_world_draw_maps_seen)."""
        L = lib()
        return _draw_maps(lambda st, lv, *rest: L.rdoom_world_draw_maps_seen(self._h, st, *rest), states, None, width, height, scale,
                          offsets, half_width, marker, rotate, show_flat, show_hidden, top_down, out, stream, seen, self.seen_words())

    # ---- seen lines --------------------------------------------------------------------------------------------------------
    def seen_words(self):
        """the 32-bit words a row of seen bits takes: a bit per line of map_lines()"""
        a = MapLines()
        _check(lib().rdoom_world_map_lines(self._h, ctypes.byref(a)))
        return (a.n_lines + 31) // 32

    def reveal_lines(self, states, fan, max_range, offsets=None, seen=None, new_out=None, stream=None):
        """rdoom_world_reveal_lines: marks the lines every player has in view -- a fan of 2-D rays (map_fan, a float32 (n_rays, 2)
        GPU tensor shared by all players) of length max_range from the player through the line table, stopped by one-sided lines
        and by two-sided ones whose opening is empty in that player's game (offsets: None or step_game's tensor, so a shut door
        blocks until that player opens it).  seen: an int32 (n, words >= seen_words()) GPU tensor whose bits are OR-ed into, bit
        l % 32 of word l // 32 of row p for line l of map_lines(); None allocates a zeroed one.  Returns seen.  new_out: an
        optional 32-bit integer tensor of n that receives how many bits of each row this call set.  Asynchronous on `stream`."""
        L = lib()
        return _reveal_lines(lambda st, lv, *rest: L.rdoom_world_reveal_lines(self._h, st, *rest), self.seen_words(), states, None, fan,
                             max_range, offsets, seen, new_out, stream)

    # ---- things ------------------------------------------------------------------------------------------------------------
    def map_things(self):
        """a copy of rdoom_world_map_things: the level's thing table, a THING record per THINGS entry that is no marker and stands in
        a sector, in lump order (position, base height and the object that moves it, radius, sector, type, flags, category, angle)"""
        return _map_things(lambda a: lib().rdoom_world_map_things(self._h, a))

    def thing_obstacles(self):
        """rdoom_world_thing_obstacles: a bool per thing of map_things(), true where the metadata entry of its type says
        obstacle = true (pack_things packs them into a row of bits)"""
        return _thing_obstacles(lambda *out: lib().rdoom_world_thing_obstacles(self._h, *out), len(self.map_things()))

    def sense_things(self, states, things, max_range, fov=None, touch_radius=0.19, touch_below=math.inf, touch_above=math.inf, collect=(),
                     offsets=None, collected=None, visible_out=None, touched_out=None, nearest_out=None, new_out=None, stream=None,
                     n=None, n_objects=None, stride=None):
        L = lib()
        return _sense_things(lambda st, lv, *rest: L.rdoom_world_sense_things(self._h, things._h, st, *rest), states, None, things,
                             max_range, fov, touch_radius, touch_below, touch_above, collect, offsets, collected, visible_out, touched_out,
                             nearest_out, new_out, stream, n, n_objects, stride)
    sense_things.__doc__ = 'rdoom_world_sense_things: ' + _SENSE_DOC

    def draw_thing_maps(self, states, things, width, height, scale, **kw):
        """things.draw_maps(states, width, height, scale, ...): the marks of `things` (a DeviceThings of this level) on the pixels
        of draw_maps with the same width, height, scale, rotate and top_down"""
        if not isinstance(things, DeviceThings):
            raise ValueError('things must be a DeviceThings')
        return things.draw_maps(states, width, height, scale, **kw)

    def stamp_things(self, floor, ceiling, things, cell, solid=None, hidden=None, offsets=None, grow=0.0, block_below=math.inf,
                     block_above=math.inf, floor_out=None, ceiling_out=None, index_out=None, stream=None, n=None, n_objects=None, stride=None):
        L = lib()
        return _stamp_things(lambda lv, *rest: L.rdoom_world_stamp_things(self._h, getattr(things, '_h', None), *rest), None, floor, ceiling,
                             things, cell, solid, hidden, offsets, grow, block_below, block_above, floor_out, ceiling_out, index_out, stream, n,
                             n_objects, stride)
    stamp_things.__doc__ = 'rdoom_world_stamp_things: ' + _STAMP_DOC

    def cast_rays_things(self, states, things, dirs, max_range, heights=0.56, grow=0.0, categories=None, select=None, hidden=None,
                         offsets=None, frac=None, frac_out=None, thing_out=None, stream=None, n=None, n_objects=None, stride=None):
        L = lib()
        return _cast_rays_things(lambda st, lv, *rest: L.rdoom_world_cast_rays_things(self._h, getattr(things, '_h', None), st, *rest), states,
                                 None, things, dirs, max_range, heights, grow, categories, select, hidden, offsets, frac, frac_out, thing_out,
                                 stream, n, n_objects, stride)
    cast_rays_things.__doc__ = 'rdoom_world_cast_rays_things: ' + _RAY_THINGS_DOC

    # ---- sectors -----------------------------------------------------------------------------------------------------------
    def map_sectors(self):
        """a copy of rdoom_world_map_sectors: the level's sector table, a MapSectors of (sectors, leaf_sector, leaf_edges, edges)"""
        return _map_sectors(lambda a: lib().rdoom_world_map_sectors(self._h, a))

    def visited_words(self):
        """the 32-bit words a row of visited bits takes: a bit per sector of map_sectors()"""
        a = MapSectorArrays()
        _check(lib().rdoom_world_map_sectors(self._h, ctypes.byref(a)))
        return (a.n_sectors + 31) // 32

    def locate_players(self, states, offsets=None, heights_out=None, visited=None, new_out=None, out=None, stream=None):
        """rdoom_world_locate_players: the sector every player stands in, an int32 tensor of n indices into
        map_sectors().sectors, -1 (SECTOR_NONE as int32) outside every sector.  states: the tensor a step leaves; offsets: None or
        step_game's tensor.  heights_out: an optional float32 (n, 2) tensor for the sector's live floor and ceiling in that player's
        game (a lift that carried the player down shows here), +inf / -inf outside.  visited: an optional int32 (n, words >=
        visited_words()) tensor whose bit s % 32 of word s // 32 of row p is OR-ed in for the player's sector s (unpack_seen unpacks
        a row); new_out: an optional 32-bit integer tensor of n that receives 1 where this call set a new bit -- with the table's
        sector_type column on the device, (types[sector] == 9) & new counts secrets found.  out: an optional preallocated tensor.
        Asynchronous on `stream`."""
        L = lib()
        return _locate_players(lambda st, lv, *rest: L.rdoom_world_locate_players(self._h, st, *rest), self.visited_words(), states, None, offsets,
                               heights_out, visited, new_out, out, stream)

    def draw_sector_maps(self, states, width, height, scale, offsets=None, rotate=False, top_down=False, sector_out=None, floor=False,
                         ceiling=False, visited=None, stream=None):
        """rdoom_world_draw_sector_maps: every player's filled top-down map on draw_maps' grid (same width, height, scale,
        rotate, top_down: the two register pixel for pixel): per pixel the sector there.  sector_out: True or an int16 / uint16
        (n, height, width) tensor for the sector index, SECTOR_NONE16 (-1 as int16) in the void; floor / ceiling: True or a float32
        tensor for the sector's live floor / ceiling in that player's game, +inf / -inf in the void.  With none of the three asked
        for, the sector plane is drawn.  visited: None or locate_players' rows: only sectors the player has entered show.  Returns
        the planes asked for, in the order sector, floor, ceiling (one tensor, or a tuple).  Asynchronous on `stream`."""
        L = lib()
        if sector_out is None and floor is False and ceiling is False:
            sector_out = True
        return _draw_sector_maps(lambda st, lv, *rest: L.rdoom_world_draw_sector_maps(self._h, st, *rest), self.visited_words(), states, None, width,
                                 height, scale, offsets, rotate, top_down, sector_out, floor, ceiling, visited, stream)

    # ---- spawn -------------------------------------------------------------------------------------------------------------
    def spawn_table(self):
        """a copy of rdoom_world_spawn_table: the level's SpawnTable of (entries, start_pos, start_yaw)"""
        return _spawn_table(lambda a: lib().rdoom_world_spawn_table(self._h, a))

    def spawn_players(self, states, seed, mask=None, episode=None, offsets=None, margin=None, clearance=0.56, max_step=0.24,
                      flags=PLAYER_CLIP, tries_out=None, stream=None):
        """rdoom_world_spawn_players: a fresh PLAYER_STATE, written in place, for every player whose mask byte is set (mask: None --
        every player -- or n bytes / bools on the GPU): at rest at a pseudo-random point of the level's floor where a body fits, with
        a random yaw, SPAWN_RISE above the floor as the level's start is.  The point is a function of (seed, the player's index,
        episode[p]) alone -- episode: None (0) or a 32-bit integer tensor of n, read only; episode.add_(mask) before the next reset
        gives other points.  A candidate is a uniform point of the floor triangles (spawn_table()); it is taken when its sector and
        those of the four points `margin` away along x and z (None: the player config's radius) have `clearance` of headroom in the
        player's own game (offsets: None or step_game's tensor -- a door the player has not opened is no place to stand) and floors
        within `max_step` of each other.  After SPAWN_TRIES candidates the player gets the level's start instead.  tries_out: an
        optional 32-bit integer tensor of n for the winning try, 1 .. SPAWN_TRIES, 0 for the start.  mask, episode and tries_out may
        be raw device pointers.  Returns states.  One launch, asynchronous on `stream`; it can be captured into a graph."""
        L = lib()
        return _spawn_players(lambda st, lv, *rest: L.rdoom_world_spawn_players(self._h, st, *rest), states, None, seed, mask, episode,
                              offsets, margin, clearance, max_step, flags, tries_out, stream)

    # ---- explored area -----------------------------------------------------------------------------------------------------
    def area_grid(self, cell):
        """rdoom_world_area_grid: the AreaGrid of the level at cell size `cell` (world units): the cells its lines touch and one of
        margin on each side"""
        return _area_grid(lambda g: lib().rdoom_world_area_grid(self._h, ctypes.c_float(cell), g))

    def area_words(self, cell):
        """the 32-bit words a plane of the explored-area grid takes at that cell size: area_grid(cell).words"""
        return _area_words(lambda w: lib().rdoom_world_area_words(self._h, ctypes.c_float(cell), w))

    def reveal_area(self, states, fan, max_range, cell, n_steps=None, offsets=None, area=None, new_out=None, stream=None):
        """rdoom_world_reveal_area: every player's explored area, a world-anchored grid of `cell`-sized cells: reveal_lines' fan
        (fan, max_range, offsets: as there) sampled at n_steps + 1 points per ray (None: area_steps(max_range, cell), half a cell
        apart); a cell a ray crossed before it was stopped is FREE, the cell where a blocking line stopped it is WALL.  area: an
        int32 (n, 2, words >= area_words(cell)) GPU tensor whose bits are OR-ed into, [:, 0] the FREE plane and [:, 1] the WALL plane
        (unpack_area unpacks a player's); None allocates a zeroed one.  Returns area.  new_out: an optional 32-bit integer (n, 2)
        tensor that receives how many FREE and WALL bits of each row this call set -- the coverage reward.  Asynchronous on
        `stream`."""
        L = lib()
        return _reveal_area(lambda st, lv, *rest: L.rdoom_world_reveal_area(self._h, st, *rest), self.area_words(cell), states, None, fan,
                            max_range, cell, n_steps, offsets, area, new_out, stream)

    def draw_area_maps(self, states, width, height, scale, area, cell, rotate=False, top_down=False, out=None, stream=None):
        """rdoom_world_draw_area_maps: every player's explored area on draw_maps' grid (same width, height, scale, rotate,
        top_down: the two register pixel for pixel), a uint8 (n, height, width) GPU tensor of AREA_FREE | AREA_WALL bits, AREA_UNKNOWN
        where nothing was seen and outside the grid.  area, cell: reveal_area's.  out: an optional preallocated tensor.
        Asynchronous on `stream`."""
        L = lib()
        return _draw_area_maps(lambda st, lv, *rest: L.rdoom_world_draw_area_maps(self._h, st, *rest), self.area_words(cell), states, None,
                               width, height, scale, area, cell, rotate, top_down, out, stream)


    # ---- goal distance -----------------------------------------------------------------------------------------------------
    def area_plane_shape(self, cell):
        """(height, width) of draw_area_planes' planes at that cell size: the (gh, gw) of area_grid(cell)"""
        g = self.area_grid(cell)
        return g.gh, g.gw

    def draw_area_planes(self, cell, n=None, offsets=None, area=None, sector_out=None, floor=False, ceiling=False, stream=None):
        """rdoom_world_draw_area_planes: the level's sector, floor and ceiling on its explored-area grid, n rows of
        area_plane_shape(cell) cells: element [p, iz, ix] is what draw_sector_maps stores for a pixel at the centre of cell (ix, iz)
        of area_grid(cell) -- planes anchored to the level, which rd.flood_grids floods whole.  n: the rows (None: those of
        the first tensor given, else 1); offsets: None or step_game's tensor, row p the game whose doors and lifts count; area: None or reveal_area's rows --
        only cells the player has seen free (and not as a wall) show, the others are void.  sector_out / floor / ceiling: as
        draw_sector_maps takes them; a caller's tensor may be larger than area_plane_shape(cell), the padding is void.  With none of
        the three asked for, the sector plane is drawn.  Returns the planes asked for, in the order sector, floor, ceiling (one
        tensor, or a tuple).  A point sample per cell: a model of walking on the grid, which nothing ties to World.step.
        Asynchronous on `stream`; it can be captured into a graph."""
        L = lib()
        if sector_out is None and floor is False and ceiling is False:
            sector_out = True
        return _draw_area_planes(lambda lv, *rest: L.rdoom_world_draw_area_planes(self._h, *rest), self.area_plane_shape(cell),
                                 self.area_words(cell), None, cell, n, offsets, area, sector_out, floor, ceiling, stream)

    def area_cells(self, states, cell, out=None, stream=None):
        """rdoom_world_area_cells: the cell (ix, iz) of area_grid(cell) every player stands in, an int32 (n, 2) tensor, (-1, -1) for
        a player outside the grid or at a NaN.  The pair indexes draw_area_planes' planes and a flood of them as [p, iz, ix], and
        the tensor is flood_grids' seeds.  out: an optional preallocated tensor.  Asynchronous on `stream`."""
        L = lib()
        return _area_cells(lambda st, lv, *rest: L.rdoom_world_area_cells(self._h, st, *rest), states, None, cell, out, stream)

    # ---- waypoints and frontiers -------------------------------------------------------------------------------------------
    def area_frontiers(self, area, dist, cell, cell_out=None, dist_out=None, count_out=None, mask_out=None, stream=None):
        """rdoom_world_area_frontiers: the frontier of every player's explored area -- the cells `dist` reaches that have a
        4-neighbour, inside the level's grid, the player has seen neither free nor as a wall -- and the nearest of them.  area:
        reveal_area's rows; dist: the (n, height, width) distances of rd.flood_grids, usually from the players' cells over
        draw_area_planes(area=area); it may be larger than area_plane_shape(cell).  Returns the int32 (n, 2) tensor of the frontier
        cell (ix, iz) with the smallest distance (ties: the smallest iz, then ix), (-1, -1) for a row without one: descend_grids'
        starts.  dist_out, count_out, mask_out: True allocates, a tensor (dist_out, count_out: or a raw device pointer) is used
        as given -- that cell's distance (FLOOD_GRID_UNREACHED for none), the number of frontier cells, and a uint8 (n, height,
        width) mask of them; those asked for are returned after the cells, in that order.  One launch, asynchronous on `stream`; it
        can be captured into a graph."""
        L = lib()
        return _area_frontiers(lambda lv, *rest: L.rdoom_world_area_frontiers(self._h, *rest), self.area_words(cell), None, area, dist, cell,
                               cell_out, dist_out, count_out, mask_out, stream)


class WorldSetLevelInfo(ctypes.Structure):
    _fields_ = [('archive_index', ctypes.c_uint32), ('destination', ctypes.c_uint32), ('start_pos', ctypes.c_float * 3),
                ('start_yaw', ctypes.c_float), ('n_triggers', ctypes.c_uint32), ('n_objects', ctypes.c_uint32),
                ('node_depth', ctypes.c_uint32), ('world', WorldArrays), ('triggers', WorldTriggerArrays)]


class WorldSet:
    """several levels' collision worlds and trigger lists (rdoom_worldset_create), each player in one of them: the game step takes a
    player who uses an exit to the slot of the next archive level, the way the reference changes level.  Slot s holds archive
    level indices[s]; a player's slot is the level_of_pose of a DeviceLevelSet built from the same list."""

    def __init__(self, wad, indices, device=True):
        self._h = ctypes.c_void_p()
        self._wad = wad
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))
        if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise RdoomError(-1, 'level index out of range')
        idx = idx.astype(np.uint32)
        _check(lib().rdoom_worldset_create(wad._h, _ptr(idx), len(idx), 0 if device else WORLD_HOST_ONLY, ctypes.byref(self._h)))
        n_levels, n_obj = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().rdoom_worldset_info(self._h, ctypes.byref(n_levels), ctypes.byref(n_obj)))
        self.n_levels, self.n_objects = n_levels.value, n_obj.value

    def close(self):
        if self._h:
            lib().rdoom_worldset_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        _close_quietly(self)

    def _info(self, slot):
        info = WorldSetLevelInfo()
        _check(lib().rdoom_worldset_level(self._h, int(slot), ctypes.byref(info)))
        return info

    def levels(self):
        """the per-level table: a WORLDSET_LEVEL record per slot (archive index, destination slot or WORLDSET_NO_DESTINATION, start
        position and yaw, triggers, game objects, BSP depth)"""
        out = np.zeros(self.n_levels, WORLDSET_LEVEL)
        for s in range(self.n_levels):
            i = self._info(s)
            out[s] = (i.archive_index, i.destination, tuple(i.start_pos), i.start_yaw, i.n_triggers, i.n_objects, i.node_depth)
        return out

    def arrays(self, slot):
        """copies of slot `slot`'s collision arrays, in its own indices: World.arrays of the same level"""
        return _world_arrays(self._info(slot).world)

    def triggers(self, slot):
        """copies of slot `slot`'s trigger list and move effects: World.triggers of the same level"""
        return _trigger_arrays(self._info(slot).triggers)

    def start_states(self, levels, flags=PLAYER_CLIP):
        """PLAYER_STATE records at the start of each player's level, as Player::reset leaves them (pitch 1e-8, at rest)"""
        levels = np.asarray(levels, np.int64).reshape(-1)
        table = self.levels()
        return player_states(table['start_pos'][levels], table['start_yaw'][levels], flags=flags)

    def game_bytes(self):
        """rdoom_worldset_game_bytes: the bytes of one player's game (the largest level's)"""
        b = ctypes.c_uint64()
        _check(lib().rdoom_worldset_game_bytes(self._h, ctypes.byref(b)))
        return b.value

    def game_state(self, levels, stream=None):
        """(game, offsets, levels) for the players of `levels` (their slots: numpy or a GPU tensor), on the current device, reset:
        game an int32 tensor of n * game_bytes / 4 words, offsets a float32 (n, n_objects, 3) tensor, levels an int32 tensor of
        the slots (the step's and Batch.render's level_of_pose)"""
        import torch
        if isinstance(levels, torch.Tensor):
            levels = levels.to(device='cuda', dtype=torch.int32).contiguous().clone()
        else:
            levels = torch.from_numpy(np.ascontiguousarray(np.asarray(levels, np.int64).reshape(-1).astype(np.int32))).cuda()
        n = int(levels.numel())
        game = torch.zeros(n * self.game_bytes() // 4, dtype=torch.int32, device='cuda')
        offsets = torch.zeros((n, self.n_objects, 3), dtype=torch.float32, device='cuda')
        self.reset_game(game, offsets, levels, stream=stream)
        return game, offsets, levels

    def reset_game(self, game, offsets, levels, mask=None, stream=None):
        """rdoom_worldset_game_reset: a fresh game of its current level for every player (levels: a GPU tensor of slots), or for
        those whose mask entry is true (mask: n bools / bytes, numpy or a GPU tensor)"""
        n, n_obj = _game_args(self.game_bytes(), game, offsets, levels)
        _reset_masked(mask, lambda pm: lib().rdoom_worldset_game_reset(self._h, ctypes.c_void_p(game.data_ptr()),
                                                                       ctypes.c_void_p(offsets.data_ptr()), n_obj,
                                                                       ctypes.c_void_p(levels.data_ptr()), n, pm,
                                                                       ctypes.c_void_p(_stream_handle(stream))))

    def step_game(self, states, inputs, game, offsets, levels, actions=None, n_ticks=None, config=None, dt=1.0 / 60.0, stream=None):
        """rdoom_worldset_step_game: n_ticks game ticks for every player on its level, with the level change on an exit.  states /
        inputs / actions / config / dt as for World.step_game (numpy states: a stepped copy is returned; a GPU tensor is stepped in
        place, asynchronously).  game, offsets, levels: from game_state, on the GPU, read and written in place."""
        a = _GameStepArgs(states, inputs, actions, n_ticks, config)
        _, n_obj = _game_args(self.game_bytes(), game, offsets, levels, players=a.n)
        _check(lib().rdoom_worldset_step_game(self._h, ctypes.c_void_p(a.ps), ctypes.c_void_p(a.pi), ctypes.c_void_p(a.pa),
                                              ctypes.c_void_p(game.data_ptr()), ctypes.c_void_p(offsets.data_ptr()), n_obj,
                                              ctypes.c_void_p(levels.data_ptr()), a.n, int(a.n_ticks), a.cfg_ptr(), ctypes.c_float(dt),
                                              ctypes.c_void_p(_stream_handle(stream))))
        return a.result()

    def thing_obstacles(self, slot):
        """rdoom_worldset_level_thing_obstacles: World.thing_obstacles of the level in `slot`"""
        return _thing_obstacles(lambda *out: lib().rdoom_worldset_level_thing_obstacles(self._h, int(slot), *out), len(self.map_things(slot)))

    def cast_rays(self, states, levels, dirs, max_range, offsets=None, frac_out=None, hit_out=None, origin_out=None, vel_out=None,
                  stream=None):
        """rdoom_worldset_cast_rays: World.cast_rays for players spread over the set's levels (levels: game_state's tensor of
        slots).  A hit is an index into arrays(slot)['triangles'] of the player's slot; a player whose slot is not in the set gets
        +inf / RAY_NO_HIT."""
        L = lib()
        return _cast_rays(lambda st, lv, *rest: L.rdoom_worldset_cast_rays(self._h, st, lv, *rest), states, levels, dirs, max_range,
                          offsets, frac_out, hit_out, origin_out, vel_out, stream)

    def triangle_objects(self, slot):
        """World.triangle_objects of slot `slot`: the object id of each triangle of arrays(slot)['triangles']"""
        return _triangle_objects(self.arrays(slot))

    def map_lines(self, slot):
        """World.map_lines of slot `slot`"""
        return _map_lines(lambda a: lib().rdoom_worldset_level_map_lines(self._h, int(slot), a))

    def draw_maps(self, states, levels, width, height, scale, offsets=None, half_width=0.75, marker=3.0, rotate=False, show_flat=False,
                  show_hidden=False, top_down=False, out=None, stream=None, seen=None):
        """rdoom_worldset_draw_maps: World.draw_maps for players spread over the set's levels (levels: game_state's tensor of
        slots); a player whose slot is not in the set gets an all-zero map.  seen: as for World.draw_maps, rows of at least
        seen_words() words, a row's bits numbering the lines of the player's own level"""
        L = lib()
        return _draw_maps(lambda st, lv, *rest: L.rdoom_worldset_draw_maps_seen(self._h, st, lv, *rest), states, levels, width, height,
                          scale, offsets, half_width, marker, rotate, show_flat, show_hidden, top_down, out, stream, seen, self.seen_words())

    def seen_words(self):
        """the 32-bit words a row of seen bits takes in this set: its largest level's World.seen_words()"""
        return max((len(self.map_lines(s)) + 31) // 32 for s in range(self.n_levels)) if self.n_levels else 0

    def reveal_lines(self, states, levels, fan, max_range, offsets=None, seen=None, new_out=None, stream=None):
        """rdoom_worldset_reveal_lines: World.reveal_lines for players spread over the set's levels (levels: game_state's tensor of
        slots).  A row's bits number the lines of the player's own level (map_lines(slot)); a player whose slot is not in the set
        keeps its row and counts 0 new lines.  A player who changes level needs its row zeroed by the caller."""
        L = lib()
        return _reveal_lines(lambda st, lv, *rest: L.rdoom_worldset_reveal_lines(self._h, st, lv, *rest), self.seen_words(), states,
                             levels, fan, max_range, offsets, seen, new_out, stream)

    # ---- sectors -----------------------------------------------------------------------------------------------------------
    def map_things(self, slot):
        """a copy of rdoom_worldset_level_map_things: the thing table of the level in `slot`, as World.map_things gives it"""
        return _map_things(lambda a: lib().rdoom_worldset_level_map_things(self._h, int(slot), a))

    def sense_things(self, states, levels, things, max_range, fov=None, touch_radius=0.19, touch_below=math.inf, touch_above=math.inf,
                     collect=(), offsets=None, collected=None, visible_out=None, touched_out=None, nearest_out=None, new_out=None,
                     stream=None, n=None, n_objects=None, stride=None):
        L = lib()
        return _sense_things(lambda *rest: L.rdoom_worldset_sense_things(self._h, things._h, *rest), states, levels, things, max_range, fov,
                             touch_radius, touch_below, touch_above, collect, offsets, collected, visible_out, touched_out, nearest_out,
                             new_out, stream, n, n_objects, stride)
    sense_things.__doc__ = 'rdoom_worldset_sense_things (levels: a GPU tensor of one 32-bit slot per player; slot l of `things` is the ' \
                           'level in slot l): ' + _SENSE_DOC

    def draw_thing_maps(self, states, levels, things, width, height, scale, **kw):
        """things.draw_maps(states, width, height, scale, levels=levels, ...): the marks of `things` (slot l of it is the level in
        slot l) on the pixels of draw_maps with the same width, height, scale, rotate and top_down"""
        if not isinstance(things, DeviceThings):
            raise ValueError('things must be a DeviceThings')
        return things.draw_maps(states, width, height, scale, levels=levels, **kw)

    def stamp_things(self, levels, floor, ceiling, things, cell, solid=None, hidden=None, offsets=None, grow=0.0, block_below=math.inf,
                     block_above=math.inf, floor_out=None, ceiling_out=None, index_out=None, stream=None, n=None, n_objects=None, stride=None):
        L = lib()
        return _stamp_things(lambda *rest: L.rdoom_worldset_stamp_things(self._h, getattr(things, '_h', None), *rest), levels, floor, ceiling,
                             things, cell, solid, hidden, offsets, grow, block_below, block_above, floor_out, ceiling_out, index_out, stream, n,
                             n_objects, stride)
    stamp_things.__doc__ = 'rdoom_worldset_stamp_things (levels: a GPU tensor of one 32-bit slot per row; slot l of `things` and row l of ' \
        '`solid` are the level in slot l; a row whose slot is outside the set passes through): ' + _STAMP_DOC

    def cast_rays_things(self, states, levels, things, dirs, max_range, heights=0.56, grow=0.0, categories=None, select=None, hidden=None,
                         offsets=None, frac=None, frac_out=None, thing_out=None, stream=None, n=None, n_objects=None, stride=None):
        L = lib()
        return _cast_rays_things(lambda *rest: L.rdoom_worldset_cast_rays_things(self._h, getattr(things, '_h', None), *rest), states, levels,
                                 things, dirs, max_range, heights, grow, categories, select, hidden, offsets, frac, frac_out, thing_out, stream,
                                 n, n_objects, stride)
    cast_rays_things.__doc__ = 'rdoom_worldset_cast_rays_things (levels: a GPU tensor of one 32-bit slot per player; slot l of `things` and ' \
        'row l of `select` are the level in slot l; a player whose slot is outside the set keeps its fractions, index -1): ' + _RAY_THINGS_DOC

    def map_sectors(self, slot):
        """a copy of rdoom_worldset_level_map_sectors: the level's sector table, a MapSectors of (sectors, leaf_sector, leaf_edges, edges)"""
        return _map_sectors(lambda a: lib().rdoom_worldset_level_map_sectors(self._h, int(slot), a))

    def visited_words(self):
        """the 32-bit words a row of visited bits takes: a bit per sector of the set's largest level"""
        if getattr(self, '_visited_words', None) is None:  # the tables do not change: counted once, without copying them
            most = 0
            for s in range(self.n_levels):
                a = MapSectorArrays()
                _check(lib().rdoom_worldset_level_map_sectors(self._h, s, ctypes.byref(a)))
                most = max(most, a.n_sectors)
            self._visited_words = (most + 31) // 32
        return self._visited_words

    def locate_players(self, states, levels, offsets=None, heights_out=None, visited=None, new_out=None, out=None, stream=None):
        """rdoom_worldset_locate_players: World.locate_players for players spread over the set's levels (levels: game_state's
        tensor of slots).  A sector is an index into map_sectors(slot) of the player's slot, a row's bits number that level's sectors;
        a player whose slot is not in the set gets SECTOR_NONE, keeps its row and has 0 in new_out."""
        L = lib()
        return _locate_players(lambda st, lv, *rest: L.rdoom_worldset_locate_players(self._h, st, lv, *rest), self.visited_words(), states, levels, offsets,
                               heights_out, visited, new_out, out, stream)

    def draw_sector_maps(self, states, levels, width, height, scale, offsets=None, rotate=False, top_down=False, sector_out=None, floor=False,
                         ceiling=False, visited=None, stream=None):
        """rdoom_worldset_draw_sector_maps: World.draw_sector_maps for players spread over the set's levels; a player whose
        slot is not in the set gets planes of none"""
        L = lib()
        if sector_out is None and floor is False and ceiling is False:
            sector_out = True
        return _draw_sector_maps(lambda st, lv, *rest: L.rdoom_worldset_draw_sector_maps(self._h, st, lv, *rest), self.visited_words(), states, levels, width,
                                 height, scale, offsets, rotate, top_down, sector_out, floor, ceiling, visited, stream)

    # ---- spawn -------------------------------------------------------------------------------------------------------------
    def spawn_table(self, slot):
        """World.spawn_table of slot `slot`"""
        return _spawn_table(lambda a: lib().rdoom_worldset_level_spawn_table(self._h, int(slot), a))

    def spawn_players(self, states, levels, seed, mask=None, episode=None, offsets=None, margin=None, clearance=0.56, max_step=0.24,
                      flags=PLAYER_CLIP, tries_out=None, stream=None):
        """rdoom_worldset_spawn_players: World.spawn_players for players spread over the set's levels (levels: game_state's tensor of
        slots), each on the floor of its own level; a player without a valid candidate gets start_states' record of its slot.  A
        player whose slot is not in the set keeps its state and has 0 in tries_out."""
        L = lib()
        return _spawn_players(lambda st, lv, *rest: L.rdoom_worldset_spawn_players(self._h, st, lv, *rest), states, levels, seed, mask,
                              episode, offsets, margin, clearance, max_step, flags, tries_out, stream)

    # ---- explored area -----------------------------------------------------------------------------------------------------
    def area_grid(self, slot, cell):
        """rdoom_worldset_level_area_grid: the AreaGrid of slot `slot`, equal to the single world's of that level"""
        return _area_grid(lambda g: lib().rdoom_worldset_level_area_grid(self._h, int(slot), ctypes.c_float(cell), g))

    def area_words(self, cell):
        """the 32-bit words a plane of the explored-area grid takes in this set: its largest level's World.area_words(cell)"""
        return _area_words(lambda w: lib().rdoom_worldset_area_words(self._h, ctypes.c_float(cell), w))

    def reveal_area(self, states, levels, fan, max_range, cell, n_steps=None, offsets=None, area=None, new_out=None, stream=None):
        """rdoom_worldset_reveal_area: World.reveal_area for players spread over the set's levels (levels: game_state's tensor of
        slots); a row's planes are laid out for the grid of the player's own level (area_grid(slot, cell)), rows of area_words(cell)
        words.  A slot outside the set leaves its row untouched and counts 0."""
        L = lib()
        return _reveal_area(lambda st, lv, *rest: L.rdoom_worldset_reveal_area(self._h, st, lv, *rest), self.area_words(cell), states, levels,
                            fan, max_range, cell, n_steps, offsets, area, new_out, stream)

    def draw_area_maps(self, states, levels, width, height, scale, area, cell, rotate=False, top_down=False, out=None, stream=None):
        """rdoom_worldset_draw_area_maps: World.draw_area_maps for players spread over the set's levels; a slot outside the set
        gets an all-zero map"""
        L = lib()
        return _draw_area_maps(lambda st, lv, *rest: L.rdoom_worldset_draw_area_maps(self._h, st, lv, *rest), self.area_words(cell), states,
                               levels, width, height, scale, area, cell, rotate, top_down, out, stream)

    # ---- goal distance -----------------------------------------------------------------------------------------------------
    def area_plane_shape(self, cell):
        """(height, width) of draw_area_planes' planes at that cell size: the largest gh and the largest gw of the set's levels"""
        grids = [self.area_grid(s, cell) for s in range(self.n_levels)]
        return max(g.gh for g in grids), max(g.gw for g in grids)

    def draw_area_planes(self, levels, cell, n=None, offsets=None, area=None, sector_out=None, floor=False, ceiling=False, stream=None):
        """rdoom_worldset_draw_area_planes: World.draw_area_planes with row p showing the level of slot levels[p] on that level's own
        grid (area_grid(slot, cell)), every row area_plane_shape(cell) cells; outside the level's grid, and for a slot outside the
        set, the planes are void"""
        L = lib()
        if sector_out is None and floor is False and ceiling is False:
            sector_out = True
        return _draw_area_planes(lambda lv, *rest: L.rdoom_worldset_draw_area_planes(self._h, lv, *rest), self.area_plane_shape(cell),
                                 self.area_words(cell), levels, cell, n, offsets, area, sector_out, floor, ceiling, stream)

    def area_cells(self, states, levels, cell, out=None, stream=None):
        """rdoom_worldset_area_cells: World.area_cells for players spread over the set's levels, each in the grid of its own level;
        (-1, -1) for a slot outside the set"""
        L = lib()
        return _area_cells(lambda st, lv, *rest: L.rdoom_worldset_area_cells(self._h, st, lv, *rest), states, levels, cell, out, stream)

    # ---- waypoints and frontiers -------------------------------------------------------------------------------------------
    def area_frontiers(self, levels, area, dist, cell, cell_out=None, dist_out=None, count_out=None, mask_out=None, stream=None):
        """rdoom_worldset_area_frontiers: World.area_frontiers with row p on the grid of slot levels[p]; a slot outside the set has
        no frontier: (-1, -1), FLOOD_GRID_UNREACHED, 0 and a mask of zeros"""
        L = lib()
        return _area_frontiers(lambda lv, *rest: L.rdoom_worldset_area_frontiers(self._h, lv, *rest), self.area_words(cell), levels, area, dist,
                               cell, cell_out, dist_out, count_out, mask_out, stream)
