/* rdoom.h -- C ABI of the MI355X pose-batch renderer for Doom WAD levels.
 *
 * This is the drop-in boundary.  It replaces what rust-doom hands to
 * glium/OpenGL; every entry point cites the reference interface it stands in for.  Plain pointers
 * and sizes only; no C++/torch types; nothing throws across it.
 *
 *   loader + builder  (host C++, mirrors `wad` + `game::level`):   rdoom_wad_*, rdoom_built_*
 *   device renderer   (hand-written HIP, gfx950):                   rdoom_level_*, rdoom_batch_*
 *   collision world + player physics (host builder, HIP kernels):   rdoom_world_*, rdoom_player_*
 *
 * Conventions
 *   - every function returns rdoom_status (0 = ok, <0 = error); rdoom_last_error() gives a
 *     thread-local message (reference: Result<T, failchain::BoxedError<ErrorKind>>,
 *     wad/src/errors.rs:6-19; visitor callbacks are infallible, bad level data is skipped).
 *   - matrices are column-major float[16], exactly the GLSL uniforms u_modelview / u_projection
 *     (engine/src/uniforms.rs:273-280).
 *   - framebuffers are 8-bit palette indices, row 0 = bottom row (glReadPixels order), background 0.
 *     rdoom_batch_resolve_rgb / rdoom_batch_read_rgb turn them into the colours the reference's window shows: PLAYPAL 0 of
 *     the pose's level where a primitive was drawn, the GL clear colour RDOOM_CLEAR_R/G/B where none was.
 *   - a rdoom_level is immutable after create (shareable), but for rdoom_level_set_decor_things; a rdoom_batch is single-owner.
 *
 * Caller memory: alignment and extent
 *   What the library asks of a device pointer, and what it does with the memory behind it (tests/test_gpu_caller_memory_*.py hold
 *   it to this, with every pointer at the least alignment allowed here and guard bands around every array).  A device pointer
 *   needs the alignment of its element and no more: 1 for bytes (frames, maps, masks, light tables given to a render), 2 for
 *   16-bit planes and distances, 4 for float, int32_t and uint32_t data (times, offsets, fans, directions, seeds, counts, `seen`,
 *   `area`, `visited` and thing-bit words, level slots, depth and primitive planes).  A record needs the alignment of its widest member:
 *   4 for rdoom_player_state, rdoom_player_input, rdoom_pose and rdoom_thing_nearest.  The exceptions, each stated at its entry point and refused with
 *   RDOOM_BAD_ARG where less is given: a game state (rdoom_world_game_bytes) needs 16 bytes, the light tables
 *   rdoom_lightset_tables writes need 4, and rdoom_selftest_sincos' device_raw needs 8.  Rows and records are tight unless a
 *   stride is an argument, so an array of records is aligned as its first record is and no better (pose 1 of an array of
 *   136-byte rdoom_pose is 8 bytes off a 16-byte boundary).  The library writes the stated extent of every output -- the frames
 *   [first, first + count) of a resolve, n players, n rows -- and not one byte outside it, in front or behind, and it writes to
 *   no input; a record an entry point leaves alone (a player a mask excludes) keeps every byte.
 */
#ifndef RDOOM_H
#define RDOOM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t rdoom_status;
#define RDOOM_OK 0
#define RDOOM_BAD_ARG (-1)
#define RDOOM_HIP_ERROR (-2)
#define RDOOM_OOM (-3)
#define RDOOM_BAD_LEVEL (-4)
#define RDOOM_IO (-5)        /* ErrorKind::Io            (wad/src/errors.rs:9-19) */
#define RDOOM_CORRUPT_WAD (-6)  /* ErrorKind::CorruptWad */
#define RDOOM_CORRUPT_META (-7) /* ErrorKind::CorruptMetadata */

/* draw kinds, in the reference's per-object attach order (game/src/level.rs:443-496) */
#define RDOOM_KIND_FLAT 0u
#define RDOOM_KIND_WALL 1u
#define RDOOM_KIND_DECOR 2u
#define RDOOM_KIND_SKY 3u
#define RDOOM_ALL_KINDS 0xFu

/* game/src/vertex.rs:5-16  StaticVertex (repr(C), 48 bytes) */
typedef struct rdoom_static_vertex {
  float a_pos[3];
  float a_atlas_uv[2];
  float a_tile_uv[2];
  float a_tile_size[2];
  float a_scroll_rate;
  float a_row_height;
  uint8_t a_num_frames;
  uint8_t a_light;
  uint8_t _pad[2];
} rdoom_static_vertex;

/* game/src/vertex.rs:30-40  SpriteVertex (repr(C), 44 bytes) */
typedef struct rdoom_sprite_vertex {
  float a_pos[3];
  float a_atlas_uv[2];
  float a_tile_uv[2];
  float a_tile_size[2];
  float a_local_x;
  uint8_t a_num_frames;
  uint8_t a_light;
  uint8_t _pad[2];
} rdoom_sprite_vertex;

/* One `frame.draw(mesh, indices, program, ...)` of the reference (engine/src/renderer.rs:100-157):
 * a range of the index array of its vertex buffer.  Draw order == array order. */
typedef struct rdoom_draw {
  uint32_t kind;        /* RDOOM_KIND_* */
  uint32_t object_id;   /* wad::ObjectId (visitor.rs:142-143); 0 = static world */
  uint32_t first_index; /* into static_indices / decor_indices / sky_indices by kind */
  uint32_t index_count; /* multiple of 3 (TrianglesList, engine/src/meshes.rs:97-106) */
} rdoom_draw;

/* Everything Builder::build + GameShaders::load_level give glium for one level
 * (game/src/level.rs:424-496, game/src/game_shaders.rs:175-453).  Caller owns all arrays;
 * rdoom_level_create copies them to the device. */
typedef struct rdoom_level_desc {
  const rdoom_static_vertex *static_verts;
  uint32_t n_static_verts;
  const uint32_t *static_indices;
  uint32_t n_static_indices;
  const float *sky_verts; /* SkyVertex: xyz triples (vertex.rs:53-57) */
  uint32_t n_sky_verts;
  const uint32_t *sky_indices;
  uint32_t n_sky_indices;
  const rdoom_sprite_vertex *decor_verts;
  uint32_t n_decor_verts;
  const uint32_t *decor_indices;
  uint32_t n_decor_indices;
  const rdoom_draw *draws;
  uint32_t n_draws;
  const uint8_t *flat_atlas; /* wad::OpaqueImage (tex.rs:47-50), U8, REPEAT/NEAREST */
  uint32_t flat_w, flat_h;   /* powers of two (tex.rs:281-286) */
  const uint16_t *wall_atlas; /* wad::TransparentImage (tex.rs:42-45), U8U8: lo=index, hi>=0x80 transparent */
  uint32_t wall_w, wall_h;    /* powers of two (tex.rs:183-200) */
  const uint16_t *decor_atlas;
  uint32_t decor_w, decor_h;
  const uint16_t *sky_texture; /* game_shaders.rs:358-387 */
  uint32_t sky_w, sky_h;
  float sky_tiled_band_size;
  const uint8_t *playpal;  /* 768 bytes, palette 0: copied to the device for rdoom_batch_resolve_rgb (NULL: that level cannot be resolved) */
  const uint8_t *colormap; /* 32*256 bytes: rows of build_palette_texture(0,0,32) before the PLAYPAL map (tex.rs:137-166) */
} rdoom_level_desc;

/* Per-frame uniforms (engine/src/renderer.rs:78-132, game/src/game_shaders.rs:84-92). */
typedef struct rdoom_pose {
  float modelview[16];
  float projection[16];
  float time; /* u_time, seconds */
  float _pad;
} rdoom_pose;

typedef struct rdoom_level rdoom_level;
typedef struct rdoom_batch rdoom_batch;
typedef struct rdoom_wad rdoom_wad;
typedef struct rdoom_built rdoom_built;

/* per-kernel GPU times of the last rdoom_batch_render, from hipEvents on the render stream */
typedef struct rdoom_timings {
  float setup_ms, raster_ms, fragment_ms, total_ms;
  uint64_t pixels; /* n_poses * width * height of that render */
  uint64_t visible_triangles;
  uint64_t fixup_pixels; /* pixels re-resolved by the alpha-leak fixup kernel (normally a handful) */
} rdoom_timings;

/* Host-side times of the load and build phases, the ones the reference logs with one-shot Instants (wad/src/tex.rs:67-88,
 * 371-408, 479-495; game/src/level.rs:333, 384-396).  Single thread, wall clock (std::chrono::steady_clock).
 * rdoom_wad_timings fills open_ms + textures_ms (the others are 0); rdoom_built_timings fills the other four. */
typedef struct rdoom_host_timings {
  float open_ms;        /* Archive::open: header, directory, metadata (archive.rs:36-106, meta.rs:143-154) */
  float textures_ms;    /* TextureDirectory::from_archive: PLAYPAL, COLORMAP, patches, TEXTURE1/2, flats, sprites (tex.rs:53-107) */
  float level_lumps_ms; /* Level::from_archive: the eight lumps of the level (level.rs:34-81) */
  float atlases_ms;     /* build_flat_atlas + build_texture_atlas (walls, decor) + sky (game_shaders.rs:175-387) */
  float analysis_ms;    /* LevelAnalysis::new (visitor.rs:323-444) */
  float walk_ms;        /* LevelWalker::walk driving the Builder, then the index lists (level.rs:330-496) */
} rdoom_host_timings;

/* counters logged by the reference at level build (game/src/level.rs:384-422) */
typedef struct rdoom_counters {
  uint32_t num_wall_quads, num_floor_polys, num_ceil_polys, num_sky_wall_quads, num_sky_floor_polys,
      num_sky_ceil_polys, num_decors, num_static_tris, num_sky_tris, num_sprite_tris, num_objects, num_lights;
} rdoom_counters;

/* Which paths the last render of a batch took (read back from the device after it): a workload whose poses overflow their
 * tile lists is rasterised from the sorted list -- correct, and slow -- and nothing else would say so.  No reference counterpart. */
typedef struct rdoom_path_stats {
  uint32_t poses;                 /* of the last render */
  uint32_t bins_overflowed_poses; /* poses whose tile lists did not fit (or a frame with too many tiles): rasterised from the sorted list */
  uint64_t tiles;                 /* 64 x 64 tiles of those poses' frames */
  uint64_t split_tiles;           /* tiles whose list (more than 64 entries) is stored per 32 x 32 quadrant */
  uint64_t tile_entries;          /* sum of the tile lists' lengths (one per triangle and tile) */
  uint64_t quadrants;             /* 32 x 32 quadrants that lie (partly) inside the frame */
  uint64_t described_quadrants;   /* of those: all pixels show one record -- no visibility words stored or read */
  /* the fragment kernel's own census, counted only in a render under rdoom_debug_set("frag_count", 1) (zero otherwise): */
  uint64_t half_runs;             /* 8-pixel runs an edge crosses whose uniform quad was shaded with the run's neighbours (one quad listed) */
  uint64_t half_fallbacks;        /* such runs that failed a guard of the packed body, or show sky / a decoration: both quads listed */
  uint64_t listed_quads;          /* 4-pixel quads shaded by the general per-pixel body */
  /* the rasteriser's census of its fast masked body, counted only in a render under rdoom_debug_set("raster_stats", 1) (zero otherwise): */
  uint64_t masked_fast_bodies;    /* sixteen-pixel bodies that alpha-tested a masked-interior record's winners (per wave) */
  uint64_t masked_fast_pixels;    /* winners alpha-tested by those bodies */
  uint64_t masked_fast_replays;   /* lanes of those bodies that replayed their block through the general rule (tie, 1/w range, certificate) */
  uint64_t masked_general_bodies; /* general bodies that ran on a masked-interior record */
  /* shared-edge pairs (two triangles that cover a quadrant but for the edge they share), counted under "raster_stats" likewise;
   * "raster_stats" = 2 counts the default routing (settle_kernel runs), 1 sends every quadrant to the rasteriser's waves: */
  uint64_t settled_pairs;         /* quadrants settle_kernel proved a pair for: expanded by the tile's wave before its gather */
  uint64_t raster_pairs;          /* quadrants the tile's wave paired itself, after its gather (the two-entry shortcut) */
} rdoom_path_stats;

const char *rdoom_last_error(void);

/* ---- devices ------------------------------------------------------------------------------ */
rdoom_status rdoom_device_count(int32_t *out_count);
rdoom_status rdoom_set_device(int32_t device);

/* ---- device renderer: replaces engine Meshes/Uniforms uploads + Renderer::update ----------- */
/* replaces VertexBuffer::immutable / IndexBuffer::persistent / Texture2d::new uploads
 * (engine/src/meshes.rs:126-201, engine/src/uniforms.rs:146-221) */
rdoom_status rdoom_level_create(const rdoom_level_desc *desc, rdoom_level **out_level);
void rdoom_level_destroy(rdoom_level *level);
/* Several levels resident together, as ONE rdoom_level handle (rdoom_level_create = a set of one): a pose batch may then mix
 * poses of different levels in one render (rdoom_batch_render_levels) -- one launch set for, say, the 9 x 128 poses one of eight
 * GPUs renders of E1M1..E1M9 instead of nine small ones.  The reference keeps one level loaded at a time and draws it frame by
 * frame (game/src/level.rs:330-496 builds and uploads it, engine/src/renderer.rs:98-157 is the draw loop); this replaces N of
 * those uploads.  The levels must come from one IWAD: their COLORMAP tables must be identical (wad/src/tex.rs:137-166 reads the
 * archive's one COLORMAP lump).  Primitive ids, object ids and light tables stay per level.  At most 2^26 atlas texels in the set. */
rdoom_status rdoom_levelset_create(const rdoom_level_desc *const *descs, uint32_t n_levels, rdoom_level **out_level);
/* how many levels the handle holds (1 for rdoom_level_create) */
rdoom_status rdoom_level_num_levels(const rdoom_level *level, uint32_t *out);

/* allocates the device scratch for up to max_poses frames of width x height -- any size up to 16384 on a side, as the
 * reference's --resolution WxH (src/main.rs:41).  Rows of the device framebuffer are rdoom_batch_framebuffer_pitch bytes
 * apart: the width itself when it is a multiple of 4, else the next multiple of 8. */
rdoom_status rdoom_batch_create(const rdoom_level *level, uint32_t width, uint32_t height, uint32_t max_poses,
                                rdoom_batch **out_batch);
void rdoom_batch_destroy(rdoom_batch *batch);

/* replaces the frame.draw loop of Renderer::update (engine/src/renderer.rs:98-157) for n_poses
 * frames at once.  lights: n_poses tables of 256 bytes (Lights::fill_buffer_at, game/src/lights.rs:26-30)
 * spaced lights_stride bytes apart (0 = one shared table).  kinds_mask selects draw kinds.
 * Asynchronous on `stream` (a hipStream_t, may be NULL); results stay on the device.  A batch's scratch is written by every
 * render: consecutive renders of ONE batch must be ordered -- the same stream, or streams the caller orders -- and the host may
 * queue two of them before it waits for the first one's pose copy (pinned staging, two deep). */
rdoom_status rdoom_batch_render(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream);
/* same, with per-kernel hipEvent timing (synchronises the stream) */
rdoom_status rdoom_batch_render_timed(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                      uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                      rdoom_timings *out);
/* Asynchronous like rdoom_batch_render, but the four hipEvents around the kernels are kept (up to 64 renders may be
 * pending); rdoom_batch_collect_timings waits for the last of them and returns the SUMS over the pending renders
 * (pixels = all their pixels; visible_triangles / fixup_pixels of the last one) and their number.  For profiling a
 * pipelined sequence of renders without a host synchronisation in between (bench.py). */
rdoom_status rdoom_batch_render_profiled(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                         uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream);
rdoom_status rdoom_batch_collect_timings(rdoom_batch *batch, rdoom_timings *out_sums, uint32_t *out_renders);
/* Same with moving objects (doors, lifts): the reference sets u_modelview = view o model transform for the draws
 * of each object (engine/src/renderer.rs:120-132; game/src/level.rs:203-255 moves the transforms).
 * object_modelviews: n_poses x n_objects column-major matrices, entry [p][o] = the u_modelview of object o's draws
 * in frame p (object 0 = the static world; an object at rest has the pose's own modelview).
 * n_objects >= rdoom_level_num_objects. */
rdoom_status rdoom_batch_render_objects(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                        uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                        const float *object_modelviews, uint32_t n_objects);
/* rdoom_batch_render / _objects / _profiled for a batch created on a level SET: pose p is a view of level level_of_pose[p]
 * (an index into the descs of rdoom_levelset_create), lights + p * lights_stride is THAT level's light table at the pose's time.
 * object_modelviews may be NULL (no moving objects); else n_poses x n_objects matrices as for rdoom_batch_render_objects, with
 * n_objects >= rdoom_level_num_objects of the set (entries of objects the pose's level does not draw are ignored).
 * flags: RDOOM_RENDER_PROFILED keeps the per-kernel events pending as rdoom_batch_render_profiled does.
 * Replaces the frame.draw loops of Renderer::update (engine/src/renderer.rs:98-157) of SEVERAL loaded levels at once. */
#define RDOOM_RENDER_PROFILED 1u
rdoom_status rdoom_batch_render_levels(rdoom_batch *batch, const rdoom_pose *poses, const uint32_t *level_of_pose, const uint8_t *lights,
                                       uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                       const float *object_modelviews, uint32_t n_objects, uint32_t flags);
/* 1 + the largest rdoom_draw.object_id of the level (of a set: of any of its levels) */
rdoom_status rdoom_level_num_objects(const rdoom_level *level, uint32_t *out);
/* Waits for the batch's last render -- on the stream it was queued on; work of other batches on other streams is not waited
 * for -- and returns ITS status: the asynchronous rdoom_batch_render cannot report what only
 * the device finds out (today: the alpha-leak fixup list overflowing, which would leave leaked transparent texels in
 * the frames).  Consumers of rdoom_batch_framebuffer_device call this -- or any of the rdoom_batch_read_* -- before
 * trusting the frames; glFinish is the nearest reference counterpart. */
rdoom_status rdoom_batch_finish(rdoom_batch *batch);

/* waits for the batch's last render like rdoom_batch_finish, then counts (see rdoom_path_stats) */
rdoom_status rdoom_batch_path_stats(rdoom_batch *batch, rdoom_path_stats *out);

/* device pointer to the n_poses palette-index framebuffers of the last render: frame i starts at byte i * height * pitch,
 * row y of it (row 0 = the bottom row, as glReadPixels) at y * pitch, `width` bytes of pixels, then padding */
rdoom_status rdoom_batch_framebuffer_device(const rdoom_batch *batch, uint8_t **out_device_ptr);
/* bytes between consecutive rows of the device framebuffer (== width when width % 4 == 0) */
rdoom_status rdoom_batch_framebuffer_pitch(const rdoom_batch *batch, uint32_t *out_pitch);
/* glReadPixels analogue: waits for the batch's last render (on its stream -- not for the device), copies frames
 * [first, first+count) to host memory, tightly packed (width bytes per row) */
rdoom_status rdoom_batch_read_framebuffer(rdoom_batch *batch, uint32_t first, uint32_t count, uint8_t *host_out);
/* RGB frames, as the reference's window shows them: its shaders end in texture(u_palette, ...).rgb (PLAYPAL 0) and the pixels
 * no primitive covers keep the clear colour (0.06, 0.07, 0.09) of window.rs:40-44, i.e. (15, 18, 23) as 8-bit UNORM.  A pixel is
 * clear exactly where rdoom_batch_read_primitive_ids would report 0xFFFFFFFF.  format = RDOOM_RGB8 or RDOOM_RGBA8, optionally
 * | RDOOM_RGB_TOP_DOWN.  Rows are tight (width * bytes per pixel, no padding); row 0 is the bottom row (glReadPixels order)
 * unless RDOOM_RGB_TOP_DOWN.  RGBA8: alpha 255 where a primitive was drawn (the shaders write vec3: opaque), 0 where the clear
 * colour shows (its alpha, window.rs:42).  Poses of a level whose desc had no playpal cannot be resolved (RDOOM_BAD_ARG). */
#define RDOOM_RGB8 3u          /* 3 bytes per pixel */
#define RDOOM_RGBA8 4u         /* 4 bytes per pixel, alpha 255 drawn / 0 clear */
#define RDOOM_RGB_TOP_DOWN 0x100u /* row 0 = the top row (default: the bottom row, glReadPixels order) */
#define RDOOM_CLEAR_R 15u      /* window.rs:40-44 clear colour as 8-bit UNORM */
#define RDOOM_CLEAR_G 18u
#define RDOOM_CLEAR_B 23u
/* Asynchronous, on `stream` (a hipStream_t, may be NULL): waits for the batch's last render, writes frames [first, first+count)
 * of it to device_out -- count * height * width * bytes-per-pixel bytes of device memory on the batch's device -- and
 * rdoom_batch_finish / the rdoom_batch_read_* then wait for it too.  The next render of this batch overwrites what the resolve
 * reads: order it after the resolve (the same stream, or after rdoom_batch_finish).  Errors the device finds in the render are
 * reported by rdoom_batch_finish. */
rdoom_status rdoom_batch_resolve_rgb(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t format, void *device_out,
                                     void *stream);
/* Synchronous: the same frames copied to host memory (count * height * width * bytes-per-pixel bytes), resolved in chunks of
 * frames through a bounded staging buffer the batch allocates on first use; reports the render's device errors like
 * rdoom_batch_read_framebuffer. */
rdoom_status rdoom_batch_read_rgb(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t format, uint8_t *host_out);
/* Per-pixel planes of the batch's LAST render, resolved on demand for frames [first, first+count) from what the render leaves
 * on the device (quadrant table, visibility words, fixup list, the poses' triangle records): nothing is switched on before the
 * render and a render costs the same whether planes are asked for or not.  plane = one RDOOM_PLANE_*, optionally
 * | RDOOM_RGB_TOP_DOWN.  Rows are tight (width elements, no padding); row 0 is the bottom row unless RDOOM_RGB_TOP_DOWN.
 *
 *   plane                  element   where a flat / wall / decor fragment won             sky pixel                 nothing drawn
 *   RDOOM_PLANE_DEPTH      float32   v_dist of the winning fragment (static.vert:42,      +inf (sky.frag has no     +inf
 *                                    sprite.vert:44): the clip-space w, i.e. the linear   v_dist)
 *                                    view-space depth in the reference's world units (the
 *                                    units of rdoom_player_state.pos), evaluated as
 *                                    1.0f / fmaf(wp[0], x + 0.5f, fmaf(wp[1], y + 0.5f, wp[2]))
 *                                    with the record's 1/w plane wp, IEEE division, no
 *                                    contraction -- the bits the fragment stage computes
 *   RDOOM_PLANE_LABEL      uint16    kind | object_id << 4  (kind: RDOOM_KIND_*, 0..3;   RDOOM_KIND_SKY |          RDOOM_LABEL_NONE
 *                                    object_id: rdoom_draw.object_id, 12 bits, 0 = the    object_id << 4
 *                                    static level)
 *   RDOOM_PLANE_PRIMITIVE  uint32    the winning primitive id (triangle index in the draw  the same                 0xFFFFFFFF
 *                                    order of the pose's level), exactly what
 *                                    rdoom_batch_read_primitive_ids reports
 *
 * No palette is needed: a level created without a playpal resolves, also after rdoom_batch_render_players. */
#define RDOOM_PLANE_DEPTH 1u
#define RDOOM_PLANE_LABEL 2u
#define RDOOM_PLANE_PRIMITIVE 3u
#define RDOOM_LABEL_NONE 0xFFFFu /* label of a pixel nothing was drawn to */
/* Asynchronous, on `stream` (a hipStream_t, may be NULL), ordered like rdoom_batch_resolve_rgb: waits for the batch's last render,
 * writes count * height * width elements to device_out -- device memory on the batch's device, aligned to the element -- and
 * rdoom_batch_finish / the rdoom_batch_read_* then wait for it too.  Order the batch's next render after it. */
rdoom_status rdoom_batch_resolve_plane(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t plane, void *device_out,
                                       void *stream);
/* Synchronous: the same plane copied to host memory, resolved in chunks of frames through the batch's bounded staging buffer;
 * reports the render's device errors like rdoom_batch_read_framebuffer. */
rdoom_status rdoom_batch_read_plane(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t plane, void *host_out);
/* Reduced-size observations of the batch's LAST render: frames [first, first+count) reduced by fx x fy on the device before
 * anything is stored -- what a policy network takes (80 x 50, 160 x 100, often grey, often channel-first, with a depth channel of
 * the same size) from a render that is large enough not to alias.  Nothing is switched on before the render.
 *
 *   fx, fy   each one of 1, 2, 4, 8, independently (so a cell never straddles a 32 x 32 quadrant); anything else: RDOOM_BAD_ARG
 *   size     ow = width / fx, oh = height / fy (integer division; ow == 0 or oh == 0: RDOOM_BAD_ARG).  Cell (cx, cy) covers
 *            framebuffer columns [cx*fx, cx*fx + fx) and rows [cy*fy, cy*fy + fy), row 0 the bottom row as stored; columns >= ow*fx
 *            and rows >= oh*fy belong to no cell.  RDOOM_RGB_TOP_DOWN or-ed into `format` reverses the order of the OUTPUT rows
 *            only: it does not move the cells.
 *   inputs   per pixel, the colour is exactly rdoom_batch_resolve_rgb's RGB8 (PLAYPAL 0 of the pose's level where drawn,
 *            RDOOM_CLEAR_R/G/B where not) and the depth exactly the RDOOM_PLANE_DEPTH element (+inf for sky and where nothing
 *            was drawn).
 *
 * With n = fx*fy and S_c the sum of channel c over the cell, all in unsigned integers:
 *
 *   format                  output                                   element
 *   RDOOM_OBS_RGB8          count x oh x ow x 3 uint8, interleaved   (2*S_c + n) / (2*n): the exact mean, a half rounds up
 *   RDOOM_OBS_RGB8_PLANAR   count x 3 x oh x ow uint8                the same bytes, channel-first
 *   RDOOM_OBS_GRAY8         count x oh x ow uint8                    (77*S_r + 150*S_g + 29*S_b + 128*n) / (256*n)
 *   RDOOM_OBS_DEPTH_MIN     count x oh x ow float32                  the smallest depth of the cell: m = +inf, then
 *                                                                    m = d < m ? d : m over the cell (a NaN is never taken)
 *
 * Rows are tight; an ow that is not a multiple of 4 is fine.  The colour formats need the levels' playpals, like
 * rdoom_batch_resolve_rgb; RDOOM_OBS_DEPTH_MIN needs none.  An unknown format, or any other bit set in it, is RDOOM_BAD_ARG.
 * At fx = fy = 1 the RGB8 bytes equal rdoom_batch_resolve_rgb's and the depth bits rdoom_batch_resolve_plane(RDOOM_PLANE_DEPTH)'s. */
#define RDOOM_OBS_RGB8 1u
#define RDOOM_OBS_RGB8_PLANAR 2u
#define RDOOM_OBS_GRAY8 3u
#define RDOOM_OBS_DEPTH_MIN 4u
/* Asynchronous, on `stream` (a hipStream_t, may be NULL), ordered exactly like rdoom_batch_resolve_rgb / rdoom_batch_resolve_plane:
 * waits for the batch's last render, writes the table's output to device_out -- device memory on the batch's device, aligned to
 * the element -- and rdoom_batch_finish / the rdoom_batch_read_* then wait for it too.  Order the batch's next render after it. */
rdoom_status rdoom_batch_resolve_observation(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t format,
                                             uint32_t fx, uint32_t fy, void *device_out, void *stream);
/* Synchronous: the same observations copied to host memory, resolved in chunks of frames through the batch's bounded staging
 * buffer; reports the render's device errors like rdoom_batch_read_framebuffer. */
rdoom_status rdoom_batch_read_observation(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t format,
                                          uint32_t fx, uint32_t fy, void *host_out);
/* Debug / test facility: capture the winning primitive id per pixel (triangle index in the draw order of the pose's level,
 * 0xFFFFFFFF = none) on the following renders, then read it back.  No GL counterpart.  It selects a slower instantiation of the
 * rasteriser and keeps 4 bytes per pixel for the whole batch: RDOOM_PLANE_PRIMITIVE above gives the same ids after any render,
 * on the device or the host, without either. */
rdoom_status rdoom_batch_enable_primitive_ids(rdoom_batch *batch);
rdoom_status rdoom_batch_read_primitive_ids(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t *host_out);

/* On-device verification of the exact short forms the fragment kernel uses instead of IEEE division
 * (rust-doom_amd/csrc/hip/fastmath.hpp).  No reference counterpart: it certifies that the kernels evaluate
 * static.frag:18-28's divisions and mod() to the same bits as the plain operations.
 * out_counts: [0] 1/x mismatches, [1] 0.9/x mismatches, [2] inputs swept, [3] mod-certificate violations,
 * [4] mod samples, [5] samples certified, [6] samples where the short form's floor differs (all rejected),
 * [7] packed-vs-scalar mismatches.  [0], [1], [3], [7] must be 0. */
rdoom_status rdoom_selftest_fastmath(uint64_t out_counts[8]);

/* On-device evaluation of the project's sine and cosine (rust-doom_amd/csrc/hip/sincos_rd.hpp, the one every world-side kernel
 * takes its yaw's from) for ALL 2^32 binary32 arguments, for a bit-for-bit comparison with a host restatement
 * (tests/sincos_sweep.c, tests/test_gpu_sincos.py).  A binade is b = bits >> 23, sign and exponent together: 512 of them, 2^23
 * arguments each.  out_sums[b] is the sum modulo 2^64, over the binade's arguments, of term(bits of x, bits of s, bits of c)
 * with (s, c) = sincos(x), a NaN result replaced by the one pattern 0x7FC00000, and, in uint64_t arithmetic,
 *   term(x, s, c):  h = x * 0x9E3779B97F4A7C15;  h ^= (s << 32) | c;  h ^= h >> 32;  h *= 0xD6E8FEB86659FD93;  h ^= h >> 32;
 *                   h *= 0xD6E8FEB86659FD93;  h ^= h >> 32;  return h
 * device_raw, if not NULL: device memory on the current device, aligned to 8 bytes, for 2^24 floats (64 MiB), which receives the
 * results of binade raw_binade (< 512) as they are, NaNs included: (s, c) of the argument (raw_binade << 23) | m at floats 2m and
 * 2m + 1.  Runs on the null stream and returns when the results are there; allocates 4 KiB of device memory for the call. */
rdoom_status rdoom_selftest_sincos(uint64_t out_sums[512], uint32_t raw_binade, float *device_raw);

/* Test hooks (no reference counterpart; the library never reads the environment).  Each option selects a differently
 * shaped but EQUIVALENT path through the kernels -- the image must not change -- so that the rarely taken ones can be
 * forced (tests/test_gpu_debug_paths.py).  Process-wide; read when a batch is created ("vis32", "entry_cap") or
 * rendered (the rest).  Names: no_bins, entry_cap, vis32, leak_mod, frag_nq, frag_bw, frag_chunk, bin_threads,
 * no_cover, no_pair, no_settle, no_settle_pairs, settle_max, raster_stats, no_qtab, keep_vis, qpath, no_split, no_half_runs, frag_count, no_masked_fast
 * (rust-doom_amd/csrc/common.hpp: DebugOptions); "reset" restores the defaults. */
rdoom_status rdoom_debug_set(const char *name, int32_t value);

/* ---- loader + builder: the `wad` crate and `game::level` static-geometry builder ----------- */
/* Archive::open (wad/src/archive.rs:36-60) + TextureDirectory::from_archive (wad/src/tex.rs:53-107) */
rdoom_status rdoom_wad_open(const char *wad_path, const char *metadata_path, rdoom_wad **out_wad);
void rdoom_wad_close(rdoom_wad *wad);
rdoom_status rdoom_wad_timings(const rdoom_wad *wad, rdoom_host_timings *out);    /* how long rdoom_wad_open's phases took */
rdoom_status rdoom_wad_num_levels(const rdoom_wad *wad, uint32_t *out);           /* Archive::num_levels */
rdoom_status rdoom_wad_level_name(const rdoom_wad *wad, uint32_t index, char out_name[9]); /* WadSystem::level_name */
/* WadName::from_bytes (wad/src/name.rs:41-75); out = 8 bytes */
rdoom_status rdoom_wad_name_from_bytes(const uint8_t *bytes, uint32_t len, uint8_t out[8]);

/* ---- the reference's own plug-in point: trait wad::LevelVisitor (wad/src/visitor.rs:65-127) -------------------
 * Thirteen callbacks, every one optional (NULL = the trait's default: do nothing).  Payloads mirror the structs of
 * visitor.rs:24-63 and are BORROWED for the duration of the call (the walker reuses its scratch per sub-sector,
 * visitor.rs:646-651): copy out what you keep.  Callbacks are infallible, as in the reference, and must not unwind
 * or longjmp across the library.  `user` is handed back untouched. */
typedef struct rdoom_light_info {   /* wad/src/light.rs:8-25 LightInfo { level, effect: Option<LightEffect> } */
  float level;
  int32_t has_effect;               /* 0: effect is None, the rest is unset */
  int32_t effect_kind;              /* 0 Glow, 1 Random, 2 Alternate (LightEffectKind) */
  float alt_level, speed, duration, sync;
} rdoom_light_info;
typedef struct rdoom_static_quad {  /* visitor.rs:24-34 */
  uint32_t object_id;
  float v1[2], v2[2];
  float tex_start[2], tex_end[2], height_range[2];
  const rdoom_light_info *light_info;
  float scroll;
  int32_t has_tex_name;             /* Option<WadName> */
  uint8_t tex_name[8];
  int32_t blocker;
} rdoom_static_quad;
typedef struct rdoom_static_poly {  /* visitor.rs:36-42 */
  uint32_t object_id;
  const float *vertices;            /* n_vertices x (x, z) */
  uint32_t n_vertices;
  float height;
  const rdoom_light_info *light_info;
  uint8_t tex_name[8];
} rdoom_static_poly;
typedef struct rdoom_sky_quad {     /* visitor.rs:44-48 */
  uint32_t object_id;
  float v1[2], v2[2], height_range[2];
} rdoom_sky_quad;
typedef struct rdoom_sky_poly {     /* visitor.rs:50-54 */
  uint32_t object_id;
  const float *vertices;
  uint32_t n_vertices;
  float height;
} rdoom_sky_poly;
typedef struct rdoom_decor {        /* visitor.rs:56-63 */
  uint32_t object_id;
  float low[3], high[3], half_width;
  const rdoom_light_info *light_info;
  uint8_t tex_name[8];
} rdoom_decor;
typedef struct rdoom_line2f {       /* math/src/line.rs:5-10 Line2 { origin, displace, length } */
  float origin[2], displace[2], length;
} rdoom_line2f;
enum { RDOOM_MARKER_START_POS = 0, RDOOM_MARKER_TELEPORT_START = 1, RDOOM_MARKER_TELEPORT_END = 2 };  /* visitor.rs:129-133 */
enum { RDOOM_BRANCH_POSITIVE = 0, RDOOM_BRANCH_NEGATIVE = 1 };                                        /* visitor.rs:135-139 */
typedef struct rdoom_visitor_vtbl { /* trait LevelVisitor, method for method (visitor.rs:65-116) */
  void (*visit_wall_quad)(void *user, const rdoom_static_quad *quad);
  void (*visit_floor_poly)(void *user, const rdoom_static_poly *poly);
  void (*visit_ceil_poly)(void *user, const rdoom_static_poly *poly);
  void (*visit_floor_sky_poly)(void *user, const rdoom_sky_poly *poly);
  void (*visit_ceil_sky_poly)(void *user, const rdoom_sky_poly *poly);
  void (*visit_sky_quad)(void *user, const rdoom_sky_quad *quad);
  void (*visit_marker)(void *user, const float pos[3], float yaw_rad, int32_t marker, uint32_t player);
  void (*visit_decor)(void *user, const rdoom_decor *decor);
  void (*visit_bsp_root)(void *user, const rdoom_line2f *line);
  void (*visit_bsp_node)(void *user, const rdoom_line2f *line, int32_t branch);
  void (*visit_bsp_leaf)(void *user, int32_t branch);
  void (*visit_bsp_leaf_end)(void *user);
  void (*visit_bsp_node_end)(void *user);
} rdoom_visitor_vtbl;
/* WadSystem::walk<V: LevelVisitor>(&self, &mut V) (game/src/wad_system.rs:47-56): LevelWalker::walk over one level with
 * the caller's visitor only -- the way game::world::WorldBuilder is driven (game/src/world.rs:306). */
rdoom_status rdoom_wad_walk(const rdoom_wad *wad, uint32_t level_index, const rdoom_visitor_vtbl *visitor, void *user);

/* WadSystem::create's level half + GameShaders::load_level + Builder::build
 * (game/src/wad_system.rs:72-113, game/src/game_shaders.rs:175-387, game/src/level.rs:330-496).
 * use_gpu_tessellation != 0 runs the SSECTOR->polygon / SEG->quad kernels on the current device
 * (results are identical to the host walk). */
rdoom_status rdoom_wad_build_level(const rdoom_wad *wad, uint32_t level_index, int32_t use_gpu_tessellation,
                                   rdoom_built **out_built);
/* The same with a second visitor chained AFTER the Builder -- `builder.chain(&mut world_builder)` of
 * game/src/level.rs:378-382 (VisitorChain, visitor.rs:1261-1331): each event reaches the Builder, then `visitor`. */
rdoom_status rdoom_wad_build_level_chained(const rdoom_wad *wad, uint32_t level_index, int32_t use_gpu_tessellation,
                                           const rdoom_visitor_vtbl *visitor, void *user, rdoom_built **out_built);
void rdoom_built_destroy(rdoom_built *built);
/* borrowed pointers into `built`, valid until rdoom_built_destroy */
rdoom_status rdoom_built_desc(const rdoom_built *built, rdoom_level_desc *out_desc);
rdoom_status rdoom_built_counters(const rdoom_built *built, rdoom_counters *out);
rdoom_status rdoom_built_timings(const rdoom_built *built, rdoom_host_timings *out); /* how long the build's phases took */
/* Lights::fill_buffer_at (game/src/lights.rs:26-30) */
rdoom_status rdoom_built_lights_at(const rdoom_built *built, float time, uint8_t out_lights[256]);
/* The level's Lights list itself (game/src/lights.rs:3-24), in push order: entry i is the info of light index i (a_light of the
 * vertices), the list rdoom_built_lights_at iterates over.  Borrowed, valid until rdoom_built_destroy; *out_n <= 255.  An entry
 * with has_effect == 0 has its effect fields zero.  Feeds rdoom_lightset_create. */
rdoom_status rdoom_built_light_infos(const rdoom_built *built, const rdoom_light_info **out, uint32_t *out_n);
/* Builder::visit_marker start pose (game/src/level.rs:757-762) */
rdoom_status rdoom_built_start(const rdoom_built *built, float out_pos[3], float *out_yaw);
/* bounds of the sub-sector floor polygons, for pose generators: n polygons, centroid xz + floor y */
rdoom_status rdoom_built_floor_centroids(const rdoom_built *built, const float **out_xyz, uint32_t *out_n);
/* Which thing every decor quad is: *out_n == n_decor_verts / 4 entries, entry q for the quad of decor vertices 4q .. 4q + 3: the
 * thing's index in the level's thing table (rdoom_world_map_things of the same level; "things" below).  Strictly increasing: the
 * build visits the things in table order and a thing emits at most one quad (none without metadata or sprite).  Borrowed, valid
 * until rdoom_built_destroy.  Feeds rdoom_level_set_decor_things.  No reference counterpart. */
rdoom_status rdoom_built_decor_things(const rdoom_built *built, const uint32_t **out, uint32_t *out_n);

/* Camera of the reference: view = inverse(T(eye) * Ry(yaw) * Rx(pitch)),
 * projection = perspective(65 deg, (w/h)*1.2, 0.01, 100) (game/src/player.rs:84-89, 325-345;
 * engine/src/projections.rs:93-101; engine/src/renderer.rs:78-87). */
rdoom_status rdoom_pose_look(const float eye[3], float yaw, float pitch, uint32_t width, uint32_t height, float time,
                             rdoom_pose *out_pose);
/* The same camera in the REFERENCE'S OWN ARITHMETIC, binary32 throughout: the player entity's Decomposed { rot =
 * Quaternion::from(Euler { x: pitch, y: yaw, z: 0 }), disp = pos } (game/src/player.rs:124-131) concatenated with the camera
 * child at (0, 0.12, 0) (player.rs:325-335, engine/src/transforms.rs:121), inverted and turned into a matrix as
 * Renderer::update does (engine/src/renderer.rs:78-87), cgmath 0.18.0's published formulas restated; the projection from
 * f = cot(fovy / 2) in binary32.  `pos` is the PLAYER's position (level.start_pos()), not the eye: the camera height is added
 * here.  rdoom_pose_look (double precision, rounded once) stays the helper of the seeded sweeps; the two agree to a few
 * units in the last place (tests/test_pose_helpers.py). */
rdoom_status rdoom_pose_from_player(const float pos[3], float yaw, float pitch, uint32_t width, uint32_t height, float time,
                                    rdoom_pose *out);

/* ---- collision world + player physics: game::world::World and game::player::Player --------------------------------
 * The reference's camera is the head of a player that walks, falls, jumps and slides along walls: each 60 Hz tick
 * Player::update (game/src/player.rs:359-408) sweeps spheres through the collision volume World (game/src/world.rs), built
 * by WorldBuilder from the same level walk as the renderer's Builder (game/src/level.rs:378-382).  Here a rdoom_world holds
 * that volume on the host and the current device; N players step K ticks in ONE launch.
 * Arithmetic: binary32, no contraction, IEEE division and sqrt; the sine / cosine of yaw and pitch come from a project-owned
 * binary32 sincos (csrc/hip/sincos_rd.hpp), not the device libm, so a step is reproducible bit for bit on any IEEE host that
 * takes the sincos's quadrant as the device's float-to-int conversion does (saturating; tests/sincos_restatement.h).
 * The sincos's domain (rdoom_selftest_sincos; tests/test_sincos_host.py, tests/test_gpu_sincos.py): its bits are reproducible
 * for every finite argument; its results are within 2 of the project's ulp measure for |x| < 512 (measured over every such
 * argument: 1.562); from there the error grows -- 2.95 below 1024, 5.68 below 2048, 12.3 below 4096, 25.2 below 8192, the
 * record is tests/golden/sincos_error.json -- and beyond 8192 no accuracy is promised.  The step computes yaw -= look.x and
 * never wraps it: a caller that lets yaw grow stays inside this statement, with the accuracy of the yaw it has reached. */
typedef struct rdoom_world rdoom_world;
typedef struct rdoom_world_node {      /* world.rs:139-143 Node: partition Line2f + Child::pack'ed children (world.rs:152-163): */
  float origin[2], displace[2], length; /* > 0 a node index, <= 0 minus a chunk index; never linked = 0 = Leaf(0), as the reference */
  int32_t positive, negative;
} rdoom_world_node;
typedef struct rdoom_world_chunk { uint32_t tri_start, tri_end; } rdoom_world_chunk;          /* world.rs:124-128 */
typedef struct rdoom_world_triangle { uint32_t v1, v2, v3, normal; } rdoom_world_triangle;    /* world.rs:135-141: vertex indices */
typedef struct rdoom_world_dynamic { uint32_t object_id, tri_start, tri_end; } rdoom_world_dynamic; /* DynamicChunk, world.rs:212-237 */
/* borrowed pointers into a rdoom_world (valid until rdoom_world_destroy) */
typedef struct rdoom_world_arrays {
  const rdoom_world_node *nodes;
  uint32_t n_nodes;
  const rdoom_world_chunk *chunks;
  uint32_t n_chunks;
  const rdoom_world_triangle *triangles; /* the static world's n_static_triangles, then each dynamic chunk's (WorldBuilder::build) */
  uint32_t n_triangles, n_static_triangles;
  const float *verts;                    /* xyz triples */
  uint32_t n_verts;
  const rdoom_world_dynamic *dynamics;   /* by ascending object_id; only objects that have collision triangles */
  uint32_t n_dynamics;
  uint32_t n_objects;                    /* 1 + the largest object_id of a dynamic chunk (1 when there is none) */
  uint32_t node_depth;                   /* nodes on the longest root-to-node path (sizes the sweep's node stack) */
} rdoom_world_arrays;

/* Player { velocity, fly, clip, last_height_diff } + the player entity's transform (player.rs:107-113, 118-133), 40 bytes.
 * Orientation is (yaw, pitch), as rdoom_pose_from_player takes it.  flags: RDOOM_PLAYER_FLY / RDOOM_PLAYER_CLIP are the
 * caller's (the reference's defaults: fly off, clip on, player.rs:347-353); RDOOM_PLAYER_DIVERGED is set by a step in which
 * the collision loop ran 100 sweeps without settling -- the reference's error!("Failed to compute collisions.")
 * (player.rs:162-165) -- and is never cleared by the library.
 * yaw is not wrapped, by the step or by anything else: every kernel takes its sine and cosine as they are, reproducible for every
 * finite yaw, within 2 of the ulp measure for |yaw| < 512 and degrading beyond (the domain statement above, at the step). */
#define RDOOM_PLAYER_FLY 1u
#define RDOOM_PLAYER_CLIP 2u
#define RDOOM_PLAYER_DIVERGED 0x100u
typedef struct rdoom_player_state {
  float pos[3], vel[3], yaw, pitch, last_height_diff;
  uint32_t flags;
} rdoom_player_state;
/* One tick's input: what Input::poll_analog2d(movement / look) and poll_gesture(jump) return (player.rs:190-192). */
typedef struct rdoom_player_input {
  float movement[2], look[2];
  uint32_t jump; /* != 0: held */
} rdoom_player_input;
/* player.rs:56-92 Config, the physics half.  The domain the tests hold the steps to (tests/step_cases.py, every field moved by
 * a quarter or more from its default, one at a time and all at once): every field finite; radius, height and spring_const_p > 0;
 * the others >= 0.  Values outside it are not checked by the library: a step takes them as they are and computes what the
 * reference's arithmetic gives.  (friction < move_force lets a walker start at all; a feet sphere at rest above the floor needs
 * height > 17 / spring_const_p, and a head sphere above it 0.2 + height - 17 / spring_const_p > radius.) */
typedef struct rdoom_player_config {
  float move_force, spring_const_p, spring_const_d, radius, height, air_drag, ground_drag, friction;
} rdoom_player_config;

/* WorldBuilder::new, LevelWalker::walk, WorldBuilder::build (world.rs:211-409, level.rs:378-382), then the arrays are copied to
 * the current device.  flags: RDOOM_WORLD_HOST_ONLY builds the host arrays only (no device is touched; rdoom_world_sweep /
 * rdoom_world_step_players then return RDOOM_BAD_ARG).  A level without BSP nodes is RDOOM_BAD_LEVEL, and so is a tree deeper
 * than RDOOM_WORLD_MAX_DEPTH nodes (the sweep's node stack lives in LDS, sized by the tree's depth). */
#define RDOOM_WORLD_HOST_ONLY 1u
#define RDOOM_WORLD_MAX_DEPTH 255u
rdoom_status rdoom_world_create(const rdoom_wad *wad, uint32_t level_index, uint32_t flags, rdoom_world **out_world);
void rdoom_world_destroy(rdoom_world *world);
rdoom_status rdoom_world_host_arrays(const rdoom_world *world, rdoom_world_arrays *out);
/* World::sweep_sphere (world.rs:40-82, math/src/sphere.rs:16-183) for n queries at once, asynchronous on `stream` (a
 * hipStream_t, may be NULL); every pointer is device memory.  d_spheres: n x (cx, cy, cz, radius); d_vels: n x (x, y, z);
 * d_out: n x (time, nx, ny, nz), time = +inf where the reference returns None.  d_object_offsets: NULL (every object at rest),
 * or n x n_objects x (x, y, z): query q sees object o displaced by entry [q][o] (entry 0, the static world, is ignored) -- the
 * `disp` that game/src/level.rs:203-255 moves; n_objects >= the world's.  Captured into a graph, it allocates and waits on nothing. */
rdoom_status rdoom_world_sweep(const rdoom_world *world, const float *d_spheres, const float *d_vels, uint32_t n,
                               const float *d_object_offsets, uint32_t n_objects, void *stream, float *d_out);
/* n_ticks ticks of Player::update (player.rs:359-408: force() with the feet probe and move_force, then clip() or noclip(),
 * then velocity += force * dt) for n_players players in one launch, asynchronous on `stream`.  d_states (device) is read and
 * written in place; d_inputs (device): n_ticks x n_players, entry [t * n_players + p] is player p's input at tick t.
 * cfg: NULL = rdoom_player_config_default.  dt: the tick (0 or -0.0 = 1/60, engine Tick's timestep); a negative, infinite or
 * NaN dt is RDOOM_BAD_ARG and queues nothing.  The tests cover cfg in the domain stated at rdoom_player_config and dt in
 * [1/120, 1/30] or 0; values outside are not checked by the library.  (The spring of player.rs:302-305 makes the height's excess
 * over the rest height a recurrence with the characteristic polynomial z^3 - 2 z^2 + (1 + p dt^2 + d dt) z - d dt, p and d
 * the spring constants: where its largest root passes 1 -- the default config at dt = 1/30 -- a standing player's height no
 * longer settles, in the reference as here.)  d_object_offsets: as for rdoom_world_sweep, per player (constant over the
 * ticks).  The look update is yaw -= look.x, pitch = clamp(pitch - look.y, +-(pi/2 - 1e-2)) -- in exact arithmetic the
 * reference's quaternion composition (player.rs:194-205).  Triggers, teleports and level changes are not simulated. */
rdoom_status rdoom_world_step_players(const rdoom_world *world, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                      uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg, float dt,
                                      const float *d_object_offsets, uint32_t n_objects, void *stream);
/* Config::default (player.rs:73-92) */
rdoom_status rdoom_player_config_default(rdoom_player_config *out);

/* ---- doors, lifts and exits: Level::poll_triggers and the move effects of Level::update --------------------------------
 * The level reacting to the player (game/src/level.rs:77-167, 184-267), N independent games at once.  Every linedef with a
 * special and both vertices is a trigger, in linedef order (wad/src/visitor.rs:341-500; none at all in a level without a
 * tagged sector).  A trigger that fires copies its move effects into the player's active set, one per object (a later one
 * replaces an earlier one on the same object); an active effect moves its object's height offset towards its first offset
 * at `speed`, waits `wait` seconds, then moves on to its second offset if it has one, and ends.  One game tick for one
 * player, in the reference's system order: Player::update's physics against the offsets as they stood at the start of the
 * tick, then every active effect advances by dt in ascending object id, then the triggers are polled from the new position
 * (walked line = -(velocity * dt) in the xz plane; a push / shoot action looks 0.5 / 100 along the camera's view).  An
 * only_once trigger that fired is swap_remove'd from the player's list after the poll, so each game keeps its own order.
 * Teleports, monsters, damage and light effects are not simulated; changing level on an exit is the world sets' (below). */
#define RDOOM_PLAYER_EXITED 0x200u /* sticky: an exit trigger fired for this player (set by the game steps only) */
#define RDOOM_TRIGGER_WALK_OVER 0u /* rdoom_trigger.trigger_type (meta.rs TriggerType) */
#define RDOOM_TRIGGER_PUSH 1u
#define RDOOM_TRIGGER_SWITCH 2u
#define RDOOM_TRIGGER_GUN 3u
#define RDOOM_TRIGGER_ANY 4u
#define RDOOM_TRIGGER_ONLY_ONCE 1u     /* rdoom_trigger.flags */
#define RDOOM_TRIGGER_EXIT 2u
#define RDOOM_TRIGGER_UNIMPLEMENTED 4u /* a special the metadata does not know: type ANY, no effects, never removed */
#define RDOOM_ACTION_NONE 0u           /* rdoom_world_step_game's d_actions (player.rs:397-406: push before shoot) */
#define RDOOM_ACTION_PUSH 1u
#define RDOOM_ACTION_SHOOT 2u
typedef struct rdoom_trigger {
  float origin[2], displace[2], length; /* Line2f::from_two_points(start vertex, end vertex), world coordinates */
  uint32_t trigger_type, flags, special_type;
  uint32_t effect_start, effect_end;    /* its move effects: rdoom_world_trigger_arrays.effects[effect_start, effect_end) */
} rdoom_trigger;
typedef struct rdoom_move_effect {      /* MoveEffect (visitor.rs:212-236) */
  uint32_t object_id;                   /* the floor or ceiling object it moves (>= 1) */
  float first_height_offset, second_height_offset; /* from_wad_height(target - the sector's height); second valid iff has_second */
  float speed, wait;                    /* speed: the metadata's / 8 * 0.7 per second; wait: seconds */
  uint32_t has_second, repeat;          /* repeat: parsed, ignored by Level::update */
} rdoom_move_effect;
/* borrowed pointers into a rdoom_world (valid until rdoom_world_destroy) */
typedef struct rdoom_world_trigger_arrays {
  const rdoom_trigger *triggers;
  uint32_t n_triggers;
  const rdoom_move_effect *effects;
  uint32_t n_effects;
  uint32_t n_objects; /* the game's objects, max(1, LevelAnalysis::num_objects): >= the collision world's n_objects and
                         >= rdoom_level_num_objects of the same level; the n_objects every game call needs at least */
} rdoom_world_trigger_arrays;
/* The trigger list and the move effects of the world's level.  Works on RDOOM_WORLD_HOST_ONLY worlds too. */
rdoom_status rdoom_world_triggers(const rdoom_world *world, rdoom_world_trigger_arrays *out);
/* The bytes of one player's game state (a multiple of 16).  N games live in one caller-owned device allocation of
 * N * bytes_per_player bytes, 16-byte aligned, player p's at byte p * bytes_per_player; a game can be moved or copied
 * bytewise.  Layout of one game, in 32-bit words, with T = n_triggers, O = n_objects, LW = ceil(T / 32), OW = ceil(O / 32):
 *   [0]           the number of live triggers (the length of the player's list), [1..3] zero
 *   live[LW]      bit t: trigger t (linedef order) is still in the list
 *   fired[LW]     zero between calls (the poll's bookkeeping)
 *   active[OW]    bit o: object o has an active effect
 *   second[OW]    bit o: that effect still holds its second offset
 *   order[T]      the list: entry i = the trigger at position i (the identity until an only_once trigger is removed)
 *   (zero padding to 16 bytes)
 *   effect[O]     4 floats per object: the active effect's first offset, second offset, wait left, speed */
rdoom_status rdoom_world_game_bytes(const rdoom_world *world, uint64_t *bytes_per_player);
/* A fresh level for player p of n wherever d_mask is NULL or d_mask[p] != 0 (d_mask: n bytes of device memory): every
 * trigger live in linedef order, no active effect, and entries [p][0 .. n_objects) of d_object_offsets (n x n_objects x xyz,
 * device memory) zero.  Other players' games and offsets are not touched.  Asynchronous on `stream`. */
rdoom_status rdoom_world_game_reset(const rdoom_world *world, void *d_game, float *d_object_offsets, uint32_t n_objects, uint32_t n,
                                    const uint8_t *d_mask, void *stream);
/* n_ticks game ticks (see above) for n_players players in one launch, asynchronous on `stream`; every pointer is device memory.
 * d_states, d_inputs, cfg, dt: as for rdoom_world_step_players, the tested domain of cfg and dt and the refused dt included;
 * dt is the tick of the physics and of the move effects alike.  d_actions: NULL (no action) or n_ticks x n_players bytes,
 * entry [t * n_players + p] = RDOOM_ACTION_NONE / PUSH / SHOOT of player p at tick t (any other value is no action).
 * d_game: n_players games (rdoom_world_game_bytes), read and written.  d_object_offsets: n_players x n_objects x xyz,
 * n_objects >= rdoom_world_trigger_arrays.n_objects; the step reads every entry (the collision sweeps) and writes only the y
 * of objects with an active effect, so the same array feeds rdoom_world_sweep, rdoom_world_step_players and
 * rdoom_object_modelviews_from_player.  An exit trigger sets RDOOM_PLAYER_EXITED; the player keeps stepping in the same
 * level.  Captured into a graph, it allocates and waits on nothing. */
rdoom_status rdoom_world_step_game(const rdoom_world *world, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                   const uint8_t *d_actions, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                   uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg, float dt, void *stream);
/* ---- world sets: several levels, and the exit that takes a player to the next -----------------------------------------
 * A rdoom_worldset holds the collision worlds and trigger lists of several levels, each built as rdoom_world_create builds it;
 * every player is in one of them (a device uint32 per player: its slot, the level_of_pose that rdoom_batch_render_levels takes
 * for a level set of the same list).  A game tick is rdoom_world_step_game's tick on the player's level, plus the level change
 * of the reference (game/src/level.rs:194-199, wad_system.rs:118-156, player.rs:118-133, 359-362): an exit trigger fires in
 * the poll of tick t; tick t + 1 still runs in the old level (effects advance, triggers fire); at the start of tick t + 2 the
 * player's slot becomes the destination, its game is fresh (every trigger live, no effect, offsets zero) and its state is
 * Player::reset's (pos = start, yaw = start yaw, pitch = 1e-8, velocity 0, last_height_diff 0; FLY / CLIP kept), then the tick
 * runs in the new level.  Slot s holds archive level level_indices[s]; its destination is the slot holding archive level
 * level_indices[s] + 1.  A slot without one (the archive's last level, or a gap in the list) keeps its players: an exit there
 * sets RDOOM_PLAYER_EXITED and nothing else, exactly as rdoom_world_step_game (the reference keeps its current level too, but
 * with its Level already removed; that broken state is not reproduced). */
typedef struct rdoom_worldset rdoom_worldset;
#define RDOOM_WORLDSET_NO_DESTINATION 0xFFFFFFFFu
typedef struct rdoom_worldset_level_info {
  uint32_t archive_index;   /* the level's index in the archive */
  uint32_t destination;     /* the slot an exit leads to, or RDOOM_WORLDSET_NO_DESTINATION */
  float start_pos[3];       /* Player::reset's position and yaw: rdoom_built_start of the same level */
  float start_yaw;
  uint32_t n_triggers;
  uint32_t n_objects;       /* the level's game objects (rdoom_world_trigger_arrays.n_objects) */
  uint32_t node_depth;
  rdoom_world_arrays world;                /* borrowed, valid until rdoom_worldset_destroy: the level's own arrays and indices, */
  rdoom_world_trigger_arrays triggers;     /* equal to rdoom_world_host_arrays / rdoom_world_triggers of the level */
} rdoom_worldset_level_info;
/* n_levels distinct archive level indices (n_levels >= 1; an empty list, an index out of range or a duplicate is
 * RDOOM_BAD_ARG).  flags: RDOOM_WORLD_HOST_ONLY builds the host arrays only (the game calls then return RDOOM_BAD_ARG). */
rdoom_status rdoom_worldset_create(const rdoom_wad *wad, const uint32_t *level_indices, uint32_t n_levels, uint32_t flags,
                                   rdoom_worldset **out_set);
void rdoom_worldset_destroy(rdoom_worldset *set);
/* out_n_objects: the set's game objects, the largest of its levels' (>= rdoom_level_num_objects of a level set of the same list);
 * the n_objects every set game call needs at least.  Either output may be NULL. */
rdoom_status rdoom_worldset_info(const rdoom_worldset *set, uint32_t *out_n_levels, uint32_t *out_n_objects);
rdoom_status rdoom_worldset_level(const rdoom_worldset *set, uint32_t slot, rdoom_worldset_level_info *out);
/* The bytes of one player's game in the set (a multiple of 16): the largest of its levels' rdoom_world_game_bytes.  A game holds
 * the layout of rdoom_world_game_bytes for the player's current level, with that level's T and O, and zero words after it.
 * Word 1 is the level change: 0 none, 1 an exit fired in the last tick, 2 the next tick loads the destination. */
rdoom_status rdoom_worldset_game_bytes(const rdoom_worldset *set, uint64_t *bytes_per_player);
/* A fresh game of its current level (d_levels[p]) for player p of n wherever d_mask is NULL or d_mask[p] != 0, and its
 * d_object_offsets row zero.  d_levels: n uint32 of device memory; a player whose slot is >= the set's size is not touched.
 * Asynchronous on `stream`. */
rdoom_status rdoom_worldset_game_reset(const rdoom_worldset *set, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                       const uint32_t *d_levels, uint32_t n, const uint8_t *d_mask, void *stream);
/* n_ticks game ticks for n_players players in one launch, asynchronous on `stream`; arguments as rdoom_world_step_game's (cfg and
 * dt: the domain the tests cover and the dt refused are rdoom_world_step_players'), with
 * d_game (rdoom_worldset_game_bytes per player) and n_objects >= rdoom_worldset_info's.  d_levels: n_players uint32 of device
 * memory, read and written: each player's slot, changed by the level change above.  A player whose slot is >= the set's size is
 * left untouched (state, game, offsets and slot).  K launches of one tick equal one launch of K ticks.  Captured into a graph,
 * it allocates and waits on nothing. */
rdoom_status rdoom_worldset_step_game(const rdoom_worldset *set, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                      const uint8_t *d_actions, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                      uint32_t *d_levels, uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg,
                                      float dt, void *stream);

/* The u_modelview of every object in the frame of a player at (pos, yaw, pitch), host arrays: out[o] (16 floats, column-major)
 * = Matrix4::from(view.concat(model_o)) with model_o = Decomposed { scale 1, rot identity, disp = offsets[o] } in the
 * reference's binary32 arithmetic (engine/src/renderer.rs:120-132), view as rdoom_pose_from_player builds it.  Object 0 (the
 * static world) and every object whose offset is (0, 0, 0) get the pose's own modelview, bit for bit.  offsets: n_objects x xyz
 * (one player's row of the step's d_object_offsets).  Ready for rdoom_batch_render_objects. */
rdoom_status rdoom_object_modelviews_from_player(const float pos[3], float yaw, float pitch, const float *offsets, uint32_t n_objects,
                                                 float *out);

/* ---- player frames: render the players in device arrays, without a host round trip ----
 * The cameras of n players whose states are in device memory, on the device: d_poses_out[p] is what rdoom_pose_from_player
 * returns for player p (projection and time bit for bit), and, when d_object_modelviews_out != NULL, the n x n_objects x 16
 * floats there are what rdoom_object_modelviews_from_player returns for player p's row of d_object_offsets (n x n_objects x
 * xyz, required then).  Same formulas, binary32, no contraction; the one difference is that sine and cosine come from the
 * project's sincos -- the world step's -- instead of libm sinf / cosf, so a modelview entry may differ from the host helpers'
 * in the last places: on 10 000 random states (yaw in +-60 pi, pitch at and inside the step's clamp) by at most 2^-19 -- absolute
 * for the rotation entries, relative to 1 + |x| + |y| + |z| of the position (plus offset) for the translation.  A test pins this
 * bound (tests/test_player_frames_host.py; observed: 2^-20).  Object 0 and every object at offset (0, 0, 0)
 * get the pose's modelview bit for bit.  Asynchronous on stream (a hipStream_t, may be NULL), on the current device. */
rdoom_status rdoom_poses_from_players_device(const rdoom_player_state *d_states, uint32_t n, uint32_t width, uint32_t height,
                                             float time, const float *d_object_offsets, uint32_t n_objects,
                                             rdoom_pose *d_poses_out, float *d_object_modelviews_out, void *stream);
/* rdoom_batch_render_levels for players whose state is on the device (all pointers here are device memory of the batch's
 * device): pose p is player p's camera as rdoom_poses_from_players_device computes it (time `time`), and it views level
 * d_levels[p] (NULL: level 0, allowed only on a batch of a single level).  Its objects sit at row p of d_object_offsets
 * (n_players x n_objects x xyz, n_objects >= rdoom_level_num_objects; NULL = every object at rest).  Its lights are
 * d_lights + d_levels[p] * lights_stride: one 256-byte table per level slot (lights_stride 256) or one shared table (0).
 * Asynchronous: it never waits on the host, and it allocates nothing after the batch's first render with objects.  A level
 * outside the set is rendered as level 0, and rdoom_batch_finish / rdoom_batch_read_* then report RDOOM_BAD_ARG naming the
 * first such pose (the frames of the other poses are correct).  The frames are those rdoom_batch_render_levels gives for the
 * same matrices, lights and levels, with one exception: the sky angle atan2(pm[8], pm[10]) (sky.vert) is correctly rounded
 * here, where the host path uses libm atan2f, so on rare poses a column of sky may sit one texel apart.  rdoom_batch_resolve_rgb
 * / rdoom_batch_read_rgb after such a render need a playpal for every level of the set.  flags: RDOOM_RENDER_PROFILED.
 * d_poses_out (n_players poses) and d_object_modelviews_out (n_players x n_objects x 16 floats, needs d_object_offsets) are
 * optional copies of what was rendered. */
rdoom_status rdoom_batch_render_players(rdoom_batch *batch, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                        const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_lights,
                                        uint32_t lights_stride, float time, uint32_t n_players, uint32_t kinds_mask,
                                        uint32_t flags, void *stream, rdoom_pose *d_poses_out, float *d_object_modelviews_out);

/* ---- device light set: every player's clock, and the sector lights at it, on the device ---------------
 * A rdoom_lightset holds the light infos of n_levels levels on the current device: infos[l] points at counts[l] infos (at most
 * 255; 0 is allowed, infos[l] may then be NULL), slot l of a level set or world set of the same list.  The infos are copied.  Any
 * table may be given, not only what rdoom_built_light_infos returns.  RDOOM_BAD_ARG: n_levels == 0, more than 255 infos in a
 * level, an info with has_effect != 0 whose effect_kind is not 0, 1 or 2. */
typedef struct rdoom_lightset rdoom_lightset;
rdoom_status rdoom_lightset_create(const rdoom_light_info *const *infos, const uint32_t *counts, uint32_t n_levels,
                                   rdoom_lightset **out);
void rdoom_lightset_destroy(rdoom_lightset *set);
/* The light tables of n players, asynchronous on `stream` (a hipStream_t, may be NULL); every pointer is device memory, nothing
 * is copied to the host and nothing waits.  Row p of d_out (n x 256 bytes, 4-byte aligned) is Lights::fill_buffer_at(d_times[p])
 * of level d_levels[p] (d_levels NULL: slot 0 for everyone): entry i < the level's count is
 *   (clamp(light_level_at(info_i, d_times[p])) * 255.0) as u8
 * and entries from the count upwards are 0.  A slot outside the set is seen on the device only: that player's row is 256 zeros,
 * and nothing else is written for it.  n == 0 queues nothing.
 * Arithmetic -- light_level_at, noise, fract, clamp of game/src/lights.rs:33-78, restated operation for operation in binary32, no
 * contraction, IEEE division and floor:
 *   no effect:  level
 *   Glow:       scale = level - alt_level; phase = time * speed / scale; |0.5 - fract(phase)| * 2 * scale + alt_level
 *   Random:     noise(sync, floor(time * speed)) < duration ? alt_level : level
 *   Alternate:  fract(time * speed + sync * 3.5435) < duration ? alt_level : level
 *   noise(s, t) = fract(1 + sin((s + t / 1000) * 12.9898 + s * 78.233) * 43758.547);  fract(x) = x - floor(x)
 *   clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x)   (a NaN passes through)
 * `as u8` is Rust's: truncation towards zero, saturation at 0 and 255, NaN gives 0.  A Glow light with level == alt_level divides
 * by zero: phase is +-inf or NaN, fract of it NaN, the entry 0 -- what Rust gives; the host's rdoom_built_lights_at casts that NaN
 * in C++, which is undefined, so this case is defined here and not by the host.
 * The one deliberate difference from rdoom_built_lights_at: the sine in noise is the binary64 sine of the binary32 argument,
 * rounded once to binary32 (the correctly rounded sine, unless the binary64 value lies within its own error of the midpoint of
 * two binary32 numbers).  The host calls libm sinf, which is not correctly rounded and which no device library reproduces.  So a
 * row equals rdoom_built_lights_at(d_times[p]) except at Random entries whose sinf differs from the correctly rounded sine at
 * that argument (about 1 % of arguments), and there only if the noise value then falls on the other side of `duration`. */
rdoom_status rdoom_lightset_tables(const rdoom_lightset *set, const uint32_t *d_levels, const float *d_times, uint32_t n,
                                   uint8_t *d_out, void *stream);
/* rdoom_poses_from_players_device with a clock per player: pose p's time is d_times[p] (n floats of device memory). */
rdoom_status rdoom_poses_from_players_device_clocked(const rdoom_player_state *d_states, uint32_t n, uint32_t width, uint32_t height,
                                                     const float *d_times, const float *d_object_offsets, uint32_t n_objects,
                                                     rdoom_pose *d_poses_out, float *d_object_modelviews_out, void *stream);
/* rdoom_batch_render_players with a clock per player: pose p's u_time is d_times[p] and its light table is row p of
 * rdoom_lightset_tables(lights, d_levels, d_times, ...), written straight into the batch's per-pose constants -- the caller owns
 * no n x 256 buffer and the host computes nothing per render.  Everything else (arguments, frames, the sky angle, a level outside
 * the set rendered as level 0 -- with level 0's lights -- and reported by rdoom_batch_finish) is rdoom_batch_render_players'.
 * It queues that render's launches plus one, the light tables; it never waits, allocates nothing after the batch's first render
 * with objects, and can be captured into a graph.  Checked on the host before anything is queued (RDOOM_BAD_ARG): a NULL light
 * set or NULL d_times; a light set whose level count differs from the batch's level set's, or that lives on another device. */
rdoom_status rdoom_batch_render_players_clocked(rdoom_batch *batch, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                                const float *d_object_offsets, uint32_t n_objects, const rdoom_lightset *lights,
                                                const float *d_times, uint32_t n_players, uint32_t kinds_mask, uint32_t flags,
                                                void *stream, rdoom_pose *d_poses_out, float *d_object_modelviews_out);

/* ---- ray casts: range-sensor rays from player states through the world --------------------------------
 * n players x n_rays rays in one launch, asynchronous on `stream`; every pointer is device memory, nothing is copied to the
 * host and nothing waits.  d_states: the n states a step leaves.  d_dirs: ONE table of n_rays camera-frame directions (xyz
 * float32, -z is forward), shared by every player; it need not be normalised.
 * Origin: ray (p, r) starts at player p's camera eye, the `disp` of player.concat(camera): rotate(q_player, (0, 0.12, 0)) + pos
 * with q_player = Quaternion::from(Euler { x: pitch, y: yaw, z: 0 }) -- what rdoom_poses_from_players_device computes, in its
 * operation order, sine and cosine from the project's sincos.  Direction: dir = rotate(q_player, d_dirs[r]), vel = dir * max_range.
 * Ray against triangle: the plane branch of Sphere::sweep_triangle (math/src/sphere.rs:16-53) at radius 0 and nothing else:
 * speed = |vel|, nvel = vel / speed; normal . nvel >= 0 rejects the triangle; signed_plane_distance < 0 rejects it;
 * distance = -signed_plane_distance / (normal . nvel); is_point_inside_triangle(origin + nvel * distance) decides the hit;
 * time = distance / speed.  Binary32, no contraction, IEEE division and square root, rdoom_world_sweep's operand order.  The
 * vertex and edge branches are left out on purpose: at radius 0 they can fire only through rounding.
 * Traversal: World::sweep_sphere at radius 0 (world.rs:40-82): Node::intersect_sphere with radius 0, the positive child first,
 * leaves swept when met, then the dynamic chunks with the origin moved by minus the object's offset (row p of d_object_offsets,
 * n x n_objects x xyz as for rdoom_world_sweep with one row per PLAYER; NULL = every object at rest); the fold keeps the later
 * candidate on equal times.  The result is defined as that fold.
 * d_frac_out[p * n_rays + r] (float32): time when time <= 1, else +inf -- the fraction of max_range, +inf = nothing within
 * range.  d_hit_out (uint32, may be NULL): the winning triangle's index in the level's own rdoom_world_arrays.triangles, or
 * 0xFFFFFFFF where the fraction is +inf; for a world set the index within that slot's arrays (rdoom_worldset_level), the set's
 * rebasing undone.  d_origin_out / d_vel_out (xyz float32 per ray, may be NULL): the origin and vel the kernel used, so that the
 * very same rays can be handed to rdoom_world_sweep with radius 0.
 * Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle, d_dirs, or (n > 0) d_states / d_frac_out /
 * d_levels; n_rays == 0; max_range not finite or not positive; d_object_offsets with n_objects smaller than the world's (the
 * set's: its largest level's); a world created with RDOOM_WORLD_HOST_ONLY.  n == 0 queues nothing.  A level slot >= the set's
 * size is seen on the device only: that player's rays get +inf / 0xFFFFFFFF and nothing else of them is written. */
#define RDOOM_RAY_NO_HIT 0xFFFFFFFFu
rdoom_status rdoom_world_cast_rays(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                                   uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects,
                                   float *d_frac_out, uint32_t *d_hit_out, float *d_origin_out, float *d_vel_out, void *stream);
rdoom_status rdoom_worldset_cast_rays(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                      uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                                      const float *d_object_offsets, uint32_t n_objects, float *d_frac_out, uint32_t *d_hit_out,
                                      float *d_origin_out, float *d_vel_out, void *stream);

/* ---- top-down maps: every player's automap, drawn on the device from its game state --------------------
 * The level's line table: one record per linedef whose two vertex indices are valid (Level::vertex, wad/src/level.rs:83-87), in
 * linedef order.  a, b: the start and end vertex in world xz (from_wad_coords, wad/src/util.rs:20-22: x = -wad_y / 100,
 * z = -wad_x / 100).  flags, special_type: WadLinedef's, verbatim (wad/src/types.rs:49-57).  front is the right side, back the
 * left (Level::right_sidedef / left_sidedef / sidedef_sector, level.rs:131-151): present = 1 when the linedef has that sidedef and
 * the sidedef's sector exists, else the record is zero; floor / ceiling: from_wad_height of the sector's heights (util.rs:12-14);
 * floor_id / ceiling_id: the objects SectorInfo gives the sector's floor and ceiling (wad/src/visitor.rs:145-156, 569-588) as the
 * game numbers them -- the ids that index d_object_offsets and that rdoom_move_effect.object_id names -- 0 for a sector no
 * DynamicSectorInfo moves. */
typedef struct rdoom_map_side {
  uint32_t present;
  float floor, ceiling;
  uint32_t floor_id, ceiling_id;
} rdoom_map_side;
typedef struct rdoom_map_line {
  uint32_t linedef;      /* its index in LINEDEFS */
  float a[2], b[2];
  uint32_t flags, special_type;
  rdoom_map_side front, back;
} rdoom_map_line;
/* borrowed pointers into a rdoom_world / rdoom_worldset (valid until it is destroyed) */
typedef struct rdoom_map_lines {
  const rdoom_map_line *lines;
  uint32_t n_lines;
} rdoom_map_lines;
/* The line table of the world's level, and of slot `slot` of a set (equal to the single world's of the same level).  Both work on
 * RDOOM_WORLD_HOST_ONLY handles. */
rdoom_status rdoom_world_map_lines(const rdoom_world *world, rdoom_map_lines *out);
rdoom_status rdoom_worldset_level_map_lines(const rdoom_worldset *set, uint32_t slot, rdoom_map_lines *out);

/* The classes of a map pixel, and the view of a map.  width x height pixels; scale: world units per pixel; half_width: half the
 * thickness of a line in pixels; marker: the size of the player marker in pixels (0: none).  flags: RDOOM_MAP_ROTATE the player's
 * view direction is up (else map north); RDOOM_MAP_SHOW_FLAT draws FLAT lines; RDOOM_MAP_SHOW_HIDDEN draws linedefs with flag 0x80;
 * RDOOM_MAP_TOP_DOWN row 0 of the output is the top row (else the bottom row). */
#define RDOOM_MAP_NONE 0u
#define RDOOM_MAP_FLAT 1u
#define RDOOM_MAP_CEILING_STEP 2u
#define RDOOM_MAP_FLOOR_STEP 3u
#define RDOOM_MAP_CLOSED 4u
#define RDOOM_MAP_ONE_SIDED 5u
#define RDOOM_MAP_PLAYER 8u
#define RDOOM_MAP_ROTATE 1u
#define RDOOM_MAP_SHOW_FLAT 2u
#define RDOOM_MAP_SHOW_HIDDEN 4u
#define RDOOM_MAP_TOP_DOWN 8u
typedef struct rdoom_map_view {
  uint32_t width, height;
  float scale, half_width, marker;
  uint32_t flags;
} rdoom_map_view;
/* n players' maps in one launch, asynchronous on `stream` (a hipStream_t, may be NULL); every pointer but `view` is device memory,
 * nothing is allocated, nothing is copied to the host and nothing waits, so the call can be captured into a graph.  d_states: the n
 * states a step leaves; d_object_offsets: NULL (every object at rest) or n x n_objects x xyz, the step's; d_levels: each player's
 * slot.  d_out: n x height x width bytes, map p at byte p * height * width, row-major, one class code per pixel.
 * Every float below is binary32, every operation is rounded once and none is contracted; a + b * c means round(a + round(b * c)).
 * Pixel to world.  The byte at row `row`, column i of map p is pixel (i, j) with j = row, or j = height - 1 - row with
 * RDOOM_MAP_TOP_DOWN.  hw = (float)width * 0.5f, hh = (float)height * 0.5f (exact);
 *   u = (((float)i + 0.5f) - hw) * scale;  v = (((float)j + 0.5f) - hh) * scale;
 * without RDOOM_MAP_ROTATE map north is up and map east is right: q = (pos.x - v, pos.z - u), pos the player's position, q in
 * world xz.  With it, (s, c) = the project's sincos of yaw (csrc/hip/sincos_rd.hpp, the step's), the forward f = (-s, -c) is up and
 * r = (c, -s) is right: q.x = (pos.x + c * u) + (-s) * v;  q.z = (pos.z + (-s) * u) + (-c) * v.
 * Segment distance, dist2(q, a, b, &ok): dx = b.x - a.x; dz = b.z - a.z; len2 = dx * dx + dz * dz; ok = len2 > 0; inv = 1.0f / len2
 * (IEEE division); wx = q.x - a.x; wz = q.z - a.z; t = (wx * dx + wz * dz) * inv; t = t < 0 ? 0 : (t > 1 ? 1 : t);
 * ex = wx - t * dx; ez = wz - t * dz; dist2 = ex * ex + ez * ez.
 * Lines.  Line l of the player's level is skipped when its len2 is not > 0, or when flags & 0x80 without RDOOM_MAP_SHOW_HIDDEN.  Its
 * class for player p: RDOOM_MAP_ONE_SIDED if front.present and back.present are not both 1 or flags & 0x20 (secret).  Otherwise, with
 * the live heights ff = front.floor + off(front.floor_id), fc = front.ceiling + off(front.ceiling_id), bf and bc alike from back,
 * off(o) = d_object_offsets[(p * n_objects + o) * 3 + 1] and 0 for o == 0, o >= n_objects or a NULL d_object_offsets:
 *   RDOOM_MAP_CLOSED if fc <= ff or bc <= bf (a shut door); else RDOOM_MAP_FLOOR_STEP if ff != bf; else RDOOM_MAP_CEILING_STEP if
 *   fc != bc; else RDOOM_MAP_FLAT, which is skipped without RDOOM_MAP_SHOW_FLAT.
 * A line covers q when ok and dist2(q, a, b) <= w2, w2 = (half_width * scale) * (half_width * scale).
 * Marker.  With marker > 0: m = marker * scale; e = (pos.x + f.x * (2.0f * m), pos.z + f.z * (2.0f * m)), f as above (under either
 * orientation); the marker covers q when ok and dist2(q, pos.xz, e) <= m * m.
 * Pixel value: RDOOM_MAP_PLAYER where the marker covers q; else the largest class among the lines that cover q; else
 * RDOOM_MAP_NONE.  A maximum, so the value does not depend on the order in which lines are visited.  A comparison with a NaN is
 * false: a player at a NaN position gets an all-zero map.
 * A level slot >= the set's size is seen on the device only: that player's map is all RDOOM_MAP_NONE.
 * Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle or view, or (n > 0) NULL d_states / d_out / d_levels;
 * width or height 0 or above 16384; scale or half_width not finite or not > 0; marker not finite or < 0; unknown flags;
 * d_object_offsets with n_objects smaller than the game's objects (rdoom_world_trigger_arrays.n_objects; the set's:
 * rdoom_worldset_info's); n x the view's 32 x 32 pixel tiles above 2^31 - 1; a handle created with RDOOM_WORLD_HOST_ONLY or living on
 * another device.  n == 0 queues nothing. */
rdoom_status rdoom_world_draw_maps(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n,
                                   const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view, uint8_t *d_out,
                                   void *stream);
rdoom_status rdoom_worldset_draw_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                      uint32_t n, const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                      uint8_t *d_out, void *stream);

/* ---- seen lines: each player's map revealed as it explores -----------------------------------------------------
 * Doom's automap draws a line only once the player has had it in view; its visibility is two-dimensional -- solid-seg clipping on
 * map lines, solid meaning one-sided or shut -- and eye height plays no part.  This is that idea made exact: a fan of 2-D rays from
 * the player through the line table, a set of seen lines per player kept on the device as a row of bits, and the maps drawn
 * through it.  Every float below is binary32, every operation is rounded once and none is contracted; divisions are IEEE;
 * a * b - c * d means round(round(a * b) - round(c * d)).
 * Fan.  d_dirs: ONE table of n_rays directions (right, forward), two floats per ray, shared by every player; it need not be
 * normalised.  With (s, c) = the project's sincos of the player's yaw (csrc/hip/sincos_rd.hpp), the map contract's r = (c, -s) and
 * f = (-s, -c):  dir.x = c * right + (-s) * forward;  dir.z = (-s) * right + (-c) * forward;  vel.x = dir.x * max_range;
 * vel.z = dir.z * max_range;  o = (pos.x, pos.z).  The ray is o + t * vel, t in [0, 1].
 * Ray against line l, a and b its end points:  dx = b.x - a.x;  dz = b.z - a.z;  len2 = dx * dx + dz * dz;  wx = a.x - o.x;
 * wz = a.z - o.z;  den = vel.x * dz - vel.z * dx;  t = (wx * dz - wz * dx) / den;  u = (wx * vel.z - wz * vel.x) / den.
 * The ray hits the line when len2 > 0, den != 0, u >= 0, u <= 1, t >= 0 and t <= 1.  (A zero den gives a NaN or an infinity, a NaN
 * fails every comparison: no hit.)
 * Blocking.  Line l blocks player p's sight when front.present and back.present are not both 1, or when its opening is empty under
 * the live heights: with ff, fc, bf, bc as the map contract defines them (height + off(id) from row p of d_object_offsets),
 * lo = ff > bf ? ff : bf;  hi = fc < bc ? fc : bc;  the line blocks when !(hi > lo).  So a shut door blocks in the game of the
 * player who has not opened it, and only there.  No flag blocks: a secret line (0x20) is seen through like any other two-sided one.
 * Seen.  For ray r, T_r is the smallest t among the blocking lines it hits, or 1 if it hits none.  Line l is seen by r when r hits
 * l with t <= T_r, t being the value that entered the minimum: the blocking line itself is seen, and every line tied with it.
 * A line is seen by the player when one of the n_rays rays sees it.
 * Accumulation.  d_seen: n rows of `stride` uint32 words.  Bit l % 32 of word p * stride + l / 32 is OR-ed in when player p sees
 * line l, l the index in the level's own table (rdoom_world_map_lines / rdoom_worldset_level_map_lines).  Bits are never cleared;
 * words of a row beyond the level's ceil(n_lines / 32) and bits beyond n_lines are never written; the caller zeroes a row to start
 * an episode.  A minimum followed by an OR: the result does not depend on the order in which rays or lines are visited.
 * d_new_out (n uint32, may be NULL): d_new_out[p] = the number of bits this call set in row p that were clear before.
 * A comparison with a NaN is false: a player at a NaN position marks nothing and counts 0.  A level slot >= the set's size is seen
 * on the device only: that player's row is untouched and its count is 0.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle, or (n > 0) NULL d_states /
 * d_seen / d_dirs / d_levels; n_rays == 0; max_range not finite or not > 0; a stride smaller than ceil(n_lines / 32) of the world's
 * table (the set's: of its largest level's); d_object_offsets with n_objects smaller than the game's objects (as for
 * rdoom_world_draw_maps); a handle created with RDOOM_WORLD_HOST_ONLY or living on another device.  n == 0 queues nothing. */
rdoom_status rdoom_world_reveal_lines(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                                      uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects,
                                      uint32_t *d_seen, uint32_t stride, uint32_t *d_new_out, void *stream);
rdoom_status rdoom_worldset_reveal_lines(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                         uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                                         const float *d_object_offsets, uint32_t n_objects, uint32_t *d_seen, uint32_t stride,
                                         uint32_t *d_new_out, void *stream);
/* The maps drawn through the set: rdoom_world_draw_maps / rdoom_worldset_draw_maps in every respect, except that player p's map
 * additionally skips line l unless bit l of row p of d_seen (rows of `stride` words, as above) is set or the linedef carries
 * RDOOM_LINE_MAPPED, Doom's "already on the map" flag (WadLinedef flags, in the table verbatim).  The marker is always drawn.  A NULL
 * d_seen gives the omniscient map, the bytes of rdoom_world_draw_maps.  One more error (RDOOM_BAD_ARG): a non-NULL d_seen with a
 * stride smaller than the table's words. */
#define RDOOM_LINE_MAPPED 0x100u
rdoom_status rdoom_world_draw_maps_seen(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n,
                                        const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                        const uint32_t *d_seen, uint32_t stride, uint8_t *d_out, void *stream);
rdoom_status rdoom_worldset_draw_maps_seen(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                           uint32_t n, const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                           const uint32_t *d_seen, uint32_t stride, uint8_t *d_out, void *stream);

/* ---- sectors: the sector under a player, and every player's filled top-down map -------------------------------
 * The level's sector table.  sectors: one record per SECTORS entry, in lump order.  floor / ceiling: from_wad_height of the
 * sector's heights, the values rdoom_map_side carries; floor_id / ceiling_id: the objects SectorInfo gives them, as in the line table
 * (they index d_object_offsets, rdoom_move_effect.object_id names them), 0 for a sector nothing moves; light_level, sector_type,
 * tag: WadSector's 16-bit fields, verbatim (wad/src/types.rs:98-108).
 * Leaves.  The collision world's BSP (rdoom_world_node, children packed: > 0 a node, <= 0 minus a chunk) has one chunk per leaf, in
 * walk order.  leaf_sector[chunk]: the sector of the sub-sector that produced the chunk -- the sector of its first seg, as
 * LevelWalker::subsector picks it (wad/src/visitor.rs:621-640) -- or RDOOM_SECTOR_NONE for a leaf the walk skipped, and for chunk 0
 * of a level whose walk met no leaf (a child that was never linked reads as chunk 0).  n_leaves = max(1, the world's n_chunks).
 * leaf_edges[chunk] = (first, count): the leaf's solid edges, edges[first .. first + count) -- those segs of its sub-sector whose
 * linedef has no sidedef on the seg's other side (Level::seg_back_sidedef), in seg order.  An edge is a = the seg's start vertex and
 * d = its end vertex - a, each component rounded once, in world xz.  The sub-sector lies where
 * cross = (q.x - a.x) * d.z - (q.z - a.z) * d.x is <= 0; cross > 0 is the outside of the edge.
 *
 * The sector at a point q = (q.x, q.z), the authority for everything below.  Every value is binary32, every operation is rounded
 * once, nothing is contracted, there is no division; a * b - c * d means round(round(a * b) - round(c * d)).
 * Descent.  From node 0 of the level (its root): with the node's origin o and displace d (rdoom_world_node, both in xz),
 *   dist = (q.x * d.y - q.z * d.x) + (d.x * o.y - d.y * o.x)
 * (Line2::signed_distance, the expression the sweep evaluates); take child `positive` when dist >= 0, else `negative`; repeat
 * while the child is > 0.  A child <= 0 names the leaf, chunk -child.
 * Void.  q is void when some solid edge of the leaf has cross > 0, cross as above.  A point exactly on an edge is inside.
 * Result.  leaf_sector[leaf], or RDOOM_SECTOR_NONE when q is void.  It is RDOOM_SECTOR_NONE too when q.x or q.z is a NaN (whose
 * comparisons, all false, would otherwise lead down the negative children into some leaf).
 * A function of the point and the tables alone: an implementation may start the descent below the root wherever that cannot change
 * the result. */
#define RDOOM_SECTOR_NONE 0xFFFFFFFFu
#define RDOOM_SECTOR_NONE16 0xFFFFu
typedef struct rdoom_map_sector {
  float floor, ceiling;
  uint32_t floor_id, ceiling_id;
  uint32_t light_level, sector_type, tag;
} rdoom_map_sector;
typedef struct rdoom_map_edge {
  float a[2], d[2];
} rdoom_map_edge;
typedef struct rdoom_map_leaf_edges {
  uint32_t first, count;
} rdoom_map_leaf_edges;
/* borrowed pointers into a rdoom_world / rdoom_worldset (valid until it is destroyed) */
typedef struct rdoom_map_sectors {
  const rdoom_map_sector *sectors;
  const uint32_t *leaf_sector;
  const rdoom_map_leaf_edges *leaf_edges;
  const rdoom_map_edge *edges;
  uint32_t n_sectors, n_leaves, n_edges;
} rdoom_map_sectors;
/* The sector table of the world's level, and of slot `slot` of a set (equal to the single world's of the same level, in the level's
 * own indices).  Both work on RDOOM_WORLD_HOST_ONLY handles. */
rdoom_status rdoom_world_map_sectors(const rdoom_world *world, rdoom_map_sectors *out);
rdoom_status rdoom_worldset_level_map_sectors(const rdoom_worldset *set, uint32_t slot, rdoom_map_sectors *out);

/* The sector under each of n players, in one launch, asynchronous on `stream`; every pointer is device memory, nothing is allocated,
 * nothing is copied to the host and nothing waits, so the call can be captured into a graph.  d_states, d_object_offsets / n_objects,
 * d_levels: as for rdoom_world_draw_maps.
 * d_sector_out[p]: the sector at (pos.x, pos.z) of player p, an index into its level's own table, or RDOOM_SECTOR_NONE.
 * d_heights_out (n x 2 floats, may be NULL): the sector's live floor and ceiling, floor + off(floor_id) and ceiling +
 *   off(ceiling_id) with the map contract's off() on row p of d_object_offsets; (+inf, -inf) where the sector is none.
 * d_visited (n rows of `stride` uint32 words, may be NULL): bit s % 32 of word p * stride + s / 32 is OR-ed in for the sector s
 *   player p stands in.  Bits are never cleared; words beyond the level's ceil(n_sectors / 32) and bits beyond n_sectors are never
 *   written; the caller zeroes a row to start an episode.
 * d_new_out (n uint32, may be NULL): 1 when this call set a bit of row p that was clear, else 0; 0 with a NULL d_visited and where
 *   the sector is none.
 * A level slot >= the set's size is seen on the device only: the sector is none, the row is untouched and d_new_out is 0.
 * Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle, or (n > 0) NULL d_states / d_sector_out / d_levels;
 * d_visited with a stride smaller than ceil(n_sectors / 32) of the world's table (the set's: of its largest level's);
 * d_object_offsets with n_objects smaller than the game's objects; a handle created with RDOOM_WORLD_HOST_ONLY or living on another
 * device.  n == 0 queues nothing. */
rdoom_status rdoom_world_locate_players(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n,
                                        const float *d_object_offsets, uint32_t n_objects, uint32_t *d_sector_out, float *d_heights_out,
                                        uint32_t *d_visited, uint32_t stride, uint32_t *d_new_out, void *stream);
rdoom_status rdoom_worldset_locate_players(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                           uint32_t n, const float *d_object_offsets, uint32_t n_objects, uint32_t *d_sector_out,
                                           float *d_heights_out, uint32_t *d_visited, uint32_t stride, uint32_t *d_new_out,
                                           void *stream);

/* Every player's filled top-down map: per pixel of the map contract's grid, the sector at the pixel's point.  view: width, height
 * and scale are read, RDOOM_MAP_ROTATE and RDOOM_MAP_TOP_DOWN honoured, any other flag is an error; half_width and marker are not
 * read.  The pixel's point q is the map contract's ("Pixel to world" above), operation for operation, so a sector map and a line map
 * of the same view register exactly.  With s = the sector at q in the player's level:
 * d_sector_out (n x height x width uint16, may be NULL): s, or RDOOM_SECTOR_NONE16 for none and for any s >= 0xFFFF.
 * d_floor_out / d_ceiling_out (n x height x width floats, may be NULL): the live floor / ceiling of s for player p, as
 *   rdoom_world_locate_players defines them; +inf / -inf for none.
 * At least one of the three is given.  d_visited / stride (may be NULL): rows as rdoom_world_locate_players keeps them; a pixel
 * whose sector's bit is clear in row p is written as none in every plane -- the filled map revealed as the player explores.
 * A level slot >= the set's size is seen on the device only: that player's planes are all none.
 * Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_world_draw_maps that concern what is read here
 * (handle, view, d_states, d_levels, width, height, scale, flags, n_objects, the tile count, host-only, the device); all three
 * outputs NULL (n > 0); d_visited with a stride smaller than the table's words.  n == 0 queues nothing. */
rdoom_status rdoom_world_draw_sector_maps(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n,
                                          const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                          const uint32_t *d_visited, uint32_t stride, uint16_t *d_sector_out, float *d_floor_out,
                                          float *d_ceiling_out, void *stream);
rdoom_status rdoom_worldset_draw_sector_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                             uint32_t n, const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                             const uint32_t *d_visited, uint32_t stride, uint16_t *d_sector_out, float *d_floor_out,
                                             float *d_ceiling_out, void *stream);

/* ---- flood: every player's sector map flooded from a seed cell, the walking distance to each cell ----------------
 * Where a player can go from where it stands, and in how many steps: a shortest-path flood over the floor and ceiling planes of a
 * filled map.  A pure function of the two planes: no handle, no table.  Every float below is binary32, every operation is rounded
 * once and none is contracted.
 * Inputs.  d_floor, d_ceiling: n x height x width floats each, exactly what rdoom_world_draw_sector_maps stores -- row r, column c,
 * either row order, a void cell +inf / -inf.  The flood works on stored rows: flipping the rows flips the result, so there is no
 * orientation flag.
 * Open.  With f the floor and g the ceiling of a cell, the cell is open when f < +inf && f > -inf && g - f >= clearance.  A NaN makes
 * every comparison false: that cell is closed.
 * Moves.  A move from cell a to a 4-neighbour b inside the grid is allowed when both cells are open, f_b - f_a <= max_step,
 * f_a - f_b <= max_drop, and fminf(g_a, g_b) - fmaxf(f_a, f_b) >= clearance.  max_drop may be +inf.  Moves are directed: a ledge can
 * be dropped from but not climbed.
 * Seeds.  d_seeds: n x 2 int32 (column, row) in stored order; NULL: (width / 2, height / 2) for every player -- the cell at, or with
 * a corner at, the player's point of the map contract.
 * d_dist_out (n x height x width uint16): the smallest number of allowed moves from player p's seed to the cell, 0 at the seed;
 *   RDOOM_FLOOD_UNREACHED where there is no path, where the cell is closed, and everywhere when the seed is closed or outside the
 *   grid.
 * d_count_out (n uint32, may be NULL): the number of cells of player p with a distance below RDOOM_FLOOD_UNREACHED.
 * params: max_step, max_drop, clearance as above; flags must be 0.  The limits model walking -- Doom's 24-unit step and 56-unit
 * body are 0.24 and 0.56 at this library's scale -- and nothing ties them to the sphere-and-spring physics of
 * rdoom_world_step_players.
 * width * height is at most rdoom_flood_max_cells' *cells_out, a constant of the library chosen from the kernel's LDS layout: at
 * least 19 200 (160 x 120) and below 65 535, so that a distance always fits.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): NULL params; (n > 0) NULL d_floor /
 * d_ceiling / d_dist_out; a zero width or height; more cells than rdoom_flood_max_cells; non-zero flags; a NaN or negative max_step,
 * max_drop or clearance; NULL cells_out.  n == 0 queues nothing. */
#define RDOOM_FLOOD_UNREACHED 0xFFFFu
typedef struct rdoom_flood_params {
  float max_step, max_drop, clearance;
  uint32_t flags;
} rdoom_flood_params;
rdoom_status rdoom_flood_max_cells(uint32_t *cells_out);
rdoom_status rdoom_flood_maps(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                              const int32_t *d_seeds, const rdoom_flood_params *params, uint16_t *d_dist_out, uint32_t *d_count_out,
                              void *stream);

/* ---- spawn: players reset on the device, at seeded random points of their level's walkable floor ---------------
 * One launch writes a fresh rdoom_player_state for every player whose mask byte is set: a pseudo-random point of the level's floor
 * where a body fits, reproducible from a seed, or the level's start.  The reference project has no counterpart of this: nothing
 * here restates it.
 * Spawn table.  One per level, a pure function of rdoom_world_arrays: the triangles whose normal vertex has y > 0 (the floors of
 * WorldBuilder::floor, static and dynamic alike), in the order of the triangle array.  With a, b, c = the triangle's v1, v2, v3, its
 * area is 0.5 * fabs((b.x - a.x) * (c.z - a.z) - (b.z - a.z) * (c.x - a.x)) in binary64 (the vertices converted, every operation
 * rounded once, nothing contracted); a triangle whose area is not > 0 has no entry.  cumulative: the binary64 sum of the areas up to
 * and including the entry, in table order, rounded once to binary32.  total = the last entry's cumulative, 0 for an empty table.
 * start_pos / start_yaw: the level's start (rdoom_worldset_level_info's), the state a fallback writes.
 * Generator.  Philox4x32-10 (Salmon et al., SC'11), integer only and stateless.  Key k = (seed & 0xFFFFFFFF, seed >> 32); counter
 * x = (p, e, t, 0) with p the player's index in the call, e = d_episode[p] (0 with a NULL d_episode) and t the try, 1 .. 8.  Ten
 * rounds of: (h0, l0) = the high and low 32 bits of 0xD2511F53 * x0, (h1, l1) = those of 0xCD9E8D57 * x2,
 * x = (h1 ^ x1 ^ k0, l1, h0 ^ x3 ^ k1, l0); between rounds (nine times) k0 += 0x9E3779B9, k1 += 0xBB67AE85, all modulo 2^32.  The four
 * draws of a try are u_i = (float)(x_i >> 8) * 0x1p-24f, exact and in [0, 1).  The same (seed, p, e) gives the same state in any batch.
 * Candidate (binary32, every operation rounded once, nothing contracted).  target = u0 * total.  The entry is the first whose
 * cumulative > target, found as: lo = 0, hi = n_entries; while lo < hi { mid = (lo + hi) >> 1; if cumulative[mid] > target
 * hi = mid; else lo = mid + 1; }; the entry is lo, or n_entries - 1 when lo == n_entries (target rounded up to total).  If
 * u1 + u2 > 1, u1 = 1 - u1 and u2 = 1 - u2.  q = (a + u1 * (b - a)) + u2 * (c - a), x, y and z alike.
 * Validity.  With s(x, z) the sector at a point ("sectors" above), and f(s), g(s) its live floor and ceiling for player p exactly as
 * rdoom_world_locate_players gives them (height + off(id) on row p of d_object_offsets), a point (x, z) is clear when s(x, z) is not
 * RDOOM_SECTOR_NONE and g - f >= clearance.  The candidate is valid when q is clear, fabsf(f(s(q)) - q.y) <= max_step (a floor
 * triangle lying under another floor is not stood on), and each of the eight points (q.x + margin, q.z), (q.x - margin, q.z),
 * (q.x, q.z + margin), (q.x, q.z - margin), (q.x + k, q.z + k), (q.x - k, q.z + k), (q.x + k, q.z - k), (q.x - k, q.z - k) with
 * k = margin * 0.70710677f is clear and, with rise = its f - f(s(q)), has fabsf(rise) <= max_step and not
 * (rise > 0 && rise < RDOOM_SPAWN_RISE - margin).  The last term is the landing rule: the body starts with its centre
 * RDOOM_SPAWN_RISE above the floor, so a floor beside it that is higher by less than RDOOM_SPAWN_RISE - margin lies under the body's
 * sphere, which would come down on that floor's edge and slide off it; a higher one is a wall to it.  A NaN in fabsf(rise) <= max_step
 * or in a clearance makes the comparison false: not valid.  A shut door (ceiling == floor) is excluded by the clearance, in the game
 * of the player who has not opened it only.
 * Tries.  t = 1, 2 .. RDOOM_SPAWN_TRIES; the first valid candidate wins.  An empty table has no candidate.
 * The state written.  pos = (q.x, f(s(q)) + RDOOM_SPAWN_RISE, q.z): as high above the live floor as the start is above the floor at
 * the start marker; vel = 0; yaw = u3 * 6.2831855f (the try's fourth draw, one binary32 product); pitch = 1e-8f;
 * last_height_diff = 0; flags = params->flags.  Without a valid candidate: pos = start_pos, yaw = start_yaw, the rest the same --
 * byte for byte the state the level's start gives.
 * d_tries_out (n uint32, may be NULL): the winning try, 1 .. RDOOM_SPAWN_TRIES, or 0 for the start state.
 * d_mask (n bytes, may be NULL: every player): where the byte is 0 neither the state nor d_tries_out[p] is written.
 * d_episode (n uint32, may be NULL) is read and never written: the caller adds the mask to it to get other points at the next reset.
 * d_states, d_object_offsets / n_objects, d_levels: as for rdoom_world_locate_players.  A level slot >= the set's size is seen on
 * the device only: that state is untouched and d_tries_out[p] is 0.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle or params; (n > 0) NULL
 * d_states / d_levels; a NaN or negative margin, clearance or max_step; d_object_offsets with n_objects smaller than the game's
 * objects; a handle created with RDOOM_WORLD_HOST_ONLY or living on another device.  An empty table is no error: every masked player
 * gets the start state.  n == 0 queues nothing. */
#define RDOOM_SPAWN_TRIES 8u
#define RDOOM_SPAWN_RISE 0.5f
typedef struct rdoom_spawn_entry {
  float a[3], b[3], c[3];
  float cumulative;
} rdoom_spawn_entry;
/* borrowed pointers into a rdoom_world / rdoom_worldset (valid until it is destroyed) */
typedef struct rdoom_spawn_table {
  const rdoom_spawn_entry *entries;
  uint32_t n_entries;
  float start_pos[3], start_yaw;
} rdoom_spawn_table;
typedef struct rdoom_spawn_params {
  float margin, clearance, max_step;
  uint32_t flags;
} rdoom_spawn_params;
/* The spawn table of the world's level, and of slot `slot` of a set (equal to the single world's of the same level).  Both work on
 * RDOOM_WORLD_HOST_ONLY handles. */
rdoom_status rdoom_world_spawn_table(const rdoom_world *world, rdoom_spawn_table *out);
rdoom_status rdoom_worldset_level_spawn_table(const rdoom_worldset *set, uint32_t slot, rdoom_spawn_table *out);
rdoom_status rdoom_world_spawn_players(const rdoom_world *world, rdoom_player_state *d_states, uint32_t n,
                                       const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_mask, uint64_t seed,
                                       const uint32_t *d_episode, const rdoom_spawn_params *params, uint32_t *d_tries_out,
                                       void *stream);
rdoom_status rdoom_worldset_spawn_players(const rdoom_worldset *set, rdoom_player_state *d_states, const uint32_t *d_levels,
                                          uint32_t n, const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_mask,
                                          uint64_t seed, const uint32_t *d_episode, const rdoom_spawn_params *params,
                                          uint32_t *d_tries_out, void *stream);

/* ---- explored area: a fog-of-war occupancy grid per player, kept on the device -------------------------------
 * A persistent, world-anchored grid per player: a cell is FREE once the player has had it in sight, WALL where sight ended on
 * something solid, unknown otherwise.  Sight is the seen-lines contract's 2-D fan, sampled at fixed steps; the grid is anchored to
 * the level, not to the player, so it accumulates as the player moves.  The reference project has no counterpart of this: nothing
 * here restates it.  Every float below is binary32, every operation is rounded once and none is contracted; divisions are IEEE;
 * a + b * c means round(a + round(b * c)).
 * The grid of a level at cell size `cell`, a finite binary32 > 0.  minx, maxx, minz, maxz: the exact minimum and maximum of a[0],
 * b[0] (x) and of a[1], b[1] (z) over the level's rdoom_map_line records; all four are 0 for a level without lines.
 *   cx(x) = (int32) floorf(x / cell);   ix0 = cx(minx) - 1;   gw = cx(maxx) + 1 - ix0 + 1;
 *   iz0 = cx(minz) - 1;   gh = cx(maxz) + 1 - iz0 + 1;   pitch = (gw + 31) / 32;   words = gh * pitch
 * -- the cells the lines touch and one cell of margin on each side; pitch is the 32-bit words of a grid row, words those of a plane.
 * Point (x, z) lies in cell (ix, iz) = (cx(x) - ix0, cx(z) - iz0) when x / cell and z / cell are finite and below 2^30 in magnitude
 * and 0 <= ix < gw, 0 <= iz < gh; otherwise, and whenever x or z is a NaN, it lies in no cell.  Cell (ix, iz) is bit ix % 32 of word
 * iz * pitch + ix / 32 of a plane.
 * Limits (RDOOM_BAD_ARG, "a grid over its limits"): a bound whose quotient by cell is not finite and below 2^30 in magnitude; gw or
 * gh above 8192; words above 2^20.
 * rdoom_world_area_grid / rdoom_worldset_level_area_grid: the grid of the world's level / of slot `slot`, by these formulas.
 * rdoom_world_area_words / rdoom_worldset_area_words: `words` of the world's level / the largest `words` among the set's levels (every
 * level must be within the limits).  All four work on RDOOM_WORLD_HOST_ONLY handles.
 *
 * rdoom_world_reveal_area / rdoom_worldset_reveal_area.  d_states, d_levels, d_dirs / n_rays, max_range, d_object_offsets / n_objects:
 * exactly as rdoom_world_reveal_lines takes them.  n_steps: 1 .. 4096.  d_area: n rows of 2 planes of `stride` uint32 words; plane
 * 0 (words p * 2 * stride ..) is FREE, plane 1 (words (p * 2 + 1) * stride ..) is WALL, each laid out as above for the grid of the
 * player's level; stride >= the handle's area words at this cell.
 * For player p and ray r, vel and T_r are the seen-lines contract's ("Fan", "Ray against line", "Blocking", "Seen" above): the same
 * expressions giving the same bits.  o = (pos.x, pos.z).
 *   For k = 0 .. n_steps:  t = (float)k / (float)n_steps;  when t <= T_r, the point (o.x + t * vel.x, o.z + t * vel.z) sets the FREE
 *   bit of its cell.
 *   When T_r < 1, the point (o.x + T_r * vel.x, o.z + T_r * vel.z) sets the WALL bit of its cell.
 * A point in no cell sets nothing.  Bits are only ever set, never cleared; words of a plane beyond the level's `words` and bits of a
 * grid row beyond gw are never written; the caller zeroes a row to start an episode.  A cell may carry both bits (sight ended in a
 * cell that another ray crossed): consumers read `wall`, and `free & ~wall`.
 * d_new_out (n x 2 uint32, may be NULL): d_new_out[2 p] = the FREE bits this call set in row p that were clear before,
 * d_new_out[2 p + 1] = the WALL bits likewise -- the growth of the explored area in cells.
 * The result is an OR of a set of bits that the expressions above fix, followed by a population count of the difference: the order in
 * which rays, steps and cells are visited, which lines are culled before the minimum, and how the work is cut into chunks, windows or
 * bands are an implementation's free choices and cannot change a bit.
 * A comparison with a NaN is false and a NaN lies in no cell: a player at a NaN position, or with a NaN yaw, marks nothing and counts
 * 0.  A level slot >= the set's size is seen on the device only: that player's row is untouched and its counts are 0.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_world_reveal_lines for the
 * arguments shared with it (a NULL handle, or (n > 0) NULL d_states / d_area / d_dirs / d_levels; n_rays == 0; max_range not finite or
 * not > 0; d_object_offsets with n_objects smaller than the game's objects; a handle created with RDOOM_WORLD_HOST_ONLY or living
 * on another device); a cell that is not finite or not > 0; n_steps 0 or above 4096; a grid over its limits; a stride smaller than
 * the handle's area words.  n == 0 queues nothing.
 *
 * rdoom_world_draw_area_maps / rdoom_worldset_draw_area_maps: every player's grid as an egocentric map.  view: width, height and scale
 * are read, RDOOM_MAP_ROTATE and RDOOM_MAP_TOP_DOWN honoured, any other flag is an error; half_width and marker are not read.  The
 * pixel's point q is the map contract's ("Pixel to world" above), operation for operation, so an area map registers pixel for pixel
 * with rdoom_world_draw_maps and rdoom_world_draw_sector_maps of the same view.  d_out (n x height x width bytes): the byte of a
 * pixel is free_bit | wall_bit << 1 of q's cell in row p of d_area (rows as above) -- RDOOM_AREA_UNKNOWN, RDOOM_AREA_FREE,
 * RDOOM_AREA_WALL, or 3 for a cell that carries both -- and 0 where q lies in no cell.  A level slot >= the set's size is seen on the
 * device only: that player's map is all 0.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of
 * rdoom_world_draw_sector_maps that concern what is read here (handle, view, d_states, d_levels, width, height, scale, flags,
 * host-only, the device); (n > 0) NULL d_area or d_out; n x ceil(width * height / 256) above 2^31 - 1; a bad cell, a grid over its
 * limits or a stride that is too small, as above.  n == 0 queues nothing. */
#define RDOOM_AREA_UNKNOWN 0u
#define RDOOM_AREA_FREE 1u
#define RDOOM_AREA_WALL 2u
#define RDOOM_AREA_MAX_SIDE 8192u
#define RDOOM_AREA_MAX_WORDS 1048576u
#define RDOOM_AREA_MAX_STEPS 4096u
typedef struct rdoom_area_grid {
  int32_t ix0, iz0;
  uint32_t gw, gh, pitch, words;
} rdoom_area_grid;
rdoom_status rdoom_world_area_grid(const rdoom_world *world, float cell, rdoom_area_grid *out);
rdoom_status rdoom_worldset_level_area_grid(const rdoom_worldset *set, uint32_t slot, float cell, rdoom_area_grid *out);
rdoom_status rdoom_world_area_words(const rdoom_world *world, float cell, uint32_t *words_out);
rdoom_status rdoom_worldset_area_words(const rdoom_worldset *set, float cell, uint32_t *words_out);
rdoom_status rdoom_world_reveal_area(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                                     uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects, float cell,
                                     uint32_t n_steps, uint32_t *d_area, uint32_t stride, uint32_t *d_new_out, void *stream);
rdoom_status rdoom_worldset_reveal_area(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                        uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                                        const float *d_object_offsets, uint32_t n_objects, float cell, uint32_t n_steps,
                                        uint32_t *d_area, uint32_t stride, uint32_t *d_new_out, void *stream);
rdoom_status rdoom_world_draw_area_maps(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n,
                                        const rdoom_map_view *view, const uint32_t *d_area, uint32_t stride, float cell,
                                        uint8_t *d_out, void *stream);
rdoom_status rdoom_worldset_draw_area_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                           uint32_t n, const rdoom_map_view *view, const uint32_t *d_area, uint32_t stride,
                                           float cell, uint8_t *d_out, void *stream);

/* ---- goal distance: walking distance to a goal over the whole level -------------------------------------------
 * The geodesic distance a navigation task is built on -- shaping reward, success test, shortest-path baseline -- as three pieces: the
 * level's walkability on its explored-area grid, a flood of grids of any size that can run towards its seed, and the cell a player
 * is in.  One flood per episode (or per goal) gives a field to_goal[p, iz, ix]; every later tick reads it with one gather at the
 * player's cell.  The reference project has no counterpart of this: nothing here restates it.  Every float below is binary32, every
 * operation is rounded once and none is contracted.
 *
 * rdoom_world_draw_area_planes / rdoom_worldset_draw_area_planes: the level's planes on its area grid.  n rows; d_levels (the set
 * form: n uint32 slots); d_object_offsets / n_objects exactly as rdoom_world_draw_sector_maps takes them -- row p is the game whose
 * doors and lifts count, NULL is all at rest; cell: the explored-area contract's; width, height: the extent of every row's planes,
 * each at least the gw / gh of the handle's grid at `cell` (for a set: of every level's grid) and at most RDOOM_AREA_MAX_SIDE;
 * d_area / area_stride: NULL, or the rows of rdoom_world_reveal_area; d_sector_out (uint16), d_floor_out, d_ceiling_out (float):
 * each n x height x width or NULL, at least one given.
 * Element (p * height + iz) * width + ix is cell (ix, iz) of the grid of row p's level.  For ix < gw && iz < gh of that level the
 * sample point is the cell's centre,
 *   x = ((float)(ix0 + (int32_t)ix) + 0.5f) * cell;   z = ((float)(iz0 + (int32_t)iz) + 0.5f) * cell
 * s is the sector at (x, z) as the "sectors" contract above defines it, and the three outputs are exactly what
 * rdoom_world_draw_sector_maps stores for a pixel whose point is that one: s (or RDOOM_SECTOR_NONE16), the live floor and ceiling of
 * s on row p of the offsets, +inf / -inf for none.  Every element outside the level's own gw x gh is written as none, so a flood
 * sees closed cells there; a level slot >= the set's size gives a row of none.
 * With d_area, a cell is written as none in every plane unless its FREE bit is set and its WALL bit is clear in row p (the
 * free & ~wall the explored-area contract tells consumers to read): the filled level map revealed as the player explores, the
 * analogue of d_visited in rdoom_world_draw_sector_maps.
 * This is a point sample per cell, as a map pixel is: a wall thinner than a cell can fall between two centres.  A flood of these
 * planes models walking on the grid, not the sphere-and-spring physics of rdoom_world_step_players.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle; (n > 0) NULL d_levels, or all
 * three outputs NULL; a cell the explored-area grid calls reject for this handle (not finite or not > 0, a grid over its limits);
 * width or height smaller than the grid's or above RDOOM_AREA_MAX_SIDE; n x ceil(width * height / 256) above 2^31 - 1;
 * d_object_offsets with n_objects smaller than the game's objects; d_area with area_stride below the handle's area words at `cell`;
 * a handle created with RDOOM_WORLD_HOST_ONLY or living on another device.  n == 0 queues nothing.
 *
 * rdoom_flood_grids: rdoom_flood_maps for grids of any size, from the seed or towards it.  d_floor, d_ceiling: n x height x width
 * floats each, row r, column c, a void cell +inf / -inf.
 * Open.  With f the floor and g the ceiling of a cell, the cell is open when f < +inf && f > -inf && g - f >= clearance.  A NaN makes
 * every comparison false: that cell is closed.
 * Moves.  A move from cell a to a 4-neighbour b inside the grid is allowed when both cells are open, f_b - f_a <= max_step,
 * f_a - f_b <= max_drop, and fminf(g_a, g_b) - fmaxf(f_a, f_b) >= clearance.  max_drop may be +inf.  Moves are directed: a ledge can
 * be dropped from but not climbed.
 * Seeds.  d_seeds: n x 2 int32 (column, row) in stored order; NULL: (width / 2, height / 2) for every player -- the cell at, or with
 * a corner at, the player's point of the map contract.
 * Distances.  d_dist_out (n x height x width uint32): without RDOOM_FLOOD_TOWARDS in params->flags the smallest number of allowed
 * moves from row p's seed to the cell; with it the smallest number of allowed moves from the cell to the seed -- the same move
 * relation, followed backwards from the seed.  0 at the seed; RDOOM_FLOOD_GRID_UNREACHED where there is no path, where the cell is
 * closed, and everywhere when the seed is closed or outside the grid.  d_count_out (n uint32, may be NULL): the number of cells of
 * row p with a distance below RDOOM_FLOOD_GRID_UNREACHED.
 * params: rdoom_flood_params; flags is 0 or RDOOM_FLOOD_TOWARDS, any other bit is an error.
 * Size.  width * height is at most rdoom_flood_grid_max_cells' *cells_out, a constant of the library: 2^22 (2048 x 2048); each side
 * is at most RDOOM_AREA_MAX_SIDE.
 * Property.  For a grid within rdoom_flood_max_cells and flags == 0, rdoom_flood_grids and rdoom_flood_maps give the same distances,
 * element for element, with 0xFFFF widened to 0xFFFFFFFF.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): NULL params; (n > 0) NULL d_floor /
 * d_ceiling / d_dist_out; a zero width or height; a side above RDOOM_AREA_MAX_SIDE; more cells than rdoom_flood_grid_max_cells; a
 * flag other than RDOOM_FLOOD_TOWARDS; a NaN or negative max_step, max_drop or clearance; NULL cells_out.  n == 0 queues nothing.
 *
 * rdoom_world_area_cells / rdoom_worldset_area_cells: which cell a player is in.  d_cells_out[p] is two int32 (ix, iz): the cell of
 * (pos.x, pos.z) of d_states[p] in the grid of the player's level at `cell`, by the explored-area contract's "point (x, z) lies in
 * cell"; (-1, -1) where the point lies in none -- a NaN, outside the grid, a level slot >= the set's size.  The layout is d_seeds',
 * so the output feeds rdoom_flood_grids directly, and the pair addresses the planes above.  One launch, asynchronous on `stream`;
 * nothing is allocated and nothing waits, so the call can be captured into a graph.  Errors, all checked before anything is queued
 * (RDOOM_BAD_ARG): those of rdoom_world_locate_players for the arguments shared with it (a NULL handle; (n > 0) NULL d_states /
 * d_cells_out / d_levels; a handle created with RDOOM_WORLD_HOST_ONLY or living on another device); a cell the explored-area grid
 * calls reject.  n == 0 queues nothing. */
#define RDOOM_FLOOD_GRID_UNREACHED 0xFFFFFFFFu
#define RDOOM_FLOOD_TOWARDS 1u
rdoom_status rdoom_world_draw_area_planes(const rdoom_world *world, uint32_t n, const float *d_object_offsets, uint32_t n_objects,
                                          float cell, uint32_t width, uint32_t height, const uint32_t *d_area, uint32_t area_stride,
                                          uint16_t *d_sector_out, float *d_floor_out, float *d_ceiling_out, void *stream);
rdoom_status rdoom_worldset_draw_area_planes(const rdoom_worldset *set, const uint32_t *d_levels, uint32_t n,
                                             const float *d_object_offsets, uint32_t n_objects, float cell, uint32_t width,
                                             uint32_t height, const uint32_t *d_area, uint32_t area_stride, uint16_t *d_sector_out,
                                             float *d_floor_out, float *d_ceiling_out, void *stream);
rdoom_status rdoom_flood_grid_max_cells(uint32_t *cells_out);
rdoom_status rdoom_flood_grids(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                               const int32_t *d_seeds, const rdoom_flood_params *params, uint32_t *d_dist_out, uint32_t *d_count_out,
                               void *stream);
rdoom_status rdoom_world_area_cells(const rdoom_world *world, const rdoom_player_state *d_states, uint32_t n, float cell,
                                    int32_t *d_cells_out, void *stream);
rdoom_status rdoom_worldset_area_cells(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                       uint32_t n, float cell, int32_t *d_cells_out, void *stream);

/* ---- waypoints and frontiers: a flood's distance field followed on the device -----------------------------------
 * What turns the fields of the two sections above into somewhere to walk: the walk down a field from a start -- the next waypoint
 * on a shortest path to a goal, or the way to a cell from the player -- and the frontier of a player's explored area with the cell
 * of it the field says is nearest.  Neither can be had from the distances alone, because moves are directed: a 4-neighbour whose
 * distance is one less is not necessarily a cell one may step into.  The reference project has no counterpart of this: nothing
 * here restates it.  Every float below is binary32, every operation is rounded once and none is contracted.
 *
 * rdoom_flood_descend: walk a field downhill.  A pure function of its arrays: no handle.  d_floor, d_ceiling: the planes
 * rdoom_flood_grids took, n x height x width floats each; d_dist: the n x height x width uint32 that call wrote with the same
 * `params` (flags 0 or RDOOM_FLOOD_TOWARDS, as there); D(c) is row p's word of cell c.  d_starts: n x 2 int32 (column, row), the
 * layout of d_seeds and of rdoom_world_area_cells' output.
 * The walk of row p.  Let a be the start.  If a is outside the grid or D(a) is RDOOM_FLOOD_GRID_UNREACHED, d_cells_out[p] =
 * (-1, -1), d_moves_out[p] = 0 and nothing is walked.  Otherwise m = 0, and while D(a) > stop_dist and m < max_moves: among the
 * 4-neighbours b of a inside the grid, taken in the order (column - 1, column + 1, row - 1, row + 1), the first with
 * D(b) == D(a) - 1 whose connecting move is allowed by "Open" and "Moves" of the goal-distance contract above -- with
 * RDOOM_FLOOD_TOWARDS the move from a to b, without it the move from b to a, because that field counts moves from the seed --
 * becomes a, and m += 1; if no neighbour qualifies the walk stops, which only happens when the field was not flooded from these
 * planes with these params.  At the end d_cells_out[p] = a (n x 2 int32, column then row) and d_moves_out[p] = m (n uint32).
 * Path.  d_path_out may be NULL; otherwise it is n x path_len x 2 int32: entry k of row p is the cell after move k + 1 for
 * k < min(m, path_len) and (-1, -1) for every later entry; every entry is written.
 * Uses.  With RDOOM_FLOOD_TOWARDS, max_moves = K and stop_dist = 0: the waypoint K moves ahead on a shortest path to the goal, or
 * the goal itself if it is nearer.  On a forward field, started at a frontier cell with max_moves = 0xFFFFFFFF and stop_dist = K:
 * the cell K moves from the player on a shortest path to that frontier.  The walk is a shortest path of the field's move relation;
 * among several, the one the neighbour order picks.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_flood_grids for the
 * arguments shared with it (NULL params; (n > 0) NULL d_floor / d_ceiling; a zero width or height; a side above
 * RDOOM_AREA_MAX_SIDE; more cells than rdoom_flood_grid_max_cells; a flag other than RDOOM_FLOOD_TOWARDS; a NaN or negative
 * max_step, max_drop or clearance); (n > 0) NULL d_dist / d_starts / d_cells_out / d_moves_out; d_path_out with path_len 0 or above
 * 2^22 (a walk is shorter than that: a distance is below the number of cells).  n == 0 queues nothing.
 *
 * rdoom_world_area_frontiers / rdoom_worldset_area_frontiers: the frontier of each player's explored area.  n rows; d_levels (the
 * set form: n uint32 slots); cell: the explored-area contract's; d_area / area_stride: the rows of rdoom_world_reveal_area;
 * width, height: the extent of every row of d_dist and d_mask_out, as rdoom_world_draw_area_planes and rdoom_flood_grids shape
 * them -- each at least the gw / gh of the handle's grid at `cell` (for a set: of every level's) and at most RDOOM_AREA_MAX_SIDE;
 * d_dist: n x height x width uint32, a field of rdoom_flood_grids (usually forwards from the players' cells, over the planes drawn
 * through d_area); D(ix, iz) is word (p * height + iz) * width + ix.
 * Frontier cell.  Cell (ix, iz) of row p is a frontier cell when ix < gw and iz < gh of the row's level, D(ix, iz) is not
 * RDOOM_FLOOD_GRID_UNREACHED, and at least one of its 4-neighbours inside that gw x gh has both its FREE bit and its WALL bit clear
 * in row p.  Bits of a grid row beyond gw, and cells beyond the grid, are not neighbours.
 * d_cell_out (n x 2 int32, ix then iz): the frontier cell with the smallest D, ties to the smallest iz, then the smallest ix;
 *   (-1, -1) when there is none.  The layout is d_starts', so the output feeds rdoom_flood_descend directly.
 * d_dist_out (n uint32, may be NULL): that cell's D, or RDOOM_FLOOD_GRID_UNREACHED when there is none.
 * d_count_out (n uint32, may be NULL): the number of frontier cells of row p.
 * d_mask_out (n x height x width bytes, may be NULL): 1 on frontier cells and 0 elsewhere, every byte written.
 * A level slot >= the set's size is seen on the device only: (-1, -1), RDOOM_FLOOD_GRID_UNREACHED, 0 and a mask of zeros.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_world_draw_area_planes for
 * the arguments shared with it (a NULL handle; (n > 0) NULL d_levels; a cell the explored-area grid calls reject; width or height
 * smaller than the grid's or above RDOOM_AREA_MAX_SIDE; area_stride below the handle's area words at `cell`; a handle created with
 * RDOOM_WORLD_HOST_ONLY or living on another device); (n > 0) NULL d_area / d_dist / d_cell_out; n above 2^31 - 1.  n == 0 queues
 * nothing. */
rdoom_status rdoom_flood_descend(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width,
                                 uint32_t height, const int32_t *d_starts, const rdoom_flood_params *params, uint32_t max_moves,
                                 uint32_t stop_dist, int32_t *d_cells_out, uint32_t *d_moves_out, int32_t *d_path_out,
                                 uint32_t path_len, void *stream);
rdoom_status rdoom_world_area_frontiers(const rdoom_world *world, uint32_t n, float cell, uint32_t width, uint32_t height,
                                        const uint32_t *d_area, uint32_t area_stride, const uint32_t *d_dist, int32_t *d_cell_out,
                                        uint32_t *d_dist_out, uint32_t *d_count_out, uint8_t *d_mask_out, void *stream);
rdoom_status rdoom_worldset_area_frontiers(const rdoom_worldset *set, const uint32_t *d_levels, uint32_t n, float cell,
                                           uint32_t width, uint32_t height, const uint32_t *d_area, uint32_t area_stride,
                                           const uint32_t *d_dist, int32_t *d_cell_out, uint32_t *d_dist_out, uint32_t *d_count_out,
                                           uint8_t *d_mask_out, void *stream);

/* ---- wall distance: how far the nearest wall is from every cell, and planes that keep a body's radius away from it
 * The floods above treat the walker as a point: a cell is open when its own centre has floor and headroom.  This is the one
 * primitive that gives the walker a radius: the exact squared distance, in cells, from every cell to the nearest cell that is not
 * open, up to a radius R, and the same planes with every cell too near such a cell made void.  The inflated planes go through
 * rdoom_flood_maps, rdoom_flood_grids, rdoom_flood_descend and the frontier calls as they are; the distances are an observation
 * channel, a wall-proximity penalty or a spawn margin.  The reference project has no counterpart of this: nothing here restates it.
 *
 * rdoom_wall_distance.  A pure function of its arrays: no handle.  d_floor, d_ceiling: n x height x width floats each, row r,
 * column c, a void cell +inf / -inf -- the planes of rdoom_world_draw_sector_maps or rdoom_world_draw_area_planes.
 * A cell is open by "Open" of the goal-distance contract above with params->clearance: f finite && g - f >= clearance, a NaN closes it.
 * Blocking cells of row p.  The cells of that row's grid that are not open.  Without RDOOM_WALL_EDGE_OPEN every cell position
 * outside width x height is blocking as well -- what the floods assume, and what rdoom_world_draw_area_planes stores outside a
 * level's grid.  With the flag only cells inside the grid block: the reading for rdoom_world_draw_sector_maps' window, whose edge
 * is unknown and not a wall.
 * D2.  D2(c, r) = min over blocking (c', r') of (c - c')^2 + (r - r')^2, in integers; nothing is rounded.
 * d_dist2_out (n x height x width uint16, may be NULL): D2 where D2 <= R * R with R = params->radius, RDOOM_WALL_FAR elsewhere.  A
 *   closed cell holds 0.  Every value up to R * R is exact; nothing beyond R * R is reported, so the corners of the square window
 *   the kernel looks at never leak.
 * d_floor_out, d_ceiling_out (n x height x width floats each; both NULL or both given): where D2 > params->close_d2 the input's
 *   32-bit word unchanged, a NaN's payload and the sign of a zero included; where D2 <= close_d2, +inf and -inf, the void cell of
 *   the planes' own contract.  close_d2 == 0 touches closed cells only.  At least one of the three outputs is given.
 * Model.  A body of radius r on a grid of cell size `cell` must not stand where a blocked centre lies within r of its own centre:
 * D2 <= (r / cell)^2, so close_d2 = floor((r / cell)^2) and R is the smallest integer with R * R >= close_d2.  This is a point
 * sample per cell like the rest of the grid: a wall thinner than a cell can still fall between two centres.  Ledges are not
 * inflated: blocking is a property of a cell alone, not of the floor one stands on, so a step too high to climb between two open
 * cells stays the business of the floods' move rule and is not this field's.
 * Size.  Each side is at most RDOOM_AREA_MAX_SIDE; width * height is at most rdoom_flood_grid_max_cells' *cells_out.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): NULL params; (n > 0) NULL d_floor /
 * d_ceiling; all three outputs NULL, or one of the two planes without the other; a zero width or height; a side above
 * RDOOM_AREA_MAX_SIDE; more cells than rdoom_flood_grid_max_cells; a radius of 0 or above RDOOM_WALL_MAX_RADIUS; close_d2 above
 * radius * radius; a flag other than RDOOM_WALL_EDGE_OPEN; a NaN or negative clearance; n x the 64 x 32 tiles of a grid above
 * 2^24 - 1; an output plane whose bytes overlap an input plane's -- the kernel reads neighbours, so there is no in-place form.
 * n == 0 queues nothing. */
#define RDOOM_WALL_FAR 0xFFFFu
#define RDOOM_WALL_MAX_RADIUS 32u
#define RDOOM_WALL_EDGE_OPEN 1u
typedef struct rdoom_wall_params {
  float clearance;   /* "Open" above, rdoom_flood_maps' word for word */
  uint32_t radius;   /* R, in cells: 1 .. RDOOM_WALL_MAX_RADIUS */
  uint32_t close_d2; /* cells with D2 <= close_d2 are void in the output planes; at most R * R */
  uint32_t flags;    /* 0 or RDOOM_WALL_EDGE_OPEN */
} rdoom_wall_params;
rdoom_status rdoom_wall_distance(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                 const rdoom_wall_params *params, uint16_t *d_dist2_out, float *d_floor_out, float *d_ceiling_out,
                                 void *stream);

/* ---- octile distance: grid floods over the eight neighbours, and their descent ------------------------------------
 * rdoom_flood_grids counts moves to 4-neighbours, so moves * cell is a Manhattan-style length that overstates a diagonal walk by up
 * to 41 %.  These two calls add the diagonal move: with integer costs 5 and 7 the free-space error against the Euclidean length is
 * between -1 % and +8 %, and the field stays exact integer arithmetic.  rdoom_flood_grids and rdoom_flood_descend are unchanged.
 * The reference project has no counterpart of this: nothing here restates it.
 *
 * rdoom_flood_grids_octile.  A pure function of its arrays: no handle.  d_floor, d_ceiling, n, width, height, d_seeds, d_count_out
 * and the limits max_step, max_drop and clearance of `params` are rdoom_flood_grids': the planes, which cells are open, which moves
 * to a 4-neighbour -- the axial moves -- are allowed and where the seed lies are defined by the goal-distance contract above and
 * by nothing here.
 * Diagonal moves.  Let a and d be cells inside the grid with d = (column +- 1, row +- 1) of a, and s1, s2 the two cells that are
 * 4-neighbours of both.  The diagonal move from a to d is allowed exactly when all four axial moves a -> s1, s1 -> d, a -> s2 and
 * s2 -> d are allowed; nothing else is compared.  So a diagonal never passes the corner of a closed cell, a ledge or a door, and it
 * is a pure function of the axial move bits of d, s1 and s2.  With RDOOM_FLOOD_TOWARDS the same rule applies to the reversed
 * relation.
 * Costs.  An axial move costs params->axial_cost, a diagonal move params->diagonal_cost, with
 * 1 <= axial_cost <= diagonal_cost <= 2 * axial_cost and (uint64_t)axial_cost * width * height <= 0x00FFFFFF: a cheapest path is
 * never dearer than an axial-only one of fewer than width * height moves, so a distance fits 24 bits.
 * Octile distances.  d_dist_out (n x height x width uint32): without RDOOM_FLOOD_TOWARDS in params->flags the smallest total cost
 * of a sequence of allowed moves from row p's seed to the cell; with it the smallest total cost from the cell to the seed.  The
 * seed holds 0; RDOOM_FLOOD_GRID_UNREACHED where there is no path, where the cell is closed, and everywhere when the seed is closed
 * or outside the grid.  d_count_out is as in rdoom_flood_grids.  dist * cell / axial_cost is the length in world units.
 * Properties, with D4 what rdoom_flood_grids gives for the same planes, seeds, limits and direction and D8 this call's distances:
 *   1. a cell is reached exactly when rdoom_flood_grids reaches it;
 *   2. with diagonal_cost == 2 * axial_cost, D8 == axial_cost * D4 on every reached cell;
 *   3. otherwise D8 <= axial_cost * D4;
 *   4. D8 >= axial_cost * (max(|dc|, |dr|) - min(|dc|, |dr|)) + diagonal_cost * min(|dc|, |dr|) for the cell at the offset
 *      (dc, dr) from the seed.
 *
 * rdoom_flood_descend_octile: rdoom_flood_descend's walk down an octile field.  d_dist: the words rdoom_flood_grids_octile wrote
 * with the same `params`.  The start, d_cells_out, d_moves_out, d_path_out and the unreached or outside start behave as in
 * rdoom_flood_descend.  While D(a) > stop_dist and m < max_moves: among the 8-neighbours b of a inside the grid, taken in the
 * order (column - 1, column + 1, row - 1, row + 1), then the (column, row) offsets (-1, -1), (+1, -1), (-1, +1), (+1, +1), the first
 * with D(b) + cost == D(a) -- cost the axial or the diagonal one of that move, the sum taken in integers, so an unreached b never
 * qualifies -- whose connecting move is allowed, with RDOOM_FLOOD_TOWARDS the move from a to b, without it the move from b to a, a
 * diagonal's by the rule above, becomes a, and m += 1; if no neighbour qualifies the walk stops.  stop_dist is in cost units;
 * max_moves and d_moves_out count moves.
 *
 * Frontiers.  rdoom_world_area_frontiers and rdoom_worldset_area_frontiers take an octile field as d_dist as they are: they then
 * pick the frontier cell nearest by octile cost, and d_dist_out is that cost.
 * Both calls are one launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so
 * they can be captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_flood_grids
 * and rdoom_flood_descend for the arguments shared with them; an axial_cost of 0; a diagonal_cost below axial_cost or above
 * 2 * axial_cost; axial_cost * width * height above 0x00FFFFFF.  n == 0 queues nothing. */
typedef struct rdoom_flood_octile_params {
  float max_step, max_drop, clearance;   /* rdoom_flood_params' */
  uint32_t flags;                        /* 0 or RDOOM_FLOOD_TOWARDS */
  uint32_t axial_cost, diagonal_cost;    /* cost units of a move to a 4-neighbour / to a diagonal neighbour */
} rdoom_flood_octile_params;             /* 24 bytes */
rdoom_status rdoom_flood_grids_octile(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                      const int32_t *d_seeds, const rdoom_flood_octile_params *params, uint32_t *d_dist_out,
                                      uint32_t *d_count_out, void *stream);
rdoom_status rdoom_flood_descend_octile(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width,
                                        uint32_t height, const int32_t *d_starts, const rdoom_flood_octile_params *params,
                                        uint32_t max_moves, uint32_t stop_dist, int32_t *d_cells_out, uint32_t *d_moves_out,
                                        int32_t *d_path_out, uint32_t path_len, void *stream);

/* ---- straight walks: the line-of-walk test and string-pulled paths -------------------------------------------------
 * "Can I walk straight from here to there?" -- asked of a goal, a waypoint, a frontier cell or another player's cell under the open
 * and move rules the floods use -- and the heading that makes of a descent's staircase of 4- or 8-neighbour moves: the farthest
 * cell of the path that can be walked to in a straight line.  Both rest on one primitive, the chain of grid moves that the straight
 * segment between two cell centres makes, defined in exact integers.  No existing call changes.  The reference project has no
 * counterpart of this: nothing here restates it.
 *
 * The line chain.  Cells are (column, row).  For a = (ca, ra) and b = (cb, rb) inside the grid: dx = |cb - ca|, dy = |rb - ra|, and
 * sx, sy are the signs of cb - ca and rb - ra.  The segment between the two centres crosses dx column boundaries and dy row
 * boundaries; column crossing i (0 <= i < dx) is at parameter (2i + 1) / (2 dx), row crossing j (0 <= j < dy) at
 * (2j + 1) / (2 dy).  The chain starts at a with i = j = 0 and runs while i < dx or j < dy:
 *   if j == dy, or i < dx and (2i + 1) * dy < (2j + 1) * dx: a column move to (c + sx, r), then i += 1;
 *   else if i == dx, or (2i + 1) * dy > (2j + 1) * dx: a row move to (c, r + sy), then j += 1;
 *   else the segment passes exactly through a cell corner: a diagonal move to (c + sx, r + sy), then i += 1 and j += 1.
 * Every product is an integer below 2^28.  Nothing is rounded.  The chain ends at b.
 * Allowed.  A column or row move from x to y is allowed by "Open" and "Moves" of the goal-distance contract above, with max_step,
 * max_drop and clearance.  A diagonal move is allowed by the octile contract's rule: all four axial moves round both sides must be
 * allowed.  So a line never cuts the corner of a closed cell, a ledge or a door.
 * Direction.  Without the reversed flag, each move of the chain is tested in the chain's direction, x to y.  With the flag, each
 * move is tested y to x, and a diagonal's four axial moves are reversed likewise: the walk from b back to a over the same cells.
 * Result of a line.  The line is clear when a and b are inside the grid, a is open, and every move of the chain is allowed.  A
 * zero-move line (a == b) is clear exactly when a is open.  `stop` is the last cell reached from a: b when clear, else the cell the
 * first refused move starts from -- a itself when a is closed.  `stop` is (-1, -1) when a or b is outside the grid.
 * Property.  The chain from b to a is the chain from a to b, reversed.
 *
 * rdoom_grid_walk_lines.  A pure function of its arrays: no handle.  d_floor, d_ceiling, n, width, height: rdoom_flood_grids' planes.
 * d_from: n x 2 int32, in the layout of d_seeds and of rdoom_world_area_cells' output; d_to: n x n_to x 2 int32.  Line (p, k) runs
 * from d_from[p] to d_to[p][k] on row p's planes.  params: rdoom_flood_params' limits; flags is 0 or RDOOM_LINE_REVERSED, any other
 * bit is an error.  d_clear_out: n x n_to bytes, 1 for clear and 0 otherwise, every byte written.  d_stop_out: n x n_to x 2 int32
 * (column, row), may be NULL.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_flood_grids for the
 * arguments shared with it; (n > 0) NULL d_from / d_to / d_clear_out; n_to == 0; n * n_to above 2^31 - 1.  n == 0 queues nothing.
 *
 * rdoom_path_straighten.  d_starts: n x 2 int32.  d_path: n x path_len x 2 int32, what rdoom_flood_descend or
 * rdoom_flood_descend_octile wrote, or any list of cells.  params->flags is the descent's: with RDOOM_FLOOD_TOWARDS the lines are
 * tested in the listed direction; without it they are tested reversed, because a forward field's path is listed from the far end
 * back to the player.
 * Row p.  m is the index of the first entry of the row that is not a cell inside the grid, or path_len if there is none.  If the
 * start is outside the grid: count 0 and length 0.  Otherwise a = start, i = 0, count = 0, length = +0.0f, and while i < m and
 * count < corner_len: K = min(max_look, m - i); k* is the largest k in [0, K) whose line from a to path[i + k] is clear -- if
 * there is none the loop ends; the corner is path[i + k*], stored as entry `count`;
 * length += sqrtf((float)(dc * dc + dr * dr)) with dc and dr the offsets from a to the corner -- the integer converted once, the
 * square root IEEE, one rounded add, no contraction; then a = corner, i += k* + 1, count += 1.
 * Outputs.  d_corners_out: n x corner_len x 2 int32; every later entry is (-1, -1), and every entry is written.
 * d_count_out[p] = count (n uint32).  d_length_out (n floats, may be NULL): the length in cells; length * cell is world units.
 * Entry 0 is the any-angle waypoint.
 * Limits.  1 <= max_look <= RDOOM_STRAIGHTEN_MAX_LOOK; 1 <= path_len <= 2^22; 1 <= corner_len <= 2^22.  i strictly grows, so the
 * loop ends.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): those of rdoom_flood_grids for the
 * arguments shared with it; (n > 0) NULL d_starts / d_path / d_corners_out / d_count_out; a max_look, path_len or corner_len
 * outside its limits.  n == 0 queues nothing. */
#define RDOOM_LINE_REVERSED 1u
#define RDOOM_STRAIGHTEN_MAX_LOOK 1024u
rdoom_status rdoom_grid_walk_lines(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                   const int32_t *d_from, const int32_t *d_to, uint32_t n_to, const rdoom_flood_params *params,
                                   uint8_t *d_clear_out, int32_t *d_stop_out, void *stream);
rdoom_status rdoom_path_straighten(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                   const int32_t *d_starts, const int32_t *d_path, uint32_t path_len, const rdoom_flood_params *params,
                                   uint32_t max_look, int32_t *d_corners_out, uint32_t corner_len, uint32_t *d_count_out,
                                   float *d_length_out, void *stream);

/* ---- things: what each player sees, touches and collects of a level's things -----------------------------------
 * The thing table.  One 32-byte record per THINGS entry, in lump order, for the entries LevelWalker::things sends down its decor
 * branch (wad/src/visitor.rs:1010-1026): sector_at finds a sector for the entry, and its type is none of the marker types 1, 2, 3,
 * 4, 11, 14.  An entry has its record whether or not the metadata knows its type and whether or not its sprite lump exists: an item
 * is somewhere even when it cannot be drawn.
 *   x, z: from_wad_coords of the entry, the low[0] and low[2] of the rdoom_decor of the same thing.
 *   base: from_wad_height of its sector's floor; of its ceiling when the metadata says hanging.
 *   radius: (float)metadata radius / 100.0f; 0 without metadata.
 *   object_id: the sector's floor_id (hanging: ceiling_id) as rdoom_map_sector carries it; 0: nothing moves it.
 *   sector: its index in rdoom_world_map_sectors' table.
 *   thing_type, flags, angle: WadThing's fields, verbatim (the angle's 16 bits as they stand in the lump).
 *   category: in the low byte the array of [things] the metadata read the type from, in the order they are merged (first match),
 *   RDOOM_THING_UNKNOWN without metadata; RDOOM_THING_HANGING or-ed in when the metadata says hanging.
 * The live height of a thing in player p's game is base + off(object_id), off() the map contract's on row p of d_object_offsets: a
 * candle on a lift rides it. */
#define RDOOM_THING_DECORATION 0u
#define RDOOM_THING_WEAPON 1u
#define RDOOM_THING_POWERUP 2u
#define RDOOM_THING_ARTIFACT 3u
#define RDOOM_THING_AMMO 4u
#define RDOOM_THING_KEY 5u
#define RDOOM_THING_MONSTER 6u
#define RDOOM_THING_UNKNOWN 7u
#define RDOOM_THING_HANGING 0x100u
typedef struct rdoom_thing {
  float x, z;
  float base;
  float radius;
  uint32_t object_id;
  uint32_t sector;
  uint16_t thing_type, flags;
  uint16_t category;
  uint16_t angle;
} rdoom_thing;
/* borrowed pointers into a rdoom_world / rdoom_worldset (valid until it is destroyed) */
typedef struct rdoom_map_things {
  const rdoom_thing *things;
  uint32_t n_things;
} rdoom_map_things;
/* The thing table of the world's level, and of slot `slot` of a set (equal to the single world's of the same level).  Both work on
 * RDOOM_WORLD_HOST_ONLY handles. */
rdoom_status rdoom_world_map_things(const rdoom_world *world, rdoom_map_things *out);
rdoom_status rdoom_worldset_level_map_things(const rdoom_worldset *set, uint32_t slot, rdoom_map_things *out);

/* A rdoom_thingset holds the thing tables of n_levels levels on the current device: things[l] points at counts[l] records, a
 * level's own table or any other -- a consumer may scatter items of its own per run.  A level may hold 0 things (things[l] may
 * then be NULL).  rdoom_thingset_info: the levels, *out_words = max(1, ceil(largest count / 32)), the stride every row of thing
 * bits needs at least, and the largest object_id of any record.  Every out pointer of it may be NULL.
 * Errors of create (RDOOM_BAD_ARG): n_levels == 0; NULL things, counts or out; a NULL table with a non-zero count; a count above
 * 2^20; a category whose low byte is above 7, or with bits other than RDOOM_THING_HANGING above it; an x, z, base or radius that
 * is not finite; a negative radius. */
typedef struct rdoom_thingset rdoom_thingset;
rdoom_status rdoom_thingset_create(const rdoom_thing *const *things, const uint32_t *counts, uint32_t n_levels, rdoom_thingset **out);
void rdoom_thingset_destroy(rdoom_thingset *set);
rdoom_status rdoom_thingset_info(const rdoom_thingset *set, uint32_t *out_n_levels, uint32_t *out_words, uint32_t *out_max_object_id);

/* Sensing: which things each of n players sees and touches, the nearest visible thing of every category, and what it collects, in
 * one launch.  params: max_range finite and > 0; cos_half_fov finite, <= -1 means no field-of-view test; touch_radius finite and
 * >= 0, the body's (0.19 is the player step's); touch_below and touch_above >= 0, +inf allowed: the vertical window; collect_mask:
 * bit c set means a touched thing of category c is collected; flags: 0.
 * Every float below is binary32, every operation is rounded once and none is contracted; divisions and the square root are IEEE;
 * a * b + c * d means round(round(a * b) + round(c * d)).
 * Player p, in level L with T things (a world: its one level; a set: slot d_levels[p], level L of `things`).  (s, c) = the
 * project's sincos of the player's yaw (csrc/hip/sincos_rd.hpp); r = (c, -s) and f = (-s, -c) are the map contract's right and
 * forward; o = (pos.x, pos.z).
 * Thing i < T is examined when its bit -- bit i % 32 of word p * stride + i / 32 -- is clear in d_collected as it stood when the
 * call began (a NULL d_collected: nothing is collected).  For an examined thing:
 *   dx = x - pos.x;  dz = z - pos.z;  d2 = dx * dx + dz * dz;  y = base + off(object_id);  dy = pos.y - y,
 * off() the map contract's on row p of d_object_offsets.
 * Touched: d2 <= tr * tr with tr = touch_radius + radius, and dy >= -touch_below, and dy <= touch_above.
 * In range: d2 <= max_range * max_range.
 * In the field of view: cos_half_fov <= -1, or dx * f.x + dz * f.z >= cos_half_fov * sqrtf(d2).
 * Visible: in range, in the field of view, and T_r == 1, T_r the seen-lines contract's for the ray o + t * vel with vel = (dx, dz):
 * its "Ray against line" and "Blocking" word for word, over the line table of the player's level.  So a shut door hides a thing in
 * the game of the player who has not opened it, and only there; and a thing exactly on a blocking line is visible, because a hit at
 * t == 1 leaves T_r at 1.
 * A comparison with a NaN is false: a player at a NaN position sees and touches nothing.  A thing that is not examined is neither
 * visible nor touched, and cannot be nearest.
 * Outputs; every one may be NULL, but not all five.  Bit rows are rows of `stride` uint32 words, stride >= the set's words.
 *   d_visible_out, d_touched_out: words [0, ceil(T / 32)) of row p are written whole, bit i % 32 of word i / 32 set for a visible /
 *   touched thing i and the bits at and above T zero.  No word beyond them is written.
 *   d_collected: the bits of the touched things whose category bit (1 << the category's low byte) is in collect_mask are OR-ed in,
 *   after everything above was evaluated: a thing collected by this call is still reported by this call and is gone in the next.
 *   Bits are never cleared; words beyond ceil(T / 32) are never written; the caller zeroes a row to start an episode.
 *   d_new_out[p * 8 + c] (n x 8 uint32): how many things of category c this call collected for p.  All eight are written.
 *   d_nearest_out[p * 8 + c] (n x 8 rdoom_thing_nearest): the visible thing of category c with the smallest d2, the lowest index
 *   among equals: index, d2, right = dx * r.x + dz * r.z, forward = dx * f.x + dz * f.z.  Where there is none: {-1, +inf, 0, 0}.
 * A level slot >= the set's size is seen on the device only: that player's bit rows are untouched, its nearest records are "none"
 * and its counts are 0.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  Errors, all checked before anything is queued (RDOOM_BAD_ARG): a NULL handle, thing set or params, or
 * (n > 0) NULL d_states / d_levels; all five outputs NULL; a stride smaller than the set's words while d_collected, d_visible_out
 * or d_touched_out is given; a thing set whose levels are not as many as the handle's (a world: not 1) or that lives on another
 * device; n_objects smaller than the game's objects (as for rdoom_world_draw_maps), or not above the set's largest object_id, while
 * d_object_offsets is given; params outside the domains above; flags not 0; a handle created with RDOOM_WORLD_HOST_ONLY or living
 * on another device.  n == 0 queues nothing. */
typedef struct rdoom_thing_sense {
  float max_range;
  float cos_half_fov;
  float touch_radius;
  float touch_below, touch_above;
  uint32_t collect_mask;
  uint32_t flags;
} rdoom_thing_sense;
typedef struct rdoom_thing_nearest {
  int32_t index;
  float d2, right, forward;
} rdoom_thing_nearest;
rdoom_status rdoom_world_sense_things(const rdoom_world *world, const rdoom_thingset *things, const rdoom_player_state *d_states,
                                      uint32_t n, const float *d_object_offsets, uint32_t n_objects, const rdoom_thing_sense *params,
                                      uint32_t *d_collected, uint32_t *d_visible_out, uint32_t *d_touched_out, uint32_t stride,
                                      rdoom_thing_nearest *d_nearest_out, uint32_t *d_new_out, void *stream);
rdoom_status rdoom_worldset_sense_things(const rdoom_worldset *set, const rdoom_thingset *things, const rdoom_player_state *d_states,
                                         const uint32_t *d_levels, uint32_t n, const float *d_object_offsets, uint32_t n_objects,
                                         const rdoom_thing_sense *params, uint32_t *d_collected, uint32_t *d_visible_out,
                                         uint32_t *d_touched_out, uint32_t stride, rdoom_thing_nearest *d_nearest_out,
                                         uint32_t *d_new_out, void *stream);

/* ---- hidden things: a collected thing leaves its player's frames ------------------------------------------------------------
 * The reference draws every decoration of a level in every frame (game/src/level.rs:764-793 builds them once; nothing is ever
 * picked up).  Here a batch may take one row of thing bits per pose -- rdoom_world_sense_things' d_collected as it stands -- and
 * the cull kernel drops the decor triangles of the things whose bit is set, for that pose only.  Every later stage reads only
 * what survives the cull, so the frames, the depth, label and primitive planes and the observations all lose the thing, and the
 * primitive ids of everything else stay what they are.
 *
 * rdoom_level_set_decor_things attaches, to level `slot` of the handle (0 for rdoom_level_create), the thing of every decor quad:
 * thing_of_quad[q] for the quad of decor vertices 4q .. 4q + 3 of that level's descriptor, n_quads == n_decor_verts / 4
 * (rdoom_built_decor_things' array for a built level).  An entry of RDOOM_NO_THING means "never hidden".  Several quads may name
 * one thing.  Synchronous; called before any batch on the level renders with hidden rows; calling again replaces the slot's table.
 * This is the one change a rdoom_level admits after create.  The handle keeps 4 bytes per triangle of the set on the device from
 * the first call on.  Errors (RDOOM_BAD_ARG): a NULL level, or a NULL thing_of_quad with n_quads > 0; a slot outside the set;
 * n_quads != n_decor_verts / 4; a decor triangle of the slot whose three indices do not lie in one quad. */
#define RDOOM_NO_THING 0xFFFFFFFFu
rdoom_status rdoom_level_set_decor_things(rdoom_level *level, uint32_t slot, const uint32_t *thing_of_quad, uint32_t n_quads);
/* Rows for every following render of the batch, by any of rdoom_batch_render, _timed, _profiled, _objects, _levels, _players and
 * _players_clocked: d_hidden is a borrowed device pointer, 4-byte aligned, to rows of `stride` uint32 words, laid out as
 * d_collected above; row p belongs to pose or player p.  A decor triangle of thing i of pose p's level is not drawn for pose p
 * when bit i % 32 of word p * stride + i / 32 is set.  A triangle whose thing is RDOOM_NO_THING or >= 32 * stride is drawn, and a
 * bit no decor quad of the pose's level maps to has no effect.  The rows are read on the render's stream when the render runs
 * (words [0, stride) of rows [0, n_poses), never written): a sense call queued before the render on the same stream is seen
 * without a host wait.  d_hidden == NULL switches it off (stride is ignored).  The call itself queues nothing.
 * Errors (RDOOM_BAD_ARG): a NULL batch; with a non-NULL d_hidden: stride == 0, a pointer that is not 4-byte aligned, or a level of
 * the batch's handle that has decor triangles and no attached table. */
rdoom_status rdoom_batch_set_hidden_things(rdoom_batch *batch, const uint32_t *d_hidden, uint32_t stride);

/* ---- thing maps: each player's thing marks on the automap grid ----------------------------------------------
 * The things of a rdoom_thingset drawn as discs on the pixels of rdoom_world_draw_maps, per player and in the player's own game:
 * a thing the player has collected is gone from its map and only from its map, and optionally only the things the player has
 * already seen are drawn.  The call needs no world handle: the thing set knows its levels, the player state gives the position and
 * the yaw, and things do not move in xz.  The reference has no automap and no counterpart.
 * n players' maps in one launch, asynchronous on `stream` (a hipStream_t, may be NULL); every pointer but `things`, `view` and
 * `marks` is device memory, nothing is allocated, nothing is copied to the host and nothing waits, so the call can be captured into
 * a graph.
 * Every float below is binary32, every operation is rounded once and none is contracted; a * b + c * d means
 * round(round(a * b) + round(c * d)).
 * Pixel to world.  The map contract's ("top-down maps"), word for word: the byte at row `row`, column i of map p is pixel (i, j)
 * with j = row, or j = height - 1 - row with RDOOM_MAP_TOP_DOWN; hw = (float)width * 0.5f, hh = (float)height * 0.5f;
 *   u = (((float)i + 0.5f) - hw) * scale;  v = (((float)j + 0.5f) - hh) * scale;
 * without RDOOM_MAP_ROTATE q = (pos.x - v, pos.z - u); with it, (s, c) = the project's sincos of yaw (csrc/hip/sincos_rd.hpp):
 * q.x = (pos.x + c * u) + (-s) * v;  q.z = (pos.z + (-s) * u) + (-c) * v.  Of `view` the call reads width, height, scale and those
 * two flags; half_width, marker, RDOOM_MAP_SHOW_FLAT and RDOOM_MAP_SHOW_HIDDEN are not read, so the view of a draw_maps call can
 * be passed as it is.
 * Which things are drawn.  Player p is in level L = d_levels[p] of the set (a NULL d_levels: every player in slot 0), which has T
 * things.  Thing i < T is drawn when codes[category & 0xFF] != 0, and its bit is clear in row p of d_hidden (a NULL d_hidden hides
 * nothing; it is rdoom_world_sense_things' d_collected as it stands), and its bit is set in row p of d_known (a NULL d_known: every
 * thing is known; a caller keeps it by OR-ing sense_things' d_visible_out into it).  Bit i is bit i % 32 of word
 * p * stride + i / 32, as in "things"; only words [0, ceil(T / 32)) of a row are read, and none is written.
 * Coverage.  For a drawn thing: rp = min_radius * scale; r = radius > rp ? radius : rp; r2 = r * r.  The thing covers q when
 *   ex = q.x - x;  ez = q.z - z;  ex * ex + ez * ez <= r2.
 * A radius so large that r * r overflows to +inf covers every pixel whose q is a number.
 * Pixel value.  Each covering thing has the key (code << 20) | (0xFFFFF - i), code = codes[category & 0xFF]; T <= 2^20, so the
 * key's low 20 bits hold 0xFFFFF - i.  The pixel takes the largest key: the larger code wins, and among equal codes the lower
 * index.  d_out gets the key's code, d_index_out its i.  Where nothing covers, d_out is 0 and d_index_out is -1.  The value is a
 * maximum, so it does not depend on the order in which things are visited, on a thing being visited twice or on where a list of
 * things is cut -- the reason "top-down maps" gives for its own rule.
 * Outputs.  d_out: n x height x width bytes; d_index_out: n x height x width int32; map p at element p * height * width, row-major.
 * Either may be NULL, but not both.  Without RDOOM_THING_MARKS_OVER every byte of d_out is written; with it only the covered bytes
 * are, and every other byte is left as it was: a call after rdoom_world_draw_maps on the same buffer overlays the marks on the line
 * map (the default codes lie above every RDOOM_MAP_* class).  d_index_out is always written whole.
 * A comparison with a NaN is false: a player at a NaN position gets no mark.  A level slot >= the set's levels is seen on the
 * device only: that player gets no mark.
 * Errors, all RDOOM_BAD_ARG and all checked before anything is queued, in this order.  What needs no set: a NULL view or marks;
 * (n > 0) a NULL d_states; both outputs NULL; width or height 0 or above 16384; scale not finite or not > 0; view flags other than
 * the four RDOOM_MAP_* flags; min_radius not finite or < 0; marks->flags other than RDOOM_THING_MARKS_OVER; n x the view's 32 x 32
 * pixel tiles above 2^31 - 1.  Then: a NULL set; a set that lives on another device than the current one; a NULL d_levels while the
 * set has more than one level; a stride smaller than the set's words while d_hidden or d_known is given.  n == 0 queues nothing. */
#define RDOOM_MAP_THING 16u            /* default code of category c: RDOOM_MAP_THING + c, clear of the RDOOM_MAP_* line classes */
#define RDOOM_THING_MARKS_OVER 1u      /* d_out is written only where a mark covers; every other byte is left as it was */
typedef struct rdoom_thing_marks {
  float min_radius;                    /* pixels; finite, >= 0: a mark is never drawn smaller than this */
  uint8_t codes[8];                    /* the byte of a thing of category c; 0: that category is not drawn */
  uint32_t flags;                      /* RDOOM_THING_MARKS_OVER or 0 */
} rdoom_thing_marks;
rdoom_status rdoom_thingset_draw_maps(const rdoom_thingset *things, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                      uint32_t n, const rdoom_map_view *view, const rdoom_thing_marks *marks,
                                      const uint32_t *d_hidden, const uint32_t *d_known, uint32_t stride,
                                      uint8_t *d_out, int32_t *d_index_out, void *stream);

/* ---- solid things: which things of a level are obstacles ----------------------------------------------------
 * The reference has no thing collision at all (its player walks through every barrel), so nothing here restates it: this header is
 * the authority, as it is for the explored area and for the things.
 * The metadata may give a [[things.*]] entry the optional boolean `obstacle` (absent: false).  The two calls below lend the level's
 * obstacle bits (borrowed pointers, valid until the handle is destroyed), in the layout every row of thing bits has: bit i % 32 of
 * word i / 32 is set when the metadata entry that gave thing i of rdoom_world_map_things its category -- the first match in merge
 * order -- says obstacle = true; a thing without metadata has a clear bit.  *out_n_words = max(1, ceil(T / 32)) for the level's T
 * things, and the bits at and above T are zero.  rdoom_thing stays as it is: solidity travels in bit rows.  Both work on
 * RDOOM_WORLD_HOST_ONLY handles.  Errors (RDOOM_BAD_ARG): a NULL argument; a slot outside the set.
 * rdoom_world_stamp_things below reads these bits on the device; the player step does not see things (DESIGN section 31 has the
 * contract of the step that will, and why it is not here). */
rdoom_status rdoom_world_thing_obstacles(const rdoom_world *world, const uint32_t **out_words, uint32_t *out_n_words);
rdoom_status rdoom_worldset_level_thing_obstacles(const rdoom_worldset *set, uint32_t slot, const uint32_t **out_words,
                                                  uint32_t *out_n_words);

/* ---- solid things on the grid: a level's obstacles stamped into the area planes -------------------------------
 * The planes of rdoom_world_draw_area_planes with the cells a solid thing stands on made void, per row and in the row's own game,
 * so that rdoom_flood_grids, rdoom_flood_grids_octile, rdoom_wall_distance, rdoom_flood_descend*, rdoom_grid_walk_lines,
 * rdoom_path_straighten and rdoom_world_area_frontiers route round them.  The reference has no counterpart: this header is the
 * authority.  Every float below is binary32, every operation is rounded once and none is contracted.
 * rdoom_world_stamp_things / rdoom_worldset_stamp_things.  n rows.  Row p is level L: the world's one level, or slot d_levels[p]
 * of the set and level L of `things` (the relation of handle and thing set is rdoom_world_sense_things'); L has T things.  cell,
 * width, height: as rdoom_world_draw_area_planes takes them, and the extents are checked as it checks them.  d_floor, d_ceiling:
 * n x height x width floats each, the planes of rdoom_world_draw_area_planes at this cell (or any planes of that layout).  The grid
 * (ix0, iz0, gw, gh) of L is the explored-area contract's.  Cell (ix, iz) with ix < gw and iz < gh has the centre
 *   xc = ((float)(ix0 + (int32_t)ix) + 0.5f) * cell;   zc = ((float)(iz0 + (int32_t)iz) + 0.5f) * cell
 * -- rdoom_world_draw_area_planes' own expression.
 * Candidates.  Thing i < T is a candidate for row p when its bit is set in row L of d_solid (levels x stride words, the bits of
 * rdoom_world_thing_obstacles; NULL: every thing is solid) and clear in row p of d_hidden (n x stride words, rdoom_world_sense_things'
 * d_collected as it stands; NULL: nothing is hidden).  Bit i is bit i % 32 of word row * stride + i / 32; only words
 * [0, ceil(T / 32)) of a row are read, and none is written.
 * Coverage.  A candidate covers a cell when either holds: with r = radius + grow, ex = xc - x, ez = zc - z,
 *   ex * ex + ez * ez <= r * r;
 * or the cell is the thing's own, the one the point (x, z) lies in by the explored-area contract ("Point (x, z) lies in cell"); a
 * point that lies in no cell has none.  So a solid thing always closes the cell it stands in, however coarse the grid.  An r * r
 * that overflows to +inf covers every cell.
 * Blocking.  A covering candidate blocks the cell when dy = f - (base + off(object_id)) satisfies dy >= -block_below and
 * dy <= block_above: f is the cell's input floor, off() the map contract's on row p of d_object_offsets (NULL: at rest).  Both bounds
 * are >= 0 and may be +inf: then there is no vertical test for any floor that is a number.  A comparison with a NaN is false: a cell
 * whose floor is a NaN is never blocked.
 * Outputs.  d_floor_out and d_ceiling_out (n x height x width floats; both or neither): +inf / -inf where some thing blocks the
 * cell, elsewhere the input's 32-bit word untouched, NaN payloads and -0 included.  d_index_out (n x height x width int32, may be
 * NULL): the lowest blocking i, -1 where nothing blocks.  At least one of the planes or the index is given.  Being blocked is an OR
 * and the index a minimum: neither depends on the order things are visited in, on culling or on how the work is cut.  Elements
 * outside the level's own gw x gh, and rows whose slot is >= the set's size (seen on the device only), are passed through, index -1.
 * In place.  A cell's output depends on its own input only: d_floor_out == d_floor together with d_ceiling_out == d_ceiling is
 * allowed.  Any other overlap of an output's bytes (n x height x width x 4 each) with an input's or another output's is an error.
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied to the host and nothing waits, so the call can be
 * captured into a graph.  n == 0 queues nothing.
 * Errors, all RDOOM_BAD_ARG and all checked before anything is queued, in this order.  What needs no handle: NULL params; grow,
 * block_below or block_above a NaN or negative, or grow not finite; flags not 0; no output at all, or one plane without the other;
 * (n > 0) a NULL d_floor or d_ceiling; the overlap rule; a zero side; a side above RDOOM_AREA_MAX_SIDE.  Then what reads the handle:
 * a NULL handle; one created with RDOOM_WORLD_HOST_ONLY or living on another device; a cell the explored-area grid calls reject
 * (not finite or not > 0, a grid over its limits); width or height below the grid's; (n > 0) NULL d_levels; n x the planes' 64 x 16
 * cell tiles above 2^31 - 1.  Then what reads the thing set: a NULL set; a set whose levels are not as many as the handle's or that
 * lives on another device; a stride smaller than the set's words while d_solid or d_hidden is given; n_objects smaller than the
 * game's objects, or not above the set's largest object_id, while d_object_offsets is given. */
typedef struct rdoom_stamp_params {
  float grow;                          /* finite, >= 0: added to every radius (0.19, the body's, stamps inflated obstacles) */
  float block_below, block_above;      /* >= 0, +inf allowed: how far the floor may lie below / above the thing's live height */
  uint32_t flags;                      /* 0 */
} rdoom_stamp_params;
rdoom_status rdoom_world_stamp_things(const rdoom_world *world, const rdoom_thingset *things, uint32_t n, const float *d_object_offsets,
                                      uint32_t n_objects, float cell, uint32_t width, uint32_t height, const uint32_t *d_solid,
                                      const uint32_t *d_hidden, uint32_t stride, const rdoom_stamp_params *params, const float *d_floor,
                                      const float *d_ceiling, float *d_floor_out, float *d_ceiling_out, int32_t *d_index_out,
                                      void *stream);
rdoom_status rdoom_worldset_stamp_things(const rdoom_worldset *set, const rdoom_thingset *things, const uint32_t *d_levels, uint32_t n,
                                         const float *d_object_offsets, uint32_t n_objects, float cell, uint32_t width, uint32_t height,
                                         const uint32_t *d_solid, const uint32_t *d_hidden, uint32_t stride,
                                         const rdoom_stamp_params *params, const float *d_floor, const float *d_ceiling,
                                         float *d_floor_out, float *d_ceiling_out, int32_t *d_index_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RDOOM_H */
