// C ABI of the device renderer (include/rdoom.h "device renderer"): level upload, batch scratch, and
// rdoom_batch_render = setup -> bin -> raster -> fragment -> fixup on the caller's stream.
//
// Replaces the reference's GL draw path: VertexBuffer / IndexBuffer / Texture2d uploads (engine/src/meshes.rs:126-201,
// engine/src/uniforms.rs:146-221) and the frame.draw loop of Renderer::update (engine/src/renderer.rs:98-157).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "kernels.hpp"
#include "rdoom_frame_things.h"

#pragma clang fp contract(off)

using namespace rdoom_dev;
using rdoom::DeviceArray;
using rdoom::PinnedArray;

namespace {
bool is_pow2(uint32_t x) { return x != 0 && (x & (x - 1)) == 0; }
}  // namespace

// A resident SET of levels (rdoom_levelset_create); rdoom_level_create makes a set of one.
struct rdoom_level {
  int device = 0;
  DeviceLevelView view{};  // its pointers are views of the arrays below
  DeviceArray<LevelTri> d_tris;
  DeviceArray<Cluster> d_clusters;
  DeviceArray<uint16_t> d_texels, d_sky;
  DeviceArray<uint8_t> d_cmap;
  DeviceArray<LevelSlice> d_slices;
  std::vector<LevelSlice> slices;      // host copy of the slice table
  uint32_t ntri = 0;        // the LARGEST level's triangle count: a pose's records and visible list have this stride
  uint32_t n_objects = 1;   // 1 + the largest object id any level of the set draws
  // PLAYPAL 0 of every level, 256 words R | G << 8 | B << 16 | 0xFF << 24 per level: read by the resolve kernels only (they take it
  // as an argument of their own, so no struct another kernel takes by value carries it)
  DeviceArray<uint32_t> d_palettes;
  std::vector<uint8_t> has_palette;  // the level's desc had a playpal (else its poses cannot be resolved to RGB)
  // Hidden things (rdoom_level_set_decor_things): per level, its descriptor's decor vertex count and, per triangle, the decor
  // quad its three indices lie in (idx / 4) -- NONE for a triangle of another kind, QUAD_SPANS for a decor triangle whose indices
  // lie in two quads.  d_tri_thing: one word per triangle of the set (view.tri_thing), allocated by the first attach.
  static constexpr uint32_t QUAD_SPANS = 0xFFFFFFFEu;
  std::vector<uint32_t> n_decor_verts;
  std::vector<std::vector<uint32_t>> tri_quad;
  std::vector<uint8_t> has_decor, things_attached;
  DeviceArray<uint32_t> d_tri_thing;
};

// The members that own something are declared in the reverse of the order they must be released in -- pinned staging, the copy
// stream, the events, the device buffers -- so that the destructor frees the device buffers FIRST: a batch destroyed while its last
// render is still in flight relies on that first release waiting for the device, before an event or the staging a queued copy reads
// goes away.  The raw pointers are views or borrowed, each says of what.
struct rdoom_batch {
  const rdoom_level *level = nullptr;  // borrowed: the caller keeps the level alive for as long as the batch
  uint32_t width = 0, height = 0, max_poses = 0, cap = 0, last_n = 0;
  // Row pitch, in pixels, of the visibility words, primitive ids and framebuffers: the width itself when it is a multiple of 4
  // (every size the kernels were written for), else the next multiple of 8 -- the reference takes any --resolution WxH
  // (src/main.rs:41).  The frame's geometry (viewport, bounding boxes, sky ndc) uses `width`; the padding columns are never
  // covered (S6 clamps every bounding box to the frame) and never read back.
  uint32_t pitch = 0;
  uint32_t entry_cap = 0, n_tiles = 0;
  uint32_t fix_cap = 1u << 20;
  bool frag_const_ready = false;
  uint32_t stage = 0;
  uint32_t ring_n = 0, ring_poses = 0;
  bool want_prim = false;
  bool vis16 = false;  // record indices fit 16 bits: visibility words are u16
  // the last render's FragmentPlan::skip_described_vis: a described quadrant's visibility words are another render's (resolve reads the table)
  bool last_skip_vis = false;
  // the last render's census of the rasteriser (hook raster_stats; else zeros): its masked bodies [0..3], settle_kernel's pairs it expanded [4], its own pairs [5]
  uint64_t last_raster_census[RASTER_CENSUS] = {};
  bool last_frag_count = false;  // the last render's FragmentPlan::count: the fragment kernel counted its half lanes and listed quads
  size_t rgb_bytes = 0;          // of d_rgb
  // the last render was rdoom_batch_render_players: its levels are on the device only (the pinned staging is an older render's)
  bool last_levels_on_device = false;
  // rdoom_batch_set_hidden_things: the caller's rows of thing bits (borrowed), read by the cull kernel of every render; null: none
  const uint32_t *d_hidden = nullptr;
  uint32_t hidden_stride = 0;

  // ---- released last: pinned host memory ----
  // Pinned staging for the per-pose constants, TWO deep: a render waits for the H2D copy of the render before the previous
  // one, not for the previous one's -- with one buffer the host could not queue a render before the stream had reached the last
  // render's copy, and a host thread that feeds several batches on several streams stalled on each in turn (the 1/8 share of
  // BASELINE config 4, nine levels x small batches, ran SLOWER on two streams than on one).
  static constexpr uint32_t STAGES = 2;
  PinnedArray<ObjectConst> h_objects[STAGES];  // max_poses x n_objects, allocated on first use
  PinnedArray<PoseConst> h_poses[STAGES];
  // ---- then the copy stream ----
  // The end of the last render on ITS stream (ev_done), and a stream of the batch's own for read-backs: rdoom_batch_finish and the
  // rdoom_batch_read_* wait for this batch's work only, never for the device -- another host thread's render on another
  // stream (one host thread per GPU or stream) does not delay them.
  rdoom::Stream copy_stream;
  // ---- then the events ----
  rdoom::Event ev_done;
  rdoom::Event ev_copy[STAGES];  // H2D of h_poses[i] finished: that staging buffer may be rewritten
  static constexpr uint32_t RING = 64;  // renders whose per-kernel events may be pending (rdoom_batch_render_profiled)
  rdoom::Event ring[RING][4];           // created on first use
  rdoom::Event ev[4];
  // ---- released first: device memory ----
  DeviceArray<PoseConst> d_poses;
  DeviceArray<TriRec> d_recs;        // max_poses x cap records in near-to-far order (setup -> bin, raster, fragment)
  DeviceArray<uint32_t> d_visible;   // max_poses x cap: the visible triangles of each pose (cull kernel -> set-up kernel)
  DeviceArray<uint2> d_tile_hdr;     // per (pose, tile): (first entry, entry count)
  DeviceArray<uint32_t> d_entries;   // per pose: entry_cap tile-list entries (record index | quadrant mask << 28)
  DeviceArray<uint2> d_hits;         // per pose: entry_cap (entry, tile) pairs: the binning kernel's count pass -> its fill pass
  DeviceArray<uint32_t> d_overflow;  // per pose: 1 = bins incomplete, rasteriser scans the sorted list
  // The words every render starts from zero -- d_fix_count (4), d_counts (max_poses), d_ghist (2048 per pose) -- are ONE
  // allocation, d_zeroed, cleared by one hipMemsetAsync: four separate fills per render were four more packets between the
  // kernels of a stream (the 1/8 share of config 4 queues 9 x 13 packets per step for a few hundred microseconds of work each).
  DeviceArray<uint32_t> d_zeroed;
  // views into d_zeroed:
  uint32_t *d_fix_count = nullptr;  // [0] = queued pixels, [1] = error flag (fixup list overflow), [2] = error flag (the set-up kernel
                                    // disagreed with the cull kernel about a triangle: the counting sort's buckets would not add up),
                                    // [3] = rdoom_batch_render_players' level error word (level_error)
  uint32_t *d_counts = nullptr;
  uint32_t *d_ghist = nullptr;  // counting sort of the set-up: per pose, one counter per depth bucket
  DeviceArray<uint2> d_fix_list;
  DeviceArray<uint32_t> d_vis;       // (u16 words when vis16)
  DeviceArray<uint8_t> d_fb;
  DeviceArray<uint8_t> d_frag_const;  // the fragment kernel's rarely read constants (fragment.hip: FragConst), written on first use
  DeviceArray<uint2> d_qpair;    // per (pose, tile, quadrant): the pair settle_kernel proved where the table says so (raster.hip: QTAB_PAIR); never cleared
  DeviceArray<uint32_t> d_qtab;  // per (pose, tile, quadrant): the record every pixel of the quadrant shows, or NONE (rasteriser -> fragment kernel)
  DeviceArray<float> d_ndc;  // (ix + 0.5) / (width / 2) - 1 for every column, then (iy + 0.5) / (height / 2) - 1 for every row
  DeviceArray<uint32_t> d_prim;        // allocated by rdoom_batch_enable_primitive_ids
  DeviceArray<ObjectConst> d_objects;  // max_poses x n_objects, allocated on first use
  DeviceArray<uint8_t> d_rgb;  // rdoom_batch_read_rgb's staging (allocated on first use, at most RGB_STAGING_BYTES or one frame)
};

// Every entry point that touches a batch's memory or waits for its work first makes the level's device current: a host
// thread that drives several GPUs (or read another batch in between) would otherwise synchronise / copy on the wrong one.
static hipError_t bind_device(const rdoom_batch *b) { return hipSetDevice(b->level->device); }

// What only the device finds out about a render: read after a synchronisation, reported as a status.
// Device -> host over the batch's own stream, after the batch's last render (and nothing else) has finished.  rows > 1: a
// strided source (pitch_bytes between rows), tightly packed at the destination.
static hipError_t read_back(const rdoom_batch *b, void *dst, const void *src, size_t row_bytes, size_t rows = 1, size_t pitch_bytes = 0) {
  hipError_t e = hipStreamWaitEvent(b->copy_stream.get(), b->ev_done.get(), 0);  // (an event never recorded counts as complete)
  if (e != hipSuccess) return e;
  if (rows <= 1 || pitch_bytes == row_bytes)
    e = hipMemcpyAsync(dst, src, row_bytes * (rows ? rows : 1), hipMemcpyDeviceToHost, b->copy_stream.get());
  else
    e = hipMemcpy2DAsync(dst, row_bytes, src, pitch_bytes, row_bytes, rows, hipMemcpyDeviceToHost, b->copy_stream.get());
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(b->copy_stream.get());
}

// fix[3] is rdoom_batch_render_players' error word: ~p for the first pose p whose level lay outside the set (0: none)
static rdoom_status level_error(const rdoom_batch *b, uint32_t word) {
  if (!word) return RDOOM_OK;
  return rdoom::fail(RDOOM_BAD_ARG, "pose %u of the last render names a level outside the set of %u (rendered as level 0)", ~word,
                     b->level->view.n_slices);
}

static rdoom_status device_flags(const rdoom_batch *b, uint32_t *out_fixups = nullptr) {
  uint32_t fix[4] = {0, 0, 0, 0};
  HIP_TRY(read_back(b, fix, b->d_fix_count, sizeof fix));
  if (out_fixups) *out_fixups = fix[0];
  if (fix[1]) return rdoom::fail(RDOOM_BAD_LEVEL, "alpha-leak fixup list overflow (%u pixels)", fix[0]);
  if (fix[2]) return rdoom::fail(RDOOM_HIP_ERROR, "internal: set-up and cull kernels disagree about a triangle (build flags changed?)");
  return level_error(b, fix[3]);
}

extern "C" {

rdoom_status rdoom_device_count(int32_t *out_count) {
  if (!out_count) return rdoom::fail(RDOOM_BAD_ARG, "out_count is null");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  *out_count = n;
  return RDOOM_OK;
}

rdoom_status rdoom_set_device(int32_t device) {
  HIP_TRY(hipSetDevice(device));
  return RDOOM_OK;
}

void rdoom_level_destroy(rdoom_level *level) { delete level; }

// One level of a set, flattened on the host: what rdoom_levelset_create concatenates and uploads.
namespace {
struct HostLevel {
  std::vector<LevelTri> tris;
  std::vector<Cluster> clusters;     // Cluster::first relative to this level's first triangle
  std::vector<uint16_t> texels;      // wall atlas, then (at multiples of 1024) the flat atlas promoted to u16, the decor atlas
  size_t flat_base = 0, decor_base = 0;
  std::vector<uint16_t> sky;
  LevelSlice dims{};                 // the atlas / sky sizes (bases and ranges are filled in when the set is assembled)
  uint32_t n_objects = 1;
  std::vector<uint32_t> tri_quad;    // per triangle: rdoom_level::tri_quad's entry
  uint32_t n_decor_verts = 0;
};
}  // namespace

static rdoom_status flatten_level(const rdoom_level_desc *d, HostLevel &out);
static rdoom_status levelset_create_impl(const rdoom_level_desc *const *descs, uint32_t n_levels, rdoom_level **out_level);

rdoom_status rdoom_levelset_create(const rdoom_level_desc *const *descs, uint32_t n_levels, rdoom_level **out_level) {
  return rdoom::guarded([&] { return levelset_create_impl(descs, n_levels, out_level); });  // (std::vector / std::map may throw)
}

rdoom_status rdoom_level_create(const rdoom_level_desc *d, rdoom_level **out_level) {
  return rdoom_levelset_create(&d, 1u, out_level);
}

static rdoom_status flatten_level(const rdoom_level_desc *d, HostLevel &out) {
  if (!d) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (!d->colormap) return rdoom::fail(RDOOM_BAD_ARG, "colormap is null");
  if ((d->flat_atlas && !(d->flat_w && d->flat_h)) || (d->wall_atlas && !(d->wall_w && d->wall_h)) ||
      (d->decor_atlas && !(d->decor_w && d->decor_h)))
    return rdoom::fail(RDOOM_BAD_ARG, "an atlas pointer is set but its size is zero");
  if ((d->flat_w | d->flat_h) && !(is_pow2(d->flat_w) && is_pow2(d->flat_h)))
    return rdoom::fail(RDOOM_BAD_ARG, "flat atlas %ux%u is not a power of two", d->flat_w, d->flat_h);
  if ((d->wall_w | d->wall_h) && !(is_pow2(d->wall_w) && is_pow2(d->wall_h)))
    return rdoom::fail(RDOOM_BAD_ARG, "wall atlas %ux%u is not a power of two", d->wall_w, d->wall_h);
  if ((d->decor_w | d->decor_h) && !(is_pow2(d->decor_w) && is_pow2(d->decor_h)))
    return rdoom::fail(RDOOM_BAD_ARG, "decor atlas %ux%u is not a power of two", d->decor_w, d->decor_h);
  if (d->flat_w > 32768 || d->flat_h > 32768 || d->wall_w > 32768 || d->wall_h > 32768 || d->decor_w > 32768 ||
      d->decor_h > 32768)
    return rdoom::fail(RDOOM_BAD_ARG, "atlas larger than 32768 texels on a side");
  // flatten the draws into one primitive list in draw order (primitive id == position)
  std::vector<LevelTri> &tris = out.tris;
  uint32_t n_objects = 1;
  // Alpha-test classification of a wall texture (all its animation frames): bit 0 = a texel in the
  // one-texel ring AROUND the rectangle is transparent (the float mod of F2 can land there), bit 1 =
  // the rectangle itself contains transparent texels (a genuinely masked texture).
  std::map<std::tuple<float, float, float, float, uint32_t, float>, uint32_t> masked_cache;
  auto region_masked = [&](const rdoom_static_vertex &v) -> uint32_t {
    auto key = std::make_tuple(v.a_atlas_uv[0], v.a_atlas_uv[1], v.a_tile_size[0], v.a_tile_size[1],
                               (uint32_t)v.a_num_frames, v.a_row_height);
    auto it = masked_cache.find(key);
    if (it != masked_cache.end()) return it->second;
    uint32_t m = 0;
    const double W = d->wall_w, au = v.a_atlas_uv[0], av = v.a_atlas_uv[1], sx = v.a_tile_size[0],
                 sy = v.a_tile_size[1];
    const uint32_t nf = v.a_num_frames == 0 ? 1u : v.a_num_frames;
    for (uint32_t f = 0; f < nf; f++) {
      double u0 = au + f * sx;
      double rows = std::ceil((u0 + sx) / W) - 1.0;
      if (nf == 1) rows = 0;
      const double md = sx > 0 ? (W - au) - sx * std::floor((W - au) / sx) : 0;
      u0 += md * rows;
      const double v0 = av + rows * v.a_row_height;
      const long xlo = (long)std::floor(u0), xhi = (long)std::ceil(u0 + sx), ylo = (long)std::floor(v0),
                 yhi = (long)std::ceil(v0 + sy);  // interior = [xlo, xhi) x [ylo, yhi)
      for (long y = ylo - 1; y <= yhi; y++)
        for (long x = xlo - 1; x <= xhi; x++) {
          const uint32_t xx = (uint32_t)x & (d->wall_w - 1), yy = (uint32_t)y & (d->wall_h - 1);
          if (d->wall_atlas[(size_t)yy * d->wall_w + xx] & 0x8000u)
            m |= (x >= xlo && x < xhi && y >= ylo && y < yhi) ? 2u : 1u;
        }
    }
    masked_cache[key] = m;
    return m;
  };
  for (uint32_t di = 0; di < d->n_draws; di++) {
    const rdoom_draw &dr = d->draws[di];
    if (dr.index_count % 3 != 0) return rdoom::fail(RDOOM_BAD_ARG, "draw %u: index_count not a multiple of 3", di);
    if (dr.object_id >= 4096u) return rdoom::fail(RDOOM_BAD_LEVEL, "draw %u: object id %u (at most 4095)", di, dr.object_id);
    n_objects = std::max(n_objects, dr.object_id + 1u);
    for (uint32_t t = 0; t < dr.index_count / 3; t++) {
      LevelTri lt;
      std::memset(&lt, 0, sizeof lt);
      lt.packed = 1u | (dr.kind << 16);
      uint32_t quad = NONE;  // of a decor triangle: the quad its indices lie in
      if (dr.kind == RDOOM_KIND_FLAT || dr.kind == RDOOM_KIND_WALL) {
        if ((uint64_t)dr.first_index + dr.index_count > d->n_static_indices)
          return rdoom::fail(RDOOM_BAD_ARG, "draw %u: static index range out of bounds", di);
        const rdoom_static_vertex *vv[3];
        for (int i = 0; i < 3; i++) {
          const uint32_t idx = d->static_indices[dr.first_index + 3 * t + i];
          if (idx >= d->n_static_verts) return rdoom::fail(RDOOM_BAD_ARG, "draw %u: vertex index out of bounds", di);
          vv[i] = &d->static_verts[idx];
          std::memcpy(&lt.pos[3 * i], vv[i]->a_pos, 12);
          lt.uv[2 * i] = vv[i]->a_tile_uv[0];
          lt.uv[2 * i + 1] = vv[i]->a_tile_uv[1];
          lt.scroll[i] = vv[i]->a_scroll_rate;
        }
        const rdoom_static_vertex &pv = *vv[2];  // flat varyings: provoking (last) vertex
        lt.atlas_u = pv.a_atlas_uv[0];
        lt.atlas_v = pv.a_atlas_uv[1];
        lt.size_x = pv.a_tile_size[0];
        lt.size_y = pv.a_tile_size[1];
        lt.row_height = pv.a_row_height;
        uint32_t masked = 0;
        if (dr.kind == RDOOM_KIND_WALL) {
          if (!d->wall_atlas) return rdoom::fail(RDOOM_BAD_ARG, "wall draw without a wall atlas");
          masked = region_masked(pv);
        } else if (!d->flat_atlas) {
          return rdoom::fail(RDOOM_BAD_ARG, "flat draw without a flat atlas");
        }
        lt.packed = (uint32_t)pv.a_num_frames | ((uint32_t)pv.a_light << 8) | (dr.kind << 16) |
                    (masked << 18);
      } else if (dr.kind == RDOOM_KIND_SKY) {
        if (!d->sky_texture || !d->sky_w || !d->sky_h) return rdoom::fail(RDOOM_BAD_ARG, "sky draw without a sky texture");
        if ((uint64_t)dr.first_index + dr.index_count > d->n_sky_indices)
          return rdoom::fail(RDOOM_BAD_ARG, "draw %u: sky index range out of bounds", di);
        for (int i = 0; i < 3; i++) {
          const uint32_t idx = d->sky_indices[dr.first_index + 3 * t + i];
          if (idx >= d->n_sky_verts) return rdoom::fail(RDOOM_BAD_ARG, "draw %u: sky vertex out of bounds", di);
          std::memcpy(&lt.pos[3 * i], &d->sky_verts[3 * idx], 12);
        }
      } else if (dr.kind == RDOOM_KIND_DECOR) {
        if ((uint64_t)dr.first_index + dr.index_count > d->n_decor_indices)
          return rdoom::fail(RDOOM_BAD_ARG, "draw %u: decor index range out of bounds", di);
        if (!d->decor_atlas) return rdoom::fail(RDOOM_BAD_ARG, "decor draw without a decor atlas");
        const rdoom_sprite_vertex *vv[3];
        for (int i = 0; i < 3; i++) {
          const uint32_t idx = d->decor_indices[dr.first_index + 3 * t + i];
          if (idx >= d->n_decor_verts) return rdoom::fail(RDOOM_BAD_ARG, "draw %u: decor vertex out of bounds", di);
          quad = i == 0 || quad == idx / 4u ? idx / 4u : rdoom_level::QUAD_SPANS;
          vv[i] = &d->decor_verts[idx];
          std::memcpy(&lt.pos[3 * i], vv[i]->a_pos, 12);
          lt.uv[2 * i] = vv[i]->a_tile_uv[0];
          lt.uv[2 * i + 1] = vv[i]->a_tile_uv[1];
          lt.scroll[i] = vv[i]->a_local_x;  // decor triangles carry a_local_x here (sprite.vert:41-42)
        }
        const rdoom_sprite_vertex &pv = *vv[2];
        lt.atlas_u = pv.a_atlas_uv[0];
        lt.atlas_v = pv.a_atlas_uv[1];
        lt.size_x = pv.a_tile_size[0];
        lt.size_y = pv.a_tile_size[1];
        lt.row_height = pv.a_tile_size[1];  // sprite.vert:37 advances animation rows by the tile height
        // sprites are alpha tested per pixel (sprite.frag:20): always the exact path of the rasteriser
        lt.packed = (uint32_t)pv.a_num_frames | ((uint32_t)pv.a_light << 8) | (dr.kind << 16) | (3u << 18);
      } else {
        return rdoom::fail(RDOOM_BAD_ARG, "draw %u: unknown kind %u", di, dr.kind);
      }
      lt.packed |= dr.object_id << 20;
      tris.push_back(lt);
      out.tri_quad.push_back(quad);
    }
  }
  if (tris.size() >= (1u << 24)) return rdoom::fail(RDOOM_BAD_LEVEL, "too many triangles (%zu)", tris.size());
  out.n_objects = n_objects;
  out.n_decor_verts = d->n_decor_verts;
  // clusters for the set-up kernel's coarse cull: runs of at most CLUSTER_TRIS consecutive triangles of one object
  std::vector<Cluster> &clusters = out.clusters;
  for (size_t t = 0; t < tris.size();) {
    const uint32_t obj = tris[t].packed >> 20;
    const bool decor = ((tris[t].packed >> 16) & 3u) == RDOOM_KIND_DECOR;
    Cluster c;
    for (int k = 0; k < 3; k++) c.lo[k] = INFINITY, c.hi[k] = -INFINITY;
    c.first = (uint32_t)t;
    uint32_t n = 0;
    while (t < tris.size() && n < CLUSTER_TRIS && (tris[t].packed >> 20) == obj &&
           (((tris[t].packed >> 16) & 3u) == RDOOM_KIND_DECOR) == decor) {
      for (int v = 0; v < 3; v++)
        for (int k = 0; k < 3; k++) {
          c.lo[k] = std::min(c.lo[k], tris[t].pos[3 * v + k]);
          c.hi[k] = std::max(c.hi[k], tris[t].pos[3 * v + k]);
        }
      t++, n++;
    }
    c.count_object = n | (obj << 8) | (decor ? 0x80000000u : 0u);
    clusters.push_back(c);
  }
  // this level's u16 texels: wall atlas, then (at a multiple of 1024 elements) the flat atlas promoted to u16, the decor atlas
  const size_t wall_n = d->wall_atlas ? (size_t)d->wall_w * d->wall_h : 0;
  const size_t flat_n = d->flat_atlas ? (size_t)d->flat_w * d->flat_h : 0;
  const size_t decor_n = d->decor_atlas ? (size_t)d->decor_w * d->decor_h : 0;
  out.flat_base = (wall_n + 1023) / 1024 * 1024;
  out.decor_base = (out.flat_base + flat_n + 1023) / 1024 * 1024;
  out.texels.assign((out.decor_base + decor_n + 1023) / 1024 * 1024, 0);
  if (wall_n) std::memcpy(out.texels.data(), d->wall_atlas, wall_n * 2);
  for (size_t i = 0; i < flat_n; i++) out.texels[out.flat_base + i] = d->flat_atlas[i];
  if (decor_n) std::memcpy(out.texels.data() + out.decor_base, d->decor_atlas, decor_n * 2);
  if (d->sky_texture && d->sky_w && d->sky_h) out.sky.assign(d->sky_texture, d->sky_texture + (size_t)d->sky_w * d->sky_h);
  out.dims.wall_w = d->wall_w, out.dims.wall_h = d->wall_h;
  out.dims.flat_w = d->flat_w, out.dims.flat_h = d->flat_h;
  out.dims.decor_w = d->decor_atlas ? d->decor_w : 0, out.dims.decor_h = d->decor_atlas ? d->decor_h : 0;
  out.dims.sky_w = out.sky.empty() ? 0 : d->sky_w, out.dims.sky_h = out.sky.empty() ? 0 : d->sky_h;
  out.dims.sky_band = d->sky_tiled_band_size;
  return RDOOM_OK;
}

static rdoom_status levelset_create_impl(const rdoom_level_desc *const *descs, uint32_t n_levels, rdoom_level **out_level) {
  if (!descs || !out_level) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out_level = nullptr;
  if (n_levels == 0 || n_levels > 4096u) return rdoom::fail(RDOOM_BAD_ARG, "n_levels %u outside 1..4096", n_levels);
  std::vector<HostLevel> host(n_levels);
  for (uint32_t k = 0; k < n_levels; k++) {
    if (!descs[k]) return rdoom::fail(RDOOM_BAD_ARG, "level %u: null descriptor", k);
    if (rdoom_status rs = flatten_level(descs[k], host[k])) return rs;
    // the fragment kernel stages ONE COLORMAP in LDS per workgroup: the levels of a set come from one IWAD
    // (build_palette_texture reads the archive's COLORMAP lump, wad/src/tex.rs:137-166)
    if (k && std::memcmp(descs[k]->colormap, descs[0]->colormap, 32 * 256) != 0)
      return rdoom::fail(RDOOM_BAD_ARG, "level %u: its COLORMAP differs from level 0's (the levels of a set share one)", k);
  }
  auto lv = std::make_unique<rdoom_level>();
  (void)hipGetDevice(&lv->device);
  // the set's arrays: triangles, clusters, texels, skies, level after level
  std::vector<LevelTri> tris;
  std::vector<Cluster> clusters;
  std::vector<uint16_t> texels, sky;
  lv->slices.resize(n_levels);
  uint32_t max_clusters = 0;
  for (uint32_t k = 0; k < n_levels; k++) {
    HostLevel &h = host[k];
    // a record addresses the store with (base >> 10) in 16 bits (ShadeRec::flags), a cluster index fits 32 bits: checked on the
    // running totals, before a base below is narrowed to 32 bits and before the set's copy grows by this level
    if (texels.size() + h.texels.size() >= ((size_t)1 << 26))
      return rdoom::fail(RDOOM_BAD_LEVEL, "atlases too large (%zu texels in the set; at most 2^26)", texels.size() + h.texels.size());
    if (tris.size() + h.tris.size() >= ((size_t)1 << 31)) return rdoom::fail(RDOOM_BAD_LEVEL, "too many triangles in the set");
    LevelSlice &sl = lv->slices[k];
    sl = h.dims;
    sl.first_tri = (uint32_t)tris.size(), sl.ntri = (uint32_t)h.tris.size();
    sl.first_cluster = (uint32_t)clusters.size(), sl.n_clusters = (uint32_t)h.clusters.size();
    sl.wall_base = (uint32_t)texels.size();
    sl.flat_base = (uint32_t)(texels.size() + h.flat_base), sl.decor_base = (uint32_t)(texels.size() + h.decor_base);
    sl.sky_base = (uint32_t)sky.size();
    for (Cluster c : h.clusters) {
      c.first += sl.first_tri;
      clusters.push_back(c);
    }
    tris.insert(tris.end(), h.tris.begin(), h.tris.end());
    texels.insert(texels.end(), h.texels.begin(), h.texels.end());
    sky.insert(sky.end(), h.sky.begin(), h.sky.end());
    lv->ntri = std::max(lv->ntri, sl.ntri);
    lv->n_objects = std::max(lv->n_objects, h.n_objects);
    max_clusters = std::max(max_clusters, sl.n_clusters);
    lv->n_decor_verts.push_back(h.n_decor_verts);
    lv->has_decor.push_back(std::any_of(h.tri_quad.begin(), h.tri_quad.end(), [](uint32_t q) { return q != NONE; }) ? 1 : 0);
    lv->things_attached.push_back(0);
    lv->tri_quad.push_back(std::move(h.tri_quad));
    h = HostLevel{};  // (released: a set of many levels would otherwise hold every atlas twice)
  }
  texels.push_back(0);  // never empty; the fragment kernel's 32-bit load at the last texel's 2-byte-aligned address reads one past it
  texels.push_back(0);
  // PLAYPAL 0 of each level (no rule that they match: a level without one is created as before and cannot be resolved)
  std::vector<uint32_t> pal((size_t)n_levels * 256u, 0u);
  lv->has_palette.assign(n_levels, 0);
  for (uint32_t k = 0; k < n_levels; k++) {
    const uint8_t *pp = descs[k]->playpal;
    if (!pp) continue;
    lv->has_palette[k] = 1;
    for (uint32_t i = 0; i < 256u; i++)
      pal[(size_t)k * 256u + i] = (uint32_t)pp[3 * i] | ((uint32_t)pp[3 * i + 1] << 8) | ((uint32_t)pp[3 * i + 2] << 16) | 0xFF000000u;
  }
  // (an empty array stays a null pointer: a set without a sky has no sky texels)
  if (rdoom_status rs = lv->d_tris.upload(tris)) return rs;
  if (rdoom_status rs = lv->d_clusters.upload(clusters)) return rs;
  if (rdoom_status rs = lv->d_texels.upload(texels)) return rs;
  if (rdoom_status rs = lv->d_sky.upload(sky)) return rs;
  if (rdoom_status rs = lv->d_cmap.upload(descs[0]->colormap, 32 * 256)) return rs;
  if (rdoom_status rs = lv->d_slices.upload(lv->slices)) return rs;
  if (rdoom_status rs = lv->d_palettes.upload(pal)) return rs;
  lv->view.tris = lv->d_tris.get();
  lv->view.clusters = lv->d_clusters.get();
  lv->view.texels = lv->d_texels.get();
  lv->view.sky_texels = lv->d_sky.get();
  lv->view.colormap = lv->d_cmap.get();
  lv->view.slices = lv->d_slices.get();
  lv->view.n_slices = n_levels;
  lv->view.max_clusters = max_clusters;
  lv->view.max_ntri = lv->ntri;
  *out_level = lv.release();
  return RDOOM_OK;
}

void rdoom_batch_destroy(rdoom_batch *b) { delete b; }

static rdoom_status batch_create_impl(const rdoom_level *level, uint32_t width, uint32_t height, uint32_t max_poses, rdoom_batch **out_batch) {
  HIP_TRY(hipSetDevice(level->device));  // the batch lives on the level's device, whatever the caller's current one is
  auto b = std::make_unique<rdoom_batch>();
  b->level = level;
  b->width = width;
  b->height = height;
  b->pitch = std::max(8u, width % 4u == 0u ? width : ((width + 7u) & ~7u));
  b->max_poses = max_poses;
  b->cap = level->ntri ? level->ntri : 1;
  const rdoom::DebugOptions &dbg = rdoom::debug_options();
  b->vis16 = b->cap < 0xFFFFu && !dbg.vis32;
  const size_t npx = (size_t)b->pitch * height * max_poses;
  if (rdoom_status rs = b->d_poses.alloc(max_poses)) return rs;
  if (rdoom_status rs = b->d_recs.alloc((size_t)b->cap * max_poses)) return rs;
  if (rdoom_status rs = b->d_visible.alloc((size_t)b->cap * max_poses)) return rs;
  b->n_tiles = ((width + TILE_W - 1) / TILE_W) * ((height + TILE_H - 1) / TILE_H);
  // tile-list entries per pose; beyond it the pose is rasterised from its sorted list (slow: every tile scans every visible
  // triangle).  A long tile's list is stored per quadrant (bin.hip), an entry once per quadrant it touches, so the array is
  // sized generously -- never beyond what the level could ever need: every triangle in every quadrant of every tile
  // (the floor scales with the frame: 256 entries per tile, at least 16 384 -- 131 072 for the 510 tiles of 1080p as before,
  // 16 384 instead of 131 072 for the 20 tiles of 320 x 200, whose 8 192-pose batches had 12.9 GB of binning scratch)
  // -- and with the level: a split list stores an entry once per quadrant it touches, so a large level at a small frame (the 10x
  // level, 36 k triangles, at 320 x 200) needs more than 16 384 per pose or every such pose silently takes the overflow path)
  const uint64_t floor_entries = std::max<uint64_t>(std::max<uint64_t>(16384u, 256u * (uint64_t)b->n_tiles), std::min<uint64_t>(2u * (uint64_t)b->cap, 1u << 20));
  b->entry_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(floor_entries, 64u * (uint64_t)b->n_tiles),
                                              (uint64_t)b->cap * b->n_tiles * 4u + 8u * (uint64_t)b->n_tiles);
  b->entry_cap = (b->entry_cap + 3u) & ~3u;
  if (dbg.entry_cap > 0) b->entry_cap = (uint32_t)dbg.entry_cap;  // tests: force that fallback
  if (rdoom_status rs = b->d_tile_hdr.alloc((size_t)b->n_tiles * max_poses)) return rs;
  if (rdoom_status rs = b->d_entries.alloc((size_t)b->entry_cap * max_poses)) return rs;
  if (rdoom_status rs = b->d_hits.alloc((size_t)b->entry_cap * max_poses)) return rs;
  if (rdoom_status rs = b->d_overflow.alloc(max_poses)) return rs;
  const size_t counts_words = ((size_t)max_poses + 3u) & ~(size_t)3u;
  if (rdoom_status rs = b->d_zeroed.alloc_bytes(sizeof(uint32_t) * (4u + counts_words) + setup_histogram_bytes(max_poses))) return rs;
  b->d_fix_count = b->d_zeroed.get(), b->d_counts = b->d_fix_count + 4, b->d_ghist = b->d_counts + counts_words;
  if (rdoom_status rs = b->d_fix_list.alloc(b->fix_cap)) return rs;
  if (rdoom_status rs = b->d_vis.alloc_bytes((b->vis16 ? sizeof(uint16_t) : sizeof(uint32_t)) * npx)) return rs;
  if (rdoom_status rs = b->d_fb.alloc(npx)) return rs;
  if (rdoom_status rs = b->d_frag_const.alloc(fragment_const_bytes())) return rs;
  if (rdoom_status rs = b->d_qtab.alloc(4u * (size_t)b->n_tiles * max_poses)) return rs;
  if (rdoom_status rs = b->d_qpair.alloc(4u * (size_t)b->n_tiles * max_poses)) return rs;
  // (the rasteriser never writes the entries of quadrants that lie outside the frame: NONE from the start, so that the
  // table is self-consistent for every reader)
  HIP_TRY(hipMemset(b->d_qtab.get(), 0xFF, sizeof(uint32_t) * 4u * (size_t)b->n_tiles * max_poses));
  {  // sky.frag:13's ndc per column / row, same two operations as the per-pixel form
    // (a run of sky that ends in the padding columns of a padded row pitch reads up to 7 values past the columns: row values, or
    // the zeros the table is extended by -- colours of pixels nobody reads)
    std::vector<float> ndc(std::max(width + height, b->pitch), 0.0f);
    for (uint32_t i = 0; i < width; i++) ndc[i] = ((float)i + 0.5f) / (0.5f * (float)width) - 1.0f;
    for (uint32_t i = 0; i < height; i++) ndc[width + i] = ((float)i + 0.5f) / (0.5f * (float)height) - 1.0f;
    if (rdoom_status rs = b->d_ndc.upload(ndc)) return rs;
  }
  for (rdoom::Event &ev : b->ev)
    if (rdoom_status rs = ev.create()) return rs;
  for (rdoom::Event &ev : b->ev_copy)
    if (rdoom_status rs = ev.create()) return rs;
  if (rdoom_status rs = b->ev_done.create()) return rs;
  if (rdoom_status rs = b->copy_stream.create(hipStreamNonBlocking)) return rs;
  for (PinnedArray<PoseConst> &h : b->h_poses)
    if (rdoom_status rs = h.alloc(max_poses)) return rs;
  *out_batch = b.release();
  return RDOOM_OK;
}

rdoom_status rdoom_batch_create(const rdoom_level *level, uint32_t width, uint32_t height, uint32_t max_poses,
                                rdoom_batch **out_batch) {
  if (!level || !out_batch) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out_batch = nullptr;
  if (width == 0 || height == 0 || max_poses == 0 || width > 16384 || height > 16384)
    return rdoom::fail(RDOOM_BAD_ARG, "bad frame size %ux%u (1..16384 on a side) or max_poses %u", width, height, max_poses);
  return rdoom::guarded([&] { return batch_create_impl(level, width, height, max_poses, out_batch); });
}

static void mat_mul_v1(const float *P, const float *M, float *pm) {  // V1: PM = P * M, plain multiply/add, left to right
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++)
      pm[c * 4 + r] = ((P[0 * 4 + r] * M[c * 4 + 0] + P[1 * 4 + r] * M[c * 4 + 1]) + P[2 * 4 + r] * M[c * 4 + 2]) +
                      P[3 * 4 + r] * M[c * 4 + 3];
}

// Records ev_done on every way out of render_impl once kernels may have been queued: rdoom_batch_finish and the read functions
// wait for THAT event, and a render that failed half-way must not leave them waiting for the render before it while its
// own kernels still write the batch's scratch.
namespace {
struct DoneGuard {
  rdoom_batch *b;
  hipStream_t st;
  bool armed = false;
  ~DoneGuard() {
    if (armed) (void)hipEventRecord(b->ev_done.get(), st);
  }
};
}  // namespace

// The four marks of a render: the batch's own, or a slot of the ring when nobody waits (RDOOM_RENDER_PROFILED)
static rdoom_status render_marks(rdoom_batch *b, bool profiled, rdoom::Event **out) {
  rdoom::Event *ev = b->ev;
  if (profiled) {
    if (b->ring_n == rdoom_batch::RING) return rdoom::fail(RDOOM_BAD_ARG, "%u profiled renders pending: collect the timings first", b->ring_n);
    ev = b->ring[b->ring_n];
    for (int k = 0; k < 4; k++)
      if (rdoom_status rs = ev[k].create()) return rs;
  }
  *out = ev;
  return RDOOM_OK;
}

// The pipeline every render queues once its per-pose constants are (or are about to be) in b->d_poses / b->d_objects: one fill of
// the zeroed words, then `constants` (the render's own launch that writes them, if any: it runs after the fill, so that it may set
// an error word), then set-up -> bin -> raster -> fragment -> fixup, ev_done, and the profiling marks ev[1..3].  ev[0] and the
// DoneGuard are the caller's, recorded and armed before anything of the render was queued.
extern "C++" {  // (a template, inside the C ABI's extern "C" block)
template <class Constants>
static rdoom_status queue_pipeline(rdoom_batch *b, uint32_t n, uint32_t kinds_mask, hipStream_t st, rdoom_timings *tm,
                                   bool objects, bool profiled, rdoom::Event *ev, DoneGuard &done, Constants &&constants) {
  const rdoom_level *lv = b->level;
  const bool marks = tm || profiled;
  const int W = (int)b->width, H = (int)b->height, PITCH = (int)b->pitch;
  // fix_count[0..3], the poses' visible-triangle counts and depth-bucket histograms (of the first n poses): one fill
  HIP_TRY(hipMemsetAsync(b->d_zeroed.get(), 0, (size_t)((const char *)b->d_ghist - (const char *)b->d_zeroed.get()) + setup_histogram_bytes(n), st));
  if (rdoom_status rs = constants()) return rs;
  if (lv->ntri)
    if (rdoom_status rs = launch_setup(st, n, lv->view, b->d_poses.get(), objects ? (const ObjectConst *)b->d_objects.get() : nullptr,
                                       lv->n_objects, W, H, kinds_mask, b->d_recs.get(), b->d_visible.get(), b->d_counts,
                                       b->d_ghist, b->cap, b->d_fix_count + 2, b->d_hidden, b->hidden_stride))
      return rs;
  const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
  bool split_lists = false;  // long tile lists stored per quadrant this render (binning kernel and rasteriser must agree)
  bool bins = false;
  if (lv->ntri && !rdoom::debug_options().no_bins)
    if (rdoom_status rs = launch_bin(st, n, b->d_recs.get(), b->d_counts, b->cap, tiles_x, tiles_y, b->d_tile_hdr.get(), b->d_entries.get(),
                                     b->entry_cap, b->d_hits.get(), b->d_overflow.get(), !rdoom::debug_options().no_split, &bins, &split_lists))
      return rs;
  if (!bins) {
    HIP_TRY(hipMemsetAsync(b->d_overflow.get(), 0xFF, sizeof(uint32_t) * n, st));
  }
  if (marks) HIP_TRY(hipEventRecord(ev[1].get(), st));
  uint32_t *prim_out = b->want_prim ? b->d_prim.get() : nullptr;
  // one reading of the debug hooks for both kernels: who writes and who reads visibility words must not change in between
  const FragmentPlan plan = plan_fragment(W, PITCH, H, (bool)b->d_qtab);
  b->last_skip_vis = plan.skip_described_vis;
  b->last_frag_count = plan.count;
  // (the rasteriser's frame is PITCH pixels wide: the padding columns of a width that is not a multiple of 4 are pixels no
  // bounding box reaches -- they stay uncovered, and the quadrants they lie in simply never count as covered)
  if (rdoom_status rs = launch_raster(st, n, lv->view, b->d_recs.get(), b->d_counts, b->cap, PITCH, H, tiles_x, tiles_y,
                                      b->d_tile_hdr.get(), b->d_entries.get(), b->entry_cap, b->d_overflow.get(), b->d_vis.get(), b->vis16, prim_out, b->d_qtab.get(),
                                      b->d_qpair.get(), plan.skip_described_vis, split_lists, bins, b->last_raster_census))
    return rs;
  if (marks) HIP_TRY(hipEventRecord(ev[2].get(), st));
  if (rdoom_status rs = launch_fragment(st, n, lv->view, b->d_recs.get(), b->d_counts, b->cap, b->d_poses.get(), W, PITCH, H, tiles_x,
                                        tiles_y, b->d_tile_hdr.get(), b->d_entries.get(), b->entry_cap, b->d_overflow.get(), b->d_vis.get(), b->vis16,
                                        prim_out, b->d_ndc.get(), b->d_fb.get(), b->d_fix_count, b->d_fix_list.get(), b->fix_cap, b->d_qtab.get(), b->d_frag_const.get(),
                                        &b->frag_const_ready, plan))
    return rs;
  HIP_TRY(hipGetLastError());
  done.armed = false;
  HIP_TRY(hipEventRecord(b->ev_done.get(), st));
  if (profiled) {
    HIP_TRY(hipEventRecord(ev[3].get(), st));
    b->ring_n++;
    b->ring_poses += n;
  }
  if (tm) {
    HIP_TRY(hipEventRecord(b->ev[3].get(), st));
    HIP_TRY(hipEventSynchronize(b->ev[3].get()));
    HIP_TRY(hipEventElapsedTime(&tm->setup_ms, b->ev[0].get(), b->ev[1].get()));
    HIP_TRY(hipEventElapsedTime(&tm->raster_ms, b->ev[1].get(), b->ev[2].get()));
    HIP_TRY(hipEventElapsedTime(&tm->fragment_ms, b->ev[2].get(), b->ev[3].get()));
    HIP_TRY(hipEventElapsedTime(&tm->total_ms, b->ev[0].get(), b->ev[3].get()));
    tm->pixels = (uint64_t)n * W * H;
    std::vector<uint32_t> counts(n);
    HIP_TRY(read_back(b, counts.data(), b->d_counts, sizeof(uint32_t) * n));
    tm->visible_triangles = 0;
    for (uint32_t c : counts) tm->visible_triangles += c;
    uint32_t fixups = 0;
    const rdoom_status fs = device_flags(b, &fixups);
    tm->fixup_pixels = fixups;
    if (fs) return fs;
  }
  return RDOOM_OK;
}
}  // extern "C++"

static rdoom_status render_impl(rdoom_batch *b, const rdoom_pose *poses, const uint8_t *lights, uint32_t lights_stride,
                                uint32_t n, uint32_t kinds_mask, hipStream_t st, rdoom_timings *tm,
                                const float *object_modelviews = nullptr, uint32_t n_objects = 0, bool profiled = false,
                                const uint32_t *level_of_pose = nullptr) {
  if (!b || !poses || !lights) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (n == 0 || n > b->max_poses) return rdoom::fail(RDOOM_BAD_ARG, "n_poses %u outside 1..%u", n, b->max_poses);
  const rdoom_level *lv = b->level;
  if (level_of_pose)
    for (uint32_t p = 0; p < n; p++)
      if (level_of_pose[p] >= lv->view.n_slices)
        return rdoom::fail(RDOOM_BAD_ARG, "pose %u names level %u of a set of %u", p, level_of_pose[p], lv->view.n_slices);
  HIP_TRY(hipSetDevice(lv->device));  // level, scratch and kernels on one device (several GPUs driven from one process)
  if (object_modelviews && n_objects < lv->n_objects)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u but the level draws objects 0..%u", n_objects, lv->n_objects - 1);
  const uint32_t sg = b->stage;  // this render's staging buffers: the H2D copy that last read them is two renders back
  b->stage = (sg + 1u) % rdoom_batch::STAGES;
  HIP_TRY(hipEventSynchronize(b->ev_copy[sg].get()));
  PoseConst *h_poses = b->h_poses[sg].get();
  if (object_modelviews) {
    const size_t count = (size_t)b->max_poses * lv->n_objects;
    if (rdoom_status rs = b->d_objects.alloc(count)) return rs;  // (on the batch's first render with objects)
    for (PinnedArray<ObjectConst> &h : b->h_objects)
      if (rdoom_status rs = h.alloc(count)) return rs;
    ObjectConst *h_objects = b->h_objects[sg].get();
    for (uint32_t p = 0; p < n; p++)
      for (uint32_t o = 0; o < lv->n_objects; o++) {
        ObjectConst &oc = h_objects[(size_t)p * lv->n_objects + o];
        const float *M = object_modelviews + ((size_t)p * n_objects + o) * 16;
        mat_mul_v1(poses[p].projection, M, oc.pm);
        std::memcpy(oc.mv, M, sizeof oc.mv);
        oc.vr0 = atan2f(oc.pm[8], oc.pm[10]);  // sky.vert:10-12
        oc.vr1 = oc.pm[9] / oc.pm[11];
        oc.pad0 = oc.pad1 = 0;
      }
  }
  for (uint32_t p = 0; p < n; p++) {  // V1: PM = P * M, plain multiply/add, left to right
    PoseConst &pc = h_poses[p];
    const float *P = poses[p].projection, *M = poses[p].modelview;
    mat_mul_v1(P, M, pc.pm);
    std::memcpy(pc.mv, M, sizeof pc.mv);
    std::memcpy(pc.proj, P, sizeof pc.proj);
    pc.time = poses[p].time;
    pc.vr0 = atan2f(pc.pm[8], pc.pm[10]);  // sky.vert:10-12
    pc.vr1 = pc.pm[9] / pc.pm[11];
    pc.zk = pc.proj[11] != 0.0f ? pc.proj[10] / pc.proj[11] : 0.0f;  // S5: Z - zk * W is small for a perspective matrix
    std::memcpy(pc.lights, lights + (size_t)p * lights_stride, 256);
    pc.level = level_of_pose ? level_of_pose[p] : 0u;
    pc.pad0 = pc.pad1 = pc.pad2 = 0u;
  }
  b->last_n = n;
  b->last_levels_on_device = false;
  rdoom::Event *ev = nullptr;
  if (rdoom_status rs = render_marks(b, profiled, &ev)) return rs;
  const bool marks = tm || profiled;
  if (marks) HIP_TRY(hipEventRecord(ev[0].get(), st));
  DoneGuard done{b, st};
  done.armed = true;  // from here on work of this render may be queued: whatever happens, ev_done is recorded after it
  HIP_TRY(hipMemcpyAsync(b->d_poses.get(), h_poses, sizeof(PoseConst) * n, hipMemcpyHostToDevice, st));
  if (object_modelviews)
    HIP_TRY(hipMemcpyAsync(b->d_objects.get(), b->h_objects[sg].get(), sizeof(ObjectConst) * (size_t)n * lv->n_objects,
                           hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(b->ev_copy[sg].get(), st));
  return queue_pipeline(b, n, kinds_mask, st, tm, object_modelviews != nullptr, profiled, ev, done, [] { return RDOOM_OK; });
}

rdoom_status rdoom_batch_render(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream) {
  return render_impl(batch, poses, lights, lights_stride, n_poses, kinds_mask, (hipStream_t)stream, nullptr);
}

rdoom_status rdoom_batch_render_timed(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                      uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                      rdoom_timings *out) {
  if (!out) return rdoom::fail(RDOOM_BAD_ARG, "out is null");
  return render_impl(batch, poses, lights, lights_stride, n_poses, kinds_mask, (hipStream_t)stream, out);
}

rdoom_status rdoom_batch_render_profiled(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                         uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream) {
  return render_impl(batch, poses, lights, lights_stride, n_poses, kinds_mask, (hipStream_t)stream, nullptr, nullptr, 0, true);
}

rdoom_status rdoom_batch_collect_timings(rdoom_batch *b, rdoom_timings *out, uint32_t *out_renders) {
  if (!b || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = rdoom_timings{};
  if (out_renders) *out_renders = b->ring_n;
  if (b->ring_n == 0) return RDOOM_OK;
  HIP_TRY(bind_device(b));
  // profiled renders may have been queued on several streams (bench.py --streams): nothing orders an earlier slot's
  // events against the last one's, so every slot's closing event is waited for
  for (uint32_t i = 0; i < b->ring_n; i++) HIP_TRY(hipEventSynchronize(b->ring[i][3].get()));
  for (uint32_t i = 0; i < b->ring_n; i++) {
    float a = 0, r = 0, f = 0, t = 0;
    HIP_TRY(hipEventElapsedTime(&a, b->ring[i][0].get(), b->ring[i][1].get()));
    HIP_TRY(hipEventElapsedTime(&r, b->ring[i][1].get(), b->ring[i][2].get()));
    HIP_TRY(hipEventElapsedTime(&f, b->ring[i][2].get(), b->ring[i][3].get()));
    HIP_TRY(hipEventElapsedTime(&t, b->ring[i][0].get(), b->ring[i][3].get()));
    out->setup_ms += a, out->raster_ms += r, out->fragment_ms += f, out->total_ms += t;
  }
  out->pixels = (uint64_t)b->ring_poses * b->width * b->height;
  std::vector<uint32_t> counts(b->last_n);  // of the last render
  HIP_TRY(read_back(b, counts.data(), b->d_counts, sizeof(uint32_t) * b->last_n));
  for (uint32_t c : counts) out->visible_triangles += c;
  uint32_t fixups = 0;
  const rdoom_status fs = device_flags(b, &fixups);
  out->fixup_pixels = fixups;
  b->ring_n = 0, b->ring_poses = 0;
  return fs;
}

rdoom_status rdoom_batch_render_objects(rdoom_batch *batch, const rdoom_pose *poses, const uint8_t *lights,
                                        uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                        const float *object_modelviews, uint32_t n_objects) {
  if (!object_modelviews) return rdoom::fail(RDOOM_BAD_ARG, "object_modelviews is null");
  return render_impl(batch, poses, lights, lights_stride, n_poses, kinds_mask, (hipStream_t)stream, nullptr,
                     object_modelviews, n_objects);
}

rdoom_status rdoom_batch_render_levels(rdoom_batch *batch, const rdoom_pose *poses, const uint32_t *level_of_pose, const uint8_t *lights,
                                       uint32_t lights_stride, uint32_t n_poses, uint32_t kinds_mask, void *stream,
                                       const float *object_modelviews, uint32_t n_objects, uint32_t flags) {
  if (!level_of_pose) return rdoom::fail(RDOOM_BAD_ARG, "level_of_pose is null");
  if (flags & ~(uint32_t)RDOOM_RENDER_PROFILED) return rdoom::fail(RDOOM_BAD_ARG, "unknown flags 0x%x", flags);
  return render_impl(batch, poses, lights, lights_stride, n_poses, kinds_mask, (hipStream_t)stream, nullptr, object_modelviews,
                     n_objects, (flags & RDOOM_RENDER_PROFILED) != 0u, level_of_pose);
}

// rdoom_batch_render_players (clock null: d_lights / lights_stride / time) and rdoom_batch_render_players_clocked (clock: a light
// set and the players' times; d_lights null) -- the clocked render queues one more launch, the light tables, after the frames'
namespace {
struct PlayerClock {
  const LightSetView *lights;
  const float *d_times;
};
}  // namespace
static rdoom_status render_players_impl(rdoom_batch *b, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                        const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_lights,
                                        uint32_t lights_stride, float time, const PlayerClock *clock, uint32_t n_players,
                                        uint32_t kinds_mask, uint32_t flags, void *stream, rdoom_pose *d_poses_out,
                                        float *d_object_modelviews_out) {
  // every check before anything is queued or allocated
  if (!b || !d_states || (!clock && !d_lights)) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (clock && clock->lights->n_levels != b->level->view.n_slices)
    return rdoom::fail(RDOOM_BAD_ARG, "the light set holds %u levels, the batch's level set %u", clock->lights->n_levels,
                       b->level->view.n_slices);
  if (clock && clock->lights->device != b->level->device)
    return rdoom::fail(RDOOM_BAD_ARG, "the light set lives on device %d, the batch on device %d", clock->lights->device, b->level->device);
  if (flags & ~(uint32_t)RDOOM_RENDER_PROFILED) return rdoom::fail(RDOOM_BAD_ARG, "unknown flags 0x%x", flags);
  if (n_players == 0 || n_players > b->max_poses) return rdoom::fail(RDOOM_BAD_ARG, "n_players %u outside 1..%u", n_players, b->max_poses);
  const rdoom_level *lv = b->level;
  if (d_object_offsets && n_objects < lv->n_objects)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u but the level draws objects 0..%u", n_objects, lv->n_objects - 1);
  if (d_object_offsets && n_objects > 4096u) return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u (at most 4096)", n_objects);
  if (d_object_modelviews_out && !d_object_offsets) return rdoom::fail(RDOOM_BAD_ARG, "object modelviews out without object offsets");
  if (!d_levels && lv->view.n_slices > 1)
    return rdoom::fail(RDOOM_BAD_ARG, "d_levels is null, but the batch's level set has %u levels", lv->view.n_slices);
  if (lights_stride != 0 && lights_stride != 256) return rdoom::fail(RDOOM_BAD_ARG, "lights_stride %u: 0 or 256", lights_stride);
  const bool profiled = (flags & RDOOM_RENDER_PROFILED) != 0u;
  if (profiled && b->ring_n == rdoom_batch::RING)
    return rdoom::fail(RDOOM_BAD_ARG, "%u profiled renders pending: collect the timings first", b->ring_n);
  PlayerFrameArgs a{};
  if (rdoom_status rs = player_projection(b->width, b->height, a.proj, &a.zk)) return rs;
  HIP_TRY(hipSetDevice(lv->device));
  if (d_object_offsets)  // (the one allocation of this path: on the batch's first render with objects)
    if (rdoom_status rs = b->d_objects.alloc((size_t)b->max_poses * lv->n_objects)) return rs;
  const hipStream_t st = (hipStream_t)stream;
  a.states = d_states, a.n = n_players, a.time = time;
  a.offsets = d_object_offsets, a.lanes = d_object_offsets ? n_objects : 1u;
  a.levels = d_levels, a.n_slices = lv->view.n_slices, a.error_word = b->d_fix_count + 3;
  a.lights = d_lights, a.lights_stride = lights_stride, a.times = clock ? clock->d_times : nullptr;
  a.pose_consts = b->d_poses.get();
  a.object_consts = d_object_offsets ? b->d_objects.get() : nullptr, a.n_render_objects = d_object_offsets ? lv->n_objects : 0u;
  a.poses_out = d_poses_out, a.modelviews_out = d_object_modelviews_out;
  // the pinned staging is not touched (no wait on ev_copy); the levels of this render live on the device only
  b->last_n = n_players;
  b->last_levels_on_device = true;
  rdoom::Event *ev = nullptr;
  if (rdoom_status rs = render_marks(b, profiled, &ev)) return rs;
  if (profiled) HIP_TRY(hipEventRecord(ev[0].get(), st));
  DoneGuard done{b, st};
  done.armed = true;
  if (!clock)
    return queue_pipeline(b, n_players, kinds_mask, st, nullptr, d_object_offsets != nullptr, profiled, ev, done,
                          [&] { return launch_player_frames(st, a); });
  // every pose's table goes straight into its PoseConst; a level outside the set shows level 0's, as its geometry
  LightTableArgs lt{};
  lt.set = *clock->lights, lt.levels = d_levels, lt.times = clock->d_times, lt.n = n_players;
  lt.out = reinterpret_cast<uint8_t *>(b->d_poses.get()) + offsetof(PoseConst, lights), lt.stride = (uint32_t)sizeof(PoseConst), lt.fallback = 0u;
  return queue_pipeline(b, n_players, kinds_mask, st, nullptr, d_object_offsets != nullptr, profiled, ev, done, [&] {
    if (rdoom_status rs = launch_player_frames(st, a)) return rs;
    return launch_light_tables(st, lt);
  });
}

rdoom_status rdoom_batch_render_players(rdoom_batch *b, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                        const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_lights,
                                        uint32_t lights_stride, float time, uint32_t n_players, uint32_t kinds_mask,
                                        uint32_t flags, void *stream, rdoom_pose *d_poses_out, float *d_object_modelviews_out) {
  if (!d_lights) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  return render_players_impl(b, d_states, d_levels, d_object_offsets, n_objects, d_lights, lights_stride, time, nullptr, n_players,
                             kinds_mask, flags, stream, d_poses_out, d_object_modelviews_out);
}

rdoom_status rdoom_batch_render_players_clocked(rdoom_batch *b, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                                const float *d_object_offsets, uint32_t n_objects, const rdoom_lightset *lights,
                                                const float *d_times, uint32_t n_players, uint32_t kinds_mask, uint32_t flags,
                                                void *stream, rdoom_pose *d_poses_out, float *d_object_modelviews_out) {
  if (!lights || !d_times)
    return rdoom::fail(RDOOM_BAD_ARG, "the clocked render needs both a light set and the players' times (%s is null)",
                       lights ? "d_times" : "the light set");
  const PlayerClock clock{lightset_view(lights), d_times};
  return render_players_impl(b, d_states, d_levels, d_object_offsets, n_objects, nullptr, 0u, 0.0f, &clock, n_players, kinds_mask,
                             flags, stream, d_poses_out, d_object_modelviews_out);
}

rdoom_status rdoom_level_num_levels(const rdoom_level *level, uint32_t *out) {
  if (!level || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = level->view.n_slices;
  return RDOOM_OK;
}

rdoom_status rdoom_level_num_objects(const rdoom_level *level, uint32_t *out) {
  if (!level || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = level->n_objects;
  return RDOOM_OK;
}

static rdoom_status set_decor_things_impl(rdoom_level *lv, uint32_t slot, const uint32_t *thing_of_quad, uint32_t n_quads) {
  if (!lv || (!thing_of_quad && n_quads)) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= lv->view.n_slices) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %u levels", slot, lv->view.n_slices);
  if (n_quads != lv->n_decor_verts[slot] / 4u)
    return rdoom::fail(RDOOM_BAD_ARG, "n_quads %u, but level %u has %u decor vertices: %u quads", n_quads, slot, lv->n_decor_verts[slot],
                       lv->n_decor_verts[slot] / 4u);
  const std::vector<uint32_t> &tri_quad = lv->tri_quad[slot];
  std::vector<uint32_t> table(tri_quad.size(), NONE);
  for (size_t t = 0; t < tri_quad.size(); t++) {
    const uint32_t q = tri_quad[t];
    if (q == NONE) continue;
    // (a vertex count that is no multiple of 4 leaves a last, partial quad the table has no entry for)
    if (q == rdoom_level::QUAD_SPANS || q >= n_quads)
      return rdoom::fail(RDOOM_BAD_ARG, "level %u: the indices of decor triangle %zu do not lie in one quad of four vertices", slot, t);
    table[t] = thing_of_quad[q];
  }
  const size_t total = (size_t)lv->slices.back().first_tri + lv->slices.back().ntri;  // triangles of the set
  HIP_TRY(hipSetDevice(lv->device));
  if (!lv->d_tri_thing && total) {
    DeviceArray<uint32_t> words;  // (the level's only once they are filled)
    if (rdoom_status rs = words.alloc(total)) return rs;
    HIP_TRY(hipMemset(words.get(), 0xFF, sizeof(uint32_t) * total));  // levels without a table: nothing is ever hidden
    lv->d_tri_thing = std::move(words);
    lv->view.tri_thing = lv->d_tri_thing.get();
  }
  if (!table.empty())
    HIP_TRY(hipMemcpy(lv->d_tri_thing.get() + lv->slices[slot].first_tri, table.data(), sizeof(uint32_t) * table.size(), hipMemcpyHostToDevice));
  lv->things_attached[slot] = 1;
  return RDOOM_OK;
}

rdoom_status rdoom_level_set_decor_things(rdoom_level *level, uint32_t slot, const uint32_t *thing_of_quad, uint32_t n_quads) {
  return rdoom::guarded([&] { return set_decor_things_impl(level, slot, thing_of_quad, n_quads); });
}

rdoom_status rdoom_batch_set_hidden_things(rdoom_batch *b, const uint32_t *d_hidden, uint32_t stride) {
  if (!b) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (!d_hidden) {
    b->d_hidden = nullptr, b->hidden_stride = 0;
    return RDOOM_OK;
  }
  if (stride == 0) return rdoom::fail(RDOOM_BAD_ARG, "stride is 0");
  if ((uintptr_t)d_hidden % 4u) return rdoom::fail(RDOOM_BAD_ARG, "d_hidden is not 4-byte aligned");
  const rdoom_level *lv = b->level;
  for (uint32_t k = 0; k < lv->view.n_slices; k++)
    if (lv->has_decor[k] && !lv->things_attached[k])
      return rdoom::fail(RDOOM_BAD_ARG, "level %u has decor triangles but no thing table (rdoom_level_set_decor_things)", k);
  b->d_hidden = d_hidden, b->hidden_stride = stride;
  return RDOOM_OK;
}

rdoom_status rdoom_batch_finish(rdoom_batch *b) {
  if (!b) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  HIP_TRY(bind_device(b));
  return device_flags(b);  // (waits for the batch's last render on its own stream: read_back)
}

rdoom_status rdoom_batch_path_stats(rdoom_batch *b, rdoom_path_stats *out) {
  if (!b || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = rdoom_path_stats{};
  HIP_TRY(bind_device(b));
  if (rdoom_status fs = device_flags(b)) return fs;
  const uint32_t n = b->last_n, T = b->n_tiles;
  out->poses = n;
  if (n == 0) return RDOOM_OK;
  return rdoom::guarded([&]() -> rdoom_status {
    std::vector<uint32_t> over(n), qtab((size_t)n * T * 4u);
    std::vector<uint2> hdr((size_t)n * T);
    HIP_TRY(read_back(b, over.data(), b->d_overflow.get(), sizeof(uint32_t) * n));
    HIP_TRY(read_back(b, hdr.data(), b->d_tile_hdr.get(), sizeof(uint2) * hdr.size()));
    HIP_TRY(read_back(b, qtab.data(), b->d_qtab.get(), sizeof(uint32_t) * qtab.size()));
    const uint32_t tiles_x = (b->width + TILE_W - 1) / TILE_W;
    for (uint32_t p = 0; p < n; p++) {
      const bool binned = over[p] == 0u;
      out->bins_overflowed_poses += binned ? 0u : 1u;
      for (uint32_t t = 0; t < T; t++) {
        if (binned) {  // (the headers of a pose that overflowed are stale)
          const uint2 h = hdr[(size_t)p * T + t];
          out->split_tiles += (h.y & TILE_SPLIT) ? 1u : 0u;
          out->tile_entries += h.y & ~TILE_SPLIT;
        }
        const uint32_t tx = (t % tiles_x) * TILE_W, ty = (t / tiles_x) * TILE_H;
        for (uint32_t q = 0; q < 4u; q++) {
          if (tx + (q & 1u) * 32u >= b->pitch || ty + (q >> 1) * 32u >= b->height) continue;  // outside the frame: never written
          out->quadrants++;
          out->described_quadrants += qtab[((size_t)p * T + t) * 4u + q] != NONE ? 1u : 0u;
        }
      }
    }
    out->tiles = (uint64_t)n * T;
    out->masked_fast_bodies = b->last_raster_census[0], out->masked_fast_pixels = b->last_raster_census[1];
    out->masked_fast_replays = b->last_raster_census[2], out->masked_general_bodies = b->last_raster_census[3];
    out->settled_pairs = b->last_raster_census[4], out->raster_pairs = b->last_raster_census[5];
    if (b->last_frag_count) {  // (rendered under the hook frag_count; zero otherwise)
      uint32_t fc[3];
      HIP_TRY(read_back(b, fc, b->d_frag_const.get() + fragment_counts_offset(), sizeof fc));
      out->half_runs = fc[0], out->half_fallbacks = fc[1], out->listed_quads = fc[2];
    }
    return RDOOM_OK;
  });
}

rdoom_status rdoom_batch_framebuffer_device(const rdoom_batch *batch, uint8_t **out_device_ptr) {
  if (!batch || !out_device_ptr) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out_device_ptr = batch->d_fb.get();
  return RDOOM_OK;
}

rdoom_status rdoom_batch_framebuffer_pitch(const rdoom_batch *batch, uint32_t *out_pitch) {
  if (!batch || !out_pitch) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out_pitch = batch->pitch;
  return RDOOM_OK;
}

rdoom_status rdoom_batch_read_framebuffer(rdoom_batch *b, uint32_t first, uint32_t count, uint8_t *host_out) {
  if (!b || !host_out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if ((uint64_t)first + count > b->last_n) return rdoom::fail(RDOOM_BAD_ARG, "frame range outside the last render");
  const size_t frame = (size_t)b->pitch * b->height;
  HIP_TRY(bind_device(b));
  if (rdoom_status fs = device_flags(b)) return fs;
  if (count) HIP_TRY(read_back(b, host_out, b->d_fb.get() + frame * first, b->width, (size_t)b->height * count, b->pitch));
  return RDOOM_OK;
}

rdoom_status rdoom_batch_enable_primitive_ids(rdoom_batch *b) {
  if (!b) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  HIP_TRY(bind_device(b));  // the ids live next to the batch's other scratch, on the level's device
  if (rdoom_status rs = b->d_prim.alloc((size_t)b->pitch * b->height * b->max_poses)) return rs;  // (once)
  b->want_prim = true;
  b->last_n = 0;  // nothing captured yet: render first
  return RDOOM_OK;
}

rdoom_status rdoom_batch_read_primitive_ids(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t *host_out) {
  if (!b || !host_out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (!b->want_prim || !b->d_prim)
    return rdoom::fail(RDOOM_BAD_ARG, "primitive ids are not captured: call rdoom_batch_enable_primitive_ids, then render");
  if ((uint64_t)first + count > b->last_n) return rdoom::fail(RDOOM_BAD_ARG, "frame range outside the last render");
  const size_t frame = (size_t)b->pitch * b->height;
  HIP_TRY(bind_device(b));
  uint32_t level_word = 0;  // (the one device flag that concerns primitive ids: a level rendered as 0 instead of the one named)
  HIP_TRY(read_back(b, &level_word, b->d_fix_count + 3, sizeof level_word));
  if (rdoom_status rs = level_error(b, level_word)) return rs;
  if (count)
    HIP_TRY(read_back(b, host_out, b->d_prim.get() + frame * first, sizeof(uint32_t) * b->width, (size_t)b->height * count, sizeof(uint32_t) * b->pitch));
  return RDOOM_OK;
}

// ---- RGB resolve (resolve.hip) --------------------------------------------------------------------------------------
// rdoom_batch_read_rgb's staging holds as many whole frames as fit in this (at least one)
static constexpr size_t RGB_STAGING_BYTES = (size_t)64 << 20;

// the colour entry points: every level the poses of frames [first, first + count) of the last render belong to needs its playpal
static rdoom_status playpal_check(const rdoom_batch *b, uint32_t first, uint32_t count) {
  const rdoom_level *lv = b->level;
  if (std::find(lv->has_palette.begin(), lv->has_palette.end(), 0) != lv->has_palette.end()) {
    // rdoom_batch_render_players: the levels are on the device, so every level of the set must have a palette
    if (b->last_levels_on_device)
      return rdoom::fail(RDOOM_BAD_ARG, "level %u of the set was created without a playpal, and the last render's levels are on the device",
                         (uint32_t)(std::find(lv->has_palette.begin(), lv->has_palette.end(), 0) - lv->has_palette.begin()));
    // the levels of the last render's poses: its pinned staging (the next render writes the other one)
    const PoseConst *pc = b->h_poses[(b->stage + rdoom_batch::STAGES - 1u) % rdoom_batch::STAGES].get();
    for (uint32_t p = first; p < first + count; p++)
      if (!lv->has_palette[pc[p].level]) return rdoom::fail(RDOOM_BAD_ARG, "pose %u: its level %u was created without a playpal", p, pc[p].level);
  }
  return RDOOM_OK;
}


// ---- reading the last render back: RGB (resolve.hip), planes and the thing plane (planes.hip), observations (observe.hip) ----
// One read-back pass over frames of the last render: which reader, and its entry point's argument as the caller gave it.
struct ReadPass {
  enum { RGB, PLANE, THING_PLANE, OBSERVATION } reader;
  uint32_t arg;     // format / plane / flags, RDOOM_RGB_TOP_DOWN among them
  uint32_t fx, fy;  // observations only
};

// what every such entry point rejects, after its own argument's checks, before it touches the device or waits for anything
static rdoom_status last_render_check(const rdoom_batch *b, uint32_t first, uint32_t count, const void *out) {
  if (!b || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (b->last_n == 0) return rdoom::fail(RDOOM_BAD_ARG, "nothing rendered yet");
  if ((uint64_t)first + count > b->last_n) return rdoom::fail(RDOOM_BAD_ARG, "frame range outside the last render");
  return RDOOM_OK;
}

static rdoom_status rgb_args(const rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, const void *out) {
  if (format & ~(0xFFu | (uint32_t)RDOOM_RGB_TOP_DOWN)) return rdoom::fail(RDOOM_BAD_ARG, "unknown format bits 0x%x", format);
  if ((format & 0xFFu) != RDOOM_RGB8 && (format & 0xFFu) != RDOOM_RGBA8)
    return rdoom::fail(RDOOM_BAD_ARG, "format 0x%x: RDOOM_RGB8 or RDOOM_RGBA8, optionally | RDOOM_RGB_TOP_DOWN", format);
  if (rdoom_status rs = last_render_check(b, first, count, out)) return rs;
  return playpal_check(b, first, count);
}

static rdoom_status plane_args(const rdoom_batch *b, uint32_t first, uint32_t count, uint32_t plane, const void *out) {
  if (plane & ~(0xFFu | (uint32_t)RDOOM_RGB_TOP_DOWN)) return rdoom::fail(RDOOM_BAD_ARG, "unknown plane bits 0x%x", plane);
  const uint32_t which = plane & 0xFFu;  // (PLANE_THING is not the caller's to name)
  if (which != RDOOM_PLANE_DEPTH && which != RDOOM_PLANE_LABEL && which != RDOOM_PLANE_PRIMITIVE)
    return rdoom::fail(RDOOM_BAD_ARG, "plane 0x%x: RDOOM_PLANE_DEPTH, _LABEL or _PRIMITIVE, optionally | RDOOM_RGB_TOP_DOWN", plane);
  if (rdoom_status rs = last_render_check(b, first, count, out)) return rs;
  if ((uintptr_t)out % plane_element_bytes(which)) return rdoom::fail(RDOOM_BAD_ARG, "output is not aligned to the plane's %zu-byte element", plane_element_bytes(which));
  return RDOOM_OK;
}

static rdoom_status thing_plane_args(const rdoom_batch *b, uint32_t first, uint32_t count, uint32_t flags, const void *out) {
  if (flags & ~(uint32_t)RDOOM_RGB_TOP_DOWN) return rdoom::fail(RDOOM_BAD_ARG, "unknown flag bits 0x%x: 0 or RDOOM_RGB_TOP_DOWN", flags);
  if (rdoom_status rs = last_render_check(b, first, count, out)) return rs;
  if ((uintptr_t)out % 4u) return rdoom::fail(RDOOM_BAD_ARG, "output is not aligned to the plane's 4-byte element");
  return RDOOM_OK;
}

static rdoom_status observation_args(const rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, uint32_t fx, uint32_t fy,
                                     const void *out) {
  if (format & ~(0xFFu | (uint32_t)RDOOM_RGB_TOP_DOWN)) return rdoom::fail(RDOOM_BAD_ARG, "unknown format bits 0x%x", format);
  const uint32_t which = format & 0xFFu;
  if (which != RDOOM_OBS_RGB8 && which != RDOOM_OBS_RGB8_PLANAR && which != RDOOM_OBS_GRAY8 && which != RDOOM_OBS_DEPTH_MIN)
    return rdoom::fail(RDOOM_BAD_ARG, "format 0x%x: RDOOM_OBS_RGB8, _RGB8_PLANAR, _GRAY8 or _DEPTH_MIN, optionally | RDOOM_RGB_TOP_DOWN", format);
  for (uint32_t v : {fx, fy})
    if (v != 1u && v != 2u && v != 4u && v != 8u) return rdoom::fail(RDOOM_BAD_ARG, "factors %u x %u: each must be 1, 2, 4 or 8", fx, fy);
  if (rdoom_status rs = last_render_check(b, first, count, out)) return rs;
  if (b->width / fx == 0 || b->height / fy == 0)
    return rdoom::fail(RDOOM_BAD_ARG, "factors %u x %u leave no cell of a %u x %u frame", fx, fy, b->width, b->height);
  if (which == RDOOM_OBS_DEPTH_MIN && (uintptr_t)out % 4u) return rdoom::fail(RDOOM_BAD_ARG, "output is not aligned to the format's 4-byte element");
  return which == RDOOM_OBS_DEPTH_MIN ? RDOOM_OK : playpal_check(b, first, count);
}

// bytes of one frame as the pass stores it
static size_t pass_frame_bytes(const rdoom_batch *b, const ReadPass &p) {
  const size_t pixels = (size_t)b->height * b->width;
  switch (p.reader) {
    case ReadPass::RGB: return pixels * (p.arg & 0xFFu);
    case ReadPass::PLANE: return pixels * plane_element_bytes(p.arg & 0xFFu);
    case ReadPass::THING_PLANE: return pixels * sizeof(int32_t);
    default: return (size_t)(b->height / p.fy) * (b->width / p.fx) * observation_cell_bytes(p.arg & 0xFFu);
  }
}

static FrameSource frame_source(const rdoom_batch *b, uint32_t first, uint32_t count, bool top_down) {
  FrameSource s{};
  s.fb = b->d_fb.get(), s.vis = b->d_vis.get(), s.vis16 = b->vis16, s.qtab = b->d_qtab.get(), s.use_qtab = b->last_skip_vis;
  s.poses = b->d_poses.get(), s.recs = b->d_recs.get(), s.cap = b->cap;
  s.fix_count = b->d_fix_count, s.fix_list = b->d_fix_list.get(), s.fix_cap = b->fix_cap;
  s.width = b->width, s.pitch = b->pitch, s.height = b->height, s.first = first, s.count = count, s.top_down = top_down;
  return s;
}

// queues the pass's two kernels on st behind the last render; ev_done then marks their end (finish / read_* wait for it)
static rdoom_status queue_pass(rdoom_batch *b, const ReadPass &p, uint32_t first, uint32_t count, void *out, hipStream_t st) {
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done.get(), 0));
  const FrameSource src = frame_source(b, first, count, (p.arg & RDOOM_RGB_TOP_DOWN) != 0u);
  const DeviceLevelView &lv = b->level->view;
  rdoom_status rs = RDOOM_OK;
  switch (p.reader) {
    case ReadPass::RGB: rs = launch_resolve(st, ResolveArgs{src, b->level->d_palettes.get(), p.arg & 0xFFu, (uint8_t *)out}); break;
    case ReadPass::PLANE: rs = launch_plane(st, PlaneArgs{src, lv.tris, lv.slices, nullptr, p.arg & 0xFFu, out}); break;
    case ReadPass::THING_PLANE: rs = launch_plane(st, PlaneArgs{src, lv.tris, lv.slices, lv.tri_thing, PLANE_THING, out}); break;
    case ReadPass::OBSERVATION: rs = launch_observe(st, ObserveArgs{src, b->level->d_palettes.get(), p.arg & 0xFFu, p.fx, p.fy, out}); break;
  }
  HIP_TRY(hipEventRecord(b->ev_done.get(), st));  // (also after a failed launch: nothing waits for a render that is not the last)
  return rs;
}

// device_out of the resolve entry points must be device memory of the batch's device with room for what the kernels write there
static rdoom_status device_out_check(const rdoom_batch *b, const void *device_out, size_t bytes) {
  hipPointerAttribute_t attr{};
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipPointerGetAttributes(&attr, device_out) != hipSuccess || attr.type != hipMemoryTypeDevice ||
      hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)device_out) != hipSuccess) {
    (void)hipGetLastError();  // (a failed query must not be reported by the next render's launch check)
    return rdoom::fail(RDOOM_BAD_ARG, "device_out is not device memory");
  }
  if (attr.device != b->level->device) return rdoom::fail(RDOOM_BAD_ARG, "device_out is on device %d, the batch on %d", attr.device, b->level->device);
  if ((const char *)device_out + bytes > (const char *)base + size)
    return rdoom::fail(RDOOM_BAD_ARG, "device_out: %zu bytes needed, its allocation ends %zu bytes after it", bytes,
                       (size_t)((const char *)base + size - (const char *)device_out));
  return RDOOM_OK;
}

// the asynchronous entry points, their arguments checked: the pass into the caller's device memory on the caller's stream
static rdoom_status resolve_to_device(rdoom_batch *b, const ReadPass &p, uint32_t first, uint32_t count, void *device_out, void *stream) {
  HIP_TRY(bind_device(b));
  if (rdoom_status rs = device_out_check(b, device_out, (size_t)count * pass_frame_bytes(b, p))) return rs;
  return queue_pass(b, p, first, count, device_out, (hipStream_t)stream);
}

// The synchronous entry points, their arguments checked: the pass into the batch's bounded staging buffer -- as many whole frames
// as fit in RGB_STAGING_BYTES, at least one; allocated on first use -- a chunk of frames at a time, each copied to the host on
// copy_stream and waited for.
static rdoom_status read_to_host(rdoom_batch *b, const ReadPass &p, uint32_t first, uint32_t count, void *host_out) {
  HIP_TRY(bind_device(b));
  if (rdoom_status fs = device_flags(b)) return fs;
  if (count == 0) return RDOOM_OK;
  const size_t frame = pass_frame_bytes(b, p);
  const uint32_t chunk = (uint32_t)std::max<size_t>(1u, std::min<size_t>(count, RGB_STAGING_BYTES / frame));
  if (b->rgb_bytes < chunk * frame) {
    b->d_rgb.reset(), b->rgb_bytes = 0;
    if (rdoom_status rs = b->d_rgb.alloc(chunk * frame)) return rs;
    b->rgb_bytes = chunk * frame;
  }
  for (uint32_t f = first; f < first + count; f += chunk) {
    const uint32_t n = std::min(chunk, first + count - f);
    if (rdoom_status rs = queue_pass(b, p, f, n, b->d_rgb.get(), b->copy_stream.get())) return rs;
    HIP_TRY(hipMemcpyAsync((uint8_t *)host_out + (size_t)(f - first) * frame, b->d_rgb.get(), n * frame, hipMemcpyDeviceToHost, b->copy_stream.get()));
    HIP_TRY(hipStreamSynchronize(b->copy_stream.get()));
  }
  return RDOOM_OK;
}

rdoom_status rdoom_batch_resolve_rgb(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, void *device_out, void *stream) {
  if (rdoom_status rs = rgb_args(b, first, count, format, device_out)) return rs;
  return resolve_to_device(b, ReadPass{ReadPass::RGB, format, 1u, 1u}, first, count, device_out, stream);
}

rdoom_status rdoom_batch_read_rgb(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, uint8_t *host_out) {
  if (rdoom_status rs = rgb_args(b, first, count, format, host_out)) return rs;
  return read_to_host(b, ReadPass{ReadPass::RGB, format, 1u, 1u}, first, count, host_out);
}

rdoom_status rdoom_batch_resolve_plane(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t plane, void *device_out, void *stream) {
  if (rdoom_status rs = plane_args(b, first, count, plane, device_out)) return rs;
  return resolve_to_device(b, ReadPass{ReadPass::PLANE, plane, 1u, 1u}, first, count, device_out, stream);
}

rdoom_status rdoom_batch_read_plane(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t plane, void *host_out) {
  if (rdoom_status rs = plane_args(b, first, count, plane, host_out)) return rs;
  return read_to_host(b, ReadPass{ReadPass::PLANE, plane, 1u, 1u}, first, count, host_out);
}

// (include/rdoom_frame_things.h)
rdoom_status rdoom_batch_resolve_thing_plane(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t flags, int32_t *d_out, void *stream) {
  if (rdoom_status rs = thing_plane_args(b, first, count, flags, d_out)) return rs;
  return resolve_to_device(b, ReadPass{ReadPass::THING_PLANE, flags, 1u, 1u}, first, count, d_out, stream);
}

rdoom_status rdoom_batch_read_thing_plane(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t flags, int32_t *host_out) {
  if (rdoom_status rs = thing_plane_args(b, first, count, flags, host_out)) return rs;
  return read_to_host(b, ReadPass{ReadPass::THING_PLANE, flags, 1u, 1u}, first, count, host_out);
}

rdoom_status rdoom_batch_resolve_observation(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, uint32_t fx, uint32_t fy,
                                             void *device_out, void *stream) {
  if (rdoom_status rs = observation_args(b, first, count, format, fx, fy, device_out)) return rs;
  return resolve_to_device(b, ReadPass{ReadPass::OBSERVATION, format, fx, fy}, first, count, device_out, stream);
}

rdoom_status rdoom_batch_read_observation(rdoom_batch *b, uint32_t first, uint32_t count, uint32_t format, uint32_t fx, uint32_t fy,
                                          void *host_out) {
  if (rdoom_status rs = observation_args(b, first, count, format, fx, fy, host_out)) return rs;
  return read_to_host(b, ReadPass{ReadPass::OBSERVATION, format, fx, fy}, first, count, host_out);
}

}  // extern "C"
