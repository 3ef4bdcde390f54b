// What the world's kernels (world.hip), the map's (automap.hip), the seen lines' (reveal.hip), the explored area's (area.hip), the sectors' (sectors.hip), the spawn's (spawn.hip), the floods' (flood.hip), the goal distance's (goal.hip), the path unit's (path.hip), the thing maps' (thingmap.hip) and the stamp's (stamp.hip) share: the pick of a lane's level,
// a wave's maximum and sum and the append into a list in LDS, what the map units read of a line, the checked launch, the device
// check of a handle, the checks of a fan, of a row of offsets and of a map view, and the map's side of a world handle (its
// tables own their device memory: device_memory.hpp).  (The sight pass of reveal.hip and area.hip is sight.hpp's.)
// One definition each, for player_quat.hpp's reason.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"

namespace rdoom_dev {

// `use(slot)` for the level record of a lane on level `lv`: the wave's one slot as a wave-uniform value when every lane of the
// wave is on the same level, so that what `use` loads from that record are scalar loads; the lane's own otherwise
template <class Use>
__device__ __forceinline__ void with_level(uint32_t lv, Use use) {
  const uint32_t u = __builtin_amdgcn_readfirstlane(lv);
  if (__builtin_amdgcn_ballot_w64(lv != u) == 0) use(u);
  else use(lv);
}

// ---- a workgroup of 64-lane waves: a wave's maximum and sum, and the append of its threads' keepers to a list in LDS ----
constexpr uint32_t WAVE_LANES = 64;
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (uint32_t o = WAVE_LANES / 2; o; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (uint32_t o = WAVE_LANES / 2; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// Where a thread that keeps its item puts it in a list that holds `start` entries, and the keepers of the whole workgroup: a ballot
// and a prefix within the wave, the waves' counts through LDS (`counts`: WAVES words).  Items stay in thread order.  Every thread of
// the workgroup calls it, with its lane and its wave: there is one barrier inside, and the caller's own follows its stores.  A
// count is the same in every lane, and is read as the scalar it is: through a pointer the compiler no longer sees that by itself
struct Appended {
  uint32_t slot, total;
};
template <uint32_t WAVES>
__device__ __forceinline__ Appended append(bool keep, uint32_t lane, uint32_t wave, uint32_t *counts, uint32_t start) {
  const uint64_t kept = __builtin_amdgcn_ballot_w64(keep);
  const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
  if (lane == 0) counts[wave] = (uint32_t)__builtin_popcountll(kept);
  __syncthreads();
  uint32_t at = start, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < WAVES; w++) {
    const uint32_t n = __builtin_amdgcn_readfirstlane(counts[w]);
    at += w < wave ? n : 0u;
    total += n;
  }
  return Appended{at + before, total};
}

// ---- a line of the table as the map contracts read it (include/rdoom.h "top-down maps", "seen lines") ----
constexpr uint32_t SIDE_FRONT = 1u << 16, SIDE_BACK = 1u << 17;  // MapDevice::flags above the linedef's 16
constexpr uint32_t BOTH_SIDES = SIDE_FRONT | SIDE_BACK;

// a segment as the contract's dist2 reads it: a, d = b - a, inv = 1 / |d|^2; ok: |d|^2 > 0
struct Segment {
  float ax, az, dx, dz, inv;
  bool ok;
};
__device__ __forceinline__ Segment segment(float ax, float az, float bx, float bz) {
  const float dx = bx - ax, dz = bz - az;
  const float len2 = dx * dx + dz * dz;
  return Segment{ax, az, dx, dz, 1.0f / len2, len2 > 0.0f};
}
__device__ __forceinline__ float dist2(float qx, float qz, float ax, float az, float dx, float dz, float inv) {
  const float wx = qx - ax, wz = qz - az;
  float t = (wx * dx + wz * dz) * inv;
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  const float ex = wx - t * dx, ez = wz - t * dz;
  return ex * ex + ez * ez;
}

// ---- the map contract's pixel-to-world mapping (include/rdoom.h "top-down maps"), the one definition the line maps (automap.hip)
// and the sector maps (sectors.hip) share, so that the two register exactly: the operations of the contract, in its order ----
struct MapFrame {
  float px, pz;     // the player's position
  float c, fx, fz;  // the cosine of the yaw and the forward f = (-s, -c); the right is (c, fx)
  float hw, hh, scale;
  uint32_t height;
  bool rotate, top_down;
};
__device__ __forceinline__ MapFrame map_frame(const rdoom_player_state *st, uint32_t width, uint32_t height, float scale, uint32_t view_flags) {
  float s, c;
  sincos_rd(st->yaw, s, c);
  return MapFrame{st->pos[0], st->pos[2], c, -s, -c, (float)width * 0.5f, (float)height * 0.5f, scale, height,
                  (view_flags & RDOOM_MAP_ROTATE) != 0, (view_flags & RDOOM_MAP_TOP_DOWN) != 0};
}
// the world point of map coordinates (u, v): u to the right, v up, in world units from the player
__device__ __forceinline__ void map_to_world(const MapFrame &f, float u, float v, float &qx, float &qz) {
  if (f.rotate) qx = (f.px + f.c * u) + f.fx * v, qz = (f.pz + f.fx * u) + f.fz * v;
  else qx = f.px - v, qz = f.pz - u;
}
// u of column i, and v of output row `row` (row 0 is the bottom row of pixels unless top_down)
__device__ __forceinline__ float map_u(const MapFrame &f, uint32_t i) { return (((float)i + 0.5f) - f.hw) * f.scale; }
__device__ __forceinline__ float map_v(const MapFrame &f, uint32_t row) {
  const int32_t j = f.top_down ? (int32_t)f.height - 1 - (int32_t)row : (int32_t)row;
  return (((float)j + 0.5f) - f.hh) * f.scale;
}

// a sector height as a player's game has it: height + off(object), off = the y of the object's row in the player's offsets
// (`off`: that player's n_objects x xyz, or null), 0 for object 0 and objects beyond the row
__device__ __forceinline__ float live_height(float height, uint32_t object, const float *off, uint32_t n_objects) {
  return height + ((off && object != 0 && object < n_objects) ? off[(size_t)object * 3 + 1] : 0.0f);
}

// ---- the sector at a point (include/rdoom.h "sectors"), the one definition the sector kernels (sectors.hip) and the spawn kernel
// (spawn.hip) share: `child_of` (a step of the descent) + `sector_in_leaf` (the void and NaN rules), in the contract's binary32
// operations; the units that use them turn contraction off ----
struct SectorTables {  // SectorDevice's arrays
  const float4 *nodes;
  const uint4 *leaves;
  const float4 *edges;
  const float4 *sectors;
};
struct SectorLevel {  // where a level's tables start, and its sectors
  uint32_t node0, leaf0, sector0, n_sectors;
};

// the child of a node on q's side, as Child::pack writes it
__device__ __forceinline__ int32_t child_of(float4 node, float qx, float qz) {
  const float dist = (qx * node.y - qz * node.x) + node.z;
  const uint32_t children = __float_as_uint(node.w);
  return dist >= 0.0f ? (int32_t)(int16_t)(children & 0xFFFFu) : (int32_t)(int16_t)(children >> 16);
}

// the descent from the root of a level (`nodes`: the level's) to a leaf of it
__device__ __forceinline__ uint32_t descend(const float4 *nodes, float qx, float qz) {
  int32_t at = child_of(nodes[0], qx, qz);
  while (at > 0) at = child_of(nodes[at], qx, qz);
  return (uint32_t)-at;
}

// the sector of q in leaf `leaf` (an index into t.leaves): the leaf's, or none when q is void or not a number
__device__ __forceinline__ uint32_t sector_in_leaf(const SectorTables &t, uint32_t leaf, float qx, float qz) {
  const uint4 record = t.leaves[leaf];
  bool inside = qx == qx && qz == qz;
  for (uint32_t e = 0; e < record.z; e++) {
    const float4 g = t.edges[record.y + e];
    const float cross = (qx - g.x) * g.w - (qz - g.y) * g.z;
    inside = inside && !(cross > 0.0f);
  }
  return inside ? record.x : RDOOM_SECTOR_NONE;
}

// player `off`'s live floor and ceiling of sector s of the level (+inf, -inf for none)
__device__ __forceinline__ float2 live_heights(const SectorTables &t, const SectorLevel &lv, uint32_t s, const float *off, uint32_t n_objects) {
  if (s == RDOOM_SECTOR_NONE) return make_float2(__builtin_inff(), -__builtin_inff());
  const float4 r = t.sectors[lv.sector0 + s];
  return make_float2(live_height(r.x, __float_as_uint(r.z), off, n_objects), live_height(r.y, __float_as_uint(r.w), off, n_objects));
}

constexpr float CELL_LIMIT = 1073741824.0f;  // 2^30

// ---- the explored-area grid of a level (include/rdoom.h "explored area": the contract's formulas; host and device), the one
// definition the explored area's kernels (area.hip), the goal unit's (goal.hip) and the path unit's (path.hip) share ----
struct Grid {
  int32_t ix0, iz0;
  uint32_t gw, gh, pitch;
};
// cx(x), and whether x / cell is finite and below 2^30 in magnitude
__host__ __device__ __forceinline__ bool cell_of(float x, float cell, int32_t &c) {
  const float q = x / cell;
  c = (int32_t)__builtin_floorf(q);
  return __builtin_fabsf(q) < CELL_LIMIT;
}
// false: a bound outside the limits (the host refuses such a grid before anything is queued, so a kernel never meets one)
__host__ __device__ __forceinline__ bool grid_of(float4 b, float cell, Grid &g) {
  int32_t x0, x1, z0, z1;
  const bool ok = cell_of(b.x, cell, x0) & cell_of(b.y, cell, x1) & cell_of(b.z, cell, z0) & cell_of(b.w, cell, z1);
  g.ix0 = x0 - 1, g.iz0 = z0 - 1;
  g.gw = (uint32_t)(x1 + 1 - g.ix0 + 1), g.gh = (uint32_t)(z1 + 1 - g.iz0 + 1);
  g.pitch = (g.gw + 31u) / 32u;
  return ok;
}
// the cell of point (x, z) in grid g: false when it lies in none.  The differences are taken modulo 2^32: a true difference is
// within -2^31 .. 2^31, so a negative or overflowing one is far above gw
__device__ __forceinline__ bool point_cell(const Grid &g, float cell, float x, float z, uint32_t &ix, uint32_t &iz) {
  int32_t cx, cz;
  const bool ok = cell_of(x, cell, cx) & cell_of(z, cell, cz);
  ix = (uint32_t)cx - (uint32_t)g.ix0, iz = (uint32_t)cz - (uint32_t)g.iz0;
  return ok && ix < g.gw && iz < g.gh;
}

// ---- walking on a grid of floor and ceiling planes (include/rdoom.h "goal distance": "Open", "Moves"), the one definition the
// floods (flood.hip), the walk down their field (path.hip) and the wall distance (walls.hip, is_open alone) share; the units
// that use them turn contraction off ----
struct WalkLimits {
  float max_step, max_drop, clearance;
};
__device__ __forceinline__ bool is_open(float f, float g, float clearance) {
  return f < __builtin_inff() && f > -__builtin_inff() && g - f >= clearance;
}
// the move from a to b
__device__ __forceinline__ bool allowed(float fa, float ga, float fb, float gb, const WalkLimits &l) {
  return is_open(fa, ga, l.clearance) && is_open(fb, gb, l.clearance) && fb - fa <= l.max_step && fa - fb <= l.max_drop &&
         fminf(ga, gb) - fmaxf(fa, fb) >= l.clearance;
}

}  // namespace rdoom_dev

namespace rdoom::game {
struct World;
}

namespace rdoom {

// kernel(args...) on `stream`, and the error of a launch that could not be queued
template <class Kernel, class... Args>
rdoom_status launch_checked(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, void *stream, Args... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, args...);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

// noun: "the world" or "the world set"
template <class Handle>
rdoom_status check_device(const Handle *h, const char *noun) {
  if (!h->on_device) return rdoom::fail(RDOOM_BAD_ARG, "%s was created with RDOOM_WORLD_HOST_ONLY: it has no device copy", noun);
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != h->device) return rdoom::fail(RDOOM_BAD_ARG, "%s lives on device %d, the current device is %d", noun, h->device, cur);
  return RDOOM_OK;
}

// what every call that takes a fan of rays checks of it
inline rdoom_status check_fan(uint32_t n_rays, float max_range) {
  if (!n_rays) return rdoom::fail(RDOOM_BAD_ARG, "n_rays is 0");
  if (!(max_range > 0.0f) || max_range == __builtin_inff())
    return rdoom::fail(RDOOM_BAD_ARG, "max_range %g is not a finite positive number", (double)max_range);
  return RDOOM_OK;
}
// a caller's rows of object offsets (null: none) against the `needed` objects of the noun: "world", "world set", "game", "set"
inline rdoom_status check_offsets(const float *d_offsets, uint32_t n_objects, uint32_t needed, const char *noun) {
  if (d_offsets && n_objects < needed)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is smaller than the %s's %u objects", n_objects, noun, needed);
  return RDOOM_OK;
}
// the size and the scale of a drawn map (automap.hip, sectors.hip, area.hip)
constexpr uint32_t MAX_SIDE = 16384;
inline rdoom_status check_view(const rdoom_map_view *view) {
  if (!view->width || !view->height || view->width > MAX_SIDE || view->height > MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "a map of %u x %u pixels (1 .. %u a side)", view->width, view->height, MAX_SIDE);
  if (!(view->scale > 0.0f) || view->scale == __builtin_inff())
    return rdoom::fail(RDOOM_BAD_ARG, "scale %g is not a finite positive number", (double)view->scale);
  return RDOOM_OK;
}

// The device copy of a line table (rdoom_map_line), a structure of arrays private to automap.hip and reveal.hip: a world's, or a world set's
// levels one after the other with `levels[slot]` = (first line, number of lines).
struct MapDevice {
  DeviceArray<float4> seg;      // a.x, a.z, b.x, b.z
  DeviceArray<float4> heights;  // front floor, front ceiling, back floor, back ceiling
  DeviceArray<uint4> ids;       // the objects of those four
  DeviceArray<uint32_t> flags;  // the linedef's flags; bit 16: the front side is present, bit 17: the back side
  DeviceArray<uint2> levels;    // a world set's slots (a world: one entry)
  DeviceArray<float4> bounds;   // a slot's minx, maxx, minz, maxz (line_bounds): what the explored-area grid is derived from (area.hip)
  uint32_t n_lines = 0, n_levels = 0;
};
// the exact bounds of a table's end points as the "explored area" contract takes them: minx, maxx, minz, maxz; zeros for no lines
inline float4 line_bounds(const rdoom_map_line *lines, size_t n) {
  if (!n) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 b = make_float4(lines[0].a[0], lines[0].a[0], lines[0].a[1], lines[0].a[1]);
  for (size_t i = 0; i < n; i++)
    for (const float *v : {lines[i].a, lines[i].b}) {
      b.x = v[0] < b.x ? v[0] : b.x, b.y = v[0] > b.y ? v[0] : b.y;
      b.z = v[1] < b.z ? v[1] : b.z, b.w = v[1] > b.w ? v[1] : b.w;
    }
  return b;
}
// automap.hip: `lines` with `n_levels` (first, count) ranges on the current device
rdoom_status map_upload(const std::vector<rdoom_map_line> &lines, const std::vector<uint2> &levels, MapDevice &out);

// The device copy of a sector table (rdoom_map_sectors) and of the BSP that leads to it, a structure of arrays private to
// sectors.hip: a world's, or a world set's levels one after the other, every index inside a level the level's own.
struct SectorDevice {
  DeviceArray<float4> nodes;    // d.x, d.y, c = d.x * o.y - d.y * o.x, and as bits the children: positive in the low 16, negative in
                                // the high 16, each an int16 as Child::pack writes it (> 0 a node, <= 0 minus a leaf)
  DeviceArray<uint4> leaves;    // the leaf's sector or RDOOM_SECTOR_NONE, its first solid edge (in `edges`), their number, 0
  DeviceArray<float4> edges;    // a.x, a.z, d.x, d.z
  DeviceArray<float4> sectors;  // floor, ceiling, and as bits floor_id, ceiling_id
  DeviceArray<uint4> levels;    // a slot's first node, first leaf, first sector, number of sectors
  uint32_t n_levels = 0;
};
// sectors.hip: the tables of `levels` on the current device (RDOOM_BAD_LEVEL: a level with more nodes or leaves than 16 bits
// address)
rdoom_status sector_upload(const std::vector<const game::World *> &levels, SectorDevice &out);

// The device copy of a spawn table (rdoom_spawn_table), private to spawn.hip: a world's, or a world set's levels one after the
// other.
struct SpawnDevice {
  DeviceArray<float> cumulative;  // an entry's cumulative area
  DeviceArray<float4> corners;    // three per entry: a, b, c as xyz
  DeviceArray<uint4> levels;      // a slot's first entry, its entries, the bound of the search ceil(log2(entries)) + 1, 0
  DeviceArray<float4> starts;     // a slot's start position and yaw
  uint32_t n_levels = 0;
  uint4 level0 = {};            // slot 0's two records on the host: a single world's launch passes them by value
  float4 start0 = {};
};
// spawn.hip: the tables of `levels` on the current device
rdoom_status spawn_upload(const std::vector<const game::World *> &levels, SpawnDevice &out);

// what automap.hip, reveal.hip, sectors.hip and spawn.hip need of a world or world-set handle (world.hip owns the handles)
struct MapSource {
  const MapDevice *map;
  const SectorDevice *sectors;
  const SpawnDevice *spawn;
  uint32_t max_sectors;   // the sectors of its table; a set's: of its largest level's (known on host-only handles too)
  uint32_t game_objects;  // the n_objects its game calls need at least
  uint32_t max_lines;     // the lines of its table; a set's: of its largest level's (known on host-only handles too)
  const float4 *bounds;   // line_bounds of every level, on the host (known on host-only handles too)
  uint32_t n_levels;      // the levels of the handle: 1 for a world
  bool on_device;
  int device;
};
MapSource map_source(const rdoom_world *w);
MapSource map_source(const rdoom_worldset *s);
// the 32-bit words a row of visited bits needs for that sector table
inline uint32_t visited_words(const MapSource &src) { return (src.max_sectors + 31u) / 32u; }
// the 32-bit words a row of seen bits needs for that table
inline uint32_t seen_words(const MapSource &src) { return (src.max_lines + 31u) / 32u; }
// the d_seen / stride of a draw or a reveal against the handle's table.  noun: "world" or "world set"
inline rdoom_status check_seen_stride(const MapSource &src, const char *noun, uint32_t stride) {
  if (stride < seen_words(src))
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the %s's %u lines takes", stride, seen_words(src), noun,
                       src.max_lines);
  return RDOOM_OK;
}

// the largest gw, gh and words of the handle's levels at `cell` (w, or set with its n_levels), by the explored-area grid calls: their
// errors are the caller's
inline rdoom_status handle_grid(const rdoom_world *w, const rdoom_worldset *set, uint32_t n_levels, float cell, rdoom_area_grid &most) {
  most = rdoom_area_grid{};
  for (uint32_t slot = 0; slot < n_levels; slot++) {
    rdoom_area_grid g;
    if (rdoom_status s = w ? rdoom_world_area_grid(w, cell, &g) : rdoom_worldset_level_area_grid(set, slot, cell, &g)) return s;
    most.gw = g.gw > most.gw ? g.gw : most.gw, most.gh = g.gh > most.gh ? g.gh : most.gh;
    most.words = g.words > most.words ? g.words : most.words;
  }
  return RDOOM_OK;
}
// flood.hip: what rdoom_flood_grids and rdoom_flood_descend check of the arguments they share -- params, the grid's size, n; and
// `pointers`, whether the caller's required pointers are there (`missing` names them)
rdoom_status check_flood_grids(const rdoom_flood_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width,
                               uint32_t height);
// flood.hip: what rdoom_flood_grids_octile and rdoom_flood_descend_octile check: the same, then the two costs
rdoom_status check_flood_octile(const rdoom_flood_octile_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width,
                                uint32_t height);
// flood.hip: what rdoom_grid_walk_lines (line.hip) checks: the arguments shared with rdoom_flood_grids, then the targets a row
rdoom_status check_walk_lines(const rdoom_flood_params *params, uint32_t n, bool pointers, uint32_t width, uint32_t height, uint32_t n_to);
// flood.hip: what rdoom_path_straighten (line.hip) checks: the same, then the look-ahead and the two lengths
rdoom_status check_path_straighten(const rdoom_flood_params *params, uint32_t n, bool pointers, uint32_t width, uint32_t height,
                                   uint32_t path_len, uint32_t max_look, uint32_t corner_len);
// flood.hip: the cells of a row, column or diagonal one thread of a grid's flood sweeps at a time
uint32_t flood_run_length(uint32_t width, uint32_t height);

}  // namespace rdoom
