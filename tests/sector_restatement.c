/* Test-side restatement of the sectors contract (include/rdoom.h "sectors"; the product's is rust-doom_amd/csrc/hip/sectors.hip), in
 * binary32, sharing no code with the product and none of its shape: every point goes down from the root on its own, node by node,
 * through the HOST arrays as the library lends them (rdoom_world_node records of rdoom_world_host_arrays, the tables of
 * rdoom_world_map_sectors) -- no packed children, no precomputed constant, no wave, no tile.  The pixel's point is the map
 * contract's, written out as tests/automap_restatement.c writes it, with the restatements' sincos (tests/sincos_restatement.h).
 * Built by the tests like the other restatements (tests/sector_ref.py): gcc -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "sincos_restatement.h"
#define SR_NONE 0xFFFFFFFFu
#define SR_NONE16 0xFFFFu

typedef struct { float origin[2], displace[2], length; int32_t positive, negative; } sr_node;
typedef struct { float floor, ceiling; uint32_t floor_id, ceiling_id, light_level, sector_type, tag; } sr_sector;
typedef struct { float a[2], d[2]; } sr_edge;
typedef struct { uint32_t first, count; } sr_range;
typedef struct {
  const sr_node *nodes;
  const sr_sector *sectors;
  const uint32_t *leaf_sector;
  const sr_range *leaf_edges;
  const sr_edge *edges;
  uint32_t n_nodes, n_sectors, n_leaves, n_edges;
} sr_level;
typedef struct { float pos[3], vel[3], yaw, pitch, last_height_diff; uint32_t flags; } sr_state;
typedef struct { uint32_t width, height; float scale, half_width, marker; uint32_t flags; } sr_view;

enum { SR_ROTATE = 1, SR_TOP_DOWN = 8 };

/* the sector at (qx, qz): the descent from the root, the void rule, the NaN rule */
static uint32_t sr_sector_at(const sr_level *lv, float qx, float qz) {
  if (qx != qx || qz != qz) return SR_NONE;
  int32_t child = 0;
  const sr_node *n = &lv->nodes[0];
  for (;;) {
    float dist = (qx * n->displace[1] - qz * n->displace[0]) + (n->displace[0] * n->origin[1] - n->displace[1] * n->origin[0]);
    child = dist >= 0.0f ? n->positive : n->negative;
    if (child <= 0) break;
    n = &lv->nodes[child];
  }
  uint32_t leaf = (uint32_t)(-child);
  sr_range r = lv->leaf_edges[leaf];
  for (uint32_t e = r.first; e < r.first + r.count; e++) {
    const sr_edge *g = &lv->edges[e];
    float cross = (qx - g->a[0]) * g->d[1] - (qz - g->a[1]) * g->d[0];
    if (cross > 0.0f) return SR_NONE;
  }
  return lv->leaf_sector[leaf];
}

static float sr_live(float height, uint32_t object, const float *off, uint32_t n_objects) {
  float by = 0.0f;
  if (off && object != 0 && object < n_objects) by = off[3 * (size_t)object + 1];
  return height + by;
}

static void sr_heights(const sr_level *lv, uint32_t s, const float *off, uint32_t n_objects, float *floor, float *ceiling) {
  if (s == SR_NONE) {
    *floor = INFINITY, *ceiling = -INFINITY;
    return;
  }
  *floor = sr_live(lv->sectors[s].floor, lv->sectors[s].floor_id, off, n_objects);
  *ceiling = sr_live(lv->sectors[s].ceiling, lv->sectors[s].ceiling_id, off, n_objects);
}

/* the sectors at n points (x, z pairs) of one level */
void sr_points(const sr_level *lv, const float *xz, uint32_t n, uint32_t *out) {
  for (uint32_t k = 0; k < n; k++) out[k] = sr_sector_at(lv, xz[2 * k], xz[2 * k + 1]);
}

/* the level of player p: levels[0] for everyone without level_of; NULL for a slot outside the set */
static const sr_level *sr_level_of(const sr_level *levels, uint32_t n_slots, const uint32_t *level_of, uint32_t p) {
  if (!level_of) return &levels[0];
  return level_of[p] < n_slots ? &levels[level_of[p]] : NULL;
}

/* every output but sector_out may be NULL; visited is read and written in place */
void sr_locate(const sr_level *levels, uint32_t n_slots, const uint32_t *level_of, const sr_state *st, uint32_t n, const float *offsets,
               uint32_t n_objects, uint32_t *sector_out, float *heights_out, uint32_t *visited, uint32_t stride, uint32_t *new_out) {
  for (uint32_t p = 0; p < n; p++) {
    const sr_level *lv = sr_level_of(levels, n_slots, level_of, p);
    uint32_t s = lv ? sr_sector_at(lv, st[p].pos[0], st[p].pos[2]) : SR_NONE;
    sector_out[p] = s;
    if (heights_out) {
      if (lv) sr_heights(lv, s, offsets ? offsets + (size_t)p * n_objects * 3 : NULL, n_objects, &heights_out[2 * p], &heights_out[2 * p + 1]);
      else heights_out[2 * p] = INFINITY, heights_out[2 * p + 1] = -INFINITY;
    }
    uint32_t fresh = 0;
    if (visited && s != SR_NONE) {
      uint32_t *word = &visited[(size_t)p * stride + s / 32];
      uint32_t bit = 1u << (s % 32);
      fresh = (*word & bit) == 0;
      *word |= bit;
    }
    if (new_out) new_out[p] = fresh;
  }
}

/* the world point of pixel (i, j) of a player's map: the map contract's */
static void sr_point(const sr_view *v, const sr_state *st, float sn, float cs, uint32_t i, uint32_t j, float *qx, float *qz) {
  float hw = (float)v->width * 0.5f, hh = (float)v->height * 0.5f;
  float u = (((float)i + 0.5f) - hw) * v->scale;
  float w = (((float)j + 0.5f) - hh) * v->scale;
  if (v->flags & SR_ROTATE) {
    *qx = (st->pos[0] + cs * u) + (-sn) * w;
    *qz = (st->pos[2] + (-sn) * u) + (-cs) * w;
  } else {
    *qx = st->pos[0] - w;
    *qz = st->pos[2] - u;
  }
}

/* players [first, first + count) of n; each plane n x height x width or NULL; visited: rows of stride words or NULL */
void sr_draw(const sr_level *levels, uint32_t n_slots, const uint32_t *level_of, const sr_state *st, uint32_t n, uint32_t first,
             uint32_t count, const float *offsets, uint32_t n_objects, const sr_view *v, const uint32_t *visited, uint32_t stride,
             uint16_t *sector_out, float *floor_out, float *ceiling_out) {
  for (uint32_t p = first; p < first + count && p < n; p++) {
    const sr_level *lv = sr_level_of(levels, n_slots, level_of, p);
    const float *off = offsets ? offsets + (size_t)p * n_objects * 3 : NULL;
    float sn, cs;
    sincos_restated(st[p].yaw, &sn, &cs);
    for (uint32_t row = 0; row < v->height; row++) {
      uint32_t j = (v->flags & SR_TOP_DOWN) ? v->height - 1 - row : row;
      for (uint32_t i = 0; i < v->width; i++) {
        size_t at = ((size_t)p * v->height + row) * v->width + i;
        uint32_t s = SR_NONE;
        float floor = INFINITY, ceiling = -INFINITY;
        if (lv) {
          float qx, qz;
          sr_point(v, &st[p], sn, cs, i, j, &qx, &qz);
          s = sr_sector_at(lv, qx, qz);
          if (s != SR_NONE && visited && !((visited[(size_t)p * stride + s / 32] >> (s % 32)) & 1u)) s = SR_NONE;
          sr_heights(lv, s, off, n_objects, &floor, &ceiling);
        }
        if (sector_out) sector_out[at] = s >= SR_NONE16 ? SR_NONE16 : (uint16_t)s;
        if (floor_out) floor_out[at] = floor;
        if (ceiling_out) ceiling_out[at] = ceiling;
      }
    }
  }
}
