/* Test-side restatement of the top-down map (include/rdoom.h "top-down maps"; the product's is
 * rust-doom_amd/csrc/hip/automap.hip), in binary32, sharing no code with the product and none of its shape: every line of the
 * level is tried against every pixel, nothing is culled, nothing is chunked.  It reads the HOST line table (rdoom_map_line records
 * as rdoom_world_map_lines lends them), not the kernel's arrays.  The sine and cosine of the yaw are the restatements' one definition of
 * the project's sincos (tests/sincos_restatement.h).
 * Built by the tests like the other restatements (tests/automap_ref.py): gcc -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "sincos_restatement.h"
typedef struct { uint32_t present; float floor, ceiling; uint32_t floor_id, ceiling_id; } am_side;
typedef struct { uint32_t linedef; float a[2], b[2]; uint32_t flags, special; am_side front, back; } am_line;
typedef struct { float pos[3], vel[3], yaw, pitch, last_height_diff; uint32_t flags; } am_state;
typedef struct { uint32_t width, height; float scale, half_width, marker; uint32_t flags; } am_view;

enum { AM_ROTATE = 1, AM_SHOW_FLAT = 2, AM_SHOW_HIDDEN = 4, AM_TOP_DOWN = 8 };
enum { AM_NONE = 0, AM_FLAT = 1, AM_CEILING_STEP = 2, AM_FLOOR_STEP = 3, AM_CLOSED = 4, AM_ONE_SIDED = 5, AM_PLAYER = 8 };

/* the contract's dist2 in its two halves: what depends on the segment a -> b alone (ok: it has a length), and the squared
 * distance of (qx, qz) from it */
typedef struct { float ax, az, dx, dz, inv; int ok; } am_seg;
static am_seg am_segment(float ax, float az, float bx, float bz) {
  am_seg g;
  g.ax = ax, g.az = az;
  g.dx = bx - ax, g.dz = bz - az;
  float len2 = g.dx * g.dx + g.dz * g.dz;
  g.ok = len2 > 0.0f;
  g.inv = 1.0f / len2;
  return g;
}
static float am_dist2(float qx, float qz, const am_seg *g) {
  float wx = qx - g->ax, wz = qz - g->az;
  float t = (wx * g->dx + wz * g->dz) * g->inv;
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  float ex = wx - t * g->dx, ez = wz - t * g->dz;
  return ex * ex + ez * ez;
}

static float am_live(float height, uint32_t object, const float *off, uint32_t n_objects) {
  float by = 0.0f;
  if (off && object != 0 && object < n_objects) by = off[3 * (size_t)object + 1];
  return height + by;
}

/* the class of line l for a player whose object offsets are `off` (NULL: at rest); 0 = not drawn under this view */
static uint32_t am_class(const am_line *l, const float *off, uint32_t n_objects, uint32_t vflags) {
  if ((l->flags & 0x80u) && !(vflags & AM_SHOW_HIDDEN)) return AM_NONE;
  if (!(l->front.present == 1 && l->back.present == 1) || (l->flags & 0x20u)) return AM_ONE_SIDED;
  float ff = am_live(l->front.floor, l->front.floor_id, off, n_objects), fc = am_live(l->front.ceiling, l->front.ceiling_id, off, n_objects);
  float bf = am_live(l->back.floor, l->back.floor_id, off, n_objects), bc = am_live(l->back.ceiling, l->back.ceiling_id, off, n_objects);
  if (fc <= ff || bc <= bf) return AM_CLOSED;
  if (ff != bf) return AM_FLOOR_STEP;
  if (fc != bc) return AM_CEILING_STEP;
  return (vflags & AM_SHOW_FLAT) ? AM_FLAT : AM_NONE;
}

/* the classes of n_lines lines for one player (what am_draw uses), for the tests' censuses */
void am_classes(const am_line *lines, uint32_t n_lines, const float *off, uint32_t n_objects, uint32_t vflags, uint8_t *out) {
  for (uint32_t l = 0; l < n_lines; l++) out[l] = (uint8_t)am_class(&lines[l], off, n_objects, vflags);
}

/* the world point of pixel (i, j) of a player's map */
static void am_point(const am_view *v, const am_state *st, float sn, float cs, uint32_t i, uint32_t j, float *qx, float *qz) {
  float hw = (float)v->width * 0.5f, hh = (float)v->height * 0.5f;
  float u = (((float)i + 0.5f) - hw) * v->scale;
  float w = (((float)j + 0.5f) - hh) * v->scale;
  if (v->flags & AM_ROTATE) {
    *qx = (st->pos[0] + cs * u) + (-sn) * w;
    *qz = (st->pos[2] + (-sn) * u) + (-cs) * w;
  } else {
    *qx = st->pos[0] - w;
    *qz = st->pos[2] - u;
  }
}

/* players [first, first + count) of n.  lines: the table of the player's level -- `ranges` NULL: all n_lines of it for everyone;
 * else ranges[2 s], ranges[2 s + 1] = first line and count of slot s, levels[p] the player's slot, n_slots the set's size (a slot
 * outside it: an all-zero map).  offsets: n x n_objects x xyz or NULL.  out: n x height x width bytes. */
void am_draw(const am_line *lines, uint32_t n_lines, const uint32_t *ranges, const uint32_t *levels, uint32_t n_slots, const am_state *st,
             uint32_t n, uint32_t first, uint32_t count, const float *offsets, uint32_t n_objects, const am_view *v, uint8_t *out) {
  float reach = v->half_width * v->scale;
  float reach2 = reach * reach;
  /* per player: the lines that are drawn at all (a class, a length) with what dist2 computes of the line alone -- d, inv -- and
   * their classes, so that the loop over the pixels is short; every pixel still meets every such line */
  float *geo = (float *)malloc(((size_t)n_lines + 1) * 5 * sizeof(float));
  uint8_t *cls = (uint8_t *)malloc((size_t)n_lines + 1);
  float *rowx = (float *)malloc((size_t)v->width * sizeof(float)), *rowz = (float *)malloc((size_t)v->width * sizeof(float));
  for (uint32_t p = first; p < first + count && p < n; p++) {
    uint8_t *map = out + (size_t)p * v->height * v->width;
    memset(map, 0, (size_t)v->height * v->width);
    const am_line *mine = lines;
    uint32_t n_mine = n_lines;
    if (ranges) {
      if (levels[p] >= n_slots) continue;
      mine = lines + ranges[2 * levels[p]], n_mine = ranges[2 * levels[p] + 1];
    }
    const float *off = offsets ? offsets + (size_t)p * n_objects * 3 : NULL;
    uint32_t drawn = 0;
    for (uint32_t l = 0; l < n_mine; l++) {
      uint32_t c = am_class(&mine[l], off, n_objects, v->flags);
      am_seg g = am_segment(mine[l].a[0], mine[l].a[1], mine[l].b[0], mine[l].b[1]);
      if (c == AM_NONE || !g.ok) continue;
      float *to = geo + 5 * (size_t)drawn;
      to[0] = g.ax, to[1] = g.az, to[2] = g.dx, to[3] = g.dz, to[4] = g.inv;
      cls[drawn++] = (uint8_t)c;
    }
    float sn, cs;
    sincos_restated(st[p].yaw, &sn, &cs);
    float mark = v->marker * v->scale;
    am_seg tip = am_segment(st[p].pos[0], st[p].pos[2], st[p].pos[0] + (-sn) * (2.0f * mark), st[p].pos[2] + (-cs) * (2.0f * mark));
    for (uint32_t row = 0; row < v->height; row++) {
      uint32_t j = (v->flags & AM_TOP_DOWN) ? v->height - 1 - row : row;
      uint8_t *out_row = map + (size_t)row * v->width;
      for (uint32_t i = 0; i < v->width; i++) am_point(v, &st[p], sn, cs, i, j, &rowx[i], &rowz[i]);
      for (uint32_t l = 0; l < drawn; l++) { /* line by line along the row: the value is a maximum, the order is free */
        const float *g = geo + 5 * (size_t)l;
        const am_seg sg = {g[0], g[1], g[2], g[3], g[4], 1};
        const uint8_t c = cls[l];
        for (uint32_t i = 0; i < v->width; i++) {
          uint8_t covered = am_dist2(rowx[i], rowz[i], &sg) <= reach2;
          out_row[i] = (covered && c > out_row[i]) ? c : out_row[i];
        }
      }
      if (v->marker > 0.0f && tip.ok)
        for (uint32_t i = 0; i < v->width; i++)
          if (am_dist2(rowx[i], rowz[i], &tip) <= mark * mark) out_row[i] = AM_PLAYER;
    }
  }
  free(rowx);
  free(rowz);
  free(geo);
  free(cls);
}

/* the world points of a player's pixels, for the test of the axes: out 2 floats (x, z) per pixel, rows as in the map */
void am_points(const am_view *v, const am_state *st, float *out) {
  float sn, cs;
  sincos_restated(st->yaw, &sn, &cs);
  for (uint32_t row = 0; row < v->height; row++)
    for (uint32_t i = 0; i < v->width; i++) {
      uint32_t j = (v->flags & AM_TOP_DOWN) ? v->height - 1 - row : row;
      am_point(v, st, sn, cs, i, j, out + 2 * ((size_t)row * v->width + i), out + 2 * ((size_t)row * v->width + i) + 1);
    }
}
