/* Test-side restatement of the explored area (include/rdoom.h "explored area"; the product's is rust-doom_amd/csrc/hip/area.hip), in
 * binary32, sharing no code with the product and none of its shape: for every player, every ray meets every line of the level for
 * its nearest blocking hit -- nothing is culled -- and then every one of its n_steps + 1 samples is taken in turn, into planes of one
 * byte per cell of the whole grid, which are packed into the caller's words at the end: no window, no bands, no chunks.  It reads
 * the HOST line table (rdoom_map_line records as rdoom_world_map_lines lends them) and derives the grid from it with its own
 * formulas.  The sine and cosine of the yaw are the restatements' one definition of the project's sincos
 * (tests/sincos_restatement.h).
 * Built by the tests like the other restatements (tests/area_ref.py): gcc -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "sincos_restatement.h"
typedef struct { uint32_t present; float floor, ceiling; uint32_t floor_id, ceiling_id; } ar_side;
typedef struct { uint32_t linedef; float a[2], b[2]; uint32_t flags, special; ar_side front, back; } ar_line;
typedef struct { float pos[3], vel[3], yaw, pitch, last_height_diff; uint32_t flags; } ar_state;
typedef struct { int32_t ix0, iz0; uint32_t gw, gh, pitch, words; } ar_grid_t;

static float ar_live(float height, uint32_t object, const float *off, uint32_t n_objects) {
  float by = 0.0f;
  if (off && object != 0 && object < n_objects) by = off[3 * (size_t)object + 1];
  return height + by;
}

static int ar_blocks(const ar_line *l, const float *off, uint32_t n_objects) {
  if (!(l->front.present == 1 && l->back.present == 1)) return 1;
  float ff = ar_live(l->front.floor, l->front.floor_id, off, n_objects), fc = ar_live(l->front.ceiling, l->front.ceiling_id, off, n_objects);
  float bf = ar_live(l->back.floor, l->back.floor_id, off, n_objects), bc = ar_live(l->back.ceiling, l->back.ceiling_id, off, n_objects);
  float lo = ff > bf ? ff : bf, hi = fc < bc ? fc : bc;
  return !(hi > lo);
}

static int ar_hit(const ar_line *l, float ox, float oz, float velx, float velz, float *t_out) {
  float dx = l->b[0] - l->a[0], dz = l->b[1] - l->a[1];
  float len2 = dx * dx + dz * dz;
  float wx = l->a[0] - ox, wz = l->a[1] - oz;
  float den = velx * dz - velz * dx;
  float t = (wx * dz - wz * dx) / den;
  float u = (wx * velz - wz * velx) / den;
  *t_out = t;
  return len2 > 0.0f && den != 0.0f && u >= 0.0f && u <= 1.0f && t >= 0.0f && t <= 1.0f;
}

/* the quotient's floor as a 64-bit integer; 0: the quotient is not finite and below 2^30 in magnitude */
static int ar_cx(float x, float cell, int64_t *c) {
  float q = x / cell;
  if (!(fabsf(q) < 1073741824.0f)) return 0;
  *c = (int64_t)floorf(q);
  return 1;
}

/* the grid of a table at `cell`; returns 0 when a bound's quotient is out of range (the limits on gw, gh and words are the caller's
 * to judge: every field is written) */
int ar_grid(const ar_line *lines, uint32_t n_lines, float cell, ar_grid_t *g) {
  float minx = 0.0f, maxx = 0.0f, minz = 0.0f, maxz = 0.0f;
  for (uint32_t l = 0; l < n_lines; l++)
    for (int e = 0; e < 2; e++) {
      float x = e ? lines[l].b[0] : lines[l].a[0], z = e ? lines[l].b[1] : lines[l].a[1];
      if (l == 0 && e == 0) minx = maxx = x, minz = maxz = z;
      if (x < minx) minx = x;
      if (x > maxx) maxx = x;
      if (z < minz) minz = z;
      if (z > maxz) maxz = z;
    }
  int64_t x0, x1, z0, z1;
  memset(g, 0, sizeof *g);
  if (!(ar_cx(minx, cell, &x0) && ar_cx(maxx, cell, &x1) && ar_cx(minz, cell, &z0) && ar_cx(maxz, cell, &z1))) return 0;
  g->ix0 = (int32_t)(x0 - 1), g->iz0 = (int32_t)(z0 - 1);
  g->gw = (uint32_t)(x1 + 1 - (x0 - 1) + 1), g->gh = (uint32_t)(z1 + 1 - (z0 - 1) + 1);
  g->pitch = (g->gw + 31) / 32;
  g->words = g->gh * g->pitch;
  return 1;
}

/* the cell of (x, z) as an index iz * gw + ix into a byte plane, or -1 for none */
static int64_t ar_cell(const ar_grid_t *g, float cell, float x, float z) {
  int64_t cx, cz;
  if (!(ar_cx(x, cell, &cx) && ar_cx(z, cell, &cz))) return -1;
  int64_t ix = cx - g->ix0, iz = cz - g->iz0;
  if (ix < 0 || iz < 0 || ix >= (int64_t)g->gw || iz >= (int64_t)g->gh) return -1;
  return iz * (int64_t)g->gw + ix;
}

/* players [first, first + count) of n.  lines / ranges / levels / n_slots: as reveal_restatement.c's rv_reveal (a slot outside the
 * set: the player's rows are left as they are, the counts are 0).  dirs: n_rays x (right, forward).  area: n x 2 x stride words,
 * OR-ed into; new_out: n x 2 counts or NULL.  For the tests' own assertions, each NULL or: limit_out per player and ray the T_r;
 * free_witness per player and cell (rows of witness_stride cells, two entries each) the first (ray, step) that set the FREE byte
 * or 0xFFFFFFFF; wall_witness per player and cell the first ray whose stop set the WALL byte or 0xFFFFFFFF. */
void ar_reveal(const ar_line *lines, uint32_t n_lines, const uint32_t *ranges, const uint32_t *levels, uint32_t n_slots, const ar_state *st,
               uint32_t n, uint32_t first, uint32_t count, const float *dirs, uint32_t n_rays, float max_range, const float *offsets,
               uint32_t n_objects, float cell, uint32_t n_steps, uint32_t *area, uint32_t stride, uint32_t *new_out, float *limit_out,
               uint32_t *free_witness, uint32_t *wall_witness, uint32_t witness_stride) {
  uint8_t *blocks = (uint8_t *)malloc((size_t)n_lines + 1);
  for (uint32_t p = first; p < first + count && p < n; p++) {
    if (new_out) new_out[2 * p] = new_out[2 * p + 1] = 0;
    const ar_line *mine = lines;
    uint32_t n_mine = n_lines;
    if (ranges) {
      if (levels[p] >= n_slots) continue;
      mine = lines + ranges[2 * levels[p]], n_mine = ranges[2 * levels[p] + 1];
    }
    ar_grid_t g;
    if (!ar_grid(mine, n_mine, cell, &g)) continue;
    const size_t cells = (size_t)g.gw * g.gh;
    uint8_t *plane = (uint8_t *)calloc(2 * cells + 1, 1);
    const float *off = offsets ? offsets + (size_t)p * n_objects * 3 : NULL;
    for (uint32_t l = 0; l < n_mine; l++) blocks[l] = (uint8_t)ar_blocks(&mine[l], off, n_objects);
    if (free_witness)
      for (size_t k = 0; k < cells; k++) free_witness[((size_t)p * witness_stride + k) * 2] = free_witness[((size_t)p * witness_stride + k) * 2 + 1] = 0xFFFFFFFFu;
    if (wall_witness)
      for (size_t k = 0; k < cells; k++) wall_witness[(size_t)p * witness_stride + k] = 0xFFFFFFFFu;
    float sn, cs;
    sincos_restated(st[p].yaw, &sn, &cs);
    float ox = st[p].pos[0], oz = st[p].pos[2];
    for (uint32_t r = 0; r < n_rays; r++) {
      float right = dirs[2 * r], forward = dirs[2 * r + 1];
      float dirx = cs * right + (-sn) * forward, dirz = (-sn) * right + (-cs) * forward;
      float velx = dirx * max_range, velz = dirz * max_range;
      float limit = 1.0f;
      for (uint32_t l = 0; l < n_mine; l++) {
        float t;
        if (blocks[l] && ar_hit(&mine[l], ox, oz, velx, velz, &t) && t < limit) limit = t;
      }
      if (limit_out) limit_out[(size_t)p * n_rays + r] = limit;
      for (uint32_t k = 0; k <= n_steps; k++) {
        float t = (float)k / (float)n_steps;
        if (!(t <= limit)) continue;
        float x = ox + t * velx, z = oz + t * velz;
        int64_t at = ar_cell(&g, cell, x, z);
        if (at < 0) continue;
        if (!plane[at] && free_witness) free_witness[((size_t)p * witness_stride + at) * 2] = r, free_witness[((size_t)p * witness_stride + at) * 2 + 1] = k;
        plane[at] = 1;
      }
      if (limit < 1.0f) {
        float x = ox + limit * velx, z = oz + limit * velz;
        int64_t at = ar_cell(&g, cell, x, z);
        if (at >= 0) {
          if (!plane[cells + at] && wall_witness) wall_witness[(size_t)p * witness_stride + at] = r;
          plane[cells + at] = 1;
        }
      }
    }
    for (int which = 0; which < 2; which++) {
      uint32_t *row = area + ((size_t)p * 2 + which) * stride, fresh = 0;
      for (uint32_t iz = 0; iz < g.gh; iz++)
        for (uint32_t ix = 0; ix < g.gw; ix++) {
          uint32_t *word = row + (size_t)iz * g.pitch + ix / 32, bit = 1u << (ix % 32);
          if (plane[which * cells + (size_t)iz * g.gw + ix] && !(*word & bit)) *word |= bit, fresh++;
        }
      if (new_out) new_out[2 * p + which] = fresh;
    }
    free(plane);
  }
  free(blocks);
}

/* the maps drawn through the rows, players [first, first + count) of n: out is n x height x width bytes, free | wall << 1 of the cell
 * of the pixel's point (the map contract's "Pixel to world", written out here), 0 outside the grid and for a slot outside the set.
 * rotate / top_down: the view's two flags */
void ar_draw(const ar_line *lines, uint32_t n_lines, const uint32_t *ranges, const uint32_t *levels, uint32_t n_slots, const ar_state *st,
             uint32_t n, uint32_t first, uint32_t count, uint32_t width, uint32_t height, float scale, int rotate, int top_down, float cell,
             const uint32_t *area, uint32_t stride, uint8_t *out) {
  for (uint32_t p = first; p < first + count && p < n; p++) {
    uint8_t *map = out + (size_t)p * width * height;
    memset(map, 0, (size_t)width * height);
    const ar_line *mine = lines;
    uint32_t n_mine = n_lines;
    if (ranges) {
      if (levels[p] >= n_slots) continue;
      mine = lines + ranges[2 * levels[p]], n_mine = ranges[2 * levels[p] + 1];
    }
    ar_grid_t g;
    if (!ar_grid(mine, n_mine, cell, &g)) continue;
    float sn, cs;
    sincos_restated(st[p].yaw, &sn, &cs);
    float px = st[p].pos[0], pz = st[p].pos[2];
    float hw = (float)width * 0.5f, hh = (float)height * 0.5f;
    const uint32_t *free_row = area + (size_t)p * 2 * stride, *wall_row = free_row + stride;
    for (uint32_t row = 0; row < height; row++)
      for (uint32_t i = 0; i < width; i++) {
        int32_t j = top_down ? (int32_t)height - 1 - (int32_t)row : (int32_t)row;
        float u = (((float)i + 0.5f) - hw) * scale, v = (((float)j + 0.5f) - hh) * scale;
        float qx, qz;
        if (rotate) qx = (px + cs * u) + (-sn) * v, qz = (pz + (-sn) * u) + (-cs) * v;
        else qx = px - v, qz = pz - u;
        int64_t cxx, czz;
        if (!(ar_cx(qx, cell, &cxx) && ar_cx(qz, cell, &czz))) continue;
        int64_t ix = cxx - g.ix0, iz = czz - g.iz0;
        if (ix < 0 || iz < 0 || ix >= (int64_t)g.gw || iz >= (int64_t)g.gh) continue;
        size_t at = (size_t)iz * g.pitch + (size_t)ix / 32;
        map[(size_t)row * width + i] = (uint8_t)(((free_row[at] >> (ix % 32)) & 1u) | (((wall_row[at] >> (ix % 32)) & 1u) << 1));
      }
  }
}
