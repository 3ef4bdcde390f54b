/* Test-side restatement of the seen lines (include/rdoom.h "seen lines"; the product's is rust-doom_amd/csrc/hip/reveal.hip), in
 * binary32, sharing no code with the product and none of its shape: for every player, every ray meets every line of the level,
 * twice -- once for the nearest blocking hit, once for the lines seen up to it -- nothing is culled, staged or skipped, and bits
 * already set are tested like any other.  It reads the HOST line table (rdoom_map_line records as rdoom_world_map_lines lends
 * them).  The sine and cosine of the yaw are the restatements' one definition of the project's sincos
 * (tests/sincos_restatement.h).
 * Built by the tests like the other restatements (tests/reveal_ref.py): gcc -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "sincos_restatement.h"
typedef struct { uint32_t present; float floor, ceiling; uint32_t floor_id, ceiling_id; } rv_side;
typedef struct { uint32_t linedef; float a[2], b[2]; uint32_t flags, special; rv_side front, back; } rv_line;
typedef struct { float pos[3], vel[3], yaw, pitch, last_height_diff; uint32_t flags; } rv_state;

enum { RV_STOP_RANGE = 0, RV_STOP_ONE_SIDED = 1, RV_STOP_TWO_SIDED = 2 };

static float rv_live(float height, uint32_t object, const float *off, uint32_t n_objects) {
  float by = 0.0f;
  if (off && object != 0 && object < n_objects) by = off[3 * (size_t)object + 1];
  return height + by;
}

/* 0: sight passes line l in the game whose offsets are `off`; else which kind of line stops it */
static int rv_blocks(const rv_line *l, const float *off, uint32_t n_objects) {
  if (!(l->front.present == 1 && l->back.present == 1)) return RV_STOP_ONE_SIDED;
  float ff = rv_live(l->front.floor, l->front.floor_id, off, n_objects), fc = rv_live(l->front.ceiling, l->front.ceiling_id, off, n_objects);
  float bf = rv_live(l->back.floor, l->back.floor_id, off, n_objects), bc = rv_live(l->back.ceiling, l->back.ceiling_id, off, n_objects);
  float lo = ff > bf ? ff : bf, hi = fc < bc ? fc : bc;
  return !(hi > lo) ? RV_STOP_TWO_SIDED : 0;
}

/* the contract's ray o + t * vel against the line a -> b */
static int rv_hit(const rv_line *l, float ox, float oz, float velx, float velz, float *t_out) {
  float dx = l->b[0] - l->a[0], dz = l->b[1] - l->a[1];
  float len2 = dx * dx + dz * dz;
  float wx = l->a[0] - ox, wz = l->a[1] - oz;
  float den = velx * dz - velz * dx;
  float t = (wx * dz - wz * dx) / den;
  float u = (wx * velz - wz * velx) / den;
  *t_out = t;
  return len2 > 0.0f && den != 0.0f && u >= 0.0f && u <= 1.0f && t >= 0.0f && t <= 1.0f;
}

/* players [first, first + count) of n.  lines / ranges / levels / n_slots: as automap_restatement.c's am_draw (a slot outside the
 * set: the player's row and count are left as they are, the count as 0).  dirs: n_rays x (right, forward).  seen: n rows of stride
 * words, OR-ed into; new_out: n counts or NULL.  For the tests' own assertions, each NULL or per player and ray: limit_out the
 * T_r, stop_out what stopped the ray (RV_STOP_*), marks_out how many lines the ray sees; and per player and line (rows of
 * witness_stride entries): witness_ray the first ray that sees the line or 0xFFFFFFFF, witness_t its t. */
void rv_reveal(const rv_line *lines, uint32_t n_lines, const uint32_t *ranges, const uint32_t *levels, uint32_t n_slots, const rv_state *st,
               uint32_t n, uint32_t first, uint32_t count, const float *dirs, uint32_t n_rays, float max_range, const float *offsets,
               uint32_t n_objects, uint32_t *seen, uint32_t stride, uint32_t *new_out, float *limit_out, uint8_t *stop_out,
               uint32_t *marks_out, uint32_t *witness_ray, float *witness_t, uint32_t witness_stride) {
  uint8_t *blocks = (uint8_t *)malloc((size_t)n_lines + 1);
  uint8_t *mark = (uint8_t *)malloc((size_t)n_lines + 1);
  for (uint32_t p = first; p < first + count && p < n; p++) {
    if (new_out) new_out[p] = 0;
    const rv_line *mine = lines;
    uint32_t n_mine = n_lines;
    if (ranges) {
      if (levels[p] >= n_slots) continue;
      mine = lines + ranges[2 * levels[p]], n_mine = ranges[2 * levels[p] + 1];
    }
    const float *off = offsets ? offsets + (size_t)p * n_objects * 3 : NULL;
    for (uint32_t l = 0; l < n_mine; l++) blocks[l] = (uint8_t)rv_blocks(&mine[l], off, n_objects), mark[l] = 0;
    if (witness_ray)
      for (uint32_t l = 0; l < n_mine; l++) witness_ray[(size_t)p * witness_stride + l] = 0xFFFFFFFFu;
    float sn, cs;
    sincos_restated(st[p].yaw, &sn, &cs);
    float ox = st[p].pos[0], oz = st[p].pos[2];
    for (uint32_t r = 0; r < n_rays; r++) {
      float right = dirs[2 * r], forward = dirs[2 * r + 1];
      float dirx = cs * right + (-sn) * forward, dirz = (-sn) * right + (-cs) * forward;
      float velx = dirx * max_range, velz = dirz * max_range;
      float limit = 1.0f;
      int stop = RV_STOP_RANGE;
      for (uint32_t l = 0; l < n_mine; l++) {
        float t;
        if (blocks[l] && rv_hit(&mine[l], ox, oz, velx, velz, &t) && t < limit) limit = t, stop = blocks[l];
      }
      uint32_t marks = 0;
      for (uint32_t l = 0; l < n_mine; l++) {
        float t;
        if (rv_hit(&mine[l], ox, oz, velx, velz, &t) && t <= limit) {
          marks++;
          if (!mark[l] && witness_ray) witness_ray[(size_t)p * witness_stride + l] = r, witness_t[(size_t)p * witness_stride + l] = t;
          mark[l] = 1;
        }
      }
      if (limit_out) limit_out[(size_t)p * n_rays + r] = limit;
      if (stop_out) stop_out[(size_t)p * n_rays + r] = (uint8_t)stop;
      if (marks_out) marks_out[(size_t)p * n_rays + r] = marks;
    }
    uint32_t fresh = 0;
    for (uint32_t l = 0; l < n_mine; l++) {
      uint32_t *word = seen + (size_t)p * stride + l / 32, bit = 1u << (l % 32);
      if (mark[l] && !(*word & bit)) *word |= bit, fresh++;
    }
    if (new_out) new_out[p] = fresh;
  }
  free(blocks);
  free(mark);
}
