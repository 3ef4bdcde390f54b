/* Range-sensor rays that see things: a level's things as vertical cylinders, met by the rays of rdoom_world_cast_rays after the
 * world cast.  A public header of its own beside rdoom.h, whose 135 functions stay as they are; the two
 * entry points below are exported by the same library.  The reference has no counterpart: this header is the authority.
 *
 * rdoom_world_cast_rays_things / rdoom_worldset_cast_rays_things are a second pass after rdoom_world_cast_rays, not a change to it:
 * they take the fractions it wrote, or none, and shorten every ray that meets a thing first.  n players, n_rays rays each; ray
 * q = p * n_rays + r is ray r of player p.  Player p is in level L: the world's one level, or slot d_levels[p] of the set and level
 * L of `things` (the relation of handle and thing set is rdoom_world_sense_things'); L has T things.
 *
 * Arithmetic.  Binary32, every operation rounded once, nothing contracted, IEEE division and sqrtf.  a * b + c * d means
 * round(round(a * b) + round(c * d)).  A comparison with a NaN is false.
 *
 * The ray.  O and V are the `origin` and `vel` rdoom_world_cast_rays computes for (p, r) -- what it writes to d_origin_out and
 * d_vel_out -- bit for bit: the player's quaternion and camera eye from d_states[p], the eye as O, and the rotated d_dirs[r] times
 * max_range as V.  A ray with a component of O or V that is not finite, or with V == (0, 0, 0), meets no thing.
 *
 * Which things.  Thing i < T of L is tried when all of these hold: its bit is set in row L of d_select (levels x stride words;
 * NULL: every thing; the bits of rdoom_world_thing_obstacles give the obstacles only); its bit is clear in row p of d_hidden
 * (n x stride words, rdoom_world_sense_things' d_collected as it stands; NULL: nothing is hidden); bit (category & 0xFF) of
 * params->category_mask is set; and R = radius + grow satisfies R > 0.  Bit i is bit i % 32 of word row * stride + i / 32; only
 * words [0, ceil(T / 32)) of a row are read, and none is written.
 *
 * Its shape.  A vertical cylinder about (x, z) of radius R.  y = base + off(object_id), off() the map contract's on row p of
 * d_object_offsets (NULL: at rest): the y of the object's row, 0 for object 0 and objects beyond the row.
 * h = params->height[category & 0xFF].  Standing: bottom = y, top = y + h.  With RDOOM_THING_HANGING: top = y, bottom = y - h.
 *
 * The hit.
 *   cx = O.x - x;  cz = O.z - z;  a = V.x * V.x + V.z * V.z;  b = cx * V.x + cz * V.z;  cc = (cx * cx + cz * cz) - R * R;
 *   in plan:   a > 0:    disc = b * b - a * cc;  no hit unless disc >= 0;  s = sqrtf(disc);  h0 = (-b - s) / a;  h1 = (-b + s) / a;
 *              else:     no hit unless cc <= 0;  h0 = -inf;  h1 = +inf;
 *   in height: V.y != 0: u0 = (bottom - O.y) / V.y;  u1 = (top - O.y) / V.y;  v0 = u1 < u0 ? u1 : u0;  v1 = u1 < u0 ? u0 : u1;
 *              else:     no hit unless O.y >= bottom && O.y <= top;  v0 = -inf;  v1 = +inf;
 *   t = h0 < v0 ? v0 : h0;   t = t > 0 ? t : +0.0f;   e = v1 < h1 ? v1 : h1;
 *   hit when t <= e && t <= 1.
 * An eye inside a thing gives t = 0.  The caps are hit from above and below.  With h = +inf the cylinder has no top, and no bottom
 * when hanging.
 *
 * The fold.  Among the things hit, the smallest t wins, and the lowest index among equal t: the minimum of the key
 * bits(t) << 32 | i (a non-negative binary32 orders as its bits), so the result cannot depend on visiting order, culling or
 * chunking.  current = d_frac_in[q], or +inf when d_frac_in is NULL.  The thing replaces current only when t < current, strictly:
 * the world wins a tie, and a NaN passes through.  d_frac_out[q] is the thing's t or current, bit for bit; d_thing_out[q] (int32,
 * may be NULL) is the thing's index or -1.  d_frac_out may be the very pointer d_frac_in: in place.  Any other overlap of their
 * n x n_rays x 4 bytes is an error.  The rows are read and never written.  A slot at or beyond the set is seen on the device only:
 * that player's rays get current and -1, and nothing else is written.
 *
 * One launch, asynchronous on `stream`; nothing is allocated, nothing is copied and nothing waits, so the call can be captured
 * into a graph.  n == 0 queues nothing.
 *
 * Errors, all RDOOM_BAD_ARG and all checked before anything is queued.  What needs no handle: a NULL thing set, params or d_dirs; (n > 0)
 * NULL d_states, d_frac_out or (the set's call) d_levels; n_rays == 0; max_range not finite or not positive; a height[c] that is a NaN or negative; grow not
 * finite or negative; flags not 0; bits of category_mask above 7; n x n_rays above 2^31; a partial overlap of d_frac_in and
 * d_frac_out.  Then what reads the handle: a NULL handle; one created with RDOOM_WORLD_HOST_ONLY or living on another device.
 * Then what reads the thing set: a set whose levels are not as many as the handle's or that lives on another device; a stride smaller than the set's words while d_select or d_hidden is given; n_objects smaller than the
 * game's objects, or not above the set's largest object_id, while d_object_offsets is given. */
#ifndef RDOOM_RAYS_H
#define RDOOM_RAYS_H

#include "rdoom.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdoom_ray_things {
  float height[8];        /* per category (low byte of rdoom_thing.category): how tall a thing of it stands; >= 0, +inf allowed */
  float grow;             /* added to every thing's radius; finite, >= 0 */
  uint32_t category_mask; /* bit c set: things of category c are seen */
  uint32_t flags;         /* 0 */
} rdoom_ray_things;       /* 44 bytes */

rdoom_status rdoom_world_cast_rays_things(const rdoom_world *world, const rdoom_thingset *things, const rdoom_player_state *d_states,
                                          uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                                          const float *d_object_offsets, uint32_t n_objects, const rdoom_ray_things *params,
                                          const uint32_t *d_select, const uint32_t *d_hidden, uint32_t stride, const float *d_frac_in,
                                          float *d_frac_out, int32_t *d_thing_out, void *stream);
rdoom_status rdoom_worldset_cast_rays_things(const rdoom_worldset *set, const rdoom_thingset *things,
                                             const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                             const float *d_dirs, uint32_t n_rays, float max_range, const float *d_object_offsets,
                                             uint32_t n_objects, const rdoom_ray_things *params, const uint32_t *d_select,
                                             const uint32_t *d_hidden, uint32_t stride, const float *d_frac_in, float *d_frac_out,
                                             int32_t *d_thing_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RDOOM_RAYS_H */
