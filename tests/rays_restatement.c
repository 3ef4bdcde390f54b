/* Test-side restatement of the ray cast (include/rdoom.h "ray casts"; the product's is rust-doom_amd/csrc/hip/world.hip
 * cast_rays_kernel), in binary32, sharing no code with the product.  On world_restatement.c's world: the walk of
 * World::sweep_sphere (game/src/world.rs:40-82) with Node::intersect_sphere at radius 0, and against each triangle the plane
 * branch of Sphere::sweep_triangle (math/src/sphere.rs:16-53) at radius 0 with is_point_inside_triangle (:178-183).  The camera
 * eye and the player's quaternion (game/src/player.rs:325-335, cgmath's Quaternion::from(Euler) and rotate_vector) are written
 * here on their own, not taken from frames_restatement.c: tests/test_rays_host.py shows that the two agree bit for bit.
 * Built by the tests like world_restatement.c (tests/rays_ref.py). */
#include "world_restatement.c"

typedef struct { float re, i, j, k; } ry_quat;

/* Quaternion::from(Euler { x: pitch, y: yaw, z: 0 }): cgmath's conversion on half angles, its products written out */
static ry_quat ry_orientation(float yaw, float pitch) {
  float sin_p, cos_p, sin_y, cos_y;
  rs_sincos(pitch * 0.5f, &sin_p, &cos_p);
  rs_sincos(yaw * 0.5f, &sin_y, &cos_y);
  const float sin_r = 0.0f, cos_r = 1.0f; /* the roll's half angle is 0 */
  ry_quat q;
  q.re = -sin_p * sin_y * sin_r + cos_p * cos_y * cos_r;
  q.i = sin_p * cos_y * cos_r + sin_y * sin_r * cos_p;
  q.j = -sin_p * sin_r * cos_y + sin_y * cos_p * cos_r;
  q.k = sin_p * sin_y * cos_r + sin_r * cos_p * cos_y;
  return q;
}

/* q * v (cgmath: tmp = q.v x v + v * q.s; q.v x tmp * 2 + v), component by component */
static void ry_turn(ry_quat q, const float v[3], float out[3]) {
  float ax = q.j * v[2] - q.k * v[1], ay = q.k * v[0] - q.i * v[2], az = q.i * v[1] - q.j * v[0];
  float tx = ax + v[0] * q.re, ty = ay + v[1] * q.re, tz = az + v[2] * q.re;
  float bx = q.j * tz - q.k * ty, by = q.k * tx - q.i * tz, bz = q.i * ty - q.j * tx;
  out[0] = bx * 2.0f + v[0], out[1] = by * 2.0f + v[1], out[2] = bz * 2.0f + v[2];
}

/* the `disp` of player.concat(camera): rot.rotate(camera.disp * scale) + disp, camera.disp = (0, 0.12, 0), scale 1 */
static void ry_eye_of(const pstate *s, ry_quat q, float eye[3]) {
  float cam[3] = {0.0f * 1.0f, 0.12f * 1.0f, 0.0f * 1.0f}, turned[3];
  ry_turn(q, cam, turned);
  for (int k = 0; k < 3; k++) eye[k] = turned[k] + s->pos[k];
}

/* n states -> n eyes (xyz) and n quaternions (s, x, y, z) */
void ry_eyes(const pstate *st, uint32_t n, float *eyes, float *quats) {
  for (uint32_t p = 0; p < n; p++) {
    ry_quat q = ry_orientation(st[p].yaw, st[p].pitch);
    ry_eye_of(&st[p], q, eyes + 3 * (size_t)p);
    quats[4 * (size_t)p] = q.re, quats[4 * (size_t)p + 1] = q.i, quats[4 * (size_t)p + 2] = q.j, quats[4 * (size_t)p + 3] = q.k;
  }
}

/* What the view of such a camera holds in its translation: inverse_transform's d = rot.invert().rotate(disp) * -(1 / scale), with
 * rot = q * identity and disp the eye (engine/src/renderer.rs:78-87).  Lets a test compare these eyes with the modelviews of
 * frames_restatement.c, which never exposes its eye. */
void ry_view_translations(const pstate *st, uint32_t n, float *out) {
  for (uint32_t p = 0; p < n; p++) {
    ry_quat q = ry_orientation(st[p].yaw, st[p].pitch);
    float eye[3];
    ry_eye_of(&st[p], q, eye);
    ry_quat one = {1.0f, 0.0f, 0.0f, 0.0f}, rot, inv;
    rot.re = q.re * one.re - q.i * one.i - q.j * one.j - q.k * one.k;
    rot.i = q.re * one.i + q.i * one.re + q.j * one.k - q.k * one.j;
    rot.j = q.re * one.j + q.j * one.re + q.k * one.i - q.i * one.k;
    rot.k = q.re * one.k + q.k * one.re + q.i * one.j - q.j * one.i;
    float norm2 = rot.re * rot.re + ((rot.i * rot.i + rot.j * rot.j) + rot.k * rot.k);
    inv.re = rot.re / norm2, inv.i = -rot.i / norm2, inv.j = -rot.j / norm2, inv.k = -rot.k / norm2;
    float turned[3], back = 1.0f / (1.0f * 1.0f);
    ry_turn(inv, eye, turned);
    for (int k = 0; k < 3; k++) out[3 * (size_t)p + k] = turned[k] * -back;
  }
}

typedef struct { float time; uint32_t tri; } ry_hit;

static float ry_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* the triangles [start, end) against the ray from o along unit u (speed = |vel|): the fold of World::sweep_chunk */
static void ry_range(const world_t *w, ry_hit *first, uint32_t start, uint32_t end, const float o[3], const float u[3], float speed) {
  for (uint32_t i = start; i < end; i++) {
    const tri_t *t = &w->tris[i];
    const float *a = w->verts + 3 * t->a, *b = w->verts + 3 * t->b, *c = w->verts + 3 * t->c, *nrm = w->verts + 3 * t->n;
    float facing = ry_dot(nrm, u);
    if (facing >= 0.0f) continue;
    float intercept = -ry_dot(a, nrm);
    float height = ry_dot(o, nrm) + intercept;
    if (height < 0.0f) continue;
    float distance = -height / facing;
    float at[3] = {o[0] + u[0] * distance, o[1] + u[1] * distance, o[2] + u[2] * distance};
    /* is_point_inside_triangle: barycentric coordinates from cross products with the (unnormalised) normal */
    float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    float m[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    float r[3] = {at[0] - a[0], at[1] - a[1], at[2] - a[2]};
    float m2 = ry_dot(m, m);
    float c1[3] = {e1[1] * r[2] - e1[2] * r[1], e1[2] * r[0] - e1[0] * r[2], e1[0] * r[1] - e1[1] * r[0]};
    float c2[3] = {r[1] * e2[2] - r[2] * e2[1], r[2] * e2[0] - r[0] * e2[2], r[0] * e2[1] - r[1] * e2[0]};
    float gamma = ry_dot(c1, m) / m2;
    float beta = ry_dot(c2, m) / m2;
    float alpha = 1.0f - gamma - beta;
    if (!(0.0f <= alpha && alpha <= 1.0f && 0.0f <= gamma && gamma <= 1.0f && 0.0f <= beta && beta <= 1.0f)) continue;
    float time = distance / speed;
    if (!(first->time < time)) first->time = time, first->tri = i; /* the later candidate wins a tie */
  }
}

static ry_hit ry_through(const world_t *w, const float o[3], const float vel[3], const float *offsets) {
  ry_hit first = {INFINITY, 0xFFFFFFFFu};
  float speed = sqrtf(ry_dot(vel, vel));
  if (speed == 0.0f) return first; /* sweep_triangle: None for every triangle */
  float u[3] = {vel[0] / speed, vel[1] / speed, vel[2] / speed};
  float endx = o[0] + vel[0], endz = o[2] + vel[2];
  uint32_t *pending = (uint32_t *)malloc(((size_t)w->n_nodes + 2) * sizeof(uint32_t)), top = 0; /* World::node_stack */
  pending[top++] = 0;
  while (top) {
    const node_t *nd = &w->nodes[pending[--top]];
    /* Node::intersect_sphere (world.rs:165-196) with radius 0: Line2::signed_distance of both ends of the ray */
    float base = nd->dx * nd->oy - nd->dy * nd->ox;
    float from = (o[0] * nd->dy - o[2] * nd->dx) + base, to = (endx * nd->dy - endz * nd->dx) + base;
    for (int side = 0; side < 2; side++) { /* the positive child first */
      if (side == 0 ? !(from >= -0.0f || to >= -0.0f) : !(from <= 0.0f || to <= 0.0f)) continue;
      int32_t child = side == 0 ? nd->pos : nd->neg;
      if (child > 0) pending[top++] = (uint32_t)child; /* (each node is pushed at most once: n_nodes slots hold them all) */
      else ry_range(w, &first, w->chunks[-child].start, w->chunks[-child].end, o, u, speed);
    }
  }
  free(pending);
  for (uint32_t d = 0; d < w->n_dyn; d++) { /* the inverse of a pure translation: the origin less the object's offset */
    float moved[3] = {o[0], o[1], o[2]};
    if (offsets)
      for (int k = 0; k < 3; k++) moved[k] = o[k] + (-offsets[3 * w->dyn[d].obj + k]);
    ry_range(w, &first, w->dyn[d].start, w->dyn[d].end, moved, u, speed);
  }
  return first;
}

/* players [first, first + count) of n; dirs: n_rays x xyz; offsets: n x n_objects x xyz or NULL.  frac / hit: the contract's
 * outputs; raw_time / raw_hit: the fold's result before the time <= 1 cut; origin / vel: xyz per ray.  Each may be NULL. */
void ry_cast(const world_t *w, const pstate *st, uint32_t n, uint32_t first, uint32_t count, const float *dirs, uint32_t n_rays,
             float max_range, const float *offsets, uint32_t n_objects, float *frac, uint32_t *hit, float *raw_time, uint32_t *raw_hit,
             float *origin, float *vel) {
  for (uint32_t p = first; p < first + count && p < n; p++) {
    ry_quat q = ry_orientation(st[p].yaw, st[p].pitch);
    float eye[3];
    ry_eye_of(&st[p], q, eye);
    for (uint32_t r = 0; r < n_rays; r++) {
      size_t at = (size_t)p * n_rays + r;
      float dir[3], v[3];
      ry_turn(q, dirs + 3 * (size_t)r, dir);
      for (int k = 0; k < 3; k++) v[k] = dir[k] * max_range;
      ry_hit h = ry_through(w, eye, v, offsets ? offsets + (size_t)p * n_objects * 3 : NULL);
      int within = h.time <= 1.0f;
      if (frac) frac[at] = within ? h.time : INFINITY;
      if (hit) hit[at] = within ? h.tri : 0xFFFFFFFFu;
      if (raw_time) raw_time[at] = h.time;
      if (raw_hit) raw_hit[at] = h.tri;
      if (origin) memcpy(origin + 3 * at, eye, sizeof eye);
      if (vel) memcpy(vel + 3 * at, v, sizeof v);
    }
  }
}
