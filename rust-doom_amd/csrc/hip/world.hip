// The collision world on the device: World::sweep_sphere (game/src/world.rs:40-120, math/src/sphere.rs:16-183) for a batch
// of queries, and K ticks of Player::update (game/src/player.rs:142-408) for a batch of players in one launch, with the C ABI
// of both (include/rdoom.h "collision world + player physics").  The host half, WorldBuilder, is csrc/host/game_world.cpp.
// Also the range-sensor rays cast from player states (include/rdoom.h "ray casts"): cast_rays_kernel and its world-set form.
//
// Arithmetic: binary32 in the reference's operation order (cgmath: dot = (x x' + y y') + z z', cross component by component,
// vector / scalar divides every component, normalize_or_zero = v / max(|v|, f32::EPSILON)); the build passes
// -ffp-contract=off and HIP divides and takes square roots correctly rounded, so every result is the one an IEEE host
// computes with the same expressions.  No fastmath.hpp short forms, no device libm: sin / cos come from sincos_rd (sincos_rd.hpp),
// a player's orientation quaternion and camera eye from player_quat.hpp.  The level pick, the checked launch and the device check
// are world_shared.hpp's, shared with the map kernels (automap.hip), whose device line table the handles here own.
//
// Shape: one lane per query / player -- the sweeps of one player are strictly sequential -- and one wave per workgroup.  Each
// lane walks the BSP with its own node stack in LDS (word `slot * 64 + lane`: no bank conflicts), sized by the tree's depth at
// create time, so nothing is spilled to scratch.  The world's arrays are read-only and shared by every lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "../common.hpp"
#include "../host/game_world.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "world_shared.hpp"

namespace {

constexpr uint32_t WAVE = 64;

struct DevNode {  // Node (world.rs:139-143): the partition's origin + displace, then the packed children
  float ox, oy, dx, dy;
  int32_t positive, negative, _pad[2];
};
struct DevDynamic {
  uint32_t object_id, tri_start, tri_end, _pad;
};

struct WorldView {
  const DevNode *nodes;
  const uint2 *chunks;
  const uint4 *tris;  // v1, v2, v3, normal
  const float *verts;
  const DevDynamic *dynamics;
  uint32_t n_dynamics;
  uint32_t stack_cap;  // node_depth + 1: a depth-first walk that pushes at most two children holds at most one pending sibling
                       // per level above the deepest, two at the deepest
};

// V3, Quat, cross and rotate are player_quat.hpp's (shared with the player cameras of frames.hip); the operators are the world's
using rdoom_dev::cross;
using rdoom_dev::player_eye;
using rdoom_dev::player_orientation;
using rdoom_dev::Quat;
using rdoom_dev::rotate;
using rdoom_dev::sincos_rd;
using rdoom_dev::V3;
using rdoom_dev::with_level;  // world_shared.hpp: the level pick, shared with the map kernels
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float magnitude(V3 a) { return __builtin_sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalize_or_zero(V3 a) {  // math/src/lib.rs:40-42 (f32::max: the other operand when one is NaN)
  const float m = magnitude(a);
  return a / (m > 1.1920929e-7f ? m : 1.1920929e-7f);
}
__device__ __forceinline__ V3 load3(const float *p) { return v3(p[0], p[1], p[2]); }

struct Contact {
  float time;
  V3 normal;
};

// sphere.rs:178-183
__device__ __forceinline__ bool inside_triangle(V3 a, V3 b, V3 c, V3 p) {
  const V3 u = b - a, v = c - a, n = cross(u, v), w = p - a;
  const float n2 = dot(n, n);
  const float gamma = dot(cross(u, w), n) / n2;
  const float beta = dot(cross(w, v), n) / n2;
  const float alpha = 1.0f - gamma - beta;
  return (0.0f <= alpha && alpha <= 1.0f) & (0.0f <= gamma && gamma <= 1.0f) & (0.0f <= beta && beta <= 1.0f);
}

// intersect_sphere_line + lowest_quadratic_root (sphere.rs:131-160); false = None
__device__ __forceinline__ bool sphere_line(V3 center, float radius, V3 p1, V3 p2, float &out) {
  const V3 edge = p2 - p1;
  const float a = dot(edge, edge);
  const float b = 2.0f * dot(edge, p1 - center);
  const float c = dot(center, center) + dot(p1, p1) - 2.0f * dot(center, p1) - radius * radius;
  float i = b * b - 4.0f * a * c;
  if (i < 0.0f) return false;
  i = __builtin_sqrtf(i);
  const float a2 = 2.0f * a;
  const float i1 = (-b + i) / a2, i2 = (-b - i) / a2;
  out = i1 < i2 ? i1 : i2;
  return true;
}

// intersect_line_line (sphere.rs:162-176) on 2-d points; false = None
__device__ __forceinline__ bool line_line(float p1x, float p1y, float p2x, float p2y, float p3x, float p3y, float p4x, float p4y,
                                          float &out) {
  const float d1x = p2x - p1x, d1y = p2y - p1y, d2x = p3x - p4x, d2y = p3y - p4y;
  const float denom = d2y * d1x - d2x * d1y;
  if (denom == 0.0f) return false;
  const float dist = d2x * (p1y - p3y) - d2y * (p1x - p3x);
  out = dist / denom;
  return true;
}

__device__ __forceinline__ float comp(V3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

__device__ __forceinline__ void sweep_vertex(V3 vertex, V3 center, float radius, V3 nvel, float &min_distance, V3 &contact_normal,
                                             bool &collision) {
  float d;
  if (sphere_line(center, radius, vertex, vertex + (-nvel), d) && d >= 0.0f && d < min_distance) {
    min_distance = d;
    contact_normal = center - (vertex + nvel * (-d));
    collision = true;
  }
}

__device__ __forceinline__ void sweep_edge(V3 e1, V3 e2, V3 center, float radius, V3 nvel, float &min_distance, V3 &contact_normal,
                                           bool &collision) {
  const V3 edge = e2 - e1;
  const V3 edge_normal = normalize_or_zero(cross(nvel, edge));
  const float edge_intercept = -dot(e1, edge_normal);
  const float edge_distance = dot(center, edge_normal) + edge_intercept;
  if (__builtin_fabsf(edge_distance) > radius) return;
  const float circle_radius = __builtin_sqrtf(radius * radius - edge_distance * edge_distance);
  const V3 circle_center = center + edge_normal * (-edge_distance);
  const V3 e1_to_circle_center = circle_center - e1;
  const V3 disp = edge * (dot(e1_to_circle_center, edge) / dot(edge, edge));
  const V3 on_line = e1 + disp;
  const V3 circle_center_to_on_line = normalize_or_zero(on_line - circle_center);
  const V3 candidate = circle_center + circle_center_to_on_line * circle_radius;
  const float ax = __builtin_fabsf(edge_normal.x), ay = __builtin_fabsf(edge_normal.y), az = __builtin_fabsf(edge_normal.z);
  int dim1, dim2;
  if (ax > ay && ax > az) dim1 = 1, dim2 = 2;
  else if (ay > az) dim1 = 0, dim2 = 2;
  else dim1 = 0, dim2 = 1;
  const V3 candidate_plus_nvel = candidate + nvel;
  float t;
  if (!line_line(comp(candidate, dim1), comp(candidate, dim2), comp(candidate_plus_nvel, dim1), comp(candidate_plus_nvel, dim2),
                 comp(e1, dim1), comp(e1, dim2), comp(e2, dim1), comp(e2, dim2), t))
    return;
  if (!(t >= 0.0f && t < min_distance)) return;
  const V3 intersection = candidate + nvel * t;
  if (dot(e1 - intersection, e2 - intersection) > 0.0f) return;
  min_distance = t;
  contact_normal = center - candidate;
  collision = true;
}

// Sphere::sweep_triangle (sphere.rs:16-127); false = None
__device__ __forceinline__ bool sweep_triangle(V3 t0, V3 t1, V3 t2, V3 normal, V3 center, float radius, V3 vel, Contact &out) {
  const float speed = magnitude(vel);
  if (speed == 0.0f) return false;
  const V3 nvel = vel / speed;
  const float normal_dot_nvel = dot(normal, nvel);
  if (normal_dot_nvel >= 0.0f) return false;
  V3 contact_normal = v3(0.0f, 0.0f, 0.0f);
  bool collision = false;
  float min_distance = 1e4f;
  const float intercept = -dot(t0, normal);
  const float signed_plane_distance = dot(center, normal) + intercept;
  if (signed_plane_distance < -radius) return false;
  if (signed_plane_distance >= radius) {  // sphere against plane
    const float distance = -(signed_plane_distance - radius) / normal_dot_nvel;
    const V3 on_plane = center + nvel * distance;
    if (inside_triangle(t0, t1, t2, on_plane)) {
      min_distance = distance;
      contact_normal = normal;
      collision = true;
    }
  }
  // (the vertices and edges one call each: an array of the three corners would be indexed in private memory)
  sweep_vertex(t0, center, radius, nvel, min_distance, contact_normal, collision);  // sphere against vertices
  sweep_vertex(t1, center, radius, nvel, min_distance, contact_normal, collision);
  sweep_vertex(t2, center, radius, nvel, min_distance, contact_normal, collision);
  sweep_edge(t0, t1, center, radius, nvel, min_distance, contact_normal, collision);  // sphere against edges
  sweep_edge(t1, t2, center, radius, nvel, min_distance, contact_normal, collision);
  sweep_edge(t2, t0, center, radius, nvel, min_distance, contact_normal, collision);
  if (!collision) return false;
  out.normal = normalize_or_zero(contact_normal);
  out.time = min_distance / speed;
  return true;
}

// World::sweep_chunk (world.rs:84-106): the fold keeps the later candidate on equal times
__device__ __forceinline__ void sweep_chunk(const WorldView &w, Contact &first, uint32_t start, uint32_t end, V3 center, float radius,
                                            V3 vel) {
  for (uint32_t i = start; i < end; i++) {
    const uint4 t = w.tris[i];
    Contact c;
    if (sweep_triangle(load3(w.verts + 3 * t.x), load3(w.verts + 3 * t.y), load3(w.verts + 3 * t.z), load3(w.verts + 3 * t.w), center,
                       radius, vel, c)) {  // (field by field: a select of two structs becomes one of their addresses in scratch)
      const bool keep = first.time < c.time;
      first.time = keep ? first.time : c.time;
      first.normal = v3(keep ? first.normal.x : c.normal.x, keep ? first.normal.y : c.normal.y, keep ? first.normal.z : c.normal.z);
    }
  }
}

// World::sweep_sphere (world.rs:40-82).  `stack`: this lane's first LDS word (stride WAVE).  `offsets`: this query's
// n_objects x xyz object displacements, or null.  time = +inf: None.
// `root`: the root node (a world set's level starts at its node base).
__device__ __forceinline__ Contact sweep_world(const WorldView &w, V3 center, float radius, V3 vel, const float *offsets,
                                               uint32_t *stack, uint32_t root = 0u) {
  Contact first{__builtin_inff(), v3(0.0f, 0.0f, 0.0f)};
  uint32_t sp = 0;
  stack[0] = root;
  sp = 1;
  while (sp) {  // statics: positive child first; leaves are swept when met, nodes pushed
    const DevNode node = w.nodes[stack[--sp * WAVE]];
    // Line2::signed_distance (math/src/line.rs:43-45) of the centre and of centre + vel, in the xz plane
    const float tx = center.x + vel.x, tz = center.z + vel.z;
    const float dist1 = (center.x * node.dy - center.z * node.dx) + (node.dx * node.oy - node.dy * node.ox);
    const float dist2 = (tx * node.dy - tz * node.dx) + (node.dx * node.oy - node.dy * node.ox);
    const bool pos = dist1 >= -radius || dist2 >= -radius;
    const bool neg = dist1 <= radius || dist2 <= radius;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (!(k == 0 ? pos : neg)) continue;
      const int32_t packed = k == 0 ? node.positive : node.negative;
      if (packed > 0) {             // Child::Node
        if (sp < w.stack_cap)       // (always: see WorldView::stack_cap; the test only keeps the LDS writes in bounds)
          stack[sp++ * WAVE] = (uint32_t)packed;
      } else {                      // Child::Leaf(-packed); a never-linked child is 0 = Leaf(0), as in the reference
        const uint2 chunk = w.chunks[(uint32_t)(-packed)];
        sweep_chunk(w, first, chunk.x, chunk.y, center, radius, vel);
      }
    }
  }
  for (uint32_t d = 0; d < w.n_dynamics; d++) {  // dynamics: the inverse of a pure translation is p + (-disp), v unchanged
    const DevDynamic dyn = w.dynamics[d];
    V3 off = v3(0.0f, 0.0f, 0.0f);
    if (offsets) off = load3(offsets + 3 * dyn.object_id);
    sweep_chunk(w, first, dyn.tri_start, dyn.tri_end, center + (-off), radius, vel);
  }
  return first;
}

__global__ __launch_bounds__(WAVE) void sweep_kernel(WorldView w, const float *spheres, const float *vels, uint32_t n,
                                                     const float *offsets, uint32_t n_objects, float *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q >= n) return;
  const float *sp = spheres + 4 * (size_t)q;
  const Contact c = sweep_world(w, v3(sp[0], sp[1], sp[2]), sp[3], load3(vels + 3 * (size_t)q),
                                offsets ? offsets + (size_t)q * n_objects * 3 : nullptr, lds_stack + threadIdx.x);
  float *o = out + 4 * (size_t)q;
  o[0] = c.time, o[1] = c.normal.x, o[2] = c.normal.y, o[3] = c.normal.z;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }  // player.rs:415-423

// step_players' level policy for player_step_kernel: every player, one world from node 0, nothing besides the physics.  Its
// level hooks are GameLevel's too.
struct NoGame {
  __device__ __forceinline__ bool begin(uint32_t) { return true; }
  __device__ __forceinline__ bool start_tick() { return false; }
  __device__ __forceinline__ V3 start_pos() const { return v3(0.0f, 0.0f, 0.0f); }
  __device__ __forceinline__ float start_yaw() const { return 0.0f; }
  __device__ __forceinline__ const WorldView &world(const WorldView &w) const { return w; }
  __device__ __forceinline__ uint32_t root() const { return 0u; }
  __device__ __forceinline__ void tick(uint32_t, V3, V3, float, float, uint32_t &) {}
};

// K ticks of Player::update (player.rs:359-396: force() with the feet probe and move_force, clip() or noclip(), then velocity
// += force * dt) for player p: the body of player_step_kernel, game_step_kernel and worldset_game_step_kernel, which differ only
// in their `Level` policy (NoGame, GameLevel, SetGame).  `level.begin(p)` false: player p is left untouched.  When
// `level.start_tick()` is true, the player starts the tick afresh at `level.start_pos()` (SetGame: a level change); the tick's
// sweeps see `level.world(w)` from node `level.root()`.  After each tick `level.tick(t, pos, vel, yaw, pitch, flags)` runs what the
// level does in the same tick (GameLevel: effects and triggers).
template <class Level>
__device__ __forceinline__ void step_players(const WorldView &w, rdoom_player_state *states, const rdoom_player_input *inputs, uint32_t n,
                                             uint32_t n_ticks, const rdoom_player_config &cfg, float dt, const float *offsets,
                                             uint32_t n_objects, Level &level) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= n) return;
  if (!level.begin(p)) return;
  uint32_t *stack = lds_stack + threadIdx.x;
  const float *off = offsets ? offsets + (size_t)p * n_objects * 3 : nullptr;
  rdoom_player_state *st = states + p;
  V3 pos = load3(st->pos), vel = load3(st->vel);
  float yaw = st->yaw, pitch = st->pitch, last_height_diff = st->last_height_diff;
  uint32_t flags = st->flags;
  const bool fly = flags & RDOOM_PLAYER_FLY, clip = flags & RDOOM_PLAYER_CLIP;
  const float pitch_limit = 1.57079637f - 1e-2f;  // FRAC_PI_2 - 1e-2 in binary32 (player.rs:196-201)
  for (uint32_t t = 0; t < n_ticks; t++) {
    if (level.start_tick()) {  // Player::reset (player.rs:118-133) at the new level's start
      pos = level.start_pos(), vel = v3(0.0f, 0.0f, 0.0f);
      yaw = level.start_yaw(), pitch = 1e-8f, last_height_diff = 0.0f;
    }
    const rdoom_player_input in = inputs[(size_t)t * n + p];
    const WorldView &wt = level.world(w);
    const uint32_t root = level.root();
    // ---- force() (player.rs:243-315): the feet probe
    float height = cfg.height;
    bool grounded = false;
    V3 ground_normal = v3(0.0f, 0.0f, 0.0f);
    {
      const Contact c = sweep_world(wt, pos, 0.2f, v3(0.0f, -cfg.height, 0.0f), off, stack, root);
      if (c.time < __builtin_inff() && c.time < 1.0f) height = cfg.height * c.time, ground_normal = c.normal, grounded = true;
    }
    // move_force (player.rs:182-241), orientation as (yaw, pitch)
    yaw = yaw - in.look[0];
    pitch = clampf(pitch - in.look[1], -pitch_limit, pitch_limit);
    float sy, cy, sp, cp;
    sincos_rd(yaw, sy, cy);
    sincos_rd(pitch, sp, cp);
    V3 force;
    if (fly) {  // rot * (normalize_or_zero(move.x, up, move.y) * move_force), rot = Ry(yaw) Rx(pitch)
      const V3 m = normalize_or_zero(v3(in.movement[0], in.jump ? 0.5f : 0.0f, in.movement[1])) * cfg.move_force;
      const float y1 = m.y * cp - m.z * sp, z1 = m.y * sp + m.z * cp;
      force = v3(m.x * cy + z1 * sy, y1, z1 * cy - m.x * sy);
    } else {  // normalize(Ry(yaw) (move.x, 0, move.y cos pitch)): the y the pitch adds is dropped before normalising
      const float a = in.movement[1] * cp;
      V3 m = normalize_or_zero(v3(in.movement[0] * cy + a * sy, 0.0f, a * cy - in.movement[0] * sy)) * cfg.move_force;
      if (grounded) {
        if (in.jump && vel.y < 0.1f) m = v3(m.x, 5.0f / dt, m.z);
      } else {
        m = m * 0.1f;
      }
      force = m;
    }
    const float speed = magnitude(vel);
    if (speed > 0.0f) {
      V3 slowdown = v3(0.0f, 0.0f, 0.0f);
      if (fly) {
        slowdown = (-vel) * (cfg.friction / speed + cfg.ground_drag * speed);
      } else if (grounded) {
        const V3 tangential = vel - ground_normal * dot(vel, ground_normal);
        const float ts = magnitude(tangential);
        if (ts > 0.0f) slowdown = (-tangential) * (cfg.friction / ts + cfg.ground_drag * ts);
      }
      slowdown = slowdown - vel * cfg.air_drag * speed;
      const float slowdown_norm = magnitude(slowdown);
      if (slowdown_norm > 0.0f) {
        const float max_slowdown = -dot(vel, slowdown) / slowdown_norm / dt;
        if (slowdown_norm >= max_slowdown) slowdown = slowdown / slowdown_norm * max_slowdown;
        force = force + slowdown;
      }
    }
    const float height_diff = cfg.height - height;
    const float derivative = (height_diff - last_height_diff) / dt;
    last_height_diff = height_diff;
    force.y = force.y + (height_diff * cfg.spring_const_p + derivative * cfg.spring_const_d);
    if (!fly) force.y = force.y - 17.0f;
    // ---- clip() (player.rs:142-166) or noclip() (player.rs:168-190)
    if (clip) {
      float time_left = dt;
      bool armed = true;
      for (int i = 0; i < 100; i++) {
        const V3 displacement = vel * time_left;
        const Contact c = sweep_world(wt, pos, cfg.radius, displacement, off, stack, root);
        if (c.time < __builtin_inff()) {
          const float adjusted_time = c.time - 0.001f / magnitude(displacement);
          if (adjusted_time < 1.0f) {
            const float time = clampf(c.time, 0.0f, 1.0f);
            pos = pos + displacement * adjusted_time;
            vel = vel - c.normal * dot(c.normal, vel);
            time_left = time_left * (1.0f - time);
            continue;
          }
        }
        pos = pos + displacement;
        armed = false;
        break;
      }
      if (armed) flags |= RDOOM_PLAYER_DIVERGED;
    } else {
      const float old_height = pos.y;
      pos = pos + vel * dt;
      if (!fly) {
        const float probe_height = 2000.0f;
        const V3 probe = pos + v3(0.0f, probe_height / 2.0f, 0.0f);
        const Contact c = sweep_world(wt, probe, cfg.radius, v3(0.0f, -probe_height, 0.0f), off, stack, root);
        const float h = c.time < __builtin_inff() ? pos.y + probe_height * (0.5f - c.time) : old_height;
        if (pos.y <= h) {
          pos.y = h;
          if (vel.y < 0.0f) vel.y = 0.0f;
        }
      }
    }
    vel = vel + force * dt;
    level.tick(t, pos, vel, yaw, pitch, flags);
  }
  st->pos[0] = pos.x, st->pos[1] = pos.y, st->pos[2] = pos.z;
  st->vel[0] = vel.x, st->vel[1] = vel.y, st->vel[2] = vel.z;
  st->yaw = yaw, st->pitch = pitch, st->last_height_diff = last_height_diff;
  st->flags = flags;
}

__global__ __launch_bounds__(WAVE) void player_step_kernel(WorldView w, rdoom_player_state *states, const rdoom_player_input *inputs,
                                                           uint32_t n, uint32_t n_ticks, rdoom_player_config cfg, float dt,
                                                           const float *offsets, uint32_t n_objects) {
  NoGame level;
  step_players(w, states, inputs, n, n_ticks, cfg, dt, offsets, n_objects, level);
}

// ---- doors, lifts and exits: Level::poll_triggers (game/src/level.rs:77-167) and the move effects of Level::update (:184-267)
struct DevTrigger {  // rdoom_trigger's line, type, flags and effect range
  float ox, oy, dx, dy, len;
  uint32_t trigger_type, flags, effect_start, effect_end, _pad[3];
};
struct DevEffect {
  uint32_t object_id, has_second;
  float first, second, wait, speed, _pad[2];
};
struct GameView {  // the shared trigger list, and the word offsets of one game's fields (include/rdoom.h rdoom_world_game_bytes)
  const DevTrigger *triggers;
  const DevEffect *effects;
  uint32_t n_triggers, n_objects;
  uint32_t live, fired, active, second, order, effect, words;  // word offsets within a game; words per game
};

struct Line2 {  // Line2f (math/src/line.rs)
  float ox, oy, dx, dy, len;
};
// Line2::from_origin_and_displace (line.rs:12-27)
__device__ __forceinline__ Line2 line_from(float ox, float oy, float vx, float vy) {
  const float len = __builtin_sqrtf(vx * vx + vy * vy);
  if (__builtin_fabsf(len) >= 1e-16f) return Line2{ox, oy, vx / len, vy / len, len};
  return Line2{ox, oy, 0.0f, 0.0f, 0.0f};
}
// a.segment_intersect_offset(b).is_some() (line.rs:47-84); a comparison with a NaN offset fails, as in the reference
__device__ __forceinline__ bool segment_hits(const Line2 &a, float box, float boy, float bdx, float bdy, float blen) {
  const float den = a.dx * bdy - a.dy * bdx;
  if (__builtin_fabsf(den) < 1e-16f) return false;
  const float off = ((box - a.ox) * bdy - (boy - a.oy) * bdx) / den;
  if (off < 0.0f || off >= a.len) return false;
  const float px = a.ox + a.dx * off, py = a.oy + a.dy * off;
  const float other = __builtin_fabsf(bdx) > __builtin_fabsf(bdy) ? (px - box) / bdx : (py - boy) / bdy;
  return !(other < 0.0f || other >= blen);
}

// One game's level: the per-player part of Level (effects, trigger list) in d_game, the offsets in the caller's array.  Trigger
// lines and effect definitions are the same for every lane and read in linedef order (scalar loads); the list order is
// resolved only on the rare tick when a lane fires two triggers or removes one.  One level for every tick: NoGame's hooks.
struct GameLevel : NoGame {
  GameView g;
  uint32_t *games;
  float *offsets;
  const uint8_t *actions;
  uint32_t n, n_objects;
  float dt;
  uint32_t *game;  // this lane's
  float *off;
  __device__ __forceinline__ bool begin(uint32_t p) {
    game = games + (size_t)p * g.words;
    off = offsets + (size_t)p * n_objects * 3;
    lane = p;
    return true;
  }
  uint32_t lane;

  // the loop of level.rs:203-255 for every active effect, ascending object id
  __device__ __forceinline__ void advance() {
    float4 *eff = reinterpret_cast<float4 *>(game + g.effect);
    for (uint32_t wi = 0; wi * 32 < g.n_objects; wi++) {
      uint32_t bits = game[g.active + wi];
      if (!bits) continue;
      uint32_t active = bits, second = game[g.second + wi];
      while (bits) {
        const uint32_t b = __builtin_ctz(bits);
        bits &= bits - 1;
        const uint32_t o = wi * 32 + b;
        float4 e = eff[o];  // first, second, wait, speed
        float *y = off + 3 * (size_t)o + 1;
        float cur = *y, ts = dt;
        bool has_second = (second >> b) & 1u, done = false;
        for (;;) {
          if (e.x != cur) {
            const float diff = e.x - cur;
            const float sign = __builtin_copysignf(1.0f, diff);
            const float time_left = __builtin_fabsf(diff) / e.w;
            if (time_left > ts) {
              cur = cur + sign * e.w * ts;
              break;
            }
            cur = e.x;
            ts = ts - time_left;
            e.x = cur;
          }
          if (e.z > ts) {
            e.z = e.z - ts;
            break;
          }
          ts = ts - e.z;
          e.z = 0.0f;
          if (has_second) {
            e.x = e.y;
            has_second = false;
            continue;
          }
          done = true;
          break;
        }
        *y = cur;
        eff[o] = e;
        if (done) active &= ~(1u << b);
        if (!has_second) second &= ~(1u << b);
      }
      game[g.active + wi] = active;
      game[g.second + wi] = second;
    }
  }

  __device__ __forceinline__ void start_effects(uint32_t i) {  // self.effects.insert for each of trigger i's effects
    const DevTrigger tr = g.triggers[i];
    float4 *eff = reinterpret_cast<float4 *>(game + g.effect);
    for (uint32_t k = tr.effect_start; k < tr.effect_end; k++) {
      const DevEffect e = g.effects[k];
      eff[e.object_id] = make_float4(e.first, e.second, e.wait, e.speed);
      const uint32_t wi = e.object_id >> 5, bit = 1u << (e.object_id & 31);
      game[g.active + wi] |= bit;
      game[g.second + wi] = e.has_second ? game[g.second + wi] | bit : game[g.second + wi] & ~bit;
    }
  }

  __device__ __forceinline__ void tick(uint32_t t, V3 pos, V3 vel, float yaw, float pitch, uint32_t &flags) {
    advance();
    // poll_triggers (level.rs:77-167) from the new position; moved = velocity * dt after this tick's update
    const V3 moved = vel * dt;
    const Line2 walked = line_from(pos.x, pos.z, -moved.x, -moved.z);
    uint32_t action = actions ? actions[(size_t)t * n + lane] : 0u;
    action = action <= RDOOM_ACTION_SHOOT ? action : RDOOM_ACTION_NONE;
    Line2 act{pos.x, pos.z, 0.0f, 0.0f, 0.0f};
    if (action) {  // look = rot.rotate_vector(-z), rot = Quaternion::from(Euler { pitch, yaw, 0 })
      const V3 look = rotate(player_orientation(yaw, pitch), v3(-0.0f, -0.0f, -1.0f));
      const float m = __builtin_sqrtf(look.x * look.x + look.z * look.z);
      const float d = m > 1.1920929e-7f ? m : 1.1920929e-7f;
      const float range = action == RDOOM_ACTION_PUSH ? 0.5f : 100.0f;
      act = line_from(pos.x, pos.z, look.x / d * range, look.z / d * range);
    }
    const bool push = action == RDOOM_ACTION_PUSH, shoot = action == RDOOM_ACTION_SHOOT;
    uint32_t n_fired = 0, first = 0;
    bool reorder = false;
    for (uint32_t i = 0; i < g.n_triggers; i++) {  // wave-uniform: every lane reads trigger i
      const DevTrigger tr = g.triggers[i];
      bool hit = false;
      if (tr.trigger_type == RDOOM_TRIGGER_WALK_OVER || tr.trigger_type == RDOOM_TRIGGER_ANY) hit = segment_hits(walked, tr.ox, tr.oy, tr.dx, tr.dy, tr.len);
      if (!hit && ((push && (tr.trigger_type == RDOOM_TRIGGER_PUSH || tr.trigger_type == RDOOM_TRIGGER_SWITCH || tr.trigger_type == RDOOM_TRIGGER_ANY)) ||
                   (shoot && tr.trigger_type == RDOOM_TRIGGER_GUN)))
        hit = segment_hits(act, tr.ox, tr.oy, tr.dx, tr.dy, tr.len);
      if (!hit || !((game[g.live + (i >> 5)] >> (i & 31)) & 1u)) continue;
      if (tr.flags & RDOOM_TRIGGER_EXIT) flags |= RDOOM_PLAYER_EXITED;
      game[g.fired + (i >> 5)] |= 1u << (i & 31);
      reorder |= n_fired > 0 || (tr.flags & RDOOM_TRIGGER_ONLY_ONCE);
      first = n_fired ? first : i;
      n_fired++;
    }
    if (!n_fired) return;
    if (!reorder) {  // one trigger, not removed: its order does not matter
      start_effects(first);
      game[g.fired + (first >> 5)] = 0u;
      return;
    }
    // the player's own order: effects in list order (a later trigger wins an object), then swap_remove descending
    uint32_t count = game[0];
    uint32_t *order = game + g.order;
    for (uint32_t k = 0; k < count; k++) {
      const uint32_t i = order[k];
      if ((game[g.fired + (i >> 5)] >> (i & 31)) & 1u) start_effects(i);
    }
    for (uint32_t k = count; k-- > 0;) {
      const uint32_t i = order[k];
      if (!((game[g.fired + (i >> 5)] >> (i & 31)) & 1u)) continue;
      game[g.fired + (i >> 5)] &= ~(1u << (i & 31));
      if (g.triggers[i].flags & RDOOM_TRIGGER_ONLY_ONCE) {
        order[k] = order[count - 1];
        count--;
        game[g.live + (i >> 5)] &= ~(1u << (i & 31));
      }
    }
    game[0] = count;
  }
};

// triggers / effects: level.g's, passed again as __restrict__ arguments -- nothing the kernel writes aliases them, so the
// wave-uniform trigger loads of the poll can be scalar loads
__global__ __launch_bounds__(WAVE) void game_step_kernel(WorldView w, GameLevel level, const DevTrigger *__restrict__ triggers,
                                                         const DevEffect *__restrict__ effects, rdoom_player_state *states,
                                                         const rdoom_player_input *inputs, uint32_t n_ticks, rdoom_player_config cfg) {
  level.g.triggers = triggers;
  level.g.effects = effects;
  step_players(w, states, inputs, level.n, n_ticks, cfg, level.dt, level.offsets, level.n_objects, level);
}

// word k of a fresh game of a level with layout l (a GameView or a DevSetLevel): all triggers live, in linedef order, no effect;
// the words past the level's own are zero
template <class Layout>
__device__ __forceinline__ uint32_t fresh_word(const Layout &l, uint32_t k) {
  if (k == 0) return l.n_triggers;
  if (k >= l.live && k < l.fired) {
    const uint32_t first = (k - l.live) * 32;
    return l.n_triggers - first >= 32 ? ~0u : (1u << (l.n_triggers - first)) - 1u;
  }
  if (k >= l.order && k < l.order + l.n_triggers) return k - l.order;
  return 0u;
}

// a fresh level for player blockIdx.x (if masked in): one workgroup per game, its lanes striding over the words
__global__ __launch_bounds__(WAVE) void game_reset_kernel(GameView g, uint32_t *games, float *offsets, uint32_t n_objects,
                                                          const uint8_t *mask) {
  const uint32_t p = blockIdx.x;
  if (mask && !mask[p]) return;
  uint32_t *game = games + (size_t)p * g.words;
  for (uint32_t k = threadIdx.x; k < g.words; k += WAVE) game[k] = fresh_word(g, k);
  float *off = offsets + (size_t)p * n_objects * 3;
  for (uint32_t k = threadIdx.x; k < n_objects * 3; k += WAVE) off[k] = 0.0f;
}

// ---- a world set: several levels, each player in one of them, and the exit that takes a player to the next
struct DevSetLevel {  // one slot of a world set: where its arrays start in the concatenation, its game layout, its start
  uint32_t root, dyn_start, n_dynamics, destination;  // destination: a slot, or rdoom::game::NO_DESTINATION
  uint32_t trig_start, n_triggers, n_objects, words;  // n_objects: the level's game objects; words: its own game's
  uint32_t live, fired, active, second, order, effect, _pad[2];
  float start[3], start_yaw;
};

__device__ __forceinline__ GameView level_view(const GameView &set, const DevSetLevel &l) {  // the level's layout within a game
  return GameView{set.triggers + l.trig_start, set.effects, l.n_triggers, l.n_objects, l.live, l.fired, l.active, l.second, l.order,
                  l.effect, l.words};
}

// Word 1 of a set's game: where the player is in the level change.  An exit fired in the poll of tick t (STAGE_EXITED); tick t + 1
// requests the next level and still runs in the old one (STAGE_REQUESTED); tick t + 2 loads it, resets the player and runs in it.
constexpr uint32_t STAGE_NONE = 0u, STAGE_EXITED = 1u, STAGE_REQUESTED = 2u;

// the set's world seen from one level: its own dynamic chunks (its nodes start at the level's root)
__device__ __forceinline__ WorldView level_world(const WorldView &w, uint32_t dyn_start, uint32_t n_dynamics) {
  return WorldView{w.nodes, w.chunks, w.tris, w.verts, w.dynamics + dyn_start, n_dynamics, w.stack_cap};
}

// A player's game in a world set: GameLevel's effects and triggers on the player's current level, and the level change.
struct SetGame {
  GameLevel gl;                // games, offsets, actions, n, dt; gl.n_objects and gl.g.words are the set's, gl.g.triggers /
                               // effects the concatenated lists
  const DevSetLevel *levels;
  uint32_t *level_of;
  uint32_t n_levels;
  uint32_t lv, stage;          // this lane's level and change stage
  uint32_t root_, dyn_start, n_dyn;

  __device__ __forceinline__ bool begin(uint32_t p) {
    lv = level_of[p];
    if (lv >= n_levels) return false;  // not a slot: the player is left untouched
    gl.begin(p);
    stage = gl.game[1];
    return true;
  }
  __device__ __forceinline__ bool start_tick() {
    bool reset = false;
    if (stage == STAGE_EXITED) {  // Level::update: exit_triggered -> change_level(current + 1) (level.rs:194-199)
      stage = STAGE_REQUESTED;
      gl.game[1] = stage;
    } else if (stage == STAGE_REQUESTED) {  // WadSystem::update loads it, Level is rebuilt, Player::update resets (player.rs:359-362)
      const uint32_t d = levels[lv].destination;
      stage = STAGE_NONE;
      if (d < n_levels) {
        lv = d;
        level_of[gl.lane] = d;
        const DevSetLevel l = levels[d];
        for (uint32_t k = 0; k < gl.g.words; k++) gl.game[k] = fresh_word(l, k);
        for (uint32_t k = 0; k < gl.n_objects * 3; k++) gl.off[k] = 0.0f;
        reset = true;
      } else {
        gl.game[1] = stage;
      }
    }
    root_ = levels[lv].root, dyn_start = levels[lv].dyn_start, n_dyn = levels[lv].n_dynamics;
    return reset;
  }
  __device__ __forceinline__ V3 start_pos() const { return load3(levels[lv].start); }
  __device__ __forceinline__ float start_yaw() const { return levels[lv].start_yaw; }
  __device__ __forceinline__ WorldView world(const WorldView &w) const { return level_world(w, dyn_start, n_dyn); }
  __device__ __forceinline__ uint32_t root() const { return root_; }

  __device__ __forceinline__ void tick(uint32_t t, V3 pos, V3 vel, float yaw, float pitch, uint32_t &flags) {
    uint32_t fired = 0u;
    GameLevel l = gl;
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) {  // (one level in the wave: its trigger loads stay scalar)
      l.g = level_view(gl.g, levels[slot]);
      l.tick(t, pos, vel, yaw, pitch, fired);
    });
    flags |= fired;
    // an exit with a destination starts the change; one fired while a change is under way is lost with the rebuilt Level
    if ((fired & RDOOM_PLAYER_EXITED) && stage == STAGE_NONE && levels[lv].destination < n_levels) {
      stage = STAGE_EXITED;
      gl.game[1] = stage;
    }
  }
};

// triggers / effects / levels: passed as __restrict__ arguments, as for game_step_kernel
__global__ __launch_bounds__(WAVE) void worldset_game_step_kernel(WorldView w, SetGame set, const DevTrigger *__restrict__ triggers,
                                                                  const DevEffect *__restrict__ effects,
                                                                  const DevSetLevel *__restrict__ levels, rdoom_player_state *states,
                                                                  const rdoom_player_input *inputs, uint32_t n_ticks, rdoom_player_config cfg) {
  set.gl.g.triggers = triggers;
  set.gl.g.effects = effects;
  set.levels = levels;
  step_players(w, states, inputs, set.gl.n, n_ticks, cfg, set.gl.dt, set.gl.offsets, set.gl.n_objects, set);
}

// ---- range-sensor rays from player states (include/rdoom.h "ray casts") ----
// Ray (p, r) starts at player p's camera eye and runs along the player's rotation of the shared camera-frame direction r, for
// max_range.  Against a triangle it is the plane branch of Sphere::sweep_triangle (sphere.rs:16-53) at radius 0 and nothing
// else; through the world it is World::sweep_sphere at radius 0 (world.rs:40-82), and the result is that fold.  Nothing is
// pruned: a ray visits exactly the nodes, chunks and triangles the radius-0 sweep visits, in its order.
//
// Shape: one lane per ray, flat index q = p * n_rays + r, so a wave holds the rays of one player or of a few neighbours and its
// lanes walk nearly the same nodes and chunks.  The node stack is sweep_world's (LDS, word `slot * 64 + lane`).

struct RayHit {
  float time;
  uint32_t tri;
};

// World::sweep_chunk for a ray: `speed` and `nvel` are the triangle test's own (the same expression for every triangle)
__device__ __forceinline__ void cast_chunk(const WorldView &w, RayHit &first, uint32_t start, uint32_t end, V3 origin, V3 nvel, float speed) {
  for (uint32_t i = start; i < end; i++) {
    const uint4 t = w.tris[i];
    const V3 normal = load3(w.verts + 3 * t.w);
    const float normal_dot_nvel = dot(normal, nvel);
    if (normal_dot_nvel >= 0.0f) continue;
    const V3 t0 = load3(w.verts + 3 * t.x);
    const float intercept = -dot(t0, normal);
    const float signed_plane_distance = dot(origin, normal) + intercept;
    if (signed_plane_distance < 0.0f) continue;
    const float distance = -signed_plane_distance / normal_dot_nvel;
    const V3 on_plane = origin + nvel * distance;
    if (!inside_triangle(t0, load3(w.verts + 3 * t.y), load3(w.verts + 3 * t.z), on_plane)) continue;
    const float time = distance / speed;
    const bool keep = first.time < time;  // the later candidate on equal times
    first.time = keep ? first.time : time;
    first.tri = keep ? first.tri : i;
  }
}

__device__ __forceinline__ RayHit cast_world(const WorldView &w, V3 origin, V3 vel, const float *offsets, uint32_t *stack, uint32_t root) {
  RayHit first{__builtin_inff(), 0xFFFFFFFFu};
  const float speed = magnitude(vel);
  if (speed == 0.0f) return first;  // sweep_triangle returns None for every triangle
  const V3 nvel = vel / speed;
  const float tx = origin.x + vel.x, tz = origin.z + vel.z;
  uint32_t sp = 1;
  stack[0] = root;
  while (sp) {  // Node::intersect_sphere with radius 0: positive child first; leaves are cast when met, nodes pushed
    const DevNode node = w.nodes[stack[--sp * WAVE]];
    const float dist1 = (origin.x * node.dy - origin.z * node.dx) + (node.dx * node.oy - node.dy * node.ox);
    const float dist2 = (tx * node.dy - tz * node.dx) + (node.dx * node.oy - node.dy * node.ox);
    const bool pos = dist1 >= -0.0f || dist2 >= -0.0f;
    const bool neg = dist1 <= 0.0f || dist2 <= 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (!(k == 0 ? pos : neg)) continue;
      const int32_t packed = k == 0 ? node.positive : node.negative;
      if (packed > 0) {
        if (sp < w.stack_cap)  // (always: see WorldView::stack_cap; the test only keeps the LDS writes in bounds)
          stack[sp++ * WAVE] = (uint32_t)packed;
      } else {
        const uint2 chunk = w.chunks[(uint32_t)(-packed)];
        cast_chunk(w, first, chunk.x, chunk.y, origin, nvel, speed);
      }
    }
  }
  for (uint32_t d = 0; d < w.n_dynamics; d++) {
    const DevDynamic dyn = w.dynamics[d];
    V3 off = v3(0.0f, 0.0f, 0.0f);
    if (offsets) off = load3(offsets + 3 * dyn.object_id);
    cast_chunk(w, first, dyn.tri_start, dyn.tri_end, origin + (-off), nvel, speed);
  }
  return first;
}

struct RayArgs {
  const rdoom_player_state *states;
  const float *dirs;     // n_rays x xyz, camera frame
  const float *offsets;  // n x n_objects x xyz, or null
  float *frac;
  uint32_t *hit;         // may be null, as origin and vel
  float *origin, *vel;
  uint32_t n_rays, n_objects, total;  // total = n * n_rays
  float max_range;
};

// ray q of a.total through `w` from node `root`; hits are reported less `tri_start`
__device__ __forceinline__ void cast_ray(const WorldView &w, const RayArgs &a, uint32_t q, uint32_t p, uint32_t root, uint32_t tri_start,
                                         uint32_t *stack) {
  const rdoom_player_state *st = a.states + p;
  const Quat player = player_orientation(st->yaw, st->pitch);
  const V3 origin = player_eye(player, load3(st->pos));
  const V3 dir = rotate(player, load3(a.dirs + 3 * (size_t)(q - p * a.n_rays)));
  const V3 vel = dir * a.max_range;
  const RayHit h = cast_world(w, origin, vel, a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr, stack, root);
  const bool in_range = h.time <= 1.0f;
  a.frac[q] = in_range ? h.time : __builtin_inff();
  if (a.hit) a.hit[q] = in_range ? h.tri - tri_start : 0xFFFFFFFFu;
  if (a.origin) a.origin[3 * (size_t)q] = origin.x, a.origin[3 * (size_t)q + 1] = origin.y, a.origin[3 * (size_t)q + 2] = origin.z;
  if (a.vel) a.vel[3 * (size_t)q] = vel.x, a.vel[3 * (size_t)q + 1] = vel.y, a.vel[3 * (size_t)q + 2] = vel.z;
}

__global__ __launch_bounds__(WAVE) void cast_rays_kernel(WorldView w, RayArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q >= a.total) return;
  cast_ray(w, a, q, q / a.n_rays, 0u, 0u, lds_stack + threadIdx.x);
}

// the world set's: player p's rays run through level level_of[p]; a slot outside the set gives +inf / no hit, nothing else
// tri_starts: each level's first triangle in the concatenation (a hit is reported in the level's own indices)
__global__ __launch_bounds__(WAVE) void worldset_cast_rays_kernel(WorldView w, RayArgs a, const DevSetLevel *__restrict__ levels,
                                                                  const uint32_t *__restrict__ tri_starts,
                                                                  const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
  const uint32_t q = blockIdx.x * WAVE + threadIdx.x;
  if (q >= a.total) return;
  const uint32_t p = q / a.n_rays;
  const uint32_t lv = level_of[p];
  if (lv >= n_levels) {
    a.frac[q] = __builtin_inff();
    if (a.hit) a.hit[q] = 0xFFFFFFFFu;
    return;
  }
  uint32_t root, dyn_start, n_dyn, tri_start;
  with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) {  // (one level in the wave always, when n_rays is a multiple of 64)
    root = levels[slot].root, dyn_start = levels[slot].dyn_start, n_dyn = levels[slot].n_dynamics, tri_start = tri_starts[slot];
  });
  cast_ray(level_world(w, dyn_start, n_dyn), a, q, p, root, tri_start, lds_stack + threadIdx.x);
}

// (defined last: the code object's final kernel, as before the ray casts)
// a fresh game of its current level for player blockIdx.x (if masked in and on a slot): one workgroup per game
__global__ __launch_bounds__(WAVE) void worldset_game_reset_kernel(const DevSetLevel *__restrict__ levels, uint32_t n_levels,
                                                                   uint32_t words, uint32_t *games, float *offsets, uint32_t n_objects,
                                                                   const uint32_t *level_of, const uint8_t *mask) {
  const uint32_t p = blockIdx.x;
  if (mask && !mask[p]) return;
  const uint32_t lv = level_of[p];
  if (lv >= n_levels) return;
  const DevSetLevel l = levels[lv];
  uint32_t *game = games + (size_t)p * words;
  for (uint32_t k = threadIdx.x; k < words; k += WAVE) game[k] = fresh_word(l, k);
  float *off = offsets + (size_t)p * n_objects * 3;
  for (uint32_t k = threadIdx.x; k < n_objects * 3; k += WAVE) off[k] = 0.0f;
}

}  // namespace

static_assert(sizeof(rdoom_world_node) == sizeof(rdoom::game::WorldNode) && sizeof(rdoom_world_chunk) == sizeof(rdoom::game::WorldChunk) &&
                  sizeof(rdoom_world_triangle) == sizeof(rdoom::game::WorldTriangle) &&
                  sizeof(rdoom_world_dynamic) == sizeof(rdoom::game::WorldDynamic),
              "the C ABI records are the host builder's");
static_assert(sizeof(rdoom_player_state) == 40 && sizeof(rdoom_player_input) == 20 && sizeof(rdoom_player_config) == 32, "ABI sizes");

static_assert(sizeof(rdoom::game::WorldChunk) == sizeof(uint2) && sizeof(rdoom::game::WorldTriangle) == sizeof(uint4),
              "the kernels read the host builder's chunks and triangles as they are");

namespace {
using rdoom::DeviceArray;
using rdoom::EMPTY_TABLE_BYTES;  // (a level without dynamic chunks: a valid, unread pointer)

// the device arrays of a host World (rdoom_world_create; a world set's concatenation)
struct DevArrays {
  DeviceArray<DevNode> nodes;
  DeviceArray<uint2> chunks;
  DeviceArray<uint4> tris;
  DeviceArray<float> verts;
  DeviceArray<DevDynamic> dynamics;
  DeviceArray<DevTrigger> triggers;
  DeviceArray<DevEffect> effects;
};
rdoom_status upload_world(const rdoom::game::World &h, DevArrays &d) {
  std::vector<DevNode> nodes(h.nodes.size());
  for (size_t i = 0; i < nodes.size(); i++) {
    const rdoom::game::WorldNode &s = h.nodes[i];
    nodes[i] = DevNode{s.origin[0], s.origin[1], s.displace[0], s.displace[1], s.positive, s.negative, {0, 0}};
  }
  std::vector<DevDynamic> dyn(h.dynamics.size());
  for (size_t i = 0; i < dyn.size(); i++) dyn[i] = DevDynamic{h.dynamics[i].object_id, h.dynamics[i].tri_start, h.dynamics[i].tri_end, 0};
  if (rdoom_status s = d.nodes.upload(nodes, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = d.chunks.upload(reinterpret_cast<const uint2 *>(h.chunks.data()), h.chunks.size(), EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = d.tris.upload(reinterpret_cast<const uint4 *>(h.triangles.data()), h.triangles.size(), EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = d.verts.upload(h.verts, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = d.dynamics.upload(dyn, EMPTY_TABLE_BYTES)) return s;
  std::vector<DevTrigger> trig(h.triggers.size());
  for (size_t i = 0; i < trig.size(); i++) {
    const rdoom_trigger &t = h.triggers[i];
    trig[i] = DevTrigger{t.origin[0], t.origin[1], t.displace[0], t.displace[1], t.length, t.trigger_type, t.flags, t.effect_start, t.effect_end, {0, 0, 0}};
  }
  std::vector<DevEffect> eff(h.effects.size());
  for (size_t i = 0; i < eff.size(); i++) {
    const rdoom_move_effect &e = h.effects[i];
    eff[i] = DevEffect{e.object_id, e.has_second, e.first_height_offset, e.second_height_offset, e.wait, e.speed, {0.0f, 0.0f}};
  }
  if (rdoom_status s = d.triggers.upload(trig, EMPTY_TABLE_BYTES)) return s;
  return d.effects.upload(eff, EMPTY_TABLE_BYTES);
}
}  // namespace

struct rdoom_world {
  rdoom::game::World host;
  bool on_device = false;
  int device = -1;
  DevArrays d;
  rdoom::MapDevice map;  // the level's line table, as automap.hip lays it out
  rdoom::SectorDevice sectors;  // its sector table, as sectors.hip lays it out
  rdoom::SpawnDevice spawn;     // its spawn table, as spawn.hip lays it out
  float4 bounds = {};           // line_bounds of its line table (area.hip's grid)
};

struct rdoom_worldset {
  rdoom::game::WorldSet host;
  std::vector<DevSetLevel> table;  // the device table's records
  uint32_t words = 0;              // a game's words: the largest level's
  bool on_device = false;
  int device = -1;
  DevArrays d;
  DeviceArray<DevSetLevel> d_table;
  DeviceArray<uint32_t> d_tri_starts;  // each level's triangle base in the concatenation (the ray cast's)
  rdoom::MapDevice map;              // the levels' line tables, one after the other
  rdoom::SectorDevice sectors;       // and their sector tables
  rdoom::SpawnDevice spawn;          // and their spawn tables
  std::vector<float4> bounds;        // line_bounds of each level's line table (area.hip's grids)
};

namespace rdoom {
MapSource map_source(const rdoom_world *w) {
  return MapSource{&w->map, &w->sectors, &w->spawn, (uint32_t)w->host.map_sectors.size(), w->host.game_objects, (uint32_t)w->host.map_lines.size(),
                   &w->bounds, 1u, w->on_device, w->device};
}
MapSource map_source(const rdoom_worldset *s) {
  size_t most = 0, most_sectors = 0;
  for (const rdoom::game::World &l : s->host.levels) most = std::max(most, l.map_lines.size()), most_sectors = std::max(most_sectors, l.map_sectors.size());
  return MapSource{&s->map, &s->sectors, &s->spawn, (uint32_t)most_sectors, s->host.game_objects, (uint32_t)most, s->bounds.data(),
                   (uint32_t)s->bounds.size(), s->on_device, s->device};
}
}  // namespace rdoom

namespace {
void fill_arrays(const rdoom::game::World &h, rdoom_world_arrays &a) {
  std::memset(&a, 0, sizeof a);
  a.nodes = reinterpret_cast<const rdoom_world_node *>(h.nodes.data());
  a.n_nodes = (uint32_t)h.nodes.size();
  a.chunks = reinterpret_cast<const rdoom_world_chunk *>(h.chunks.data());
  a.n_chunks = (uint32_t)h.chunks.size();
  a.triangles = reinterpret_cast<const rdoom_world_triangle *>(h.triangles.data());
  a.n_triangles = (uint32_t)h.triangles.size();
  a.n_static_triangles = h.n_static_triangles;
  a.verts = h.verts.data();
  a.n_verts = (uint32_t)(h.verts.size() / 3);
  a.dynamics = reinterpret_cast<const rdoom_world_dynamic *>(h.dynamics.data());
  a.n_dynamics = (uint32_t)h.dynamics.size();
  a.n_objects = h.n_objects;
  a.node_depth = h.node_depth;
}

void fill_sectors(const rdoom::game::World &h, rdoom_map_sectors &m) {
  m = rdoom_map_sectors{h.map_sectors.data(), h.leaf_sector.data(), h.leaf_edges.data(), h.map_edges.data(), (uint32_t)h.map_sectors.size(),
                        (uint32_t)h.leaf_sector.size(), (uint32_t)h.map_edges.size()};
}

void fill_spawn(const rdoom::game::World &h, rdoom_spawn_table &t) {
  t = rdoom_spawn_table{h.spawn.data(), (uint32_t)h.spawn.size(), {h.start_pos[0], h.start_pos[1], h.start_pos[2]}, h.start_yaw};
}

void fill_triggers(const rdoom::game::World &h, rdoom_world_trigger_arrays &t) {
  std::memset(&t, 0, sizeof t);
  t.triggers = h.triggers.data();
  t.n_triggers = (uint32_t)h.triggers.size();
  t.effects = h.effects.data();
  t.n_effects = (uint32_t)h.effects.size();
  t.n_objects = h.game_objects;
}

WorldView view(const DevArrays &d, uint32_t n_dynamics, uint32_t node_depth) {
  return WorldView{d.nodes.get(), d.chunks.get(), d.tris.get(), d.verts.get(), d.dynamics.get(), n_dynamics, node_depth + 1};
}

// kernel(v, args...) with one lane per query, player or ray: one wave per workgroup, each lane's node stack in LDS
template <class Kernel, class... Args>
rdoom_status launch_lanes(Kernel kernel, uint32_t n_lanes, const WorldView &v, void *stream, Args... args) {
  return rdoom::launch_checked(kernel, dim3((n_lanes + WAVE - 1) / WAVE), dim3(WAVE), WAVE * v.stack_cap * sizeof(uint32_t), stream, v,
                               args...);
}
using rdoom::check_device;  // world_shared.hpp

GameView game_layout(const rdoom::game::World &h) {  // the layout include/rdoom.h documents at rdoom_world_game_bytes
  const uint32_t t = (uint32_t)h.triggers.size(), o = h.game_objects;
  const uint32_t lw = (t + 31) / 32, ow = (o + 31) / 32;
  GameView g{nullptr, nullptr, t, o, 4, 0, 0, 0, 0, 0, 0};
  g.fired = g.live + lw, g.active = g.fired + lw, g.second = g.active + ow, g.order = g.second + ow;
  g.effect = (g.order + t + 3) / 4 * 4;
  g.words = g.effect + 4 * o;
  return g;
}

GameView game_view(const rdoom_world *w) {
  GameView g = game_layout(w->host);
  g.triggers = w->d.triggers.get(), g.effects = w->d.effects.get();
  return g;
}

// the game arguments of a world's reset and step, or (set: d_levels too) a world set's
rdoom_status check_game(bool set, uint32_t game_objects, const void *d_game, const float *d_offsets, uint32_t n_objects,
                        const uint32_t *d_levels) {
  if (!d_game || !d_offsets || (set && !d_levels))
    return rdoom::fail(RDOOM_BAD_ARG, "%s", set ? "null game state, object offsets or levels" : "null game state or object offsets");
  if ((uintptr_t)d_game % 16) return rdoom::fail(RDOOM_BAD_ARG, "the game state is not 16-byte aligned");
  return rdoom::check_offsets(d_offsets, n_objects, game_objects, set ? "set" : "game");
}

rdoom_status check_offsets(const rdoom_world *w, const float *offsets, uint32_t n_objects) {
  return rdoom::check_offsets(offsets, n_objects, w->host.n_objects, "world");
}

// the arguments every step checks: states and inputs, and dt; resolves dt (0: 1/60) and the config (cfg null: the default) into c
rdoom_status step_args(const rdoom_player_state *d_states, const rdoom_player_input *d_inputs, uint32_t n_players, uint32_t n_ticks,
                       const rdoom_player_config *cfg, float &dt, rdoom_player_config &c) {
  if (n_players && (!d_states || (n_ticks && !d_inputs)))
    return rdoom::fail(RDOOM_BAD_ARG, "null states or inputs with n_players = %u", n_players);
  if (!(dt >= 0.0f) || dt == __builtin_inff()) return rdoom::fail(RDOOM_BAD_ARG, "dt %g is not a finite non-negative number", (double)dt);
  if (cfg) c = *cfg;
  else rdoom_player_config_default(&c);
  if (dt == 0.0f) dt = 1.0f / 60.0f;
  return RDOOM_OK;
}

// a game step's GameLevel, less the trigger and effect pointers (g's) the kernel takes as arguments of their own
GameLevel game_level(const GameView &g, void *d_game, float *d_offsets, const uint8_t *d_actions, uint32_t n_players, uint32_t n_objects,
                     float dt) {
  GameLevel level{};
  level.g = g;
  level.games = (uint32_t *)d_game;
  level.offsets = d_offsets;
  level.actions = d_actions;
  level.n = n_players, level.n_objects = n_objects;
  level.dt = dt;
  return level;
}
// the arguments of a ray cast, checked, as the kernel takes them.  world_objects: the world's (or the set's) collision objects
rdoom_status ray_args(const rdoom_player_state *d_states, uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                      const float *d_offsets, uint32_t n_objects, uint32_t world_objects, const char *noun, float *d_frac, uint32_t *d_hit,
                      float *d_origin, float *d_vel, RayArgs &a) {
  if (rdoom_status s = rdoom::check_fan(n_rays, max_range)) return s;
  if (!d_dirs) return rdoom::fail(RDOOM_BAD_ARG, "null ray directions");
  if (n && (!d_states || !d_frac)) return rdoom::fail(RDOOM_BAD_ARG, "null states or fraction output with n = %u", n);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, world_objects, noun)) return s;
  if ((uint64_t)n * n_rays > 0xFFFFFFFFull - WAVE) return rdoom::fail(RDOOM_BAD_ARG, "%u players x %u rays: too many for one launch", n, n_rays);
  a = RayArgs{d_states, d_dirs, d_offsets, d_frac, d_hit, d_origin, d_vel, n_rays, n_objects, n * n_rays, max_range};
  return RDOOM_OK;
}
}  // namespace

extern "C" {

void rdoom_world_destroy(rdoom_world *w) { delete w; }

rdoom_status rdoom_world_create(const rdoom_wad *wad, uint32_t level_index, uint32_t flags, rdoom_world **out_world) {
  if (!wad || !out_world) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (flags & ~RDOOM_WORLD_HOST_ONLY) return rdoom::fail(RDOOM_BAD_ARG, "unknown flags 0x%x", flags);
  *out_world = nullptr;
  return rdoom::guarded([&]() -> rdoom_status {  // (the host build and the uploads' tables are std containers)
    auto w = std::make_unique<rdoom_world>();
    w->host = rdoom::game::build_world(*rdoom::game::loaded_wad(wad), level_index);
    const rdoom::game::World &h = w->host;
    w->bounds = rdoom::line_bounds(h.map_lines.data(), h.map_lines.size());
    if (h.node_depth > RDOOM_WORLD_MAX_DEPTH)
      return rdoom::fail(RDOOM_BAD_LEVEL, "the level's BSP is %u nodes deep (at most %u)", h.node_depth, RDOOM_WORLD_MAX_DEPTH);
    if (!(flags & RDOOM_WORLD_HOST_ONLY)) {
      HIP_TRY(hipGetDevice(&w->device));
      if (rdoom_status st = upload_world(h, w->d)) return st;
      if (rdoom_status st = rdoom::map_upload(h.map_lines, {make_uint2(0u, (uint32_t)h.map_lines.size())}, w->map)) return st;
      if (rdoom_status st = rdoom::sector_upload({&h}, w->sectors)) return st;
      if (rdoom_status st = rdoom::spawn_upload({&h}, w->spawn)) return st;
      w->on_device = true;
    }
    *out_world = w.release();
    return RDOOM_OK;
  });
}

rdoom_status rdoom_world_host_arrays(const rdoom_world *w, rdoom_world_arrays *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  fill_arrays(w->host, *out);
  return RDOOM_OK;
}

rdoom_status rdoom_world_sweep(const rdoom_world *w, const float *d_spheres, const float *d_vels, uint32_t n,
                               const float *d_object_offsets, uint32_t n_objects, void *stream, float *d_out) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  if (n && (!d_spheres || !d_vels || !d_out)) return rdoom::fail(RDOOM_BAD_ARG, "null array with n = %u", n);
  if (rdoom_status s = check_offsets(w, d_object_offsets, n_objects)) return s;
  if (rdoom_status s = check_device(w, "the world")) return s;
  if (!n) return RDOOM_OK;
  return launch_lanes(sweep_kernel, n, view(w->d, (uint32_t)w->host.dynamics.size(), w->host.node_depth), stream, d_spheres, d_vels, n,
                      d_object_offsets, n_objects, d_out);
}

rdoom_status rdoom_player_config_default(rdoom_player_config *out) {
  if (!out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = rdoom_player_config{60.0f, 200.0f, 22.4f, 0.19f, 0.21f, 0.02f, 0.7f, 30.0f};  // player.rs:73-92
  return RDOOM_OK;
}

rdoom_status rdoom_world_step_players(const rdoom_world *w, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                      uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg, float dt,
                                      const float *d_object_offsets, uint32_t n_objects, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  rdoom_player_config c;
  if (rdoom_status s = step_args(d_states, d_inputs, n_players, n_ticks, cfg, dt, c)) return s;
  if (rdoom_status s = check_offsets(w, d_object_offsets, n_objects)) return s;
  if (rdoom_status s = check_device(w, "the world")) return s;
  if (!n_players || !n_ticks) return RDOOM_OK;
  return launch_lanes(player_step_kernel, n_players, view(w->d, (uint32_t)w->host.dynamics.size(), w->host.node_depth), stream, d_states,
                      d_inputs, n_players, n_ticks, c, dt, d_object_offsets, n_objects);
}

rdoom_status rdoom_world_triggers(const rdoom_world *w, rdoom_world_trigger_arrays *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  fill_triggers(w->host, *out);
  return RDOOM_OK;
}

rdoom_status rdoom_world_map_lines(const rdoom_world *w, rdoom_map_lines *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = rdoom_map_lines{w->host.map_lines.data(), (uint32_t)w->host.map_lines.size()};
  return RDOOM_OK;
}

rdoom_status rdoom_world_map_sectors(const rdoom_world *w, rdoom_map_sectors *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  fill_sectors(w->host, *out);
  return RDOOM_OK;
}

rdoom_status rdoom_world_map_things(const rdoom_world *w, rdoom_map_things *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = rdoom_map_things{w->host.things.data(), (uint32_t)w->host.things.size()};
  return RDOOM_OK;
}

rdoom_status rdoom_world_thing_obstacles(const rdoom_world *w, const uint32_t **out_words, uint32_t *out_n_words) {
  if (!w || !out_words || !out_n_words) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out_words = w->host.thing_obstacles.data();
  *out_n_words = (uint32_t)w->host.thing_obstacles.size();
  return RDOOM_OK;
}

rdoom_status rdoom_world_spawn_table(const rdoom_world *w, rdoom_spawn_table *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  fill_spawn(w->host, *out);
  return RDOOM_OK;
}

rdoom_status rdoom_world_game_bytes(const rdoom_world *w, uint64_t *bytes_per_player) {
  if (!w || !bytes_per_player) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *bytes_per_player = (uint64_t)game_view(w).words * sizeof(uint32_t);
  return RDOOM_OK;
}

rdoom_status rdoom_world_game_reset(const rdoom_world *w, void *d_game, float *d_object_offsets, uint32_t n_objects, uint32_t n,
                                    const uint8_t *d_mask, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  if (rdoom_status s = check_game(false, w->host.game_objects, d_game, d_object_offsets, n_objects, nullptr)) return s;
  if (rdoom_status s = check_device(w, "the world")) return s;
  if (!n) return RDOOM_OK;
  hipLaunchKernelGGL(game_reset_kernel, dim3(n), dim3(WAVE), 0, (hipStream_t)stream, game_view(w), (uint32_t *)d_game, d_object_offsets,
                     n_objects, d_mask);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

rdoom_status rdoom_world_step_game(const rdoom_world *w, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                   const uint8_t *d_actions, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                   uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg, float dt, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  rdoom_player_config c;
  if (rdoom_status s = step_args(d_states, d_inputs, n_players, n_ticks, cfg, dt, c)) return s;
  if (rdoom_status s = check_game(false, w->host.game_objects, d_game, d_object_offsets, n_objects, nullptr)) return s;
  if (rdoom_status s = check_device(w, "the world")) return s;
  if (!n_players || !n_ticks) return RDOOM_OK;
  const GameLevel level = game_level(game_view(w), d_game, d_object_offsets, d_actions, n_players, n_objects, dt);
  return launch_lanes(game_step_kernel, n_players, view(w->d, (uint32_t)w->host.dynamics.size(), w->host.node_depth), stream, level,
                      level.g.triggers, level.g.effects, d_states, d_inputs, n_ticks, c);
}

void rdoom_worldset_destroy(rdoom_worldset *s) { delete s; }

rdoom_status rdoom_worldset_create(const rdoom_wad *wad, const uint32_t *level_indices, uint32_t n_levels, uint32_t flags,
                                   rdoom_worldset **out_set) {
  if (!wad || !out_set || (n_levels && !level_indices)) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (flags & ~RDOOM_WORLD_HOST_ONLY) return rdoom::fail(RDOOM_BAD_ARG, "unknown flags 0x%x", flags);
  *out_set = nullptr;
  return rdoom::guarded([&]() -> rdoom_status {
    auto s = std::make_unique<rdoom_worldset>();
    s->host = rdoom::game::build_world_set(*rdoom::game::loaded_wad(wad), level_indices, n_levels);
    const rdoom::game::WorldSet &h = s->host;
    if (h.node_depth > RDOOM_WORLD_MAX_DEPTH)
      return rdoom::fail(RDOOM_BAD_LEVEL, "a level's BSP is %u nodes deep (at most %u)", h.node_depth, RDOOM_WORLD_MAX_DEPTH);
    for (size_t i = 0; i < h.levels.size(); i++) {
      const rdoom::game::World &l = h.levels[i];
      const rdoom::game::WorldSetLevel &t = h.table[i];
      const GameView g = game_layout(l);
      DevSetLevel r{};
      r.root = t.node_base, r.dyn_start = t.dynamic_base, r.n_dynamics = (uint32_t)l.dynamics.size(), r.destination = t.destination;
      r.trig_start = t.trigger_base, r.n_triggers = g.n_triggers, r.n_objects = g.n_objects, r.words = g.words;
      r.live = g.live, r.fired = g.fired, r.active = g.active, r.second = g.second, r.order = g.order, r.effect = g.effect;
      std::memcpy(r.start, l.start_pos, sizeof r.start);
      r.start_yaw = l.start_yaw;
      s->table.push_back(r);
      s->words = std::max(s->words, g.words);
      s->bounds.push_back(rdoom::line_bounds(l.map_lines.data(), l.map_lines.size()));
    }
    if (!(flags & RDOOM_WORLD_HOST_ONLY)) {
      HIP_TRY(hipGetDevice(&s->device));
      if (rdoom_status st = upload_world(h.all, s->d)) return st;
      if (rdoom_status st = s->d_table.upload(s->table, EMPTY_TABLE_BYTES)) return st;
      std::vector<uint32_t> tri_starts;
      for (const rdoom::game::WorldSetLevel &t : h.table) tri_starts.push_back(t.triangle_base);
      if (rdoom_status st = s->d_tri_starts.upload(tri_starts, EMPTY_TABLE_BYTES)) return st;
      std::vector<uint2> map_ranges;
      for (size_t i = 0; i < h.levels.size(); i++) map_ranges.push_back(make_uint2(h.table[i].map_base, (uint32_t)h.levels[i].map_lines.size()));
      if (rdoom_status st = rdoom::map_upload(h.all.map_lines, map_ranges, s->map)) return st;
      std::vector<const rdoom::game::World *> each;
      for (const rdoom::game::World &l : h.levels) each.push_back(&l);
      if (rdoom_status st = rdoom::sector_upload(each, s->sectors)) return st;
      if (rdoom_status st = rdoom::spawn_upload(each, s->spawn)) return st;
      s->on_device = true;
    }
    *out_set = s.release();
    return RDOOM_OK;
  });
}

rdoom_status rdoom_worldset_info(const rdoom_worldset *s, uint32_t *out_n_levels, uint32_t *out_n_objects) {
  if (!s) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (out_n_levels) *out_n_levels = (uint32_t)s->host.levels.size();
  if (out_n_objects) *out_n_objects = s->host.game_objects;
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level(const rdoom_worldset *s, uint32_t slot, rdoom_worldset_level_info *out) {
  if (!s || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  const rdoom::game::World &l = s->host.levels[slot];
  std::memset(out, 0, sizeof *out);
  out->archive_index = s->host.table[slot].archive_index;
  out->destination = s->host.table[slot].destination;
  std::memcpy(out->start_pos, l.start_pos, sizeof out->start_pos);
  out->start_yaw = l.start_yaw;
  out->n_triggers = (uint32_t)l.triggers.size();
  out->n_objects = l.game_objects;
  out->node_depth = l.node_depth;
  fill_arrays(l, out->world);
  fill_triggers(l, out->triggers);
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level_map_lines(const rdoom_worldset *s, uint32_t slot, rdoom_map_lines *out) {
  if (!s || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  const std::vector<rdoom_map_line> &lines = s->host.levels[slot].map_lines;
  *out = rdoom_map_lines{lines.data(), (uint32_t)lines.size()};
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level_map_sectors(const rdoom_worldset *s, uint32_t slot, rdoom_map_sectors *out) {
  if (!s || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  fill_sectors(s->host.levels[slot], *out);
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level_map_things(const rdoom_worldset *s, uint32_t slot, rdoom_map_things *out) {
  if (!s || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  const std::vector<rdoom_thing> &things = s->host.levels[slot].things;
  *out = rdoom_map_things{things.data(), (uint32_t)things.size()};
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level_thing_obstacles(const rdoom_worldset *s, uint32_t slot, const uint32_t **out_words, uint32_t *out_n_words) {
  if (!s || !out_words || !out_n_words) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  const std::vector<uint32_t> &words = s->host.levels[slot].thing_obstacles;
  *out_words = words.data();
  *out_n_words = (uint32_t)words.size();
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_level_spawn_table(const rdoom_worldset *s, uint32_t slot, rdoom_spawn_table *out) {
  if (!s || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (slot >= s->host.levels.size()) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %zu levels", slot, s->host.levels.size());
  fill_spawn(s->host.levels[slot], *out);
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_game_bytes(const rdoom_worldset *s, uint64_t *bytes_per_player) {
  if (!s || !bytes_per_player) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *bytes_per_player = (uint64_t)s->words * sizeof(uint32_t);
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_game_reset(const rdoom_worldset *s, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                       const uint32_t *d_levels, uint32_t n, const uint8_t *d_mask, void *stream) {
  if (!s) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (rdoom_status st = check_game(true, s->host.game_objects, d_game, d_object_offsets, n_objects, d_levels)) return st;
  if (rdoom_status st = check_device(s, "the world set")) return st;
  if (!n) return RDOOM_OK;
  hipLaunchKernelGGL(worldset_game_reset_kernel, dim3(n), dim3(WAVE), 0, (hipStream_t)stream, s->d_table.get(), (uint32_t)s->table.size(),
                     s->words, (uint32_t *)d_game, d_object_offsets, n_objects, d_levels, d_mask);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

rdoom_status rdoom_worldset_step_game(const rdoom_worldset *s, rdoom_player_state *d_states, const rdoom_player_input *d_inputs,
                                      const uint8_t *d_actions, void *d_game, float *d_object_offsets, uint32_t n_objects,
                                      uint32_t *d_levels, uint32_t n_players, uint32_t n_ticks, const rdoom_player_config *cfg,
                                      float dt, void *stream) {
  if (!s) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  rdoom_player_config c;
  if (rdoom_status st = step_args(d_states, d_inputs, n_players, n_ticks, cfg, dt, c)) return st;
  if (rdoom_status st = check_game(true, s->host.game_objects, d_game, d_object_offsets, n_objects, d_levels)) return st;
  if (rdoom_status st = check_device(s, "the world set")) return st;
  if (!n_players || !n_ticks) return RDOOM_OK;
  SetGame set{};
  set.gl = game_level(GameView{s->d.triggers.get(), s->d.effects.get(), 0, s->host.game_objects, 0, 0, 0, 0, 0, 0, s->words}, d_game,
                      d_object_offsets, d_actions, n_players, n_objects, dt);
  set.level_of = d_levels;
  set.n_levels = (uint32_t)s->table.size();
  return launch_lanes(worldset_game_step_kernel, n_players, view(s->d, 0u, s->host.node_depth), stream, set, s->d.triggers.get(), s->d.effects.get(),
                      s->d_table.get(), d_states, d_inputs, n_ticks, c);
}

rdoom_status rdoom_world_cast_rays(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                                   uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects,
                                   float *d_frac_out, uint32_t *d_hit_out, float *d_origin_out, float *d_vel_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  RayArgs a;
  if (rdoom_status s = ray_args(d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, w->host.n_objects, "world", d_frac_out,
                                d_hit_out, d_origin_out, d_vel_out, a))
    return s;
  if (rdoom_status s = check_device(w, "the world")) return s;
  if (!n) return RDOOM_OK;
  return launch_lanes(cast_rays_kernel, a.total, view(w->d, (uint32_t)w->host.dynamics.size(), w->host.node_depth), stream, a);
}

rdoom_status rdoom_worldset_cast_rays(const rdoom_worldset *s, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                      const float *d_dirs, uint32_t n_rays, float max_range, const float *d_object_offsets,
                                      uint32_t n_objects, float *d_frac_out, uint32_t *d_hit_out, float *d_origin_out, float *d_vel_out,
                                      void *stream) {
  if (!s) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  RayArgs a;
  if (rdoom_status st = ray_args(d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, s->host.all.n_objects, "world set",
                                 d_frac_out, d_hit_out, d_origin_out, d_vel_out, a))
    return st;
  if (rdoom_status st = check_device(s, "the world set")) return st;
  if (!n) return RDOOM_OK;
  return launch_lanes(worldset_cast_rays_kernel, a.total, view(s->d, 0u, s->host.node_depth), stream, a, s->d_table.get(),
                      s->d_tri_starts.get(), d_levels, (uint32_t)s->table.size());
}

}  // extern "C"
