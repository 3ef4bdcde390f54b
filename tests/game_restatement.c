/* Test-side restatement of the level reacting to the player, in binary32, sharing no code with the product
 * (rust-doom_amd/csrc/hip/world.hip game_step_kernel): Level::poll_triggers (game/src/level.rs:77-167), the move effects of
 * Level::update (level.rs:203-255) and the tick order of the reference's systems, on top of world_restatement.c's tick().
 * It walks each player's trigger list in its current order, as the reference does, and keeps every effect in a per-object
 * table; the product's bit sets and its fast path for a single fired trigger are not restated.
 * Built by the tests like world_restatement.c (tests/game_ref.py). */
/* the census of this file's own branch outcomes (tests/test_game_census_host.py), appended to world_restatement.c's table and
 * counted only under -DRS_CENSUS, inside rs_game_step: seg_offset, the poll, the removals and advance */
#define RS_CENSUS_MORE_NAMES(X) \
  X(seg_parallel) X(seg_offset_negative) X(seg_offset_beyond) X(seg_other_negative) X(seg_other_beyond) X(seg_axis_x) X(seg_axis_y) \
  X(seg_hit) \
  X(walked_zero) X(walked_nonzero) X(action_push) X(action_shoot) X(action_clamped) \
  X(hit_walk_over) X(hit_push) X(hit_switch) X(hit_gun) X(hit_any_walk) X(hit_any_push) \
  X(fired_one_plain) X(fired_one_once) X(fired_two) X(fired_three_plus) X(fired_many_with_once) X(exit_alone) X(exit_with_others) \
  X(fired_index_32) X(fired_index_64) X(fired_index_96) X(trigger_no_effect) X(trigger_two_effects) \
  X(effect_on_active) X(effect_on_started_this_tick) X(object_id_32) \
  X(removed_one) X(removed_two_plus) X(removed_last) X(swapped_in_fired) X(dead_trigger_hit) \
  X(adv_up) X(adv_down) X(adv_arrived) X(adv_arrived_exactly) X(adv_at_first) X(adv_waiting) X(adv_wait_over) X(adv_wait_zero) \
  X(adv_second_started) X(adv_second_moving_same_tick) X(adv_second_arrives_same_tick) X(adv_done_with_second) \
  X(adv_done_without_second) X(adv_two_active) X(adv_speed_zero)
#include "world_restatement.c"

typedef struct { float ox, oy, dx, dy, len; uint32_t trigger_type, flags, special, e0, e1; } trig_t; /* rdoom_trigger */
typedef struct { uint32_t obj; float first, second, speed, wait; uint32_t has_second, repeat; } effdef_t; /* rdoom_move_effect */
typedef struct { float first, second, wait, speed; } active_t;

enum { WALK_OVER, PUSH, SWITCH, GUN, ANY };
enum { ONLY_ONCE = 1, EXIT = 2 };

typedef struct { float ox, oy, dx, dy, len; } line_t;

static line_t line_od(float ox, float oy, float vx, float vy) { /* Line2::from_origin_and_displace (math/src/line.rs:12-27) */
  line_t l;
  float len = sqrtf(vx * vx + vy * vy);
  l.ox = ox, l.oy = oy;
  if (fabsf(len) >= 1e-16f) l.dx = vx / len, l.dy = vy / len, l.len = len;
  else l.dx = 0.0f, l.dy = 0.0f, l.len = 0.0f;
  return l;
}

static int seg_offset(line_t a, const trig_t *b) { /* a.segment_intersect_offset(&b.line).is_some() (line.rs:47-84) */
  float den = a.dx * b->dy - a.dy * b->dx;
  if (fabsf(den) < 1e-16f) { CENSUS(seg_parallel); return 0; }
  float ex = b->ox - a.ox, ey = b->oy - a.oy;
  float off = (ex * b->dy - ey * b->dx) / den;
  CENSUS_IF(off < 0.0f, seg_offset_negative);
  CENSUS_IF(!(off < 0.0f) && off >= a.len, seg_offset_beyond);
  if (off < 0.0f || off >= a.len) return 0;
  float px = a.ox + a.dx * off, py = a.oy + a.dy * off;
  float other;
  CENSUS_IF(fabsf(b->dx) > fabsf(b->dy), seg_axis_x);
  CENSUS_IF(!(fabsf(b->dx) > fabsf(b->dy)), seg_axis_y);
  if (fabsf(b->dx) > fabsf(b->dy)) other = (px - b->ox) / b->dx;
  else other = (py - b->oy) / b->dy;
  CENSUS_IF(other < 0.0f, seg_other_negative);
  CENSUS_IF(!(other < 0.0f) && other >= b->len, seg_other_beyond);
  if (other < 0.0f || other >= b->len) return 0;
  CENSUS(seg_hit);
  return 1;
}

/* level.rs:203-255 for one effect; returns 1 when the effect is done.  (census) `leg`: the second legs started in this call --
 * adv_done_with_second is a call that starts the second leg and ends the effect, adv_done_without_second one that ends it only */
static int advance(active_t *e, uint32_t *has_second, float *current, float dt) {
  float timestep = dt;
  CENSUS_ONLY(int leg = 0;)
  CENSUS_IF(e->first == *current, adv_at_first);
  for (;;) {
    if (e->first != *current) {
      float diff = e->first - *current;
      float sign = diff < 0.0f ? -1.0f : 1.0f; /* f32::signum of a non-zero number */
      float time_left = fabsf(diff) / e->speed;
      CENSUS_IF(diff < 0.0f, adv_down);
      CENSUS_IF(!(diff < 0.0f), adv_up);
      CENSUS_IF(e->speed == 0.0f, adv_speed_zero);
      if (time_left > timestep) {
        CENSUS_IF(leg, adv_second_moving_same_tick);
        *current += sign * e->speed * timestep;
        return 0;
      }
      CENSUS(adv_arrived);
      CENSUS_IF(time_left == timestep, adv_arrived_exactly);
      CENSUS_IF(leg, adv_second_arrives_same_tick);
      *current = e->first;
      timestep -= time_left;
      e->first = *current;
    }
    if (e->wait > timestep) {
      CENSUS(adv_waiting);
      e->wait -= timestep;
      return 0;
    }
    CENSUS_IF(e->wait > 0.0f, adv_wait_over);
    CENSUS_IF(e->wait == 0.0f, adv_wait_zero);
    timestep -= e->wait;
    e->wait = 0.0f;
    if (*has_second) {
      CENSUS(adv_second_started);
      CENSUS_ONLY(leg++;)
      *has_second = 0;
      e->first = e->second;
      continue;
    }
    CENSUS_IF(leg, adv_done_with_second);
    CENSUS_IF(!leg, adv_done_without_second);
    return 1;
  }
}

/* players [first, first + count) of n for n_ticks ticks.  Per player p: order[p * n_trig ..] its trigger list and count[p] the
 * list's length; act[p * n_objects + o] the active effect on object o and aflags[..] its bits (1 active, 2 has a second offset);
 * offsets n x n_objects x xyz.  actions: n_ticks x n bytes or NULL. */
void rs_game_step(const world_t *w, const trig_t *trig, uint32_t n_trig, const effdef_t *effs, pstate *states, const pinput *inputs,
                  const uint8_t *actions, uint32_t n, uint32_t first, uint32_t count, uint32_t n_ticks, const float cfg[8], float dt,
                  float *offsets, uint32_t n_objects, uint32_t *order, uint32_t *counts, active_t *act, uint32_t *aflags) {
  pconfig c;
  memcpy(&c, cfg, sizeof c);
  uint32_t *removed = (uint32_t *)malloc((n_trig + 1) * sizeof(uint32_t));
  /* (census) per tick: the triggers fired, the objects an effect was started on, and the triggers in the list at the poll's start */
  CENSUS_ONLY(uint8_t *fired_now = (uint8_t *)calloc(n_trig + 1, 1); uint8_t *started_now = (uint8_t *)calloc(n_objects + 1, 1);
              uint8_t *listed = (uint8_t *)calloc(n_trig + 1, 1);)
  for (uint32_t p = first; p < first + count && p < n; p++) {
    pstate *s = &states[p];
    float *off = offsets + (size_t)p * n_objects * 3;
    uint32_t *ord = order + (size_t)p * n_trig;
    active_t *a = act + (size_t)p * n_objects;
    uint32_t *af = aflags + (size_t)p * n_objects;
    for (uint32_t t = 0; t < n_ticks; t++) {
      /* Player::update's physics against the offsets as the previous tick left them */
      tick(w, s, &inputs[(size_t)t * n + p], &c, dt, off);
      CENSUS_ONLY(rs_in_tick = 1;) /* (tick() counts its own and leaves the flag clear) */
      CENSUS_ONLY(uint32_t n_active = 0; for (uint32_t o = 0; o < n_objects; o++) n_active += af[o] & 1u;)
      CENSUS_IF(n_active >= 2, adv_two_active);
      /* Level::update: the effects, ascending object id (VecMap) */
      for (uint32_t o = 0; o < n_objects; o++) {
        if (!(af[o] & 1u)) continue;
        uint32_t second = (af[o] >> 1) & 1u;
        int done = advance(&a[o], &second, &off[3 * o + 1], dt);
        af[o] = (done ? 0u : 1u) | (second << 1);
      }
      /* Level::poll_triggers */
      float mx = s->vel[0] * dt, mz = s->vel[2] * dt;
      line_t walked = line_od(s->pos[0], s->pos[2], -mx, -mz);
      uint32_t action = actions ? actions[(size_t)t * n + p] : 0u;
      CENSUS_IF(walked.len == 0.0f, walked_zero);
      CENSUS_IF(walked.len != 0.0f, walked_nonzero);
      CENSUS_IF(action == 1, action_push);
      CENSUS_IF(action == 2, action_shoot);
      CENSUS_IF(action > 2, action_clamped);
      if (action > 2) action = 0;
      line_t act_line = walked;
      if (action) {
        float sx, cx, sy, cy;
        rs_sincos(s->pitch * 0.5f, &sx, &cx);
        rs_sincos(s->yaw * 0.5f, &sy, &cy);
        float sz = 0.0f, cz = 1.0f;
        float qs = -sx * sy * sz + cx * cy * cz, qx = sx * cy * cz + sy * sz * cx, qy = -sx * sz * cy + sy * cx * cz,
              qz = sx * sy * cz + sz * cx * cy;
        vec qv = mk(qx, qy, qz), v = mk(-0.0f, -0.0f, -1.0f);
        vec tmp = vadd(vcross(qv, v), vmul(v, qs));
        vec c2 = vcross(qv, tmp);
        vec look = mk(c2.x * 2.0f + v.x, c2.y * 2.0f + v.y, c2.z * 2.0f + v.z);
        float m = sqrtf(look.x * look.x + look.z * look.z);
        float d = m > 1.1920929e-7f ? m : 1.1920929e-7f;
        float lx = look.x / d, lz = look.z / d;
        float range = action == 1 ? 0.5f : 100.0f;
        act_line = line_od(s->pos[0], s->pos[2], lx * range, lz * range);
      }
      uint32_t n_removed = 0;
      CENSUS_ONLY(uint32_t n_fired = 0, n_once = 0, n_exit = 0; memset(listed, 0, n_trig);)
      for (uint32_t k = 0; k < counts[p]; k++) {
        const trig_t *tr = &trig[ord[k]];
        int hit = 0;
        CENSUS_ONLY(listed[ord[k]] = 1;)
        switch (tr->trigger_type) {
          case WALK_OVER: hit = seg_offset(walked, tr); CENSUS_IF(hit, hit_walk_over); break;
          case PUSH:
          case SWITCH: hit = action == 1 && seg_offset(act_line, tr); break;
          case GUN: hit = action == 2 && seg_offset(act_line, tr); CENSUS_IF(hit, hit_gun); break;
          default: hit = seg_offset(walked, tr) || (action == 1 && seg_offset(act_line, tr)); break;
        }
        if (!hit) continue;
        CENSUS_IF(tr->trigger_type == PUSH, hit_push);
        CENSUS_IF(tr->trigger_type == SWITCH, hit_switch);
        CENSUS_ONLY(if (tr->trigger_type > GUN) { /* by the walked line, or only by the push: asked again, uncounted */
          rs_in_tick = 0;
          int by_walk = seg_offset(walked, tr);
          rs_in_tick = 1;
          CENSUS_IF(by_walk, hit_any_walk);
          CENSUS_IF(!by_walk, hit_any_push);
        })
        CENSUS_ONLY(if (!n_fired) { memset(fired_now, 0, n_trig); memset(started_now, 0, n_objects); })
        CENSUS_ONLY(n_fired++; n_once += (tr->flags & ONLY_ONCE) != 0; n_exit += (tr->flags & EXIT) != 0; fired_now[ord[k]] = 1;)
        CENSUS_IF(ord[k] >= 32, fired_index_32);
        CENSUS_IF(ord[k] >= 64, fired_index_64);
        CENSUS_IF(ord[k] >= 96, fired_index_96);
        CENSUS_IF(tr->e1 == tr->e0, trigger_no_effect);
        CENSUS_IF(tr->e1 - tr->e0 >= 2 && tr->e1 > tr->e0, trigger_two_effects);
        for (uint32_t e = tr->e0; e < tr->e1; e++) {
          const effdef_t *d = &effs[e];
          active_t x = {d->first, d->second, d->wait, d->speed};
          CENSUS_IF((af[d->obj] & 1u) && !started_now[d->obj], effect_on_active);
          CENSUS_IF(started_now[d->obj], effect_on_started_this_tick);
          CENSUS_IF(d->obj >= 32, object_id_32);
          CENSUS_ONLY(started_now[d->obj] = 1;)
          a[d->obj] = x;
          af[d->obj] = 1u | (d->has_second ? 2u : 0u);
        }
        if (tr->flags & ONLY_ONCE) removed[n_removed++] = k;
        if (tr->flags & EXIT) s->flags |= 0x200u;
      }
      CENSUS_IF(n_fired == 1 && !n_once, fired_one_plain);
      CENSUS_IF(n_fired == 1 && n_once, fired_one_once);
      CENSUS_IF(n_fired == 2, fired_two);
      CENSUS_IF(n_fired >= 3, fired_three_plus);
      CENSUS_IF(n_fired >= 2 && n_once, fired_many_with_once);
      CENSUS_IF(n_exit && n_fired == 1, exit_alone);
      CENSUS_IF(n_exit && n_fired >= 2, exit_with_others);
      CENSUS_IF(n_removed == 1, removed_one);
      CENSUS_IF(n_removed >= 2, removed_two_plus);
      /* (census) the triggers that left the list earlier are not evaluated above; the product evaluates every line and looks at
       * its `live` bit after the geometric hit.  Counted here, with seg_offset's own outcomes left out */
      CENSUS_ONLY(if (counts[p] < n_trig) {
        uint32_t dead_hits = 0;
        rs_in_tick = 0;
        for (uint32_t i = 0; i < n_trig; i++) {
          if (listed[i]) continue;
          const trig_t *tr = &trig[i];
          switch (tr->trigger_type) {
            case WALK_OVER: dead_hits += seg_offset(walked, tr); break;
            case PUSH:
            case SWITCH: dead_hits += action == 1 && seg_offset(act_line, tr); break;
            case GUN: dead_hits += action == 2 && seg_offset(act_line, tr); break;
            default: dead_hits += seg_offset(walked, tr) || (action == 1 && seg_offset(act_line, tr)); break;
          }
        }
        rs_in_tick = 1;
        if (dead_hits) CENSUS(dead_trigger_hit);
      })
      while (n_removed) { /* Vec::swap_remove, descending */
        uint32_t k = removed[--n_removed];
        CENSUS_IF(k == counts[p] - 1, removed_last);
        CENSUS_IF(k != counts[p] - 1 && fired_now[ord[counts[p] - 1]], swapped_in_fired);
        ord[k] = ord[counts[p] - 1];
        counts[p]--;
      }
      CENSUS_ONLY(rs_in_tick = 0;)
    }
  }
  free(removed);
  CENSUS_ONLY(free(fired_now); free(started_now); free(listed);)
}

/* rdoom_object_modelviews_from_player's concat, restated from cgmath: the view of the player (rdoom_pose_from_player's
 * arithmetic, libm sinf / cosf) concatenated with a translation by `off` */
typedef struct { float s, x, y, z; } quat;
static vec qrot(quat q, vec v) {
  vec qv = mk(q.x, q.y, q.z);
  vec tmp = vadd(vcross(qv, v), vmul(v, q.s));
  vec c2 = vcross(qv, tmp);
  return mk(c2.x * 2.0f + v.x, c2.y * 2.0f + v.y, c2.z * 2.0f + v.z);
}
static quat qmul(quat a, quat b) {
  quat r = {a.s * b.s - a.x * b.x - a.y * b.y - a.z * b.z, a.s * b.x + a.x * b.s + a.y * b.z - a.z * b.y,
            a.s * b.y + a.y * b.s + a.z * b.x - a.x * b.z, a.s * b.z + a.z * b.s + a.x * b.y - a.y * b.x};
  return r;
}
void rs_object_modelview(const float pos[3], float yaw, float pitch, const float off[3], float out[16]) {
  float sx = sinf(pitch * 0.5f), cx = cosf(pitch * 0.5f), sy = sinf(yaw * 0.5f), cy = cosf(yaw * 0.5f), sz = 0.0f, cz = 1.0f;
  quat pl = {-sx * sy * sz + cx * cy * cz, sx * cy * cz + sy * sz * cx, -sx * sz * cy + sy * cx * cz, sx * sy * cz + sz * cx * cy};
  quat id = {1.0f, 0.0f, 0.0f, 0.0f};
  quat rot = qmul(pl, id);
  vec rc = qrot(pl, mk(0.0f, 0.12f, 0.0f));
  vec disp = mk(rc.x + pos[0], rc.y + pos[1], rc.z + pos[2]);
  float vv = (rot.x * rot.x + rot.y * rot.y) + rot.z * rot.z;
  float mag2 = rot.s * rot.s + vv;
  quat r = {rot.s / mag2, -rot.x / mag2, -rot.y / mag2, -rot.z / mag2};
  vec rd = qrot(r, disp);
  vec d = mk(rd.x * -1.0f, rd.y * -1.0f, rd.z * -1.0f);
  /* view.concat(model): rot = r * identity, disp = r.rotate(off * 1) + d, scale 1 */
  quat cr = qmul(r, id);
  vec ro = qrot(r, mk(off[0] * 1.0f, off[1] * 1.0f, off[2] * 1.0f));
  vec cd = mk(ro.x + d.x, ro.y + d.y, ro.z + d.z);
  float x2 = cr.x + cr.x, y2 = cr.y + cr.y, z2 = cr.z + cr.z;
  float xx2 = x2 * cr.x, xy2 = x2 * cr.y, xz2 = x2 * cr.z, yy2 = y2 * cr.y, yz2 = y2 * cr.z, zz2 = z2 * cr.z;
  float sy2 = y2 * cr.s, sz2 = z2 * cr.s, sx2 = x2 * cr.s;
  float m3[9] = {1.0f - yy2 - zz2, xy2 + sz2, xz2 - sy2, xy2 - sz2, 1.0f - xx2 - zz2, yz2 + sx2, xz2 + sy2, yz2 - sx2, 1.0f - xx2 - yy2};
  memset(out, 0, 16 * sizeof(float));
  for (int col = 0; col < 3; col++)
    for (int row = 0; row < 3; row++) out[col * 4 + row] = m3[col * 3 + row] * 1.0f;
  out[12] = cd.x, out[13] = cd.y, out[14] = cd.z, out[15] = 1.0f;
}
