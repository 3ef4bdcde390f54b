/* Test-side restatement of the game step with solid things, in binary32, sharing no code with the product.
 * The reference has no thing collision, so the thing contact is written from the contract alone: a plain loop over the things
 * with one bit test each.  game_restatement.c gives sweep_sphere, the vector helpers and the trigger and effect code;
 * tick() of world_restatement.c is static and has no hook, so the tick and the loop of rs_game_step are written out again here
 * with the one difference, and tests/test_solid_host.py pins the copy: with no blocking thing rs_solid_step equals rs_step and
 * rs_game_step bit for bit over the cases of tests/step_cases.py.
 * Built by the tests like game_restatement.c (tests/solid_ref.py). */
#include "game_restatement.c"

typedef struct { float x, z, base, radius; uint32_t object_id, sector; uint16_t thing_type, flags, category, angle; } thing_t; /* rdoom_thing */

typedef struct {
  const thing_t *things;
  uint32_t n_things;
  const uint32_t *solid;  /* the level's row, or NULL: every thing is solid */
  const uint32_t *hidden; /* the player's row, or NULL: nothing is hidden */
  float below, above;
} block_t;

static int row_bit(const uint32_t *row, uint32_t i) { return (int)((row[i / 32] >> (i % 32)) & 1u); }

/* off() of the map contract: the y of the object's row, 0 for object 0 and for an object beyond the row */
static float off_y(const float *off, uint32_t n_objects, uint32_t id) {
  if (!off || id == 0 || id >= n_objects) return 0.0f;
  return off[3 * (size_t)id + 1];
}

/* the things of the level against the sweep from pos along D, after the world's contact *c; the index of the thing whose contact
 * stands in *c afterwards, or -1 */
static int32_t thing_contact(const block_t *b, contact *c, vec pos, vec D, float body, const float *off, uint32_t n_objects) {
  int32_t which = -1;
  float a = D.x * D.x + D.z * D.z;
  if (!(a > 0.0f)) return -1;
  for (uint32_t i = 0; i < b->n_things; i++) {
    const thing_t *th = &b->things[i];
    if (b->solid && !row_bit(b->solid, i)) continue;
    if (b->hidden && row_bit(b->hidden, i)) continue;
    float y = th->base + off_y(off, n_objects, th->object_id);
    float dy = pos.y - y;
    if (!(dy >= -b->below && dy <= b->above)) continue;
    float cx = pos.x - th->x, cz = pos.z - th->z, R = body + th->radius;
    float bb = cx * D.x + cz * D.z;
    if (!(bb < 0.0f)) continue;
    float cc = (cx * cx + cz * cz) - R * R;
    float t, nx, nz;
    if (cc <= 0.0f) {
      t = 0.0f, nx = cx, nz = cz;
    } else {
      float disc = bb * bb - a * cc;
      if (!(disc >= 0.0f)) continue;
      t = (-bb - sqrtf(disc)) / a;
      nx = cx + D.x * t, nz = cz + D.z * t;
    }
    float m = sqrtf(nx * nx + nz * nz);
    if (!(m > 0.0f)) continue;
    if (t < c->time) {
      c->time = t;
      c->normal = mk(nx / m, 0.0f, nz / m);
      which = (int32_t)i;
    }
  }
  return which;
}

/* tick() of world_restatement.c, written out again, with the thing contact after the world's in every sweep of clip() */
static void tick_things(const world_t *w, pstate *s, const pinput *in, const pconfig *cfg, float dt, const float *offsets,
                        uint32_t n_objects, const block_t *blk, int32_t *bumped) {
  int fly = (s->flags & 1u) != 0, clip = (s->flags & 2u) != 0;
  vec head = mk(s->pos[0], s->pos[1], s->pos[2]);
  vec vel = mk(s->vel[0], s->vel[1], s->vel[2]);
  contact feet = sweep_sphere(w, head, 0.2f, mk(0.0f, -cfg->height, 0.0f), offsets);
  float height = cfg->height;
  int grounded = 0;
  vec gn = mk(0.0f, 0.0f, 0.0f);
  if (feet.time < INFINITY && feet.time < 1.0f) height = cfg->height * feet.time, gn = feet.normal, grounded = 1;
  float lim = 1.57079637f - 1e-2f;
  s->yaw = s->yaw - in->look[0];
  s->pitch = clampf_(s->pitch - in->look[1], -lim, lim);
  float sy, cy, sp, cp;
  rs_sincos(s->yaw, &sy, &cy);
  rs_sincos(s->pitch, &sp, &cp);
  vec force;
  if (fly) {
    vec m = vmul(vnorm0(mk(in->mv[0], in->jump ? 0.5f : 0.0f, in->mv[1])), cfg->move_force);
    float y1 = m.y * cp - m.z * sp;
    float z1 = m.y * sp + m.z * cp;
    force = mk(m.x * cy + z1 * sy, y1, z1 * cy - m.x * sy);
  } else {
    float fz = in->mv[1] * cp;
    vec m = vmul(vnorm0(mk(in->mv[0] * cy + fz * sy, 0.0f, fz * cy - in->mv[0] * sy)), cfg->move_force);
    if (grounded) {
      if (in->jump && vel.y < 0.1f) m = mk(m.x, 5.0f / dt, m.z);
    } else {
      m = vmul(m, 0.1f);
    }
    force = m;
  }
  float speed = vlen(vel);
  if (speed > 0.0f) {
    vec slow = mk(0.0f, 0.0f, 0.0f);
    if (fly) {
      slow = vmul(vneg(vel), cfg->friction / speed + cfg->ground_drag * speed);
    } else if (grounded) {
      vec tang = vsub(vel, vmul(gn, vdot(vel, gn)));
      float ts = vlen(tang);
      if (ts > 0.0f) slow = vmul(vneg(tang), cfg->friction / ts + cfg->ground_drag * ts);
    }
    slow = vsub(slow, vmul(vmul(vel, cfg->air_drag), speed));
    float sn = vlen(slow);
    if (sn > 0.0f) {
      float mx = -vdot(vel, slow) / sn / dt;
      if (sn >= mx) slow = vmul(vdiv(slow, sn), mx);
      force = vadd(force, slow);
    }
  }
  float hd = cfg->height - height;
  float der = (hd - s->lhd) / dt;
  s->lhd = hd;
  force.y = force.y + (hd * cfg->kp + der * cfg->kd);
  if (!fly) force.y = force.y - 17.0f;
  if (clip) {
    float left = dt;
    int armed = 1;
    for (int i = 0; i < 100; i++) {
      vec disp = vmul(vel, left);
      contact c = sweep_sphere(w, head, cfg->radius, disp, offsets);
      int32_t which = thing_contact(blk, &c, head, disp, cfg->radius, offsets, n_objects); /* the one difference */
      if (c.time < INFINITY) {
        float adj = c.time - 0.001f / vlen(disp);
        if (adj < 1.0f) {
          float tm = clampf_(c.time, 0.0f, 1.0f);
          if (which >= 0 && *bumped < 0) *bumped = which; /* clip() slides along a thing's contact */
          head = vadd(head, vmul(disp, adj));
          vel = vsub(vel, vmul(c.normal, vdot(c.normal, vel)));
          left = left * (1.0f - tm);
          continue;
        }
      }
      head = vadd(head, disp);
      armed = 0;
      break;
    }
    if (armed) s->flags |= 0x100u;
  } else {
    float old = head.y;
    head = vadd(head, vmul(vel, dt));
    if (!fly) {
      float H = 2000.0f;
      contact c = sweep_sphere(w, vadd(head, mk(0.0f, H / 2.0f, 0.0f)), cfg->radius, mk(0.0f, -H, 0.0f), offsets);
      float h = c.time < INFINITY ? head.y + H * (0.5f - c.time) : old;
      if (head.y <= h) {
        head.y = h;
        if (vel.y < 0.0f) vel.y = 0.0f;
      }
    }
  }
  vel = vadd(vel, vmul(force, dt));
  s->pos[0] = head.x, s->pos[1] = head.y, s->pos[2] = head.z;
  s->vel[0] = vel.x, s->vel[1] = vel.y, s->vel[2] = vel.z;
}

/* rs_game_step with the things of one level: `things` its n_things records, `solid` its row of bits or NULL, `hidden` n rows of
 * `stride` words or NULL, the window, and bumped[p], in and out: the first thing player p slid along, -1 while there is none */
void rs_solid_step(const world_t *w, const trig_t *trig, uint32_t n_trig, const effdef_t *effs, pstate *states, const pinput *inputs,
                   const uint8_t *actions, uint32_t n, uint32_t first, uint32_t count, uint32_t n_ticks, const float cfg[8], float dt,
                   float *offsets, uint32_t n_objects, uint32_t *order, uint32_t *counts, active_t *act, uint32_t *aflags,
                   const thing_t *things, uint32_t n_things, const uint32_t *solid, const uint32_t *hidden, uint32_t stride, float below,
                   float above, int32_t *bumped) {
  pconfig c;
  memcpy(&c, cfg, sizeof c);
  uint32_t *removed = (uint32_t *)malloc((n_trig + 1) * sizeof(uint32_t));
  for (uint32_t p = first; p < first + count && p < n; p++) {
    pstate *s = &states[p];
    float *off = offsets + (size_t)p * n_objects * 3;
    uint32_t *ord = order + (size_t)p * n_trig;
    active_t *a = act + (size_t)p * n_objects;
    uint32_t *af = aflags + (size_t)p * n_objects;
    block_t blk = {things, n_things, solid, hidden ? hidden + (size_t)p * stride : NULL, below, above};
    for (uint32_t t = 0; t < n_ticks; t++) {
      tick_things(w, s, &inputs[(size_t)t * n + p], &c, dt, off, n_objects, &blk, &bumped[p]);
      for (uint32_t o = 0; o < n_objects; o++) { /* Level::update: the effects, ascending object id */
        if (!(af[o] & 1u)) continue;
        uint32_t second = (af[o] >> 1) & 1u;
        int done = advance(&a[o], &second, &off[3 * o + 1], dt);
        af[o] = (done ? 0u : 1u) | (second << 1);
      }
      /* Level::poll_triggers */
      float mx = s->vel[0] * dt, mz = s->vel[2] * dt;
      line_t walked = line_od(s->pos[0], s->pos[2], -mx, -mz);
      uint32_t action = actions ? actions[(size_t)t * n + p] : 0u;
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
      for (uint32_t k = 0; k < counts[p]; k++) {
        const trig_t *tr = &trig[ord[k]];
        int hit = 0;
        switch (tr->trigger_type) {
          case WALK_OVER: hit = seg_offset(walked, tr); break;
          case PUSH:
          case SWITCH: hit = action == 1 && seg_offset(act_line, tr); break;
          case GUN: hit = action == 2 && seg_offset(act_line, tr); break;
          default: hit = seg_offset(walked, tr) || (action == 1 && seg_offset(act_line, tr)); break;
        }
        if (!hit) continue;
        for (uint32_t e = tr->e0; e < tr->e1; e++) {
          const effdef_t *d = &effs[e];
          active_t x = {d->first, d->second, d->wait, d->speed};
          a[d->obj] = x;
          af[d->obj] = 1u | (d->has_second ? 2u : 0u);
        }
        if (tr->flags & ONLY_ONCE) removed[n_removed++] = k;
        if (tr->flags & EXIT) s->flags |= 0x200u;
      }
      while (n_removed) { /* Vec::swap_remove, descending */
        uint32_t k = removed[--n_removed];
        ord[k] = ord[counts[p] - 1];
        counts[p]--;
      }
    }
  }
  free(removed);
}

/* the thing contact alone, for the cases the tests work out by hand: out = time, normal xyz; returns the thing or -1 */
int32_t rs_thing_contact(const thing_t *things, uint32_t n_things, const uint32_t *solid, const uint32_t *hidden, float below, float above,
                         const float world_contact[4], const float pos[3], const float D[3], float body, const float *off,
                         uint32_t n_objects, float out[4]) {
  block_t blk = {things, n_things, solid, hidden, below, above};
  contact c = {world_contact[0], {world_contact[1], world_contact[2], world_contact[3]}};
  int32_t which = thing_contact(&blk, &c, mk(pos[0], pos[1], pos[2]), mk(D[0], D[1], D[2]), body, off, n_objects);
  out[0] = c.time, out[1] = c.normal.x, out[2] = c.normal.y, out[3] = c.normal.z;
  return which;
}
