/* Test-side restatement of the player cameras on the device (rust-doom_amd/csrc/hip/frames.hip player_frames_kernel), sharing no
 * code with the product: cgmath's Quaternion::from(Euler), Decomposed::concat / inverse_transform and Matrix4::from(Decomposed)
 * in binary32 (game/src/player.rs:325-345, engine/src/renderer.rs:78-132), with sine and cosine from world_restatement.c's twin
 * of the project's sincos.  Also the render's per-pose sky angle both ways: glibc atan2f, as the host path computes it, and
 * binary64 atan2 rounded once, as the device does.  Built by the tests like world_restatement.c (tests/frames_ref.py). */
#include "world_restatement.c"

typedef struct { float s, x, y, z; } quat;  /* (vec, mk and vcross are world_restatement.c's) */

static vec qrot(quat q, vec v) { /* v * q: tmp = q.v x v + v q.s; (q.v x tmp) 2 + v */
  vec qv = mk(q.x, q.y, q.z);
  vec c = vcross(qv, v);
  vec t = mk(c.x + v.x * q.s, c.y + v.y * q.s, c.z + v.z * q.s);
  vec c2 = vcross(qv, t);
  return mk(c2.x * 2.0f + v.x, c2.y * 2.0f + v.y, c2.z * 2.0f + v.z);
}

static quat qprod(quat a, quat b) {
  quat r;
  r.s = a.s * b.s - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.s * b.x + a.x * b.s + a.y * b.z - a.z * b.y;
  r.y = a.s * b.y + a.y * b.s + a.z * b.x - a.x * b.z;
  r.z = a.s * b.z + a.z * b.s + a.x * b.y - a.y * b.x;
  return r;
}

static void to_matrix(float scale, quat r, vec d, float *m) { /* Matrix3::from(Quaternion) * scale, w = disp */
  float x2 = r.x + r.x, y2 = r.y + r.y, z2 = r.z + r.z;
  float xx2 = x2 * r.x, xy2 = x2 * r.y, xz2 = x2 * r.z, yy2 = y2 * r.y, yz2 = y2 * r.z, zz2 = z2 * r.z;
  float sy2 = y2 * r.s, sz2 = z2 * r.s, sx2 = x2 * r.s;
  float cols[3][3] = {{1.0f - yy2 - zz2, xy2 + sz2, xz2 - sy2}, {xy2 - sz2, 1.0f - xx2 - zz2, yz2 + sx2}, {xz2 + sy2, yz2 - sx2, 1.0f - xx2 - yy2}};
  for (int c = 0; c < 3; c++) {
    for (int k = 0; k < 3; k++) m[4 * c + k] = cols[c][k] * scale;
    m[4 * c + 3] = 0.0f;
  }
  m[12] = d.x, m[13] = d.y, m[14] = d.z, m[15] = 1.0f;
}

/* n states -> n poses (modelview, projection, time, pad: 34 floats) and, when offsets, n x n_objects x 16 modelviews */
void fr_cameras(const pstate *st, uint32_t n, const float *proj, float time, const float *offsets, uint32_t n_objects, float *poses,
                float *mvs) {
  for (uint32_t p = 0; p < n; p++) {
    float sx, cx, sy, cy, sz = 0.0f, cz = 1.0f;
    rs_sincos(st[p].pitch * 0.5f, &sx, &cx);
    rs_sincos(st[p].yaw * 0.5f, &sy, &cy);
    quat q;  /* Quaternion::from(Euler { x: pitch, y: yaw, z: 0 }) */
    q.s = -sx * sy * sz + cx * cy * cz;
    q.x = sx * cy * cz + sy * sz * cx;
    q.y = -sx * sz * cy + sy * cx * cz;
    q.z = sx * sy * cz + sz * cx * cy;
    quat one = {1.0f, 0.0f, 0.0f, 0.0f};
    float scale = 1.0f * 1.0f;
    quat rot = qprod(q, one);  /* player.concat(camera) */
    vec head = qrot(q, mk(0.0f * 1.0f, 0.12f * 1.0f, 0.0f * 1.0f));
    vec disp = mk(head.x + st[p].pos[0], head.y + st[p].pos[1], head.z + st[p].pos[2]);
    float inv = 1.0f / scale;  /* inverse_transform */
    float m2 = rot.s * rot.s + ((rot.x * rot.x + rot.y * rot.y) + rot.z * rot.z);
    quat r = {rot.s / m2, -rot.x / m2, -rot.y / m2, -rot.z / m2};
    vec rd = qrot(r, disp);
    vec d = mk(rd.x * -inv, rd.y * -inv, rd.z * -inv);
    float *pose = poses + 34 * (size_t)p;
    to_matrix(inv, r, d, pose);
    memcpy(pose + 16, proj, 16 * sizeof(float));
    pose[32] = time, pose[33] = 0.0f;
    if (!offsets) continue;
    for (uint32_t o = 0; o < n_objects; o++) {
      const float *off = offsets + 3 * ((size_t)p * n_objects + o);
      float *m = mvs + 16 * ((size_t)p * n_objects + o);
      if (o == 0 || (off[0] == 0.0f && off[1] == 0.0f && off[2] == 0.0f)) {
        memcpy(m, pose, 16 * sizeof(float));
        continue;
      }
      vec od = qrot(r, mk(off[0] * inv, off[1] * inv, off[2] * inv));  /* view.concat(model_o) */
      to_matrix(inv * 1.0f, qprod(r, one), mk(od.x + d.x, od.y + d.y, od.z + d.z), m);
    }
  }
}

/* PM = P * M in the renderer's V1 order, then sky.vert's angle atan2(PM[8], PM[10]): host = glibc atan2f, cr = binary64 rounded */
void fr_sky_angles(const float *proj, const float *mvs, uint32_t n, float *host, float *cr) {
  for (uint32_t i = 0; i < n; i++) {
    const float *m = mvs + 16 * (size_t)i;
    float pm[16];
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++)
        pm[4 * c + r] = ((proj[r] * m[4 * c] + proj[4 + r] * m[4 * c + 1]) + proj[8 + r] * m[4 * c + 2]) + proj[12 + r] * m[4 * c + 3];
    host[i] = atan2f(pm[8], pm[10]);
    cr[i] = (float)atan2((double)pm[8], (double)pm[10]);
  }
}
