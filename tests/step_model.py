"""A float64 model of Player::update (the reference's game/src/player.rs:142-311, 359-395) for players over one infinite horizontal
floor, in plain numpy, sharing nothing with tests/world_restatement.c: no BSP, no triangles and no general sphere sweep -- of
math/src/sphere.rs only the plane branch (:23-53).  It is the reference's arithmetic in binary64, so it differs from the product
and from the restatement by binary32 rounding accumulated over the ticks; tests/golden/step_model_error.json records how much.

The model holds while no wall and no ceiling is in reach and no sphere overlaps the floor's plane (where the reference goes on to
a triangle's edges and vertices, sphere.rs:55-119, which an infinite plane does not have): `Trace` records what a test needs to
assert that of every case."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)  # Scalar::default_epsilon of normalize_or_zero (math/src/lib.rs:40-46)
PITCH_LIMIT = np.pi / 2 - 1e-2         # player.rs:208-214
FEET_RADIUS = 0.2                      # player.rs:253-256


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _normalize_or_zero(v):
    return v / np.maximum(_norm(v), EPS)[..., None]  # math/src/lib.rs:40-42


def plane_sweep(y, radius, disp, floor):
    """Sphere::sweep_triangle (sphere.rs:16-53, 121-125) of spheres centred at height y against the plane y = floor (normal +y),
    moved by disp (n, 3): the contact time, +inf for None.  (overlap: the sphere is through the plane, :41-45 -- no plane contact)"""
    speed = _norm(disp)                                    # sphere.rs:23
    moving = speed > 0.0                                   # sphere.rs:24-26
    safe = np.where(moving, speed, 1.0)
    normal_dot_nvel = disp[:, 1] / safe                    # sphere.rs:27-28, normal = (0, 1, 0)
    towards = moving & (normal_dot_nvel < 0.0)             # sphere.rs:30-32
    signed = y - floor                                     # sphere.rs:37-40
    outside = signed >= radius                             # sphere.rs:45
    hit = towards & outside
    distance = -(signed - radius) / np.where(hit, normal_dot_nvel, -1.0)  # sphere.rs:46 (:48: every point of the plane is inside)
    time = np.where(hit, distance / safe, np.inf)          # sphere.rs:49-51, 121-125
    overlap = towards & ~outside & (signed >= -radius)     # sphere.rs:41-43 passed, :45 not
    return time, overlap


class Trace:
    """what a run came near: per player and tick the horizontal position, the head's top, whether a sphere overlapped the floor,
    and whether noclip() put the head sphere on the floor (player.rs:183-187)"""

    def __init__(self):
        self.x, self.z, self.top, self.overlap, self.landed = [], [], [], [], []

    def valid_ticks(self, lo, hi, ceiling, margin):
        """per player, the ticks before the first at which a wall of the box [lo, hi]^2 is within `margin` (radius + 0.3), the
        ceiling within the head sphere's reach, or a sphere overlaps the floor"""
        x, z, top, ov = (np.array(a) for a in (self.x, self.z, self.top, self.overlap))
        bad = (x - lo <= margin) | (hi - x <= margin) | (z - lo <= margin) | (hi - z <= margin) | (top >= ceiling - 0.05) | ov
        first = np.where(bad.any(0), bad.argmax(0), len(bad))
        return first

    def first_landing(self):
        """per player, the tick of its first landing in noclip(), or the number of ticks where it never lands"""
        landed = np.array(self.landed)
        return np.where(landed.any(0), landed.argmax(0), len(landed))


def step(states, inputs, config, dt, floor=0.0, trace=None, n_ticks=None):
    """`states` (n PLAYER_STATE records) after the ticks of `inputs` ((n_ticks, n) PLAYER_INPUT records), as float64 arrays in a
    dict (pos, vel, yaw, pitch, last_height_diff; landings: the ticks in which noclip() put the head sphere on the floor,
    player.rs:183-187).  n_ticks: None, or per player the ticks it runs (the others leave it frozen).
    config: a mapping of the eight fields.  dt > 0."""
    c = {k: float(config[k]) for k in ('move_force', 'spring_const_p', 'spring_const_d', 'radius', 'height', 'air_drag',
                                      'ground_drag', 'friction')}
    n = len(states)
    pos = np.array(states['pos'], np.float64)
    vel = np.array(states['vel'], np.float64)
    yaw, pitch = np.array(states['yaw'], np.float64), np.array(states['pitch'], np.float64)
    lhd = np.array(states['last_height_diff'], np.float64)
    fly, clip = (states['flags'] & 1) != 0, (states['flags'] & 2) != 0
    up = np.array([0.0, 1.0, 0.0])
    landings = np.zeros(n, np.int64)
    for t in range(len(inputs)):
        live = np.ones(n, bool) if n_ticks is None else t < np.asarray(n_ticks)
        before = (pos.copy(), vel.copy(), yaw.copy(), pitch.copy(), lhd.copy())
        mv = np.array(inputs['movement'][t], np.float64)
        look = np.array(inputs['look'][t], np.float64)
        jump = np.array(inputs['jump'][t]) != 0
        overlap = np.zeros(n, bool)
        # force(): the feet probe (player.rs:253-267)
        probe = np.zeros((n, 3))
        probe[:, 1] = -c['height']                                         # player.rs:257
        ftime, ov = plane_sweep(pos[:, 1], FEET_RADIUS, probe, floor)      # player.rs:258
        overlap |= ov
        grounded = ftime < 1.0                                             # player.rs:260
        height = np.where(grounded, c['height'] * ftime, c['height'])      # player.rs:261-266
        # move_force() (player.rs:192-241); the rotation is Ry(yaw) Rx(pitch), yaw -= look.x, pitch clamped (:207-217)
        yaw = yaw - look[:, 0]                                             # player.rs:215
        pitch = np.clip(pitch - look[:, 1], -PITCH_LIMIT, PITCH_LIMIT)     # player.rs:207-214, 217
        sy, cy, sp, cp = np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch)

        def rotate(v):  # rot.rotate_vector: Rx(pitch) first, then Ry(yaw)
            y1 = v[:, 1] * cp - v[:, 2] * sp
            z1 = v[:, 1] * sp + v[:, 2] * cp
            return np.stack([v[:, 0] * cy + z1 * sy, y1, z1 * cy - v[:, 0] * sy], 1)

        fly_in = np.stack([mv[:, 0], np.where(jump, 0.5, 0.0), mv[:, 1]], 1)      # player.rs:220
        fly_force = rotate(_normalize_or_zero(fly_in) * c['move_force'])          # player.rs:221-223
        walk = rotate(np.stack([mv[:, 0], np.zeros(n), mv[:, 1]], 1))             # player.rs:225-227
        walk[:, 1] = 0.0                                                          # player.rs:228
        walk = _normalize_or_zero(walk) * c['move_force']                         # player.rs:229-230
        jumping = grounded & jump & (vel[:, 1] < 0.1)                             # player.rs:231-232
        walk[:, 1] = np.where(jumping, 5.0 / dt, walk[:, 1])                      # player.rs:233
        walk = np.where(grounded[:, None], walk, walk * 0.1)                      # player.rs:237-238
        force = np.where(fly[:, None], fly_force, walk)                           # player.rs:219, 224
        # the slowdown (player.rs:276-301)
        speed = _norm(vel)                                                        # player.rs:276
        s1 = np.where(speed > 0.0, speed, 1.0)
        tangential = vel - up * vel[:, 1:2]                                       # player.rs:281, normal = (0, 1, 0)
        ts = _norm(tangential)                                                    # player.rs:282
        t1 = np.where(ts > 0.0, ts, 1.0)
        ground_slow = np.where((ts > 0.0)[:, None], -tangential * (c['friction'] / t1 + c['ground_drag'] * t1)[:, None], 0.0)  # :283-287
        fly_slow = -vel * (c['friction'] / s1 + c['ground_drag'] * s1)[:, None]   # player.rs:279
        slowdown = np.where(fly[:, None], fly_slow, np.where(grounded[:, None], ground_slow, 0.0))  # player.rs:278-290
        slowdown = slowdown - vel * c['air_drag'] * speed[:, None]                # player.rs:291
        sn = _norm(slowdown)                                                      # player.rs:293
        sn1 = np.where(sn > 0.0, sn, 1.0)
        max_slowdown = -(vel * slowdown).sum(1) / sn1 / dt                        # player.rs:295
        slowdown = np.where((sn >= max_slowdown)[:, None], slowdown / sn1[:, None] * max_slowdown[:, None], slowdown)  # :296-298
        force = force + np.where(((speed > 0.0) & (sn > 0.0))[:, None], slowdown, 0.0)  # player.rs:277, 294, 299
        # the spring and gravity (player.rs:302-309)
        height_diff = c['height'] - height                                        # player.rs:302
        derivative = (height_diff - lhd) / dt                                     # player.rs:303
        lhd = height_diff                                                         # player.rs:304
        force[:, 1] += height_diff * c['spring_const_p'] + derivative * c['spring_const_d']  # player.rs:305
        force[:, 1] -= np.where(fly, 0.0, 17.0)                                   # player.rs:307-309
        # clip() (player.rs:142-166)
        cpos, cvel = pos.copy(), vel.copy()
        time_left = np.full(n, dt)                                                # player.rs:143
        active = clip.copy()
        for _ in range(100):                                                      # player.rs:145
            if not active.any():
                break
            disp = cvel * time_left[:, None]                                      # player.rs:146
            ctime, ov = plane_sweep(cpos[:, 1], c['radius'], disp, floor)         # player.rs:147
            overlap |= ov & active
            dn = _norm(disp)
            adjusted = ctime - 0.001 / np.where(dn > 0.0, dn, 1.0)                # player.rs:148
            contact = active & np.isfinite(ctime) & (adjusted < 1.0)              # player.rs:147, 149
            free = active & ~contact
            cpos = np.where(contact[:, None], cpos + disp * np.where(contact, adjusted, 0.0)[:, None], cpos)  # player.rs:151-152
            cvel = np.where(contact[:, None], cvel - up * cvel[:, 1:2], cvel)     # player.rs:153, normal = (0, 1, 0)
            time_left = np.where(contact, time_left * (1.0 - np.clip(ctime, 0.0, 1.0)), time_left)  # player.rs:150, 154
            cpos = np.where(free[:, None], cpos + disp, cpos)                     # player.rs:158
            active = contact                                                      # player.rs:155, 159-160
        assert not active.any(), 'clip() did not end (player.rs:163-165)'
        # noclip() (player.rs:168-190)
        npos, nvel = pos + vel * dt, vel.copy()                                   # player.rs:169-170
        down = np.zeros((n, 3))
        down[:, 1] = -2000.0                                                      # player.rs:173, 178
        ptime, ov = plane_sweep(npos[:, 1] + 1000.0, c['radius'], down, floor)    # player.rs:174-178
        overlap |= ov & ~clip & ~fly
        h = np.where(np.isfinite(ptime), npos[:, 1] + 2000.0 * (0.5 - ptime), pos[:, 1])  # player.rs:179-180
        landed = ~fly & (npos[:, 1] <= h)                                         # player.rs:172, 183
        npos[:, 1] = np.where(landed, h, npos[:, 1])                              # player.rs:184
        nvel[:, 1] = np.where(landed & (nvel[:, 1] < 0.0), 0.0, nvel[:, 1])       # player.rs:185-187
        landings += landed & ~clip & live  # (the ticks in which noclip()'s probe set the height)
        pos = np.where(clip[:, None], cpos, npos)                                 # player.rs:388-394
        vel = np.where(clip[:, None], cvel, nvel)
        vel = vel + force * dt                                                    # player.rs:395
        if n_ticks is not None:
            f = ~live
            pos[f], vel[f], yaw[f], pitch[f], lhd[f] = before[0][f], before[1][f], before[2][f], before[3][f], before[4][f]
        if trace is not None:
            trace.x.append(pos[:, 0].copy()), trace.z.append(pos[:, 2].copy())
            trace.top.append(pos[:, 1] + c['radius']), trace.overlap.append(overlap & live)
            trace.landed.append(landed & ~clip & live)
    return dict(pos=pos, vel=vel, yaw=yaw, pitch=pitch, last_height_diff=lhd, landings=landings)
