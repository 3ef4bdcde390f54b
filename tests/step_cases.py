"""The shared cases of the player step away from its default config and tick length: the configs, the tick lengths, the scripted
inputs and players of tests/test_gpu_world.py (moved here; that file imports them back), and the cases of the float64 model
(tests/step_model.py) in room A of the analytic level.  Used by tests/test_step_configs_host.py, tests/test_step_model_host.py,
tests/gpu_step_child.py and tests/golden/make_step_model_error.py.  Also the players of tests/test_gpu_game.py and
tests/test_gpu_worldset.py, and the `rare` family: the branch outcomes of the step that none of those inputs takes
(tests/step_census.py, tests/test_gpu_step_rare.py).  Nothing here needs torch or a device."""
import os

import numpy as np

import game_ref
import rust_doom_amd as rd
import step_model
import world_ref

F = np.float32
FIELDS = ('move_force', 'spring_const_p', 'spring_const_d', 'radius', 'height', 'air_drag', 'ground_drag', 'friction')
DEFAULT = (60.0, 200.0, 22.4, 0.19, 0.21, 0.02, 0.7, 30.0)  # Config::default (player.rs:72-92)
# one field changed by at least 25 %, the others at their defaults
SINGLE = [('move_force', 35.0), ('spring_const_p', 320.0), ('spring_const_d', 12.0), ('radius', 0.12), ('radius', 0.26),
          ('height', 0.30), ('air_drag', 0.2), ('ground_drag', 1.4), ('friction', 12.0)]
# every field changed, each by at least 25 % of its default
ALL_FIELDS = {'all_a': (45.0, 260.0, 30.0, 0.14, 0.27, 0.05, 1.0, 20.0), 'all_b': (90.0, 150.0, 16.0, 0.24, 0.28, 0.0, 0.4, 40.0)}

DT_DEFAULT = 1.0 / 60.0
DTS = {'35': 1.0 / 35.0, '120': 1.0 / 120.0, '30': 1.0 / 30.0, '0': 0.0}  # 0 means 1/60, bit for bit (include/rdoom.h)
N_PLAYERS, N_TICKS = 256, 120
LEVELS = (0, 1)  # E1M1 and the analytic two-room level (tools/mkwad.py: kat_level)


def config(values):
    """a PLAYER_CONFIG record of the eight values in FIELDS' order"""
    cfg = np.zeros(1, rd.PLAYER_CONFIG)[0]
    for name, v in zip(FIELDS, values):
        cfg[name] = v
    return cfg


def _single(name, value):
    v = list(DEFAULT)
    v[FIELDS.index(name)] = value
    return tuple(v)


def configs():
    """{name: eight values}: the default, the single-field configs and the two all-field ones, in a fixed order"""
    out = {'default': DEFAULT}
    for name, value in SINGLE:
        out['%s=%g' % (name, value)] = _single(name, value)
    out.update(ALL_FIELDS)
    return out


CONFIGS = configs()
SINGLE_NAMES = [k for k in CONFIGS if '=' in k]


def resolve_dt(dt):
    """the tick length a step runs with: 0 means 1/60 (include/rdoom.h)"""
    return DT_DEFAULT if dt == 0 else dt


def check_domain():
    """what the issue keeps of every config: friction < move_force, spring_const_d * dt < 2, the head sphere's bottom above the
    floor at rest, and at least 25 % between a changed field and its default"""
    for name, v in CONFIGS.items():
        c = dict(zip(FIELDS, v))
        assert c['friction'] < c['move_force'], name
        assert all(c['spring_const_d'] * resolve_dt(dt) < 2 for dt in DTS.values()), name
        assert 0.2 + c['height'] - 17.0 / c['spring_const_p'] - c['radius'] > 0, name
        changed = [f for f, d in zip(FIELDS, DEFAULT) if c[f] != d]
        assert all(abs(c[f] - d) >= 0.25 * d for f, d in zip(FIELDS, DEFAULT) if f in changed), name
        assert len(changed) == (0 if name == 'default' else 1 if '=' in name else 8), name


def script(n, ticks, seed):
    """scripted inputs, player p runs script p % 6: walk forward (into whatever wall is ahead), strafe, jump while walking,
    look up while walking, stand still, turn and walk with random look"""
    rng = np.random.default_rng(seed)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    s = np.arange(n) % 6
    t = np.arange(ticks)[:, None]
    inp['movement'][:, :, 1] = np.where((s == 0) | (s == 2) | (s == 3) | (s == 5), -1.0, 0.0)
    inp['movement'][:, :, 0] = np.where(s == 1, 1.0, np.where(s == 0, (t > 150) * 1.0, 0.0))  # into the wall, then strafe along it
    inp['jump'] = np.where((s == 2) & (t % 40 < 5), 1, 0)
    inp['look'][:, :, 1] = np.where(s == 3, -0.015, 0.0)  # Up (player.rs:30-36: step 0.015 per tick)
    inp['look'][:, :, 0] = np.where(s == 5, rng.normal(scale=0.02, size=(ticks, n)), 0.0).astype(np.float32)
    inp['movement'][:, :, 1] = np.where(s == 4, 0.0, inp['movement'][:, :, 1])
    return inp


def players(built, n, seed):
    """start pose and floor centroids; every 7th player flies, every 5th does not clip"""
    rng = np.random.default_rng(seed)
    pos, yaw = built.start()
    cent = built.floor_centroids()
    p = np.concatenate([pos[None], cent[rng.integers(0, len(cent), n - 1)] + np.array([0, 0.3, 0], np.float32)])
    yaws = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    yaws[0] = yaw
    flags = np.full(n, rd.PLAYER_CLIP, np.uint32)
    flags[np.arange(n) % 7 == 3] |= rd.PLAYER_FLY
    flags[np.arange(n) % 5 == 4] &= ~np.uint32(rd.PLAYER_CLIP)
    return rd.player_states(p, yaws, flags=flags)


def shared(built, index):
    """(states, inputs) of the shared 256 x 120 run on level `index`"""
    return players(built, N_PLAYERS, seed=100 + index), script(N_PLAYERS, N_TICKS, seed=100 + index)


def u32(a):
    """(n, k) uint32 view: one row per record"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def differing(a, b):
    """the share of records of a that differ from b's in any bit"""
    return float((u32(a) != u32(b)).any(1).mean())


# ---- the model's cases: room A of the analytic level (cells 2..6 x 2..6 of tools/mkwad.py: kat_level) -----------------------------
ROOM_LO, ROOM_HI = -3.84, -1.28  # room A in world units, in x and in z: 2.56 square, floor 0, ceiling 1.28
ROOM_FLOOR, ROOM_CEILING = 0.0, 1.28
ROOM_CENTRE = (ROOM_LO + ROOM_HI) / 2
WALL_MARGIN = 0.3  # the model holds while every wall is further than radius + this
MODEL_TICKS = 60
MODEL_LEVEL = 1


def rest_height(c):
    """where a standing player rests above the floor: the feet sphere (radius 0.2, player.rs:253-256) probes `height` down and the
    spring carries gravity's 17 (player.rs:302-309)"""
    return 0.2 + c['height'] - 17.0 / c['spring_const_p']


def steady_speed(c):
    """the speed at which move_force balances friction and the two drags (player.rs:276-292), walking or flying"""
    return np.sqrt((c['move_force'] - c['friction']) / (c['ground_drag'] + c['air_drag']))


def model_cases(values):
    """(names, states PLAYER_STATE, inputs (MODEL_TICKS, n) PLAYER_INPUT) for the config `values`: from room A's centre at rest
    height and 0.3 above it -- walking in 8 directions, standing, jumping every 40 ticks, flying forward and up, running with
    clipping off; dropped onto the floor; and, for the closed forms, a walker and a flyer that cross the room's diagonal from a
    corner of the box."""
    c = dict(zip(FIELDS, values))
    rest = rest_height(c)
    names, pos, yaw, flags, kinds = [], [], [], [], []

    def add(name, p, y, f, kind):
        names.append(name), pos.append(p), yaw.append(y), flags.append(f), kinds.append(kind)

    for lift, tag in ((0.0, 'rest'), (0.3, 'high')):
        at = (ROOM_CENTRE, ROOM_FLOOR + rest + lift, ROOM_CENTRE)
        for k in range(8):
            add('walk%d_%s' % (k, tag), at, 2 * np.pi * k / 8 + 0.1, rd.PLAYER_CLIP, 'walk')
        add('stand_%s' % tag, at, 0.3, rd.PLAYER_CLIP, 'stand')
        add('jump_%s' % tag, at, 0.3, rd.PLAYER_CLIP, 'jump')
        add('fly_%s' % tag, at, 1.1, rd.PLAYER_CLIP | rd.PLAYER_FLY, 'walk')
        add('flyup_%s' % tag, at, 2.3, rd.PLAYER_CLIP | rd.PLAYER_FLY, 'flyup')
        add('noclip_%s' % tag, at, 4.0, 0, 'walk')
    # dropped at 4 units a second from the rest height: a head sphere wider than the feet's 0.2 meets the floor in clip() -- the
    # one way `radius` shows over a floor alone (a narrower one is cut short where the feet sphere reaches the plane)
    add('drop', (ROOM_CENTRE, ROOM_FLOOR + rest, ROOM_CENTRE), 0.7, rd.PLAYER_CLIP, 'stand')
    # the same with clipping off: the head sphere lands through noclip()'s 2000-unit probe (player.rs:173-187).  The probe's
    # height is a binary32 sum about 1000 (an ulp of 6e-5), so the cases with clipping off have a recorded error of their own
    add('noclip_drop', (ROOM_CENTRE, ROOM_FLOOR + rest, ROOM_CENTRE), 0.7, 0, 'stand')
    # the diagonal: from the box's corner towards the opposite one (forward is (-sin yaw, -cos yaw) in (x, z), player.rs:215-227)
    half = (ROOM_HI - ROOM_LO) / 2 - c['radius'] - WALL_MARGIN - 0.02
    corner = (ROOM_CENTRE + half, ROOM_FLOOR + rest, ROOM_CENTRE + half)
    add('diagonal_walk', corner, np.pi / 4, rd.PLAYER_CLIP, 'walk')
    add('diagonal_fly', corner, np.pi / 4, rd.PLAYER_CLIP | rd.PLAYER_FLY, 'walk')
    n = len(names)
    st = rd.player_states(np.array(pos, F), np.array(yaw, F), flags=np.array(flags, np.uint32))
    st['vel'][[names.index('drop'), names.index('noclip_drop')], 1] = -4.0
    # a player at the rest height is at rest: Player::reset's last_height_diff of 0 (player.rs:132) would kick it upwards by
    # spring_const_d * (17 / spring_const_p) / dt in its first tick (player.rs:303-305)
    at_rest = np.array([not k.endswith('_high') for k in names])
    st['last_height_diff'][at_rest] = 17.0 / c['spring_const_p']
    inp = np.zeros((MODEL_TICKS, n), rd.PLAYER_INPUT)
    t = np.arange(MODEL_TICKS)[:, None]
    kinds = np.array(kinds)
    inp['movement'][:, :, 1] = np.where((kinds == 'walk') | (kinds == 'flyup'), -1.0, 0.0)
    inp['movement'][:, :, 0] = np.where(kinds == 'jump', 0.25, 0.0)
    inp['jump'] = np.where((kinds == 'jump') & (t % 40 < 5) | (kinds == 'flyup') & (t < 6), 1, 0)
    inp['look'][:, :, 1] = np.where(kinds == 'flyup', -0.01, 0.0)
    return names, st, inp


MIN_MODEL_TICKS = 3  # every case runs at least this long inside the box
# A case with clipping off ends this many ticks after its first landing: noclip() takes the landing height from a binary32 sum
# about 1000 (player.rs:173-181), off by up to an ulp of 6e-5 where other roundings are 3e-8, and a player that goes on bouncing
# lands again and again (radius 0.26 at dt = 1/30: 7 landings in 52 ticks, 1e-2 apart from the model at the end).
AFTER_LANDING = 6


def spring_root(c, dt):
    """the largest root of the spring's recurrence.  With the height's excess over the rest height y_n at tick n, player.rs:302-305
    and :395 make y_{n+2} - 2 y_{n+1} + (1 + kp dt^2 + kd dt) y_n - kd dt y_{n-1} = 0 (the spring reads the height at the tick's
    start and the derivative as the last tick's difference).  Above 1 the rest height is unstable: every rounding grows by this
    factor per tick, in the reference as in the product -- at dt = 1/30 it is 1.03 for the default config and 1.17 for all_a."""
    dt = resolve_dt(dt)
    a, b = c['spring_const_p'] * dt * dt, c['spring_const_d'] * dt
    return float(np.abs(np.roots([1.0, -2.0, 1.0 + a + b, -b])).max())


def tick_cap(c, dt):
    """the ticks a case runs at most: MODEL_TICKS, or where the spring is unstable as many as let a rounding grow fourfold"""
    r = spring_root(c, dt)
    return MODEL_TICKS if r <= 1 else min(MODEL_TICKS, int(np.log(4.0) / np.log(r)))


def model_run(values, dt):
    """the model over the cases of config `values` at tick length dt (0: 1/60): (names, states, inputs, ticks, final) -- ticks
    the number of ticks each case stays inside the box by the model's own trajectory (at most tick_cap, and AFTER_LANDING past
    a first landing with clipping off), final the model's
    float64 state of each case after that many"""
    c = dict(zip(FIELDS, values))
    names, st, inp = model_cases(values)
    trace = step_model.Trace()
    step_model.step(st, inp, c, resolve_dt(dt), floor=ROOM_FLOOR, trace=trace)
    ticks = np.minimum(trace.valid_ticks(ROOM_LO, ROOM_HI, ROOM_CEILING, c['radius'] + WALL_MARGIN), tick_cap(c, dt))
    ticks = np.minimum(ticks, trace.first_landing() + 1 + AFTER_LANDING)
    final = step_model.step(st, inp, c, resolve_dt(dt), floor=ROOM_FLOOR, n_ticks=ticks)
    return names, st, inp, ticks, final


def snapshots(step, st, inp, ticks):
    """each player's record after its own number of ticks: step(states, inputs) -> states is run over the stretches between the
    distinct counts, every player in every stretch, and player p's record is kept from the launch that ends at ticks[p]"""
    out = np.array(st, rd.PLAYER_STATE)
    cur, done = np.array(st, rd.PLAYER_STATE), 0
    for k in sorted(set(int(t) for t in ticks)):
        if k > done:
            cur = step(cur, inp[done:k])
            done = k
        out[ticks == k] = cur[ticks == k]
    return out


QUANTITIES = ('pos', 'vel', 'last_height_diff')
CLASSES = ('clip', 'noclip')


def classes(st):
    """{class: mask of the cases}: clipping on (clip(), player.rs:142-166) and off (noclip(), :168-190) -- each has its own record"""
    on = (st['flags'] & rd.PLAYER_CLIP) != 0
    return {'clip': on, 'noclip': ~on}


def model_error(got, final, mask):
    """the worst absolute difference of pos, vel and last_height_diff between the PLAYER_STATE records `got` and the model's
    float64 state, over the cases of `mask`"""
    return {q: float(np.abs(np.asarray(got[q], np.float64) - final[q])[mask].max()) for q in QUANTITIES}


RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_model_error.json')
POS_CAP = 1e-3


def bounds():
    """{(config, dt key): {class: {quantity: allowed difference from the model}}}: `factor` (8) times the record of
    tests/golden/step_model_error.json for the cases with clipping on and for those with clipping off, pos capped at 1e-3"""
    import json
    with open(RECORD) as f:
        rec = json.load(f)
    out = {}
    for r in rec['records']:
        out[r['config'], r['dt']] = {}
        for cls in CLASSES:
            b = {q: rec['factor'] * r[cls][q] for q in QUANTITIES}
            b['pos'] = min(b['pos'], POS_CAP)
            out[r['config'], r['dt']][cls] = b
    return out


def within(got, final, st, b):
    """({class: error}, ok): the errors of both classes and whether each is inside its bound b[class]"""
    errs = {cls: model_error(got, final, mask) for cls, mask in classes(st).items()}
    return errs, all(errs[cls][q] <= b[cls][q] for cls in CLASSES for q in QUANTITIES)


def speed_of(kind, vel):
    """what a closed form speaks of: the horizontal speed of a walker, the whole speed of a flyer"""
    vel = np.asarray(vel, np.float64)
    return float(np.hypot(vel[0], vel[2])) if kind == 'diagonal_walk' else float(np.sqrt((vel * vel).sum()))


def closed_forms(values, dt, names, st, inp, ticks, final):
    """[(label, case index, the closed form's value, the model's value at the case's end, gap)]: the rest height of the two
    standing cases and the steady speed of the two diagonal cases, each where the model run ten times longer settles at all
    (it must where spring_root <= 1, but for the drop of 0.3).  gap is how far the model's case is from the model run ten
    times longer over the same inputs -- the case's distance from its steady state, by the model alone.  The long run must be
    the closed form itself (asserted here to 1e-6, relative)."""
    c = dict(zip(FIELDS, values))
    trace = step_model.Trace()
    long_run = step_model.step(st, np.tile(inp[-1:], (10 * MODEL_TICKS, 1)), c, resolve_dt(dt), floor=ROOM_FLOOR, trace=trace)
    out = []
    for case in ('stand_rest', 'stand_high', 'diagonal_walk', 'diagonal_fly'):
        i = names.index(case)
        if case.startswith('stand'):
            closed, at_end, steady = rest_height(c), final['pos'][i, 1] - ROOM_FLOOR, long_run['pos'][i, 1] - ROOM_FLOOR
        else:
            closed, at_end, steady = steady_speed(c), speed_of(case, final['vel'][i]), speed_of(case, long_run['vel'][i])
        settled = abs(steady - closed) <= 1e-6 * closed and not np.array(trace.overlap)[:, i].any()
        if not settled:  # no steady state to speak of: allowed of the drop of 0.3 (a long tick carries the feet sphere into the
            assert case == 'stand_high' or spring_root(c, dt) > 1, (case, steady, closed)  # floor) and of an unstable spring
            continue
        out.append((case, i, float(closed), float(at_end), abs(float(at_end) - float(steady))))
    return out


# ---- doors, lifts and exits: the players, scripts and set-ups of tests/test_gpu_game.py (moved here; that file imports them back) ---
GAME_TICKS = 200


def front(trig, dist):
    """a point `dist` in front of each trigger line's midpoint (the side its right sidedef faces; behind it for dist < 0) and the
    yaw that looks at the line"""
    mid = trig['origin'] + trig['displace'] * (trig['length'][:, None] * F(0.5))
    normal = np.stack([-trig['displace'][:, 1], trig['displace'][:, 0]], 1)  # the right side in world coordinates
    p = mid + normal * F(dist)
    face = -normal * F(np.sign(dist))  # towards the line; forward = (-sin yaw, -cos yaw) in (x, z)
    return p, np.arctan2(-face[:, 0], -face[:, 1]).astype(F)


def floor_y(ref, xz, top=10.0):
    """the floor under each (x, z): a sweep down from just below the sector's ceiling is not known, so from several heights"""
    n = len(xz)
    best = np.full(n, np.nan, F)
    for y0 in (-2.0, -1.0, 0.0, 1.0, 2.0, 3.0):
        sph = np.zeros((n, 4), F)
        sph[:, 0], sph[:, 1], sph[:, 2], sph[:, 3] = xz[:, 0], y0, xz[:, 1], 0.2
        vel = np.zeros((n, 3), F)
        vel[:, 1] = -3.0
        hit = ref.sweep(sph, vel)
        y = F(y0) - F(3.0) * hit[:, 0]
        ok = np.isfinite(hit[:, 0]) & (hit[:, 2] > 0.5) & np.isnan(best)
        best[ok] = y[ok]
    return best


def seed_players(ref, trig, n, seed, dist=0.45):
    """n players on the floor in front of random trigger lines, facing them"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(trig), n)
    p, yaw = front(trig[pick], dist)
    y = floor_y(ref, p)
    ok = np.isfinite(y)
    pos = np.stack([p[:, 0], np.where(ok, y + F(0.25), F(0)), p[:, 1]], 1).astype(F)
    st = rd.player_states(pos, yaw + rng.normal(scale=0.1, size=n).astype(F))
    return st[ok], pick[ok]


def game_script(n, ticks, seed, push=0.05, shoot=0.02):
    """(inputs, actions) of random walking, looking and jumping, with a push on `push` and a shot on `shoot` of the player-ticks"""
    rng = np.random.default_rng(seed)
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    fwd = rng.random((ticks, n)) < 0.6
    inp['movement'][..., 1] = np.where(fwd, -1.0, rng.uniform(-1, 1, (ticks, n))).astype(F)
    inp['movement'][..., 0] = np.where(fwd, 0.0, rng.uniform(-1, 1, (ticks, n))).astype(F)
    inp['look'][..., 0] = rng.normal(scale=0.01, size=(ticks, n)).astype(F)
    inp['look'][..., 1] = rng.normal(scale=0.005, size=(ticks, n)).astype(F)
    inp['jump'] = rng.random((ticks, n)) < 0.01
    r = rng.random((ticks, n))
    act = np.where(r < push, rd.ACTION_PUSH, np.where(r < push + shoot, rd.ACTION_SHOOT, rd.ACTION_NONE)).astype(np.uint8)
    return inp, act


def game_setup(directory, n, seed):
    """(wad, RefWorld, triggers, effects, n_objects, states, inputs, actions) of n players in front of the patched E1M1's trigger
    lines, with test_gpu_game's script of pushes -- the test-side trigger list, no device"""
    from test_game_host import patched_variant  # (a host module: the patched level is its own)
    wad_path, meta_path = patched_variant(directory)
    wad = rd.Wad(wad_path, meta_path)
    ref = world_ref.RefWorld(wad, 0)
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
    st, _ = seed_players(ref, trig, n, seed)
    inp, act = game_script(len(st), GAME_TICKS, seed + 1, push=0.1)
    return wad, ref, trig, effs, n_obj, st, inp, act


SET = [0, 1, 2]  # the three-level set of tests/test_gpu_worldset.py


def set_players(exits, n, seed, slots=SET, device=True):
    """n players: a third walking at an exit from 0.45 in front of it, the rest at their level's start; random slots of `slots`.
    The players of tests/test_gpu_worldset.py (moved here; that file imports them back); device=False builds the set on the host"""
    wad_path, meta_path, lines = exits
    rng = np.random.default_rng(seed)
    lv = rng.choice(np.arange(len(slots)), n)
    ws = rd.Wad(wad_path, meta_path).build_world_set(slots, device=device)
    st = ws.start_states(lv)
    at_exit = rng.random(n) < 0.35
    for p in np.nonzero(at_exit)[0]:
        _, xz, yaw, y = lines[slots[lv[p]]]
        st[p]['pos'] = (xz[0], y + F(0.25), xz[1])
        st[p]['yaw'] = yaw + F(rng.normal(scale=0.05))
    inp, act = game_script(n, 600, seed + 1)
    walk = at_exit[None, :] & (np.arange(600) < 40)[:, None]  # the exit walkers go forward for 40 ticks first
    inp['movement'][..., 0] = np.where(walk, 0.0, inp['movement'][..., 0])
    inp['movement'][..., 1] = np.where(walk, -1.0, inp['movement'][..., 1])
    inp['look'] = np.where(walk[..., None], 0.0, inp['look'])
    return ws, st, lv, inp, act


def door_setup(directory, key):
    """Players 0.45 in front of the patched E1M1's manual doors (a Push line with one rising effect), four a door, facing it;
    each pushes once, on tick 3, and stands.  The run ends when the lowest door is half open.  By the restatement alone, a tick
    at a time: `fired` the tick at whose end each player's door first has an active effect (-1: never), `moving` the players
    whose door is still rising at the end, `final` the states.  The test-side trigger list, no device."""
    dt, cfg = DTS[key], config(CONFIGS['all_a'])
    from test_game_host import patched_variant  # (a host module: the patched level is its own)
    wad_path, meta_path = patched_variant(directory)
    wad = rd.Wad(wad_path, meta_path)
    ref = world_ref.RefWorld(wad, 0)
    trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, 0)
    doors = [i for i in np.nonzero(trig['trigger_type'] == rd.TRIGGER_PUSH)[0]
             if trig['effect_end'][i] - trig['effect_start'][i] == 1 and effs[trig['effect_start'][i]]['first_height_offset'] > 0.5]
    pick = np.repeat(doors, 4)
    p, yaw = front(trig[pick], 0.45)
    y = floor_y(ref, p)
    ok = np.isfinite(y)
    pick, p, yaw, y = pick[ok], p[ok], yaw[ok], y[ok]
    n = len(pick)
    rng = np.random.default_rng(5)
    st = rd.player_states(np.stack([p[:, 0], y + np.float32(0.25), p[:, 1]], 1).astype(np.float32),
                          yaw + rng.normal(scale=0.05, size=n).astype(np.float32))
    eff = effs[trig['effect_start'][pick]]
    speed, first, obj = eff['speed'].astype(np.float64), eff['first_height_offset'].astype(np.float64), eff['object_id']
    push_tick = 3
    n_ticks = push_tick + 1 + int(0.5 * (first / speed).min() / dt)
    inp = np.zeros((n_ticks, n), rd.PLAYER_INPUT)
    act = np.zeros((n_ticks, n), np.uint8)
    act[push_tick] = rd.ACTION_PUSH
    rg = game_ref.RefGame(ref, trig, effs, n, n_obj)
    fired = np.full(n, -1)
    s = st
    for k in range(n_ticks):
        s = rg.step(s, inp[k:k + 1], act[k:k + 1], config=cfg, dt=dt, threads=1)
        now = (rg.aflags[np.arange(n), obj] & 1) != 0
        fired[now & (fired < 0)] = k
    moving = (fired >= 0) & ((rg.aflags[np.arange(n), obj] & 1) != 0) & (speed * (n_ticks - fired - 1) * dt < first)
    return dict(wad=wad, trig=trig, effs=effs, pick=pick, obj=obj, states=st, inputs=inp, actions=act, config=cfg, fired=fired,
                moving=moving, final=s, offsets=rg.offsets.copy(), speed=speed, first=first)


# ---- the rare family: one small constructed case per branch outcome of the step that the inputs above never take ---------------
# (the census of tests/world_restatement.c under -DRS_CENSUS says which: tests/test_step_census_host.py).  Every case is at most 65
# players and 120 ticks, is placed on E1M1 (level 0) or the analytic level (level 1) of the test IWAD, and names the outcomes it
# exists for; tests/test_gpu_step_rare.py steps each on the device.
RARE_DT = DTS['30']
# Players that run clip()'s 100 sweeps out (RDOOM_PLAYER_DIVERGED) on E1M1 at dt = 1/30: (pos, vel, yaw).  Found by the
# restatement alone: 400 000 players at floor centroids + (N(0, 0.3), 0.33, N(0, 0.3)) with a horizontal velocity of 8, 10 or 30
# units a second in a random direction, one tick of 1/30 s; 237 set the flag in their first tick and 153 more within three.  What
# they have in common: the sphere comes to rest against two edges of a stair or a corner whose contact normals are 6 to 10 degrees
# apart, each sweep ends 0.001 short of one of them after a contact time of about 0.002 -- so time_left hardly shrinks -- and the
# velocity loses only the factor cos(angle) a sweep: after 100 sweeps two thirds of the speed and half of the tick are left.
DIVERGING = [
    ((-18.5654202, 0.810000002, -26.778595), (-1.32662141, 0, -7.88923788), -2.85607004),     # speed 8
    ((-9.6081028, 0.0100000203, -12.2565155), (3.6876936, 0, -7.09936047), 0.0372912399),     # speed 8
    ((-12.2681561, 0.170000017, -8.18871498), (-6.15717983, 0, -7.87966633), 0.364877284),    # speed 10
    ((-21.9377422, 0.810000002, -4.54011774), (-7.68394756, 0, 6.39976168), -1.62300634),     # speed 10
    ((-10.9672194, 0.649999976, -18.4684296), (-26.8451271, 0, -13.3917561), -1.35087621),    # speed 30
    ((-18.3714523, 0.810000002, -26.0473499), (27.3320084, 0, -12.367754), -1.19544041),      # speed 30
]
# ... and players that set it in their second or third tick, not their first
DIVERGING_LATE = [
    ((-7.62000036, 0.810000002, -6.49035549), (7.99831438, 0, 0.164220482), -0.435841709),    # speed 8
    ((-10.9794731, 0.649999976, -18.2424927), (-5.77771616, 0, -8.1619854), -0.0327656679),   # speed 10
    ((-5.59885693, 0.810000002, -12.0516033), (-28.0457478, 0, 10.6506329), -1.94203734),     # speed 30
]


class Rare:
    """a case of the rare family: `states` stepped over `inputs` (ticks, n) on level `level` of the test IWAD with the config
    `config` (a name of CONFIGS) at tick length `dt`; `outcomes` the census names it exists for"""

    def __init__(self, name, outcomes, level, states, inputs, config='default', dt=RARE_DT):
        self.name, self.outcomes, self.level, self.states, self.inputs = name, tuple(outcomes), level, states, inputs
        self.config_name, self.dt = config, dt
        assert len(states) <= 65 and len(inputs) <= 120 and inputs.shape[1] == len(states), name

    @property
    def config(self):
        return config(CONFIGS[self.config_name])


def _placed(rows, flags=None):
    """PLAYER_STATE records of (pos, vel, yaw) rows"""
    st = rd.player_states(np.array([r[0] for r in rows], F), np.array([r[2] for r in rows], F),
                          flags=rd.PLAYER_CLIP if flags is None else np.asarray(flags, np.uint32))
    st['vel'] = np.array([r[1] for r in rows], F)
    return st


def diverging_states():
    """the players of DIVERGING on E1M1: each sets RDOOM_PLAYER_DIVERGED in its first tick of 1/30 s"""
    return _placed(DIVERGING)


def rare():
    """[Rare]: the family, in a fixed order"""
    out = []
    # clip()'s loop runs its 100 sweeps: in the first tick, and in a later one; then ordinary ticks with the flag set
    st = _placed(DIVERGING + DIVERGING_LATE)
    # (their sweeps end on the vertices and edges of triangles whose planes the sphere overlaps: those winners, inside a tick)
    out.append(Rare('diverged', ['clip_diverged', 'clip_diverged_already', 'sweep_vertex_wins', 'sweep_edge_wins', 'tri_overlap'], 0,
                    st, np.zeros((6, len(st)), rd.PLAYER_INPUT)))
    # looking down until the pitch stops at -(pi/2 - 1e-2) (looking up: the scripts above), walking, flying and with clipping off
    centre = (ROOM_CENTRE, ROOM_FLOOR + 0.325, ROOM_CENTRE)
    st = _placed([(centre, (0, 0, 0), 0.3 * k) for k in range(6)],
                 flags=[rd.PLAYER_CLIP, rd.PLAYER_CLIP | rd.PLAYER_FLY, 0, rd.PLAYER_CLIP, rd.PLAYER_CLIP | rd.PLAYER_FLY, 0])
    inp = np.zeros((40, 6), rd.PLAYER_INPUT)
    inp['look'][:, :3, 1], inp['look'][:, 3:, 1] = 0.09, -0.09  # 18 ticks to the limit, then held against it
    inp['movement'][:, :, 1] = -1.0
    out.append(Rare('pitch_low', ['pitch_clamped_low', 'pitch_clamped_high'], MODEL_LEVEL, st, inp))
    # a config without air drag: a player in the air (walking or with clipping off) has no slowdown at all while it moves
    st = _placed([((ROOM_CENTRE, ROOM_FLOOR + 0.85, ROOM_CENTRE), (1.0, 0.0, 0.5), 0.4 * k) for k in range(4)],
                 flags=[rd.PLAYER_CLIP, 0, rd.PLAYER_CLIP, 0])
    inp = np.zeros((30, 4), rd.PLAYER_INPUT)
    inp['movement'][:, 2:, 1] = -1.0
    out.append(Rare('no_drag', ['drag_norm_zero'], MODEL_LEVEL, st, inp, config='all_b'))
    return out
