"""The test side of world sets: one game_ref.RefGame per level, stepped one tick at a time over the players then in that level,
with the level change applied here (game/src/level.rs:194-199, wad_system.rs:118-156, player.rs:118-133, 359-362): an exit fired
in the poll of tick t; tick t + 1 runs in the old level; tick t + 2 starts with the player reset at the destination's start and a
fresh game there.  And the exit variant of the synthetic IWAD: a walk-over exit line near the start of E1M1, E1M2 and E1M3."""
import os
import shutil

import numpy as np

import game_ref
import rust_doom_amd as rd
import world_ref
from util import META_PATH, ensure_wad

F = np.float32
EXIT_SPECIAL = 52  # a walk-over exit the synthetic metadata does not define; the variant's metadata adds it
EXIT_META = '''
[[linedef]]
special_type = %d
trigger = "WalkOver"
exit = "Normal"
''' % EXIT_SPECIAL
EXIT_LEVELS = (0, 1, 2)


def _passable(ref, a, b):
    """(front point xz, yaw facing the line, floor y) of a player 0.45 in front of line a-b who walks through it unhindered, or None"""
    d = (b - a) / np.linalg.norm(b - a)
    normal = np.array([-d[1], d[0]], F)
    mid = (a + b) * F(0.5)
    for side in (1.0, -1.0):
        p = (mid + normal * F(0.45 * side)).astype(F)
        face = -normal * F(side)
        y = floor_y(ref, p[None])[0]
        if not np.isfinite(y):
            continue
        hit = ref.sweep(np.array([[p[0], y + 0.25, p[1], 0.19]], F), np.array([[face[0], 0.0, face[1]]], F) * F(1.2))
        if hit[0, 0] > 1.0:
            return p, F(np.arctan2(-face[0], -face[1])), y
    return None


def floor_y(ref, xz):
    """the floor under each (x, z) of a world_ref.RefWorld: the first upward-facing contact of a sweep down from a few heights"""
    best = np.full(len(xz), np.nan, F)
    for y0 in (-2.0, -1.0, 0.0, 1.0, 2.0, 3.0):
        sph = np.zeros((len(xz), 4), F)
        sph[:, 0], sph[:, 1], sph[:, 2], sph[:, 3] = xz[:, 0], y0, xz[:, 1], 0.2
        vel = np.zeros((len(xz), 3), F)
        vel[:, 1] = -3.0
        hit = ref.sweep(sph, vel)
        ok = np.isfinite(hit[:, 0]) & (hit[:, 2] > 0.5) & np.isnan(best)
        best[ok] = (F(y0) - F(3.0) * hit[:, 0])[ok]
    return best


def exit_variant(directory):
    """(wad path, metadata path, {level: (linedef index, front point xz, yaw towards the line, floor y)}): the synthetic IWAD with
    the passable two-sided line nearest each level's start turned into a walk-over exit (one without a special when there is one:
    E1M2's only two-sided line is its lift's)"""
    from oracle import wad_oracle as wo
    src = ensure_wad()
    with open(src, 'rb') as f:
        data = f.read()
    archive = wo.Archive(src, META_PATH)
    wad = rd.Wad(src, META_PATH)
    lines = {}
    for index in EXIT_LEVELS:
        level = wo.Level(archive, index)
        start = np.asarray(wad.build_level(index).start()[0], F)[[0, 2]]
        ref = world_ref.RefWorld(wad, index)
        cands = []
        for i, ld in enumerate(level.linedefs):
            if ld[6] < 0:
                continue
            a, b = level.vertex(ld[0]), level.vertex(ld[1])
            if a is None or b is None:
                continue
            a, b = np.asarray(a, F), np.asarray(b, F)
            cands.append((ld[3] != 0, float(np.linalg.norm((a + b) * 0.5 - start)), i, a, b))
        for _, _, i, a, b in sorted(cands, key=lambda c: c[:3]):
            found = _passable(ref, a, b)
            if found is not None:
                lines[index] = (i,) + found
                break
        assert index in lines, 'no passable two-sided line in level %d' % index
        data = game_ref.patch_linedefs(data, archive.levels[index], {lines[index][0]: (EXIT_SPECIAL, 0)})
    path = os.path.join(directory, 'exits.wad')
    with open(path, 'wb') as f:
        f.write(data)
    meta = os.path.join(directory, 'exits.toml')
    shutil.copy(META_PATH, meta)
    with open(meta, 'a') as f:
        f.write(EXIT_META)
    return path, meta, lines


# the outcomes of the level change that RefWorldSet counts as it steps (tests/test_game_census_host.py)
SET_CENSUS_NAMES = ('change_started', 'exit_no_destination', 'exit_during_change', 'change_with_effect_active',
                    'change_with_trigger_removed', 'change_with_nonzero_offset')


class RefWorldSet:
    """N players over the levels `indices` of a WAD: per level a world_ref.RefWorld and a game_ref.RefGame with a row for every
    player (only the rows of the players in that level are stepped), the players' slots, and the change stage of each.
    `set_census` counts the level change's outcomes, {name of SET_CENSUS_NAMES: times taken}: an exit that starts a change, one
    in a level without a destination, one fired while a change is under way; and a change that arrives (the old game is dropped)
    with an effect active, with a trigger removed, with an object's offset not zero"""

    def __init__(self, wad_path, meta_path, indices, levels, census=False):
        self.wad = rd.Wad(wad_path, meta_path)
        self.indices = list(indices)
        self.levels = np.array(levels, np.int64)
        n = len(self.levels)
        self.worlds, self.games, self.starts = [], [], []
        for index in self.indices:
            trig, effs, n_obj = game_ref.triggers(wad_path, meta_path, index)
            ref = world_ref.RefWorld(self.wad, index, census=census)
            self.worlds.append(ref)
            self.games.append(game_ref.RefGame(ref, trig, effs, n, n_obj, census=census))
            pos, yaw = self.wad.build_level(index).start()
            self.starts.append((np.asarray(pos, F), F(yaw)))
        self.dest = [self.indices.index(i + 1) if i + 1 in self.indices else None for i in self.indices]
        self.n_objects = max(g.n_objects for g in self.games)
        self.stage = np.zeros(n, np.int64)
        self.set_census = dict.fromkeys(SET_CENSUS_NAMES, 0)

    def _fresh(self, slot, p):
        g = self.games[slot]
        g.order[p] = np.arange(len(g.trig), dtype=np.uint32)
        g.counts[p] = len(g.trig)
        g.act[p], g.aflags[p], g.offsets[p] = 0, 0, 0

    def step(self, states, inputs, actions=None, config=None, dt=1.0 / 60.0, threads=16):
        """n_ticks ticks, one at a time: (states, inputs (n_ticks, n), actions (n_ticks, n) or None) -> the stepped states; dt 0
        means 1/60 (include/rdoom.h), as in RefWorld.step"""
        dt = float(np.float32(1.0) / np.float32(60.0)) if dt == 0 else dt
        states = np.array(states, rd.PLAYER_STATE).reshape(-1)
        n = len(states)
        inputs = np.asarray(inputs, rd.PLAYER_INPUT).reshape(-1, n)
        for t in range(len(inputs)):
            exited, requested = np.nonzero(self.stage == 1)[0], np.nonzero(self.stage == 2)[0]
            self.stage[exited] = 2  # Level::update requests the next level; this tick still runs in the old one
            for p in requested:     # WadSystem::update loads it, Level is rebuilt, Player::update resets
                self.stage[p] = 0
                d = self.dest[self.levels[p]]
                old = self.games[self.levels[p]]
                self.set_census['change_with_effect_active'] += int((old.aflags[p] & 1).any())
                self.set_census['change_with_trigger_removed'] += int(old.counts[p] < len(old.trig))
                self.set_census['change_with_nonzero_offset'] += int((old.offsets[p] != 0).any())
                self.levels[p] = d
                self._fresh(d, p)
                pos, yaw = self.starts[d]
                s = states[p]
                s['pos'], s['vel'], s['yaw'], s['pitch'], s['last_height_diff'] = pos, 0.0, yaw, F(1e-8), 0.0
            for slot, g in enumerate(self.games):
                sel = np.nonzero(self.levels == slot)[0]
                if not len(sel):
                    continue
                sub = game_ref.RefGame.__new__(game_ref.RefGame)
                sub.w, sub.trig, sub.effs, sub.n, sub.n_objects = g.w, g.trig, g.effs, len(sel), g.n_objects
                sub.L = g.L
                sub.order, sub.counts, sub.act = g.order[sel].copy(), g.counts[sel].copy(), g.act[sel].copy()
                sub.aflags, sub.offsets = g.aflags[sel].copy(), g.offsets[sel].copy()
                before = states[sel].copy()
                before['flags'] &= ~np.uint32(rd.PLAYER_EXITED)
                act = None if actions is None else np.asarray(actions, np.uint8).reshape(-1, n)[t:t + 1, sel]
                after = sub.step(before, inputs[t:t + 1, sel], act, config=config, dt=dt, threads=threads)
                fired = (after['flags'] & rd.PLAYER_EXITED) != 0
                after['flags'] |= states[sel]['flags']
                states[sel] = after
                g.order[sel], g.counts[sel], g.act[sel], g.aflags[sel], g.offsets[sel] = sub.order, sub.counts, sub.act, sub.aflags, sub.offsets
                if self.dest[slot] is not None:
                    start = sel[fired & (self.stage[sel] == 0)]
                    self.stage[start] = 1
                    self.set_census['change_started'] += len(start)
                    self.set_census['exit_during_change'] += int((fired & (self.stage[sel] != 0)).sum()) - len(start)
                else:
                    self.set_census['exit_no_destination'] += int(fired.sum())
        return states

    def offsets(self):
        """the players' object offsets as the set lays them out: (n, n_objects, 3), each row its level's, zero beyond"""
        out = np.zeros((len(self.levels), self.n_objects, 3), F)
        for slot, g in enumerate(self.games):
            sel = self.levels == slot
            out[sel, :g.n_objects] = g.offsets[sel]
        return out
