"""The `volley` family: the branch outcomes of the game tick (world.hip GameLevel::tick, advance, start_effects, SetGame) that
the other game tests' inputs never take -- several triggers fired by one shot, removals that reorder a player's list, effects
restarted, a whole cycle inside one tick, an exit fired in a volley and during a level change.  The census of
tests/game_restatement.c under -DRS_CENSUS says which (tests/test_game_census_host.py); tests/test_gpu_game_rare.py steps each case
on the device.  Built like test_game_host.patched_variant: game_ref.patch_linedefs on the synthetic IWAD and metadata appended to a
copy of synth.toml.  Nothing here needs torch or a device.

The place: E1M1's corridor at x = -12.48, which 17 trigger lines cross at right angles.  A shot is 100 units long and ignores
walls, so a player in the corridor who shoots along it fires every Gun line ahead.  From z = -15, in the one gap:

  looking south (yaw 0)   37 91 92 108 93 94 109 95 96        words 1, 2 and 3 of `live`, every line plain
  looking north (yaw pi)  61 106 88 87 85 105 104 41          words 1, 2 and 3, three only_once lines and the exit

The positions come from the float64 table of where the axis crosses each line (z = -24.32 ... -1.28): each player stands at
least 0.3 from the nearest line, so that no rounding decides which lines lie ahead; tests/test_game_census_host.py checks by the
census that each case takes what it is named for."""
import os
import shutil

import numpy as np

import game_ref
import rust_doom_amd as rd
import worldset_ref
from util import META_PATH, ensure_wad

F = np.float32
# the specials the volley adds (none of them is in synth.toml or in the other variants' metadata)
DOOR, DOOR_B, LIFT, LIFT_B, ONCE, EXIT, BOTH, CYCLE, NO_SPEED = 201, 202, 203, 204, 205, 206, 207, 208, 209
_DOOR = 'ceiling = { first = { to = "LowestCeiling", off = -4 }, second = { to = "Floor" } }'
_LIFT = 'floor = { first = { to = "LowestFloor" }, second = { to = "Floor" } }'
VOLLEY_META = '''
[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 0.5, speed = 64, %s }

[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 0.5, speed = 32, %s }

[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 3.0, speed = 8, %s }

[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 3.0, speed = 16, %s }

[[linedef]]
special_type = %d
trigger = "Gun"
only_once = true
move = { speed = 4, floor = { first = { to = "NextFloor" } } }

[[linedef]]
special_type = %d
trigger = "Gun"
exit = "Normal"

[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 1.0, speed = 16, %s, %s }

[[linedef]]
special_type = %d
trigger = "Push"
move = { wait = 0.0, speed = 4096, %s }

[[linedef]]
special_type = %d
trigger = "Gun"
move = { wait = 1.0, ceiling = { first = { to = "LowestCeiling", off = -4 } } }
''' % (DOOR, _DOOR, DOOR_B, _DOOR, LIFT, _LIFT, LIFT_B, _LIFT, ONCE, EXIT, BOTH, _LIFT, _DOOR, CYCLE, _DOOR, NO_SPEED)

# {trigger index of E1M1: special}; the linedefs keep their tags, so each effect stays on the sector its line moved before
SOUTH = {37: BOTH, 91: DOOR, 92: BOTH, 108: LIFT, 93: LIFT_B, 94: LIFT, 109: LIFT_B, 95: DOOR_B, 96: DOOR}
NORTH = {61: LIFT, 106: LIFT_B, 88: EXIT, 87: DOOR_B, 85: NO_SPEED, 105: ONCE, 104: ONCE, 41: ONCE}
CYCLE_DOOR = 45  # a manual door away from the corridor (its ceiling's object id is above 32): one push runs its whole cycle
SHORT_LAST = 106  # the short variants' last trigger: the specials of every later linedef are cleared
VARIANTS = ('full', 'short_plain', 'short_once')
X = -12.48  # the corridor's axis
GAP_Z = -15.0


def _patches(level, name):
    specials = [i for i, ld in enumerate(level.linedefs) if ld[3] != 0]
    assign = dict(SOUTH)
    assign.update(NORTH)
    assign[CYCLE_DOOR] = CYCLE
    if name == 'short_once':
        assign[SHORT_LAST] = ONCE
    patches = {specials[t]: (s, level.linedefs[specials[t]][4]) for t, s in assign.items()}
    if name != 'full':
        patches.update({i: (0, 0) for i in specials[SHORT_LAST + 1:]})
    return patches


def volley_variant(directory, name='full', exits=False):
    """(wad path, metadata path) of E1M1 with the volley's specials, written into `directory`.  name: 'full' (all 128 triggers; the
    list's last is far from the corridor), 'short_plain' (the list ends with trigger 106, a plain lift line of the north volley) or
    'short_once' (the same, that line only_once).  exits: on top of worldset_ref.exit_variant's walk-over exits in E1M1 to E1M3;
    then (wad path, metadata path, exit_variant's lines)"""
    from oracle import wad_oracle as wo
    assert name in VARIANTS, name
    lines = None
    if exits:
        src, src_meta, lines = worldset_ref.exit_variant(directory)
    else:
        src, src_meta = ensure_wad(), META_PATH
    with open(src, 'rb') as f:
        data = f.read()
    archive = wo.Archive(src, src_meta)
    patches = _patches(wo.Level(wo.Archive(ensure_wad(), META_PATH), 0), name)  # (by linedef: an exit line shifts no linedef)
    tag = name + ('_exits' if exits else '')
    wad = os.path.join(directory, 'volley_%s.wad' % tag)
    with open(wad, 'wb') as f:
        f.write(game_ref.patch_linedefs(data, archive.levels[0], patches))
    meta = os.path.join(directory, 'volley_%s.toml' % tag)
    shutil.copy(src_meta, meta)
    with open(meta, 'a') as f:
        f.write(VOLLEY_META)
    assert not exits or lines[0][0] not in patches, 'the exit line of E1M1 is one of the volley\'s'
    return (wad, meta, lines) if exits else (wad, meta)


class Case:
    """a case of the family: `states` stepped over `inputs` and `actions` (ticks, n) on the variant `variant` at tick length 1/60;
    `outcomes` the census names it exists for.  actions may hold bytes above ACTION_SHOOT: they go to the device as they are"""

    def __init__(self, name, outcomes, variant, states, inputs, actions):
        self.name, self.outcomes, self.variant, self.states, self.inputs = name, tuple(outcomes), variant, states, inputs
        self.actions = np.ascontiguousarray(actions, np.uint8)
        assert len(states) <= 64 and len(inputs) <= 240 and inputs.shape == self.actions.shape == (len(inputs), len(states)), name


NORTH_YAW, SOUTH_YAW = F(np.pi), F(0.0)  # forward is (-sin yaw, -cos yaw) in (x, z)
# (x, y, z, yaw): standing on the floor (its height + 0.25) in the corridor's gap, between lines 88 and 87, and between 109 and 95
GAP_NORTH, GAP_SOUTH = (X, 0.85, GAP_Z, NORTH_YAW), (X, 0.85, GAP_Z, SOUTH_YAW)
MID_NORTH = (X, 0.61, -9.3, NORTH_YAW)     # ahead: 87 85 105 104 41
DOORS_SOUTH = (X, 0.21, -22.5, SOUTH_YAW)  # ahead: 95 and 96, the two faces of one door
AT_CYCLE_DOOR = (-19.52, 0.93, -25.41, F(-np.pi))  # 0.45 in front of CYCLE_DOOR, facing it


def _players(rows):
    rows = np.array(rows, F)
    return rd.player_states(rows[:, :3], rows[:, 3])


def _script(n, ticks, shots, action=rd.ACTION_SHOOT):
    """still players; {tick: action of every player} or {tick: (players, action)}"""
    inp = np.zeros((ticks, n), rd.PLAYER_INPUT)
    act = np.zeros((ticks, n), np.uint8)
    for t, a in shots.items():
        if isinstance(a, tuple):
            act[t, a[0]] = a[1]
        else:
            act[t] = a
    return inp, act


def cases():
    """[Case]: the family on the single level, in a fixed order"""
    out = []
    shoot = rd.ACTION_SHOOT
    # one shot, nine plain triggers over three `live` words; two of them with two effects (one on objects on both sides of id 32),
    # three pairs on one object with different speeds; and the same shot again a tick later and mid-motion
    out.append(Case('plain_volley', ['fired_three_plus', 'fired_index_32', 'fired_index_64', 'fired_index_96', 'trigger_two_effects',
                                     'effect_on_started_this_tick', 'effect_on_active', 'object_id_32', 'adv_two_active', 'hit_gun'],
                    'full', _players([GAP_SOUTH]), *_script(1, 40, {0: shoot, 1: shoot, 20: shoot})))
    # one shot, eight triggers, three of them only_once, with the exit, a door, a lift pair on one object and a speed-0 effect; the
    # same shot again: the dead lines are hit and ignored, the list is the shortened one, the effects restart.  Three arrangements:
    once = ['fired_three_plus', 'fired_many_with_once', 'removed_two_plus', 'exit_with_others', 'dead_trigger_hit', 'trigger_no_effect',
            'adv_speed_zero', 'effect_on_active']
    for variant, extra in (('full', []), ('short_plain', ['swapped_in_fired']), ('short_once', ['removed_last'])):
        out.append(Case('once_volley_' + variant, once + extra, variant, _players([GAP_NORTH, MID_NORTH]),
                        *_script(2, 12, {0: shoot, 1: shoot, 6: shoot})))
    # a door shot through both its faces (two triggers, one object, the later line's speed), and shot again while it rises, while
    # it waits at the top and while it closes
    out.append(Case('restarts', ['fired_two', 'effect_on_active', 'effect_on_started_this_tick', 'adv_at_first', 'adv_second_started'],
                    'full', _players([DOORS_SOUTH]), *_script(1, 140, {0: shoot, 5: shoot, 30: shoot, 66: shoot})))
    # one push, and the door opens and shuts within the next tick; pushed again at once and later; and the action bytes that are
    # none of the three: nothing fires
    out.append(Case('cycle', ['adv_second_arrives_same_tick', 'adv_done_with_second', 'adv_wait_zero', 'object_id_32', 'action_clamped',
                              'hit_push', 'fired_one_plain'],
                    'full', _players([AT_CYCLE_DOOR] * 3),
                    *_script(3, 12, {0: ([0], rd.ACTION_PUSH), 1: ([0], rd.ACTION_PUSH), 2: ([1], 3), 3: ([2], 255), 6: ([0], rd.ACTION_PUSH),
                                     7: ([1, 2], rd.ACTION_PUSH)})))
    return out


def neighbours(n, ticks):
    """(states, inputs, actions) of n players who stay on the tick's fast path: each pushes CYCLE_DOOR now and then, one plain
    trigger at a time"""
    st = _players([AT_CYCLE_DOOR] * max(n, 1))[:n]
    st['yaw'] += (np.arange(n) % 7).astype(F) * F(0.02)
    inp, act = _script(n, ticks, {})
    t, p = np.meshgrid(np.arange(ticks), np.arange(n), indexing='ij')
    act[(t + p) % 5 == 0] = rd.ACTION_PUSH
    return st, inp, act


# ---- the set: exit_variant's three levels, E1M1 with the volley's specials -----------------------------------------------------
SET = [0, 1, 2]
OUT_OF_RANGE = 7  # not a slot: the player is left untouched
SET_CASE_NAMES = ('set_volley',)


class SetCase(Case):
    """a case on the set: `levels` the players' slots at the start"""

    def __init__(self, name, outcomes, states, levels, inputs, actions):
        Case.__init__(self, name, outcomes, 'full', states, inputs, actions)
        self.levels = np.asarray(levels, np.int64)


def set_cases(exits):
    """[SetCase] on volley_variant(..., exits=True)'s result `exits`"""
    lines = exits[2]
    shoot = rd.ACTION_SHOOT
    out = []
    # player 0: the north volley (exit, door, only_once lines) in E1M1; the change arrives two ticks later, the door moving and the
    # lines removed; then the fresh game of E1M2.  Player 1: the same, and the same shot again in the tick between -- an exit
    # fired during a change.  Player 2: beside them, in no slot.  Player 3: walks over E1M3's exit, which leads nowhere in this
    # set, and on.  Player 4: the south volley, no exit: stays.
    _, xz, yaw, y = lines[2]
    st = _players([GAP_NORTH, GAP_NORTH, GAP_NORTH, (xz[0], y + F(0.25), xz[1], yaw), GAP_SOUTH])
    inp, act = _script(5, 40, {0: ([0, 1, 2, 4], shoot), 1: ([1, 2], shoot), 8: ([0, 1, 4], shoot)})
    inp['movement'][:30, 3, 1] = -1.0
    out.append(SetCase('set_volley', ['change_started', 'exit_during_change', 'change_with_effect_active', 'change_with_trigger_removed',
                                      'change_with_nonzero_offset', 'exit_no_destination'],
                       st, [0, 0, OUT_OF_RANGE, 2, 0], inp, act))
    return out
