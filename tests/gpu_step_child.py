"""Child process of tests/test_gpu_step_configs.py: one case per process, so that each GPU step runs under the parent's time limit
and a fault ends that case alone.  Prints what it measured and 'RESULT ok', and exits 0, when every assertion of the case held.

  step LEVEL            World.step against world_ref.RefWorld.step, bit for bit, on the shared run of tests/step_cases.py: every
                        config x {1/60, 1/35}, the two all-field configs x every tick length; config=None is the default and
                        dt = 0 is 1/60; once with per-player object offsets; once as 120 launches of one tick on device tensors
  game CONFIG DT        World.step_game against game_ref.RefGame on the patched E1M1: states, game words, offsets
  worldset CONFIG DT    WorldSet.step_game against worldset_ref.RefWorldSet on the exit variant: states, game words, offsets, levels
  edges                 n_ticks = 0, dt = 0 and -0.0, and dt = inf / nan / negative as RDOOM_BAD_ARG that queues nothing, on the
                        three entry points
  model FIRST LAST      World.step against the float64 model (tests/step_model.py) within 8 x tests/golden/step_model_error.json
                        (the record of the case's class: clipping on or off), and the closed forms, for configs [FIRST, LAST) of step_cases.CONFIGS at every tick length
  doors DT              a pushed door rises at its effect's speed at tick length DT"""
import sys
import tempfile

import numpy as np

import conftest  # noqa: F401  (sys.path)
import game_ref
import rust_doom_amd as rd
import step_cases as sc
import world_ref
import worldset_ref
from test_game_host import patched_variant
from util import META_PATH, ensure_wad

import torch

F = np.float32
u32 = sc.u32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(got, want, what):
    bad = np.nonzero((u32(got) != u32(want)).any(1))[0]
    print('%-44s %d differing records of %d' % (what, len(bad), len(got)))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[bad[:2]], want[bad[:2]])


# ---- step -------------------------------------------------------------------------------------------------------------------------
def case_step(index):
    wad = rd.Wad(ensure_wad(), META_PATH)
    world, ref = wad.build_world(index), world_ref.RefWorld(wad, index)
    st, inp = sc.shared(wad.build_level(index), index)
    results = {}
    pairs = [(name, dt) for name in sc.CONFIGS for dt in (sc.DT_DEFAULT, sc.DTS['35'])]
    pairs += [(name, dt) for name in sc.ALL_FIELDS for dt in (sc.DTS['120'], sc.DTS['30'], sc.DTS['0'])]
    for name, dt in pairs:
        cfg = sc.config(sc.CONFIGS[name])
        got = world.step(st, inp, config=cfg, dt=dt)
        same(got, ref.step(st, inp, config=cfg, dt=dt), 'level %d %s dt %.6f' % (index, name, dt))
        results[name, dt] = got
    moved = np.linalg.norm(results['default', sc.DT_DEFAULT]['pos'] - st['pos'], axis=1)
    assert (moved > 0.5).mean() > 0.3, (moved > 0.5).mean()  # (they really walked)
    # config=None is the explicit default; dt = 0 is 1/60 (the restatement's side of both: tests/test_step_configs_host.py)
    same(world.step(st, inp), results['default', sc.DT_DEFAULT], 'config=None == the default config')
    for name in sc.ALL_FIELDS:
        same(results[name, 0.0], results[name, sc.DT_DEFAULT], '%s: dt 0 == dt 1/60' % name)
        assert sc.differing(results[name, sc.DTS['35']], results[name, sc.DT_DEFAULT]) >= 0.9
    # per-player object offsets
    cfg, dt = sc.config(sc.CONFIGS['all_a']), sc.DTS['35']
    off = np.zeros((len(st), world.n_objects, 3), F)
    off[:, :, 1] = np.random.default_rng(3).uniform(0.0, 1.2, (len(st), world.n_objects)).astype(F)
    with_off = world.step(st, inp, config=cfg, dt=dt, object_offsets=off)
    same(with_off, ref.step(st, inp, config=cfg, dt=dt, offsets=off), 'all_a dt 1/35 with object offsets')
    if world.n_objects > 1:
        assert sc.differing(with_off, results['all_a', dt]) > 0  # (the offsets changed some answers)
    # 120 launches of one tick == one launch of 120, on device tensors
    s_dev, i_dev = dev(st), dev(inp)
    step = len(st) * rd.PLAYER_INPUT.itemsize
    for t in range(len(inp)):
        world.step(s_dev, i_dev[t * step:(t + 1) * step], n_ticks=1, config=cfg, dt=dt)
    torch.cuda.synchronize()
    same(s_dev.cpu().numpy().view(rd.PLAYER_STATE), results['all_a', dt], '120 launches of one tick == one of 120')


# ---- game and world set -----------------------------------------------------------------------------------------------------------
def ref_game_words(rg, n_trig, n_obj, words):
    """rg's games in the layout of include/rdoom.h (rdoom_world_game_bytes), `words` 32-bit words a player: [0] the list's
    length, live[LW], fired[LW] (zero), active[OW], second[OW], order[T], padding to 16 bytes, effect[O] x 4 floats"""
    lw, ow = (n_trig + 31) // 32, (n_obj + 31) // 32
    out = np.zeros((rg.n, words), np.uint32)
    out[:, 0] = rg.counts
    for p in range(rg.n):
        for t in rg.order[p, :rg.counts[p]]:
            out[p, 4 + (t >> 5)] |= np.uint32(1 << (t & 31))
        for o in np.nonzero(rg.aflags[p] & 1)[0]:
            out[p, 4 + 2 * lw + (o >> 5)] |= np.uint32(1 << (o & 31))
        for o in np.nonzero((rg.aflags[p] & 3) == 3)[0]:
            out[p, 4 + 2 * lw + ow + (o >> 5)] |= np.uint32(1 << (o & 31))
    order = 4 + 2 * lw + 2 * ow
    effect = (order + n_trig + 3) // 4 * 4
    return out, order, effect


def same_games(game, rg, n_trig, n_obj, what):
    """the device games against rg's: the length, the live, fired, active and second bits, the list up to its length and the
    effect record of every active object (what lies beyond the list's length, and an ended effect's record, is nobody's promise)"""
    got = game.cpu().numpy().view(np.uint32).reshape(rg.n, -1)
    want, order, effect = ref_game_words(rg, n_trig, n_obj, got.shape[1])
    assert effect + 4 * n_obj <= got.shape[1]
    bad = (got[:, :order] != want[:, :order]).any(1)
    for p in range(rg.n):
        k = rg.counts[p]
        bad[p] |= (got[p, order:order + k] != rg.order[p, :k]).any()
        for o in np.nonzero(rg.aflags[p] & 1)[0]:
            bad[p] |= (got[p, effect + 4 * o:effect + 4 * o + 4] != rg.act[p, o].view(np.uint32)).any()
    print('%-44s %d differing games of %d' % (what, int(bad.sum()), rg.n))
    assert not bad.any(), (what, np.nonzero(bad)[0][:8].tolist())


def case_game(name, key):
    cfg, dt = sc.config(sc.CONFIGS[name]), sc.DTS[key]
    with tempfile.TemporaryDirectory() as tmp:
        wad, ref, trig, effs, n_obj, st, inp, act = sc.game_setup(tmp, sc.N_PLAYERS, 61)
        world = wad.build_world(0)
        t = world.triggers()
        assert t['triggers'].tobytes() == trig.tobytes() and t['effects'].tobytes() == effs.tobytes() and n_obj == world.game_objects
        n = len(st)
        game, offs = world.game_state(n)
        got = world.step_game(st, inp, game, offs, actions=act, config=cfg, dt=dt)
        rg = game_ref.RefGame(ref, trig, effs, n, n_obj)
        want = rg.step(st, inp, act, config=cfg, dt=dt)
        what = 'step_game %s dt 1/%s: ' % (name, key)
        same(got, want, what + 'states')
        same(offs.cpu().numpy().reshape(n, -1), rg.offsets.reshape(n, -1), what + 'offsets')
        same_games(game, rg, len(trig), n_obj, what + 'game words')
        moved = int((rg.offsets[:, :, 1] != 0).any(1).sum())
        print('%d of %d games end with a door or lift off its rest, %d players exited' % (moved, n, int((got['flags'] & rd.PLAYER_EXITED != 0).sum())))
        assert moved > 20 and (rg.aflags & 1).any()
        # against the default config and tick length: the config and dt reached the physics and the effects
        g0, o0 = world.game_state(n)
        base = world.step_game(st, inp, g0, o0, actions=act)
        assert sc.differing(got, base) > 0.9 and not torch.equal(o0, offs)


def case_worldset(name, key):
    from test_gpu_worldset import SET, _players
    cfg, dt = sc.config(sc.CONFIGS[name]), sc.DTS[key]
    ticks = 160
    with tempfile.TemporaryDirectory() as tmp:
        exits = worldset_ref.exit_variant(tmp)
        ws, st, lv, inp, act = _players(exits, sc.N_PLAYERS, 31)
        inp, act = inp[:ticks], act[:ticks]
        n = len(st)
        game, offs, levels = ws.game_state(lv)
        got = ws.step_game(st, inp, game, offs, levels, actions=act, config=cfg, dt=dt)
        ref = worldset_ref.RefWorldSet(exits[0], exits[1], SET, lv)
        want = ref.step(st, inp, act, config=cfg, dt=dt)
        what = 'set step_game %s dt 1/%s: ' % (name, key)
        same(got, want, what + 'states')
        assert levels.cpu().numpy().tolist() == ref.levels.tolist()
        same(offs.cpu().numpy().reshape(n, -1), ref.offsets().reshape(n, -1), what + 'offsets')
        words = game.cpu().numpy().view(np.uint32).reshape(n, -1)
        for slot, g in enumerate(ref.games):  # each player's game in its current level's layout, zero words after it
            sel = np.nonzero(ref.levels == slot)[0]
            if not len(sel):
                continue
            sub = game_ref.RefGame(g.w, g.trig, g.effs, len(sel), g.n_objects)
            sub.order, sub.counts, sub.act, sub.aflags = g.order[sel], g.counts[sel], g.act[sel], g.aflags[sel]
            mine = words[sel].copy()
            stage = mine[:, 1].copy()
            mine[:, 1] = 0  # word 1 is the set's level change (include/rdoom.h: rdoom_worldset_game_bytes)
            assert np.array_equal(stage, ref.stage[sel]), (slot, stage, ref.stage[sel])
            same_games(torch.from_numpy(mine.view(np.int32)), sub, len(g.trig), g.n_objects, what + 'game words, slot %d' % slot)
        changed = int((ref.levels != lv).sum())
        print('%d of %d players changed level' % (changed, n))
        assert changed > 10 and (got['flags'][ref.levels != lv] & rd.PLAYER_EXITED).all()
        g0, o0, l0 = ws.game_state(lv)
        base = ws.step_game(st, inp, g0, o0, l0, actions=act)
        assert sc.differing(got, base) > 0.9


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def case_edges():
    with tempfile.TemporaryDirectory() as tmp:
        wad_path, meta_path = patched_variant(tmp)
        wad = rd.Wad(wad_path, meta_path)
        world, ws = wad.build_world(0), wad.build_world_set([0])
        st, inp = sc.shared(wad.build_level(0), 0)
        n = len(st)
        cfg = sc.config(sc.CONFIGS['all_b'])
        raw = np.ascontiguousarray(st).view(np.uint8).reshape(-1)
        empty = torch.empty(0, dtype=torch.uint8, device='cuda')
        i_dev = dev(inp)

        def entry_points():
            """(name, step(states tensor, inputs tensor, n_ticks, dt), the tensors besides the states that must not change)"""
            game, offs = world.game_state(n)
            sgame, soffs, slevels = ws.game_state(np.zeros(n, np.int64))
            return [('step', lambda s, i, k, dt: world.step(s, i, n_ticks=k, config=cfg, dt=dt), []),
                    ('step_game', lambda s, i, k, dt: world.step_game(s, i, game, offs, n_ticks=k, config=cfg, dt=dt), [game, offs]),
                    ('set step_game', lambda s, i, k, dt: ws.step_game(s, i, sgame, soffs, slevels, n_ticks=k, config=cfg, dt=dt),
                     [sgame, soffs, slevels])]

        for what, step, others in entry_points():
            before = [t.clone() for t in others]
            # n_ticks = 0 leaves every byte
            s_dev = dev(st)
            step(s_dev, empty, 0, sc.DTS['35'])
            torch.cuda.synchronize()
            assert np.array_equal(s_dev.cpu().numpy(), raw), what
            # a tick length that is no finite non-negative number is RDOOM_BAD_ARG and queues nothing
            for dt in (float('inf'), float('nan'), -1.0 / 60.0, -1e-30, float('-inf')):
                try:
                    step(s_dev, i_dev, len(inp), dt)
                except rd.RdoomError as e:
                    assert e.status == -1, (what, dt, e.status)
                else:
                    raise AssertionError('%s took dt = %r' % (what, dt))
                torch.cuda.synchronize()
                assert np.array_equal(s_dev.cpu().numpy(), raw), (what, dt)
            assert all(torch.equal(a, b) for a, b in zip(before, others)), what
            print('%-16s n_ticks = 0 and 5 bad tick lengths leave every byte' % what)
        # dt = 0 and dt = -0.0 are 1/60, on each entry point (fresh games each time)
        outs = {}
        for dt in (sc.DT_DEFAULT, 0.0, -0.0):
            for what, step, others in entry_points():
                s_dev = dev(st)
                step(s_dev, i_dev, len(inp), dt)
                torch.cuda.synchronize()
                outs[what, str(dt)] = [s_dev.cpu().numpy()] + [t.cpu().numpy() for t in others]
        for what in ('step', 'step_game', 'set step_game'):
            for zero in ('0.0', '-0.0'):
                assert all(np.array_equal(a, b) for a, b in zip(outs[what, zero], outs[what, str(sc.DT_DEFAULT)])), (what, zero)
            assert not np.array_equal(outs[what, '0.0'][0], raw)
            print('%-16s dt 0 and -0.0 are 1/60' % what)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def case_model(first, last):
    wad = rd.Wad(ensure_wad(), META_PATH)
    world = wad.build_world(sc.MODEL_LEVEL)
    bounds = sc.bounds()
    for name in list(sc.CONFIGS)[first:last]:
        values = sc.CONFIGS[name]
        cfg = sc.config(values)
        for key, dt in sc.DTS.items():
            names, st, inp, ticks, final = sc.model_run(values, dt)
            got = sc.snapshots(lambda s, i: world.step(s, i, config=cfg, dt=dt), st, inp, ticks)
            b = bounds[name, key]
            errs, ok = sc.within(got, final, st, b)
            for cls, e in errs.items():
                print('%-22s dt %-4s %-6s pos %.2e of %.2e  vel %.2e of %.2e  last_height_diff %.2e of %.2e' % (
                    name, key, cls, e['pos'], b[cls]['pos'], e['vel'], b[cls]['vel'], e['last_height_diff'], b[cls]['last_height_diff']))
            assert ok, (name, key, errs, b)
            assert not (got['flags'] & rd.PLAYER_DIVERGED).any()
            for case, i, closed, at_end, gap in sc.closed_forms(values, dt, names, st, inp, ticks, final):
                # the product against the formula alone; the tolerance is the model's own distance from its steady state plus
                # the recorded rounding (a speed is within sqrt(3) component bounds of the model's)
                if case.startswith('stand'):
                    mine, tol = float(got['pos'][i, 1]) - sc.ROOM_FLOOR, gap + b['clip']['pos']
                else:
                    mine, tol = sc.speed_of(case, got['vel'][i]), gap + 2 * b['clip']['vel']
                print('    %-14s %.6f, the formula %.6f, tolerance %.2e (relative %.1e)' % (case, mine, closed, tol, tol / closed))
                assert abs(mine - closed) <= tol, (name, key, case, mine, closed, tol)


# ---- doors ------------------------------------------------------------------------------------------------------------------------
def case_doors(key):
    dt = sc.DTS[key]
    with tempfile.TemporaryDirectory() as tmp:
        d = sc.door_setup(tmp, key)
        world = d['wad'].build_world(0)
        t = world.triggers()
        assert t['triggers'].tobytes() == d['trig'].tobytes() and t['effects'].tobytes() == d['effs'].tobytes()
        n, obj, moving, fired = len(d['states']), d['obj'], d['moving'], d['fired']
        eff = t['effects'][t['triggers']['effect_start'][d['pick']]]  # speed and first offset from the product's own list
        speed, first = eff['speed'].astype(np.float64), eff['first_height_offset'].astype(np.float64)
        print('dt 1/%s: %d ticks, %d players; %d pushed their door open and it is still rising' % (
            key, len(d['inputs']), n, int(moving.sum())))
        assert moving.sum() >= 16, int(moving.sum())
        game, offs = world.game_state(n)
        got = world.step_game(d['states'], d['inputs'], game, offs, actions=d['actions'], config=d['config'], dt=dt)
        same(got, d['final'], 'doors dt 1/%s: states' % key)
        total, t_fired = len(d['inputs']) * dt, (fired + 1) * dt  # the effect is there at the end of tick `fired`
        height = offs.cpu().numpy()[np.arange(n), obj, 1].astype(np.float64)
        want = np.minimum(speed * (total - t_fired), first)
        worst = np.abs(height - want)[moving] / (speed * dt)[moving]
        print('the doors stand at %.4f .. %.4f; off speed * (T - T_fired) by %.3f of speed * dt at the most' % (
            height[moving].min(), height[moving].max(), worst.max()))
        assert (np.abs(height - want)[moving] <= (speed * dt)[moving]).all(), worst.max()
        assert (height[moving] > 0).all() and (height[fired < 0] == 0).all()


def main():
    rd.set_device(0)
    case, args = sys.argv[1], sys.argv[2:]
    if case == 'step':
        case_step(int(args[0]))
    elif case == 'game':
        case_game(*args)
    elif case == 'worldset':
        case_worldset(*args)
    elif case == 'edges':
        case_edges()
    elif case == 'model':
        case_model(int(args[0]), int(args[1]))
    elif case == 'doors':
        case_doors(args[0])
    else:
        raise SystemExit('unknown case %r' % case)
    print('RESULT ok')
    return 0


if __name__ == '__main__':
    sys.exit(main())
