"""Rank > 0 shards of every device environment and update kind on ONE GPU in ONE process.

tests/test_distributed_gpu.py runs the reference maze as two spawned ranks; everything else reached Trainer with rank 0 of
1 only.  Here the other ranks are stood in for through Trainer's `grad_sync` callable (tests/sharded_cases.py):

A. Trainer(rank=1, world_size=2) of every environment family against OracleTrainer on the host models of the global
   actors [B, 2B): the loop and bars of the family's own test_process_on_*_matches_oracle, world * g against the oracle's
   mean gradient.  B is chosen so that local and global indices disagree where they matter (5 actors on 3 tasks or 3
   layouts; rank 2 of 3 at B = 4 for the mixture: actor_base 8 = 2 mod 3, and 1 / 3 is no power of two).
B. Two ranks, each on its own PhiloxDraws columns, against one process holding all actors: per-actor integers exact, pi at
   the forward bar, the ranks' gradients adding up to the one-process gradient, parameters at tests/test_distributed_gpu.py's
   bars.  The exact comparison holds only while no action draw of the one-process run lies within the forward bar of a step
   of its row's CDF: asserted on every row, the measured closest distance is written next to each case's seed.
C. Update kinds whose W-rank job has no one-process counterpart (groups, minibatches, the opponent pool, advantage
   normalisation, the exploration bonus: blocks, slots, statistics and counts are per rank): world_size = 2 with a doubling
   exchange against world_size = 1 on the same actors, draws and weights."""
import numpy as np
import pytest

try:
    import sharded_cases as SC
    import maze_model as MM
    import fp_maze_model as FP
    import nav_maze_model as NM
    import gen_maze_model as GM
    import styled_maze_model as STM
    import goal_maze_model as GOAL
    import forage_maze_model as FM
    import arcade_model as AM
    import duel_model as DM
    import invaders_model as IM
    import repeat_model as RM
    import mix_model as MIX
    import selfplay_model as SPM
    import test_nav_maze_gpu as TNAV
    import test_styled_maze_gpu as TSTY
    import test_goal_maze_gpu as TGOAL
    import test_forage_maze_gpu as TFOR
    import test_arcade_gpu as TA
    import test_duel_gpu as TD
    import test_invaders_gpu as TI
    import test_arcade_mix_gpu as TMIX
    import test_selfplay_gpu as TSP
except ImportError:            # imported as tests.<module>
    from tests import sharded_cases as SC
    from tests import maze_model as MM
    from tests import fp_maze_model as FP
    from tests import nav_maze_model as NM
    from tests import gen_maze_model as GM
    from tests import styled_maze_model as STM
    from tests import goal_maze_model as GOAL
    from tests import forage_maze_model as FM
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests import invaders_model as IM
    from tests import repeat_model as RM
    from tests import mix_model as MIX
    from tests import selfplay_model as SPM
    from tests import test_nav_maze_gpu as TNAV
    from tests import test_styled_maze_gpu as TSTY
    from tests import test_goal_maze_gpu as TGOAL
    from tests import test_forage_maze_gpu as TFOR
    from tests import test_arcade_gpu as TA
    from tests import test_duel_gpu as TD
    from tests import test_invaders_gpu as TI
    from tests import test_arcade_mix_gpu as TMIX
    from tests import test_selfplay_gpu as TSP

pytestmark = pytest.mark.gpu

# three 5 x 5 rooms that differ in their inner walls: with 10 actors over 3 layouts, the shard [5, 10) holds other layouts than
# [0, 5); random cells in rooms of 21..25 free cells rarely put the goal beside the start (shard_against_oracle's fill)
ROOMS = [["+++++++", "+-----+", "+-----+", "+--S--+", "+-----+", "+-----+", "+++++++"],
         ["+++++++", "+-----+", "+-+-+-+", "+--S--+", "+-+-+-+", "+-----+", "+++++++"],
         ["+++++++", "+--+--+", "+-----+", "+--S--+", "+-----+", "+--+--+", "+++++++"]]
FP_ROOMS = [["+++++++", "+----G+", "+-----+", "+--S--+", "+-----+", "+-----+", "+++++++"],
            ["+++++++", "+-----+", "+-+-+-+", "+--S--+", "+-+-+-+", "+G----+", "+++++++"],
            ["+++++++", "+--+--+", "+-----+", "+--S--+", "+-----+", "+--+-G+", "+++++++"]]
MIX_SHORT = tuple(dict(s, max_episode_steps=m) for s, m in zip(MIX.MIX3, (9, 7, 8)))     # tests/test_arcade_mix_gpu.py


def _maze(layouts, **kw):
    def register(name):
        from unreal_amd.environment.environment import Environment
        Environment.register_maze_config(name, layouts, **kw)
        return Environment.MAZE_CONFIG[name]
    return register


def _maze_hosts(model):
    return lambda conf, B, seed, base, total: model.host_batch(conf, B, actor_base=base, actors_total=total, seed=seed)


def _arcade_hosts(model, **kw):
    return lambda conf, B, seed, base, total: model.host_batch(conf, B, seed, actor_base=base, **kw)


def _cells(tr, hosts, what, heading=True):
    B, ring = len(hosts), tr.ring
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(h.x, h.y) for h in hosts], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(h.gx, h.gy) for h in hosts], err_msg=what)
    if heading:
        np.testing.assert_array_equal(ring.heading.cpu().numpy(), [h.h for h in hosts], err_msg=what)


def _check_topdown(tr, hosts, what):
    _cells(tr, hosts, what, heading=False)
    np.testing.assert_array_equal(tr.ring.layout.cpu().numpy(), [h.layout for h in hosts], err_msg=what)
    assert len(set(h.layout for h in hosts)) > 1


def _check_fp(tr, hosts, what):
    _cells(tr, hosts, what)
    np.testing.assert_array_equal(tr.ring.layout.cpu().numpy(), [h.layout for h in hosts], err_msg=what)
    np.testing.assert_array_equal(SC.current_frames(tr.ring), [h.frame.reshape(-1) for h in hosts], err_msg=what)


def _check_nav(tr, hosts, what):
    _cells(tr, hosts, what)
    np.testing.assert_array_equal(tr.ring.nav.cpu().numpy().reshape(len(hosts), 8), [h.record() for h in hosts], err_msg=what)


def _check_gen(tr, hosts, what):
    _cells(tr, hosts, what)
    np.testing.assert_array_equal(tr.ring.gen.cpu().numpy().reshape(len(hosts), -1), [h.actor_record() for h in hosts],
                                  err_msg=what)
    walls = tr.environment.current_layouts()[0]
    assert len(set(w.tobytes() for w in walls)) > 1, what


def _check_styled(tr, hosts, what):
    _cells(tr, hosts, what)
    np.testing.assert_array_equal(tr.ring.actor_records.cpu().numpy(), [h.actor_record() for h in hosts], err_msg=what)
    np.testing.assert_array_equal(SC.current_frames(tr.ring), [h.frame.reshape(-1) for h in hosts], err_msg=what)
    np.testing.assert_array_equal(tr.environment.current_styles().reshape(len(hosts), -1), [h.style_ids() for h in hosts],
                                  err_msg=what)


def _check_goal(tr, hosts, what):
    np.testing.assert_array_equal(TGOAL._records(tr.ring), np.stack([h.actor_record() for h in hosts]), err_msg=what)
    TGOAL._check_current_objective(tr.ring, hosts, what)


def _check_records(tr, hosts, what):
    np.testing.assert_array_equal(tr.environment.current_records(), [h.record() for h in hosts], err_msg=what)


def _check_selfplay(tr, hosts, what):
    np.testing.assert_array_equal(TSP._mirrored(tr.environment), [h.record() for h in hosts], err_msg=what)


def _arcade(register, **kw):
    return lambda name: register(name, **kw)


REPEAT4 = dict(action_repeat=4, return_reward=2)                 # tests/test_arcade_repeat_gpu.py
# the duel's ball is served from the middle at 4 pixels a step: the first point falls around step 12, so a limit of 15 steps
# gives 20 rollout steps both rewarded steps and episodes that end (at 9 steps every episode only timed out)
NAV_KW = dict(TNAV.NAV_KW, random_start=True, max_episode_steps=7)
A_CASES = [
    # net_seed 4: with 3 (the other cases') an episode of the fill ends on its first step (shard_against_oracle's fill)
    dict(id="topdown", env_type="maze", B=5, net_seed=4, check=_check_topdown, hosts=_maze_hosts(MM),
         register=_maze(ROOMS, random_start=True, random_goal=True, max_episode_steps=12)),
    dict(id="first_person", env_type="maze", B=5, check=_check_fp, hosts=_maze_hosts(FP),
         register=_maze(FP_ROOMS, view="first_person", show_goal=True, random_start=True, max_episode_steps=6)),
    dict(id="navigation", env_type="maze", B=3, A=6, check=_check_nav, hosts=_maze_hosts(NM),
         register=_maze([TNAV.NAV_ROOM], view="first_person", goal_respawn=True, **NAV_KW)),
    dict(id="generated", env_type="maze", B=3, check=_check_gen, hosts=_maze_hosts(GM),
         register=_maze(None, random_start=True, random_goal=True, view="first_person", generate=7, gen_loops=2,
                        show_goal=True, max_episode_steps=7)),
    dict(id="styled", env_type="maze", B=3, check=_check_styled, hosts=_maze_hosts(STM),
         register=_maze(None, view="first_person", wall_styles=TSTY.STYLES[:4], random_start=True, random_goal=True,
                        generate=7, gen_loops=2, gen_landmark_density=128, show_goal=True, max_episode_steps=7)),
    dict(id="goal_sense", env_type="maze", B=3, A=6, objective_size=3, check=_check_goal, hosts=_maze_hosts(GOAL),
         register=_maze([TNAV.NAV_ROOM], view="first_person", goal_sense=True, progress_reward=1, **NAV_KW)),
    dict(id="forage", env_type="maze", B=3, A=6, check=_check_nav, hosts=_maze_hosts(FM),
         register=_maze([TFOR.FORAGE_ROOM], view="first_person", random_start=True, max_episode_steps=7, **TFOR.FORAGE_KW)),
    dict(id="breakout", env_type="arcade", B=3, check=_check_records, hosts=_arcade_hosts(AM),
         register=_arcade(TA._register, **TA.SHORT)),
    dict(id="duel", env_type="arcade", B=3, check=_check_records, hosts=_arcade_hosts(DM),
         register=_arcade(TA._register, **dict(TD.SHORT, max_episode_steps=15))),
    dict(id="invaders", env_type="arcade", B=3, check=_check_records, hosts=_arcade_hosts(IM),
         register=_arcade(TA._register, **dict(TI.SHORT, max_episode_steps=15))),
    dict(id="repeat4", env_type="arcade", B=3, check=_check_records, hosts=_arcade_hosts(RM),
         register=_arcade(TA._register, **dict(TD.SHORT, max_episode_steps=9, **REPEAT4))),
    dict(id="mixture", env_type="arcade", B=5, check=_check_records, hosts=_arcade_hosts(MIX), mix=True,
         register=lambda name: TMIX._register_mix(name, MIX_SHORT)),
    dict(id="mixture_rank2of3", env_type="arcade", B=4, rank=2, world=3, check=_check_records, hosts=_arcade_hosts(MIX),
         mix=True, register=lambda name: TMIX._register_mix(name, MIX_SHORT)),
    dict(id="selfplay", env_type="arcade", B=4, check=_check_selfplay, partner="selfplay",
         hosts=lambda conf, B, seed, base, total: SPM.host_batch(conf, B, seed, actor_base=base,
                                                                 scripts=[[] for _ in range(B)]),
         register=_arcade(TSP._register, **dict(TSP.SHORT, max_episode_steps=15))),
    dict(id="opponent_pool", env_type="arcade", B=4, check=_check_records, partner="pool",
         hosts=lambda conf, B, seed, base, total: [SPM.HostSeat(conf, 2 * (base + b), seed, partner=[]) for b in range(B)],
         register=_arcade(TSP._register, **dict(TSP.SHORT, max_episode_steps=15))),
]


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A_CASES, ids=[c["id"] for c in A_CASES])
def test_a_shard_matches_the_oracle_on_its_global_actors(case):
    """Trainer(rank, world_size) of one environment family, LSTM + full UNREAL, H = 40, T = 5, 4 updates, against
    OracleTrainer(envs=host_batch(..., actor_base=rank B, actors_total=world B))."""
    rank, world, B = case.get("rank", 1), case.get("world", 2), case["B"]
    out = SC.shard_against_oracle(case, rank, world, B)
    tr, hosts = out["tr"], out["hosts"]
    assert out["n_term"] > 0, "no episode ended inside a rollout"
    print("family A %s: rewards seen %s, %d episodes ended" % (case["id"], sorted(out["rewards"]), out["n_term"]))
    assert out["rewards"] - {0.0}, "no step of any rollout was rewarded: the episodes only ever timed out"
    if case["env_type"] == "arcade":
        assert tr.full_environment.arcade[1] == rank * B                  # the kernels' actor_base
    if case.get("mix"):
        K = 3
        task = tr.full_environment.task_of_actor()
        assert list(task) == [(rank * B + b) % K for b in range(B)] and list(task) != [b % K for b in range(B)]
        scores = tr.task_scores()
        assert [s["game"] for s in scores] == ["breakout", "duel", "invaders"]
        assert sum(s["episodes"] for s in scores) == out["n_term"]
        # per task: the episodes the rollouts finished on the actors whose GLOBAL index is on that task
        for k, s in enumerate(scores):
            assert s["episodes"] == sum(int(out["ended"][b]) for b in range(B) if (rank * B + b) % K == k), (k, scores)


# ---- B ------------------------------------------------------------------------------------------------------------------------
def _register_b(kind, name):
    from unreal_amd.environment.environment import Environment
    if kind == "mixture":
        TMIX._register_mix(name, MIX_SHORT)
    elif kind == "selfplay":
        TSP._register(name, **dict(TSP.SHORT, max_episode_steps=15))
    elif kind == "generated":
        Environment.register_maze_config(name, None, random_start=True, random_goal=True, view="first_person", generate=7,
                                         gen_loops=2, show_goal=True, max_episode_steps=4)
    else:
        Environment.register_maze_config(name, ROOMS, random_start=True, random_goal=True, max_episode_steps=4)
    return Environment.MAZE_CONFIG if kind in ("generated", "topdown") else Environment.ARCADE_CONFIG


# (kind, actors per rank, trainer seed, exchanges per call, trainer options).  The seed is one at which no action draw of the
# one-process run (fill and rollouts, every row) lies within 1e-5 of a step of its row's CDF; beside each case the closest
# distance measured on MI355X, 35 to 150 times the forward bar.
B_CASES = [
    ("mixture", 5, 0xA3C, 2, dict(reuse_epochs=2, adam=SC.ADAM)),                                  # closest 1.003e-03
    ("selfplay", 4, 0xA3C, 1, dict()),                                                             # closest 1.046e-03
    ("generated", 5, 0xA3C, 1, dict(depth=True, bootstrap_timeouts=True, gae_lambda=0.9)),         # closest 4.403e-04
    ("topdown", 5, 0xA3C, 1, dict()),                                                              # closest 3.493e-04
]


@pytest.mark.parametrize("kind,B,seed,syncs,options", B_CASES, ids=[c[0] for c in B_CASES])
def test_two_ranks_in_one_process_match_one_process_with_all_actors(kind, B, seed, syncs, options):
    """Family B: groups = 1, H = 50, T = 5, three updates after the fill; every trainer on its own draws."""
    T, H = 5, 50
    env_type = "maze" if kind in ("generated", "topdown") else "arcade"
    name = "sharded_b_" + kind
    registry = _register_b(kind, name)
    try:
        def make(rank, world, batch, sync):
            state = dict(generated=SC.RING_GENERATED, topdown=SC.RING_TOPDOWN).get(kind, SC.RING_ARCADE)
            net, applier, tr = SC.build(env_type, name, batch, T, H, state=state, rank=rank, world_size=world, grad_sync=sync,
                                        seed=seed, **options)
            assert tr._own_draws and (tr.draws.col0, tr.draws.stride) == (rank * batch, world * batch)
            return net, applier, tr
        closest = SC.compare_ranks_with_whole(make, B, T, updates=3, world=2, syncs_per_call=syncs)
        print("family B %s seed %#x: closest action draw to a CDF step %.3e" % (kind, seed, closest))
    finally:
        registry.pop(name, None)


# ---- C ------------------------------------------------------------------------------------------------------------------------
C_CASES = [
    ("groups", "mixture", 8, 2, dict(groups=2)),
    ("minibatches", "mixture", 8, 4, dict(reuse_epochs=2, reuse_minibatches=2, adam=SC.ADAM)),
    ("opponent_pool", "selfplay", 4, 1, dict(opponent_pool=2, opponent_snapshot_every=1)),
    ("normalize_explore", "mixture", 8, 1, dict(normalize_advantages=True, explore_beta=0.0625)),
]


@pytest.mark.parametrize("what,kind,B,steps,options", C_CASES, ids=[c[0] for c in C_CASES])
def test_world_size_scales_update_kinds_that_are_per_rank(what, kind, B, steps, options):
    """Family C: H = 50, T = 5, three process() calls; `steps` optimiser steps a call (G, E M, 1)."""
    name = "sharded_c_" + what
    registry = _register_b(kind, name)
    try:
        two, one = SC.run_scaled_pair("arcade", name, B, 5, 50, steps, calls=3, **options)
        assert any(s["terminal_end"].any() for s in one["snaps"])
    finally:
        registry.pop(name, None)


def test_pool_opponents_of_a_rank_draw_their_global_columns():
    """The opponents' own stream (Trainer.opp_draws) is keyed like the learner's: rank r's uniforms of the fill's last step
    and of a rollout are the columns [r B, (r + 1) B) of a one-process trainer's with 2 B actors, bit for bit (the draws do not
    depend on the weights or the games, so the slots being cut per rank does not matter here)."""
    B, T, H = 4, 5, 12
    name = "sharded_pool_draws"
    registry = _register_b("selfplay", name)
    try:
        runs = []
        for rank, world, batch in ((0, 1, 2 * B), (0, 2, B), (1, 2, B)):
            net, applier, tr = SC.build("arcade", name, batch, T, H, rank=rank, world_size=world, opponent_pool=2)
            assert (tr.opp_draws.col0, tr.opp_draws.stride) == (rank * batch, world * batch)
            while not tr._full:
                tr.process(None, 0)
            fill = (tr.opp_u[:batch].cpu().numpy().copy(), tr.u_act[:batch].cpu().numpy().copy())
            tr.process(None, 0)
            runs.append((fill, SC.snapshot(tr)))
        (wfill, whole), ranks = runs[0], runs[1:]
        assert len(set(whole["opp_u"].reshape(-1).tolist())) == 2 * B * T
        for r, (fill, s) in enumerate(ranks):
            cols = slice(r * B, (r + 1) * B)
            for got, want in zip(fill, wfill):
                np.testing.assert_array_equal(got, want[cols])
            np.testing.assert_array_equal(s["opp_u"], whole["opp_u"][:, cols])
            np.testing.assert_array_equal(s["u_act"], whole["u_act"][:, cols])
    finally:
        registry.pop(name, None)
