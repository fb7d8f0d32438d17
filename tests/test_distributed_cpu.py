"""N > 1 path on CPU: world_size 2 over gloo (127.0.0.1).  Each rank owns its shard of the actors,
produces its local mean gradient in the product's flat layout (the per-actor gradients come from the
oracle here -- the HIP kernels need a GPU), and the product's exchange step (`parallel.all_reduce_sum`,
the one collective of the path) must reproduce the single-process mean over ALL actors."""
import inspect
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.trainer import OracleTrainer, ExplicitDraws

CFG = dict(action_size=4, use_lstm=True, use_pixel_change=True, use_value_replay=True,
           use_reward_prediction=True, pixel_change_lambda=0.05, entropy_beta=0.001, local_t_max=5,
           n_step_TD=5, gamma=0.99, gamma_pc=0.9, experience_history_size=12, max_time_step=10 ** 6,
           rmsp_alpha=0.99, rmsp_epsilon=0.1, grad_norm_clip=40.0, initial_alpha_low=1e-4,
           initial_alpha_high=5e-3, initial_alpha_log_rate=0.5)


def _actor_draws(gid):
    rs = np.random.RandomState(1000 + gid)
    d = ExplicitDraws()
    d.action_u = list(rs.random_sample(CFG["experience_history_size"] + CFG["n_step_TD"]))
    d.seq_starts = list(rs.randint(0, CFG["experience_history_size"] - CFG["local_t_max"] - 2, size=2))
    d.rp_coin = [int(rs.randint(2))]
    d.rp_u = [float(rs.random_sample())]
    return d


def _local_mean_grad(actor_ids, scale):
    """Sum over this shard's actors of (per-actor gradient * scale), flattened in the product layout."""
    from unreal_amd.model.model import FlatParams, param_spec
    tr = OracleTrainer(CFG, n_actors=len(actor_ids), draws=[_actor_draws(g) for g in actor_ids], seed=7,
                       dtype=torch.float64)
    tr.fill()
    fp = FlatParams(param_spec(4), "cpu")
    flat = torch.zeros(fp.size, dtype=torch.float64)
    views = fp.make_views(flat)
    steps = 0
    for a in tr.actors:
        t0 = a.local_t
        a.draws.action_u = a.draws.action_u[:CFG["n_step_TD"]]
        g, _, _, _ = tr.actor_grad(a)
        steps += a.local_t - t0
        for (name, _), gi in zip(tr.params.items(), g):
            views[name] += gi.reshape(-1) * scale
    return flat, steps


def _worker(rank, world, port, per_rank, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from unreal_amd import parallel
    r, lr, w = parallel.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    lo, hi = parallel.actor_range(rank, per_rank)
    flat, steps = _local_mean_grad(list(range(lo, hi)), 1.0 / (per_rank * world))
    parallel.all_reduce_sum(flat)
    tot_steps = parallel.sum_over_ranks([steps], "cpu")[0]
    mx = parallel.max_over_ranks(float(rank), "cpu")
    parallel.barrier()
    q.put((rank, flat.numpy(), tot_steps, mx))
    torch.distributed.destroy_process_group()


def test_two_rank_gradient_exchange_equals_global_mean():
    world, per_rank = 2, 1
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, per_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    ref, steps = _local_mean_grad(list(range(world * per_rank)), 1.0 / (world * per_rank))
    for rank, flat, tot_steps, mx in res:
        np.testing.assert_allclose(flat, ref.numpy(), rtol=1e-12, atol=1e-14)
        assert tot_steps == steps and mx == world - 1
    np.testing.assert_array_equal(res[0][1], res[1][1])       # replicas stay bit-identical
    assert np.abs(ref.numpy()).max() > 0


# ---- the reference side of tests/test_sharded_gpu.py's family A ---------------------------------------------------------------
# A rank > 0 shard is held against host_batch(conf, B, actor_base=B, actors_total=2B).  That is evidence only if the models'
# own actor_base handling is right: the models B .. 2B-1 of one batch of 2B must be the same actors.
_ROOMS = [["+++++++", "+++++++", "++--G++", "++-S-++", "++---++", "+++++++", "+++++++"],
          ["+++++++", "++G--++", "++-S-++", "++---++", "++---++", "+++++++", "+++++++"],
          ["+++++++", "+++++++", "+----++", "+--S-++", "+G---++", "+++++++", "+++++++"]]
_NAV_ROOM = ["+++++++", "+++++++", "++A-G++", "++-SA++", "++A-A++", "+++++++", "+++++++"]
_FORAGE_ROOM = ["+++++++", "+++++++", "++ABA++", "++-SB++", "++A-C++", "+++++++", "+++++++"]
_NAV_KW = dict(view="first_person", goal_reward=10, apple_reward=1, hit_reward=0, action_set="lab", show_goal=True,
               random_start=True, max_episode_steps=7)
_STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (255, 255, 255, 0xFF), (10, 20, 250, 0x0F)]
_GEN_KW = dict(random_start=True, random_goal=True, view="first_person", generate=7, gen_loops=2, show_goal=True,
               max_episode_steps=7)


def _host_batch_cases():
    """-> [(id, model module name, config factory, action count, extra host_batch keywords)]"""
    def maze(layouts, **kw):
        def make():
            from unreal_amd.environment.maze_environment import MazeConfig
            return MazeConfig(layouts, **kw)
        return make

    def arcade(**kw):
        def make():
            from unreal_amd.environment.arcade_environment import ArcadeConfig
            return ArcadeConfig(**kw)
        return make

    def mix():
        from unreal_amd.environment.arcade_environment import ArcadeConfig, ArcadeMix
        import mix_model
        return ArcadeMix([ArcadeConfig(**dict(s, max_episode_steps=m)) for s, m in zip(mix_model.MIX3, (9, 7, 8))])

    def selfplay():
        from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
        return ArcadeSelfPlay(points=2, paddle_width=24, ball_speed=4, serve_wait=1, win_reward=7, lose_reward=-3,
                              max_episode_steps=9)
    short = dict(paddle_width=24, ball_speed=4, serve_wait=1, max_episode_steps=12)
    return [
        ("topdown", "maze_model", maze(_ROOMS, random_start=True, random_goal=True, max_episode_steps=7), 4, {}),
        ("first_person", "fp_maze_model", maze(_ROOMS, view="first_person", show_goal=True, random_start=True,
                                               max_episode_steps=7), 4, {}),
        ("navigation", "nav_maze_model", maze([_NAV_ROOM], goal_respawn=True, **_NAV_KW), 6, {}),
        ("generated", "gen_maze_model", maze(None, **_GEN_KW), 4, {}),
        ("styled", "styled_maze_model", maze(None, wall_styles=_STYLES, gen_landmark_density=128, **_GEN_KW), 4, {}),
        ("goal_sense", "goal_maze_model", maze([_NAV_ROOM], goal_sense=True, progress_reward=1, **_NAV_KW), 6, {}),
        ("forage", "forage_maze_model", maze([_FORAGE_ROOM], view="first_person", no_goal=True, apple_reward=1, hit_reward=0,
                                             action_set="lab", random_start=True, max_episode_steps=7,
                                             pickups=[(-1, (255, 255, 0), False), (20, (255, 0, 255), True)]), 6, {}),
        ("breakout", "arcade_model", arcade(rows=2, row_rewards=(7, 1), lives=1, life_reward=-1, **short), 4, {}),
        ("duel", "duel_model", arcade(game="duel", points=2, opponent_width=4, opponent_speed=1, win_reward=7, lose_reward=-1,
                                      **short), 4, {}),
        ("invaders", "invaders_model", arcade(game="invaders", alien_rows=1, lives=2, bomb_period=2, bomb_speed=4,
                                              march_period=1, descend=8, alien_rewards=(7,), life_reward=-1, **short), 4, {}),
        ("repeat4", "repeat_model", arcade(game="duel", points=2, opponent_width=4, opponent_speed=1, win_reward=7,
                                           lose_reward=-1, action_repeat=4, return_reward=2, **short), 4, {}),
        ("mixture", "mix_model", mix, 4, {}),
        ("selfplay", "selfplay_model", selfplay, 4, {"scripts": True}),
    ]


def _signature(m):
    """Everything a host model says about its actor's state."""
    sig = [np.asarray(m.last_state["image"])]
    for f in ("record", "actor_record", "style_ids", "objective"):
        if hasattr(m, f):
            sig.append(np.asarray(getattr(m, f)()))
    sig.append(np.asarray([getattr(m, n, -1) for n in ("x", "y", "gx", "gy", "h", "layout", "episode", "ep_steps")]))
    return sig


def test_host_batch_cases_cover_every_model_module():
    import glob
    have = set()
    for path in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "*_model.py")):
        with open(path) as f:
            if "def host_batch" in f.read():
                have.add(os.path.basename(path)[:-3])
    assert have == set(c[1] for c in _host_batch_cases())


@pytest.mark.parametrize("case", _host_batch_cases(), ids=[c[0] for c in _host_batch_cases()])
def test_host_batch_shard_is_the_same_actors_as_the_whole_batch(case):
    """host_batch(conf, B, actor_base=B, actors_total=2B) against models B .. 2B-1 of host_batch(conf, 2B, actors_total=2B):
    the same action script for 60 steps, a reset after every terminal; rewards, terminals, pixel change, records and frames."""
    import importlib
    _, module, make_conf, A, extra = case
    model = importlib.import_module(module)
    B, seed, steps = 4, 0xA3C, 60
    conf = make_conf()
    kw_whole, kw_shard = {}, dict(actor_base=B)
    if "actors_total" in inspect.signature(model.host_batch).parameters:
        kw_whole, kw_shard = dict(actors_total=2 * B), dict(actor_base=B, actors_total=2 * B)
    if extra.get("scripts"):
        kw_whole["scripts"], kw_shard["scripts"] = [[] for _ in range(2 * B)], [[] for _ in range(B)]
    whole = model.host_batch(conf, 2 * B, seed=seed, **kw_whole)
    shard = model.host_batch(conf, B, seed=seed, **kw_shard)
    first = model.host_batch(conf, B, seed=seed, **{k: v for k, v in kw_shard.items() if k != "actor_base"})
    rs = np.random.RandomState(5)
    acts = rs.randint(0, A, (steps, 2 * B))
    n_term, differs_from_first = 0, False
    for b in range(B):
        for x, y in zip(_signature(shard[b]), _signature(whole[B + b])):
            np.testing.assert_array_equal(x, y, err_msg="actor %d at reset" % b)
    for s in range(steps):
        for b in range(B):
            pair = (shard[b], whole[B + b])
            out = []
            for m in pair:
                if extra.get("scripts"):
                    m.partner = [int(acts[s, B + (b ^ 1)])]
                out.append(m.process(int(acts[s, B + b])))
            (_, r0, t0, pc0), (_, r1, t1, pc1) = out
            assert (r0, bool(t0)) == (r1, bool(t1)), (s, b)
            np.testing.assert_array_equal(pc0, pc1, err_msg="step %d actor %d pixel change" % (s, b))
            if t0:
                n_term += 1
                for m in pair:
                    m.reset()
            for x, y in zip(_signature(pair[0]), _signature(pair[1])):
                np.testing.assert_array_equal(x, y, err_msg="step %d actor %d" % (s, b))
            # the actors [0, B) fed the same actions are other actors (else the comparison above says nothing)
            m = first[b]
            if extra.get("scripts"):
                m.partner = [int(acts[s, B + (b ^ 1)])]
            if m.process(int(acts[s, B + b]))[2]:
                m.reset()
            differs_from_first |= any(not np.array_equal(x, y) for x, y in zip(_signature(m), _signature(pair[0])))
    assert n_term > 0 and differs_from_first
