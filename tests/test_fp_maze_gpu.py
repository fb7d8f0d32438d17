"""First-person views of configured mazes on the device (maze.hip, the unreal_maze_* entries with view 1) against the
host model of tests/fp_maze_model.py, the two-launch paths, OracleTrainer and the top-down maze."""
import numpy as np
import pytest
import torch

try:
    import fp_maze_model as FP
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import maze_model as MM
try:
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_maze_config_gpu import GOAL_ROOM, RING_ARRAYS, CFG_ARRAYS
except ImportError:
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_maze_config_gpu import GOAL_ROOM, RING_ARRAYS, CFG_ARRAYS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
FP_ARRAYS = RING_ARRAYS + CFG_ARRAYS + ("heading",)


def _config(N, L=5, seed=0, marks="", **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    return MazeConfig([MM.random_layout(N, rs, marks=marks) for _ in range(L)], view="first_person", **kw)


def _env(B, H, config, seed=0, **kw):
    from unreal_amd.environment.maze_environment import batched_maze_environment, FirstPersonMazeEnvironment
    env = batched_maze_environment(B, H, DEV, config=config, seed=seed, **kw)
    assert isinstance(env, FirstPersonMazeEnvironment) and env.frame_scale == 1.0 / 255.0
    env.ring.frames.zero_()           # (torch.empty: slots no step has written would hold stale allocator bytes)
    env.ring.r_pc.zero_()
    env.reset()
    return env


def _hosts(cfg, B, seed):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = FP.host_batch(cfg, B, seed=seed)
    for m in models:
        m.reset()
    return models


def _current_frames(ring):
    idx = ring.cur_idx().long()
    return ring.frames.view(-1, FB)[idx].cpu().numpy()


def _check_state(ring, models, what, count=None):
    B = len(models)
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.heading.cpu().numpy(), [m.h for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    want = np.stack([m.frame.reshape(-1) for m in models])
    got = _current_frames(ring)
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), "%s: frames of actors %s differ" % (what, bad[:8])


# (N, B, flags, start_heading): every N and every batch size, random / fixed cells, shown / hidden goal, fixed / drawn headings
RESET_CASES = [(7, 4096, "goal show", None), (12, 512, "start goal show", 1), (14, 64, "start", None),
               (21, 3, "start goal show", None), (21, 512, "", 3), (7, 64, "start goal", None)]


@pytest.mark.parametrize("N,B,flags,heading", RESET_CASES)
def test_reset_frames_match_the_host_model(N, B, flags, heading):
    """The first observation of every actor, byte for byte, with its cell, heading and goal; then a masked reset."""
    seed = 0xF00D + N + B
    cfg = _config(N, L=7, seed=B, marks="SG", random_start="start" in flags, random_goal="goal" in flags,
                  show_goal="show" in flags, start_heading=heading)
    env = _env(B, 2, cfg, seed=seed)
    models = _hosts(cfg, B, seed)
    _check_state(env.ring, models, "reset")
    if heading is None and B >= 64:
        assert len(set(m.h for m in models)) == 4
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    _check_state(env.ring, models, "masked reset")


@pytest.mark.parametrize("N", [7, 12, 14, 21])
def test_random_steps_match_the_host_model(N):
    """Seven layouts over 200 actors, random start / goal, the goal shown, a step limit of 37, 120 random actions with a
    masked reset half way: frames, pixel change (bit for bit, and equal to unreal_pixel_change_u8 on the two stored
    frames), rewards, terminals, counts, cells, headings, episode steps / indices and last action / reward."""
    from unreal_amd import ops
    B, H, steps, seed = 200, 3, 120, 0xBEEF + N
    H1 = H + 1
    cfg = _config(N, L=7, seed=N, random_start=True, random_goal=True, show_goal=True, max_episode_steps=37)
    env = _env(B, H, cfg, seed=seed)
    ring = env.ring
    models = _hosts(cfg, B, seed)
    assert len(set(ring.layout.cpu().numpy())) == 7
    rs = np.random.RandomState(N)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    pc_u8 = torch.zeros(B * PC, dtype=torch.float32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n_goal = n_timeout = n_hit = 0
    _check_state(ring, models, "after reset", count)
    for step in range(steps):
        acts = rs.randint(0, 4, B).astype(np.int32)
        env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True, track_score=True)
        want_r, want_t, want_pc = [], [], []
        for b, m in enumerate(models):
            _, r, t, pc = m.process(acts[b])
            want_r.append(r); want_t.append(t); want_pc.append(pc)
            n_goal += t and not m.timed_out
            n_timeout += t and m.timed_out
            n_hit += r == -1
            if t:
                m.reset()
        np.testing.assert_array_equal(out_r.cpu().numpy(), np.array(want_r, dtype=np.float32), err_msg=str(step))
        term = np.array(want_t, dtype=bool)
        np.testing.assert_array_equal(out_t.cpu().numpy(), term.astype(np.int32), err_msg=str(step))
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(discard, old, old + 1)
        committed_terminal = np.where(discard, committed_terminal, term)
        _check_state(ring, models, "step %d" % step, count)
        base = np.arange(B) * H1 + old % H1
        pc_dev = ring.r_pc.view(-1, PC)[torch.from_numpy(base).to(DEV)].cpu().numpy()
        np.testing.assert_array_equal(pc_dev, np.stack(want_pc).reshape(B, PC), err_msg=str(step))
        live = np.flatnonzero(~term)
        if len(live):
            idx_new = torch.from_numpy((live * H1 + count[live] % H1).astype(np.int32)).to(DEV)
            idx_old = torch.from_numpy((live * H1 + old[live] % H1).astype(np.int32)).to(DEV)
            ops.pixel_change_u8(ring.frames, idx_new, idx_old, 48.0 * 255.0, pc_u8[:len(live) * PC])
            np.testing.assert_array_equal(pc_u8[:len(live) * PC].cpu().numpy().reshape(-1, PC), pc_dev[live])
        if step == steps // 2:
            mask = rs.uniform(size=B) < 0.5
            env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
            for b in np.flatnonzero(mask):
                models[b].reset()
            _check_state(ring, models, "masked reset", count)
    assert n_goal > 0 and n_timeout > 0 and n_hit > 0, (n_goal, n_timeout, n_hit)


def _rollout_state(B, xld):
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
    return dict(active=torch.ones(B, dtype=torch.int32, device=DEV), log=z(B), n=z(B), te=z(B), r=z(B, torch.float32),
                t=z(B), a=z(B), pi=z(B * 4, torch.float32), v=z(B, torch.float32), idx=z(B),
                lar=torch.zeros(B * xld, device=DEV))


@pytest.mark.parametrize("B", [64, 300])
def test_fused_rollout_steps_are_the_two_launch_paths(B):
    """On two views of each environment (index_parent: frame indices into the whole ring):
    rollout_step == process + rollout_advance (+ cur_idx and the [one-hot last action | last reward] columns), and
    policy_rollout_step == policy_step + rollout_step, bit for bit, with goals and time-outs ending episodes."""
    from unreal_amd import ops
    H, A, xld = 4, 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    cfg = _config(7, L=3, random_goal=True, random_start=True, show_goal=True, max_episode_steps=4)
    envs = [_env(B, H, cfg, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    st = [_rollout_state(B, xld) for _ in envs]
    n_term = 0
    for step in range(8):
        X = dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = dev(rs.uniform(0, 1, B), torch.float64)
        for k, (e, s) in enumerate(zip(envs, st)):
            for v, (b0, b1) in zip(views[k], ((0, cut), (cut, B))):
                sl = {n: t[b0:b1] for n, t in s.items() if n not in ("pi", "lar")}
                pi, lar = s["pi"][4 * b0:4 * b1], s["lar"][b0 * xld:b1 * xld]
                nxt = dict(next_idx=sl["idx"], next_lar=lar, lar_ld=xld, lar_col0=256, A=A)
                if k == 0:             # the two-launch step: policy_step, process, rollout_advance, cur_idx
                    ops.policy_step(b1 - b0, A, X[b0 * 256:], 256, Wp, bp, Wv, bv, u[b0:b1], pi, sl["v"], sl["a"])
                    act_before = sl["active"].clone()
                    v.process(sl["a"], act_before, sl["r"], sl["t"], reset_on_terminal=True, track_score=True)
                    ops.rollout_advance(b1 - b0, sl["t"], sl["active"], sl["log"], sl["n"], sl["te"])
                    v.ring.cur_idx(out=sl["idx"], base_actor=b0)
                elif k == 1:           # policy_step + the fused rollout step
                    ops.policy_step(b1 - b0, A, X[b0 * 256:], 256, Wp, bp, Wv, bv, u[b0:b1], pi, sl["v"], sl["a"])
                    v.rollout_step(sl["a"], sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"],
                                   index_parent=True, **nxt)
                else:                  # everything in one launch
                    feat = X[b0 * 256:b1 * 256]
                    net = type("Net", (), {"p": dict(W_base_fc_p=Wp, b_base_fc_p=bp, W_base_fc_v=Wv, b_base_fc_v=bv)})
                    v.policy_rollout_step(net, feat, 256, u[b0:b1], pi, sl["v"], sl["a"], sl["r"], sl["t"], sl["active"],
                                          sl["log"], sl["n"], sl["te"], index_parent=True, **nxt)
        for name in FP_ARRAYS:
            for e in envs[1:]:
                assert torch.equal(getattr(envs[0].ring, name), getattr(e.ring, name)), (step, name)
        for key in ("active", "log", "n", "te", "a", "pi", "v", "idx"):
            for s in st[1:]:
                assert torch.equal(st[0][key], s[key]), (step, key)
        for key in ("r", "t"):         # written for the actors that stepped
            live = st[0]["log"].bool()
            for s in st[1:]:
                assert torch.equal(st[0][key][live], s[key][live]), (step, key)
        assert torch.equal(st[1]["lar"], st[2]["lar"]), step
        lar = st[1]["lar"].view(B, xld)[:, 256:261].cpu().numpy()
        la, lr = envs[0].ring.last_action.cpu().numpy(), envs[0].ring.last_reward.cpu().numpy()
        np.testing.assert_array_equal(lar[:, :4], np.eye(4, dtype=np.float32)[la], err_msg=str(step))
        np.testing.assert_array_equal(lar[:, 4], lr, err_msg=str(step))
        n_term += int(st[0]["te"].sum())
        if step == 3:                  # a new rollout: every actor active again
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert n_term > 0


# the goal two cells from the start: no episode ends on its first step, so no actor discards a successive terminal frame
# (the device fills all actors in lock-step, the oracle each actor to exactly its history: their counts then agree)
FP_ROOM = ["+++++++",
           "+++++++",
           "++--G++",
           "++-S-++",
           "++---++",
           "+++++++",
           "+++++++"]


def _register(name, layout=FP_ROOM, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config(name, [layout], view="first_person", **kw)
    return Environment.MAZE_CONFIG[name]


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_a_first_person_maze_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor, at the bars of
    test_process_on_a_configured_maze_matches_oracle: full UNREAL (pixel control on the first-person pixel change) and
    FF with no auxiliary task."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import FirstPersonMazeEnvironment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "fp_room_%d%d" % (use_lstm, aux)
    conf = _register(name, show_goal=True, max_episode_steps=7)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name=name)
        assert isinstance(tr.environment, FirstPersonMazeEnvironment) and net.frame_scale == 1.0 / 255.0
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = FP.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(tr.ring.heading.cpu().numpy(), [h.h for h in hosts])
        ends = set()
        for it in range(4):
            draws.log.clear()
            lr = tr._anneal_learning_rate(0)
            tr.compute_gradients()
            g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
            losses_dev = tr._publish_losses()
            _feed_draws(cfg, draws.log, edraws, T, B)
            steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(0)
            n_dev = tr.n_steps.cpu().numpy()
            acts = tr.actions.cpu().numpy().reshape(T, B)
            rews = tr.rewards.cpu().numpy().reshape(T, B)
            assert int(n_dev.sum()) == steps_o
            for b in range(B):
                n = infos[b]["n"]
                assert n_dev[b] == n
                assert list(acts[:n, b]) == infos[b]["actions"]
                assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]]
                assert bool(tr.terminal_end.cpu()[b]) == infos[b]["terminal_end"]
                if infos[b]["terminal_end"]:
                    ends.add("goal" if infos[b]["rewards"][-1] == 1 else "timeout")
            for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
                if key not in losses_dev or key not in losses_o[0]:
                    continue
                want = np.mean([l[key] for l in losses_o])
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[pname] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, pname)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            np.testing.assert_array_equal(tr.ring.pos.cpu().numpy().reshape(B, 2), [(h.x, h.y) for h in hosts])
            np.testing.assert_array_equal(tr.ring.heading.cpu().numpy(), [h.h for h in hosts])
        assert "timeout" in ends, ends
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_grouped_process_on_a_first_person_maze_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes (views of the first-person environment), each
    with its own update, against OracleTrainer.process_async in actor order (the bars of
    test_grouped_process_is_the_reference_algorithm_actor_after_actor)."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "fp_room_grouped"
    conf = _register(name, max_episode_steps=5)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = FP.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for k, u in enumerate(draws.log):
            edraws[k % B].action_u.append(float(u[0]))
        orc.fill()
        np.testing.assert_array_equal(tr.full_ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        global_t, n_scores = 0, 0
        for it in range(3):
            draws.log.clear()
            steps_dev, score_dev = tr.process(None, global_t)
            assert len(draws.log) == 5 * B
            steps_o = 0
            for b in range(B):
                lg = draws.log[5 * b:5 * b + 5]
                edraws[b].action_u = [float(x) for x in lg[0]]
                edraws[b].seq_starts = [int(lg[1][0]), int(lg[2][0])]
                edraws[b].rp_coin, edraws[b].rp_u = [int(lg[3][0])], [float(lg[4][0])]
                d, sc, _ = orc.process_async(b, global_t + b * T)
                steps_o += d
                n_scores += sc is not None
                edraws[b].action_u = []
            assert steps_dev == steps_o
            for pname, ref in orc.params.items():
                got = net.p[pname].cpu().double().numpy()
                want = ref.numpy().reshape(-1)
                assert np.abs(got - want).max() <= 2e-6 + 2e-5 * np.abs(want).max(), (it, pname)
            np.testing.assert_array_equal(tr.full_ring.heading.cpu().numpy(), [h.h for h in hosts])
            global_t += steps_dev
        assert n_scores > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_evaluate_on_a_first_person_maze_matches_the_host_model():
    """Evaluate(maze=name) on a first-person config: per-actor rewards / terminals of every step and the first episode's
    outcome agree with the host model replaying the device's actions; the counts are those of the first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "fp_room_eval"
    conf = _register(name, GOAL_ROOM, random_goal=True, random_start=True, show_goal=True, max_episode_steps=10)
    try:
        cfg = _cfg(True, False, 40, 20)
        net, _, _, _ = _build(cfg, 1, seed=31, env_name=name)
        B, seed = 16, 0x5EED
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, maze=name)
        assert net.frame_scale == 1.0 / 255.0
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = FP.host_batch(conf, B, seed=seed)
        for h in hosts:
            h.reset()                  # Evaluate.process: self.env.reset()
        first = [None] * B
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                if t:
                    if first[b] is None:
                        first[b] = "timeout" if h.timed_out else "goal"
                    h.reset()
        assert None not in first
        n_goal = first.count("goal")
        assert res["episodes"] == B and res["timeouts"] == B - n_goal
        assert abs(res["success_rate"] - n_goal / float(B)) < 1e-12
        assert n_goal > 0, first
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_batch1_environment_gives_host_model_frames_at_one_255th():
    """Environment.create_environment('maze', name) on a first-person config: images are the host model's bytes / 255,
    rewards, terminals and pixel change the host model's (no reset on terminal: the caller resets)."""
    from unreal_amd.environment.environment import Environment
    name = "fp_room_batch1"
    conf = _register(name, GOAL_ROOM, random_goal=True, random_start=True, show_goal=True, max_episode_steps=9)
    try:
        env = Environment.create_environment("maze", name)
        host = FP.HostFirstPersonMaze(conf, 0, 1, seed=0)
        host.reset()                   # (MazeEnvironment's constructor resets twice: its batched environment's, its own)
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term = 0
        for step in range(60):
            a = int(rs.randint(0, 4))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            assert (env.last_action, env.last_reward) == (host.last_action, host.last_reward)
            if terminal:
                n_term += 1
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_top_down_view_argument_changes_nothing():
    """A top-down config registered with view="top_down" steps bit for bit like one registered without the argument,
    in the same process as first-person environments."""
    from unreal_amd.environment.maze_environment import MazeConfig, BatchedMazeEnvironment, batched_maze_environment
    rs = np.random.RandomState(4)
    lays = [MM.random_layout(12, rs) for _ in range(3)]
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=9)
    B, H = 300, 3
    envs = []
    for c in (MazeConfig(lays, **kw), MazeConfig(lays, view="top_down", **kw)):
        e = batched_maze_environment(B, H, DEV, config=c, seed=7)
        assert type(e) is BatchedMazeEnvironment and e.frame_scale == 1.0
        e.ring.frames.zero_(); e.ring.r_pc.zero_()
        e.reset()
        envs.append(e)
    fp = _env(B, H, _config(12, L=3, random_goal=True, random_start=True), seed=7)
    out = [(torch.zeros(B, dtype=torch.float32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)) for _ in range(3)]
    for step in range(30):
        a = torch.from_numpy(rs.randint(0, 4, B).astype(np.int32)).to(DEV)
        for e, (r, t) in zip(envs + [fp], out):
            e.process(a, None, r, t, track_score=True)
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), step
        for name in RING_ARRAYS + CFG_ARRAYS:
            assert torch.equal(getattr(envs[0].ring, name), getattr(envs[1].ring, name)), (step, name)
    assert int(envs[0].ring.episode.max()) >= 1
