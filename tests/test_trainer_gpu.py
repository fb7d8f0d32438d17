"""End-to-end parity (GPU): the batched `Trainer.process()` on HIP kernels vs the CPU oracle running the
reference algorithm actor by actor (oracle/trainer.py, fp64 as arbiter) on the SAME parameters and the
SAME random draws (the device Philox draws are recorded and replayed into the oracle).

Checked per update: per-actor step counts and actions (exact), rewards / terminals (exact), the eight
loss scalars, the mean gradient of every variable, the pre-clip global norm and the parameters after
the RMSProp step.  Tolerances (fp32 kernels vs fp64 oracle) are written at each assert."""
import numpy as np
import pytest
import torch

try:
    import margins
except ImportError:            # imported as tests.<module> (__graft_entry__.smoke): tests/ itself is not on sys.path
    from tests import margins

pytestmark = pytest.mark.gpu

# Bars of the end-to-end comparison (fp32-grade kernels vs the fp64 oracle).  Losses: SURVEY 8d's rel 1e-4 (rounds 1-3:
# 2e-4 abs + 2e-4 rel; the absolute term only guards a loss that is exactly 0).  Gradients: SURVEY names no bar; 2e-5 of
# the variable's largest element (rounds 1-3: 2e-4).  Measured worst |error| / bar over the seven flag sets on MI355X:
# losses 0.06, gradients 0.04 (profiles/r04_parity_margins.md).
LOSS_ATOL, LOSS_RTOL = 1e-6, 1e-4
GRAD_ATOL, GRAD_REL = 1e-6, 2e-5
# host-fed actors (uint8 observations / 255, raw rewards): the same bars (rounds 1-3: 3e-4 / 3e-4; measured on MI355X
# with those: losses <= 0.004 of rel 1e-4, gradients <= 0.007 of 3e-4 of max |g|)
HF_LOSS_ATOL, HF_LOSS_RTOL = LOSS_ATOL, LOSS_RTOL
HF_GRAD_ATOL, HF_GRAD_REL = GRAD_ATOL, GRAD_REL

from oracle import maze as OM
from oracle.trainer import OracleTrainer, ExplicitDraws

DEV = "cuda:0"


class RecordingDraws(object):
    def __init__(self, inner):
        self.inner = inner
        self.log = []

    def uniform(self, out):
        self.inner.uniform(out)
        self.log.append(out.cpu().numpy().copy())
        return out

    def randint(self, high, out):
        self.inner.randint(high, out)
        self.log.append(out.cpu().numpy().copy())
        return out


def _cfg(use_lstm, aux, H, T):
    """aux: True / False for all three auxiliary tasks, or a (pixel_change, value_replay, reward_prediction) triple."""
    pc, vr, rp = (aux, aux, aux) if isinstance(aux, bool) else aux
    return dict(action_size=4, use_lstm=use_lstm, use_pixel_change=pc, use_value_replay=vr,
                use_reward_prediction=rp, pixel_change_lambda=0.05, entropy_beta=0.001, local_t_max=T,
                n_step_TD=T, gamma=0.99, gamma_pc=0.9, experience_history_size=H, max_time_step=10 ** 6,
                rmsp_alpha=0.99, rmsp_epsilon=0.1, grad_norm_clip=40.0, initial_alpha_low=1e-4,
                initial_alpha_high=5e-3, initial_alpha_log_rate=0.5)


def _build(cfg, B, seed, env_type="maze", simulator=None, frame_scale=None, env_name="", groups=1, overlap_host=None,
           rank=0, world_size=1):
    """rank / world_size: the shard the trainer is (tests/sharded_cases.py); the injected draws stay the plain stream."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, PhiloxDraws
    Environment.action_size = -1
    A = Environment.get_action_size(env_type, env_name)
    assert A == cfg["action_size"]
    net = UnrealModel(A, Environment.get_objective_size(env_type, env_name), -1, cfg["use_lstm"], cfg["use_pixel_change"], cfg["use_value_replay"],
                      cfg["use_reward_prediction"], cfg["pixel_change_lambda"], cfg["entropy_beta"], DEV, seed=seed,
                      frame_scale=frame_scale)
    applier = RMSPropApplier(None, decay=cfg["rmsp_alpha"], momentum=0.0, epsilon=cfg["rmsp_epsilon"],
                             clip_norm=cfg["grad_norm_clip"], device=DEV)
    draws = RecordingDraws(PhiloxDraws(0xA3C, 0))
    tr = Trainer(0, net, 7.0711e-4, None, applier, env_type, env_name, cfg["use_lstm"], cfg["use_pixel_change"],
                 cfg["use_value_replay"], cfg["use_reward_prediction"], cfg["pixel_change_lambda"],
                 cfg["entropy_beta"], cfg["local_t_max"], cfg["n_step_TD"], cfg["gamma"], cfg["gamma_pc"],
                 cfg["experience_history_size"], cfg["max_time_step"], DEV, batch_size=B, draws=draws,
                 simulator=simulator, groups=groups, overlap_host=overlap_host, rank=rank, world_size=world_size)
    tr.prepare()
    return net, applier, tr, draws


def _feed_draws(cfg, log, edraws, T, B):
    """Replay one compute_gradients() call's recorded device draws into the oracle's per-actor draw objects.  Order per
    call: T action uniforms, [pixel-control start], [value-replay start], [reward-prediction coin, pick]."""
    u_act = log[0].reshape(T, B)
    k = 1
    for b in range(B):
        edraws[b].action_u = [float(u_act[t, b]) for t in range(T)]
        edraws[b].seq_starts = []
        edraws[b].rp_coin, edraws[b].rp_u = [], []
    for flag in ("use_pixel_change", "use_value_replay"):
        if cfg[flag]:
            for b in range(B):
                edraws[b].seq_starts.append(int(log[k][b]))
            k += 1
    if cfg["use_reward_prediction"]:
        for b in range(B):
            edraws[b].rp_coin = [int(log[k][b])]
            edraws[b].rp_u = [float(log[k + 1][b])]
        k += 2
    assert k == len(log), "the device made %d draw calls, the flag set explains %d" % (len(log), k)


def _teleport(tr, orc, b, x, y):
    """Put actor b at cell (x,y) on both sides (to provoke terminals inside a rollout)."""
    ring = tr.ring
    from unreal_amd import ops
    cnt = int(ring.count.cpu()[b])
    slot = b * ring.H1 + cnt % ring.H1
    img = OM.render(x, y)
    ring.frames[slot * ops.FRAME_BYTES:(slot + 1) * ops.FRAME_BYTES].copy_(
        torch.from_numpy(img.astype(np.uint8).reshape(-1)))
    pos = ring.pos.cpu()
    pos[2 * b], pos[2 * b + 1] = x, y
    ring.pos.copy_(pos)
    env = orc.actors[b].env
    env.x, env.y = x, y
    env.last_state = {'image': img}


# flag sets: full UNREAL, config 1 (FF, no aux), and the partial sets the reference's own tests build
# (model/model_test.py:22-66: PC only = 18 variables, VR only = 12, RP only = 14 with the LSTM on; PC only is also
# BASELINE config 4's flag set).  With exactly one of PC / VR the trainer runs the replay pass with that one lane
# (_train_replay on the one-lane workspaces), with both the two-lane replay pass.
@pytest.mark.parametrize("use_lstm,aux,n_vars", [(True, True, 20), (False, False, 10),
                                                 (True, (True, False, False), 18),
                                                 (True, (False, True, False), 12),
                                                 (True, (False, False, True), 14),
                                                 (True, (True, False, True), 20),
                                                 (False, (True, True, False), 16)])
def test_process_matches_oracle(use_lstm, aux, n_vars):
    B, H, T = 3, 40, 20
    cfg = _cfg(use_lstm, aux, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    net, applier, tr, draws = _build(cfg, B, seed=3)
    assert len(net.get_vars()) == n_vars                      # model/model_test.py:14-58
    assert (tr.replay_width == 2) == (cfg["use_pixel_change"] and cfg["use_value_replay"])
    named = net.export_named()
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in named.items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params)

    # ---- replay fill ------------------------------------------------------------------------------
    calls = 0
    while not tr._full:
        d, s = tr.process(None, 0)
        assert (d, s) == (0, None)
        calls += 1
    assert calls == H
    assert len(draws.log) == H
    for step_u in draws.log:
        for b in range(B):
            edraws[b].action_u.append(float(step_u[b]))
    orc.fill()
    assert all(len(e.action_u) == 0 for e in edraws)
    np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
    for b in range(B):
        a = orc.actors[b]
        assert tuple(tr.ring.pos.cpu().numpy()[2 * b:2 * b + 2]) == (a.env.x, a.env.y) == OM.START

    global_t = 0
    for it in range(4):
        if it == 1:
            _teleport(tr, orc, 0, 5, 0)      # one RIGHT from the goal
            _teleport(tr, orc, 1, 4, 0)
        draws.log.clear()
        lr = tr._anneal_learning_rate(global_t)
        tr.compute_gradients()
        g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
        tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
        norm_dev = float(tr.last_grad_norm.cpu()[0])
        tr.stats.zero_()
        from unreal_amd import ops
        ops.rollout_stats(B, tr.n_steps, tr.ring.score_valid, tr.ring.score_out, tr.stats)
        steps_dev, episodes_dev, score_dev = tr.read_stats()
        losses_dev = tr._publish_losses()

        # replay the draws into the oracle
        _feed_draws(cfg, draws.log, edraws, T, B)
        steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(global_t)

        # ---- exact: step counts, actions, rewards, terminals ------------------------------------
        n_dev = tr.n_steps.cpu().numpy()
        acts = tr.actions.cpu().numpy().reshape(T, B)
        rews = tr.rewards.cpu().numpy().reshape(T, B)
        assert steps_dev == steps_o == int(n_dev.sum())
        for b in range(B):
            n = infos[b]["n"]
            assert n_dev[b] == n
            assert list(acts[:n, b]) == infos[b]["actions"]
            assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]]
            assert bool(tr.terminal_end.cpu()[b]) == infos[b]["terminal_end"]
        sc = [i["score"] for i in infos if i["score"] is not None]
        assert episodes_dev == len(sc)
        if sc:
            assert abs(score_dev - sum(sc)) < 1e-6
        if it == 1:
            assert episodes_dev >= 1, "teleported actors should finish an episode (ragged rollout is covered)"

        # ---- losses: mean over actors of the per-actor sums; SURVEY 8d: rel 1e-4 --------------------
        for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
            if key in losses_o[0]:
                want = np.mean([l[key] for l in losses_o])
                margins.record(key, abs(losses_dev[key] - want) / (LOSS_ATOL + LOSS_RTOL * abs(want)),
                               "%g abs + %g rel" % (LOSS_ATOL, LOSS_RTOL), abs(losses_dev[key] - want) / (1e-4 * abs(want) + 1e-30))
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            else:
                assert losses_dev[key] == 0.0, (key, losses_dev[key])          # a task that is off contributes nothing
        want_ent = np.mean([l["entropy"].sum() for l in losses_o])
        margins.record("entropy", abs(losses_dev["entropy"] - want_ent) / (LOSS_ATOL + LOSS_RTOL * abs(want_ent)),
                       "%g abs + %g rel" % (LOSS_ATOL, LOSS_RTOL), abs(losses_dev["entropy"] - want_ent) / (1e-4 * abs(want_ent) + 1e-30))
        assert abs(losses_dev["entropy"] - want_ent) <= LOSS_ATOL + LOSS_RTOL * abs(want_ent)

        # ---- gradients: per variable, |d| <= 1e-6 + 2e-5 * max|g_ref| ---------------------------
        for (name, _), gref in zip(orc.params.items(), mean_g):
            gr = gref.numpy().reshape(-1)
            gd = g_dev[name]
            tol = GRAD_ATOL + GRAD_REL * np.abs(gr).max()
            margins.record("g[%s]" % name, np.abs(gd - gr).max() / tol, "%g + %g of max |g|" % (GRAD_ATOL, GRAD_REL))
            assert np.abs(gd - gr).max() <= tol, (it, name, np.abs(gd - gr).max(), np.abs(gr).max())
        margins.record("grad norm", abs(norm_dev - norm_o) / (1e-4 * max(1.0, norm_o)), "1e-4 rel")
        assert abs(norm_dev - norm_o) <= 1e-4 * max(1.0, norm_o), (norm_dev, norm_o)

        # ---- parameters after the update: |d| <= 2e-6 + 1e-5 rel --------------------------------
        for name, ref in orc.params.items():
            got = net.p[name].cpu().double().numpy()
            want = ref.numpy().reshape(-1)
            margins.record("param %s after RMSProp" % name, np.abs(got - want).max() / (2e-6 + 1e-5 * np.abs(want).max()),
                           "2e-6 + 1e-5 of max |p|")
            assert np.abs(got - want).max() <= 2e-6 + 1e-5 * np.abs(want).max(), (it, name)
        global_t += steps_dev
    assert all(len(e.seq_starts) == 0 and len(e.rp_u) == 0 for e in edraws)


def test_grouped_process_is_the_reference_algorithm_actor_after_actor():
    """groups = B: one process() call = B sequential single-actor passes, each with its own clip + RMSProp step on the
    weights the previous actor left -- the reference's algorithm (trainer.py:438-636) executed thread after thread
    (oracle: process_async in actor order; hogwild order = call order).  Checked after every call: step counts /
    actions exact, parameters <= 2e-6 + 2e-5 rel (3 chained updates per call)."""
    B, H, T = 3, 40, 20
    cfg = _cfg(True, True, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    net, applier, tr, draws = _build(cfg, B, seed=13, groups=B)
    assert tr.Bg == 1 and tr.grad_scale == 1.0
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params)
    while not tr._full:
        assert tr.process(None, 0) == (0, None)
    assert len(draws.log) == H * B                       # one draw call per group and fill step
    for k, u in enumerate(draws.log):
        edraws[k % B].action_u.append(float(u[0]))
    orc.fill()
    np.testing.assert_array_equal(tr.full_ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
    global_t = 0
    for it in range(3):
        if it == 1:
            tr._select_group(0)
            _teleport(tr, orc, 0, 5, 0)                  # actor 0 finishes an episode inside this call
        draws.log.clear()
        steps_dev, score_dev = tr.process(None, global_t)
        assert len(draws.log) == 5 * B
        steps_o, scores = 0, []
        for b in range(B):
            lg = draws.log[5 * b:5 * b + 5]
            edraws[b].action_u = [float(x) for x in lg[0]]
            edraws[b].seq_starts = [int(lg[1][0]), int(lg[2][0])]
            edraws[b].rp_coin, edraws[b].rp_u = [int(lg[3][0])], [float(lg[4][0])]
            d, sc, losses = orc.process_async(b, global_t + b * T)
            steps_o += d
            if sc is not None:
                scores.append(sc)
            edraws[b].action_u = []                      # a terminal leaves unused uniforms behind
        assert steps_dev == steps_o
        assert (score_dev is None) == (not scores)
        if scores:
            assert abs(score_dev - np.mean(scores)) < 1e-6 and it == 1
        for name, ref in orc.params.items():
            got = net.p[name].cpu().double().numpy()
            want = ref.numpy().reshape(-1)
            assert np.abs(got - want).max() <= 2e-6 + 2e-5 * np.abs(want).max(), (it, name)
        global_t += steps_dev
    # the last group's losses are the last actor's; the published ones are the mean over the call's updates
    assert np.isfinite(tr.last_losses["total_loss"])


def test_batch1_runners_match_oracle():
    """Reference-shaped batch-1 entry points (model.py:630-728) against the oracle network."""
    from oracle import model as M
    cfg = _cfg(True, True, 40, 20)
    net, applier, tr, draws = _build(cfg, 2, seed=5)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    env = OM.OracleMaze()
    rs = np.random.RandomState(0)
    state = (torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float64))
    net.reset_state()
    for step in range(3):
        lar = np.zeros(5)
        lar[env.last_action] = 1.0
        lar[4] = env.last_reward
        x = torch.tensor(env.last_state['image']).unsqueeze(0)
        tl = torch.tensor(lar).unsqueeze(0)
        feat, st = M.trunk(x, tl, p, True, state)
        pi_o, v_o = M.policy_value(feat, p)
        v_only = net.run_base_value(None, env.last_state, lar)
        pi, v, _ = net.run_base_policy_and_value(None, env.last_state, lar)
        np.testing.assert_allclose(pi, pi_o[0].numpy(), atol=2e-6, rtol=1e-5)
        margins.record("batch-1 V", max(abs(v - float(v_o[0])), abs(v_only - float(v_o[0]))) / 1e-5, "1e-5 abs")
        assert abs(v - float(v_o[0])) < 1e-5 and abs(v_only - float(v_o[0])) < 1e-5
        fz, _ = M.trunk(x, tl, p, True, None)
        _, qm = M.pc_head(fz, p)
        np.testing.assert_allclose(net.run_pc_q_max(None, env.last_state, lar), qm[0].numpy(), atol=1e-5, rtol=1e-5)
        _, vz = M.policy_value(fz, p)
        assert abs(net.run_vr_value(None, env.last_state, lar) - float(vz[0])) < 1e-5
        state = st
        env.process(int(rs.randint(4)))
    hist = [{'image': OM.render(0, 2)}, {'image': OM.render(1, 2)}, {'image': OM.render(1, 3)}]
    rp_o = M.rp_head(torch.tensor(np.stack([h['image'] for h in hist])), p)
    np.testing.assert_allclose(net.run_rp_c(None, hist), rp_o[0].numpy(), atol=2e-6, rtol=1e-5)


def test_maze_environment_reference_surface():
    """The reference's own environment test (environment/environment_test.py:36-54) with the documented
    adapter (last_state is a dict with 'image')."""
    from unreal_amd.environment.environment import Environment
    Environment.action_size = -1
    env = Environment.create_environment("maze", "")
    assert Environment.get_action_size("maze", "") == 4
    ref = OM.OracleMaze()
    for a in (0, 0, 0, 3, 1, 1):
        state, reward, terminal, pc = env.process(a)
        _, r2, t2, pc2 = ref.process(a)
        assert state.shape == (84, 84, 3) and env.last_state['image'].shape == (84, 84, 3)
        assert pc.shape == (20, 20)
        assert 0.0 <= state.min() and state.max() <= 1.0 and 0.0 <= pc.min() and pc.max() <= 1.0
        np.testing.assert_array_equal(state, ref.last_state['image'])
        np.testing.assert_array_equal(pc, pc2.astype(np.float32))
        assert (reward, terminal) == (r2, t2)
    env.stop()


def _hostfed_parity(cfg, B, H, T, tr, net, applier, draws, orc, edraws, check_frame, iters=3):
    """Fill the replay on both sides with the recorded draws, compare the ring, then `iters` updates: per-actor actions /
    rewards / step counts, mean losses, mean gradient of every variable, global norm."""
    from unreal_amd import ops
    while not tr._full:
        assert tr.process(None, 0) == (0, None)
    assert len(draws.log) == H
    for step_u in draws.log:
        for b in range(B):
            edraws[b].action_u.append(float(step_u[b]))
    orc.fill()
    np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
    # ring contents after the fill: frames, rewards, terminals, pixel change (+ whatever check_frame adds)
    H1 = H + 1
    fr = tr.ring.frames.cpu().numpy().reshape(B, H1, 84, 84, 3)
    rr = tr.ring.r_reward.cpu().numpy().reshape(B, H1)
    rt = tr.ring.r_terminal.cpu().numpy().reshape(B, H1)
    rpc = tr.ring.r_pc.cpu().numpy().reshape(B, H1, 20, 20)
    for b in range(B):
        x = orc.actors[b].exp
        for i in range(x.top, x.count):
            f = x.frames[i]
            np.testing.assert_array_equal(fr[b, i % H1], np.rint(f.state['image'] * 255.0).astype(np.uint8))
            assert rr[b, i % H1] == f.reward and bool(rt[b, i % H1]) == bool(f.terminal)
            # reference: float32 arithmetic on obs/255; kernel: exact integer SAD / (48*255) -> 1e-6 relative
            np.testing.assert_allclose(rpc[b, i % H1], f.pixel_change, rtol=2e-6, atol=1e-7)
            if check_frame is not None:
                check_frame(b, i % H1, f)
    global_t = 0
    for it in range(iters):
        draws.log.clear()
        lr = tr._anneal_learning_rate(global_t)
        tr.compute_gradients()
        g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
        tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
        norm_dev = float(tr.last_grad_norm.cpu()[0])
        tr.stats.zero_()
        ops.rollout_stats(B, tr.n_steps, tr.ring.score_valid, tr.ring.score_out, tr.stats)
        steps_dev, episodes_dev, score_dev = tr.read_stats()
        losses_dev = tr._publish_losses()
        _feed_draws(cfg, draws.log, edraws, T, B)
        steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(global_t)
        n_dev = tr.n_steps.cpu().numpy()
        acts = tr.actions.cpu().numpy().reshape(T, B)
        rews = tr.rewards.cpu().numpy().reshape(T, B)
        assert steps_dev == steps_o
        for b in range(B):
            n = infos[b]["n"]
            assert n_dev[b] == n and list(acts[:n, b]) == infos[b]["actions"]
            assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]]      # raw (unclipped) rewards
        sc = [i["score"] for i in infos if i["score"] is not None]
        assert episodes_dev == len(sc) and (not sc or abs(score_dev - sum(sc)) < 1e-5)
        for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
            if key not in losses_o[0]:
                assert losses_dev[key] == 0.0
                continue
            want = np.mean([l[key] for l in losses_o])
            margins.record("host-fed " + key, abs(losses_dev[key] - want) / (HF_LOSS_ATOL + HF_LOSS_RTOL * abs(want)),
                           "%g abs + %g rel" % (HF_LOSS_ATOL, HF_LOSS_RTOL), abs(losses_dev[key] - want) / (1e-4 * abs(want) + 1e-30))
            assert abs(losses_dev[key] - want) <= HF_LOSS_ATOL + HF_LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
        for (name, _), gref in zip(orc.params.items(), mean_g):
            gr = gref.numpy().reshape(-1)
            tol = HF_GRAD_ATOL + HF_GRAD_REL * np.abs(gr).max()
            margins.record("host-fed g[%s]" % name, np.abs(g_dev[name] - gr).max() / tol, "%g + %g of max |g|" % (HF_GRAD_ATOL, HF_GRAD_REL))
            assert np.abs(g_dev[name] - gr).max() <= tol, (it, name, np.abs(g_dev[name] - gr).max(), np.abs(gr).max())
        margins.record("host-fed grad norm", abs(norm_dev - norm_o) / (2e-4 * max(1.0, norm_o)), "2e-4 rel")
        assert abs(norm_dev - norm_o) <= 2e-4 * max(1.0, norm_o)
        global_t += steps_dev


# B = 4: two half-batches alternate between host and device (overlap_host).  aux (False, ...) = BASELINE config 4's own
# flag set, "A3C-LSTM + pixel-control": no value replay, no reward prediction -> the one-lane replay pass (_train_replay)
@pytest.mark.parametrize("B,aux", [(3, True), (4, True), (3, (True, False, False)), (4, (True, False, False))])
def test_hostfed_lab_contract_matches_oracle(B, aux):
    """SURVEY 8f-1 / BASELINE config 4: host simulators (synthetic stand-in for DeepMind Lab: uint8 frames, A = 6,
    sparse rewards incl. values > 1, fixed-length episodes) -> pinned staging -> HBM ring -> the same batched
    learner, against the oracle running the Lab wrapper contract (lab_environment.py:78-119) with the upstream
    replay semantics (experience_lab_ver.py) actor by actor.  Parity unpinned by the reference (no Lab fixtures)."""
    from oracle.hostfed import OracleLabEnv
    from unreal_amd.environment.synthetic_sim import SyntheticBatchSimulator, SyntheticActorSim
    H, T = 40, 20
    cfg = _cfg(True, aux, H, T)
    cfg.update(action_size=6, lab_ver=True, initial_learning_rate=7.0711e-4)
    kw = dict(episode_len=23, reward_p=0.2, big_reward_p=0.06)
    sim = SyntheticBatchSimulator(B, seed=4, **kw)
    net, applier, tr, draws = _build(cfg, B, seed=9, env_type="lab", simulator=sim, frame_scale=1.0 / 255.0,
                                     overlap_host=(B % 2 == 0))
    assert tr.overlap_host == (B % 2 == 0)
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    envs = [OracleLabEnv(SyntheticActorSim(4 * 100003 + b, **kw), 6) for b in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=envs)
    _hostfed_parity(cfg, B, H, T, tr, net, applier, draws, orc, edraws, None)
    # the simulator did emit rewards above 1 and the replay holds them clipped (experience_lab_ver.py:14,18)
    assert all(abs(f.last_reward) <= 1 and abs(f.reward) <= 1 for a in orc.actors for f in a.exp.frames.values())
    assert float(tr.ring.r_reward.abs().max()) <= 1.0


@pytest.mark.parametrize("B", [3, 4])
def test_hostfed_indoor_objective_matches_oracle(B):
    """SURVEY 8f-4 / BASELINE config 5: the multimodal MINOS contract (indoor_environment.py:63-139): A = 3, every
    observation carries a measurement vector ('objective') that is stored beside the frame and concatenated into the
    LSTM input (experience.py:42-44, model.py:144,343; the bootstrap value gets the PREVIOUS state's objective,
    trainer.py:300); rewards are divided by termination_time and not clipped; this fork's replay buckets.  Synthetic
    simulator (MINOS is not in the image): parity unpinned by the reference, checked against the oracle."""
    from oracle.hostfed import OracleIndoorEnv
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.synthetic_sim import SyntheticBatchIndoorSimulator, SyntheticIndoorSim
    H, T, OBJ = 40, 20, 5
    cfg = _cfg(True, True, H, T)
    cfg.update(action_size=3, objective_size=OBJ, initial_learning_rate=7.0711e-4)
    kw = dict(episode_len=23, reward_p=0.15, big_reward_p=0.05, objective_size=OBJ, termination_time=50.0)
    Environment.register_indoor_config("synthetic_rooms", OBJ)
    sim = SyntheticBatchIndoorSimulator(B, seed=5, **kw)
    net, applier, tr, draws = _build(cfg, B, seed=11, env_type="indoor", env_name="synthetic_rooms", simulator=sim,
                                     frame_scale=1.0 / 255.0, overlap_host=(B % 2 == 0))
    assert net.K_x == 256 + 3 + 1 + OBJ and net.params.shaped("lstm_kernel").shape == (net.K_x + 256, 1024)
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    envs = [OracleIndoorEnv(SyntheticIndoorSim(5 * 100003 + b, **kw), 50.0) for b in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=envs)
    robj = [None]

    def check_objective(b, slot, f):
        if robj[0] is None:
            robj[0] = tr.ring.r_objective.cpu().numpy().reshape(B, H + 1, OBJ)
        np.testing.assert_array_equal(robj[0][b, slot], f.state['objective'].astype(np.float32))

    _hostfed_parity(cfg, B, H, T, tr, net, applier, draws, orc, edraws, check_objective)
    rews = [f.reward for a in orc.actors for f in a.exp.frames.values()]
    assert min(rews) < 0 < max(rews) and max(abs(r) for r in rews) <= 0.5       # scaled by 1/termination_time
    # the objective rows of the LSTM kernel received gradient
    g = net.grads.shaped("lstm_kernel")[256 + 4:256 + 4 + OBJ]
    assert float(g.abs().max()) > 0


def test_config1_long_horizon_drift_is_fp32_grade():
    """SURVEY 8(d) asks that config 1's per-update losses track the restatement over a long run on identical draws.
    120 consecutive updates of maze / FF / no aux / one actor: the device, the oracle in fp32 (the "CPU restatement") and
    the oracle in fp64 (the arbiter) consume the SAME recorded Philox draws.  Trajectories (step counts, actions) must be
    identical throughout; the device's distance from the fp64 arbiter -- losses and parameters -- must stay within a small
    factor of the fp32 restatement's own distance from it (rounding differences are amplified by the training dynamics
    alike for both: ~1e-2 relative on a loss near zero after 100 updates, measured with tools/exp/long_parity.py)."""
    N, B, H, T = 120, 1, 30, 20
    cfg = _cfg(False, False, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    net, applier, tr, draws = _build(cfg, B, seed=3)
    named = net.export_named()
    orcs, eds = {}, {}
    for dt in (torch.float32, torch.float64):
        eds[dt] = [ExplicitDraws()]
        orcs[dt] = OracleTrainer(cfg, n_actors=B, draws=eds[dt], dtype=dt,
                                 params={k: torch.tensor(v, dtype=dt) for k, v in named.items()})
    while not tr._full:
        tr.process(None, 0)
    for dt in orcs:
        eds[dt][0].action_u = [float(u[0]) for u in draws.log]
        orcs[dt].fill()
    g_t = 0
    keys = ("policy_loss", "value_loss")
    worst_dev = worst_o32 = 0.0
    for it in range(N):
        draws.log.clear()
        steps, _ = tr.process(None, g_t)
        ld = tr.last_losses
        out = {}
        for dt in orcs:
            eds[dt][0].action_u = [float(x) for x in draws.log[0].reshape(-1)]
            out[dt] = orcs[dt].process_batched(g_t)
        s64, i64, l64 = out[torch.float64][0], out[torch.float64][1][0], out[torch.float64][2][0]
        s32, i32 = out[torch.float32][0], out[torch.float32][1][0]
        acts = list(tr.actions.cpu().numpy().reshape(-1)[:i64["n"]])
        assert steps == s64 and acts == i64["actions"], "update %d: device trajectory left the arbiter's" % it
        assert s32 == s64 and i32["actions"] == i64["actions"], "update %d: fp32 restatement left the arbiter's" % it
        l32 = out[torch.float32][2][0]
        d_dev = max(abs(ld[k] - float(l64[k])) / (1.0 + abs(float(l64[k]))) for k in keys)
        d_o32 = max(abs(float(l32[k]) - float(l64[k])) / (1.0 + abs(float(l64[k]))) for k in keys)
        p64 = {n: r.double().numpy().reshape(-1) for n, r in orcs[torch.float64].params.items()}
        pd_dev = max(float(np.abs(net.p[n].cpu().double().numpy() - p64[n]).max()) for n in p64)
        pd_o32 = max(float(np.abs(r.double().numpy().reshape(-1) - p64[n]).max()) for n, r in orcs[torch.float32].params.items())
        worst_dev, worst_o32 = max(worst_dev, d_dev), max(worst_o32, d_o32)
        assert d_dev <= 4.0 * max(worst_o32, 2e-6) + 1e-6, (it, d_dev, d_o32, worst_o32)
        assert pd_dev <= 4.0 * max(pd_o32, 1e-7) + 1e-7, (it, pd_dev, pd_o32)
        g_t += steps
    assert worst_dev < 5e-2


@pytest.mark.parametrize("use_lstm,groups", [(True, 1), (False, 1), (True, 2)])
def test_half_batch_rollout_on_two_streams_is_the_lockstep_rollout(use_lstm, groups, monkeypatch):
    """Trainer._rollout_steps_split (maze actors: the T rollout steps as two half-batches on their own HIP streams) runs the
    same kernels on the same rows with the same draws as the lock-step loop: after the replay fill and three updates,
    every rollout product (actions, rewards, terminals, step counts, frame indices, pi, V, carried LSTM state) is
    IDENTICAL, and losses / parameters agree to the last bits (a half's GEMMs may run under the running maximum of its
    own rows instead of all actors': the same power-of-two scale unless the two straddle a binade)."""
    from unreal_amd.train.trainer import Trainer
    B, H, T = 64, 40, 20
    cfg = _cfg(use_lstm, True, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    out = []
    for parts in (0, 2):
        monkeypatch.setattr(Trainer, "rollout_parts_default", parts)
        monkeypatch.setattr(Trainer, "ROLLOUT_SPLIT_MIN_ACTORS", 2)
        net, applier, tr, draws = _build(cfg, B, seed=5, groups=groups)
        assert (tr._split is not None) == (parts == 2)
        while not tr._full:
            tr.process(None, 0)
        g = 0
        snaps = []
        for it in range(3):
            steps, _ = tr.process(None, g)
            g += steps
            snaps.append(dict(actions=tr.actions.cpu().numpy().copy(), rewards=tr.rewards.cpu().numpy().copy(),
                              terminals=tr.terminals.cpu().numpy().copy(), n_steps=tr.n_steps.cpu().numpy().copy(),
                              idx=tr.base_ws.frame_idx.cpu().numpy().copy(), pi=tr.pi.cpu().numpy().copy(),
                              v=tr.v.cpu().numpy().copy(), c=tr.full_lstm_c.cpu().numpy().copy(),
                              steps=steps, losses=dict(tr.last_losses), params=net.params.flat.cpu().numpy().copy()))
        out.append(snaps)
    for a, b in zip(*out):
        for k in ("actions", "rewards", "terminals", "n_steps", "idx"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert a["steps"] == b["steps"]
        for k in ("pi", "v", "c"):
            np.testing.assert_allclose(b[k], a[k], rtol=2e-6, atol=2e-7, err_msg=k)
        for k in ("total_loss", "pc_loss", "vr_loss", "rp_loss", "grad_norm"):
            assert abs(a["losses"][k] - b["losses"][k]) <= 1e-5 * max(1.0, abs(a["losses"][k])), k
        np.testing.assert_allclose(b["params"], a["params"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("batch_aux", [True, False])
def test_one_launch_pixel_control_pass_is_the_two_launch_pass(batch_aux, monkeypatch):
    """Trainer.fuse_pc_deconv (unreal_pc_deconv_train: loss + backward of the pixel-control deconvolutions in one launch,
    d_dec on chip under per-frame scales) against the two-launch form (unreal_pc_deconv_fwd + unreal_pc_deconv_bwd, one
    scale per launch) through whole process() calls, batched and per-branch replay schedule: same rollouts and samples;
    the first update's losses and gradient agree at the parity bars (the two differ in the rounding of d_dec's lo planes
    only), parameters after three updates to 1e-5."""
    from unreal_amd.train.trainer import Trainer
    B, H, T = 32, 40, 20
    cfg = _cfg(True, True, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    out = []
    for fused in (True, False):
        monkeypatch.setattr(Trainer, "fuse_pc_deconv", fused)
        monkeypatch.setattr(Trainer, "batch_aux_default", batch_aux)
        net, applier, tr, draws = _build(cfg, B, seed=11)
        assert (tr.replay_width == 2) == batch_aux
        while not tr._full:
            tr.process(None, 0)
        g, snaps = 0, []
        for it in range(3):
            steps, _ = tr.process(None, g)
            g += steps
            snaps.append(dict(actions=tr.actions.cpu().numpy().copy(), losses=dict(tr.last_losses),
                              grads=net.grads.flat.cpu().numpy().copy(), params=net.params.flat.cpu().numpy().copy()))
        assert (tr.replay[tr.replay_width].gws.d_dec is None) == fused
        out.append(snaps)
    a, b = out[0][0], out[1][0]
    np.testing.assert_array_equal(a["actions"], b["actions"])
    for k in ("total_loss", "pc_loss", "grad_norm"):
        assert abs(a["losses"][k] - b["losses"][k]) <= LOSS_ATOL + LOSS_RTOL * abs(b["losses"][k]), k
    gmax = float(np.abs(b["grads"]).max())
    d = float(np.abs(a["grads"] - b["grads"]).max())
    margins.record("one-launch vs two-launch pixel-control pass: max |d grad| / max |grad| (batch_aux=%s)" % batch_aux,
                   d / (GRAD_ATOL + GRAD_REL * gmax), "%g + %g rel" % (GRAD_ATOL, GRAD_REL))
    assert d <= GRAD_ATOL + GRAD_REL * gmax, (d, gmax)
    np.testing.assert_allclose(out[0][2]["params"], out[1][2]["params"], rtol=1e-5, atol=1e-6)


def test_few_rows_fc_slabs_is_the_one_launch_fc(monkeypatch):
    """UnrealModel.fc_few_rows_slabs (the fc product of <= 1024-row launches as K slabs + ordered sum) against the one-launch
    kernel through whole grouped process() calls (B = 64, G = 8: 8-row rollout steps, 160 / 320-row replay passes): identical
    rollouts (actions, rewards, step counts), losses and gradient at the parity bars, parameters after three updates to 1e-5."""
    from unreal_amd.model.model import UnrealModel
    B, H, T = 64, 40, 20
    cfg = _cfg(True, True, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    out = []
    for slabs in (True, False):
        monkeypatch.setattr(UnrealModel, "fc_few_rows_slabs", slabs)
        net, applier, tr, draws = _build(cfg, B, seed=13, groups=8)
        while not tr._full:
            tr.process(None, 0)
        g, snaps = 0, []
        for it in range(3):
            steps, _ = tr.process(None, g)
            g += steps
            snaps.append(dict(actions=tr.actions.cpu().numpy().copy(), rewards=tr.rewards.cpu().numpy().copy(), steps=steps,
                              losses=dict(tr.last_losses), params=net.params.flat.cpu().numpy().copy()))
        out.append(snaps)
    a, b = out[0][0], out[1][0]
    np.testing.assert_array_equal(a["actions"], b["actions"])
    np.testing.assert_array_equal(a["rewards"], b["rewards"])
    assert a["steps"] == b["steps"]
    for k in ("total_loss", "pc_loss", "vr_loss", "rp_loss", "grad_norm"):
        assert abs(a["losses"][k] - b["losses"][k]) <= LOSS_ATOL + LOSS_RTOL * abs(b["losses"][k]), k
    np.testing.assert_allclose(out[0][2]["params"], out[1][2]["params"], rtol=1e-5, atol=1e-6)
