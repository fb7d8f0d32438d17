"""unreal_maze_policy_rollout_step_encode (csrc/rollout_fused.hip): the maze step and the conv encoder of the next
observation in one launch, against the two launches it replaces -- unreal_maze_policy_rollout_step, then unreal_encoder_fwd
with the prepared block on next_idx -- from the same start state, BITWISE: ring, per-actor state, rollout outputs and
bookkeeping, f2, saved conv1, ReLU bits and both absmax slots (maxima do not depend on the order)."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
try:
    from test_trainer_gpu import _cfg, _build
except ImportError:
    from tests.test_trainer_gpu import _cfg, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC, A, XLD = 21168, 400, 4, 264
RING_ARRAYS = ("frames", "r_reward", "r_action", "r_terminal", "r_last_action", "r_last_reward", "r_pc", "pos", "count",
               "last_action", "last_reward", "episode_reward", "score_out", "score_valid")
CFG_ARRAYS = ("goal", "layout", "ep_steps", "episode")
REFERENCE_MAP = ["--+---G", "--+-+++", "S-+---+", "--+++--", "--+-+--", "--+----", "-----++"]


def _env(B, H, config=None, seed=0):
    from unreal_amd.environment.maze_environment import BatchedMazeEnvironment
    env = BatchedMazeEnvironment(B, H, DEV, config=config, seed=seed)
    env.ring.frames.zero_()           # (torch.empty: slots no step has written would hold stale allocator bytes)
    env.ring.r_pc.zero_()
    env.reset()
    return env


def _dev(a, dt):
    return torch.from_numpy(np.asarray(a)).to(DEV, dt)


class Pair(object):
    """Two environments in the same state, the heads' and the encoder's weights, and the outputs of both routes."""

    def __init__(self, B, H, config=None, seed=3):
        from unreal_amd import ops
        self.B, self.ops = B, ops
        rs = self.rs = np.random.RandomState(B + 7 * H)
        # logits = 40 * X[:, :4] + noise: a row with X[a] = 1 draws action a whatever u is
        wp = rs.uniform(-.3, .3, (256, A))
        wp[:A] = 0.0
        wp[:A] += 40.0 * np.eye(A)
        self.Wp = _dev(wp.reshape(-1), torch.float32); self.bp = _dev(rs.uniform(-.1, .1, A), torch.float32)
        self.Wv = _dev(rs.uniform(-.3, .3, 256), torch.float32); self.bv = _dev(rs.uniform(-.1, .1, 1), torch.float32)
        self.W1 = _dev(rs.uniform(-.07, .07, 3072), torch.float32); self.b1 = _dev(rs.uniform(-.07, .07, 16), torch.float32)
        self.W2 = _dev(rs.uniform(-.06, .06, 8192), torch.float32); self.b2 = _dev(rs.uniform(-.06, .06, 32), torch.float32)
        self.scale = 1.0
        self.prep = ops.encoder_prepare(self.W1, self.b1, self.W2, self.scale)
        self.envs = [_env(B, H, config, seed), _env(B, H, config, seed)]
        self.templates = ops.maze_wall_templates(self.envs[1].maze, 1 if config is None else config.L, DEV)
        z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
        f = torch.float32
        self.st = [dict(active=torch.ones(B, dtype=torch.int32, device=DEV), log=z(B), n=z(B), te=z(B), r=z(B, f), t=z(B),
                        a=z(B), pi=z(B * A, f), v=z(B, f), idx=z(B), lar=z(B * XLD, f), f2=z(B * 2592, f),
                        c1=z(B * 6400, f), bits=z(B * 162, torch.int16), s_f2=z(1, f), s_c1=z(1, f)) for _ in self.envs]

    def set_state(self, pos=None, goal=None, active=None):
        for e, s in zip(self.envs, self.st):
            if pos is not None:
                e.ring.pos.copy_(_dev(np.asarray(pos).reshape(-1), torch.int32))
            if goal is not None:
                e.ring.goal.copy_(_dev(np.asarray(goal).reshape(-1), torch.int32))
            if active is not None:
                s["active"].copy_(_dev(active, torch.int32))

    def step(self, actions=None):
        """One rollout step on both routes (`actions`: forced through the feature rows; None: drawn) and the comparison."""
        ops, B, rs = self.ops, self.B, self.rs
        x = rs.uniform(-1, 1, (B, 256))
        x[:, :A] = 0.0
        if actions is not None:
            x[np.arange(B), np.asarray(actions)] = 1.0
        X = _dev(x, torch.float32).view(-1)
        u = _dev(rs.uniform(0, 1, B), torch.float64)
        (e0, e1), (s0, s1) = self.envs, self.st
        heads = (X, 256, self.Wp, self.bp, self.Wv, self.bv, u)
        nxt = dict(lar_ld=XLD, lar_col0=256, A=A)
        ops.maze_policy_rollout_step(e0.ring, *heads, s0["pi"], s0["v"], s0["a"], s0["r"], s0["t"], s0["active"], s0["log"],
                                     s0["n"], s0["te"], next_idx=s0["idx"], next_lar=s0["lar"], maze=e0.maze, **nxt)
        ops.encoder_fwd(e0.ring.frames, s0["idx"], self.scale, self.W1, self.b1, self.W2, self.b2, s0["f2"], s0["c1"],
                        relu_bits=s0["bits"], f2_max=s0["s_f2"], c1_max=s0["s_c1"], prepared=self.prep)
        ops.maze_policy_rollout_step_encode(e1.ring, *heads, s1["pi"], s1["v"], s1["a"], s1["r"], s1["t"], s1["active"],
                                            s1["log"], s1["n"], s1["te"], self.templates, self.scale, self.W1, self.b1,
                                            self.W2, self.b2, s1["f2"], s1["c1"], s1["bits"], self.prep, f2_max=s1["s_f2"],
                                            c1_max=s1["s_c1"], next_idx=s1["idx"], next_lar=s1["lar"], maze=e1.maze, **nxt)
        if actions is not None:
            np.testing.assert_array_equal(s0["a"].cpu().numpy(), actions)
        for k in s0:
            assert torch.equal(s0[k], s1[k]), k
        names = RING_ARRAYS + (CFG_ARRAYS if e0.maze is not None else ())
        for name in names:
            assert torch.equal(getattr(e0.ring, name), getattr(e1.ring, name)), name
        # (the slots keep the running maximum over the steps)
        assert float(s1["s_f2"]) >= float(s1["f2"].max()) > 0 and float(s1["s_c1"]) >= float(s1["c1"].max()) > 0


@pytest.mark.parametrize("B", [1, 3, 8, 9, 17])
def test_step_and_encode_is_the_two_launches_on_the_reference_map(B):
    """A partial workgroup, one full, one full + one partial; history 6 with 8 steps, so the ring wraps.  Step 0 is
    forced: actor 0 stands next to the goal and walks into it (terminal, reset to the start cell), actor 1 walks into the
    border, actor 2 into a wall; the last actor of B > 3 is idle throughout.  (Actors a terminal has idled run again
    from the next step on: every step here is the first of a rollout.)"""
    p = Pair(B, 6)
    pos = np.tile([0, 2], (B, 1))
    act = np.full(B, 1, dtype=np.int32)
    pos[0] = (5, 0); act[0] = 3                     # (6, 0) is G
    if B > 1:
        pos[1] = (0, 0); act[1] = 2                 # the border
    if B > 2:
        pos[2] = (1, 0); act[2] = 3                 # (2, 0) is a wall
    active = np.ones(B, dtype=np.int32)
    if B > 3:
        active[B - 1] = 0
    p.set_state(pos=pos, active=active)
    p.step(act)
    s = p.st[1]
    assert int(s["t"][0]) == 1 and float(s["r"][0]) == 1.0 and int(s["te"][0]) == 1 and int(s["active"][0]) == 0
    assert p.envs[1].ring.pos[:2].tolist() == [0, 2]             # reset: the start cell
    if B > 2:
        assert float(s["r"][1]) == -1.0 and float(s["r"][2]) == -1.0 and p.envs[1].ring.pos[2:6].tolist() == [0, 0, 1, 0]
    if B > 3:
        assert int(s["log"][B - 1]) == 0 and int(s["n"][B - 1]) == 0
    for step in range(7):
        p.set_state(active=active)
        p.step()
    assert int(p.envs[1].ring.count.max()) > p.envs[1].ring.H1 == 7


@pytest.mark.parametrize("N,show_goal", [(7, True), (7, False), (12, True), (14, False), (14, True), (21, True), (21, False)])
def test_step_and_encode_on_a_configured_maze(N, show_goal):
    """Every grid size the step kernel is built for: two layouts whose boundary falls inside a workgroup, random start and
    goal cells, the goal block shown or not, a step limit of 3 reached inside the 8 steps (time-outs, resets and new
    goal / start cells), the ring wrapping, and an idle actor."""
    from unreal_amd.environment.maze_environment import MazeConfig
    B = 17
    rs = np.random.RandomState(N)
    cfg = MazeConfig([MM.random_layout(N, rs) for _ in range(2)], random_start=True, random_goal=True, show_goal=show_goal,
                     max_episode_steps=3)
    p = Pair(B, 6, cfg, seed=N)
    layout = p.envs[1].ring.layout.cpu().numpy()
    groups = np.concatenate([layout, np.repeat(layout[-1:], -B % 8)]).reshape(-1, 8)
    assert (groups != groups[:, :1]).any()          # a workgroup with actors of both layouts
    active = np.ones(B, dtype=np.int32)
    active[4] = 0
    n_term = 0
    for step in range(8):
        if step % 3 == 0:
            p.set_state(active=active)
        p.step()
        n_term += int(p.st[1]["t"].sum())
    assert n_term > 0 and int(p.envs[1].ring.episode.max()) >= 1


def test_patched_pieces_are_the_rendered_frame_for_every_agent_and_goal_cell():
    """Template + agent / goal patch against a host rendering of the frame (walls in channel 0, the agent's block in
    channel 1, the goal's in channel 2), byte for byte, at N = 7: one actor per (start cell, goal cell, action), which
    leaves the agent on every free cell next to every other goal cell -- and 561 workgroups' worth of the two-launch
    comparison."""
    from unreal_amd.environment.maze_environment import MazeConfig
    N, C = 7, 12
    cfg = MazeConfig([REFERENCE_MAP], show_goal=True)
    walls = np.array([[ch == '+' for ch in row] for row in REFERENCE_MAP])
    free = [(x, y) for y in range(N) for x in range(N) if not walls[y, x]]
    cases = [(s, g, a) for s in free for g in free if g != s for a in range(4)]
    B = len(cases)
    assert B == 34 * 33 * 4
    p = Pair(B, 1, cfg)
    p.set_state(pos=[c[0] for c in cases], goal=[c[1] for c in cases])
    p.step(np.array([c[2] for c in cases], dtype=np.int32))
    ring = p.envs[1].ring
    pos = ring.pos.cpu().numpy().reshape(B, 2)
    goal = ring.goal.cpu().numpy().reshape(B, 2)
    frames = ring.frames.view(-1, FB)[p.st[1]["idx"].long()].cpu().numpy().reshape(B, 84, 84, 3)
    want = np.zeros((B, 84, 84, 3), dtype=np.uint8)
    want[:, :, :, 0] = np.kron(walls, np.ones((C, C), dtype=np.uint8))[None]
    seen = set()
    for b in range(B):
        (x, y), (gx, gy) = pos[b], goal[b]
        want[b, C * y:C * y + C, C * x:C * x + C, 1] = 1
        want[b, C * gy:C * gy + C, C * gx:C * gx + C, 2] = 1
        seen.add((x, y, gx, gy))
    np.testing.assert_array_equal(frames, want)
    assert seen >= {(s[0], s[1], g[0], g[1]) for s in free for g in free if g != s}


def test_trainer_with_the_fused_step_is_the_trainer_without(monkeypatch):
    """Trainer.fuse_env_encoder on and off through whole process() calls at 2048 actors (the 8-actors-per-workgroup regime):
    identical actions, rewards, terminals and frame indices; parameters within the bar of
    test_half_batch_rollout_on_two_streams_is_the_lockstep_rollout for two schedules of one rollout (gradient atomics
    reorder).  History 8 holds replay sequences of at most 5 steps: T = 4."""
    from unreal_amd.train.trainer import Trainer
    from unreal_amd import _lib
    B, H, T = 2048, 8, 4
    cfg = _cfg(True, True, H, T)
    cfg["initial_learning_rate"] = 7.0711e-4
    out = []
    for fused in (True, False):
        monkeypatch.setattr(Trainer, "fuse_env_encoder", fused)
        calls = []
        real = _lib._Lib.call
        monkeypatch.setattr(_lib._Lib, "call", lambda self, name, *a: (calls.append(name), real(self, name, *a))[1])
        net, applier, tr, draws = _build(cfg, B, seed=5)
        while not tr._full:
            tr.process(None, 0)
        g, snaps = 0, []
        for it in range(2):
            steps, _ = tr.process(None, g)
            g += steps
            snaps.append(dict(actions=tr.actions.cpu().numpy().copy(), rewards=tr.rewards.cpu().numpy().copy(),
                              terminals=tr.terminals.cpu().numpy().copy(), n_steps=tr.n_steps.cpu().numpy().copy(),
                              idx=tr.base_ws.frame_idx.cpu().numpy().copy(), steps=steps,
                              params=net.params.flat.cpu().numpy().copy()))
        monkeypatch.setattr(_lib._Lib, "call", real)
        n_fused = calls.count("unreal_maze_policy_rollout_step_encode")
        assert n_fused == (2 * (T - 1) if fused else 0), n_fused
        out.append(snaps)
    for a, b in zip(*out):
        for k in ("actions", "rewards", "terminals", "n_steps", "idx"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert a["steps"] == b["steps"]
        np.testing.assert_allclose(b["params"], a["params"], rtol=1e-5, atol=1e-7)
