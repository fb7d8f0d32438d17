"""Gym / Atari environments on the device: the frame resize against a numpy float32 mirror of its formula and float64
bilinear, the gym terminal rule of the ring commit, and Trainer(env_type='gym') end to end against the oracle trainer
driving a transcription of reference environment/gym_environment.py (with the ring's uint8 rounding of the frame)."""
import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import DEV, dev

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def _axis(n_in, dt):
    d = np.arange(84, dtype=dt)
    s = (d + dt(0.5)) * (dt(n_in) / dt(84)) - dt(0.5)
    i0 = np.floor(s).astype(np.int64)
    f = (s - i0.astype(dt)).astype(dt)
    lo = i0 < 0
    f[lo], i0[lo] = 0, 0
    hi = i0 >= n_in - 1
    f[hi], i0[hi] = 0, n_in - 1
    return i0, np.minimum(i0 + 1, n_in - 1), f


def _bilinear(src, dt):
    """src uint8 [..., Hs, Ws, 3] -> the formula of csrc/gym.hip in dtype dt (every operation rounded on its own).  The
    sample positions are the contract's fp32 ones in both cases: on a noise image a neighbour differs by up to 255, so the
    ~1e-5 pixel a 250 / 84 scale moves between fp32 and fp64 coordinates alone is worth 5e-3 of a level."""
    Hs, Ws = src.shape[-3], src.shape[-2]
    y0, y1, fy = _axis(Hs, F32)
    x0, x1, fx = _axis(Ws, F32)
    fy, fx = fy.astype(dt), fx.astype(dt)
    p = src.astype(dt)
    r0, r1 = p[..., y0, :, :], p[..., y1, :, :]
    p00, p01, p10, p11 = r0[..., x0, :], r0[..., x1, :], r1[..., x0, :], r1[..., x1, :]
    fx, fy = fx[:, None], fy[:, None, None]
    gx, gy = (dt(1) - fx).astype(dt), (dt(1) - fy).astype(dt)
    return gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11)


def resize_mirror(src):
    """The device resize restated in numpy float32, rounded to nearest-even uint8."""
    return np.clip(np.rint(_bilinear(src, F32)), 0, 255).astype(np.uint8)


def _check_resize(got, src):
    want = resize_mirror(src)
    v64 = _bilinear(src, np.float64)
    tie = np.abs(v64 - np.floor(v64) - 0.5) < 1e-3
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert ((d == 0) | (tie & (d <= 1))).all(), "resize differs from the fp32 mirror at %d elements" % int((d != 0).sum())
    assert np.abs(got.astype(np.float64) - v64).max() <= 0.5 + 1e-3


@pytest.mark.parametrize("shape", [(210, 160), (250, 160), (84, 84), (97, 131)])
@pytest.mark.parametrize("n", [1, 3, 4096])
def test_frame_resize_matches_formula(ops, shape, n):
    Hs, Ws = shape
    rs = np.random.RandomState(Hs * 7 + Ws + n)
    distinct = min(n, 16)              # n = 4096: 16 distinct frames, tiled (the launch shape is the point)
    base = rs.randint(0, 256, size=(distinct, Hs, Ws, 3)).astype(np.uint8)
    base[0, :Hs // 2] = 255            # saturated and flat regions
    base[-1, :, :Ws // 3] = 0
    src = np.tile(base, (n // distinct, 1, 1, 1)) if n > distinct else base
    dst = torch.full((n * 21168,), 77, dtype=torch.uint8, device=DEV)
    ops.frame_resize(n, Hs, Ws, dev(src.reshape(-1)), dst)
    got = dst.cpu().numpy().reshape(n, 84, 84, 3)
    if shape == (84, 84):
        np.testing.assert_array_equal(got, src)
    for i in range(distinct):
        _check_resize(got[i], base[i])
    if n > distinct:
        np.testing.assert_array_equal(got, np.tile(got[:distinct], (n // distinct, 1, 1, 1)))
    # masked rows are left alone
    mask = (np.arange(n) % 2).astype(np.int32)
    dst2 = torch.full((n * 21168,), 77, dtype=torch.uint8, device=DEV)
    ops.frame_resize(n, Hs, Ws, dev(src.reshape(-1)), dst2, mask=dev(mask))
    g2 = dst2.cpu().numpy().reshape(n, 84, 84, 3)
    assert (g2[mask == 0] == 77).all()
    np.testing.assert_array_equal(g2[mask == 1], got[mask == 1])


def test_gym_terminal_obs_pixel_change_and_reset(ops):
    """A terminal step's pixel change is taken against the terminal observation (gym_environment.py:86), not 0 as for Lab;
    the next slot gets the post-reset observation, last action / reward are reset, the reward is stored raw."""
    from oracle.maze import calc_pixel_change
    B, H = 3, 6
    rs = np.random.RandomState(5)
    ring = ops.Ring(B, H, DEV)
    f0 = rs.randint(0, 256, size=(B, 84, 84, 3)).astype(np.uint8)
    ops.hostfed_reset(ring, dev(f0.reshape(-1)))
    f1 = rs.randint(0, 256, size=(B, 84, 84, 3)).astype(np.uint8)
    fr = rs.randint(0, 256, size=(B, 84, 84, 3)).astype(np.uint8)
    actions = np.array([7, 17, 2], np.int32)
    rewards = np.array([3.0, -1.0, 12.0], np.float32)
    terminals = np.array([1, 0, 1], np.int32)
    ops.hostfed_step(ring, dev(f1.reshape(-1)), dev(actions), dev(rewards), dev(terminals), clip_reward=False,
                     reset_staged=dev(fr.reshape(-1)), terminal_obs=True)
    H1 = H + 1
    pc = ring.r_pc.cpu().numpy().reshape(B, H1, 20, 20)
    frames = ring.frames.cpu().numpy().reshape(B, H1, 84, 84, 3)
    for b in range(B):
        want = calc_pixel_change(f1[b].astype(F32) / 255.0, f0[b].astype(F32) / 255.0)
        assert pc[b, 0].max() > 0
        np.testing.assert_allclose(pc[b, 0], want, rtol=2e-6, atol=1e-7)
        np.testing.assert_array_equal(frames[b, 0], f0[b])
        np.testing.assert_array_equal(frames[b, 1], fr[b] if terminals[b] else f1[b])
    np.testing.assert_array_equal(ring.r_reward.cpu().numpy().reshape(B, H1)[:, 0], rewards)       # unclipped
    np.testing.assert_array_equal(ring.r_terminal.cpu().numpy().reshape(B, H1)[:, 0], terminals)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), np.where(terminals, 0, actions))
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.where(terminals, 0, rewards))
    np.testing.assert_array_equal(ring.count.cpu().numpy(), [1, 1, 1])


class OracleGymEnv(object):
    """reference environment/gym_environment.py:18-96 transcribed around a gym-API object (worker + GymEnvironment in one
    process), with the ring's rounding of the resized frame: state = uint8(resize) / 255."""

    def __init__(self, env, action_size):
        self.env = env
        self.action_size = action_size
        self.env.reset()                              # the worker's own reset at start-up (:27)
        self.reset()

    @staticmethod
    def _preprocess_frame(obs):
        return resize_mirror(np.asarray(obs)).astype(F32) / F32(255.0)

    def reset(self):
        obs = self.env.reset()
        self.last_state = {'image': self._preprocess_frame(obs)}
        self.last_action = 0
        self.last_reward = 0

    def process(self, action, flag=0):
        from oracle.maze import calc_pixel_change
        reward = 0
        for _ in range(4):
            obs, r, terminal, _ = self.env.step(int(action))
            reward += r
            if terminal:
                break
        state = {'image': self._preprocess_frame(obs)}
        pc = calc_pixel_change(state['image'], self.last_state['image'])
        self.last_state = state
        self.last_action = int(action)
        self.last_reward = reward
        return state, reward, terminal, pc

    def stop(self):
        pass


# B = 4 runs the overlapped half-batch schedule; aux (True, False, False) = pixel control only
@pytest.mark.parametrize("A", [18, 9])
@pytest.mark.parametrize("B,aux", [(3, True), (4, True), (3, (True, False, False)), (4, (True, False, False))])
def test_gym_trainer_matches_oracle(A, B, aux):
    from oracle.trainer import OracleTrainer, ExplicitDraws
    from tests.test_trainer_gpu import _build, _cfg, _hostfed_parity
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.gym_environment import SyntheticAtariEnv, synthetic_atari_batch
    H, T = 40, 20
    name = "SyntheticAtari%d-v0" % A
    Environment.register_gym_config(name, A)
    cfg = _cfg(True, aux, H, T)
    cfg.update(action_size=A, initial_learning_rate=7.0711e-4)
    kw = dict(episode_len=29)
    sim = synthetic_atari_batch(B, action_size=A, seed=6, **kw)
    net, applier, tr, draws = _build(cfg, B, seed=13, env_type="gym", env_name=name, simulator=sim,
                                     frame_scale=1.0 / 255.0, overlap_host=(B % 2 == 0))
    assert tr.overlap_host == (B % 2 == 0)
    assert net.K_x == 256 + A + 1
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    envs = [OracleGymEnv(SyntheticAtariEnv(6 * 100003 + b, A, **kw), A) for b in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=envs)
    _hostfed_parity(cfg, B, H, T, tr, net, applier, draws, orc, edraws, None)
    # rewards above 1 reach the replay unclipped (train/experience.py stores them raw)
    assert max(f.reward for a in orc.actors for f in a.exp.frames.values()) > 1
    assert float(tr.ring.r_reward.max()) > 1.0
    assert any(f.terminal for a in orc.actors for f in a.exp.frames.values())
