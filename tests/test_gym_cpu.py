"""Gym / Atari environments without a GPU: the batch simulator's action repeat against a transcription of the reference
worker (gym_environment.py:25-50), the action-size registry, and the argument checks of the new C-ABI entries (they
return UNREAL_EINVAL before any launch, so they run on a machine without a GPU)."""
import ctypes

import numpy as np
import pytest

from unreal_amd.environment.environment import Environment
from unreal_amd.environment.gym_environment import GymBatchSimulator, SyntheticAtariEnv, synthetic_atari_batch

EINVAL = -22


def _worker_step(env, action):
    """gym_environment.py:34-42, transcribed: repeat 4 times, sum, stop at a terminal."""
    reward = 0
    for _ in range(4):
        obs, r, terminal, _ = env.step(action)
        reward += r
        if terminal:
            break
    return obs, reward, terminal


@pytest.mark.parametrize("A,episode_len", [(18, 47), (9, 8), (5, 13)])
def test_batch_simulator_repeats_sums_and_stops_like_the_worker(A, episode_len):
    B, steps = 5, 60
    sim = synthetic_atari_batch(B, action_size=A, seed=3, episode_len=episode_len)
    ref = [SyntheticAtariEnv(3 * 100003 + b, A, episode_len=episode_len) for b in range(B)]
    first = [r.reset() for r in ref]
    f0 = sim.reset()
    assert f0.shape == (B, 210, 160, 3) and f0.dtype == np.uint8
    for b in range(B):
        np.testing.assert_array_equal(f0[b], first[b])
    rs = np.random.RandomState(0)
    saw_big = saw_terminal = False
    for t in range(steps):
        actions = rs.randint(0, A, size=B).astype(np.int32)
        active = (rs.random_sample(B) < 0.8).astype(np.int32)
        frames, rewards, terminals = sim.step(actions, active)
        frames = frames.copy()
        for b in range(B):
            if not active[b]:
                assert rewards[b] == 0 and terminals[b] == 0
                continue
            obs, r, term = _worker_step(ref[b], int(actions[b]))
            np.testing.assert_array_equal(frames[b], obs)
            assert rewards[b] == np.float32(r) and bool(terminals[b]) == term
            saw_big |= r > 1
            saw_terminal |= term
        if terminals.any():
            after = sim.reset(terminals)
            for b in np.nonzero(terminals)[0]:
                np.testing.assert_array_equal(after[b], ref[b].reset())
    assert saw_big and saw_terminal


def test_synthetic_env_stream_does_not_depend_on_reset_count():
    a, b = SyntheticAtariEnv(11, 18), SyntheticAtariEnv(11, 18)
    a.reset()
    a.reset()
    b.reset()
    for act in (3, 17, 0, 5):
        oa, ra, ta, _ = a.step(act)
        ob, rb, tb, _ = b.step(act)
        np.testing.assert_array_equal(oa, ob)
        assert (ra, ta) == (rb, tb)
    with pytest.raises(ValueError):
        a.step(18)


def test_get_action_size_gym():
    saved = Environment.action_size
    try:
        Environment.register_gym_config("SyntheticPong-v0", 18)
        Environment.register_gym_config("SyntheticNine-v0", 9)
        Environment.action_size = -1
        assert Environment.get_action_size("gym", "SyntheticPong-v0") == 18
        Environment.action_size = -1
        assert Environment.get_action_size("gym", "SyntheticNine-v0") == 9
        Environment.action_size = -1
        with pytest.raises(KeyError):
            Environment.get_action_size("gym", "NotRegistered-v0")
        for bad in (0, 1, 19):
            with pytest.raises(ValueError):
                Environment.register_gym_config("Bad-v0", bad)
        assert Environment.get_objective_size("gym", "SyntheticPong-v0") == 0
    finally:
        Environment.action_size = saved


def test_gym_simulator_rejects_non_rgb_frames():
    class Gray(object):
        def reset(self):
            return np.zeros((210, 160), np.uint8)

    with pytest.raises(ValueError):
        GymBatchSimulator([Gray()])


# ---- argument checks of the new and widened entries (no launch happens) --------------------------------------------
class _RC(object):
    """Return codes of the raw entries (lib().call raises on a non-zero code)."""

    def __init__(self, lib):
        self.lib = lib

    def call(self, name, *args):
        return self.lib._fn[name](*args)


def _lib():
    from unreal_amd._lib import lib
    try:
        return _RC(lib())
    except Exception as e:                       # the library is built by build(); without it there is nothing to check
        pytest.skip("libunreal_hip.so not loadable: %s" % e)


class _Buf(object):
    """Host buffers with chosen alignment, passed as raw addresses (never dereferenced: the checks fail first)."""

    def __init__(self):
        self.keep = []

    def __call__(self, nbytes=4096, offset=0):
        b = ctypes.create_string_buffer(nbytes + 64)
        self.keep.append(b)
        base = (ctypes.addressof(b) + 15) // 16 * 16
        return base + offset


def test_frame_resize_argument_checks():
    L, buf = _lib(), _Buf()
    src, dst = buf(), buf()
    assert L.call("unreal_frame_resize", 0, 210, 160, src, None, dst, None) == EINVAL
    assert L.call("unreal_frame_resize", 1, 0, 160, src, None, dst, None) == EINVAL
    assert L.call("unreal_frame_resize", 1, 210, 0, src, None, dst, None) == EINVAL
    assert L.call("unreal_frame_resize", 1, 210, 160, None, None, dst, None) == EINVAL
    assert L.call("unreal_frame_resize", 1, 210, 160, src, None, None, None) == EINVAL
    assert L.call("unreal_frame_resize", 1, 210, 160, src, None, buf(offset=4), None) == EINVAL     # misaligned dst


def test_hostfed_step_argument_checks():
    """unreal_hostfed_step refuses on the host what any of the three contracts (Lab, indoor, gym) refused."""
    L, buf = _lib(), _Buf()
    p = [buf() for _ in range(20)]
    CLIP, TERMINAL_OBS = 1, 2
    r = dict(last_action=p[5], last_reward=p[6], r_reward=p[9], r_action=p[10], r_terminal=p[11], r_last_action=p[12],
             r_last_reward=p[13])

    def call(B=2, H1=4, stride=21168, staged=p[0], reset=p[1], frames=p[8], r_pc=p[14], reset_on_terminal=1, track=0,
             flags=TERMINAL_OBS, denom=48.0 * 255.0, **kw):
        q = dict(r, **kw)
        return L.call("unreal_hostfed_step", B, H1, stride, staged, reset, p[2], p[3], p[4], None, q["last_action"],
                      q["last_reward"], p[7], frames, q["r_reward"], q["r_action"], q["r_terminal"], q["r_last_action"],
                      q["r_last_reward"], r_pc, None, None, None, None, None, reset_on_terminal, track, flags, denom, None)

    assert call(B=0) == EINVAL
    assert call(H1=1) == EINVAL
    assert call(staged=None) == EINVAL
    assert call(reset=None) == EINVAL                    # reset_on_terminal needs the post-reset observations
    assert call(track=1) == EINVAL                       # score tracking needs its buffers
    assert call(denom=0.0) == EINVAL
    assert call(staged=buf(offset=8)) == EINVAL          # misaligned
    assert call(reset=buf(offset=4)) == EINVAL
    assert call(frames=buf(offset=4)) == EINVAL
    # the Lab and indoor checks, now the same entry's
    assert call(stride=21168 + 8) == EINVAL              # not a multiple of 16
    assert call(stride=1200 - 16, r_pc=None) == EINVAL   # below 20 x 20 x 3
    assert call(stride=691200 + 16, r_pc=None) == EINVAL  # above 480 x 480 x 3
    assert call(stride=1200) == EINVAL                   # pixel change at 84 x 84 only
    assert call(flags=CLIP) == EINVAL                    # reset_staged without the gym terminal rule
    assert call(flags=0, reset=None, denom=0.0) == EINVAL
    assert call(flags=4) == EINVAL                       # no such flag
    for name in r:                                       # every pointer the step writes through
        assert call(**{name: None}) == EINVAL, name
        assert call(flags=CLIP, reset=None, **{name: None}) == EINVAL, name


@pytest.mark.parametrize("A", [0, 19])
def test_action_count_bounds(A):
    """A <= 18 is the new bound of every A-dependent entry; A = 0 and A = 19 are still rejected before any launch."""
    L, buf = _lib(), _Buf()
    p = [buf(1 << 16) for _ in range(24)]
    assert L.call("unreal_softmax_sample", 4, A, p[0], max(A, 1), p[1], p[2], None) == EINVAL
    assert L.call("unreal_policy_step", 4, A, p[0], 256, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], None) == EINVAL
    assert L.call("unreal_base_loss_grad", 4, A, p[0], max(A, 1), p[1], p[2], p[3], p[4], p[5], 0.01, 1.0, p[6], p[7], p[8],
                  None) == EINVAL
    assert L.call("unreal_pc_deconv_fwd", 4, A, p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, None, None, 0.05, 1.0, None,
                  None, None, None) == EINVAL
    assert L.call("unreal_pc_deconv_bwd", 4, A, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                  None) == EINVAL
    assert L.call("unreal_pc_deconv_train", 4, A, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], 0.05, 1.0, p[9],
                  p[10], p[11], p[12], p[13], p[14], p[15], None, None) == EINVAL
    # linear_small: NOUT = A + 1 <= 19 is the widest instance
    assert L.call("unreal_linear_small_fwd", 4, 256, A + 1 if A else 0, p[0], 256, p[1], p[2], p[3], 32, None) == EINVAL
    assert L.call("unreal_linear_small_bwd", 4, 256, A + 1 if A else 0, p[0], 256, p[1], 32, p[2], None, 0, 0, p[3], 0, 0,
                  None, None) == EINVAL
