"""Gym / Atari environments, host-fed (reference environment/gym_environment.py:18-96).

`GymBatchSimulator` wraps a list of objects with gym's old API (reset() -> obs, step(a) -> (obs, reward, done, info)) and
does what the reference's worker process does per command (gym_environment.py:25-50): an action is repeated 4 times, the
rewards summed, the repeat stops at a terminal.  It hands RAW uint8 frames [n, Hs, Ws, 3] to the host-fed environment,
which stages them as they are; the resize to 84 x 84 (preprocess_frame, :18-23) runs on the device (ops.frame_resize) and
the ring commit follows the gym terminal rule (ops.hostfed_step, terminal_obs).  Rewards are not clipped (this fork's
train/experience.py).

gym and cv2 are not in the image: `SyntheticAtariEnv` is a deterministic stand-in with the Atari frame shape."""
import numpy as np

ACTION_REPEAT = 4                     # gym_environment.py:38


class SyntheticAtariEnv(object):
    """Deterministic gym-API stand-in: textured 210 x 160 x 3 uint8 frames, `action_size` actions, episodes of
    `episode_len` raw steps, rewards in {-1, 0, 1, 3} (sums of up to four per agent step: values > 1 are common).  The frame
    and reward of a step depend on the seed, the step within the episode and a hash of the episode's actions -- not on how
    often reset() was called, so two instances with one seed produce the same stream under any reset schedule."""
    _BANK = {}
    BANK_SIZE = 16
    _REWARDS = (0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0)

    def __init__(self, seed, action_size=18, episode_len=47, shape=(210, 160)):
        self.seed, self.action_size, self.episode_len = int(seed), int(action_size), int(episode_len)
        self.shape = tuple(shape)
        self.bank = self._bank(self.shape)
        self.t, self.h = 0, 0

    @classmethod
    def _bank(cls, shape):
        if shape not in cls._BANK:
            H, W = shape
            rs = np.random.RandomState(1234)
            yy, xx = np.mgrid[0:H, 0:W]
            frames = np.empty((cls.BANK_SIZE, H, W, 3), np.uint8)
            for k in range(cls.BANK_SIZE):
                for c in range(3):
                    smooth = (xx * (3 + c) + yy * (5 + 2 * k) + 37 * k * (c + 1)) % 256
                    frames[k, :, :, c] = ((smooth + rs.randint(0, 48, size=(H, W))) % 256).astype(np.uint8)
            cls._BANK[shape] = frames
        return cls._BANK[shape]

    def _obs(self):
        return self.bank[(self.h + self.t) % self.BANK_SIZE]

    def reset(self):
        self.t, self.h = 0, self.seed % 9973
        return self._obs()

    def step(self, action):
        a = int(action)
        if not 0 <= a < self.action_size:
            raise ValueError("action %d outside [0, %d)" % (a, self.action_size))
        self.t += 1
        self.h = (self.h * 31 + a + 1) % 1000003
        reward = self._REWARDS[(self.h + 3 * self.t) % len(self._REWARDS)]
        done = self.t >= self.episode_len
        return self._obs(), reward, done, {}


class GymBatchSimulator(object):
    """B gym-API environments behind the batched host-fed interface, raw frames out.

    reset(mask) -> uint8 [B, Hs, Ws, 3]: the reset observation where mask (all when None), the current one elsewhere.
    step(actions, active) -> (frames uint8 [B, Hs, Ws, 3], rewards f32 [B], terminals i32 [B]): the frame after the action
    repeat (the TERMINAL observation where terminal; the host-fed environment then resets those actors itself)."""
    gym = True

    def __init__(self, envs):
        self.envs = list(envs)
        self.B = len(self.envs)
        first = np.asarray(self.envs[0].reset())
        if first.dtype != np.uint8 or first.ndim != 3 or first.shape[2] != 3:
            raise ValueError("gym frames must be uint8 [H, W, 3], got %s %s" % (first.dtype, first.shape))
        self.frame_shape = first.shape[:2]
        self._frames = np.empty((self.B,) + first.shape, np.uint8)
        self._frames[0] = first
        for b in range(1, self.B):
            self._frames[b] = self.envs[b].reset()

    def reset(self, mask=None):
        for b, e in enumerate(self.envs):
            if mask is None or mask[b]:
                self._frames[b] = e.reset()
        return self._frames

    def step(self, actions, active=None):
        rewards = np.zeros(self.B, np.float32)
        terminals = np.zeros(self.B, np.int32)
        for b, e in enumerate(self.envs):
            if active is not None and not active[b]:
                continue
            reward = 0.0
            for _ in range(ACTION_REPEAT):            # gym_environment.py:35-41
                obs, r, terminal, _ = e.step(int(actions[b]))
                reward += r
                if terminal:
                    break
            self._frames[b] = obs
            rewards[b], terminals[b] = reward, int(terminal)
        return self._frames, rewards, terminals


def synthetic_atari_batch(batch, action_size=18, seed=7, **kw):
    """GymBatchSimulator over `batch` SyntheticAtariEnv with seeds seed * 100003 + b."""
    return GymBatchSimulator([SyntheticAtariEnv(seed * 100003 + b, action_size, **kw) for b in range(batch)])
