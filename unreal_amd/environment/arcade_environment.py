"""Device arcade (csrc/arcade.hip): games stepped and rendered on the GPU.  One game, Breakout with ALE's
minimal action set (0 noop, 1 fire, 2 right, 3 left): integer-only and a pure function of (config, seed, global actor,
episode, actions).  The rules are written out with the entries in include/unreal_hip.h."""
import numpy as np
import torch

from . import environment
from .. import ops

GAMES = {"breakout": ops.ARCADE_BREAKOUT}


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (name, v))
    if not lo <= v <= hi:
        raise ValueError("%s = %d outside [%d, %d]" % (name, v, lo, hi))
    return int(v)


class ArcadeConfig(object):
    """Settings of one arcade game (Environment.register_arcade_config).  Raises ValueError outside the documented ranges."""
    ACTION_SIZE = 4
    MAX_ROWS, COLUMNS = 6, 10

    def __init__(self, game="breakout", rows=6, row_rewards=None, paddle_width=12, paddle_speed=3, ball_speed=2, lives=3,
                 serve_wait=8, life_reward=0, max_episode_steps=5000):
        if game not in GAMES:
            raise ValueError("arcade game %r: known games are %s" % (game, sorted(GAMES)))
        self.game = game
        self.rows = _int("rows", rows, 1, self.MAX_ROWS)
        if row_rewards is None:
            row_rewards = (1,) * self.rows
        if isinstance(row_rewards, (str, bytes)) or not hasattr(row_rewards, "__len__") or len(row_rewards) != self.rows:
            raise ValueError("row_rewards must hold rows = %d integers, not %r" % (self.rows, row_rewards))
        self.row_rewards = tuple(_int("row_rewards[%d]" % i, r, 0, 100) for i, r in enumerate(row_rewards))
        self.paddle_width = _int("paddle_width", paddle_width, 4, 24)
        if self.paddle_width % 2:
            raise ValueError("paddle_width = %d must be even" % self.paddle_width)
        self.paddle_speed = _int("paddle_speed", paddle_speed, 1, 8)
        self.ball_speed = _int("ball_speed", ball_speed, 1, 4)
        self.lives = _int("lives", lives, 1, 5)
        self.serve_wait = _int("serve_wait", serve_wait, 0, 255)
        self.life_reward = _int("life_reward", life_reward, -100, 0)
        # mandatory: a ball that loops between the walls never ends an episode on its own
        self.max_episode_steps = _int("max_episode_steps", max_episode_steps, 1, 2 ** 31 - 1)

    @property
    def action_size(self):
        return self.ACTION_SIZE

    def block(self, seed):
        """The int32 block of the kernels (UNREAL_ARCADE_CFG_WORDS words; layout: include/unreal_hip.h)."""
        seed = int(seed) & (2 ** 64 - 1)
        w = np.zeros(ops.ARCADE_CFG_WORDS, dtype=np.int64)
        w[0] = GAMES[self.game]
        w[2], w[3] = self.rows, self.max_episode_steps
        w[4], w[5] = seed & 0xFFFFFFFF, seed >> 32
        w[6:12] = (self.paddle_width, self.paddle_speed, self.ball_speed, self.lives, self.serve_wait, self.life_reward)
        w[12:12 + self.rows] = self.row_rewards
        return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


class BatchedArcadeEnvironment(object):
    """B actors of one arcade game on the device, with the interface of BatchedMazeEnvironment."""
    ACTION_SIZE = 4
    frame_scale = 1.0 / 255.0          # ring bytes 0..255
    objective_size = 0

    def __init__(self, batch, history_size, device="cuda:0", config=None, actor_base=0, actors_total=None, seed=0):
        """`actor_base` / `actors_total`: global index of actor 0 and the number of actors over every rank (the serve
        draws are keyed by the global index); `seed`: their key."""
        if not isinstance(config, ArcadeConfig):
            raise ValueError("BatchedArcadeEnvironment needs an ArcadeConfig")
        self.B = batch
        self.config = config
        total = batch if actors_total is None else int(actors_total)
        if actor_base < 0 or actor_base + batch > total:
            raise ValueError("actors [%d, %d) outside the %d actors of the job" % (actor_base, actor_base + batch, total))
        self.ring = ops.Ring(batch, history_size, torch.device(device), arcade=True)
        block = torch.from_numpy(config.block(seed)).to(self.ring.count.device)
        self.arcade = (block, int(actor_base))
        self.reset()

    def view(self, b0, b1):
        """The environments [b0, b1) as a batched environment of their own (shares the ring memory), as
        BatchedMazeEnvironment.view."""
        v = object.__new__(BatchedArcadeEnvironment)
        v.B, v.ring = b1 - b0, ops.ring_view(self.ring, b0, b1)
        v.base_actor = b0
        v.config = self.config
        v.arcade = (self.arcade[0], self.arcade[1] + b0)
        return v

    @staticmethod
    def get_action_size():
        return 4

    def reset(self, mask=None):
        ops.arcade_reset(self.ring, mask, arcade=self.arcade)

    def process(self, actions, active=None, out_reward=None, out_terminal=None, reset_on_terminal=True,
                track_score=False):
        ops.arcade_step(self.ring, actions, active, out_reward, out_terminal, reset_on_terminal, track_score,
                        arcade=self.arcade)

    def rollout_step(self, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                     index_parent=False, **nxt):
        ops.arcade_rollout_step(self.ring, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                                base_actor=getattr(self, "base_actor", 0) if index_parent else 0, arcade=self.arcade,
                                **nxt)

    def policy_rollout_step(self, net, feat, ld, u, pi_out, v_out, actions, out_reward, out_terminal, active, active_log_t,
                            n_steps, terminal_end, index_parent=False, **nxt):
        p = net.p
        ops.arcade_policy_rollout_step(self.ring, feat, ld, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                       p["b_base_fc_v"], u, pi_out, v_out, actions, out_reward, out_terminal, active,
                                       active_log_t, n_steps, terminal_end,
                                       base_actor=getattr(self, "base_actor", 0) if index_parent else 0,
                                       arcade=self.arcade, **nxt)

    def current_records(self):
        """The game records -> int32 [B, 16]: px, bx, by, vx, vy, wait, lives, bricks lo, hi, serve_index, then the
        running totals of bricks, lives lost and walls cleared."""
        return self.ring.actor_records.cpu().numpy().copy()

    def stop(self):
        pass


class ArcadeEnvironment(environment.Environment):
    """The batch-1 surface of the reference's environments: process(action) -> image, reward, terminal, pixel_change.
    No reset on terminal: the caller resets."""

    @staticmethod
    def get_action_size():
        return 4

    def __init__(self, device="cuda:0", config=None, seed=0):
        environment.Environment.__init__(self)
        self._env = BatchedArcadeEnvironment(1, 2, device, config=config, seed=seed)
        self._a = torch.zeros(1, dtype=torch.int32, device=device)
        self._r = torch.zeros(1, dtype=torch.float32, device=device)
        self._t = torch.zeros(1, dtype=torch.int32, device=device)
        self.reset()

    def _image(self):
        ring = self._env.ring
        slot = int(ring.count.cpu()[0]) % ring.H1
        fr = ring.frames[slot * ops.FRAME_BYTES:(slot + 1) * ops.FRAME_BYTES]
        return fr.cpu().numpy().reshape(84, 84, 3).astype(np.float64) / 255.0

    def reset(self):
        self._env.reset()
        self.last_state = {'image': self._image()}
        self.last_action = 0
        self.last_reward = 0

    def process(self, action, flag=0):
        ring = self._env.ring
        self._a[0] = int(action)
        slot = int(ring.count.cpu()[0]) % ring.H1
        self._env.process(self._a, None, self._r, self._t, reset_on_terminal=False)
        image = self._image()
        reward = int(self._r.cpu()[0])
        terminal = bool(self._t.cpu()[0])
        pc = ring.r_pc[slot * ops.PC_CELLS:(slot + 1) * ops.PC_CELLS].cpu().numpy().reshape(20, 20)
        self.last_state = {'image': image}
        self.last_action = int(action)
        self.last_reward = reward
        rec = self._env.current_records()[0]
        self._last_full_state = {"success": terminal and not (rec[7] | rec[8])}
        return image, reward, terminal, pc
