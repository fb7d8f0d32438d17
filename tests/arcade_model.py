"""Host model of the device arcade (csrc/arcade.hip): Breakout in plain Python / numpy, written from the rules
in include/unreal_hip.h and the issue's text, not from the kernel: record, frame bytes, reward, terminal, pixel change.

Corner cases the rules leave open are fixed HERE (DESIGN §7k lists them): the wall-cleared / life-lost check that ends
the micro-steps early is made after a whole micro-step (x move and y move); a reset zeroes bx, by, vx, vy; a lost life
leaves them as they are; without a reset on terminal the game simply goes on from the terminal state (lives may fall
below 0; a cleared wall stays cleared), and `terminal` stays set while lives <= 0, no brick is live or steps >= the limit."""
import numpy as np

try:
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests.maze_model import philox4x32_10

SERVE_STREAM = 0x41524B53
PC_DENOM = 48 * 255
BORDER, WHITE, PADDLE = (142, 142, 142), (236, 236, 236), (200, 72, 72)
ROW_COLOURS = [(200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200)]
NOOP, FIRE, RIGHT, LEFT = 0, 1, 2, 3


def pixel_change(new, old):
    """20 x 20 float32 pixel change of two uint8 frames: the [2:-2] crop in 4 x 4 blocks over 48 * 255."""
    d = np.abs(new[2:-2, 2:-2].astype(np.int64) - old[2:-2, 2:-2].astype(np.int64)).sum(2)
    s = d.reshape(20, 4, 20, 4).sum(axis=(1, 3))
    return (s / float(PC_DENOM)).astype(np.float32)


class HostBreakout(object):
    """One actor: global index g, the key `seed` of its serve draws.  Like the device environment its constructor resets
    once (episode 0); `events` collects what happened in the last step (names: see process)."""

    def __init__(self, config, g=0, seed=0, frames=True):
        self.c, self.g, self.seed, self.frames = config, int(g), int(seed) & (2 ** 64 - 1), frames
        self.px = self.bx = self.by = self.vx = self.vy = self.wait = self.lives = 0
        self.bricks = 0
        self.serve_index = 0
        self.totals = [0, 0, 0]           # bricks, lives lost, walls cleared
        self.ep_steps, self.episode = 0, -1
        self.events = set()
        self.frame = self.last_state = None
        self.reset()

    # ---- state -------------------------------------------------------------------------------------------------------
    def reset(self):
        c = self.c
        self.episode += 1
        self.px = 42 - c.paddle_width // 2
        self.bx = self.by = self.vx = self.vy = 0
        self.wait, self.lives = 0, c.lives
        self.bricks = (1 << (10 * c.rows)) - 1
        self.serve_index, self.ep_steps = 0, 0
        self.last_action, self.last_reward = 0, 0
        if self.frames:
            self.frame = self.render()
            self.last_state = {'image': self.frame / 255.0}

    def record(self):
        rec = [self.px, self.bx, self.by, self.vx, self.vy, self.wait, self.lives, self.bricks & 0xFFFFFFFF,
               self.bricks >> 32, self.serve_index] + self.totals + [0, 0, 0]
        return np.array(rec, dtype=np.int64).astype(np.uint32).view(np.int32)

    def render(self):
        c = self.c
        f = np.zeros((84, 84, 3), dtype=np.uint8)
        f[0:6, :] = BORDER
        f[:, 0:2] = BORDER
        f[:, 82:84] = BORDER
        for k in range(self.lives):
            f[2:4, 4 + 4 * k:6 + 4 * k] = WHITE
        for r in range(c.rows):
            for col in range(10):
                if (self.bricks >> (10 * r + col)) & 1:
                    f[18 + 3 * r:21 + 3 * r, 2 + 8 * col:10 + 8 * col] = ROW_COLOURS[r]
        f[78:80, self.px:self.px + c.paddle_width] = PADDLE
        if self.wait < 0:
            f[self.by:self.by + 2, self.bx:self.bx + 2] = WHITE
        return f

    # ---- rules -------------------------------------------------------------------------------------------------------
    def _brick_at(self, x, y):
        """The live brick with the lowest bit that the 2 x 2 box at (x, y) overlaps, or -1."""
        best = -1
        for yy in (y, y + 1):
            for xx in (x, x + 1):
                if 2 <= xx <= 81 and 18 <= yy < 18 + 3 * self.c.rows:
                    bit = 10 * ((yy - 18) // 3) + (xx - 2) // 8
                    if (self.bricks >> bit) & 1 and (best < 0 or bit < best):
                        best = bit
        return best

    def _take(self, bit, axis):
        self.bricks &= ~(1 << bit)
        self.totals[0] += 1
        self.events.add("brick_" + axis)
        self.step_bricks += 1
        if self.bricks == 0:
            self.totals[2] += 1
        return self.c.row_rewards[bit // 10]

    def _serve(self):
        u = philox4x32_10((self.g, self.episode, SERVE_STREAM, self.serve_index), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        self.bx = 2 + 2 * (int(u[0]) % 39)
        self.by = 40
        self.vx = 1 if int(u[1]) & 1 else -1
        self.vy = 1
        self.wait = -1
        self.serve_index += 1

    def _micro_step(self):
        """-> (reward, life lost)."""
        c, reward = self.c, 0
        tx = self.bx + self.vx
        if tx < 2 or tx + 1 > 81:
            self.events.add("wall_left" if tx < 2 else "wall_right")
            self.vx = -self.vx
        else:
            bit = self._brick_at(tx, self.by)
            if bit >= 0:
                reward += self._take(bit, "x")
                self.vx = -self.vx
            else:
                self.bx = tx
        ty = self.by + self.vy
        if ty < 6:
            self.events.add("wall_top")
            self.vy = 1
            return reward, False
        bit = self._brick_at(self.bx, ty)
        if bit >= 0:
            reward += self._take(bit, "y")
            self.vy = -self.vy
        elif self.vy > 0 and ty + 1 == 78 and self.bx + 1 >= self.px and self.bx <= self.px + c.paddle_width - 1:
            w = c.paddle_width
            d = (self.bx + 1) - (self.px + w // 2)
            self.vy = -1
            seg = 0 if 4 * d < -w else 1 if d < 0 else 2 if 4 * d < w else 3
            self.vx = (-2, -1, 1, 2)[seg]
            self.events.add("paddle_%d" % seg)
        elif ty + 1 > 83:
            self.lives -= 1
            self.totals[1] += 1
            self.wait = 0
            self.events.add("life_lost")
            return reward + c.life_reward, True
        else:
            self.by = ty
        return reward, False

    def process(self, action, flag=0):
        """One step, without the reset (the caller resets at a terminal) -> (state, reward, terminal, pixel change).
        events: wall_left / wall_right / wall_top, brick_x / brick_y, two_bricks, paddle_0..3, life_lost, serve_fire /
        serve_auto, end_lives / end_clear / end_timeout."""
        c = self.c
        a = int(action)
        self.events = set()
        self.step_bricks = 0
        reward = 0
        self.ep_steps += 1
        if a == RIGHT:
            self.px = min(self.px + c.paddle_speed, 82 - c.paddle_width)
        elif a == LEFT:
            self.px = max(self.px - c.paddle_speed, 2)
        if self.wait >= 0:
            if a == FIRE or (c.serve_wait > 0 and self.wait >= c.serve_wait):
                self.events.add("serve_fire" if a == FIRE else "serve_auto")
                self._serve()
            else:
                self.wait += 1
        else:
            for _ in range(c.ball_speed):
                r, lost = self._micro_step()
                reward += r
                if lost or self.bricks == 0:
                    break
        if self.step_bricks >= 2:
            self.events.add("two_bricks")
        terminal = self.lives <= 0 or self.bricks == 0 or self.ep_steps >= c.max_episode_steps
        if terminal:
            self.events.add("end_lives" if self.lives <= 0 else "end_clear" if self.bricks == 0 else "end_timeout")
        self.success = terminal and self.bricks == 0
        pc = None
        if self.frames:
            frame = self.render()
            pc = pixel_change(frame, self.frame)
            self.frame = frame
            self.last_state = {'image': frame / 255.0}
        self.last_action = a
        self.last_reward = reward
        return self.last_state, reward, terminal, pc

    def stop(self):
        pass


def host_batch(conf, B, seed, actor_base=0, frames=True):
    """The host models of the actors [actor_base, actor_base + B) of a device environment with key `seed`, each reset
    once as the environment's constructor does; OracleTrainer(envs=...) accepts them."""
    return [HostBreakout(conf, actor_base + b, seed, frames=frames) for b in range(B)]


# ---- the traces the GPU test compares step by step (tests/test_arcade_gpu.py); tests/test_arcade_cpu.py checks on this
# model alone that they hold the events below ------------------------------------------------------------------------------
TRACE_B, TRACE_STEPS, TRACE_FRAMES = 200, 300, 6       # actors, steps, actors whose frames and pixel change are compared
TRACE_SEED = 1                                         # key of the serve draws
TRACE_SETTINGS = [dict(),
                  dict(rows=2, lives=2, paddle_width=4, ball_speed=4, row_rewards=(7, 1), life_reward=-1),
                  dict(rows=1, paddle_width=24, ball_speed=1, serve_wait=0)]
_COMMON = {"wall_left", "wall_right", "brick_x", "brick_y", "paddle_0", "paddle_1", "paddle_2", "paddle_3", "life_lost",
           "end_lives", "serve_fire"}
# what each setting's random trace holds (rows = 1 at one pixel per step reaches the top wall; serve_wait = 0 never
# serves by itself).  Within 300 steps no random actor clears a wall, and max_episode_steps is 5000 in all three: those two
# endings come from the scripted trace below.
TRACE_EVENTS = [_COMMON | {"two_bricks", "serve_auto"}, _COMMON | {"two_bricks", "serve_auto"}, _COMMON | {"wall_top"}]
# a fourth trace: a policy that follows the ball clears one row of bricks; where its ball ends up in a loop the episode
# runs into max_episode_steps
SCRIPTED_SETTING = dict(rows=1, paddle_width=24, paddle_speed=8, ball_speed=4, serve_wait=0, lives=5, max_episode_steps=300)
SCRIPTED_B, SCRIPTED_STEPS = 12, 320
SCRIPTED_EVENTS = {"end_clear", "end_timeout", "wall_top", "brick_y", "serve_fire"}


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each."""
    rs = np.random.RandomState(100 * k + 1)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active


def follow_ball(m):
    """The scripted policy: fire while the ball waits, else keep the paddle's middle under where the ball is heading."""
    if m.wait >= 0:
        return FIRE
    mid, aim = m.px + m.c.paddle_width // 2, m.bx + 1 + 2 * m.vx
    return RIGHT if aim > mid + 2 else LEFT if aim < mid - 2 else NOOP
