"""Host model of the device arcade's two-paddle duel (csrc/arcade.hip) in plain Python / numpy, written from
the rules in include/unreal_hip.h and the issue's text, not from the kernel: record, frame bytes, reward, terminal, pixel
change.  It has HostBreakout's interface (tests/arcade_model.py), so OracleTrainer(envs=...) accepts it.

Corner cases the rules leave open are fixed HERE (DESIGN §7l lists them): the opponent moves before the serve and before the
ball, from the ball state the step started with (so a ball served in this step is not followed yet, and in a step that
scores the opponent has still moved); a paddle return leaves `by` as it is (the ball turns one pixel off the paddle, as in
Breakout); a paddle is tested before the field's ends, and only on the exact line (ty + 1 == 78, ty == 9), so a ball beside
a paddle flies on through the paddle's rows to the end of the field; a point is made in the y move, after that micro-step's
x move, and ends the micro-steps; a point leaves bx, by, vx, vy as they are (the ball is not drawn while it waits), a reset
zeroes them; `terminal` names its ending in this order: the agent's score, the opponent's, the step limit (a match point
in the last allowed step is a win or a loss, any other point there is a time-out); without a reset on terminal the game
goes on, scores run past `points` (nine blocks drawn at the most), matches-won is not counted again, `terminal` stays set."""
import numpy as np

try:
    from maze_model import philox4x32_10
    from arcade_model import pixel_change, SERVE_STREAM, BORDER, WHITE, PADDLE, NOOP, FIRE, RIGHT, LEFT
except ImportError:            # imported as tests.<module>
    from tests.maze_model import philox4x32_10
    from tests.arcade_model import pixel_change, SERVE_STREAM, BORDER, WHITE, PADDLE, NOOP, FIRE, RIGHT, LEFT

OPPONENT = (66, 72, 200)
MAX_BLOCKS = 9


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


class HostDuel(object):
    """One actor: global index g, the key `seed` of its serve draws.  Like the device environment its constructor resets
    once (episode 0); `events` collects what happened in the last step (names: see process)."""

    def __init__(self, config, g=0, seed=0, frames=True):
        self.c, self.g, self.seed, self.frames = config, int(g), int(seed) & (2 ** 64 - 1), frames
        self.px = self.bx = self.by = self.vx = self.vy = self.wait = self.ox = 0
        self.mine = self.theirs = 0
        self.serve_index = 0
        self.totals = [0, 0, 0]           # points won, points lost, matches won
        self.ep_steps, self.episode = 0, -1
        self.events = set()
        self.success = False
        self.frame = self.last_state = None
        self.reset()

    # ---- state -------------------------------------------------------------------------------------------------------
    def reset(self):
        c = self.c
        self.episode += 1
        self.px = 42 - c.paddle_width // 2
        self.ox = 42 - c.opponent_width // 2
        self.bx = self.by = self.vx = self.vy = 0
        self.wait = 0
        self.mine = self.theirs = 0
        self.serve_index, self.ep_steps = 0, 0
        self.last_action, self.last_reward = 0, 0
        if self.frames:
            self.frame = self.render()
            self.last_state = {'image': self.frame / 255.0}

    def record(self):
        rec = [self.px, self.bx, self.by, self.vx, self.vy, self.wait, self.ox, self.mine, self.theirs,
               self.serve_index] + self.totals + [0, 0, 0]
        return np.array(rec, dtype=np.int64).astype(np.uint32).view(np.int32)

    def render(self):
        c = self.c
        f = np.zeros((84, 84, 3), dtype=np.uint8)
        f[0:6, :] = BORDER
        f[:, 0:2] = BORDER
        f[:, 82:84] = BORDER
        for k in range(min(self.mine, MAX_BLOCKS)):
            f[2:4, 4 + 4 * k:6 + 4 * k] = WHITE
        for k in range(min(self.theirs, MAX_BLOCKS)):
            f[2:4, 78 - 4 * k:80 - 4 * k] = OPPONENT
        f[78:80, self.px:self.px + c.paddle_width] = PADDLE
        f[8:10, self.ox:self.ox + c.opponent_width] = OPPONENT
        if self.wait < 0:
            f[self.by:self.by + 2, self.bx:self.bx + 2] = WHITE
        return f

    # ---- rules -------------------------------------------------------------------------------------------------------
    def _serve(self):
        u = philox4x32_10((self.g, self.episode, SERVE_STREAM, self.serve_index), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        self.bx = 2 + 2 * (int(u[0]) % 39)
        self.by = 40
        self.vx = 1 if int(u[1]) & 1 else -1
        self.vy = 1 if int(u[2]) & 1 else -1
        self.wait = -1
        self.serve_index += 1

    @staticmethod
    def _segment(bx, x, w):
        d = (bx + 1) - (x + w // 2)
        return 0 if 4 * d < -w else 1 if d < 0 else 2 if 4 * d < w else 3

    def _micro_step(self):
        """-> (reward, a point was made)."""
        c = self.c
        tx = self.bx + self.vx
        if tx < 2 or tx + 1 > 81:
            self.events.add("wall_left" if tx < 2 else "wall_right")
            self.vx = -self.vx
        else:
            self.bx = tx
        ty = self.by + self.vy
        if self.vy > 0 and ty + 1 == 78 and self.bx + 1 >= self.px and self.bx <= self.px + c.paddle_width - 1:
            seg = self._segment(self.bx, self.px, c.paddle_width)
            self.vy, self.vx = -1, (-2, -1, 1, 2)[seg]
            self.events.add("paddle_%d" % seg)
        elif self.vy < 0 and ty == 9 and self.bx + 1 >= self.ox and self.bx <= self.ox + c.opponent_width - 1:
            seg = self._segment(self.bx, self.ox, c.opponent_width)
            self.vy, self.vx = 1, (-2, -1, 1, 2)[seg]
            self.events.add("opp_%d" % seg)
        elif ty + 1 > 83:
            self.theirs += 1
            self.totals[1] += 1
            self.wait = 0
            self.events.add("point_lost")
            return c.lose_reward, True
        elif ty < 6:
            self.mine += 1
            self.totals[0] += 1
            if self.mine == c.points:
                self.totals[2] += 1
            self.wait = 0
            self.events.add("point_won")
            return c.win_reward, True
        else:
            self.by = ty
        return 0, False

    def process(self, action, flag=0):
        """One step, without the reset (the caller resets at a terminal) -> (state, reward, terminal, pixel change).
        events: wall_left / wall_right, paddle_0..3, opp_0..3, point_won / point_lost, serve_fire / serve_auto,
        end_win / end_lose / end_timeout."""
        c = self.c
        a = int(action)
        self.events = set()
        reward = 0
        self.ep_steps += 1
        if a == RIGHT:
            self.px = min(self.px + c.paddle_speed, 82 - c.paddle_width)
        elif a == LEFT:
            self.px = max(self.px - c.paddle_speed, 2)
        target = self.bx + 1 if (self.wait < 0 and self.vy < 0) else 42
        d = target - (self.ox + c.opponent_width // 2)
        self.ox = _clamp(self.ox + _clamp(d, -c.opponent_speed, c.opponent_speed), 2, 82 - c.opponent_width)
        if self.wait >= 0:
            if a == FIRE or (c.serve_wait > 0 and self.wait >= c.serve_wait):
                self.events.add("serve_fire" if a == FIRE else "serve_auto")
                self._serve()
            else:
                self.wait += 1
        else:
            for _ in range(c.ball_speed):
                r, point = self._micro_step()
                reward += r
                if point:
                    break
        terminal = self.mine >= c.points or self.theirs >= c.points or self.ep_steps >= c.max_episode_steps
        if terminal:
            self.events.add("end_win" if self.mine >= c.points else "end_lose" if self.theirs >= c.points else "end_timeout")
        self.success = terminal and self.mine >= c.points
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
    return [HostDuel(conf, actor_base + b, seed, frames=frames) for b in range(B)]


# ---- the traces the GPU test compares step by step (tests/test_duel_gpu.py); tests/test_duel_cpu.py checks on this model
# alone that they hold the events below -----------------------------------------------------------------------------------
TRACE_B, TRACE_STEPS, TRACE_FRAMES = 200, 300, 6       # actors, steps, actors whose frames and pixel change are compared
TRACE_SEED = 1                                         # key of the serve draws
TRACE_SETTINGS = [dict(game="duel"),
                  dict(game="duel", points=2, paddle_width=4, ball_speed=4, opponent_width=24, opponent_speed=8,
                       win_reward=7, lose_reward=-3),
                  dict(game="duel", points=1, paddle_width=24, ball_speed=1, serve_wait=0, opponent_width=4,
                       opponent_speed=1),
                  dict(game="duel", points=9, opponent_speed=0, opponent_width=4, paddle_width=24, paddle_speed=8,
                       ball_speed=3)]
EVERY_EVENT = {"wall_left", "wall_right", "paddle_0", "paddle_1", "paddle_2", "paddle_3", "opp_0", "opp_1", "opp_2", "opp_3",
               "point_won", "point_lost", "serve_fire", "serve_auto", "end_win", "end_lose", "end_timeout"}
# what each setting's random trace holds on this model: no random actor wins a match against the default or the wide,
# fast opponent (the second setting's never even loses a point to them); serve_wait = 0 never serves by itself;
# max_episode_steps is 5000 in all four, so the time-out comes from the scripted trace below
TRACE_EVENTS = [EVERY_EVENT - {"end_win", "end_timeout"}, EVERY_EVENT - {"end_win", "end_timeout", "point_won"},
                EVERY_EVENT - {"serve_auto", "end_timeout"}, EVERY_EVENT - {"end_timeout"}]


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each (arcade_model.trace_inputs' draw)."""
    rs = np.random.RandomState(100 * k + 1)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active


# a fifth trace: a policy that follows the ball (arcade_model.follow_ball) wins matches against a slow opponent; where the
# rally never ends the episode runs into max_episode_steps
SCRIPTED_SETTING = dict(game="duel", points=3, paddle_width=24, paddle_speed=8, ball_speed=4, serve_wait=0, opponent_speed=1,
                        max_episode_steps=300)
SCRIPTED_B, SCRIPTED_STEPS = 12, 320
SCRIPTED_EVENTS = {"end_win", "end_timeout", "point_won", "serve_fire"}
