"""Host model of the device arcade's invaders game (csrc/arcade.hip) in plain Python / numpy, written from the
rules in include/unreal_hip.h and the issue's text, not from the kernel: record, frame bytes, reward, terminal, pixel
change, and the agent step of `action_repeat` ticks.  It has HostBreakout's interface (tests/arcade_model.py), so
OracleTrainer(envs=...) accepts it.

Cases the rules leave open are fixed HERE (DESIGN §7n lists them):
  * a shot fired in a tick makes its micro-steps in that same tick (the tick order is taken literally); it is tested only
    after a micro-step, never where it starts; fire while a shot flies is a noop; a removed shot has sx = sy = 0, and sy = 0
    is "no shot" (a shot in flight has 6 <= sy <= 76);
  * a shot is removed by the micro-step that takes its box above y = 6 (sy < 6), before the alien test of that micro-step;
  * the march counter counts ticks from 0 and the grid moves in the tick in which it reaches march_period; the edge test is
    on the grid's origin (gx + 2 dir outside 2..20), whatever columns still live; a descent does not move gx; gy stops at 84
    (a game stepped on past its end keeps marching: the grid leaves the frame and stays there);
  * bombs move in slot order, each making all its micro-steps before the next; a bomb is removed by the micro-step that
    takes its box below y = 83 (y + 1 > 83), before the cannon test of that micro-step; the cannon test is on boxes
    ([x, x+1] meets [px, px+w-1] and [y, y+1] meets [78, 79]) and is made only after a bomb's micro-step, so a cannon that
    moves under a bomb is hit in the next tick; the hit ends the tick's bomb moves;
  * a hit sets the grace to serve_wait + 1: step 5 of the same tick uses up the one, so no bomb is dropped in the tick of the
    hit nor in the serve_wait ticks after it; a reset sets it to serve_wait;
  * step 5: the grace counter, if > 0, goes down by one and forbids the drop; the bomb counter counts every tick and returns
    to 0 in the tick in which it reaches bomb_period, whether or not a bomb is dropped; a drop refused (grace, no alien, no
    free slot) makes no draw, so the draw index counts bombs dropped; the bomb takes the first free slot;
  * the column is cols[u[0] % len(cols)] of the ascending list of columns with a live alien; the bomb starts at
    (gx + 8 c + 2, gy + 6 r + 4) below the lowest live alien (r, c) of that column and first moves in the next tick;
  * the invasion test is made in step 6 of a tick that marched, only while lives > 0 and an alien lives: life_reward is
    paid once, the lives-lost total grows by the lives left, lives = 0;
  * a cleared wave (counted when the last alien goes) does not stop the rest of the tick: bombs in flight still fall and can
    take a life in that tick;
  * `terminal` names its ending in this order: wave cleared, no lives (an invasion included), step limit; without a reset
    on terminal the game goes on (lives fall below 0, no alien is left to shoot, `terminal` stays set), and an agent step
    then runs one tick;
  * draw order, front to back: shot, bombs (slot 0 in front), cannon, aliens, life blocks, border."""
import functools

import numpy as np

try:
    from maze_model import philox4x32_10
    from arcade_model import pixel_change, BORDER, WHITE, PADDLE, ROW_COLOURS, NOOP, FIRE, RIGHT, LEFT
except ImportError:            # imported as tests.<module>
    from tests.maze_model import philox4x32_10
    from tests.arcade_model import pixel_change, BORDER, WHITE, PADDLE, ROW_COLOURS, NOOP, FIRE, RIGHT, LEFT

BOMB_STREAM = 0x494E5642          # counter word 2 of a bomb draw ("INVB")
BOMB = (214, 214, 92)
COLS, MAX_BOMBS = 8, 3


class HostInvaders(object):
    """One actor: global index g, the key `seed` of its bomb draws.  Like the device environment its constructor resets
    once (episode 0); `events` collects what happened in the last agent step (names: see process)."""

    def __init__(self, config, g=0, seed=0, frames=True):
        self.c, self.g, self.seed, self.frames = config, int(g), int(seed) & (2 ** 64 - 1), frames
        self.px = self.sx = self.sy = self.gx = self.gy = self.dir = self.lives = 0
        self.mask = 0
        self.march = self.bomb = self.grace = 0
        self.bombs = [None] * MAX_BOMBS
        self.draw_index = 0
        self.totals = [0, 0, 0]           # aliens shot, lives lost, waves cleared
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
        self.sx = self.sy = 0
        self.gx, self.gy, self.dir = 10, 10, 1
        self.lives = c.lives
        self.mask = (1 << (COLS * c.alien_rows)) - 1
        self.march = self.bomb = 0
        self.grace = c.serve_wait
        self.bombs = [None] * MAX_BOMBS
        self.draw_index, self.ep_steps = 0, 0
        self.last_action, self.last_reward = 0, 0
        if self.frames:
            self.frame = self.render()
            self.last_state = {'image': self.frame / 255.0}

    def record(self):
        rec = [self.px, self.sx, self.sy, self.gx, self.gy, self.dir, self.lives, self.mask,
               self.march | self.bomb << 8 | self.grace << 16, self.draw_index] + self.totals + \
              [0 if b is None else b[0] | b[1] << 8 for b in self.bombs]
        return np.array(rec, dtype=np.int64).astype(np.uint32).view(np.int32)

    def render(self):
        c = self.c
        f = np.zeros((84, 84, 3), dtype=np.uint8)
        f[0:6, :] = BORDER
        f[:, 0:2] = BORDER
        f[:, 82:84] = BORDER
        for k in range(self.lives):
            f[2:4, 4 + 4 * k:6 + 4 * k] = WHITE
        for r in range(c.alien_rows):
            for col in range(COLS):
                if (self.mask >> (COLS * r + col)) & 1:
                    f[self.gy + 6 * r:self.gy + 6 * r + 4, self.gx + 8 * col:self.gx + 8 * col + 6] = ROW_COLOURS[r]
        f[78:80, self.px:self.px + c.paddle_width] = PADDLE
        for b in reversed(self.bombs):
            if b is not None:
                f[b[1]:b[1] + 2, b[0]:b[0] + 2] = BOMB
        if self.sy:
            f[self.sy:self.sy + 2, self.sx:self.sx + 2] = WHITE
        return f

    # ---- rules -------------------------------------------------------------------------------------------------------
    def _alien_at(self, x, y):
        """The live alien with the lowest bit that the 2 x 2 box at (x, y) overlaps, or -1."""
        best = -1
        for yy in (y, y + 1):
            for xx in (x, x + 1):
                rx, ry = xx - self.gx, yy - self.gy
                if 0 <= rx < 8 * COLS and 0 <= ry < 6 * self.c.alien_rows and rx % 8 < 6 and ry % 6 < 4:
                    bit = COLS * (ry // 6) + rx // 8
                    if (self.mask >> bit) & 1 and (best < 0 or bit < best):
                        best = bit
        return best

    def lowest_row(self):
        """Row of the lowest live alien, or -1."""
        return (self.mask.bit_length() - 1) // COLS if self.mask else -1

    def ended(self):
        return self.lives <= 0 or self.mask == 0

    def _drop(self):
        cols = [col for col in range(COLS) if any((self.mask >> (COLS * r + col)) & 1 for r in range(self.c.alien_rows))]
        u = philox4x32_10((self.g, self.episode, BOMB_STREAM, self.draw_index), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        col = cols[int(u[0]) % len(cols)]
        row = max(r for r in range(self.c.alien_rows) if (self.mask >> (COLS * r + col)) & 1)
        self.draw_index += 1
        self.last_drop = (row, col)
        return (self.gx + 8 * col + 2, self.gy + 6 * row + 4)

    def tick(self, a):
        """One game tick with action a -> its reward.  Adds to self.events."""
        c, ev, reward = self.c, self.events, 0
        # 1. cannon
        if a == RIGHT:
            self.px = min(self.px + c.paddle_speed, 82 - c.paddle_width)
        elif a == LEFT:
            self.px = max(self.px - c.paddle_speed, 2)
        elif a == FIRE:
            if self.sy == 0:
                self.sx, self.sy = self.px + c.paddle_width // 2 - 1, 76
                ev.add("fire")
            else:
                ev.add("fire_ignored")
        # 2. shot
        if self.sy:
            for _ in range(c.ball_speed):
                self.sy -= 1
                if self.sy < 6:
                    self.sx = self.sy = 0
                    ev.add("shot_out")
                    break
                bit = self._alien_at(self.sx, self.sy)
                if bit >= 0:
                    self.mask &= ~(1 << bit)
                    self.totals[0] += 1
                    reward += c.alien_rewards[bit // COLS]
                    ev.add("alien_shot")
                    if self.mask == 0:
                        self.totals[2] += 1
                        ev.add("wave_cleared")
                    self.sx = self.sy = 0
                    break
        # 3. march
        marched = False
        self.march += 1
        if self.march >= c.march_period:
            self.march, marched = 0, True
            nx = self.gx + 2 * self.dir
            if nx < 2 or nx > 20:
                self.gy = min(self.gy + c.descend, 84)
                self.dir = -self.dir
                ev.add("descent")
            else:
                self.gx = nx
        # 4. bombs
        for k in range(MAX_BOMBS):
            if self.bombs[k] is None:
                continue
            x, y = self.bombs[k]
            hit = False
            for _ in range(c.bomb_speed):
                y += 1
                if y + 1 > 83:
                    ev.add("floor")
                    x = None
                    break
                if y + 1 >= 78 and y <= 79 and x + 1 >= self.px and x <= self.px + c.paddle_width - 1:
                    hit = True
                    break
            if hit:
                self.lives -= 1
                self.totals[1] += 1
                reward += c.life_reward
                self.sx = self.sy = 0
                self.bombs = [None] * MAX_BOMBS
                self.grace = c.serve_wait + 1
                ev.add("life_lost")
                break
            self.bombs[k] = None if x is None else (x, y)
        # 5. drop
        graced = self.grace > 0
        if graced:
            self.grace -= 1
        self.bomb += 1
        if self.bomb >= c.bomb_period:
            self.bomb = 0
            if graced:
                ev.add("drop_graced")
            elif self.mask:
                if None in self.bombs:
                    self.bombs[self.bombs.index(None)] = self._drop()
                    ev.add("drop")
                else:
                    ev.add("drop_refused")
        # 6. invasion
        if marched and self.lives > 0 and self.mask and self.gy + 6 * self.lowest_row() + 3 >= 76:
            reward += c.life_reward
            self.totals[1] += self.lives
            self.lives = 0
            ev.add("invasion")
        return reward

    def process(self, action, flag=0):
        """One agent step of up to action_repeat ticks, without the reset (the caller resets at a terminal) -> (state,
        reward, terminal, pixel change).  The first tick always runs; the ticks stop after one that ends the game.
        events: fire, fire_ignored, shot_out, alien_shot, wave_cleared, descent, floor, life_lost, drop, drop_graced,
        drop_refused, invasion, cut_short, end_clear / end_lives / end_timeout."""
        c, a = self.c, int(action)
        self.events = set()
        reward, ticks = 0, 0
        self.ep_steps += 1
        for _ in range(c.action_repeat):
            reward += self.tick(a)
            ticks += 1
            if self.ended():
                break
        if ticks < c.action_repeat:
            self.events.add("cut_short")
        self.ticks = ticks
        terminal = self.ended() or self.ep_steps >= c.max_episode_steps
        if terminal:
            self.events.add("end_clear" if self.mask == 0 else "end_lives" if self.lives <= 0 else "end_timeout")
        self.success = terminal and self.mask == 0
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
    return [HostInvaders(conf, actor_base + b, seed, frames=frames) for b in range(B)]


# ---- the traces the GPU test compares step by step (tests/test_invaders_gpu.py); tests/test_invaders_cpu.py checks on this
# model alone that they hold the events below -----------------------------------------------------------------------------
TRACE_B, TRACE_STEPS, TRACE_FRAMES = 200, 300, 6       # actors, steps, actors whose frames and pixel change are compared
TRACE_SEED = 1                                         # key of the bomb draws
TRACE_SETTINGS = [dict(game="invaders"),
                  dict(game="invaders", alien_rows=1, lives=2, paddle_width=4, ball_speed=4, bomb_period=2, bomb_speed=4,
                       march_period=1, descend=8, serve_wait=0, alien_rewards=(7,), life_reward=-1),
                  dict(game="invaders", alien_rows=4, paddle_width=24, ball_speed=1, bomb_period=64, march_period=16)]
# what the three random traces hold together, and what the scripted one holds (asserted on the model by the CPU test)
TRACE_EVENTS = {"alien_shot", "life_lost", "floor", "descent", "drop_refused", "fire", "fire_ignored", "shot_out", "drop",
                "drop_graced"}
# the random trace of the small setting at four ticks per agent step
REPEAT_SETTING = dict(TRACE_SETTINGS[1], action_repeat=4)
REPEAT_EVENTS = {"alien_shot", "life_lost", "floor", "descent", "drop_refused", "cut_short", "invasion", "end_lives"}


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each (arcade_model.trace_inputs' draw)."""
    rs = np.random.RandomState(100 * k + 1)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active


# the scripted trace: two rows that march every second tick.  Actor b sweeps under the grid and fires whenever the shot
# would hit (b % 3 == 0: it clears the wave), does nothing (b % 3 == 1: the grid reaches the cannon's rows after 292 ticks),
# or shoots the lower row only and then stands still (b % 3 == 2: the upper row would need 312 ticks; the step limit of 300
# comes first).
SCRIPTED_SETTING = dict(game="invaders", alien_rows=2, lives=5, paddle_width=12, paddle_speed=2, ball_speed=4, bomb_period=64,
                        march_period=2, descend=4, serve_wait=0, life_reward=-1, max_episode_steps=300)
SCRIPTED_B, SCRIPTED_STEPS = 12, 330
SCRIPTED_EVENTS = {"end_clear", "wave_cleared", "invasion", "end_lives", "end_timeout", "alien_shot"}


def _would_hit(m):
    """Would a shot fired now hit an alien, with no further action?  Played on a copy of the model."""
    t = HostInvaders.__new__(HostInvaders)
    t.__dict__.update(m.__dict__)
    t.totals, t.bombs, t.events, t.frames = list(m.totals), [None] * MAX_BOMBS, set(), False
    t.tick(FIRE)
    for _ in range(24):
        if t.sy == 0:
            break
        t.tick(NOOP)
    return t.totals[0] > m.totals[0]


def sweep_and_fire(m, b):
    """The scripted policy of actor b (see SCRIPTED_SETTING)."""
    kind = b % 3
    if kind == 1 or m.mask == 0 or (kind == 2 and m.mask >> COLS == 0):
        return NOOP
    if m.sy == 0 and _would_hit(m):
        return FIRE
    # sweep: to the right in even episodes of 40 steps, to the left in odd ones
    lo, hi = 2, 82 - m.c.paddle_width
    right = (m.ep_steps // ((hi - lo) // m.c.paddle_speed + 1)) % 2 == 0
    return RIGHT if right else LEFT


# ---- the traces on the model alone, computed once and shared (read-only) by tests/test_invaders_cpu.py,
# tests/test_invaders_gpu.py and tools/check_arcade_host.py ---------------------------------------------------------------------
N_TRACES = 5                   # 0..2: the random settings; 3: the small one at four ticks a step; 4: the scripted one


def trace_config(k):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**(TRACE_SETTINGS + [REPEAT_SETTING, SCRIPTED_SETTING])[k])


def frame_of(conf, record):
    """The frame of a record -> uint8 [84, 84, 3] (a frame is a function of the config and the record alone)."""
    m = HostInvaders(conf, frames=False)
    rec = [int(v) for v in record]
    m.px, m.sx, m.sy, m.gx, m.gy, m.dir, m.lives = rec[:7]
    m.mask = rec[7] & 0xFFFFFFFF
    m.bombs = [None if w == 0 else (w & 255, w >> 8) for w in rec[13:16]]
    return m.render()


@functools.lru_cache(maxsize=None)
def run_trace(k):
    """Trace k: the actors start in episode 0 and step with reset on terminal; after every agent step everything a device
    environment shows is recorded (the layout of tests/repeat_model.run_trace).  -> dict of acts, active [S, B]; records
    [S, B, 16]; reward, terminal (of the active actors; -7.5 / -7 elsewhere), count, ep_steps, episode, last_action,
    last_reward [S, B]; pc [S, F, 400] with pc_slot [S, F] (ring slot of the step's pixel change at H1 = 4; -1: idle) and
    pre_reset [S, F, 16] (the record the pixel change was made from, before a reset); events."""
    conf = trace_config(k)
    scripted = k == 4
    B, S = (SCRIPTED_B, SCRIPTED_STEPS) if scripted else (TRACE_B, TRACE_STEPS)
    F = B if scripted else TRACE_FRAMES
    H1 = 4
    models = [HostInvaders(conf, b, TRACE_SEED, frames=b < F) for b in range(B)]
    if scripted:
        acts, active = np.zeros((S, B), np.int32), np.ones((S, B), np.int32)
    else:
        acts, active = trace_inputs(1 if k == 3 else k)
    out = dict(acts=acts, active=active, records=np.zeros((S, B, 16), np.int32),
               reward=np.full((S, B), -7.5, np.float32), terminal=np.full((S, B), -7, np.int32),
               pc=np.zeros((S, F, 400), np.float32), pc_slot=np.full((S, F), -1, np.int64),
               pre_reset=np.zeros((S, F, 16), np.int32))
    for name in ("count", "ep_steps", "episode", "last_action"):
        out[name] = np.zeros((S, B), np.int64)
    out["last_reward"] = np.zeros((S, B), np.float32)
    count, prev_term, seen = np.zeros(B, np.int64), np.zeros(B, bool), set()
    for s in range(S):
        if scripted:
            acts[s] = [sweep_and_fire(m, b) for b, m in enumerate(models)]
        for b, m in enumerate(models):
            if active[s, b]:
                _, r, t, pc = m.process(acts[s, b])
                seen |= m.events
                out["reward"][s, b], out["terminal"][s, b] = r, int(t)
                if b < F:
                    out["pc"][s, b], out["pc_slot"][s, b] = pc.reshape(-1), b * H1 + count[b] % H1
                    out["pre_reset"][s, b] = m.record()
                if not (t and count[b] > 0 and prev_term[b]):
                    count[b] += 1
                prev_term[b] = t
                if t:
                    m.reset()
            out["records"][s, b] = m.record()
            out["ep_steps"][s, b], out["episode"][s, b] = m.ep_steps, m.episode
            out["last_action"][s, b], out["last_reward"][s, b] = m.last_action, m.last_reward
        out["count"][s] = count
    out["events"] = frozenset(seen)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
