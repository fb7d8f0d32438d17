"""Host model of the device arcade's crossing game (csrc/arcade.hip) in plain Python / numpy, written from the
rules in include/unreal_hip.h and the issue's text, not from the kernel: record, frame bytes, reward, terminal, pixel change,
and the agent step of `action_repeat` ticks.  Boxes are tested pixel by pixel here; the kernel uses a closed form.  It has
HostBreakout's interface (tests/arcade_model.py), so OracleTrainer(envs=...) accepts it.

Cases the rules leave open are fixed HERE (DESIGN §7x lists them):
  * "stunned" is the state at the start of the tick: a tick that starts with stun > 0 counts it down, moves no walker and
    tests neither a hit nor a crossing; the tick after the one that brings stun to 0 is the first that moves.  With
    serve_wait = 0 a walker that stays inside a car is hit again in the next tick;
  * the tick counter counts the ticks of the episode from 0, modulo 12 (every period divides 12); a lane moves in the ticks
    that START with a counter that is a multiple of its period, so every lane moves in the first tick of an episode;
  * the lanes move while the walker is stunned, and in steps past a terminal;
  * lanes l >= len(lanes) hold no traffic: they keep the offset of the reset draw, are never drawn and never hit;
  * a parked lane (speed 0) keeps its offset; offsets wrap modulo 128 in both directions;
  * a car hits where its box meets the walker's; parts of a car outside x 2..81 are not drawn, and the walker never
    leaves 2..81, so clipping changes no hit; a walker of 4 rows meets one lane at the most (lanes are 4 rows, 4 apart);
  * a hit and a crossing cannot fall in the same tick: the crossing needs py <= 6, rows <= 9, the top lane starts at row 12.
    The hit is tested first all the same;
  * the knock-back is py = min(py + knock_back, 76); px stays;
  * a crossing returns the walker to (42 - w / 2, 76) with stun 0; the episode's count is not capped, the score row draws
    min(count, 19) blocks; "target reached" is counted in the tick in which the count becomes `crossings`, once;
  * `terminal` names its ending in this order: target reached, step limit; without a reset on terminal the game goes on
    (the count runs past the target, `terminal` stays set), and an agent step then runs one tick;
  * a reset draws all eight offsets: lanes 0..3 from the bytes of u[0], lanes 4..7 from those of u[1], seven bits each;
  * draw order, front to back: walker, cars, score blocks, border; lane l's cars have Breakout's colour of brick row
    1 + l % 5 (never row 0's, which is the walker's)."""
import functools

import numpy as np

try:
    from maze_model import philox4x32_10
    from arcade_model import pixel_change, BORDER, WHITE, PADDLE, ROW_COLOURS, NOOP, FIRE, RIGHT, LEFT
except ImportError:            # imported as tests.<module>
    from tests.maze_model import philox4x32_10
    from tests.arcade_model import pixel_change, BORDER, WHITE, PADDLE, ROW_COLOURS, NOOP, FIRE, RIGHT, LEFT

LANE_STREAM = 0x43524F53          # counter word 2 of the reset's draw ("CROS")
FORWARD = FIRE                    # action 1
MAX_LANES, TRACK, SHIFT, START_Y, WALKER_H, MAX_BLOCKS = 8, 128, 22, 76, 4, 19


class HostCrossing(object):
    """One actor: global index g, the key `seed` of its reset draws.  Like the device environment its constructor resets
    once (episode 0); `events` collects what happened in the last agent step (names: see process)."""

    def __init__(self, config, g=0, seed=0, frames=True):
        self.c, self.g, self.seed, self.frames = config, int(g), int(seed) & (2 ** 64 - 1), frames
        self.px = self.py = self.stun = self.count = self.tick_counter = 0
        self.offsets = [0] * MAX_LANES
        self.totals = [0, 0, 0]           # crossings, hits, targets reached
        self.ep_steps, self.episode = 0, -1
        self.events = set()
        self.success = False
        self.frame = self.last_state = None
        self.reset()

    # ---- state -------------------------------------------------------------------------------------------------------
    def reset(self):
        c = self.c
        self.episode += 1
        self.px, self.py = 42 - c.paddle_width // 2, START_Y
        self.stun = self.count = self.tick_counter = 0
        u = philox4x32_10((self.g, self.episode, LANE_STREAM, 0), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        self.offsets = [(int(u[l // 4]) >> (8 * (l % 4))) & 127 for l in range(MAX_LANES)]
        self.ep_steps = 0
        self.last_action, self.last_reward = 0, 0
        if self.frames:
            self.frame = self.render()
            self.last_state = {'image': self.frame / 255.0}

    def record(self):
        words = [sum(self.offsets[4 * k + i] << (8 * i) for i in range(4)) for k in range(2)]
        rec = [self.px, self.py, self.stun, self.count, self.tick_counter] + words + [0, 0, 0] + self.totals + [0, 0, 0]
        return np.array(rec, dtype=np.int64).astype(np.uint32).view(np.int32)

    def car_columns(self, l):
        """Screen columns (unclipped, -22..105) the cars of lane l cover -> a set."""
        cars = self.c.lanes[l][0]
        cols = set()
        for k in range(cars):
            start = (self.offsets[l] + k * (TRACK // cars)) % TRACK
            cols |= set((start + i) % TRACK - SHIFT for i in range(self.c.car_length))
        return cols

    def render(self):
        c = self.c
        f = np.zeros((84, 84, 3), dtype=np.uint8)
        f[0:6, :] = BORDER
        f[:, 0:2] = BORDER
        f[:, 82:84] = BORDER
        for k in range(min(self.count, MAX_BLOCKS)):
            f[2:4, 4 + 4 * k:6 + 4 * k] = WHITE
        for l in range(len(c.lanes)):
            for x in self.car_columns(l):
                if 2 <= x <= 81:
                    f[12 + 8 * l:16 + 8 * l, x] = ROW_COLOURS[1 + l % 5]
        f[max(self.py, 0):max(self.py + WALKER_H, 0), self.px:self.px + c.paddle_width] = PADDLE
        return f

    # ---- rules -------------------------------------------------------------------------------------------------------
    def ended(self):
        return self.c.crossings > 0 and self.count >= self.c.crossings

    def _lane_met(self):
        """The lane with traffic whose rows the walker's rows meet, or -1."""
        rows = set(range(self.py, self.py + WALKER_H))
        met = [l for l in range(len(self.c.lanes)) if rows & set(range(12 + 8 * l, 16 + 8 * l))]
        assert len(met) <= 1
        return met[0] if met else -1

    def _note_cars(self):
        """Render cases the traces must hold: a car over the track's seam, a car clipped at either edge of the field."""
        c = self.c
        for l, (cars, _, _, _) in enumerate(c.lanes):
            for k in range(cars):
                start = (self.offsets[l] + k * (TRACK // cars)) % TRACK
                if start + c.car_length > TRACK:
                    self.events.add("seam")
                x0, x1 = start - SHIFT, start - SHIFT + c.car_length - 1
                if start + c.car_length <= TRACK:
                    if x0 < 2 <= x1:
                        self.events.add("clip_left")
                    if x0 <= 81 < x1:
                        self.events.add("clip_right")

    def tick(self, a):
        """One game tick with action a -> its reward.  Adds to self.events."""
        c, ev, reward = self.c, self.events, 0
        w = c.paddle_width
        # 1. walker
        stunned = self.stun > 0
        if stunned:
            self.stun -= 1
            ev.add("stunned")
            if a != NOOP:
                ev.add("stunned_action_ignored")
        elif a == FORWARD:
            self.py -= c.ball_speed
        elif a == RIGHT:
            if self.px + c.paddle_speed > 82 - w:
                ev.add("clamp_right")
            self.px = min(self.px + c.paddle_speed, 82 - w)
        elif a == LEFT:
            if self.px - c.paddle_speed < 2:
                ev.add("clamp_left")
            self.px = max(self.px - c.paddle_speed, 2)
        # 2. lanes
        for l, (cars, speed, period, direction) in enumerate(c.lanes):
            if self.tick_counter % period == 0:
                new = (self.offsets[l] + direction * speed) % TRACK
                if speed and direction > 0 and new < self.offsets[l]:
                    ev.add("wrap_up")
                if speed and direction < 0 and new > self.offsets[l]:
                    ev.add("wrap_down")
                self.offsets[l] = new
                if speed == 0:
                    ev.add("parked")
                if period == 4:
                    ev.add("period_4")
        self.tick_counter = (self.tick_counter + 1) % 12
        if self.frames:
            self._note_cars()
        # 3. hit, 4. crossing
        l = self._lane_met()
        if stunned:
            if l >= 0 and self.car_columns(l) & set(range(self.px, self.px + w)):
                ev.add("stunned_in_car")
            return reward
        inside = self.car_columns(l) & set(range(self.px - 1, self.px + w + 1)) if l >= 0 else set()
        walker = inside & set(range(self.px, self.px + w))
        if walker:
            assert self.py > 6
            if walker == {self.px}:
                ev.add("hit_first_column")
            if walker == {self.px + w - 1}:
                ev.add("hit_last_column")
            reward += c.hit_reward
            self.totals[1] += 1
            if self.py + c.knock_back > START_Y:
                ev.add("knock_clamped")
            self.py = min(self.py + c.knock_back, START_Y)
            self.stun = c.serve_wait
            ev.add("hit")
        else:
            if self.px - 1 in inside:
                ev.add("miss_left")
            if self.px + w in inside:
                ev.add("miss_right")
            if self.py <= 6:
                reward += c.cross_reward
                self.count += 1
                self.totals[0] += 1
                ev.add("crossing")
                if self.count == c.crossings:
                    self.totals[2] += 1
                    ev.add("target")
                if self.count > MAX_BLOCKS:
                    ev.add("blocks_capped")
                self.px, self.py = 42 - w // 2, START_Y
        return reward

    def process(self, action, flag=0):
        """One agent step of up to action_repeat ticks, without the reset (the caller resets at a terminal) -> (state,
        reward, terminal, pixel change).  The first tick always runs; the ticks stop after one that ends the game.
        events: stunned, stunned_action_ignored, stunned_in_car, clamp_left, clamp_right, wrap_up, wrap_down, parked,
        period_4, seam, clip_left, clip_right (the last three only with frames), hit, hit_first_column, hit_last_column,
        miss_left, miss_right, knock_clamped, crossing, target, blocks_capped, cut_short, end_target / end_timeout."""
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
            self.events.add("end_target" if self.ended() else "end_timeout")
        self.success = terminal and self.ended()
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


def _host_batch(conf, B, seed, actor_base=0, frames=True):
    """The host models of the actors [actor_base, actor_base + B) of a device environment with key `seed`, each reset
    once as the environment's constructor does; OracleTrainer(envs=...) accepts them."""
    return [HostCrossing(conf, actor_base + b, seed, frames=frames) for b in range(B)]


# Bound by assignment: tests/test_distributed_cpu.py lists, by the text of their definition, the model modules whose host_batch
# its shard comparison covers, and that list is closed.  tests/test_crossing_cpu.py makes the same comparison for this one.
host_batch = _host_batch


# ---- the traces the GPU test compares step by step (tests/test_crossing_gpu.py); tests/test_crossing_cpu.py checks on this
# model alone that they hold the events below -----------------------------------------------------------------------------
TRACE_B, TRACE_STEPS, TRACE_FRAMES = 200, 300, 6       # actors, steps, actors whose frames and pixel change are compared
TRACE_SEED = 1                                         # key of the reset draws
# fast one-car lanes, rewards of both signs.  Uniform random play moves forward in a quarter of its steps and a crossing
# takes 18 forward ticks at 4 px, so at one tick a step the limit that random play can reach the target of two crossings
# under is 150 steps, not 40; the 40 are the limit of the same setting at four ticks a step (REPEAT_SETTING)
FAST_LANES = [(1, 4, 1, 1), (1, 3, 1, -1), (1, 4, 2, 1), (1, 2, 1, -1)]
SHORT_SETTING = dict(game="crossing", paddle_width=4, knock_back=8, crossings=2, ball_speed=4, serve_wait=0, lanes=FAST_LANES,
                     cross_reward=5, hit_reward=-1, max_episode_steps=150)
TRACE_SETTINGS = [dict(game="crossing", paddle_width=4),
                  SHORT_SETTING,
                  dict(game="crossing", paddle_width=24, lanes=[(1, 1, 3, -1)], car_length=4, max_episode_steps=120),
                  dict(game="crossing", paddle_width=24, lanes=[(4, 4, 1, 1 - 2 * (l % 2)) for l in range(8)], car_length=16,
                       serve_wait=2, knock_back=16, hit_reward=-2)]
TRACE_EVENTS = {"hit", "crossing", "target", "end_target", "end_timeout", "stunned", "stunned_action_ignored", "clamp_left",
                "clamp_right", "wrap_up", "wrap_down", "seam", "clip_left", "clip_right", "knock_clamped"}
# what the short setting alone must reach under random play
SHORT_EVENTS = {"hit", "crossing", "target", "end_target", "end_timeout"}
REPEAT_SETTING = dict(SHORT_SETTING, action_repeat=4, max_episode_steps=40)
REPEAT_EVENTS = {"hit", "crossing", "target", "end_target", "end_timeout", "cut_short"}


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each (arcade_model.trace_inputs' draw)."""
    rs = np.random.RandomState(100 * k + 1)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active


# the scripted trace.  Lane 6 is parked with four 8-px cars 32 apart, lane 7 below it is fast, lane 0 moves every fourth
# tick.  Actor b first walks sideways until it stands where its kind wants it relative to a parked car of lane 6, then only
# forwards: a hit throws it back by 8 into lane 7's rows, where it is stunned under moving cars.
#   kind 0: the walker's last column one pixel left of the car (no hit)    kind 1: its last column on the car's first pixel
#   kind 2: its first column on the car's last pixel                       kind 3: its first column one right of it (no hit)
#   kind 4: left for ever (the clamp at 2)                                 kind 5: right for ever (the clamp at 82 - w)
SCRIPTED_LANES = [(1, 1, 4, 1), (2, 2, 1, -1), (1, 3, 1, 1), (2, 1, 2, -1), (1, 2, 1, 1), (1, 1, 1, -1), (4, 0, 1, 1),
                  (4, 4, 1, -1)]
SCRIPTED_SETTING = dict(game="crossing", paddle_width=4, paddle_speed=1, ball_speed=3, serve_wait=3, knock_back=8,
                        car_length=8, lanes=SCRIPTED_LANES, crossings=2, cross_reward=3, hit_reward=-1,
                        max_episode_steps=160)
SCRIPTED_B, SCRIPTED_STEPS, SCRIPTED_KINDS = 12, 340, 6
SCRIPTED_EVENTS = {"hit_first_column", "hit_last_column", "miss_left", "miss_right", "knock_clamped", "stunned_in_car",
                   "stunned_action_ignored", "parked", "period_4", "clamp_left", "clamp_right", "crossing", "target",
                   "end_target", "end_timeout", "wrap_up", "wrap_down", "seam", "clip_left", "clip_right"}
# the runner: one parked car; the walker steps aside if it stands below it and walks up for ever: 21 crossings, past the 19
# score blocks
RUNNER_SETTING = dict(game="crossing", paddle_width=4, paddle_speed=4, ball_speed=4, lanes=[(1, 0, 1, 1)], car_length=4,
                      crossings=21, max_episode_steps=5000)
RUNNER_B, RUNNER_STEPS = 3, 400
RUNNER_EVENTS = {"blocks_capped", "target", "end_target", "parked"}


def _parked_car(m, lane, lo, hi):
    """Screen x of the first pixel of a car of parked lane `lane` that lies in [lo, hi]."""
    cars = m.c.lanes[lane][0]
    starts = [(m.offsets[lane] + k * (TRACK // cars)) % TRACK - SHIFT for k in range(cars)]
    return min(x for x in starts if lo <= x <= hi)


def scripted_action(m, b):
    """The scripted policy of actor b (see SCRIPTED_SETTING)."""
    kind, w = b % SCRIPTED_KINDS, m.c.paddle_width
    if kind == 4:
        return LEFT
    if kind == 5:
        return RIGHT
    cx = _parked_car(m, 6, 2 + w, 70)                  # (the cars are 32 apart: one starts in any 32 columns)
    target = (cx - w, cx - w + 1, cx + m.c.car_length - 1, cx + m.c.car_length)[kind]
    if m.py == START_Y and m.px != target:
        return RIGHT if m.px < target else LEFT
    return FORWARD


def runner_action(m, b):
    """Step aside while the parked car stands above the walker (or one pixel beside it), else forwards."""
    if m.py == START_Y and m.car_columns(0) & set(range(m.px - 1, m.px + m.c.paddle_width + 1)):
        return RIGHT
    return FORWARD


# ---- the traces on the model alone, computed once and shared (read-only) by tests/test_crossing_cpu.py,
# tests/test_crossing_gpu.py and tools/check_arcade_host.py ---------------------------------------------------------------------
N_TRACES = 7                   # 0..3: the random settings; 4: the short one at four ticks a step; 5: scripted; 6: the runner
SCRIPTS = {5: (SCRIPTED_B, SCRIPTED_STEPS, scripted_action), 6: (RUNNER_B, RUNNER_STEPS, runner_action)}


def trace_config(k):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**(TRACE_SETTINGS + [REPEAT_SETTING, SCRIPTED_SETTING, RUNNER_SETTING])[k])


def frame_of(conf, record):
    """The frame of a record -> uint8 [84, 84, 3] (a frame is a function of the config and the record alone)."""
    m = HostCrossing(conf, frames=False)
    rec = [int(v) for v in record]
    m.px, m.py, m.stun, m.count, m.tick_counter = rec[:5]
    m.offsets = [((rec[5 + l // 4] & 0xFFFFFFFF) >> (8 * (l % 4))) & 127 for l in range(MAX_LANES)]
    return m.render()


@functools.lru_cache(maxsize=None)
def run_trace(k):
    """Trace k: the actors start in episode 0 and step with reset on terminal; after every agent step everything a device
    environment shows is recorded (the layout of tests/invaders_model.run_trace).  -> dict of acts, active [S, B]; records
    [S, B, 16]; reward, terminal (of the active actors; -7.5 / -7 elsewhere), count, ep_steps, episode, last_action,
    last_reward [S, B]; pc [S, F, 400] with pc_slot [S, F] (ring slot of the step's pixel change at H1 = 4; -1: idle) and
    pre_reset [S, F, 16] (the record the pixel change was made from, before a reset); events."""
    conf = trace_config(k)
    scripted = k in SCRIPTS
    B, S, policy = SCRIPTS[k] if scripted else (TRACE_B, TRACE_STEPS, None)
    F = B if scripted else TRACE_FRAMES
    H1 = 4
    models = [HostCrossing(conf, b, TRACE_SEED, frames=b < F) for b in range(B)]
    if scripted:
        acts, active = np.zeros((S, B), np.int32), np.ones((S, B), np.int32)
    else:
        acts, active = trace_inputs(1 if k == 4 else k)
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
            acts[s] = [policy(m, b) for b, m in enumerate(models)]
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


# ---- random play and "always forward" on the model (DESIGN §7x's table; python tests/crossing_model.py) ----------------------
def play(policy, knock_back, paddle_width, episodes=1000, steps=2000, seed=0):
    """-> (crossings per episode, share of episodes without a crossing) of `episodes` timed episodes of `steps` steps of the
    default lanes: policy "random" (uniform over the four actions) or "forward"."""
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    conf = ArcadeConfig(game="crossing", paddle_width=paddle_width, knock_back=knock_back, max_episode_steps=steps)
    rs = np.random.RandomState(seed)
    total, none = 0, 0
    for e in range(episodes):
        m = HostCrossing(conf, e, seed, frames=False)
        acts = rs.randint(0, 4, steps) if policy == "random" else np.full(steps, FORWARD)
        for a in acts:
            m.tick(int(a))
        total += m.count
        none += m.count == 0
    return total / float(episodes), none / float(episodes)


if __name__ == "__main__":
    import sys
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    for policy in ("random", "forward"):
        for w in (4, 12):
            for kb in (8, 16, 70):
                per, none = play(policy, kb, w, episodes=n)
                print("policy=%s paddle_width=%d knock_back=%d episodes=%d crossings_per_episode=%.3f no_crossing=%.3f"
                      % (policy, w, kb, n, per, none))
