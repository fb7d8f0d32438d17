"""Host models of the device arcade with `action_repeat` and `return_reward` (csrc/arcade.hip), written from the
rules under "An agent step" in include/unreal_hip.h, not from the kernel.  RepeatBreakout / RepeatDuel subclass the one-tick
models of tests/arcade_model.py and tests/duel_model.py and drive them tick by tick; `ep_steps`, `events`, the frame and the
pixel change are kept per agent step, so OracleTrainer(envs=...) and the helpers of the existing GPU tests accept them.

Cases the rules leave open are fixed HERE (DESIGN §7m lists them): the first tick always runs, also in an ended game (the
batch-1 environment stepped past a terminal: one tick per step); the check that stops the ticks is made after a whole tick
and looks at the state only, never at the step count; a step's events are the union of its ticks' events, and an ending is
named once, from the record after the last tick, in the one-tick models' order; `return_reward` is paid by the micro-step
that returns the ball, so it is in the tick's reward before the tick's later micro-steps; the frame of the states between
ticks is never drawn, so a ball that leaves and re-enters a row inside one step changes no pixel of it.

New events of a step: cut_short (fewer than action_repeat ticks ran), serve_and_fly (a serve and at least one flight tick),
lost_then_wait (a life or point lost, then a tick in which the ball waited), two_rewards (two ticks paid a reward),
returned (return_reward > 0 was paid)."""
import functools

import numpy as np

try:
    import arcade_model as AM
    import duel_model as DM
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM

NEW_EVENTS = {"cut_short", "serve_and_fly", "lost_then_wait", "two_rewards", "returned"}
_ENDINGS = ("end_lives", "end_clear", "end_win", "end_lose", "end_timeout")


class _Repeat(object):
    """The agent step around a one-tick model (mixed in before HostBreakout / HostDuel)."""

    def _tick(self, action):
        """One tick: the base model's process() without its frame -> the tick's reward (return_reward included)."""
        return self.BASE.process(self, action)[1]

    def _micro_step(self):
        """The base model's micro-step; a return off the agent's paddle (a new paddle_<segment> event: after a return the
        ball rises, and at a speed <= 4 it is not back on the paddle's line within the tick) also pays return_reward."""
        returns = len([e for e in self.events if e.startswith("paddle_")])
        reward, end = self.BASE._micro_step(self)
        if len([e for e in self.events if e.startswith("paddle_")]) > returns:
            reward += self.c.return_reward
            if self.c.return_reward > 0:
                self.events.add("returned")
        return reward, end

    def process(self, action, flag=0):
        """One agent step of up to action_repeat ticks, without the reset -> (state, reward, terminal, pixel change)."""
        c, a = self.c, int(action)
        steps, frames = self.ep_steps, self.frames
        self.frames = False                            # the states between ticks are not drawn
        events, reward, ticks, paying = set(), 0, 0, 0
        served = lost = False
        for _ in range(c.action_repeat):
            waiting = self.wait >= 0
            r = self._tick(a)
            ticks += 1
            reward += r
            paying += r != 0
            serves = bool(self.events & {"serve_fire", "serve_auto"})
            if served and not waiting:
                events.add("serve_and_fly")
            if lost and waiting and not serves:
                events.add("lost_then_wait")
            served |= serves
            lost |= bool(self.events & {"life_lost", "point_lost"})
            events |= self.events - set(_ENDINGS)
            if self.ended():
                break
        if ticks < c.action_repeat:
            events.add("cut_short")
        if paying >= 2:
            events.add("two_rewards")
        self.frames, self.ep_steps = frames, steps + 1
        terminal = self.ended() or self.ep_steps >= c.max_episode_steps
        if terminal:
            events.add(self.ending())
        self.success = terminal and self.won()
        self.events, self.ticks = events, ticks
        pc = None
        if self.frames:
            frame = self.render()
            pc = AM.pixel_change(frame, self.frame)
            self.frame = frame
            self.last_state = {'image': frame / 255.0}
        self.last_action, self.last_reward = a, reward
        return self.last_state, reward, terminal, pc


class RepeatBreakout(_Repeat, AM.HostBreakout):
    BASE = AM.HostBreakout

    def ended(self):
        return self.lives <= 0 or self.bricks == 0

    def won(self):
        return self.bricks == 0

    def ending(self):
        return "end_lives" if self.lives <= 0 else "end_clear" if self.bricks == 0 else "end_timeout"


class RepeatDuel(_Repeat, DM.HostDuel):
    BASE = DM.HostDuel

    def ended(self):
        return self.mine >= self.c.points or self.theirs >= self.c.points

    def won(self):
        return self.mine >= self.c.points

    def ending(self):
        return "end_win" if self.mine >= self.c.points else "end_lose" if self.theirs >= self.c.points else "end_timeout"


def model_class(conf):
    return RepeatDuel if conf.game == "duel" else RepeatBreakout


def host_batch(conf, B, seed, actor_base=0, frames=True):
    """The host models of the actors [actor_base, actor_base + B) of a device environment with key `seed`, each reset
    once as the environment's constructor does; OracleTrainer(envs=...) accepts them."""
    return [model_class(conf)(conf, actor_base + b, seed, frames=frames) for b in range(B)]


def frame_of(conf, record):
    """The frame of a record -> uint8 [84, 84, 3] (a frame is a function of the config and the record alone)."""
    m = model_class(conf)(conf, frames=False)
    rec = [int(v) for v in record]
    m.px, m.bx, m.by, m.vx, m.vy, m.wait = rec[:6]
    if conf.game == "duel":
        m.ox, m.mine, m.theirs = rec[6:9]
    else:
        m.lives, m.bricks = rec[6], (rec[7] & 0xFFFFFFFF) | (rec[8] & 0xFFFFFFFF) << 32
    return m.render()


# ---- the traces of tests/test_arcade_repeat_gpu.py and of the stand-alone check of the kernel's own functions on the CPU;
# tests/test_arcade_repeat_cpu.py checks on these models alone that they hold the events below ---------------------------------
TRACE_B, TRACE_STEPS, TRACE_FRAMES = 200, 300, 6       # actors, agent steps, actors whose frames and pixel change are compared
TRACE_SEED = 1
# random traces: per game k = 2, 4, 8; the second of each has return_reward > 0 at ball_speed = 4
TRACE_SETTINGS = [
    dict(action_repeat=2),
    dict(action_repeat=4, return_reward=3, rows=2, lives=2, paddle_width=12, ball_speed=4, row_rewards=(7, 1), life_reward=-1),
    dict(action_repeat=8, return_reward=1, rows=1, lives=1, paddle_width=24, ball_speed=1, serve_wait=0),
    dict(game="duel", action_repeat=2),
    dict(game="duel", action_repeat=4, return_reward=2, points=2, paddle_width=12, ball_speed=4, opponent_width=24,
         opponent_speed=8, win_reward=7, lose_reward=-3),
    dict(game="duel", action_repeat=8, return_reward=5, points=1, paddle_width=24, ball_speed=1, serve_wait=0,
         opponent_width=4, opponent_speed=1),
]
# scripted traces at k = 4: tests/arcade_model.py's and tests/duel_model.py's scripted settings with the paddle's and the
# ball's speed divided by four, so that a step moves them as far as there; 12 actors follow the ball
SCRIPTED_SETTINGS = [
    dict(action_repeat=4, return_reward=1, rows=1, paddle_width=24, paddle_speed=2, ball_speed=1, serve_wait=0, lives=5,
         max_episode_steps=300),
    dict(game="duel", action_repeat=4, return_reward=1, points=3, paddle_width=24, paddle_speed=2, ball_speed=1, serve_wait=0,
         opponent_speed=1, max_episode_steps=300),
]
SCRIPTED_B, SCRIPTED_STEPS = 12, 320


def trace_config(k):
    """ArcadeConfig of trace k: 0..5 the random ones, 6 and 7 the scripted ones."""
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**(TRACE_SETTINGS + SCRIPTED_SETTINGS)[k])


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each, active with probability 0.9."""
    rs = np.random.RandomState(1000 + k)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active


@functools.lru_cache(maxsize=None)
def run_trace(k):
    """Trace k on the models alone, computed once and shared (read-only) by the tests: the actors start in episode 0, step
    with reset on terminal, and after every agent step everything a device environment shows is recorded.  -> dict of
    acts, active [S, B]; records [S, B, 16]; reward, terminal (of the active actors; -7.5 / -7 elsewhere), count, ep_steps,
    episode, last_action, last_reward [S, B]; pc [S, F, 400] with pc_slot [S, F] (ring slot of the step's pixel change at
    H1 = 4; -1: idle) and pre_reset [S, F, 16] (the record the pixel change was made from, before a reset); events."""
    conf = trace_config(k)
    scripted = k >= len(TRACE_SETTINGS)
    B, S = (SCRIPTED_B, SCRIPTED_STEPS) if scripted else (TRACE_B, TRACE_STEPS)
    F = B if scripted else TRACE_FRAMES
    H1 = 4
    models = [model_class(conf)(conf, b, TRACE_SEED, frames=b < F) for b in range(B)]
    if scripted:
        acts, active = np.zeros((S, B), np.int32), np.ones((S, B), np.int32)
    else:
        acts, active = trace_inputs(k)
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
            acts[s] = [AM.follow_ball(m) for m in models]
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


# what each trace holds on the models (tests/test_arcade_repeat_cpu.py asserts it, and that together they hold every new
# event and every ending).  Random play clears no wall and wins no match against the default or the wide opponent, and
# max_episode_steps is 5000 in the random settings: those endings come from the scripted traces.
_BREAKOUT = {"wall_left", "wall_right", "brick_x", "brick_y", "paddle_0", "paddle_1", "paddle_2", "paddle_3", "life_lost",
             "end_lives", "serve_fire"}
_DUEL = {"wall_left", "wall_right", "paddle_0", "paddle_1", "paddle_2", "paddle_3", "opp_0", "opp_1", "opp_2", "opp_3",
         "point_lost", "serve_fire", "end_lose"}
_BOTH = {"cut_short", "serve_and_fly"}
TRACE_EVENTS = [
    _BREAKOUT | _BOTH | {"two_bricks", "serve_auto", "lost_then_wait", "two_rewards"},
    _BREAKOUT | _BOTH | {"two_bricks", "serve_auto", "lost_then_wait", "two_rewards", "returned", "wall_top"},
    _BREAKOUT | _BOTH | {"end_clear", "wall_top", "returned"},            # one life: nothing follows a lost one
    _DUEL | _BOTH | {"point_won", "end_win", "serve_auto", "lost_then_wait"},
    _DUEL | _BOTH | {"serve_auto", "lost_then_wait", "returned"},
    _DUEL | _BOTH | {"point_won", "end_win", "returned"},                 # one point: nothing follows a lost one
    _BOTH | {"end_clear", "end_timeout", "wall_top", "brick_y", "serve_fire", "returned"},
    _BOTH | {"end_win", "end_timeout", "point_won", "serve_fire", "returned"},
]
# two_rewards is Breakout's alone: in the duel a reward is a point or a return, and from either the ball needs more than the
# 32 micro-steps of a step (8 ticks at speed 4) to the next one (40 -> 78 after a serve, 78 -> 6 after a return).
EVERY_EVENT = NEW_EVENTS | _BREAKOUT | _DUEL | {"two_bricks", "serve_auto", "wall_top", "point_won", "end_clear", "end_win",
                                                "end_timeout"}
