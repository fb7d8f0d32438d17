"""Scripted traces of time-limit bootstrapping, shared by tests/test_timelimit_cpu.py (which checks on the host
models alone that every trace holds the cases it is there for) and tests/test_timelimit_gpu.py (which steps the device
through them).  Host truth: the models of tests/repeat_model.py (Breakout and the duel at any action_repeat),
tests/invaders_model.py, tests/nav_maze_model.py and tests/forage_maze_model.py, imported and not edited.

A step's FLAG is what the kernels commit to r_terminal / out_terminal / terminal_end with the final-observation store on:
0 no end, 1 a true end (the game or the maze's own rules end the episode, also in the step that reaches the limit),
2 a truncation (the step limit alone).  The kinds a trace is asked to hold: "true" (flag 1 before the limit), "cut"
(flag 2), "both" (flag 1 in the very step that reaches the limit: the coincidence)."""
import numpy as np

try:
    import repeat_model as RM
    import invaders_model as IM
    import nav_maze_model as NM
    import forage_maze_model as FM
except ImportError:            # imported as tests.<module>
    from tests import repeat_model as RM
    from tests import invaders_model as IM
    from tests import nav_maze_model as NM
    from tests import forage_maze_model as FM

B, STEPS, SEED = 6, 40, 1
NOOP, FIRE, RIGHT, LEFT = 0, 1, 2, 3

# ---- arcade -------------------------------------------------------------------------------------------------------------
# The anchor (verified by test_timelimit_cpu): Breakout with one row, one life, a 4-px paddle, a fast ball and no
# self-serve.  An actor that fires on its first step and then holds RIGHT loses its only life at step 12; one that never
# fires ends only at the limit.
BREAKOUT = dict(rows=1, lives=1, paddle_width=4, ball_speed=4, serve_wait=0)
DUEL = dict(game="duel", points=1, paddle_width=4, ball_speed=4, serve_wait=0)
INVADERS = dict(game="invaders", lives=1, serve_wait=0, bomb_period=1, bomb_speed=4, paddle_width=24)


def fire_right(m):
    return FIRE if m.ep_steps == 0 else RIGHT


def idle(m):
    return NOOP


EVEN_FIRE = (fire_right, idle) * 3          # actors 0, 2, 4 play, actors 1, 3, 5 never serve
ALL_IDLE = (idle,) * 6

# (name, settings, script of every actor, the kinds the trace must hold)
ARCADE_CASES = [
    ("breakout-20", dict(BREAKOUT, max_episode_steps=20), EVEN_FIRE, {"true", "cut"}),      # true ends at 12, cuts at 20
    ("breakout-12", dict(BREAKOUT, max_episode_steps=12), EVEN_FIRE, {"both", "cut"}),      # the coincidence
    ("breakout-9", dict(BREAKOUT, max_episode_steps=9), EVEN_FIRE, {"cut"}),                # both kinds of actor are cut
    ("breakout-x3-6", dict(BREAKOUT, action_repeat=3, max_episode_steps=6), EVEN_FIRE, {"true", "cut"}),
    ("breakout-x3-4", dict(BREAKOUT, action_repeat=3, max_episode_steps=4), EVEN_FIRE, {"both", "cut"}),
    ("duel-15", dict(DUEL, max_episode_steps=15), EVEN_FIRE, {"true", "cut"}),              # points at 10 and 12
    ("duel-10", dict(DUEL, max_episode_steps=10), EVEN_FIRE, {"both", "cut"}),
    ("duel-x3-6", dict(DUEL, action_repeat=3, max_episode_steps=6), EVEN_FIRE, {"true", "cut"}),
    ("duel-x3-4", dict(DUEL, action_repeat=3, max_episode_steps=4), EVEN_FIRE, {"both", "cut"}),
    ("invaders-20", dict(INVADERS, max_episode_steps=20), ALL_IDLE, {"true", "cut"}),       # bombs hit at 14 / 15 / 29
    ("invaders-15", dict(INVADERS, max_episode_steps=15), ALL_IDLE, {"true", "both", "cut"}),
    ("invaders-x3-8", dict(INVADERS, action_repeat=3, max_episode_steps=8), ALL_IDLE, {"true", "cut"}),
]
ARCADE_NAMES = [c[0] for c in ARCADE_CASES]


def arcade_config(settings):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**settings)


def arcade_models(conf, n, seed=SEED, actor_base=0):
    """Host models of a device environment built and reset once more (episode 1), as the GPU tests' environments are."""
    batch = IM.host_batch if conf.game == "invaders" else RM.host_batch
    models = batch(conf, n, seed, actor_base=actor_base)
    for m in models:
        m.reset()
    return models


def arcade_flag(m, terminal):
    return 0 if not terminal else 2 if "end_timeout" in m.events else 1


# ---- first-person mazes, N = 7 --------------------------------------------------------------------------------------------
# every layout: the start in the top-left corner, heading +x (start_heading 0), a free top row.  Actions: 0 turn left,
# 2 step forward.
FORWARD, TURN = 2, 0
_REST = "-------" * 5 + "A------"       # an apple far from the top row makes the block a navigation block
NAV_LAYOUTS = ["S----G-" + _REST,       # the goal is reached in step 5
               "S--G---" + _REST]       # ... in step 3
NAV_KW = dict(view="first_person", start_heading=0, max_episode_steps=5)
_PICK = "-------" * 6
# B: a lemon, C: a small good one, D: the melon, which ends the episode
KINDS = [(-1, (255, 255, 0), False), (5, (0, 255, 255), False), (20, (255, 0, 255), True)]
FORAGE_LAYOUTS = ["S--D--G" + _PICK,    # the melon ends the episode at step 3
                  "S-BC--G" + _PICK,    # two pickups that end nothing: cut at step 5
                  "S----DG" + _PICK]    # the melon in the step that reaches the limit


def forward(m):
    return FORWARD


def turn(m):
    return TURN


WALKERS = (forward, turn, forward, forward, turn, forward)      # (by actor: actors 1 and 4 never leave their cell)

# (name, MazeConfig arguments, host models, script of every actor, the kinds the trace must hold)
MAZE_CASES = [
    # with goal_respawn a goal is no end: the walkers are cut at step 5, one of them standing on the goal it has just reached
    ("nav-respawn", (NAV_LAYOUTS, dict(NAV_KW, goal_respawn=True)), "nav", WALKERS, {"cut", "goal-cut"}),
    # without it the same step is a true end
    ("nav-plain", (NAV_LAYOUTS, dict(NAV_KW)), "nav", WALKERS, {"true", "both", "cut"}),
    ("forage", (FORAGE_LAYOUTS, dict(NAV_KW, pickups=KINDS)), "forage", (forward, turn) * 3, {"true", "both", "cut"}),
]
MAZE_NAMES = [c[0] for c in MAZE_CASES]


def maze_config(args):
    from unreal_amd.environment.maze_environment import MazeConfig
    layouts, kw = args
    return MazeConfig(list(layouts), **kw)


def maze_models(conf, kind, n, seed=SEED, actor_base=0, actors_total=None):
    batch = FM.host_batch if kind == "forage" else NM.host_batch
    models = batch(conf, n, actor_base=actor_base, actors_total=n if actors_total is None else actors_total, seed=seed)
    for m in models:
        m.reset()
    return models


def maze_flag(m, terminal):
    return 0 if not terminal else 2 if m.timed_out else 1


# ---- the host side of a trace ----------------------------------------------------------------------------------------------
def host_trace(models, scripts, flag_of, limit, steps=STEPS):
    """Drive the models by their scripts, resetting at every end -> dict of
    actions, flags, rewards [steps, n]; final {(step, actor): the uint8 frame the limit cut off}; kinds: the set seen."""
    n = len(models)
    actions, flags = np.zeros((steps, n), np.int32), np.zeros((steps, n), np.int32)
    rewards = np.zeros((steps, n), np.float32)
    final, kinds = {}, set()
    for s in range(steps):
        for b, m in enumerate(models):
            a = scripts[b](m)
            _, r, t, _ = m.process(a)
            f = flag_of(m, t)
            actions[s, b], flags[s, b], rewards[s, b] = a, f, r
            if f == 2:
                final[(s, b)] = m.frame.copy()
                kinds.add("cut")
                if getattr(m, "at_goal", False):
                    kinds.add("goal-cut")
            elif f == 1:
                kinds.add("both" if m.ep_steps >= limit else "true")
            if t:
                m.reset()
    return dict(actions=actions, flags=flags, rewards=rewards, final=final, kinds=kinds)


def arcade_trace(k, n=B, actor_base=0):
    name, settings, scripts, want = ARCADE_CASES[k]
    conf = arcade_config(settings)
    return conf, host_trace(arcade_models(conf, n, actor_base=actor_base), scripts[actor_base:actor_base + n], arcade_flag,
                            conf.max_episode_steps)


def maze_trace(k, n=B):
    name, args, kind, scripts, want = MAZE_CASES[k]
    conf = maze_config(args)
    return conf, host_trace(maze_models(conf, kind, n), scripts[:n], maze_flag, conf.max_episode_steps)


# ---- the returns scan, in numpy fp64 -------------------------------------------------------------------------------------
def gae_scan(rewards, values, n_steps, boot_v, terminal_end, gamma, lam):
    """unreal_base_returns_tl as the issue states it; [T, B] inputs -> (R, adv) float64 [T, B]."""
    T, n = rewards.shape
    R, adv = np.zeros((T, n)), np.zeros((T, n))
    for b in range(n):
        next_v = 0.0 if terminal_end[b] == 1 else float(boot_v[b])
        gae = 0.0
        for t in range(int(n_steps[b]) - 1, -1, -1):
            v = float(values[t, b])
            delta = float(rewards[t, b]) + gamma * next_v - v
            gae = delta + gamma * lam * gae
            adv[t, b], R[t, b] = gae, gae + v
            next_v = v
    return R, adv


def ulp32(x):
    """One fp32 unit in the last place of |x| (of the smallest normal number below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
