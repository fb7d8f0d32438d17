"""Host model of a game mixture (csrc/arcade.hip): no game logic of its own.  Global actor g of a mixture of K
tasks plays what actor g of a single-game environment of task g % K with the same seed plays, so the model of a mixture is
one existing host model per actor: the classes the games' own tests use (tests/repeat_model.py for Breakout and the duel,
which drives the one-tick models through `action_repeat` ticks; tests/invaders_model.py), each built for its global actor
and its task's config.

The traces of tests/test_arcade_mix_gpu.py are run here on the models alone, once, and shared read-only;
tests/test_arcade_mix_cpu.py asserts on them that every task of every trace ends an episode by the game and one by its
own step limit, so the comparison on the device is not vacuous."""
import functools

import numpy as np

try:
    import repeat_model as RM
    import invaders_model as IM
except ImportError:            # imported as tests.<module>
    from tests import repeat_model as RM
    from tests import invaders_model as IM


def model_class(conf):
    return IM.HostInvaders if conf.game == "invaders" else RM.model_class(conf)


def host_batch(mix, B, seed, actor_base=0, frames=True):
    """The host models of the actors [actor_base, actor_base + B) of a device environment of the mixture with key `seed`:
    actor b is global actor actor_base + b and plays task (actor_base + b) % K.  Each is reset once, as the environment's
    constructor does; OracleTrainer(envs=...) accepts them."""
    K = len(mix.tasks)
    out = []
    for b in range(B):
        g = actor_base + b
        conf = mix.tasks[g % K]
        out.append(model_class(conf)(conf, g, seed, frames=frames))
    return out


# ---- the mixtures of the tests ---------------------------------------------------------------------------------------------------
# the three games' short settings (tests/test_arcade_gpu.py, test_duel_gpu.py, test_invaders_gpu.py: SHORT), made to differ
# per task in max_episode_steps (30 / 20 / 25) and action_repeat (1 / 4 / 2: the four ticks go to the duel, because invaders'
# short setting at four ticks a step is always invaded before any of the three limits and would never be cut by its own)
SHORT = (dict(rows=2, row_rewards=(7, 1), lives=1, paddle_width=24, ball_speed=4, serve_wait=1, life_reward=-1),
         dict(game="duel", points=2, paddle_width=24, ball_speed=4, serve_wait=1, opponent_width=4, opponent_speed=1,
              win_reward=7, lose_reward=-1),
         dict(game="invaders", alien_rows=1, lives=2, paddle_width=24, ball_speed=4, bomb_period=2, bomb_speed=4,
              march_period=1, descend=8, serve_wait=1, alien_rewards=(7,), life_reward=-1))
MIX3 = tuple(dict(s, max_episode_steps=m, action_repeat=k) for s, m, k in zip(SHORT, (30, 20, 25), (1, 4, 2)))
# sixteen tasks: the three above, then variants of all three games (paddle widths, ball speeds, bomb periods, points,
# action_repeat 1..8, return_reward, step limits 5..24)
_B, _D, _I = SHORT
MIX16 = MIX3 + (
    dict(_B, paddle_width=12, ball_speed=2, action_repeat=2, max_episode_steps=15),
    dict(_D, points=1, opponent_width=12, action_repeat=1, max_episode_steps=24),
    dict(_I, bomb_period=4, lives=1, action_repeat=1, max_episode_steps=20),
    dict(_B, rows=1, row_rewards=(3,), lives=2, action_repeat=4, return_reward=2, max_episode_steps=12),
    dict(_D, ball_speed=2, action_repeat=4, return_reward=1, max_episode_steps=10),
    dict(_I, alien_rows=2, alien_rewards=(5, 1), bomb_speed=2, lives=1, action_repeat=3, max_episode_steps=13),
    dict(_B, paddle_width=4, action_repeat=8, max_episode_steps=8),
    dict(_D, opponent_speed=8, opponent_width=24, action_repeat=8, max_episode_steps=9),
    dict(_I, lives=1, action_repeat=8, max_episode_steps=5),
    dict(_B, ball_speed=3, paddle_speed=8, action_repeat=3, max_episode_steps=16),
    dict(_D, paddle_width=4, action_repeat=3, max_episode_steps=14),
    dict(_I, paddle_width=4, paddle_speed=8, action_repeat=3, max_episode_steps=22),
    dict(_B, ball_speed=1, action_repeat=5, max_episode_steps=11),
)


def make_mix(settings):
    from unreal_amd.environment.arcade_environment import ArcadeConfig, ArcadeMix
    return ArcadeMix([ArcadeConfig(**s) for s in settings])


# ---- the traces ---------------------------------------------------------------------------------------------------------------
# (tasks, actors): K = 3 with every task on exactly one actor, an uneven split and many workgroups per task; K = 16 at 19
TRACE_CASES = ((MIX3, 3), (MIX3, 7), (MIX3, 64), (MIX16, 19))
TRACE_STEPS = 120
TRACE_FRAMES = 19              # frames and pixel change: every actor up to this many actors, else of the first 8
# (key of the draws, seed of the actions) per trace, chosen so that every task of the trace ends an episode by the game and
# one by its step limit (tests/test_arcade_mix_cpu.py asserts it)
TRACE_SEEDS = ((1, 4), (2, 0), (1, 0), (5, 2))
TRACE_H1 = 4


def trace_mix(case):
    return make_mix(TRACE_CASES[case][0])


def trace_framed(case):
    B = TRACE_CASES[case][1]
    return B if B <= TRACE_FRAMES else 8


def trace_inputs(case, action_seed=None):
    """Actions and active flags of a trace -> int32 [TRACE_STEPS, B] each, active with probability 0.9."""
    B = TRACE_CASES[case][1]
    rs = np.random.RandomState(2000 + 16 * (TRACE_SEEDS[case][1] if action_seed is None else action_seed) + case)
    acts = rs.randint(0, 4, (TRACE_STEPS, B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, B) < 0.9).astype(np.int32)
    return acts, active


def simulate(case, seed, action_seed, framed):
    """A trace on the models alone: the actors start in episode 1 (the constructor's reset and one more, as the GPU test's
    environment), step with reset on terminal, and after every step everything a device environment shows is recorded.
    -> dict of acts, active [S, B]; records [S, B, 16]; reward, terminal (of the active actors; -7.5 / -7 elsewhere), count,
    ep_steps, episode, last_action, last_reward [S, B]; frames [S, F, 21168] (the current observation after the step), pc
    [S, F, 400] with pc_slot [S, F] (ring slot of the step's pixel change at H1 = 4; -1: idle); done_return, done_episodes
    [B] (the sums over the finished episodes); flags [S, B]: what a _tl entry reports of the step, 0, 1 (ended by the game)
    or 2 (cut by the task's step limit alone), -7 where idle; final: {(s, b): frame} the observation a cut left behind, of
    the framed actors; endings: the set of (task, "game" | "limit") seen."""
    mix = trace_mix(case)
    K, B, S, F, H1 = len(mix.tasks), TRACE_CASES[case][1], TRACE_STEPS, framed, TRACE_H1
    models = host_batch(mix, B, seed)
    for b, m in enumerate(models):
        m.frames = b < F
        m.reset()
    acts, active = trace_inputs(case, action_seed)
    out = dict(acts=acts, active=active, records=np.zeros((S, B, 16), np.int32),
               reward=np.full((S, B), -7.5, np.float32), terminal=np.full((S, B), -7, np.int32),
               frames=np.zeros((S, F, 21168), np.uint8), pc=np.zeros((S, F, 400), np.float32),
               pc_slot=np.full((S, F), -1, np.int64), flags=np.full((S, B), -7, np.int32), final={}, done_return=np.zeros(B, np.float64), done_episodes=np.zeros(B, np.int64))
    for name in ("count", "ep_steps", "episode", "last_action"):
        out[name] = np.zeros((S, B), np.int64)
    out["last_reward"] = np.zeros((S, B), np.float32)
    count, prev_term, ret, endings = np.zeros(B, np.int64), np.zeros(B, bool), np.zeros(B, np.int64), set()
    for s in range(S):
        for b, m in enumerate(models):
            if active[s, b]:
                _, r, t, pc = m.process(acts[s, b])
                out["reward"][s, b], out["terminal"][s, b] = r, int(t)
                ret[b] += r
                if b < F:
                    out["pc"][s, b], out["pc_slot"][s, b] = pc.reshape(-1), b * H1 + count[b] % H1
                if not (t and count[b] > 0 and prev_term[b]):
                    count[b] += 1
                prev_term[b] = t
                out["flags"][s, b] = 0
                if t:
                    cut = "end_timeout" in m.events
                    endings.add((b % K, "limit" if cut else "game"))
                    out["flags"][s, b] = 2 if cut else 1
                    if cut and b < F:
                        out["final"][(s, b)] = m.frame.reshape(-1).copy()
                    out["done_return"][b] += ret[b]
                    out["done_episodes"][b] += 1
                    ret[b] = 0
                    m.reset()
            out["records"][s, b] = m.record()
            out["ep_steps"][s, b], out["episode"][s, b] = m.ep_steps, m.episode
            out["last_action"][s, b], out["last_reward"][s, b] = m.last_action, m.last_reward
            if b < F:
                out["frames"][s, b] = m.frame.reshape(-1)
        out["count"][s] = count
    out["endings"] = frozenset(endings)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def run_trace(case):
    """Trace `case` with its seeds, computed once and shared (read-only) by the tests."""
    return simulate(case, TRACE_SEEDS[case][0], None, trace_framed(case))


def every_ending(case):
    K = len(TRACE_CASES[case][0])
    return {(k, e) for k in range(K) for e in ("game", "limit")}
