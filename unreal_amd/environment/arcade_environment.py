"""Device arcade (csrc/arcade.hip): games stepped and rendered on the GPU.  Three games with ALE's
minimal action set (0 noop, 1 fire, 2 right, 3 left): Breakout, the two-paddle duel that keeps Breakout's geometry, ball and
serve and puts an opponent's paddle where the wall was, and invaders, a fixed shooter on Breakout's field: a marching grid
of aliens that drop bombs, a cannon that shoots them.  The fourth, crossing, has a sparse reward: a walker crosses up to
eight lanes of traffic from the bottom to the top (0 noop, 1 forward, 2 right, 3 left).  All are integer-only and a pure
function of (config, seed, global actor, episode, actions).  An agent step is `action_repeat` game ticks with one action (§7m).  The rules are written out
with the entries in include/unreal_hip.h.  ArcadeSelfPlay (§7v) is the duel with both paddles driven by actors: actors 2 i
and 2 i + 1 are the two seats of game i."""
import numpy as np
import torch

from . import environment
from .. import ops

# the two games of DESIGN §7k and §7l by id, kept as it was (tests/test_duel_cpu.py pins this dictionary as a whole), and
# every game by id: what ArcadeConfig accepts and writes into word 0 of the block
GAMES = {"breakout": ops.ARCADE_BREAKOUT, "duel": ops.ARCADE_DUEL}
GAME_IDS = dict(GAMES, invaders=ops.ARCADE_INVADERS)
# the settings that not every game has, with the game's defaults (None given to ArcadeConfig: the default); a setting is
# refused by the games that do not list it (lives and life_reward: by the duel only)
GAME_SETTINGS = {"breakout": dict(rows=6, row_rewards=None, lives=3, life_reward=0),
                 "duel": dict(points=5, opponent_width=12, opponent_speed=2, win_reward=1, lose_reward=-1),
                 "invaders": dict(alien_rows=3, alien_rewards=None, lives=3, life_reward=0, march_period=4, descend=4,
                                  bomb_period=12, bomb_speed=1)}
# crossing comes in through tables of its own: the three dictionaries above are pinned by tests as they are
CROSSING_SETTINGS = dict(lanes=None, car_length=8, knock_back=8, crossings=0, cross_reward=1, hit_reward=0)
ALL_GAME_IDS = dict(GAME_IDS, crossing=ops.ARCADE_CROSSING)
ALL_GAME_SETTINGS = dict(GAME_SETTINGS, crossing=CROSSING_SETTINGS)
# lanes=None: eight lanes, top lane first, as (cars, speed, period, direction): directions alternate, speeds are mixed
DEFAULT_LANES = ((2, 1, 1, 1), (1, 2, 1, -1), (4, 1, 2, 1), (2, 3, 1, -1), (2, 1, 1, 1), (1, 4, 1, -1), (4, 1, 3, 1),
                 (2, 2, 1, -1))


def _int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (name, v))
    if not lo <= v <= hi:
        raise ValueError("%s = %d outside [%d, %d]" % (name, v, lo, hi))
    return int(v)


def _even(name, v, lo, hi):
    v = _int(name, v, lo, hi)
    if v % 2:
        raise ValueError("%s = %d must be even" % (name, v))
    return v


class ArcadeConfig(object):
    """Settings of one arcade game (Environment.register_arcade_config).  Raises ValueError outside the documented ranges,
    and for a setting of another game (rows, row_rewards are Breakout's; points, opponent_width, opponent_speed,
    win_reward, lose_reward the duel's; alien_rows, alien_rewards, march_period, descend, bomb_period, bomb_speed
    invaders'; lives and life_reward are Breakout's and invaders'; lanes, car_length, knock_back, crossings, cross_reward,
    hit_reward crossing's; None: the game's default).  Every game: action_repeat in
    1..8 game ticks per agent step.  return_reward in 0..100 is paid when the agent's paddle returns the ball; invaders has
    no such event and takes only 0.  There paddle_width and paddle_speed are the cannon's, ball_speed the shot's, and
    serve_wait the ticks after a reset or a lost life in which no bomb is dropped.
    game="crossing" (DESIGN §7x): paddle_width is the walker's width, paddle_speed its lateral and ball_speed its forward
    speed in px per tick, serve_wait the ticks it is stunned after a hit; return_reward takes only 0.  lanes: a list of
    1..8 (cars, speed, period, direction) tuples, top lane first, with cars in {1, 2, 4}, speed in 0..4 px (0: parked),
    period in 1..4 ticks per move and direction +1 (to the right) or -1 (None: DEFAULT_LANES, eight lanes); car_length
    in 4..16 px (None: 8); a hit throws the walker back by knock_back in 1..70 px (None: 8) and pays hit_reward in -100..0
    (None: 0); a crossing pays cross_reward in 0..100 (None: 1); the episode ends with `crossings` in 0..99 crossings
    (the success; None: 0, never: only max_episode_steps ends it)."""
    MAX_LANES = 8
    ACTION_SIZE = 4
    MAX_ACTION_REPEAT = 8
    MAX_ROWS, COLUMNS = 6, 10
    MAX_POINTS = 9                      # the score row holds nine blocks a side
    MAX_ALIEN_ROWS, ALIEN_COLUMNS = 4, 8

    def __init__(self, game="breakout", rows=None, row_rewards=None, paddle_width=12, paddle_speed=3, ball_speed=2,
                 lives=None, serve_wait=8, life_reward=None, max_episode_steps=5000, points=None, opponent_width=None,
                 opponent_speed=None, win_reward=None, lose_reward=None, action_repeat=1, return_reward=0, alien_rows=None,
                 alien_rewards=None, march_period=None, descend=None, bomb_period=None, bomb_speed=None, lanes=None,
                 car_length=None, knock_back=None, crossings=None, cross_reward=None, hit_reward=None):
        if game not in ALL_GAME_IDS:
            raise ValueError("arcade game %r: known games are %s" % (game, sorted(ALL_GAME_IDS)))
        self.game = game
        own = dict(rows=rows, row_rewards=row_rewards, lives=lives, life_reward=life_reward, points=points,
                   opponent_width=opponent_width, opponent_speed=opponent_speed, win_reward=win_reward,
                   lose_reward=lose_reward, alien_rows=alien_rows, alien_rewards=alien_rewards, march_period=march_period,
                   descend=descend, bomb_period=bomb_period, bomb_speed=bomb_speed, lanes=lanes, car_length=car_length,
                   knock_back=knock_back, crossings=crossings, cross_reward=cross_reward, hit_reward=hit_reward)
        for other, names in ALL_GAME_SETTINGS.items():
            for name in names:
                if other != game and name not in ALL_GAME_SETTINGS[game] and own[name] is not None:
                    raise ValueError("%s is a setting of game %r, not of %r" % (name, other, game))
        own = {k: (own[k] if own[k] is not None else v) for k, v in ALL_GAME_SETTINGS[game].items()}
        if game == "breakout":
            self.rows = _int("rows", own["rows"], 1, self.MAX_ROWS)
            row_rewards = own["row_rewards"]
            if row_rewards is None:
                row_rewards = (1,) * self.rows
            if isinstance(row_rewards, (str, bytes)) or not hasattr(row_rewards, "__len__") or len(row_rewards) != self.rows:
                raise ValueError("row_rewards must hold rows = %d integers, not %r" % (self.rows, row_rewards))
            self.row_rewards = tuple(_int("row_rewards[%d]" % i, r, 0, 100) for i, r in enumerate(row_rewards))
        elif game == "invaders":
            self.alien_rows = _int("alien_rows", own["alien_rows"], 1, self.MAX_ALIEN_ROWS)
            rewards = own["alien_rewards"]
            if rewards is None:
                rewards = (1,) * self.alien_rows
            if isinstance(rewards, (str, bytes)) or not hasattr(rewards, "__len__") or len(rewards) != self.alien_rows:
                raise ValueError("alien_rewards must hold alien_rows = %d integers, not %r" % (self.alien_rows, rewards))
            self.alien_rewards = tuple(_int("alien_rewards[%d]" % i, r, 0, 100) for i, r in enumerate(rewards))
            self.march_period = _int("march_period", own["march_period"], 1, 16)
            self.descend = _int("descend", own["descend"], 1, 8)
            self.bomb_period = _int("bomb_period", own["bomb_period"], 1, 64)
            self.bomb_speed = _int("bomb_speed", own["bomb_speed"], 1, 4)
        elif game == "crossing":
            lanes = DEFAULT_LANES if own["lanes"] is None else own["lanes"]
            if isinstance(lanes, (str, bytes)) or not hasattr(lanes, "__len__") or not 1 <= len(lanes) <= self.MAX_LANES:
                raise ValueError("lanes must hold 1..%d (cars, speed, period, direction) tuples, not %r"
                                 % (self.MAX_LANES, lanes))
            checked = []
            for i, lane in enumerate(lanes):
                if isinstance(lane, (str, bytes)) or not hasattr(lane, "__len__") or len(lane) != 4:
                    raise ValueError("lanes[%d] must be (cars, speed, period, direction), not %r" % (i, lane))
                cars = _int("lanes[%d] cars" % i, lane[0], 1, 4)
                if cars == 3:
                    raise ValueError("lanes[%d] cars = 3: a lane holds 1, 2 or 4 cars" % i)
                direction = _int("lanes[%d] direction" % i, lane[3], -1, 1)
                if direction == 0:
                    raise ValueError("lanes[%d] direction = 0: +1 (to the right) or -1" % i)
                checked.append((cars, _int("lanes[%d] speed" % i, lane[1], 0, 4), _int("lanes[%d] period" % i, lane[2], 1, 4),
                                direction))
            self.lanes = tuple(checked)
            self.car_length = _int("car_length", own["car_length"], 4, 16)
            self.knock_back = _int("knock_back", own["knock_back"], 1, 70)
            self.crossings = _int("crossings", own["crossings"], 0, 99)
            self.cross_reward = _int("cross_reward", own["cross_reward"], 0, 100)
            self.hit_reward = _int("hit_reward", own["hit_reward"], -100, 0)
        else:
            self.points = _int("points", own["points"], 1, self.MAX_POINTS)
            self.opponent_width = _even("opponent_width", own["opponent_width"], 4, 24)
            self.opponent_speed = _int("opponent_speed", own["opponent_speed"], 0, 8)
            self.win_reward = _int("win_reward", own["win_reward"], 0, 100)
            self.lose_reward = _int("lose_reward", own["lose_reward"], -100, 0)
        self.paddle_width = _even("paddle_width", paddle_width, 4, 24)
        self.paddle_speed = _int("paddle_speed", paddle_speed, 1, 8)
        self.ball_speed = _int("ball_speed", ball_speed, 1, 4)
        if game not in ("duel", "crossing"):
            self.lives = _int("lives", own["lives"], 1, 5)
        self.serve_wait = _int("serve_wait", serve_wait, 0, 255)
        if game not in ("duel", "crossing"):
            self.life_reward = _int("life_reward", own["life_reward"], -100, 0)
        # mandatory: a ball that loops between the walls never ends an episode on its own
        self.max_episode_steps = _int("max_episode_steps", max_episode_steps, 1, 2 ** 31 - 1)
        self.action_repeat = _int("action_repeat", action_repeat, 1, self.MAX_ACTION_REPEAT)
        self.return_reward = _int("return_reward", return_reward, 0, 0 if game in ("invaders", "crossing") else 100)

    @property
    def action_size(self):
        return self.ACTION_SIZE

    def block(self, seed):
        """The int32 block of the kernels (UNREAL_ARCADE_CFG_WORDS words; the games' layouts: include/unreal_hip.h)."""
        seed = int(seed) & (2 ** 64 - 1)
        w = np.zeros(ops.ARCADE_CFG_WORDS, dtype=np.int64)
        w[0] = ALL_GAME_IDS[self.game]
        w[1], w[18] = self.action_repeat - 1, self.return_reward
        w[3] = self.max_episode_steps
        w[4], w[5] = seed & 0xFFFFFFFF, seed >> 32
        w[6:9] = (self.paddle_width, self.paddle_speed, self.ball_speed)
        w[10] = self.serve_wait
        if self.game == "breakout":
            w[2], w[9], w[11] = self.rows, self.lives, self.life_reward
            w[12:12 + self.rows] = self.row_rewards
        elif self.game == "invaders":
            w[2], w[9], w[11] = self.alien_rows, self.lives, self.life_reward
            w[12:12 + self.alien_rows] = self.alien_rewards
            w[16], w[17], w[19], w[20] = self.march_period, self.descend, self.bomb_period, self.bomb_speed
        elif self.game == "crossing":
            w[2], w[9], w[11] = len(self.lanes), self.crossings, self.hit_reward
            w[12], w[13], w[14] = self.cross_reward, self.knock_back, self.car_length
            for l, (cars, speed, period, direction) in enumerate(self.lanes):      # one word per field over all lanes
                w[15] |= (cars.bit_length() - 1) << (2 * l)
                w[16] |= speed << (3 * l)
                w[17] |= (period - 1) << (2 * l)
                w[19] |= int(direction > 0) << l
        else:
            w[2], w[9], w[11] = self.points, self.opponent_width, self.lose_reward
            w[12], w[13] = self.win_reward, self.opponent_speed
        return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


class ArcadeMix(object):
    """A game mixture (Environment.register_arcade_mix): an ordered list of 1..16 ArcadeConfigs ("tasks"),
    different games or one game with different settings.  Global actor g plays task g % K for the whole run, by the
    task's own rules (action_repeat, return_reward and max_episode_steps included); listing a task more than once gives
    it more actors.  Raises ValueError for an empty list, more than 16 tasks or an item that is no ArcadeConfig."""
    ACTION_SIZE = 4
    MAX_TASKS = ops.ARCADE_MIX_MAX
    game = "mix"

    def __init__(self, tasks, names=None):
        tasks = list(tasks)
        if not 1 <= len(tasks) <= self.MAX_TASKS:
            raise ValueError("a game mixture holds 1..%d tasks, not %d" % (self.MAX_TASKS, len(tasks)))
        for t in tasks:
            if isinstance(t, ArcadeSelfPlay):
                raise ValueError("self-play inside a game mixture is out of scope: its actors come in pairs (DESIGN §7v)")
            if not isinstance(t, ArcadeConfig):
                raise ValueError("a task of a game mixture must be an ArcadeConfig, not %r" % (t,))
        names = ["%d:%s" % (k, t.game) for k, t in enumerate(tasks)] if names is None else [str(n) for n in names]
        if len(names) != len(tasks):
            raise ValueError("%d names for %d tasks" % (len(names), len(tasks)))
        self.tasks = tuple(tasks)
        self.task_names = tuple(names)

    @property
    def action_size(self):
        return self.ACTION_SIZE

    def __len__(self):
        return len(self.tasks)

    def task_of(self, global_actor):
        """Index of the task global actor `global_actor` plays (an integer or an integer array)."""
        if np.any(np.asarray(global_actor) < 0):
            raise ValueError("global actor %r < 0" % (global_actor,))
        return global_actor % len(self.tasks)

    def block(self, seed):
        """The K consecutive blocks of the _mix entries: every task's own block(seed)."""
        return np.concatenate([t.block(seed) for t in self.tasks])


class ArcadeSelfPlay(object):
    """The duel with both paddles driven by actors (Environment.register_arcade_selfplay): global actors 2 i and
    2 i + 1 are seat 0 and seat 1 of game i, the top paddle is seat 1's and as wide and as fast as the bottom one, either
    seat's fire serves, and seat 1 sees the game mirrored, itself at the bottom.  Built from the duel's settings;
    `opponent_width` is no keyword (the width is paddle_width).  `.scripted` is the duel against the scripted opponent
    with the same settings, the only place `opponent_speed` is used: what the batch-1 surface and Evaluate without
    `versus` play.  Raises ValueError as ArcadeConfig does."""
    ACTION_SIZE = 4
    game = "selfplay"

    def __init__(self, points=None, paddle_width=12, paddle_speed=3, ball_speed=2, serve_wait=8, win_reward=None,
                 lose_reward=None, max_episode_steps=5000, action_repeat=1, return_reward=0, opponent_speed=None):
        paddle_width = _even("paddle_width", paddle_width, 4, 24)          # (checked here: it is the opponent's, too)
        self.scripted = ArcadeConfig(game="duel", points=points, paddle_width=paddle_width, paddle_speed=paddle_speed,
                                     ball_speed=ball_speed, serve_wait=serve_wait, win_reward=win_reward,
                                     lose_reward=lose_reward, max_episode_steps=max_episode_steps,
                                     action_repeat=action_repeat, return_reward=return_reward,
                                     opponent_speed=opponent_speed, opponent_width=paddle_width)
        for name in ("points", "paddle_width", "paddle_speed", "ball_speed", "serve_wait", "win_reward", "lose_reward",
                     "max_episode_steps", "action_repeat", "return_reward", "opponent_speed"):
            setattr(self, name, getattr(self.scripted, name))

    @property
    def action_size(self):
        return self.ACTION_SIZE

    def block(self, seed):
        """The duel's block of `.scripted` (word 9 equals word 6; the _selfplay entries ignore word 13)."""
        return self.scripted.block(seed)


class ArcadeOpponent(object):
    """The other paddle of the B games of a versus environment: `actions` (int32 [B], the input of every step),
    and what the step keeps of seat 1's side: `frames` (uint8, one frame per game: the observation seat 1 would see),
    `last_action` (int32 [B]) and `last_reward` (float32 [B]).  Shaped enough like a ring for
    UnrealModel.encode_rows(..., lar_from_ring=False) to read it with frame index b."""

    def __init__(self, B, device):
        self.B = B
        self.frame_shape, self.frame_stride = ops.FRAME_SHAPE, ops.FRAME_BYTES
        self.actions = torch.zeros(B, dtype=torch.int32, device=device)
        self.frames = torch.zeros(B * ops.FRAME_BYTES, dtype=torch.uint8, device=device)
        self.last_action = torch.zeros(B, dtype=torch.int32, device=device)
        self.last_reward = torch.zeros(B, dtype=torch.float32, device=device)

    def view(self, b0, b1):
        v = object.__new__(ArcadeOpponent)
        v.B, v.frame_shape, v.frame_stride = b1 - b0, self.frame_shape, self.frame_stride
        v.actions, v.last_action, v.last_reward = self.actions[b0:b1], self.last_action[b0:b1], self.last_reward[b0:b1]
        v.frames = self.frames[b0 * ops.FRAME_BYTES:b1 * ops.FRAME_BYTES]
        return v


class BatchedArcadeEnvironment(object):
    """B actors of one arcade game, of a game mixture (ArcadeMix) or of B / 2 self-play games (ArcadeSelfPlay: actors
    2 i and 2 i + 1 are the seats of game i, so B, actor_base and a view's bounds are even), on the device, with the
    interface of BatchedMazeEnvironment.  `versus=True` (an ArcadeSelfPlay only): B games with one actor
    each, seat 0 of game actor_base + b of the self-play environment; the other paddle plays `.opponent.actions`, and
    B, actor_base and a view's bounds may be odd."""
    ACTION_SIZE = 4
    frame_scale = 1.0 / 255.0          # ring bytes 0..255
    objective_size = 0

    def __init__(self, batch, history_size, device="cuda:0", config=None, actor_base=0, actors_total=None, seed=0,
                 final_obs=False, depth_labels=False, bonus=False, versus=False):
        """`bonus`: exploration bonus: the ring keeps r_bonus beside r_reward.
        `actor_base` / `actors_total`: global index of actor 0 and the number of actors over every rank (the serve
        draws are keyed by the global index); `seed`: their key.  `final_obs`: time-limit bootstrapping: the
        rollout steps keep the final observation of an episode that ends by max_episode_steps alone in ring.final_obs
        and flag it 2 instead of 1.  `depth_labels`: refused (first-person mazes only)."""
        if depth_labels:
            raise ValueError("depth_labels is out of scope for the arcade: a game has no wall distances (it needs a "
                             "first-person device maze)")
        if not isinstance(config, (ArcadeConfig, ArcadeMix, ArcadeSelfPlay)):
            raise ValueError("BatchedArcadeEnvironment needs an ArcadeConfig, an ArcadeMix or an ArcadeSelfPlay")
        selfplay = isinstance(config, ArcadeSelfPlay)
        if versus and not selfplay:
            raise ValueError("versus=True needs an ArcadeSelfPlay config: the other paddle is a self-play game's seat 1")
        if selfplay and not versus and (batch % 2 or actor_base % 2):
            raise ValueError("self-play actors come in pairs: batch = %d and actor_base = %d must be even"
                             % (batch, actor_base))
        self.B = batch
        self.config = config
        total = batch if actors_total is None else int(actors_total)
        if actor_base < 0 or actor_base + batch > total:
            raise ValueError("actors [%d, %d) outside the %d actors of the job" % (actor_base, actor_base + batch, total))
        mix = isinstance(config, ArcadeMix)
        self.ring = ops.Ring(batch, history_size, torch.device(device), arcade=True, final_obs=bool(final_obs),
                             bonus=bool(bonus), arcade_stats=mix)
        block = torch.from_numpy(config.block(seed)).to(self.ring.count.device)
        # a mixture: (K blocks, actor_base, K), which selects the _mix entries (ops._arcade_args); self-play: (block,
        # actor_base, ops.ARCADE_SELFPLAY), which selects the _selfplay entries
        # versus: (block, actor_base, ops.ARCADE_VERSUS, the opponent's buffers), which selects the _versus entries
        self.opponent = ArcadeOpponent(batch, self.ring.count.device) if versus else None
        self.arcade = (block, int(actor_base)) + ((len(config),) if mix else (ops.ARCADE_VERSUS, self.opponent) if versus
                                                  else (ops.ARCADE_SELFPLAY,) if selfplay else ())
        self.reset()

    def view(self, b0, b1):
        """The environments [b0, b1) as a batched environment of their own (shares the ring memory), as
        BatchedMazeEnvironment.view."""
        versus = getattr(self, "opponent", None) is not None
        if isinstance(self.config, ArcadeSelfPlay) and not versus and (b0 % 2 or b1 % 2):
            raise ValueError("a view of a self-play environment holds whole pairs: [%d, %d) has an odd bound" % (b0, b1))
        v = object.__new__(BatchedArcadeEnvironment)
        v.B, v.ring = b1 - b0, ops.ring_view(self.ring, b0, b1)
        v.base_actor = b0
        v.config = self.config
        v.opponent = self.opponent.view(b0, b1) if versus else None
        v.arcade = (self.arcade[0], self.arcade[1] + b0) + ((ops.ARCADE_VERSUS, v.opponent) if versus else self.arcade[2:])
        return v

    def task_of_actor(self):
        """Index of the task every actor of this environment (or view) plays -> int [B]; zeros for a single game."""
        if not isinstance(self.config, ArcadeMix):
            return np.zeros(self.B, dtype=np.int64)
        return self.config.task_of(self.arcade[1] + np.arange(self.B, dtype=np.int64))

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
                                final_obs=self.ring.final_obs, **nxt)

    def policy_rollout_step(self, net, feat, ld, u, pi_out, v_out, actions, out_reward, out_terminal, active, active_log_t,
                            n_steps, terminal_end, index_parent=False, **nxt):
        p = net.p
        ops.arcade_policy_rollout_step(self.ring, feat, ld, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                       p["b_base_fc_v"], u, pi_out, v_out, actions, out_reward, out_terminal, active,
                                       active_log_t, n_steps, terminal_end,
                                       base_actor=getattr(self, "base_actor", 0) if index_parent else 0,
                                       arcade=self.arcade, final_obs=self.ring.final_obs, **nxt)

    def current_records(self):
        """The game records -> int32 [B, 16].  Breakout: px, bx, by, vx, vy, wait, lives, bricks lo, hi, serve_index, then
        the running totals of bricks, lives lost and walls cleared.  Duel: px, bx, by, vx, vy, wait, ox, mine, theirs,
        serve_index, then the running totals of points won, points lost and matches won.  Words 13..15 are 0.  Invaders: px,
        sx, sy (0: no shot), gx, gy, direction, lives, alien mask, march | bomb << 8 | grace << 16 counters, draw_index,
        then the running totals of aliens shot, lives lost and waves cleared, then the three bombs as x | y << 8 (0: free).
        Crossing: px, py, stun, the episode's crossings, tick counter (modulo 12), the lanes' 7-bit offsets (lanes 0..3 in
        the bytes of word 5, lanes 4..7 in those of word 6), words 7..9 0, then the running totals of crossings, hits and
        targets reached; words 13..15 are 0.
        Self-play: one duel record per SEAT; rows 2 i hold game i's canonical record (seat 0 at the bottom),
        rows 2 i + 1 its mirror image, the game as seat 1 sees it (px and ox, mine and theirs, words 10 and 11, words 12
        and 13 swapped, by = 86 - by, vy = -vy); word 13 is the other seat's matches won, words 14..15 are 0.  Versus (DESIGN
        §7w): row b holds game b's canonical record."""
        return self.ring.actor_records.cpu().numpy().copy()

    def stop(self):
        pass


class ArcadeEnvironment(environment.Environment):
    """The batch-1 surface of the reference's environments: process(action) -> image, reward, terminal, pixel_change.
    No reset on terminal: the caller resets."""

    @staticmethod
    def get_action_size():
        return 4

    def __init__(self, device="cuda:0", config=None, seed=0, task=0):
        """`task`: of a game mixture (ArcadeMix), the task this one actor plays (a single game takes only 0)."""
        environment.Environment.__init__(self)
        n_tasks = len(config) if isinstance(config, ArcadeMix) else 1
        if isinstance(task, bool) or not isinstance(task, (int, np.integer)) or not 0 <= task < n_tasks:
            raise ValueError("task = %r outside the %d task(s) of the config" % (task, n_tasks))
        if isinstance(config, ArcadeMix):
            config = config.tasks[task]
        if isinstance(config, ArcadeSelfPlay):         # one actor: seat 0 against the scripted opponent
            config = config.scripted
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
        if self._env.config.game == "duel":            # the match is won
            success = terminal and int(rec[7]) >= self._env.config.points
        elif self._env.config.game == "crossing":      # the target is reached
            success = terminal and 0 < self._env.config.crossings <= int(rec[3])
        elif self._env.config.game == "invaders":      # the wave is cleared
            success = terminal and not rec[7]
        else:                                          # the wall is cleared
            success = terminal and not (rec[7] | rec[8])
        self._last_full_state = {"success": bool(success)}
        return image, reward, terminal, pc
