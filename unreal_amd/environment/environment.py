"""Environment factory with the reference's surface (/root/reference/environment/environment.py:11-102).

The maze and the arcade (arcade_environment.py: Breakout, the two-paddle duel and invaders) are device environments; lab / indoor actors are HOST-FED (hostfed_environment.py) by simulator objects
the caller supplies, because deepmind_lab / minos / gym are not in the image.  Gym actors are host-fed through
gym_environment.GymBatchSimulator (any object with gym's reset / step API)."""


class Environment(object):
    action_size = -1          # class-cached: first query wins (environment.py:13,46-47)
    LOG_DIR = None
    # stands in for minos.config.sim_config (indoor_environment.py:27-29; main.py:196 reads height / width from it):
    # env_name -> {'objective_size': n, 'height': H, 'width': W}
    INDOOR_CONFIG = {}
    # stands in for gym.make(env_name).action_space.n (gym_environment.py:55-60): env_name -> action count
    GYM_CONFIG = {}
    # env_name -> maze_environment.MazeConfig: user mazes on the device (an unregistered name is the reference's map)
    MAZE_CONFIG = {}
    # env_name -> arcade_environment.ArcadeConfig: arcade games stepped and rendered on the device
    ARCADE_CONFIG = {}

    @staticmethod
    def register_indoor_config(env_name, objective_size, height=84, width=84):
        from .. import ops
        h, w = int(height), int(width)
        if (h, w) != ops.FRAME_SHAPE:
            ops.frame_dims(h, w)               # raises outside 20 <= H, W <= 480
        Environment.INDOOR_CONFIG[env_name] = {'objective_size': int(objective_size), 'height': h, 'width': w}

    @staticmethod
    def register_gym_config(env_name, action_size):
        a = int(action_size)
        if not 2 <= a <= 18:
            raise ValueError("gym action_size %d: the device heads support 2..18 actions" % a)
        Environment.GYM_CONFIG[env_name] = a

    @staticmethod
    def register_maze_config(env_name, layouts=None, random_start=False, random_goal=False, show_goal=False,
                             max_episode_steps=0, view="top_down", start_heading=None, goal_reward=1, apple_reward=1,
                             hit_reward=-1, goal_respawn=False, action_set="turn", generate=None, gen_loops=0,
                             gen_apples=0, wall_styles=None, gen_landmark_density=0, goal_sense=False, progress_reward=0,
                             pickups=None, gen_pickups=None, no_goal=False):
        """Mazes of `env_name`: `layouts` = N x N maps (strings, or lists of row strings; + wall, - free, S start, G goal),
        N in {7, 12, 14, 21}, up to 1024 of them; global actor g runs layout g * L // (all actors).  random_start /
        random_goal: drawn at every reset, uniformly over the free cells (the start never on the goal); show_goal: the
        goal block in channel 2; max_episode_steps > 0: an episode that has not reached the goal ends (terminal) at
        that step.  view="first_person": a raycast 84 x 84 camera in the agent's cell (actions turn left / right, step
        forward / back), start_heading None (drawn at every reset) or 0..3.  First person only:
        'A' layout cells hold apples (at most 64 per layout); goal_reward / apple_reward / hit_reward are integers in
        [-100, 100]; goal_respawn=True (needs max_episode_steps > 0) moves the agent to a start cell at the goal instead
        of ending the episode; action_set="lab" selects Lab's six actions (look left / right, strafe left / right,
        forward, back).  generate=N (first person, layouts=None, random_start and random_goal): no layouts
        are given; every reset of an actor writes a new N x N maze on the device, a spanning tree of the rooms at the
        even cells plus gen_loops extra openings, with gen_apples apples in drawn rooms -- a pure function of (seed,
        global actor, episode), so training on one seed and evaluating on another tests generalisation over layouts.
        wall_styles (first person): 1 to 7 styles (r, g, b, pattern), integers in 0..255; layout digits 1..7
        are wall cells drawn in style k: its colour, halved in the eighths of a cell's face whose bit of `pattern` is set
        (stripes fixed to the world, the same from every cell and heading); gen_landmark_density in 0..256 (with generate
        and wall_styles): every wall cell of a generated maze is such a landmark with probability density / 256.
        goal_sense=True (first person): every state carries an 'objective' vector [gf / 32, gs / 32, d / 512]:
        the goal's offset ahead of and to the right of the agent, in cells, and the length d of the shortest path to it;
        get_objective_size('maze', env_name) is then 3 and the network needs objective_size=3.  progress_reward (an
        integer in [-100, 100]; needs goal_sense) adds progress_reward * (d before the move - d after it) to every step's
        reward.
        pickups (first person): 1 to 3 kinds (reward, (r, g, b), ends_episode) next to the apple: layout cells
        'B', 'C', 'D' hold a pickup of kind 1, 2, 3, drawn on the floor in its colour, paying its reward (an integer in
        [-100, 100]) once per episode and, with ends_episode=True, ending the episode; at most 64 pickups of all kinds
        per layout; not with goal_sense.  gen_pickups (with generate and pickups): how many rooms of a generated maze hold
        each kind.  no_goal=True (first person; needs max_episode_steps > 0): the layouts have no 'G', nothing is drawn as
        a goal, and an episode ends at its time-out or at an ending pickup: with lemons at -1 the seek-avoid arena, with
        one large ending pickup stairway-to-melon.
        Raises ValueError on a malformed config."""
        from .maze_environment import MazeConfig
        Environment.MAZE_CONFIG[env_name] = MazeConfig(layouts, random_start, random_goal, show_goal, max_episode_steps,
                                                       view, start_heading, goal_reward, apple_reward, hit_reward,
                                                       goal_respawn, action_set, generate, gen_loops, gen_apples,
                                                       wall_styles, gen_landmark_density, goal_sense, progress_reward,
                                                       pickups, gen_pickups, no_goal)

    @staticmethod
    def register_arcade_config(env_name, game="breakout", rows=None, row_rewards=None, paddle_width=12, paddle_speed=3,
                               ball_speed=2, lives=None, serve_wait=8, life_reward=None, max_episode_steps=5000,
                               points=None, opponent_width=None, opponent_speed=None, win_reward=None, lose_reward=None,
                               action_repeat=1, return_reward=0, alien_rows=None, alien_rewards=None, march_period=None,
                               descend=None, bomb_period=None, bomb_speed=None, lanes=None, car_length=None,
                               knock_back=None, crossings=None, cross_reward=None, hit_reward=None):
        """Arcade game of `env_name` on the device (env_type 'arcade'), with ALE's minimal action set
        (0 noop, 1 fire, 2 right, 3 left) on an 84 x 84 RGB frame.  Both games: paddle_width even in 4..24 px;
        paddle_speed in 1..8 px per step; ball_speed in 1..4 micro-steps per step; serve_wait in 0..255: a waiting ball
        serves itself after that many steps (0: only fire serves); max_episode_steps in 1..2^31 - 1 ends an episode (a
        looping ball would never), counted in agent steps; action_repeat in 1..8: an agent step is that many game
        ticks with the same action, fewer where a tick ends the game, and pays their rewards' sum;
        return_reward in 0..100 is paid in the tick in which the agent's paddle returns the ball.
        game="breakout": rows in 1..6 rows of 10 bricks (None: 6); row_rewards: one integer in 0..100 per row from the
        top (None: all 1); lives in 1..5 (None: 3); life_reward in -100..0 is paid with every lost life (None: 0).  An
        episode also ends with the last life or the last brick (success).
        game="duel": an opponent's paddle at the top follows the ball; a ball past it pays win_reward in 0..100 (None: 1),
        a ball past the agent's pays lose_reward in -100..0 (None: -1); the first side with `points` in 1..9 (None: 5)
        wins the match, which ends the episode (success: the agent's); opponent_width even in 4..24 (None: 12);
        opponent_speed in 0..8 px per step (None: 2; 0: it stands).
        game="invaders" (DESIGN §7n): alien_rows in 1..4 rows of 8 aliens (None: 3) march 2 px every march_period in 1..16
        ticks (None: 4) and come down by descend in 1..8 px at each edge (None: 4); alien_rewards: one integer in 0..100
        per row from the top (None: all 1); every bomb_period in 1..64 ticks (None: 12) a random column drops a bomb, three
        in flight at the most, falling bomb_speed in 1..4 px per tick (None: 1); a bomb on the cannon takes one of lives in
        1..5 (None: 3) and pays life_reward in -100..0 (None: 0).  paddle_width and paddle_speed are the cannon's,
        ball_speed the shot's, serve_wait the ticks without a new bomb after a reset or a lost life; return_reward must
        be 0.  An episode also ends with the last life, when the aliens reach the cannon's rows, or with the last alien
        (success).
        game="crossing" (actions 0 noop, 1 forward, 2 right, 3 left): a walker of paddle_width x 4 px crosses
        the lanes of traffic from the bottom to the top, ball_speed px per forward tick, paddle_speed px sideways.
        lanes: 1..8 (cars, speed, period, direction) tuples, top lane first: cars in {1, 2, 4} of car_length in 4..16 px
        (None: 8) move speed in 0..4 px every period in 1..4 ticks to the right (+1) or the left (-1) (None: eight lanes
        of alternating directions and mixed speeds).  A car that hits the walker throws it back by knock_back in 1..70 px
        (None: 8; 70: to the start), pays hit_reward in -100..0 (None: 0) and stuns it for serve_wait ticks; a crossing
        pays cross_reward in 0..100 (None: 1).  `crossings` in 0..99 crossings end the episode (success; None: 0: only
        max_episode_steps does); return_reward must be 0.
        Raises ValueError outside these ranges and for a setting of another game."""
        from .arcade_environment import ArcadeConfig
        Environment.ARCADE_CONFIG[env_name] = ArcadeConfig(game, rows, row_rewards, paddle_width, paddle_speed, ball_speed,
                                                           lives, serve_wait, life_reward, max_episode_steps, points,
                                                           opponent_width, opponent_speed, win_reward, lose_reward,
                                                           action_repeat, return_reward, alien_rows, alien_rewards,
                                                           march_period, descend, bomb_period, bomb_speed, lanes,
                                                           car_length, knock_back, crossings, cross_reward, hit_reward)

    @staticmethod
    def register_arcade_mix(env_name, tasks):
        """Game mixture of `env_name` on the device (env_type 'arcade'): `tasks` is a list of 1..16 items, each
        the name of a registered arcade config or a dict of register_arcade_config's keywords.  Global actor g plays task
        g % len(tasks) for the whole run, by that task's own rules; list a task more than once to give it more actors.
        Raises KeyError for a name that is not registered and ValueError for a registered mixture's name, any other item
        or a task count outside 1..16."""
        from .arcade_environment import ArcadeConfig, ArcadeMix
        if isinstance(tasks, (str, bytes, dict)) or not hasattr(tasks, "__iter__"):
            raise ValueError("tasks must be a list of config names or dicts, not %r" % (tasks,))
        confs, names = [], []
        for k, t in enumerate(tasks):
            if isinstance(t, str):
                conf = Environment.arcade_config(t)
                if not isinstance(conf, ArcadeConfig):
                    raise ValueError("task %r is a mixture itself or a self-play game: a mixture lists single games" % t)
                confs.append(conf)
                names.append(t)
            elif isinstance(t, dict):
                confs.append(ArcadeConfig(**t))
                names.append("%d:%s" % (k, confs[-1].game))
            else:
                raise ValueError("task %d must be a registered config's name or a dict of settings, not %r" % (k, t))
        Environment.ARCADE_CONFIG[env_name] = ArcadeMix(confs, names)

    @staticmethod
    def register_arcade_selfplay(env_name, **settings):
        """Self-play duel of `env_name` on the device (env_type 'arcade'): both paddles are actors, global
        actors 2 i and 2 i + 1 the two seats of game i, so every actor count the trainer steps at once must be even.
        `settings` are the duel's keywords of register_arcade_config without `game` and `opponent_width` (the top paddle
        is as wide as the bottom one): points, paddle_width, paddle_speed, ball_speed, serve_wait, win_reward,
        lose_reward, max_episode_steps, action_repeat, return_reward, and opponent_speed, which only the scripted opponent
        of the batch-1 surface and of Evaluate without `versus` uses.  The name shares register_arcade_config's namespace:
        registering a name again replaces what it named, as there.  Raises ValueError outside the duel's ranges and
        TypeError for any other keyword."""
        from .arcade_environment import ArcadeSelfPlay
        Environment.ARCADE_CONFIG[env_name] = ArcadeSelfPlay(**settings)

    @staticmethod
    def arcade_config(env_name):
        if env_name not in Environment.ARCADE_CONFIG:
            raise KeyError("arcade env %r: call Environment.register_arcade_config(name, ...) first" % env_name)
        return Environment.ARCADE_CONFIG[env_name]

    @staticmethod
    def create_environment(env_type, env_name, termination_time=50.0, env_args=None, thread_index=0):
        if env_type == 'maze':
            from . import maze_environment
            return maze_environment.MazeEnvironment(config=Environment.MAZE_CONFIG.get(env_name))
        if env_type == 'arcade':
            from . import arcade_environment
            return arcade_environment.ArcadeEnvironment(config=Environment.arcade_config(env_name))
        raise NotImplementedError("env_type %r needs an external simulator that is out of scope (SURVEY 8f)" % env_type)

    @staticmethod
    def get_action_size(env_type, env_name):
        conf = Environment.MAZE_CONFIG.get(env_name) if env_type == 'maze' else None
        if conf is not None and conf.action_set == "lab":
            return 6                             # a navigation maze with Lab's actions: the class cache is not involved
        if env_type == 'arcade':                 # nor here: the game's own action count
            return Environment.arcade_config(env_name).action_size
        if Environment.action_size >= 0:
            return Environment.action_size
        if env_type == 'maze':
            from . import maze_environment
            Environment.action_size = maze_environment.MazeEnvironment.get_action_size()
        elif env_type == 'lab':
            Environment.action_size = 6      # lab_environment.py:57-73
        elif env_type == 'indoor':
            Environment.action_size = 3      # indoor_environment.py:16-20
        elif env_type == 'gym':
            if env_name not in Environment.GYM_CONFIG:
                raise KeyError("gym env %r: call Environment.register_gym_config(name, action_size) first" % env_name)
            Environment.action_size = Environment.GYM_CONFIG[env_name]
        else:
            raise NotImplementedError(env_type)
        return Environment.action_size

    @staticmethod
    def get_objective_size(env_type, env_name):
        if env_type == 'indoor':               # environment.py:68-72 -> indoor_environment.py:26-29
            return Environment.INDOOR_CONFIG.get(env_name, {}).get('objective_size', 0)
        conf = Environment.MAZE_CONFIG.get(env_name) if env_type == 'maze' else None
        if conf is not None and conf.goal_sense:       # a goal-sense maze: goal offset and path distance
            return conf.OBJECTIVE_SIZE
        return 0

    @staticmethod
    def get_image_shape(env_type, env_name):
        """[height, width] of the environment's frames (main.py:196: the MINOS config's, default 84; every other
        environment type is 84 x 84)."""
        if env_type == 'indoor':
            cfg = Environment.INDOOR_CONFIG.get(env_name, {})
            return [cfg.get('height', 84), cfg.get('width', 84)]
        return [84, 84]

    def __init__(self):
        pass

    def process(self, action):
        pass

    def reset(self):
        pass

    def stop(self):
        pass

    def is_all_scheduled_episodes_done(self):
        return False
