"""Host model of first-person navigation mazes (numpy, integer arithmetic).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7f independently of maze.hip, on top of tests/fp_maze_model.py (camera, walls, goal tile, reset draws):

  actions   turn set: 0 / 1 turn left / right, 2 / 3 step forward / back; lab set: 0 / 1 look left / right, 2 / 3 strafe
            left / right (-r / +r, r = DIRS[(h + 1) % 4]), 4 / 5 step forward / back
  reward    the first that applies: goal_reward for a step that ends on the goal cell, apple_reward for a move into a cell
            whose apple is still there, hit_reward for a move into a wall or off the map (the agent stays), else 0
  apples    collected by a move into their cell, at most once per episode, restored only at a reset; an apple on the
            episode's goal cell is inactive (neither drawn nor collectable)
  respawn   with goal_respawn the goal is not terminal: the agent moves to S, or to a free cell other than the goal drawn
            from Philox4x32-10 (key = seed, counter = (g, episode, RESPAWN_STREAM, goals_total)), word 1; the heading is
            start_heading or word 2 mod 4; goals_total counts this goal
  time-out  the step at which the episode's step count reaches max_episode_steps is terminal with its own reward
  frames    the floor of every cell with an active, uncollected apple is APPLE_FLOOR; the goal tile keeps its colour

goals_total / apples_total count since the actor's first reset and are never zeroed.  `HostNavMaze` has the attribute
surface OracleActor uses.
"""
import numpy as np

try:
    import fp_maze_model as FP
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests.maze_model import philox4x32_10

H, W, DIRS = FP.H, FP.W, FP.DIRS
FLOOR = np.array(FP.FLOOR, np.uint8)
APPLE_FLOOR = (40, 255, 40)
RESPAWN_STREAM = 0x4D415A52


def respawn_cell(config, layout, g, episode, goals, goal, seed):
    """(start cell, heading) of global actor g's respawn after its goal number `goals` (counted) in episode `episode`."""
    seed = int(seed) & (2 ** 64 - 1)
    u = philox4x32_10((g, episode, RESPAWN_STREAM, goals), (seed & 0xFFFFFFFF, seed >> 32))
    if config.random_start:
        others = [int(c) for c in config.free[layout] if c != goal]
        start = others[int(u[1]) % len(others)]
    else:
        start = config.start[layout]
    heading = config.start_heading if config.start_heading is not None else int(u[2]) % 4
    return start, heading


_CACHE = {}


def render(config, layout, x, y, h, gx, gy, apple_cells):
    """-> uint8 [84, 84, 3]: fp_maze_model.render with the floor of the cells in `apple_cells` (a frozenset of y*N+x)
    drawn as APPLE_FLOOR."""
    img = FP.render(config, layout, x, y, h, gx, gy)
    if not apple_cells:
        return img
    key = (id(config), layout, x, y, h, gx, gy, apple_cells)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is config:
        return hit[1]
    N = config.N
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    q = (2 * np.arange(W, dtype=np.int64) + 1 - W)[None, :]
    p = np.maximum(2 * np.arange(H, dtype=np.int64) + 1 - H, 1)[:, None]
    ahead = (2 * H + p) // (2 * p)                  # cells ahead of the eye, to its right (floor divisions)
    side = (2 * H * q + p * W) // (2 * p * W)
    cx, cy = x + ahead * dx + side * rx, y + ahead * dy + side * ry
    inside = (cx >= 0) & (cx < N) & (cy >= 0) & (cy < N)
    cell = np.where(inside, cy * N + cx, -1)
    floor = (img == FLOOR).all(2) & (np.arange(H)[:, None] >= H // 2)      # plain floor pixels (rows below the horizon)
    on = floor & np.isin(cell, list(apple_cells))
    out = img.copy()
    out[on] = APPLE_FLOOR
    out.setflags(write=False)
    _CACHE[key] = (config, out)
    return out


class HostNavMaze(FP.HostFirstPersonMaze):
    """One navigation-maze actor (MazeConfig.nav): global index g, its layout, the key `seed` of its draws."""

    def __init__(self, config, g=0, actors_total=1, seed=0):
        self.action_size = config.action_size
        self.goals_total = self.apples_total = 0
        self.collected = 0                         # apple bits of the running episode (bit k: the k-th apple cell)
        FP.HostFirstPersonMaze.__init__(self, config, g, actors_total, seed)

    def reset(self):
        self.collected = 0
        FP.HostFirstPersonMaze.reset(self)

    @property
    def goal_cell(self):
        return self.gy * self.config.N + self.gx

    def active_apples(self):
        cells = self.config.apples[self.layout]
        return frozenset(int(c) for k, c in enumerate(cells) if not (self.collected >> k) & 1 and c != self.goal_cell)

    def _render(self):
        return render(self.config, self.layout, self.x, self.y, self.h, self.gx, self.gy, self.active_apples())

    def move(self, action):
        """-> (x, y, h, hit) after `action`."""
        a = int(action)
        if not 0 <= a < self.action_size:          # not an action of the set: nothing happens
            return self.x, self.y, self.h, False
        if self.config.action_set != "lab" or a in (0, 1):
            return FP.HostFirstPersonMaze.move(self, action)
        N = self.config.N
        dx, dy = DIRS[self.h]
        rx, ry = DIRS[(self.h + 1) % 4]
        mx, my = {2: (-rx, -ry), 3: (rx, ry), 4: (dx, dy), 5: (-dx, -dy)}.get(a, (0, 0))
        if (mx, my) == (0, 0):
            return self.x, self.y, self.h, False
        nx, ny = self.x + mx, self.y + my
        if not (0 <= nx < N and 0 <= ny < N) or self.config.walls[self.layout][ny * N + nx]:
            return self.x, self.y, self.h, True
        return nx, ny, self.h, False

    def process(self, action, flag=0):
        """-> (state, reward, terminal, pixel change); `timed_out`: the episode ended at its time-out (not at a
        terminal goal), `at_goal`, `respawned`, `apple`, `hit`: what the step did."""
        conf, N = self.config, self.config.N
        active = self.active_apples()
        nx, ny, nh, hit = self.move(action)
        moved = (nx, ny) != (self.x, self.y)
        self.x, self.y, self.h = nx, ny, nh
        self.ep_steps += 1
        cell = ny * N + nx
        self.at_goal = cell == self.goal_cell
        limit = conf.max_episode_steps
        timeout = limit > 0 and self.ep_steps >= limit
        terminal = timeout if conf.goal_respawn else (self.at_goal or timeout)
        self.timed_out = timeout and (conf.goal_respawn or not self.at_goal)
        self.apple = not self.at_goal and moved and cell in active
        self.hit = hit
        if self.at_goal:
            reward = conf.goal_reward
        elif self.apple:
            reward = conf.apple_reward
        elif hit:
            reward = conf.hit_reward
        else:
            reward = 0
        if self.apple:
            self.collected |= 1 << int(np.searchsorted(conf.apples[self.layout], cell))
            self.apples_total += 1
        self.respawned = False
        if self.at_goal:
            self.goals_total += 1
            if conf.goal_respawn and not terminal:
                start, self.h = respawn_cell(conf, self.layout, self.g, self.episode, self.goals_total, self.goal_cell,
                                             self.seed)
                self.x, self.y = start % N, start // N
                self.respawned = True
        frame = self._render()
        pc = FP.pixel_change(frame, self.frame)
        self.frame = frame
        self.last_state = {'image': frame / 255.0}
        self.last_action = int(action)
        self.last_reward = reward
        return self.last_state, reward, terminal, pc

    def record(self):
        """The per-actor record of the device: (heading, apple bits lo, hi, goals_total, apples_total, 0, 0, 0)."""
        c = self.collected
        lo, hi = c & 0xFFFFFFFF, c >> 32
        as_i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        return [self.h, as_i32(lo), as_i32(hi), self.goals_total, self.apples_total, 0, 0, 0]


def host_batch(config, B, actor_base=0, actors_total=None, seed=0):
    """Host models of the global actors [actor_base, actor_base + B)."""
    total = B if actors_total is None else actors_total
    return [HostNavMaze(config, actor_base + b, total, seed) for b in range(B)]
