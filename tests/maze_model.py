"""Host model of the configured maze (numpy).  TEST INFRASTRUCTURE ONLY.

Restates the semantics of Environment.register_maze_config independently of the kernels: moves, walls, clamping, hits and
rewards as the reference's maze (maze_environment.py:76-128) with the bound N - 1; a goal reached is terminal with reward
+1; a time-out (the episode's step count reaching max_episode_steps) is terminal with the move's reward; every reset draws
the goal, then the start, from Philox4x32-10 (key = seed, counter = (global actor, episode, MAZE_STREAM, 0)).  Frames are
84 x 84 x 3 with 0 / 1 values: walls in channel 0, the agent in channel 1, the goal in channel 2 when shown.

`HostMaze` has the attribute surface OracleActor uses (x, y, last_state, last_action, last_reward, process, reset), so
instances can be handed to oracle.trainer.OracleTrainer(envs=[...]).
"""
import numpy as np

from oracle.maze import calc_pixel_change

MAZE_STREAM = 0x4D415A45
_M32 = np.uint64(0xFFFFFFFF)
ACTION_DELTA = ((0, -1), (0, 1), (-1, 0), (1, 0))   # UP, DOWN, LEFT, RIGHT


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter = 4 uint32 words, key = 2 -> 4 uint32 words (numpy arrays, any
    broadcastable shapes)."""
    c = [np.asarray(w, dtype=np.uint64) & _M32 for w in counter]
    k0, k1 = (np.asarray(w, dtype=np.uint64) & _M32 for w in key)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                  # < 2^64: exact in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & _M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return [w.astype(np.uint32) for w in c]


def reset_cells(config, layout, g, episode, seed):
    """(goal cell, start cell) of global actor g's episode `episode`: cells are y * N + x."""
    free = config.free[layout]
    seed = int(seed) & (2 ** 64 - 1)
    u = philox4x32_10((g, episode, MAZE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    if config.random_goal:
        gi = int(u[0]) % len(free)
        goal = int(free[gi])
    else:
        goal = config.goal[layout]
        gi = int(np.searchsorted(free, goal))
    if config.random_start:
        j = int(u[1]) % (len(free) - 1)
        start = int(free[j if j < gi else j + 1])
    else:
        start = config.start[layout]
    return goal, start


def render(config, layout, x, y, gx, gy):
    N = config.N
    c = 84 // N
    img = np.zeros((84, 84, 3), dtype=np.float64)
    walls = config.walls[layout].reshape(N, N)
    img[:, :, 0] = np.kron(walls.astype(np.float64), np.ones((c, c)))
    img[c * y:c * y + c, c * x:c * x + c, 1] = 1.0
    if config.show_goal:
        img[c * gy:c * gy + c, c * gx:c * gx + c, 2] = 1.0
    return img


class HostMaze(object):
    """One configured-maze actor: global index g, its layout (config.layout_ids), the key `seed` of its reset draws."""

    action_size = 4

    def __init__(self, config, g=0, actors_total=1, seed=0):
        self.config, self.g, self.seed = config, int(g), int(seed)
        self.layout = int(config.layout_ids(self.g, 1, actors_total)[0])
        self.episode = -1
        self.reset()

    def reset(self):
        N = self.config.N
        self.episode += 1
        goal, start = reset_cells(self.config, self.layout, self.g, self.episode, self.seed)
        self.gx, self.gy = goal % N, goal // N
        self.x, self.y = start % N, start // N
        self.ep_steps = 0
        self.last_state = {'image': self._render()}
        self.last_action = 0
        self.last_reward = 0

    def _render(self):
        return render(self.config, self.layout, self.x, self.y, self.gx, self.gy)

    def move(self, action):
        N = self.config.N
        dx, dy = ACTION_DELTA[int(action)]
        nx, ny = self.x + dx, self.y + dy
        clamped = not (0 <= nx < N and 0 <= ny < N)
        nx, ny = min(max(nx, 0), N - 1), min(max(ny, 0), N - 1)
        hit_wall = bool(self.config.walls[self.layout][ny * N + nx])
        if hit_wall:
            nx, ny = self.x, self.y
        return nx, ny, clamped or hit_wall

    def process(self, action, flag=0):
        """-> (state, reward, terminal, pixel change); `timed_out` tells a time-out from a goal."""
        self.x, self.y, hit = self.move(action)
        self.ep_steps += 1
        at_goal = (self.x, self.y) == (self.gx, self.gy)
        limit = self.config.max_episode_steps
        self.timed_out = not at_goal and limit > 0 and self.ep_steps >= limit
        terminal = at_goal or self.timed_out
        reward = 1 if at_goal else (-1 if hit else 0)
        image = self._render()
        pc = calc_pixel_change(image, self.last_state['image'])
        self.last_state = {'image': image}
        self.last_action = int(action)
        self.last_reward = reward
        return self.last_state, reward, terminal, pc

    def stop(self):
        pass


def host_batch(config, B, actor_base=0, actors_total=None, seed=0):
    """Host models of the global actors [actor_base, actor_base + B)."""
    total = B if actors_total is None else actors_total
    return [HostMaze(config, actor_base + b, total, seed) for b in range(B)]


def random_layout(N, rs, wall_frac=0.3, marks="SG"):
    """A random N x N layout with 4-connected free cells: walls are added one at a time where they keep the free cells
    connected.  `marks` are placed on distinct free cells."""
    grid = np.zeros(N * N, dtype=bool)

    def connected(g):
        free = np.flatnonzero(~g)
        seen, todo = {free[0]}, [free[0]]
        while todo:
            c = todo.pop()
            x, y = c % N, c // N
            for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                d = ny * N + nx
                if 0 <= nx < N and 0 <= ny < N and not g[d] and d not in seen:
                    seen.add(d)
                    todo.append(d)
        return len(seen) == len(free)

    for c in rs.permutation(N * N)[:int(wall_frac * N * N)]:
        grid[c] = True
        if not connected(grid):
            grid[c] = False
    cells = np.array(['+' if w else '-' for w in grid])
    free = np.flatnonzero(~grid)
    for ch, c in zip(marks, rs.choice(free, len(marks), replace=False)):
        cells[c] = ch
    return "".join(cells)
