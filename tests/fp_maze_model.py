"""Host model of the first-person maze view (numpy, integer arithmetic).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7e independently of maze.hip.  The state is a cell (x, y) and a heading h (0: +x, 1: +y, 2: -x,
3: -y); actions 0 / 1 turn left / right, 2 / 3 step forward / back (a step into a wall or off the map stays: reward -1);
the goal is terminal with +1 and max_episode_steps works as in tests/maze_model.py.  Resets draw goal and start exactly as
the top-down maze (maze_model.reset_cells) and, with start_heading None, the heading as word 2 of the same draw, mod 4.

The camera sits at the cell centre.  Column i casts W d + q r (q = 2i + 1 - W); the k-th forward cell boundary is crossed
at t = (2k+1)/2 and the m-th side boundary at t = (2m+1) W / 2|q|; the first wall / off-map cell gives t = tn / td, and row
y is wall iff |2y+1-H| tn < H td.  Other rows are ceiling (above the horizon) or floor; a floor pixel (p = 2y+1-H > 0)
lies floor((2H+p) / 2p) cells ahead and floor((2Hq + pW) / 2pW) cells to the right of the eye.  Frames are uint8; images
handed out are bytes / 255, and the pixel change is the reference formula on them, evaluated exactly (sum of |bytes| over
48 * 255, rounded once to float32).

`HostFirstPersonMaze` has the attribute surface OracleActor uses (last_state, last_action, last_reward, process, reset).
"""
import numpy as np

try:
    from maze_model import philox4x32_10, reset_cells, MAZE_STREAM
except ImportError:            # imported as tests.<module>
    from tests.maze_model import philox4x32_10, reset_cells, MAZE_STREAM

H = W = 84
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))        # heading -> forward (dx, dy); right = DIRS[(h + 1) % 4]
CEILING = (0, 0, 0)
FLOOR, GOAL_FLOOR = (40, 40, 40), (40, 40, 255)
WALL_X, WALL_Y = 255, 160                          # shade of faces crossed along x / along y
PC_DENOM = 48 * 255


def reset_heading(config, g, episode, seed):
    """Heading of global actor g's episode `episode`: start_heading, or Philox word 2 of the reset draw mod 4."""
    if config.start_heading is not None:
        return config.start_heading
    seed = int(seed) & (2 ** 64 - 1)
    u = philox4x32_10((g, episode, MAZE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return int(u[2]) % 4


def cast(walls, N, ex, ey, h, i):
    """Column i's ray from cell (ex, ey) along heading h -> (tn, td, border, xface, ties): the first wall / off-map cell at
    t = tn / td; `ties` counts equal boundary crossings met on the way (the design says there are none)."""
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    q = 2 * i + 1 - W
    aq, sg = abs(q), (1 if q > 0 else -1)
    f = s = k = m = ties = 0
    while True:
        fwd, side = (2 * k + 1) * aq, (2 * m + 1) * W
        ties += fwd == side
        if fwd < side:
            f += 1
            tn, td, xface = 2 * k + 1, 2, dx != 0
            k += 1
        else:
            s += sg
            tn, td, xface = (2 * m + 1) * W, 2 * aq, rx != 0
            m += 1
        cx, cy = ex + f * dx + s * rx, ey + f * dy + s * ry
        if not (0 <= cx < N and 0 <= cy < N):
            return tn, td, True, xface, ties
        if walls[cy * N + cx]:
            return tn, td, False, xface, ties


_CACHE = {}        # (id(config), layout, x, y, h, gx, gy) -> (config, frame): random walks revisit their views


def render(config, layout, x, y, h, gx, gy):
    """-> uint8 [84, 84, 3] view from cell (x, y) along heading h (a read-only array)."""
    key = (id(config), layout, x, y, h, gx, gy)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is config:
        return hit[1]
    N = config.N
    walls = config.walls[layout]
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    gf = (gx - x) * dx + (gy - y) * dy            # the goal cell: ahead of the eye, to its right
    gs = (gx - x) * rx + (gy - y) * ry
    tn, td = np.zeros(W, np.int64), np.zeros(W, np.int64)
    colour = np.zeros((W, 3), np.uint8)
    for i in range(W):
        tn[i], td[i], border, xface, _ = cast(walls, N, x, y, h, i)
        colour[i, 1 if border else 0] = WALL_X if xface else WALL_Y
    q = 2 * np.arange(W, dtype=np.int64) + 1 - W
    p = (2 * np.arange(H, dtype=np.int64) + 1 - H)[:, None]
    wall = np.abs(p) * tn[None, :] < H * td[None, :]
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[:] = CEILING
    floor = ~wall & (p > 0)
    img[floor] = FLOOR
    if config.show_goal:
        pp = np.maximum(p, 1)                      # (rows above the horizon are not floor)
        ahead = (2 * H + pp) // (2 * pp)
        side = (2 * H * q[None, :] + pp * W) // (2 * pp * W)
        img[floor & (ahead == gf) & (side == gs)] = GOAL_FLOOR
    img[wall] = np.broadcast_to(colour[None], (H, W, 3))[wall]
    img.setflags(write=False)
    _CACHE[key] = (config, img)
    return img


def pixel_change(new, old):
    """20 x 20 float32 pixel change of two uint8 frames: the reference formula on bytes / 255, evaluated exactly."""
    d = np.abs(new[2:-2, 2:-2].astype(np.int64) - old[2:-2, 2:-2].astype(np.int64)).sum(2)
    s = d.reshape(20, 4, 20, 4).sum(axis=(1, 3))
    return (s / float(PC_DENOM)).astype(np.float32)


class HostFirstPersonMaze(object):
    """One first-person actor: global index g, its layout (config.layout_ids), the key `seed` of its reset draws."""

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
        self.h = reset_heading(self.config, self.g, self.episode, self.seed)
        self.ep_steps = 0
        self.frame = self._render()
        self.last_state = {'image': self.frame / 255.0}
        self.last_action = 0
        self.last_reward = 0

    def _render(self):
        return render(self.config, self.layout, self.x, self.y, self.h, self.gx, self.gy)

    def move(self, action):
        """-> (x, y, h, hit) after `action`."""
        N = self.config.N
        a = int(action)
        if a in (0, 1):
            return self.x, self.y, (self.h + (1 if a == 1 else 3)) % 4, False
        sgn = 1 if a == 2 else -1
        dx, dy = DIRS[self.h]
        nx, ny = self.x + sgn * dx, self.y + sgn * dy
        if not (0 <= nx < N and 0 <= ny < N) or self.config.walls[self.layout][ny * N + nx]:
            return self.x, self.y, self.h, True
        return nx, ny, self.h, False

    def process(self, action, flag=0):
        """-> (state, reward, terminal, pixel change); `timed_out` tells a time-out from a goal."""
        self.x, self.y, self.h, hit = self.move(action)
        self.ep_steps += 1
        at_goal = (self.x, self.y) == (self.gx, self.gy)
        limit = self.config.max_episode_steps
        self.timed_out = not at_goal and limit > 0 and self.ep_steps >= limit
        terminal = at_goal or self.timed_out
        reward = 1 if at_goal else (-1 if hit else 0)
        frame = self._render()
        pc = pixel_change(frame, self.frame)
        self.frame = frame
        self.last_state = {'image': frame / 255.0}
        self.last_action = int(action)
        self.last_reward = reward
        return self.last_state, reward, terminal, pc

    def stop(self):
        pass


def host_batch(config, B, actor_base=0, actors_total=None, seed=0):
    """Host models of the global actors [actor_base, actor_base + B)."""
    total = B if actors_total is None else actors_total
    return [HostFirstPersonMaze(config, actor_base + b, total, seed) for b in range(B)]
