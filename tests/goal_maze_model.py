"""Host model of goal-sense first-person mazes (numpy, integer arithmetic).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7i independently of maze.hip and of MazeConfig.distance_field, on top of the §7f / §7g / §7h host models
(nav_maze_model.py, gen_maze_model.py, styled_maze_model.py), whose frames, moves, apples, respawns and resets it keeps:

  field     d(c): length of the shortest 4-connected path over free cells from cell c to the episode's goal, d(goal) = 0;
            NO_PATH in walls.  Computed (a deque breadth-first search) at every reset, after the goal is drawn and, for a
            generated maze, after the layout is; a respawn at the goal keeps it
  objective of a state (cell (x, y), heading h, goal (gx, gy)), with d = DIRS[h] and r = DIRS[(h + 1) % 4]:
            gf = (gx - x) dx + (gy - y) dy, gs = (gx - x) rx + (gy - y) ry; last_state['objective'] = [gf / 32, gs / 32,
            d(x, y) / 512] (float64, exact)
  reward    the §7f reward plus progress_reward * (d before the action - d of the cell the move ends in, before any
            respawn or reset): 0 for turns, looks and hits, goal_reward + progress_reward for a goal step
  record    words 5..7 of the navigation record are gf, gs, d of the current state; the per-actor record ends in the
            field, 16 bits per cell: cell c in half c & 1 of word c >> 1, NO_PATH in the unused half of the last word
"""
from collections import deque

import numpy as np

try:
    import fp_maze_model as FP
    import nav_maze_model as NAV
    import gen_maze_model as GM
    import styled_maze_model as SM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import nav_maze_model as NAV
    from tests import gen_maze_model as GM
    from tests import styled_maze_model as SM

DIRS = FP.DIRS
NO_PATH = 0xFFFF
OFFSET_SCALE, DISTANCE_SCALE = 32.0, 512.0


def serpentine_layout(N=21):
    """Free rows joined at alternating ends, S at the first cell and G at the last: the longest shortest path an N x N
    layout of this family has (N = 21: 11 rows of 20 moves and 10 joints of 2: 240)."""
    rows = []
    for y in range(N):
        if y % 2 == 0:
            rows.append("-" * N)
        else:
            gap = N - 1 if (y // 2) % 2 == 0 else 0
            rows.append("".join("-" if x == gap else "+" for x in range(N)))
    rows[0] = "S" + rows[0][1:]
    last = N - 1 if ((N - 1) // 2) % 2 == 0 else 0
    rows[N - 1] = rows[N - 1][:last] + "G" + rows[N - 1][last + 1:]
    return rows


def dist_words(N):
    return (N * N + 1) // 2


def bfs(walls, N, goal):
    """-> list of N * N path distances to cell `goal` over the free cells of `walls` (bool [N * N]); NO_PATH in walls."""
    d = [NO_PATH] * (N * N)
    d[goal] = 0
    todo = deque([goal])
    while todo:
        c = todo.popleft()
        x, y = c % N, c // N
        for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            n = ny * N + nx
            if 0 <= nx < N and 0 <= ny < N and not walls[n] and d[n] == NO_PATH and n != goal:
                d[n] = d[c] + 1
                todo.append(n)
    return d


def field_words(N, d):
    """The field as the device keeps it -> int32 [dist_words(N)]."""
    half = np.full(2 * dist_words(N), NO_PATH, dtype=np.int64)
    half[:N * N] = d
    words = half[0::2] | (half[1::2] << 16)
    return (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def goal_offset(x, y, h, gx, gy):
    """(gf, gs): the goal's offset ahead of and to the right of a camera in cell (x, y) with heading h."""
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    return (gx - x) * dx + (gy - y) * dy, (gx - x) * rx + (gy - y) * ry


_BLANK = np.zeros((FP.H, FP.W, 3), dtype=np.uint8)
_BLANK.setflags(write=False)


class _Sense(object):
    """Mixin over a navigation actor (static, generated, styled): the distance field, the objective, the shaped reward.
    `frames` False (host_batch(frames=False)): the actor renders nothing (its frames are blank), for tests of state and
    rewards over many steps; what a frame shows is tested where `frames` is True."""

    frames = True

    def _walls(self):
        return self.config.walls[self.layout]

    def _render(self):
        return super(_Sense, self)._render() if self.frames else _BLANK

    def reset(self):
        super(_Sense, self).reset()
        self.dist = bfs(self._walls(), self.config.N, self.goal_cell)
        self._field_words = field_words(self.config.N, self.dist)
        self._tail = None                      # the layout, apple and style words of the episode (generated mazes)
        self.last_state['objective'] = self.objective()

    def distance(self):
        return self.dist[self.y * self.config.N + self.x]

    def sense(self):
        """(gf, gs, d) of the current state."""
        return goal_offset(self.x, self.y, self.h, self.gx, self.gy) + (self.distance(),)

    def objective(self):
        gf, gs, d = self.sense()
        return np.array([gf / OFFSET_SCALE, gs / OFFSET_SCALE, d / DISTANCE_SCALE], dtype=np.float64)

    def distance_field(self):
        N = self.config.N
        return np.array(self.dist, dtype=np.uint16).reshape(N, N)

    def process(self, action, flag=0):
        N = self.config.N
        self.d_before = self.distance()
        nx, ny, _, _ = self.move(action)
        self.d_after = self.dist[ny * N + nx]
        state, reward, terminal, pc = super(_Sense, self).process(action, flag)
        reward = reward + self.config.progress_reward * (self.d_before - self.d_after)
        self.last_reward = reward
        state['objective'] = self.objective()
        return state, reward, terminal, pc

    def record(self):
        rec = super(_Sense, self).record()
        rec[5:8] = self.sense()
        return rec

    def actor_record(self):
        """The whole per-actor record: the record of the actor it is mixed into, then the field."""
        head = np.array(self.record(), dtype=np.int32)
        base = getattr(super(_Sense, self), "actor_record", None)
        if base is None:
            return np.concatenate([head, self._field_words])
        if self._tail is None:                 # (constant over an episode: collected apples are bits of the head)
            self._tail = base()[len(head):]
        return np.concatenate([head, self._tail, self._field_words])


class HostGoalMaze(_Sense, NAV.HostNavMaze):
    pass


class HostGoalStyledMaze(_Sense, SM.HostStyledNavMaze):
    pass


class HostGoalGenMaze(_Sense, GM.HostGenNavMaze):
    pass


class HostGoalStyledGenMaze(_Sense, SM.HostStyledGenNavMaze):
    pass


def host_batch(config, B, actor_base=0, actors_total=None, seed=0, frames=True):
    """Host models of the global actors [actor_base, actor_base + B) of a goal-sense config."""
    assert config.goal_sense and config.nav
    total = B if actors_total is None else actors_total
    if config.generate is not None:
        cls = HostGoalStyledGenMaze if config.styled else HostGoalGenMaze
    else:
        cls = HostGoalStyledMaze if config.styled else HostGoalMaze
    if not frames:
        cls = type(cls.__name__ + "Blind", (cls,), {"frames": False})
    return [cls(config, actor_base + b, total, seed) for b in range(B)]
