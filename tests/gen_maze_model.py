"""Host model of generated first-person mazes (numpy).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7g independently of maze.hip and of MazeConfig.generated_layout, with plain Kruskal on the test Philox
(tests/maze_model.py):

  rooms    R = (N + 1) // 2 per side; room (i, j) is cell (2i, 2j); every other cell is a wall unless an edge opens it
  edges    E = 2 R (R - 1): horizontal first, row-major (rooms (i, j), (i + 1, j): e = j (R - 1) + i, cell (2i + 1, 2j)),
           then vertical (rooms (i, j), (i, j + 1): e = R (R - 1) + j R + i, cell (2i, 2j + 1))
  weights  edge e: word e & 3 of Philox4x32-10(key = seed, counter = (g, episode, GEN_STREAM, e >> 2)); the sort key is
           (weight << 8) | e
  open     the minimum spanning tree of the room grid under the keys, plus the `loops` lightest edges outside it
  apples   room r = j R + i: word r & 3 of the draw with counter (g, episode, APPLE_STREAM, r >> 2), key (weight << 8) | r;
           the `apples` rooms with the smallest keys hold one

The actors are the first-person / navigation host models (fp_maze_model.py, nav_maze_model.py) whose `reset` first
regenerates the layout of the episode it starts; goal, start and heading are then drawn over it as over any layout.
"""
import numpy as np

try:
    import fp_maze_model as FP
    import nav_maze_model as NAV
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import nav_maze_model as NAV
    from tests.maze_model import philox4x32_10

GEN_STREAM, APPLE_STREAM = 0x4D415A47, 0x4D415A41
NAV_WORDS, REC_HEADER, APPLE_WORDS = 8, 18, 65


def _weights(seed, g, episode, stream, n):
    seed = int(seed) & (2 ** 64 - 1)
    out = []
    for blk in range((n + 3) // 4):
        u = philox4x32_10((g, episode, stream, blk), (seed & 0xFFFFFFFF, seed >> 32))
        out += [int(w) for w in u]
    return out[:n]


def edges(N):
    """[(room a, room b, cell)] of the room grid in edge order; room index j * R + i."""
    R = (N + 1) // 2
    out = []
    for j in range(R):
        for i in range(R - 1):
            out.append((j * R + i, j * R + i + 1, (2 * j) * N + 2 * i + 1))
    for j in range(R - 1):
        for i in range(R):
            out.append((j * R + i, (j + 1) * R + i, (2 * j + 1) * N + 2 * i))
    return out


def generate(N, loops, apples, seed, g, episode):
    """-> (walls: bool [N * N], apple cells ascending) of global actor g's episode `episode`."""
    R = (N + 1) // 2
    ed = edges(N)
    w = _weights(seed, g, episode, GEN_STREAM, len(ed))
    order = sorted(range(len(ed)), key=lambda e: (w[e] << 8) | e)
    parent = list(range(R * R))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    walls = np.ones(N * N, dtype=bool)
    for j in range(R):
        for i in range(R):
            walls[(2 * j) * N + 2 * i] = False
    rejected = []
    for e in order:                      # Kruskal
        a, b, cell = ed[e]
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            walls[cell] = False
        else:
            rejected.append(e)
    for e in rejected[:loops]:
        walls[ed[e][2]] = False
    cells = []
    if apples:
        aw = _weights(seed, g, episode, APPLE_STREAM, R * R)
        rooms = sorted(range(R * R), key=lambda r: (aw[r] << 8) | r)[:apples]
        cells = sorted((2 * (r // R)) * N + 2 * (r % R) for r in rooms)
    return walls, cells


def layout_string(walls, apple_cells):
    s = np.where(walls, "+", "-")
    s[list(apple_cells)] = "A"
    return "".join(s)


class LayoutView(object):
    """The base config's options over the one layout of an episode: what the host models read of a config."""

    def __init__(self, base, seed, g, episode):
        self.base = base
        walls, apples = generate(base.N, base.gen_loops, base.gen_apples, seed, g, episode)
        self.walls = [walls]
        self.free = [np.flatnonzero(~walls).astype(np.int32)]
        self.apples = [np.array(apples, dtype=np.int32)]
        self.start, self.goal = [-1], [-1]

    def __getattr__(self, name):         # N, flags, rewards, limits, action set ...
        return getattr(self.base, name)

    def layout_ids(self, actor_base, batch, actors_total):
        return np.zeros(batch, dtype=np.int32)


class _Regenerates(object):
    def _regenerate(self):
        base = self.config.base if isinstance(self.config, LayoutView) else self.config
        for cache in (FP._CACHE, NAV._CACHE):        # frames of past episodes' layouts are never asked for again
            if len(cache) > 4000:
                cache.clear()
        self.config = LayoutView(base, self.seed, self.g, self.episode + 1)

    def layout_record(self):
        """The layout and apple records the device keeps for the actor (after the 8 navigation words)."""
        N = self.config.N
        walls, free, apples = self.config.walls[0], self.config.free[0], self.config.apples[0]
        bits = np.zeros(448, dtype=np.int64)
        bits[:N * N] = walls
        rec = np.zeros(REC_HEADER + N * N + APPLE_WORDS, dtype=np.int64)
        rec[:14] = (bits.reshape(14, 32) << np.arange(32)).sum(1)
        rec[14], rec[15], rec[16], rec[17] = -1, -1, len(free), -1
        rec[REC_HEADER:REC_HEADER + len(free)] = free
        a = rec[REC_HEADER + N * N:]
        a[0] = len(apples)
        a[1:1 + len(apples)] = apples
        return (rec & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

    def actor_record(self):
        """The whole per-actor record: navigation words, layout record, apple record."""
        return np.concatenate([np.array(self.record(), dtype=np.int32), self.layout_record()])


class HostGenMaze(_Regenerates, FP.HostFirstPersonMaze):
    """One actor of a generated maze without navigation options."""

    def reset(self):
        self._regenerate()
        FP.HostFirstPersonMaze.reset(self)

    def record(self):
        return [self.h, 0, 0, 0, 0, 0, 0, 0]


class HostGenNavMaze(_Regenerates, NAV.HostNavMaze):
    """One actor of a generated navigation maze (apples, rewards, respawn, Lab's actions)."""

    def reset(self):
        self._regenerate()
        NAV.HostNavMaze.reset(self)


def host_batch(config, B, actor_base=0, actors_total=None, seed=0):
    """Host models of the global actors [actor_base, actor_base + B)."""
    total = B if actors_total is None else actors_total
    cls = HostGenNavMaze if config.nav else HostGenMaze
    return [cls(config, actor_base + b, total, seed) for b in range(B)]
