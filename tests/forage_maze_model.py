"""Host model of foraging first-person mazes (numpy, integer arithmetic).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7j independently of maze.hip, on top of the §7f / §7g / §7h host models (nav_maze_model.py,
gen_maze_model.py, styled_maze_model.py), and reads of a MazeConfig only its options and layout strings:

  kinds     a pickup has a kind 0..3, the layout letters 'A' .. 'D'.  Kind 0 is §7f's apple (apple_reward, (40, 255, 40),
            never ends the episode); kind k >= 1 is pickups[k - 1] = (reward, (r, g, b), ends_episode)
  pickups   entry k of a layout is its k-th pickup cell of any kind, ascending by cell; bit k of `collected` is entry k.  A
            pickup is active while its bit is clear and it does not sit on the episode's goal cell
  reward    the first that applies: goal_reward for a step that ends on the goal cell, the kind's reward for a move into the
            cell of an active pickup, hit_reward for a move into a wall or off the map, else 0.  A reset or a respawn onto
            a pickup collects nothing
  terminal  the time-out, the goal without goal_respawn, or the collection of a kind with ends_episode (also under
            goal_respawn).  A terminal step carries its own reward; the reset that follows brings every pickup back
  frames    the floor of an active pickup's cell has its kind's colour; s_{t+1} shows the pickup just collected gone
  no goal   the goal is (-1, -1): no cell is the goal.  The start is S, or with random_start free cell number
            (word 1 of the reset draw) % n_free; word 0 is unused, the heading is word 2 mod 4 as ever
  generated rooms ranked by §7g's apple keys: the first gen_apples rooms hold 'A', the next gen_pickups[0] 'B', then 'C',
            then 'D'
  totals    record words 4..7 count the collected pickups of kinds 0..3 since the actor's first reset, never zeroed

`frames` False (host_batch(frames=False)): the actor renders nothing (blank frames), for tests of state and rewards over
many steps.
"""
import numpy as np

try:
    import fp_maze_model as FP
    import nav_maze_model as NAV
    import gen_maze_model as GM
    import styled_maze_model as SM
    from maze_model import philox4x32_10, MAZE_STREAM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import nav_maze_model as NAV
    from tests import gen_maze_model as GM
    from tests import styled_maze_model as SM
    from tests.maze_model import philox4x32_10, MAZE_STREAM

H, W, DIRS = FP.H, FP.W, FP.DIRS
FLOOR = np.array(FP.FLOOR, np.uint8)
LETTERS = "ABCD"
FORAGE_FLAG, FORAGE_WORDS = 128, 16

_BLANK = np.zeros((H, W, 3), dtype=np.uint8)
_BLANK.setflags(write=False)


def kind_table(config):
    """[(reward, (r, g, b), ends_episode)] of kinds 0..K."""
    return [(config.apple_reward, NAV.APPLE_FLOOR, False)] + [tuple(k) for k in (config.pickups or [])]


def layout_pickups(layout_string):
    """(cells ascending, kinds) of the pickups of one layout string."""
    cells = [c for c, ch in enumerate(layout_string) if ch in LETTERS]
    return cells, [LETTERS.index(layout_string[c]) for c in cells]


def forage_section(config):
    """The 16 words a forage block ends in."""
    sec = [0] * FORAGE_WORDS
    kinds = config.pickups or []
    sec[0], sec[1] = len(kinds), 1 if config.no_goal else 0
    for k, (reward, (r, g, b), ends) in enumerate(kinds):
        sec[4 + k] = reward
        sec[8 + k] = r | g << 8 | b << 16 | (1 if ends else 0) << 24
    for k, n in enumerate(config.gen_pickups or ()):
        sec[12 + k] = n
    return np.array(sec, dtype=np.int64).astype(np.int32)


def no_goal_start(config, free, start, g, episode, seed):
    """Start cell of a goal-less episode: S, or free cell number word 1 % n_free of the reset draw."""
    if not config.random_start:
        return start
    seed = int(seed) & (2 ** 64 - 1)
    u = philox4x32_10((g, episode, MAZE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return int(free[int(u[1]) % len(free)])


def generate_pickups(N, counts, seed, g, episode):
    """(cells ascending, kinds) of a generated maze: rooms ranked by §7g's apple keys, counts[k] rooms of kind k in turn."""
    R = (N + 1) // 2
    if not sum(counts):
        return [], []
    seed = int(seed) & (2 ** 64 - 1)
    blocks = np.arange((R * R + 3) // 4)             # word r & 3 of the draw with counter word 3 = r >> 2
    u = philox4x32_10((g, episode, GM.APPLE_STREAM, blocks), (seed & 0xFFFFFFFF, seed >> 32))
    aw = [int(w) for w in np.stack(u, 1).reshape(-1)[:R * R]]
    ranked = sorted(range(R * R), key=lambda r: (aw[r] << 8) | r)
    kind_of, first = {}, 0
    for kind, n in enumerate(counts):
        for r in ranked[first:first + n]:
            kind_of[(2 * (r // R)) * N + 2 * (r % R)] = kind
        first += n
    cells = sorted(kind_of)
    return cells, [kind_of[c] for c in cells]


_CACHE = {}


def render(base, x, y, h, N, active):
    """`base` (a frame without pickups) with the floor of the cells of `active`, a frozenset of (cell, (r, g, b)),
    repainted.  Only plain floor pixels change: walls, ceiling and the goal tile keep their bytes."""
    if not active:
        return base
    key = (id(base), x, y, h, active)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is base:
        return hit[1]
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    q = (2 * np.arange(W, dtype=np.int64) + 1 - W)[None, :]
    p = np.maximum(2 * np.arange(H, dtype=np.int64) + 1 - H, 1)[:, None]
    ahead = (2 * H + p) // (2 * p)
    side = (2 * H * q + p * W) // (2 * p * W)
    cx, cy = x + ahead * dx + side * rx, y + ahead * dy + side * ry
    inside = (cx >= 0) & (cx < N) & (cy >= 0) & (cy < N)
    cell = np.where(inside, cy * N + cx, -1)
    floor = (base == FLOOR).all(2) & (np.arange(H)[:, None] >= H // 2)
    out = base.copy()
    for c, colour in active:
        out[floor & (cell == c)] = colour
    out.setflags(write=False)
    if len(_CACHE) > 20000:
        _CACHE.clear()
    _CACHE[key] = (base, out)
    return out


class _Forage(object):
    """Mixin over a navigation actor (static, styled, generated): kinds, ending pickups, goal-less episodes."""

    frames = True

    def _base_config(self):
        return self.config.base if isinstance(self.config, GM.LayoutView) else self.config

    def _pickups(self):
        """(cells, kinds) of the running episode's layout."""
        conf = self._base_config()
        if conf.generate is not None:
            return self._gen_pickups
        if self._static_pickups is None:
            self._static_pickups = layout_pickups(conf.layouts[self.layout])
        return self._static_pickups

    def _regenerate(self):
        super(_Forage, self)._regenerate()
        base = self.config.base
        counts = (base.gen_apples,) + tuple(base.gen_pickups or ())
        self._gen_pickups = generate_pickups(base.N, counts, self.seed, self.g, self.episode + 1)
        self._tail = None

    def reset(self):
        conf = self._base_config()
        if not conf.no_goal:
            super(_Forage, self).reset()
            return
        # without a goal: the bases' reset with the cells drawn here
        if conf.generate is not None:
            self._regenerate()
        self.collected = 0
        N = conf.N
        self.episode += 1
        start = no_goal_start(conf, self.config.free[self.layout], self.config.start[self.layout], self.g, self.episode,
                              self.seed)
        self.gx = self.gy = -1
        self.x, self.y = start % N, start // N
        self.h = FP.reset_heading(conf, self.g, self.episode, self.seed)
        self.ep_steps = 0
        self.frame = self._render()
        self.last_state = {'image': self.frame / 255.0}
        self.last_action = 0
        self.last_reward = 0

    @property
    def goal_cell(self):
        return -1 if self.gx < 0 else self.gy * self.config.N + self.gx

    def active_pickups(self):
        """{cell: (entry, kind)} of the pickups that can be seen and collected."""
        cells, kinds = self._pickups()
        return dict((c, (k, kinds[k])) for k, c in enumerate(cells)
                    if not (self.collected >> k) & 1 and c != self.goal_cell)

    def active_apples(self):             # the base render draws none: this model paints every kind
        return frozenset()

    def _render(self):
        if not self.frames:
            return _BLANK
        base = super(_Forage, self)._render()
        table = kind_table(self._base_config())
        active = frozenset((c, tuple(table[kind][1])) for c, (_, kind) in self.active_pickups().items())
        return render(base, self.x, self.y, self.h, self.config.N, active)

    def process(self, action, flag=0):
        """-> (state, reward, terminal, pixel change); `picked`: the kind collected or -1, `ended_by_pickup`, `timed_out`,
        `at_goal`, `respawned`, `hit`; `on_pickup`: the step left the agent, by a reset or a respawn, on a pickup's cell."""
        conf, N = self._base_config(), self.config.N
        table = kind_table(conf)
        active = self.active_pickups()
        nx, ny, nh, hit = self.move(action)
        moved = (nx, ny) != (self.x, self.y)
        self.x, self.y, self.h = nx, ny, nh
        self.ep_steps += 1
        cell = ny * N + nx
        self.at_goal = cell == self.goal_cell
        self.picked = active[cell][1] if moved and not self.at_goal and cell in active else -1
        ends = self.picked >= 0 and table[self.picked][2]
        limit = conf.max_episode_steps
        timeout = limit > 0 and self.ep_steps >= limit
        terminal = timeout or ends or (self.at_goal and not conf.goal_respawn)
        self.ended_by_pickup = bool(ends)
        self.timed_out = timeout and not ends and (conf.goal_respawn or not self.at_goal)
        self.hit = hit
        if self.at_goal:
            reward = conf.goal_reward
        elif self.picked >= 0:
            reward = table[self.picked][0]
        elif hit:
            reward = conf.hit_reward
        else:
            reward = 0
        if self.picked >= 0:
            self.collected |= 1 << active[cell][0]
            self.totals[self.picked] += 1
        self.respawned = False
        if self.at_goal:
            self.goals_total += 1
            if conf.goal_respawn and not terminal:
                start, self.h = NAV.respawn_cell(self.config, self.layout, self.g, self.episode, self.goals_total,
                                                 self.goal_cell, self.seed)
                self.x, self.y = start % N, start // N
                self.respawned = True
        self.on_pickup = self.respawned and (self.y * N + self.x) in self._pickups()[0]
        frame = self._render()
        pc = FP.pixel_change(frame, self.frame) if self.frames else None
        self.frame = frame
        self.last_state = {'image': frame / 255.0}
        self.last_action = int(action)
        self.last_reward = reward
        return self.last_state, reward, terminal, pc

    def starts_on_pickup(self):
        """The agent stands on a pickup's cell (after a reset: nothing was collected)."""
        return (self.y * self.config.N + self.x) in self._pickups()[0]

    def record(self):
        c = self.collected
        as_i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        return [self.h, as_i32(c & 0xFFFFFFFF), as_i32(c >> 32), self.goals_total] + list(self.totals)

    def apple_record(self):
        """The 65-word record of the episode's pickups: [n, cell | kind << 16 ascending, 0 ...]."""
        cells, kinds = self._pickups()
        rec = np.zeros(GM.APPLE_WORDS, dtype=np.int32)
        rec[0] = len(cells)
        rec[1:1 + len(cells)] = [c | k << 16 for c, k in zip(cells, kinds)]
        return rec

    def actor_record(self):
        """The whole per-actor record: 8 words for a static maze; a generated maze's layout record, this model's pickup
        record and, styled, the nibble words after them."""
        head = np.array(self.record(), dtype=np.int32)
        if self._base_config().generate is None:
            return head
        if getattr(self, "_tail", None) is None:
            N = self.config.N
            tail = super(_Forage, self).actor_record()[len(head):].copy()
            at = GM.REC_HEADER + N * N
            tail[at:at + GM.APPLE_WORDS] = self.apple_record()
            self._tail = tail
        return np.concatenate([head, self._tail])


class _Totals(object):
    def __init__(self, *a, **kw):
        self.totals = [0, 0, 0, 0]
        self._gen_pickups, self._static_pickups, self._tail = ([], []), None, None
        super(_Totals, self).__init__(*a, **kw)


class HostForageMaze(_Totals, _Forage, NAV.HostNavMaze):
    pass


class HostForageStyledMaze(_Totals, _Forage, SM.HostStyledNavMaze):
    pass


class HostForageGenMaze(_Totals, _Forage, GM.HostGenNavMaze):
    pass


class HostForageStyledGenMaze(_Totals, _Forage, SM.HostStyledGenNavMaze):
    pass


def host_batch(config, B, actor_base=0, actors_total=None, seed=0, frames=True):
    """Host models of the global actors [actor_base, actor_base + B) of a forage config.  `frames`: True, False, or the
    number of leading actors that render (the others are blind)."""
    assert config.forage and config.nav
    total = B if actors_total is None else actors_total
    if config.generate is not None:
        cls = HostForageStyledGenMaze if config.styled else HostForageGenMaze
    else:
        cls = HostForageStyledMaze if config.styled else HostForageMaze
    blind = type(cls.__name__ + "Blind", (cls,), {"frames": False})
    n_seeing = B if frames is True else int(frames)
    return [(cls if b < n_seeing else blind)(config, actor_base + b, total, seed) for b in range(B)]
