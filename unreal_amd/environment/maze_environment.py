"""Maze environment on the device (/root/reference/environment/maze_environment.py:10-128).

`BatchedMazeEnvironment` steps B mazes with one kernel launch and writes frames straight into the
replay ring; `MazeEnvironment` is the reference's batch-1 object surface over the same kernels
(`process(action) -> (image, reward, terminal, pixel_change)`, `reset`, `last_state` dict with 'image',
`last_action`, `last_reward`), with the adapter semantics of SURVEY H1 (`flag` ignored).

`MazeConfig` describes user mazes (Environment.register_maze_config): N x N layouts in the reference map's alphabet, optional
random start / goal cells drawn at every reset, an optional goal block in channel 2 and an optional episode step limit.
With view="first_person" the same mazes are seen through a raycast camera (`FirstPersonMazeEnvironment`, maze.hip);
`batched_maze_environment` picks the class from the config.  First-person configs may be navigation mazes:
apples ('A' cells), configurable rewards, respawn at the goal and Lab's six actions.  With generate=N a first-person
config has no layouts: every reset writes a new maze for the actor on the device;
`MazeConfig.generated_layout` computes the same maze on the host.  With wall_styles, first-person wall cells written as
digits 1..7 (or drawn as landmarks of a generated maze, gen_landmark_density) show a colour and a stripe pattern of
their own.  With goal_sense a first-person config hands the agent a measurement vector, the goal's offset
in its own frame and the shortest-path distance to it, as the state's 'objective', and progress_reward pays for getting
closer.  With pickups a first-person config has up to three more kinds of pickup next to the apple ('B', 'C',
'D' cells), each with its own reward, floor colour and ends-the-episode bit, and with no_goal its episodes have no goal
cell at all: the foraging levels."""
from collections import deque

import numpy as np
import torch

from .. import ops
from . import environment

REFERENCE_MAP = ("--+---G"
                 "--+-+++"
                 "S-+---+"
                 "--+++--"
                 "--+-+--"
                 "--+----"
                 "-----++")       # maze_environment.py:18-25


class MazeConfig(object):
    """Validated layouts and options of a configured maze, and the int32 configuration block the kernels read (the maze
    tail of the unreal_maze_* entries in include/unreal_hip.h).  Raises ValueError on a malformed configuration."""
    SIZES = (7, 12, 14, 21)          # the grid sizes whose cells tile the 84-px frame: 12, 7, 6, 4 px
    MAX_LAYOUTS = 1024
    RANDOM_START, RANDOM_GOAL, SHOW_GOAL, NAV, GENERATED, STYLED, GOAL_SENSE = 1, 2, 4, 8, 16, 32, 64
    # foraging: a 16-word section after everything else (maze_common.h): [K, mode (1: no goal), 0, 0, the
    # kinds' rewards x 3, 0, r | g << 8 | b << 16 | ends << 24 x 3, 0, gen_pickups x 3, 0]; an apple entry is then
    # cell | kind << 16 (kind 0: 'A')
    FORAGE, FORAGE_WORDS, FORAGE_NO_GOAL, MAX_KINDS, PICKUP_CHARS = 128, 16, 1, 3, "ABCD"
    FORAGE_REWARD, FORAGE_COLOUR, FORAGE_GEN = 4, 8, 12
    # goal sense: objective = [gf / 32, gs / 32, d / 512]; progress_reward is word 6 of the navigation header
    OBJECTIVE_SIZE, OFFSET_SCALE, DISTANCE_SCALE, PROGRESS_WORD, NO_PATH = 3, 32, 512, 6, 0xFFFF
    GEN_STREAM, APPLE_STREAM = 0x4D415A47, 0x4D415A41      # Philox counter word 2 of a generated maze's edge / apple draws
    STYLE_STREAM = 0x4D415A53                              # ... and of its landmark draws
    # style section after everything else (maze_common.h): header [S, gen_landmark_density, 0 x 6], 8 style words
    # r | g << 8 | b << 16 | pattern << 24, then per static layout (N * N + 7) // 8 words of 4-bit style ids
    STYLE_HEADER, STYLE_SLOTS, MAX_STYLES, WALL_CHARS = 8, 8, 7, "+1234567"
    HEADER, RECORD_HEADER = 8, 18
    VIEWS = ("top_down", "first_person")
    # navigation extension after the layout records (maze_common.h): header [goal, apple, hit reward, mode, 0 x 4], then
    # per layout [n apples, apple cells ascending, padding to 64]
    NAV_HEADER, NAV_RECORD, MAX_APPLES = 8, 65, 64
    NAV_RESPAWN, NAV_LAB_ACTIONS = 1, 2
    ACTION_SETS = ("turn", "lab")
    MAX_REWARD = 100

    def __init__(self, layouts=None, random_start=False, random_goal=False, show_goal=False, max_episode_steps=0,
                 view="top_down", start_heading=None, goal_reward=1, apple_reward=1, hit_reward=-1,
                 goal_respawn=False, action_set="turn", generate=None, gen_loops=0, gen_apples=0, wall_styles=None,
                 gen_landmark_density=0, goal_sense=False, progress_reward=0, pickups=None, gen_pickups=None,
                 no_goal=False):
        self.generate, self.gen_loops, self.gen_apples = None, 0, 0
        self._check_styles(wall_styles, gen_landmark_density, view, generate)
        self._check_forage(pickups, gen_pickups, no_goal, view, generate, random_goal, show_goal, goal_respawn,
                           goal_sense, goal_reward, max_episode_steps)
        if generate is not None:
            self._check_generate(layouts, random_start, random_goal, view, generate, gen_loops, gen_apples)
            layouts = []
        elif isinstance(gen_loops, (bool, np.bool_)) or isinstance(gen_apples, (bool, np.bool_)) or gen_loops != 0 or \
                gen_apples != 0:
            raise ValueError("gen_loops and gen_apples are settings of a generated maze; generate is None")
        elif layouts is None or isinstance(layouts, str) or not len(layouts):
            raise ValueError("layouts: a non-empty list of layouts (strings, or lists of row strings)")
        if len(layouts) > self.MAX_LAYOUTS:
            raise ValueError("%d layouts: at most %d per config" % (len(layouts), self.MAX_LAYOUTS))
        self.random_start, self.random_goal, self.show_goal = bool(random_start), bool(random_goal), bool(show_goal)
        if int(max_episode_steps) != max_episode_steps or not 0 <= max_episode_steps <= 2 ** 31 - 1:
            raise ValueError("max_episode_steps %r: an integer in [0, 2**31 - 1] (0: no limit; the kernels count steps "
                             "in int32)" % (max_episode_steps,))
        self.max_episode_steps = int(max_episode_steps)
        if self.no_goal and self.max_episode_steps == 0:
            raise ValueError("no_goal needs max_episode_steps > 0 (without an ending kind only the time-out ends an "
                             "episode)")
        if view not in self.VIEWS:
            raise ValueError("view %r: one of %s" % (view, self.VIEWS))
        if start_heading is not None:
            if view != "first_person":
                raise ValueError("start_heading is a first-person setting; view is %r" % (view,))
            if isinstance(start_heading, bool) or int(start_heading) != start_heading or not 0 <= start_heading <= 3:
                raise ValueError("start_heading %r: None (drawn at every reset) or 0..3 (0: +x, 1: +y, 2: -x, 3: -y)"
                                 % (start_heading,))
            start_heading = int(start_heading)
        self.view, self.start_heading = view, start_heading
        rewards = dict(goal_reward=goal_reward, apple_reward=apple_reward, hit_reward=hit_reward,
                       progress_reward=progress_reward)
        for k, v in rewards.items():
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or \
                    not -self.MAX_REWARD <= v <= self.MAX_REWARD:
                raise ValueError("%s %r: an integer in [-%d, %d]" % (k, v, self.MAX_REWARD, self.MAX_REWARD))
        self.goal_reward, self.apple_reward, self.hit_reward = int(goal_reward), int(apple_reward), int(hit_reward)
        self.goal_sense, self.progress_reward = bool(goal_sense), int(progress_reward)
        if self.goal_sense and view != "first_person":
            raise ValueError("goal_sense is a first-person setting; view is %r" % (view,))
        if self.progress_reward and not self.goal_sense:
            raise ValueError("progress_reward %d needs goal_sense (the path distance it pays for)" % self.progress_reward)
        if action_set not in self.ACTION_SETS:
            raise ValueError("action_set %r: one of %s" % (action_set, self.ACTION_SETS))
        self.goal_respawn, self.action_set = bool(goal_respawn), action_set
        nav_options = (self.goal_reward, self.apple_reward, self.hit_reward, self.goal_respawn, action_set) != \
            (1, 1, -1, False, "turn")
        if nav_options and view != "first_person":
            raise ValueError("goal_reward, apple_reward, hit_reward, goal_respawn and action_set are first-person "
                             "settings; view is %r" % (view,))
        if self.goal_respawn and self.max_episode_steps == 0:
            raise ValueError("goal_respawn needs max_episode_steps > 0 (the time-out ends every episode)")
        if self.goal_respawn and self.random_goal and not self.random_start:
            raise ValueError("goal_respawn with random_goal needs random_start (a respawn at S could be on the goal)")
        self.layouts = [self._parse(i, lay) for i, lay in enumerate(layouts)]
        sizes = set(int(round(len(m) ** 0.5)) for m in self.layouts) if self.generate is None else {self.generate}
        if len(sizes) != 1:
            raise ValueError("layouts of one config must share their size; got %s" % sorted(sizes))
        self.N = sizes.pop()
        self.L = len(self.layouts)
        self.walls, self.start, self.goal, self.free, self.apples, self.styles = [], [], [], [], [], []
        self.pickup_cells, self.pickup_kinds = [], []
        for i, m in enumerate(self.layouts):
            self._check(i, m)
        # a navigation maze: any of the options above, or an apple in a layout (the default block stays word for word)
        # (a generated maze with apples is one too)
        # (and so is a goal-sense maze: its block carries the rewards header, its actors keep records)
        # (and a forage maze)
        self.nav = nav_options or any(len(a) for a in self.apples) or self.gen_apples > 0 or self.goal_sense or self.forage

    def _check_styles(self, wall_styles, density, view, generate):
        integer = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))
        self.wall_styles, self.gen_landmark_density = None, 0
        if wall_styles is not None:
            if view != "first_person":
                raise ValueError("wall_styles is a first-person setting; view is %r" % (view,))
            seq = (list, tuple, np.ndarray)
            if not isinstance(wall_styles, seq) or not 1 <= len(wall_styles) <= self.MAX_STYLES:
                raise ValueError("wall_styles: a list of 1 to %d styles (r, g, b, pattern)" % self.MAX_STYLES)
            styles = []
            for k, st in enumerate(wall_styles):
                if not isinstance(st, seq) or len(st) != 4 or not all(integer(v) and 0 <= v <= 255 for v in st):
                    raise ValueError("wall_styles[%d] %r: (r, g, b, pattern), four integers in 0..255" % (k, st))
                styles.append(tuple(int(v) for v in st))
            self.wall_styles = styles
        if not integer(density) or not 0 <= density <= 256:
            raise ValueError("gen_landmark_density %r: an integer in [0, 256]" % (density,))
        if density and (generate is None or wall_styles is None):
            raise ValueError("gen_landmark_density needs generate and wall_styles (static layouts take their styles "
                             "from the digits 1..7)")
        self.gen_landmark_density = int(density)

    @property
    def styled(self):
        return self.wall_styles is not None

    def _check_forage(self, pickups, gen_pickups, no_goal, view, generate, random_goal, show_goal, goal_respawn,
                      goal_sense, goal_reward, max_episode_steps):
        integer = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))
        seq = (list, tuple, np.ndarray)
        self.pickups, self.gen_pickups, self.no_goal = None, None, False
        if not isinstance(no_goal, (bool, np.bool_)):
            raise ValueError("no_goal %r: a bool" % (no_goal,))
        for name, used in (("pickups", pickups is not None), ("gen_pickups", gen_pickups is not None),
                           ("no_goal", bool(no_goal))):
            if used and view != "first_person":
                raise ValueError("%s is a first-person setting; view is %r" % (name, view))
        if pickups is not None:
            if goal_sense:
                raise ValueError("pickups with goal_sense: words 5..7 of the actor record cannot count the kinds and hold "
                                 "the goal's offset and distance")
            if not isinstance(pickups, seq) or not 1 <= len(pickups) <= self.MAX_KINDS:
                raise ValueError("pickups: None, or a list of 1 to %d kinds (reward, (r, g, b), ends_episode)"
                                 % self.MAX_KINDS)
            kinds = []
            for k, kind in enumerate(pickups):
                if not isinstance(kind, seq) or len(kind) != 3:
                    raise ValueError("pickups[%d] %r: (reward, (r, g, b), ends_episode)" % (k, kind))
                reward, colour, ends = kind
                if not integer(reward) or not -self.MAX_REWARD <= reward <= self.MAX_REWARD:
                    raise ValueError("pickups[%d]: reward %r: an integer in [-%d, %d]"
                                     % (k, reward, self.MAX_REWARD, self.MAX_REWARD))
                if not isinstance(colour, seq) or len(colour) != 3 or not all(integer(v) and 0 <= v <= 255 for v in colour):
                    raise ValueError("pickups[%d]: colour %r: (r, g, b), three integers in 0..255" % (k, colour))
                if not isinstance(ends, (bool, np.bool_)):
                    raise ValueError("pickups[%d]: ends_episode %r: a bool" % (k, ends))
                kinds.append((int(reward), tuple(int(v) for v in colour), bool(ends)))
            self.pickups = kinds
        if gen_pickups is not None:
            if generate is None or self.pickups is None:
                raise ValueError("gen_pickups needs generate and pickups (static layouts place their pickups as 'B', 'C', "
                                 "'D' cells)")
            if not isinstance(gen_pickups, seq) or len(gen_pickups) != len(self.pickups) or \
                    not all(integer(v) and v >= 0 for v in gen_pickups):
                raise ValueError("gen_pickups %r: %d integers >= 0, one per kind of pickups"
                                 % (gen_pickups, len(self.pickups)))
            self.gen_pickups = tuple(int(v) for v in gen_pickups)
        if no_goal:
            if random_goal:
                raise ValueError("no_goal: random_goal must be False (there is no goal to draw)")
            if show_goal or goal_respawn or goal_sense:
                raise ValueError("no_goal: show_goal, goal_respawn and goal_sense need a goal")
            if isinstance(goal_reward, (bool, np.bool_)) or goal_reward != 1:
                raise ValueError("no_goal: goal_reward %r is never paid (leave it at its default)" % (goal_reward,))
            self.no_goal = True

    @property
    def forage(self):
        """A forage config: pickups or no_goal is used."""
        return self.pickups is not None or self.no_goal

    @staticmethod
    def style_words(N):
        """int32 words of one layout's 4-bit style ids (UNREAL_MAZE_STYLE_WORDS(N))."""
        return (N * N + 7) // 8

    @staticmethod
    def gen_rooms(N):
        """(R, E): rooms per side of a generated N x N maze (the even cells) and edges between neighbouring rooms."""
        R = (N + 1) // 2
        return R, 2 * R * (R - 1)

    def _check_generate(self, layouts, random_start, random_goal, view, generate, gen_loops, gen_apples):
        integer = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))
        if layouts is not None:
            raise ValueError("generate: a generated maze has no layouts (layouts must be None)")
        if not integer(generate) or generate not in self.SIZES:
            raise ValueError("generate %r: None, or a grid size N in %s" % (generate, self.SIZES))
        if view != "first_person":
            raise ValueError("generate is a first-person setting; view is %r" % (view,))
        if self.no_goal and not random_start:
            raise ValueError("generate with no_goal needs random_start (a generated layout has no 'S' cell)")
        if not self.no_goal and not (random_start and random_goal):
            raise ValueError("generate needs random_start and random_goal (a generated layout has no 'S' or 'G' cell)")
        R, E = self.gen_rooms(int(generate))
        if not integer(gen_loops) or not 0 <= gen_loops <= E - (R * R - 1):
            raise ValueError("gen_loops %r: an integer in [0, %d] (the edges of the %d x %d room grid outside its "
                             "spanning tree)" % (gen_loops, E - (R * R - 1), R, R))
        if not integer(gen_apples) or not 0 <= gen_apples <= min(self.MAX_APPLES, R * R):
            raise ValueError("gen_apples %r: an integer in [0, %d] (at most one per room, %d per layout)"
                             % (gen_apples, min(self.MAX_APPLES, R * R), self.MAX_APPLES))
        if self.gen_pickups is not None and gen_apples + sum(self.gen_pickups) > min(self.MAX_APPLES, R * R):
            raise ValueError("gen_apples %d + gen_pickups %r: at most %d pickups (one per room, %d per layout)"
                             % (gen_apples, self.gen_pickups, min(self.MAX_APPLES, R * R), self.MAX_APPLES))
        self.generate, self.gen_loops, self.gen_apples = int(generate), int(gen_loops), int(gen_apples)

    def generated_layout(self, seed, g, episode):
        """The layout of global actor g's episode `episode` under the key `seed`, as a string in the layout alphabet
        ('+' wall, '-' free, 'A' apple, 'B' / 'C' / 'D' a pickup of kind 1 / 2 / 3: the rooms ranked after the apples'
        by the same keys, gen_pickups[0] of 'B', then 'C', then 'D'): what the device writes at that reset.  Rooms are the even cells;
        edge e between neighbouring rooms (horizontal first, row-major, then vertical) has the key (w << 8) | e, w = word
        e & 3 of Philox4x32-10(key = seed, counter = (g, episode, GEN_STREAM, e >> 2)); open are the minimum spanning
        tree of the room grid under these keys and the gen_loops lightest other edges.  Apples lie in the gen_apples
        rooms with the smallest keys (w << 8) | r drawn with APPLE_STREAM.  A styled config writes the
        landmarks as digits: wall cell c with w = word c & 3 of the draw with counter (g, episode, STYLE_STREAM, c >> 2) is
        one iff (w >> 24) < gen_landmark_density, of style 1 + (w & 0xFFFFFF) % len(wall_styles)."""
        if self.generate is None:
            raise ValueError("generated_layout: the config is not a generated maze (generate is None)")
        N = self.N
        R, E = self.gen_rooms(N)
        eh = R * (R - 1)
        e = np.arange(E)
        a = np.where(e < eh, (e // (R - 1)) * R + e % (R - 1), e - eh)      # rooms a, b of every edge
        b = np.where(e < eh, a + 1, a + R)
        room_cell = lambda r: 2 * (r // R) * N + 2 * (r % R)
        edge_cell = room_cell(a) + np.where(e < eh, 1, N)
        key = (_philox_words(seed, g, episode, self.GEN_STREAM, E).astype(np.uint64) << np.uint64(8)) | e.astype(np.uint64)
        # Prim from room 0: with distinct keys every algorithm finds the same tree
        in_tree = np.zeros(R * R, dtype=bool)
        in_tree[0] = True
        tree = np.zeros(E, dtype=bool)
        for _ in range(R * R - 1):
            cut = np.flatnonzero(in_tree[a] != in_tree[b])
            pick = cut[np.argmin(key[cut])]
            tree[pick] = True
            in_tree[a[pick]] = in_tree[b[pick]] = True
        rest = np.flatnonzero(~tree)
        extra = rest[np.argsort(key[rest])[:self.gen_loops]]
        cells = np.full(N * N, "+")
        cells[room_cell(np.arange(R * R))] = "-"
        cells[edge_cell[tree]] = "-"
        cells[edge_cell[extra]] = "-"
        counts = (self.gen_apples,) + (self.gen_pickups or ())
        if sum(counts):
            r = np.arange(R * R)
            akey = (_philox_words(seed, g, episode, self.APPLE_STREAM, R * R).astype(np.uint64) << np.uint64(8)) | \
                r.astype(np.uint64)
            ranked, first = np.argsort(akey), 0
            for kind, n in enumerate(counts):
                cells[room_cell(ranked[first:first + n])] = self.PICKUP_CHARS[kind]
                first += n
        if self.styled and self.gen_landmark_density:
            w = _philox_words(seed, g, episode, self.STYLE_STREAM, N * N).astype(np.int64)
            mark = (cells == "+") & ((w >> 24) < self.gen_landmark_density)
            style = 1 + (w & 0xFFFFFF) % len(self.wall_styles)
            cells[mark] = style[mark].astype(str)
        return "".join(cells)

    def _parse(self, i, lay):
        if isinstance(lay, str):
            m = "".join(lay.split())
        else:
            rows = [str(r) for r in lay]
            if len(set(len(r) for r in rows)) != 1 or len(rows) != len(rows[0]):
                raise ValueError("layout %d: %d rows of lengths %s, not N x N" % (i, len(rows), [len(r) for r in rows]))
            m = "".join(rows)
        n = int(round(len(m) ** 0.5))
        if n * n != len(m) or n not in self.SIZES:
            raise ValueError("layout %d: %d cells; supported are N x N with N in %s" % (i, len(m), self.SIZES))
        bad = set(m) - set("+-SGA1234567" + self.PICKUP_CHARS[1:1 + len(self.pickups or ())])
        if bad & set(self.PICKUP_CHARS) and self.pickups is not None:
            raise ValueError("layout %d: pickup %s, but pickups holds %d kinds ('B' is kind 1)"
                             % (i, sorted(bad & set(self.PICKUP_CHARS)), len(self.pickups)))
        if bad:
            raise ValueError("layout %d: unknown characters %s (use + wall, - free, S start, G goal, A apple, 1..7 "
                             "styled wall; B, C, D a pickup of pickups)" % (i, sorted(bad)))
        digits = [int(ch) for ch in set(m) if ch.isdigit()]
        if digits and max(digits) > len(self.wall_styles or ()):
            raise ValueError("layout %d: wall digit %d, but wall_styles holds %d styles"
                             % (i, max(digits), len(self.wall_styles or ())))
        if "A" in m and self.view != "first_person":
            raise ValueError("layout %d: apples ('A') are a first-person setting; view is %r" % (i, self.view))
        if m.count("A") > self.MAX_APPLES:
            raise ValueError("layout %d: %d apples; at most %d per layout" % (i, m.count("A"), self.MAX_APPLES))
        n_pick = sum(m.count(ch) for ch in self.PICKUP_CHARS)
        if n_pick > self.MAX_APPLES:
            raise ValueError("layout %d: %d pickups of all kinds; at most %d per layout (an actor has %d collected bits)"
                             % (i, n_pick, self.MAX_APPLES, self.MAX_APPLES))
        return m

    def _check(self, i, m):
        N = int(round(len(m) ** 0.5))
        n_s, n_g = m.count("S"), m.count("G")
        if not self.random_start and n_s != 1:
            raise ValueError("layout %d: %d 'S' cells; exactly one is needed without random_start" % (i, n_s))
        if self.no_goal:
            if n_g:
                raise ValueError("layout %d: %d 'G' cells; a no_goal config has none" % (i, n_g))
        elif not self.random_goal and n_g != 1:
            raise ValueError("layout %d: %d 'G' cells; exactly one is needed without random_goal" % (i, n_g))
        wall = self.WALL_CHARS
        free = [c for c in range(N * N) if m[c] not in wall]
        if self.random_start and len(free) < 2:
            raise ValueError("layout %d: %d free cells; random_start needs at least 2" % (i, len(free)))
        if not free:
            raise ValueError("layout %d has no free cell" % i)
        seen, todo = {free[0]}, deque([free[0]])        # 4-connectivity of the free cells (BFS)
        while todo:
            c = todo.popleft()
            x, y = c % N, c // N
            for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                d = ny * N + nx
                if 0 <= nx < N and 0 <= ny < N and m[d] not in wall and d not in seen:
                    seen.add(d)
                    todo.append(d)
        if len(seen) != len(free):
            raise ValueError("layout %d: the free cells are not 4-connected (%d of %d reachable)" % (i, len(seen), len(free)))
        self.walls.append(np.array([ch in wall for ch in m], dtype=bool))
        self.styles.append(np.array([int(ch) if ch.isdigit() else 0 for ch in m], dtype=np.uint8))
        self.start.append(m.index("S") if n_s == 1 else -1)
        self.goal.append(m.index("G") if n_g == 1 else -1)
        self.free.append(np.array(free, dtype=np.int32))
        self.apples.append(np.array([c for c in range(N * N) if m[c] == "A"], dtype=np.int32))
        if self.forage:       # every pickup, ascending by cell, and its kind ('A': 0); self.apples keeps the 'A' cells
            cells = [c for c in range(N * N) if m[c] in self.PICKUP_CHARS]
            self.pickup_cells.append(np.array(cells, dtype=np.int32))
            self.pickup_kinds.append(np.array([self.PICKUP_CHARS.index(m[c]) for c in cells], dtype=np.int32))

    @property
    def flags(self):
        return (self.RANDOM_START * self.random_start) | (self.RANDOM_GOAL * self.random_goal) | \
            (self.SHOW_GOAL * self.show_goal) | (self.NAV * self.nav) | (self.GENERATED * (self.generate is not None)) | \
            (self.STYLED * self.styled) | (self.GOAL_SENSE * self.goal_sense) | (self.FORAGE * self.forage)

    @property
    def action_size(self):
        return 6 if self.action_set == "lab" else 4

    @property
    def reward_bound(self):
        """max |reward| over the kinds of step (1 for every config without navigation rewards): a goal step pays
        goal_reward + p (it always gets one cell closer), an apple step apple_reward +- p, a hit hit_reward, any other
        move +- p, with p = progress_reward.  A forage config: a pickup of kind k pays its own reward, and
        without a goal goal_reward is never paid."""
        p = self.progress_reward
        kinds = [abs(r) for r, _, _ in self.pickups or ()]
        goal = [] if self.no_goal else [abs(self.goal_reward + p)]
        return max(goal + kinds + [abs(self.apple_reward) + abs(p), abs(self.hit_reward), abs(p)])

    @staticmethod
    def dist_words(N):
        """int32 words of one actor's distance field, 16 bits per cell (UNREAL_MAZE_DIST_WORDS(N))."""
        return (N * N + 1) // 2

    @property
    def record_words(self):
        """int32 words of the per-actor record the kernels keep for this config (0: none, a plain heading array)."""
        dist = self.dist_words(self.N) if self.goal_sense else 0
        if self.generate is not None:
            return ops.gen_record_words(self.N, self.styled) + dist
        return ops.NAV_RECORD + dist if self.nav else 0

    def distance_field(self, layout, goal):
        """Path distances to cell `goal` (y * N + x) over `layout`, a layout string or an index into this config's
        layouts -> uint16 [N, N] ([y, x]): the length of the shortest 4-connected path over free cells, NO_PATH in walls:
        what the device writes at a reset."""
        N = self.N
        if isinstance(layout, str):
            wall = np.array([ch in self.WALL_CHARS for ch in "".join(layout.split())], dtype=bool)
        else:
            wall = self.walls[layout]
        d = np.full(N * N, self.NO_PATH, dtype=np.uint16)
        d[goal] = 0
        todo = deque([int(goal)])
        while todo:
            c = todo.popleft()
            x, y = c % N, c // N
            for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                n = ny * N + nx
                if 0 <= nx < N and 0 <= ny < N and not wall[n] and d[n] == self.NO_PATH and n != goal:
                    d[n] = d[c] + 1
                    todo.append(n)
        return d.reshape(N, N)

    def block(self, seed):
        """-> int32 numpy array: header [N, L, flags, max_episode_steps, seed lo, seed hi, record words, start heading + 1
        (first person with a fixed heading; else 0)], then per
        layout [wall bits of cell y*N+x as 7 x (lo, hi) uint32, S cell, G cell, n_free, index of G in the free list,
        free cells ascending] (-1: none); a navigation maze (flag NAV) appends [goal reward, apple reward, hit reward, mode
        (1: goal_respawn, 2: Lab's actions), 0, 0, 0, 0] and per layout [n apples, apple cells ascending, 0 padding to
        65 words]; a goal-sense maze (flag GOAL_SENSE) is a navigation maze whose header word 6 is
        progress_reward.  A generated maze (flag GENERATED) has L = 0 and no records: after the header come the 8 words
        [goal reward, apple reward, hit reward, mode, gen_loops, gen_apples, 0, 0]; the layout and apple records are
        per actor, written on the device at every reset.  A styled maze (flag STYLED) appends, after all of
        this, [S, gen_landmark_density, 0 x 6], the 8 style words r | g << 8 | b << 16 | pattern << 24 (unused: 0) and,
        per static layout, (N * N + 7) // 8 words of 4-bit style ids (cell c: nibble c & 7 of word c >> 3).  A forage
        maze (flag FORAGE, always with NAV) appends, after all of this, the 16 words [K, mode (1: no goal), 0,
        0, rewards of kinds 1..3, 0, r | g << 8 | b << 16 | ends << 24 of kinds 1..3, 0, gen_pickups, 0]; its apple
        records hold every pickup, ascending by cell, as cell | kind << 16 ('A': kind 0), and a layout record of a
        no_goal maze has G = -1."""
        N, rec = self.N, self.RECORD_HEADER + self.N * self.N
        seed = int(seed) & (2 ** 64 - 1)
        out = np.zeros(self.HEADER + self.L * rec, dtype=np.int64)
        heading = 0 if self.start_heading is None else self.start_heading + 1
        out[:8] = [N, self.L, self.flags, self.max_episode_steps, seed & 0xFFFFFFFF, seed >> 32, rec, heading]
        for l in range(self.L):
            r = out[self.HEADER + l * rec:self.HEADER + (l + 1) * rec]
            bits = np.zeros(448, dtype=np.int64)
            bits[:N * N] = self.walls[l]
            words = (bits.reshape(14, 32) << np.arange(32)).sum(1)
            r[:14] = words
            free, g = self.free[l], self.goal[l]
            r[14], r[15], r[16] = self.start[l], g, len(free)
            r[17] = int(np.searchsorted(free, g)) if g >= 0 else -1
            r[self.RECORD_HEADER:self.RECORD_HEADER + len(free)] = free
        if self.nav or self.generate is not None:
            ext = np.zeros(self.NAV_HEADER + self.L * self.NAV_RECORD, dtype=np.int64)
            mode = self.NAV_RESPAWN * self.goal_respawn | self.NAV_LAB_ACTIONS * (self.action_set == "lab")
            ext[:6] = [self.goal_reward, self.apple_reward, self.hit_reward, mode, self.gen_loops, self.gen_apples]
            ext[self.PROGRESS_WORD] = self.progress_reward
            for l, a in enumerate(self.apples):
                r = ext[self.NAV_HEADER + l * self.NAV_RECORD:]
                if self.forage:
                    a = self.pickup_cells[l] | self.pickup_kinds[l] << 16
                r[0] = len(a)
                r[1:1 + len(a)] = a
            out = np.concatenate([out, ext])
        if self.styled:
            sw = self.style_words(N)
            sec = np.zeros(self.STYLE_HEADER + self.STYLE_SLOTS + self.L * sw, dtype=np.int64)
            sec[0], sec[1] = len(self.wall_styles), self.gen_landmark_density
            for k, (r, g, b, pat) in enumerate(self.wall_styles):
                sec[self.STYLE_HEADER + k] = r | g << 8 | b << 16 | pat << 24
            for l, ids in enumerate(self.styles):
                nib = np.zeros(8 * sw, dtype=np.int64)
                nib[:N * N] = ids
                sec[self.STYLE_HEADER + self.STYLE_SLOTS + l * sw:][:sw] = (nib.reshape(sw, 8) << (4 * np.arange(8))).sum(1)
            out = np.concatenate([out, sec])
        if self.forage:
            sec = np.zeros(self.FORAGE_WORDS, dtype=np.int64)
            sec[0], sec[1] = len(self.pickups or ()), self.FORAGE_NO_GOAL * self.no_goal
            for k, (reward, (r, g, b), ends) in enumerate(self.pickups or ()):
                sec[self.FORAGE_REWARD + k] = reward
                sec[self.FORAGE_COLOUR + k] = r | g << 8 | b << 16 | int(ends) << 24
            for k, n in enumerate(self.gen_pickups or ()):
                sec[self.FORAGE_GEN + k] = n
            out = np.concatenate([out, sec])
        return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

    def layout_ids(self, actor_base, batch, actors_total):
        """Layout of global actors [actor_base, actor_base + batch): g * L // actors_total (contiguous blocks)."""
        g = np.arange(actor_base, actor_base + batch, dtype=np.int64)
        return (g * self.L // int(actors_total)).astype(np.int32)

    def layout_config(self, layout_string):
        """A config with this one's options and the single static layout `layout_string` (host-side views of a generated
        maze: its walls, free cells and apples as a MazeConfig)."""
        return MazeConfig([layout_string], self.random_start, self.random_goal, self.show_goal, self.max_episode_steps,
                          self.view, self.start_heading, self.goal_reward, self.apple_reward, self.hit_reward,
                          self.goal_respawn, self.action_set, wall_styles=self.wall_styles, goal_sense=self.goal_sense,
                          progress_reward=self.progress_reward, pickups=self.pickups, no_goal=self.no_goal)

    @staticmethod
    def reference():
        """The reference's map as a configuration (renders and steps exactly like the unconfigured maze)."""
        return MazeConfig([REFERENCE_MAP])


def _philox_words(seed, g, episode, stream, n):
    """Words 0 .. n-1 of Philox4x32-10 (Salmon et al., SC'11) with key = seed and counters (g, episode, stream, i >> 2):
    word i is output word i & 3 of counter i >> 2 -> uint32 [n]."""
    m32 = np.uint64(0xFFFFFFFF)
    seed = int(seed) & (2 ** 64 - 1)
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    c = [np.full_like(blocks, int(g) & 0xFFFFFFFF), np.full_like(blocks, int(episode) & 0xFFFFFFFF),
         np.full_like(blocks, stream), blocks]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]        # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).reshape(-1)[:n].astype(np.uint32)


def check_final_obs(config):
    """Time-limit bootstrapping covers first-person mazes without goal_sense: raises ValueError for the rest."""
    if config is None or config.view != "first_person":
        raise ValueError("time-limit bootstrapping is out of scope for top-down mazes: it needs a MazeConfig with "
                         "view='first_person'")
    if config.goal_sense:
        raise ValueError("time-limit bootstrapping is out of scope for goal_sense mazes: the final state's objective "
                         "vector is not kept")
    if not config.max_episode_steps > 0:
        raise ValueError("time-limit bootstrapping needs a step limit (max_episode_steps > 0)")


def check_depth_labels(config):
    """Depth labels exist for first-person mazes: raises ValueError for the reference's map and every
    top-down config."""
    if config is None or config.view != "first_person":
        raise ValueError("depth labels are out of scope for top-down mazes: they need a MazeConfig with "
                         "view='first_person'")


class BatchedMazeEnvironment(object):
    ACTION_SIZE = 4
    frame_scale = 1.0          # ring bytes are the pixel values themselves (0 / 1)

    def __init__(self, batch, history_size, device="cuda:0", config=None, actor_base=0, actors_total=None, seed=0,
                 final_obs=False, depth_labels=False, bonus=False):
        """`bonus`: exploration bonus: the ring keeps r_bonus beside r_reward.
        `depth_labels`: depth prediction, first-person configs only: every kernel that changes an actor's
        state is followed by the launch that writes the 12 depth classes of its view into ring.r_depth.
        `config`: a MazeConfig (None: the reference's map).  `actor_base` / `actors_total`: global index of actor 0 and
        the number of actors over every rank (layouts are assigned and reset draws keyed by the global index);
        `seed`: key of the reset draws.  `final_obs`: time-limit bootstrapping, first-person configs without
        goal_sense only: the rollout steps keep the final observation of an episode that ends by max_episode_steps alone
        in ring.final_obs and flag it 2 instead of 1."""
        self.B = batch
        self.config = config
        if final_obs:
            check_final_obs(config)
        if depth_labels:
            check_depth_labels(config)
        self.depth_labels = bool(depth_labels)
        sense = config is not None and config.goal_sense
        self.ring = ops.Ring(batch, history_size, torch.device(device), maze_state=config is not None,
                             nav=config is not None and config.nav,
                             gen=(config.generate or 0) if config is not None else 0,
                             gen_styled=config is not None and config.styled,
                             objective_size=config.OBJECTIVE_SIZE if sense else 0, sense=config.N if sense else 0,
                             final_obs=bool(final_obs), depth=self.depth_labels, bonus=bool(bonus))
        self.maze = None
        if config is not None:
            total = batch if actors_total is None else int(actors_total)
            if actor_base < 0 or actor_base + batch > total:
                raise ValueError("actors [%d, %d) outside the %d actors of the job" % (actor_base, actor_base + batch, total))
            block = torch.from_numpy(config.block(seed)).to(self.ring.count.device)
            self.ring.layout.copy_(torch.from_numpy(config.layout_ids(actor_base, batch, total)))
            view = ops.MAZE_FIRST_PERSON if config.view == "first_person" else ops.MAZE_TOP_DOWN
            if config.generate is not None:
                view = ops.MAZE_FIRST_PERSON_GENERATED
            if config.goal_sense:                  # kernels of their own
                view = ops.MAZE_FIRST_PERSON_SENSE if config.generate is None else ops.MAZE_FIRST_PERSON_GENERATED_SENSE
            if config.forage:                      # and so have forage blocks
                view = ops.MAZE_FIRST_PERSON_FORAGE if config.generate is None else ops.MAZE_FIRST_PERSON_GENERATED_FORAGE
            self.maze = (view, config.N, block, int(actor_base)) + ((True,) if config.styled else ())
        self.reset()

    def view(self, b0, b1):
        """The environments [b0, b1) as a batched environment of their own (shares the ring memory).  `base_actor` = b0:
        frame indices the view's rollout_step prepares are indices into THIS environment's ring."""
        v = object.__new__(BatchedMazeEnvironment)
        v.B, v.ring = b1 - b0, ops.ring_view(self.ring, b0, b1)
        v.base_actor = b0
        v.config = self.config
        v.depth_labels = getattr(self, "depth_labels", False)
        v.maze = None if self.maze is None else self.maze[:3] + (self.maze[3] + b0,) + self.maze[4:]
        return v

    @staticmethod
    def get_action_size():
        return 4

    @property
    def objective_size(self):
        return self.ring.objective_size

    def _objective(self, nxt=None):
        """Goal-sense configs: the objective of every actor's current state into its ring slot, after every kernel that
        changes the state (and into the next step's LSTM-input rows, next to the columns the step has written).  With
        depth_labels, at the same points: the depth classes of every actor's current view into its slot."""
        if getattr(self, "depth_labels", False):
            ops.maze_depth_labels(self.ring, self.maze)
        if not self.ring.objective_size:
            return
        if nxt and nxt.get("next_lar") is not None:
            ops.maze_objective(self.ring, nxt["next_lar"], nxt["lar_ld"], nxt["lar_col0"] + nxt["A"] + 1)
        else:
            ops.maze_objective(self.ring)

    def reset(self, mask=None):
        ops.maze_reset(self.ring, mask, maze=self.maze)
        self._objective()

    def process(self, actions, active=None, out_reward=None, out_terminal=None, reset_on_terminal=True,
                track_score=False):
        ops.maze_step(self.ring, actions, active, out_reward, out_terminal, reset_on_terminal, track_score, maze=self.maze)
        self._objective()

    def rollout_step(self, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                     index_parent=False, **nxt):
        """process() + the rollout loop's bookkeeping (+ the next step's frame indices / LSTM-input columns) fused.
        `index_parent` (views only): the prepared frame indices address the ring this view was cut from."""
        ops.maze_rollout_step(self.ring, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                              base_actor=getattr(self, "base_actor", 0) if index_parent else 0, maze=self.maze,
                              final_obs=self.ring.final_obs, **nxt)
        self._objective(nxt)

    def policy_rollout_step(self, net, feat, ld, u, pi_out, v_out, actions, out_reward, out_terminal, active, active_log_t,
                            n_steps, terminal_end, index_parent=False, **nxt):
        """The policy head + action draw of `net` on the feature rows `feat` and rollout_step() in one launch."""
        p = net.p
        if self.config is not None:
            nxt["A"] = self.config.action_size
        ops.maze_policy_rollout_step(self.ring, feat, ld, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                     p["b_base_fc_v"], u, pi_out, v_out, actions, out_reward, out_terminal, active,
                                     active_log_t, n_steps, terminal_end,
                                     base_actor=getattr(self, "base_actor", 0) if index_parent else 0, maze=self.maze,
                                     final_obs=self.ring.final_obs, **nxt)
        self._objective(nxt)

    @property
    def fused_encoder_ok(self):
        """True where policy_rollout_step_encode serves this environment: a top-down maze (the reference's map or a
        config), without a final-observation store or depth labels (first person only anyway)."""
        top_down = self.maze is None or self.maze[0] == ops.MAZE_TOP_DOWN
        return top_down and self.ring.final_obs is None and not getattr(self, "depth_labels", False) and \
            not self.ring.objective_size

    def policy_rollout_step_encode(self, net, feat, ld, u, pi_out, v_out, actions, out_reward, out_terminal, active,
                                   active_log_t, n_steps, terminal_end, f2_out, c1_out, relu_bits, f2_max, c1_max,
                                   index_parent=False, **nxt):
        """policy_rollout_step() and `net`'s conv encoder of the observations it leaves, in one launch: row b of f2_out /
        c1_out / relu_bits is what net.encoder_forward gives for next_idx[b] (bit for bit)."""
        p = net.p
        tmpl = getattr(self, "_wall_templates", None)
        if tmpl is None:            # once per environment (a view builds its own): layouts never change
            tmpl = self._wall_templates = ops.maze_wall_templates(self.maze, 1 if self.config is None else self.config.L,
                                                                  self.ring.frames.device)
        ops.maze_policy_rollout_step_encode(self.ring, feat, ld, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                            p["b_base_fc_v"], u, pi_out, v_out, actions, out_reward, out_terminal, active,
                                            active_log_t, n_steps, terminal_end, tmpl, net.frame_scale,
                                            p["W_base_conv1"], p["b_base_conv1"], p["W_base_conv2"], p["b_base_conv2"],
                                            f2_out, c1_out, relu_bits, net.enc_prepared, f2_max=f2_max, c1_max=c1_max,
                                            base_actor=getattr(self, "base_actor", 0) if index_parent else 0,
                                            maze=self.maze, **nxt)

    def current_distances(self):
        """The distance fields of the running episodes of a goal-sense config -> uint16 [B, N, N] ([b, y, x]): path
        distance of every cell to the actor's goal, MazeConfig.NO_PATH in walls."""
        if self.config is None or not self.config.goal_sense:
            raise ValueError("current_distances: the config has no goal_sense")
        N = self.config.N
        words = self.ring.actor_records.cpu().numpy()[:, self.ring.record_words - ops.dist_words(N):]
        halves = np.ascontiguousarray(words).view(np.uint16)              # little-endian: half c & 1 of word c >> 1
        return halves[:, :N * N].reshape(self.B, N, N).copy()

    def current_layouts(self):
        """The layouts the actors of a generated maze are in -> (walls, apples): bool [B, N, N] (True: wall; [b, y, x])
        and a list of B int arrays of apple cells y * N + x, ascending (collected ones included).  A forage config
        (DESIGN §7j): a third item, a list of B layout strings with the letters 'A' .. 'D' of every pickup, and the
        second lists the cells of every kind."""
        if self.config is None or self.config.generate is None:
            raise ValueError("current_layouts: the config is not a generated maze")
        N = self.config.N
        rec = self.ring.actor_records.cpu().numpy()[:, ops.NAV_RECORD:ops.gen_record_words(N)]
        words = rec[:, :14].astype(np.int64) & 0xFFFFFFFF
        bits = (words[:, :, None] >> np.arange(32)) & 1
        walls = bits.reshape(self.B, 448)[:, :N * N].astype(bool).reshape(self.B, N, N)
        arec = rec[:, ops.MAZE_RECORD_HEADER + N * N:]
        if self.config.forage:
            entries = [arec[b, 1:1 + arec[b, 0]] for b in range(self.B)]
            letters = []
            for b, e in enumerate(entries):
                cells = np.where(walls[b].reshape(-1), "+", "-")
                cells[e & 0xFFFF] = np.array(list(MazeConfig.PICKUP_CHARS))[(e >> 16) & 3]
                letters.append("".join(cells))
            return walls, [e & 0xFFFF for e in entries], letters
        return walls, [arec[b, 1:1 + arec[b, 0]].copy() for b in range(self.B)]

    def current_styles(self):
        """The style ids of the mazes the actors are in -> uint8 [B, N, N] ([b, y, x]; 0: a free cell or a plain
        wall, k: a wall of wall_styles[k - 1]), of a static or a generated styled config."""
        if self.config is None or not self.config.styled:
            raise ValueError("current_styles: the config has no wall_styles")
        N = self.config.N
        if self.config.generate is None:
            ids = np.stack(self.config.styles)[self.ring.layout.cpu().numpy()]
            return ids.reshape(self.B, N, N)
        words = self.ring.actor_records.cpu().numpy()[:, ops.gen_record_words(N):ops.gen_record_words(N, True)]
        words = words.astype(np.int64) & 0xFFFFFFFF
        nib = (words[:, :, None] >> (4 * np.arange(8))) & 15
        return nib.reshape(self.B, -1)[:, :N * N].astype(np.uint8).reshape(self.B, N, N)

    def stop(self):
        pass


class FirstPersonMazeEnvironment(BatchedMazeEnvironment):
    """B first-person views of a configured maze (MazeConfig(view="first_person")), stepped by the maze.hip kernels:
    actions 0 turn left, 1 turn right, 2 step forward, 3 step back; frames are raycast RGB bytes 0..255.
    With action_set="lab": 0 / 1 look left / right, 2 / 3 strafe left / right, 4 / 5 step forward / back."""
    frame_scale = 1.0 / 255.0          # ring bytes 0..255, read like Lab's obs / 255

    def __init__(self, batch, history_size, device="cuda:0", config=None, actor_base=0, actors_total=None, seed=0,
                 final_obs=False, depth_labels=False, bonus=False):
        if config is None or config.view != "first_person":
            raise ValueError("FirstPersonMazeEnvironment needs a MazeConfig with view='first_person'")
        BatchedMazeEnvironment.__init__(self, batch, history_size, device, config, actor_base, actors_total, seed, final_obs,
                                        depth_labels, bonus)

    def view(self, b0, b1):
        v = BatchedMazeEnvironment.view(self, b0, b1)
        v.__class__ = FirstPersonMazeEnvironment
        return v


def batched_maze_environment(batch, history_size, device="cuda:0", config=None, actor_base=0, actors_total=None, seed=0,
                             final_obs=False, depth_labels=False, bonus=False):
    """The batched maze environment of `config` (None: the reference's map): first-person or top-down, by config.view."""
    cls = FirstPersonMazeEnvironment if config is not None and config.view == "first_person" else BatchedMazeEnvironment
    return cls(batch, history_size, device, config=config, actor_base=actor_base, actors_total=actors_total, seed=seed,
               final_obs=final_obs, depth_labels=depth_labels, bonus=bonus)


class MazeEnvironment(environment.Environment):
    @staticmethod
    def get_action_size():
        return 4

    def __init__(self, device="cuda:0", config=None, seed=0):
        environment.Environment.__init__(self)
        self._env = batched_maze_environment(1, 2, device, config=config, seed=seed)
        self._a = torch.zeros(1, dtype=torch.int32, device=device)
        self._r = torch.zeros(1, dtype=torch.float32, device=device)
        self._t = torch.zeros(1, dtype=torch.int32, device=device)
        self.reset()

    def _image(self):
        ring = self._env.ring
        slot = int(ring.count.cpu()[0]) % ring.H1
        fr = ring.frames[slot * ops.FRAME_BYTES:(slot + 1) * ops.FRAME_BYTES]
        img = fr.cpu().numpy().reshape(84, 84, 3).astype(np.float64)
        # the pixel values (top-down 0 / 1; first person bytes / 255)
        return img if self._env.frame_scale == 1.0 else img / round(1.0 / self._env.frame_scale)

    def _state(self, image):
        """The state dict: 'image' and, for a goal-sense config, 'objective' (float64 [3]: goal ahead / 32, goal to the
        right / 32, path distance / 512) as indoor_environment.py:70-73 hands its measurements over."""
        state = {'image': image}
        ring = self._env.ring
        if ring.objective_size:
            slot = int(ring.count.cpu()[0]) % ring.H1
            state['objective'] = ring.r_objective[3 * slot:3 * slot + 3].cpu().numpy().astype(np.float64)
        return state

    def reset(self):
        self._env.reset()
        self.last_state = self._state(self._image())
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
        self.last_state = self._state(image)
        self.last_action = int(action)
        self.last_reward = reward
        self._last_full_state = {"success": terminal}
        return image, reward, terminal, pc
