"""Host model of styled first-person walls and landmarks (numpy, integer arithmetic).  TEST INFRASTRUCTURE ONLY.

Restates DESIGN §7h independently of maze.hip, on top of the §7e / §7f / §7g host models (fp_maze_model.py,
nav_maze_model.py, gen_maze_model.py), whose frames it repaints:

  ray      column i's ray is §7e's.  Only its colour changes, and only when the first blocked cell is an interior wall
           cell of style k >= 1; the map border and style 0 keep their bytes
  texel    u in 0..7, the eighth of the face that was hit, in world coordinates.  With d = (dx, dy) forward, r = (rx, ry)
           right, q = 2i + 1 - W, aq = |q|:
             forward crossing k (t = (2k+1)/2):       sigma = rx + ry, n = sigma q (2k+1) + W,   den = 2W
             side crossing m (t = (2m+1) W / 2 aq):   sigma = dx + dy, n = sigma (2m+1) W + aq,  den = 2 aq
           u = ((n mod den) * 8) div den, mod the non-negative remainder
  colour   style k = (r, g, b, pattern): each channel c -> c >> 1 if bit u of pattern is set, then (5 c) >> 3 on a face
           crossed along y (the faces whose plain shade is 160)
  landmarks (generated mazes) after the walls of episode (seed, g, episode) are known: cell c gets w = word c & 3 of
           Philox4x32-10(key = seed, counter = (g, episode, STYLE_STREAM, c >> 2)); a wall cell with (w >> 24) < density
           has style 1 + (w & 0xFFFFFF) mod S, every other cell style 0.  A respawn redraws nothing.
"""
import numpy as np

try:
    import fp_maze_model as FP
    import nav_maze_model as NAV
    import gen_maze_model as GM
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import nav_maze_model as NAV
    from tests import gen_maze_model as GM
    from tests.maze_model import philox4x32_10

H, W, DIRS = FP.H, FP.W, FP.DIRS
STYLE_STREAM = 0x4D415A53
STYLE_HEADER, STYLE_SLOTS = 8, 8


def style_words(N):
    return (N * N + 7) // 8


def texel(h, i, forward, index):
    """u of column i's hit at forward crossing `index` (forward=True) or side crossing `index`, heading h."""
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    q = 2 * i + 1 - W
    aq = abs(q)
    if forward:
        n, den = (rx + ry) * q * (2 * index + 1) + W, 2 * W
    else:
        n, den = (dx + dy) * (2 * index + 1) * W + aq, 2 * aq
    return ((n % den) * 8) // den           # (Python's % of a positive modulus is the non-negative remainder)


def cast(walls, N, ex, ey, h, i):
    """Column i's ray from cell (ex, ey) along h -> (tn, td, hit cell or -1 for the border, xface, forward, index): §7e's
    walk, which also tells which crossing hit."""
    dx, dy = DIRS[h]
    rx, ry = DIRS[(h + 1) % 4]
    q = 2 * i + 1 - W
    aq, sg = abs(q), (1 if q > 0 else -1)
    f = s = k = m = 0
    while True:
        if (2 * k + 1) * aq < (2 * m + 1) * W:
            f += 1
            tn, td, xface, forward, index = 2 * k + 1, 2, dx != 0, True, k
            k += 1
        else:
            s += sg
            tn, td, xface, forward, index = (2 * m + 1) * W, 2 * aq, rx != 0, False, m
            m += 1
        cx, cy = ex + f * dx + s * rx, ey + f * dy + s * ry
        if not (0 <= cx < N and 0 <= cy < N):
            return tn, td, -1, xface, forward, index
        if walls[cy * N + cx]:
            return tn, td, cy * N + cx, xface, forward, index


def colour(style, u, xface):
    """The three bytes a style (r, g, b, pattern) leaves at texel u of a face."""
    out = []
    for c in style[:3]:
        if (style[3] >> u) & 1:
            c >>= 1
        if not xface:
            c = (5 * c) >> 3
        out.append(c)
    return out


_CACHE = {}


def repaint(img, walls, ids, wall_styles, N, x, y, h, key=None):
    """`img` (a frame of the unstyled models) with the wall pixels of every column that hits a styled cell repainted."""
    hit = _CACHE.get(key) if key is not None else None
    if hit is not None and hit[0] is img:
        return hit[1]
    out = None
    p = np.abs(2 * np.arange(H, dtype=np.int64) + 1 - H)
    for i in range(W):
        tn, td, cell, xface, forward, index = cast(walls, N, x, y, h, i)
        if cell < 0 or not ids[cell]:
            continue
        if out is None:
            out = img.copy()
        rows = p * tn < H * td
        out[rows, i] = colour(wall_styles[int(ids[cell]) - 1], texel(h, i, forward, index), xface)
    if out is None:
        out = img
    else:
        out.setflags(write=False)
    if key is not None:
        if len(_CACHE) > 20000:
            _CACHE.clear()
        _CACHE[key] = (img, out)
    return out


def landmark_ids(N, walls, n_styles, density, seed, g, episode):
    """uint8 [N * N] style ids of a generated maze with the wall cells `walls`."""
    seed = int(seed) & (2 ** 64 - 1)
    ids = np.zeros(N * N, dtype=np.uint8)
    for blk in range((N * N + 3) // 4):
        u = philox4x32_10((g, episode, STYLE_STREAM, blk), (seed & 0xFFFFFFFF, seed >> 32))
        for e in range(4):
            c = 4 * blk + e
            w = int(u[e])
            if c < N * N and walls[c] and (w >> 24) < density:
                ids[c] = 1 + (w & 0xFFFFFF) % n_styles
    return ids


def nibble_words(N, ids):
    """The 4-bit style ids as the device keeps them: cell c in nibble c & 7 of word c >> 3 -> int32 [style_words(N)]."""
    sw = style_words(N)
    nib = np.zeros(8 * sw, dtype=np.int64)
    nib[:N * N] = ids
    words = np.array([sum(int(v) << (4 * j) for j, v in enumerate(row)) for row in nib.reshape(sw, 8)], dtype=np.int64)
    return (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def layout_string(walls, apple_cells, ids):
    s = np.where(walls, "+", "-")
    s[list(apple_cells)] = "A"
    for c in np.flatnonzero(ids):
        s[c] = str(int(ids[c]))
    return "".join(s)


def style_section(wall_styles, density, N, layout_ids):
    """The words a styled block ends in: header, style words, the nibble words of every static layout."""
    sec = [len(wall_styles), density, 0, 0, 0, 0, 0, 0]
    sec += [r | g << 8 | b << 16 | pat << 24 for r, g, b, pat in wall_styles] + [0] * (STYLE_SLOTS - len(wall_styles))
    words = np.array(sec, dtype=np.int64)
    words = (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return np.concatenate([words] + [nibble_words(N, ids) for ids in layout_ids])


class _Styled(object):
    """Mixin over a §7e / §7f / §7g actor: the frames of its _render, repainted."""

    def _styles(self):
        return self.config.styles[self.layout]

    def _render(self):
        img = super(_Styled, self)._render()
        conf = self.config
        key = (id(img), self.x, self.y, self.h)
        return repaint(img, conf.walls[self.layout], self._styles(), conf.wall_styles, conf.N, self.x, self.y, self.h, key)

    def style_ids(self):
        return np.asarray(self._styles(), dtype=np.uint8)


class HostStyledMaze(_Styled, FP.HostFirstPersonMaze):
    pass


class HostStyledNavMaze(_Styled, NAV.HostNavMaze):
    pass


class _StyledGen(_Styled):
    def _regenerate(self):
        super(_StyledGen, self)._regenerate()
        base = self.config.base
        self.config.styles = [landmark_ids(base.N, self.config.walls[0], len(base.wall_styles), base.gen_landmark_density,
                                           self.seed, self.g, self.episode + 1)]

    def actor_record(self):
        """The per-actor record of a styled generated block: §7g's, then the nibble words."""
        return np.concatenate([super(_StyledGen, self).actor_record(), nibble_words(self.config.N, self._styles())])


class HostStyledGenMaze(_StyledGen, GM.HostGenMaze):
    pass


class HostStyledGenNavMaze(_StyledGen, GM.HostGenNavMaze):
    pass


def host_batch(config, B, actor_base=0, actors_total=None, seed=0):
    """Host models of the global actors [actor_base, actor_base + B) of a styled config."""
    total = B if actors_total is None else actors_total
    if config.generate is not None:
        cls = HostStyledGenNavMaze if config.nav else HostStyledGenMaze
    else:
        cls = HostStyledNavMaze if config.nav else HostStyledMaze
    return [cls(config, actor_base + b, total, seed) for b in range(B)]
