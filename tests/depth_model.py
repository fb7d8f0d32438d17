"""Host model of the depth labels of first-person mazes.  TEST INFRASTRUCTURE ONLY.

Built on fp_maze_model.cast, the host restatement of the camera: position j of 12 is frame column i = 7 j + 3, the centre
of a 7-column band; its ray ends at t = tn / td at the first wall cell or map border (a border is a depth like any other);
the class is the number of edges e in EDGES with t >= e, decided in integers as 2 tn >= 2 e td, so a ray that ends exactly
on an edge is in the upper class.  Pickups, the goal and wall styles do not enter.
"""
import numpy as np

try:
    import fp_maze_model as FP
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP

POSITIONS, CLASSES = 12, 8
EDGES = (1, 2, 3, 4, 6, 8, 12)


def column(j):
    """Frame column of position j."""
    return 7 * j + 3


def depth_class(tn, td):
    return sum(1 for e in EDGES if 2 * tn >= 2 * e * td)


def on_edge(tn, td):
    return any(tn == e * td for e in EDGES)


def rays(walls, N, x, y, h):
    """[(tn, td)] of the 12 positions seen from cell (x, y) along heading h over `walls` (bool [N * N], cell y * N + x)."""
    return [FP.cast(walls, N, x, y, h, column(j))[:2] for j in range(POSITIONS)]


def labels(walls, N, x, y, h):
    """-> uint8 [12]: the depth classes of the view from cell (x, y) along heading h."""
    return np.array([depth_class(tn, td) for tn, td in rays(walls, N, x, y, h)], dtype=np.uint8)


def room_census(N):
    """Every cell and heading of an empty N x N room -> (class counts [8], rays exactly on an edge, largest tn or td)."""
    walls = np.zeros(N * N, dtype=bool)
    counts = np.zeros(CLASSES, dtype=np.int64)
    edge = big = 0
    for y in range(N):
        for x in range(N):
            for h in range(4):
                for tn, td in rays(walls, N, x, y, h):
                    counts[depth_class(tn, td)] += 1
                    edge += on_edge(tn, td)
                    big = max(big, tn, td)
    return counts, edge, big
