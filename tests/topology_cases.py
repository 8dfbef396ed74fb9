"""Hand-built occupancies for the solid-topology tests, each with the answer it must give written out as
literals: pairs of points joined by exactly one neighbour offset across exactly one kind of brick border, a 143-point snake that
fills one 8^3 brick with a single path, checkerboards, buried one-point voids, framed planes and rods.  The literals are checked
against tests/topology_ref.py without a GPU (tests/test_topology_cpu.py) and against the kernels with one
(tests/test_gpu_topology_borders.py).  Occupancies are bool arrays indexed (k, j, i).  Test infrastructure only."""
import itertools

import numpy as np

OFFSETS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]            # (di, dj, dk): all 26
BRICK = 8


def faces_of(d):
    return sum(1 for x in d if x != 0)


def straddles(d):
    """Every subset of d's non-zero axes, as a tuple of axis numbers (0 = i)."""
    axes = [a for a in range(3) if d[a] != 0]
    return [s for r in range(len(axes) + 1) for s in itertools.combinations(axes, r)]


BORDER_CASES = [(d, s) for d in OFFSETS for s in straddles(d)]                             # 6 x 2 + 12 x 4 + 8 x 8 = 124


def pair(d, s, shift=(0, 0, 0)):
    """The points a and a + d, (i, j, k) each.  On the axes in s the pair straddles the brick border 15|16 (a at 15 for +1, at 16
    for -1); on every other axis both points lie inside one brick, at 11 and 11 + d."""
    a = tuple((15 if d[x] > 0 else 16) if x in s else 11 for x in range(3))
    a = tuple(a[x] + shift[x] for x in range(3))
    return a, tuple(a[x] + d[x] for x in range(3))


def crosses_a_border(p, q):
    return any(p[x] // BRICK != q[x] // BRICK for x in range(3))


PACKED_SHAPE = (26, 26, 26)                                                                # nz, ny, nx: points 10 .. 24 are used


def packed_pairs(d):
    """All straddle subsets of offset d in one lattice of PACKED_SHAPE: subset number n at the shift 8 * (bits of n), which keeps
    brick borders brick borders and any two pairs at least 2 points apart on an axis."""
    out = []
    for n, s in enumerate(straddles(d)):
        a, b = pair(d, s, (8 * (n & 1), 8 * ((n >> 1) & 1), 8 * ((n >> 2) & 1)))
        assert crosses_a_border(a, b) == bool(s)
        out.append((a, b))
    return out


THIN_SHAPE = (23, 18, 17)                                                                  # nz, ny, nx: the last brick in x is 1 point thick, in y 2


def thin_pair(d):
    """The pair of offset d that straddles a border on all of d's axes, for the lattice THIN_SHAPE."""
    return pair(d, tuple(a for a in range(3) if d[a] != 0))


def occupancy_of(pairs, shape, inside):
    """inside: the pairs' points are the only inside points.  Otherwise they are the only outside points."""
    occ = np.zeros(shape, dtype=bool) if inside else np.ones(shape, dtype=bool)
    for p in itertools.chain.from_iterable(pairs):
        assert occ[p[2], p[1], p[0]] != inside                                               # no point twice
        occ[p[2], p[1], p[0]] = inside
    return occ


def expected_of_pairs(d, pairs, shape, inside):
    """The counts a lattice of such pairs must give, as far as they are known by construction: 6-adjacency joins an inside pair
    only across a face; 26-adjacency joins every void pair; a void with a point on the lattice's border is exterior."""
    n_points = shape[0] * shape[1] * shape[2]
    if inside:
        bodies = len(pairs) * (1 if faces_of(d) == 1 else 2)
        return {"bodies": bodies, "cavities": 0, "points": 2 * len(pairs), "exterior_points": n_points - 2 * len(pairs),
                "euler": bodies, "tunnels": 0, "cavity_sizes": []}
    on_border = [any(p[x] in (0, shape[2 - x] - 1) for p in ab for x in range(3)) for ab in pairs]
    cavities = on_border.count(False)
    return {"bodies": 1, "cavities": cavities, "points": n_points - 2 * len(pairs), "exterior_points": 2 * on_border.count(True),
            "cavity_sizes": [2] * cavities}


def check_expected(counts, cavity_rows, want):
    """The literal part of a result: counts (a dict) and the first entry of each cavity row against expected_of_pairs."""
    for key, value in want.items():
        if key == "cavity_sizes":
            assert [int(r[0]) for r in cavity_rows] == value
        else:
            assert counts[key] == value, key


# ---- a snake in one brick ---------------------------------------------------------------------------------------------------------
SNAKE_POINTS = 143


def snake():
    """8 x 8 x 8: one path of 143 points.  Even planes hold the even rows, joined at i = 7, 0, 7 (rows 1, 3, 5); the odd planes
    hold one point each, at (i, j) = (0, 6), (0, 0), (0, 6), which joins the end of one plane's path to the next plane's."""
    s = np.zeros((8, 8, 8), dtype=bool)
    for k in range(0, 8, 2):
        s[k, 0::2, :] = True
        s[k, 1, 7] = s[k, 3, 0] = s[k, 5, 7] = True
    s[1, 6, 0] = s[3, 0, 0] = s[5, 6, 0] = True
    assert np.count_nonzero(s) == SNAKE_POINTS
    return s


ORIENTATIONS = list(itertools.product((False, True), repeat=3))                             # mirrored in (k, j, i) or not
SNAKE_WAYS = {"aligned": (1, 0, 1, 0), "across": (1, 0, 1, 0), "complement": (1, 1, 2, 0)}  # (bodies, cavities, euler, tunnels)


def snake_case(way, mirror):
    """24^3 points: the snake at [8, 16)^3 (one brick), at [4, 12)^3 (eight bricks), or its complement at [8, 16)^3 in a full
    lattice (one body around one cavity of 143 points)."""
    s = snake()
    for axis, m in enumerate(mirror):
        if m:
            s = np.flip(s, axis)
    occ = np.zeros((24, 24, 24), dtype=bool)
    lo = 4 if way == "across" else 8
    occ[lo:lo + 8, lo:lo + 8, lo:lo + 8] = s
    return ~occ if way == "complement" else occ


# ---- many components --------------------------------------------------------------------------------------------------------------
def checkerboard(shape, parity=0):
    k, j, i = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return (i + j + k) % 2 == parity


def buried_voids(n=64):
    """A full n^3 lattice with one-point voids at every all-odd coordinate below n - 1: ((n - 2) / 2)^3 cavities."""
    occ = np.ones((n, n, n), dtype=bool)
    occ[1:n - 1:2, 1:n - 1:2, 1:n - 1:2] = False
    return occ


SMALL = (17, 20, 33)                                                                        # nz, ny, nx
FRAMED = {"k": (1, 8, 9, 0), "j": (1, 9, 10, 0), "i": (1, 16, 17, 0)}                       # (bodies, cavities, euler, tunnels)


def framed_planes(axis, shape=SMALL):
    """All six border planes and every second plane along `axis` inside: the voids between are plane-shaped cavities, each
    crossing every brick of its plane."""
    occ = np.zeros(shape, dtype=bool)
    occ[0], occ[-1], occ[:, 0], occ[:, -1], occ[:, :, 0], occ[:, :, -1] = (True,) * 6
    if axis == "k":
        occ[0::2] = True
    elif axis == "j":
        occ[:, 0::2] = True
    else:
        occ[:, :, 0::2] = True
    return occ


def rods(shape=SMALL):
    """Rods along i at every even (j, k): 10 x 9 = 90 bodies of 33 points, each through 5 bricks."""
    occ = np.zeros(shape, dtype=bool)
    occ[0::2, 0::2, :] = True
    return occ
