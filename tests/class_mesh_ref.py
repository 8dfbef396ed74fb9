"""A numpy restatement of the lattice-meshing contract, for the tests: mesh(data, set_a, set_b, origin,
step) gives the five arrays and all counts of rm_mesh_classes.  Faces are found on three shifted views of the padded lattice, laid
out over the corner lattice so that a C-order flatten is the key order; vertices by a cumulative sum over the touched corners;
edges by a bincount of the four edges of every face.  Written from the contract, not from the kernel.  Test infrastructure only."""
import numpy as np

NO_ID = 0xFFFFFFFF
COUNT_NAMES = ("vertices", "triangles", "faces", "faces_pos_x", "faces_neg_x", "faces_pos_y", "faces_neg_y", "faces_pos_z",
               "faces_neg_z", "edges", "open_edges", "branch_edges")


def class_mask(classes):
    mask = 0
    for a in ([classes] if isinstance(classes, (int, np.integer)) else classes):
        assert 0 <= int(a) < 8
        mask |= 1 << int(a)
    return mask


def complement(classes):
    return [c for c in range(8) if not (class_mask(classes) >> c) & 1]


def classes_of(data):
    """min(byte, 7) of an array of a one-byte type, indexed [k, j, i]."""
    return np.minimum(np.ascontiguousarray(data).view(np.uint8), 7)


def mesh(data, set_a, set_b=None, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
    """rm_mesh_classes + rm_read_class_mesh for `data` (nz, ny, nx) of a one-byte type: a dict with vertices (V, 3) float32,
    triangles (T, 3) uint32, ids (T, 2) uint32 and counts (a dict: COUNT_NAMES)."""
    set_b = complement(set_a) if set_b is None else set_b
    mask_a, mask_b = class_mask(set_a), class_mask(set_b)
    assert mask_a and mask_b and not mask_a & mask_b
    c = classes_of(data)
    nz, ny, nx = c.shape
    cx, cy, cz = nx + 1, ny + 1, nz + 1
    p = np.pad(c, 1, constant_values=0).astype(np.int64)           # point (i, j, k) at [k + 1, j + 1, i + 1]
    in_a, in_b = ((mask_a >> p) & 1).astype(bool), ((mask_b >> p) & 1).astype(bool)
    hi = (slice(1, cz + 1), slice(1, cy + 1), slice(1, cx + 1))    # over the corner lattice: the point (ci, cj, ck) ...
    exists = np.zeros((cz, cy, cx, 3), dtype=bool)
    positive = np.zeros((cz, cy, cx, 3), dtype=bool)
    for a in range(3):                                             # ... and the point one lower along a
        lo = list(hi)
        lo[2 - a] = slice(0, (cx, cy, cz)[a])
        lo = tuple(lo)
        pos, neg = in_a[lo] & in_b[hi], in_b[lo] & in_a[hi]
        exists[..., a], positive[..., a] = pos | neg, pos
    keys = np.flatnonzero(exists.reshape(-1))                      # ascending 3 L + a
    L, axis = keys // 3, keys % 3
    pos = positive.reshape(-1)[keys]
    corner = np.stack([L % cx, (L // cx) % cy, L // (cx * cy)], axis=1)      # (F, 3): ci, cj, ck
    unit = np.eye(3, dtype=np.int64)
    eu, ev = unit[(axis + 1) % 3], unit[(axis + 2) % 3]
    lin = lambda q: q[:, 0] + cx * (q[:, 1] + cy * q[:, 2])  # noqa: E731
    q00, q10, q11, q01 = lin(corner), lin(corner + eu), lin(corner + eu + ev), lin(corner + ev)
    n_corners = cx * cy * cz
    used = np.zeros(n_corners, dtype=bool)
    for q in (q00, q10, q11, q01):
        used[q] = True
    rank = np.cumsum(used) - 1
    Lv = np.flatnonzero(used)
    cv = np.stack([Lv % cx, (Lv // cx) % cy, Lv // (cx * cy)], axis=1).astype(np.float32)
    o, s = np.asarray(origin, dtype=np.float32), np.asarray(step, dtype=np.float32)
    vertices = (o[None, :] + ((cv - np.float32(0.5)) * s[None, :]).astype(np.float32)).astype(np.float32)
    r00, r10, r11, r01 = rank[q00], rank[q10], rank[q11], rank[q01]
    first = np.where(pos[:, None], np.stack([r00, r10, r11], axis=1), np.stack([r00, r11, r10], axis=1))
    second = np.where(pos[:, None], np.stack([r00, r11, r01], axis=1), np.stack([r00, r01, r11], axis=1))
    triangles = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.uint32)
    # ids: the A side is the lower point of a positive face, the higher (the corner's own) of a negative one
    high, low = corner, corner - unit[axis]
    side_a, side_b = np.where(pos[:, None], low, high), np.where(pos[:, None], high, low)
    cls = lambda q: p[q[:, 2] + 1, q[:, 1] + 1, q[:, 0] + 1]  # noqa: E731
    word0 = cls(side_a) | cls(side_b) << 8 | (2 * axis + pos) << 16
    inside = np.all((side_a >= 0) & (side_a < np.array([nx, ny, nz])), axis=1)
    word1 = np.where(inside, side_a[:, 0] + nx * (side_a[:, 1] + ny * side_a[:, 2]), NO_ID)
    ids = np.repeat(np.stack([word0, word1], axis=1), 2, axis=0).astype(np.uint32)
    # edges: (lower corner, direction) of the four edges of every face
    u, v = (axis + 1) % 3, (axis + 2) % 3
    edge_keys = np.concatenate([3 * q00 + u, 3 * q00 + v, 3 * q01 + u, 3 * q10 + v])
    per_edge = np.bincount(edge_keys, minlength=1)
    F = len(keys)
    counts = {"vertices": int(used.sum()), "triangles": 2 * F, "faces": F, "edges": int((per_edge >= 1).sum()),
              "open_edges": int(((per_edge == 1) | (per_edge == 3)).sum()), "branch_edges": int((per_edge >= 3).sum())}
    for a, name in enumerate("xyz"):
        counts["faces_pos_" + name] = int((pos & (axis == a)).sum())
        counts["faces_neg_" + name] = int((~pos & (axis == a)).sum())
    return {"vertices": vertices, "triangles": triangles, "ids": ids, "counts": counts}


def checkerboard(shape):
    """uint8 (nz, ny, nx) for a shape (nx, ny, nz): class 1 where i + j + k is even."""
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return ((i + j + k) % 2 == 0).astype(np.uint8)


def torus(R, r, margin=2):
    """The occupancy (uint8) of a torus around z: major radius R, minor radius r, in index units around the lattice's middle."""
    n, nz = 2 * (int(np.ceil(R + r)) + margin) + 1, 2 * (int(np.ceil(r)) + margin) + 1
    k, j, i = np.meshgrid(np.arange(nz), np.arange(n), np.arange(n), indexing="ij")
    x, y, z = i - (n - 1) / 2.0, j - (n - 1) / 2.0, k - (nz - 1) / 2.0
    return (((np.sqrt(x * x + y * y) - R) ** 2 + z * z) < r * r).astype(np.uint8)
