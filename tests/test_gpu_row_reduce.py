"""The row reductions (csrc/rm_reduce.h) at the fold's boundary, through the public calls: rm_rows_fold_kernel combines 256 rows
per workgroup, and the lattices of the other GPU tests give at most 125 (topology), 32 (distance) and 2 (voxelisation) rows.  Here
each analysis runs with exactly 256 rows -- one full folded row -- and with a few more, so that a second workgroup folds a short
tail.  Expected values are the numpy restatements' (topology_ref, distance_ref, voxel_ref), compared with ==; the literals are
what those restatements give at these shapes."""
import functools

import numpy as np
import pytest

import distance_ref as DR
import topology_ref as TR
import voxel_ref as VR
from test_gpu_topology import same as same_topology
from test_gpu_distance import same as same_distance
from test_gpu_voxelize import UNIT, check as check_voxels
from ray_marching_amd import renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)      # no program: every call here takes an occupancy or a mesh
    yield r
    r.close()


# ---- topology: a row per brick of 8 x 8 x 8 points --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def topology_case(shape):
    """A box with a cavity (the slices clip it to the lattice) and its restatement."""
    occ = np.zeros(shape, dtype=np.uint8)
    occ[2:31, 2:62, 2:62] = 1
    occ[10:14, 10:14, 10:14] = 0
    return occ, TR.topology(occ != 0)


@pytest.mark.parametrize("shape, bricks, exterior", [((32, 64, 64), 256, 26672), ((33, 64, 64), 320, 30768)])
def test_topology_rows_fill_and_pass_one_folded_row(res, shape, bricks, exterior):
    """256 bricks: one full folded row.  320: a second one, and the last layer of bricks is one point thick."""
    nz, ny, nx = shape
    assert -(-nz // 8) * -(-ny // 8) * -(-nx // 8) == bricks
    occ, want = topology_case(shape)
    assert want["counts"] == dict(bodies=1, cavities=1, points=104336, edges=305880, faces=298889, cells=97343, euler=2, tunnels=0,
                                  exterior_points=exterior)
    got = res.label_occupancy(occ)
    same_topology(got, want, "box with a cavity %s" % (shape,))       # the nine counts, both moment tables, the labels


# ---- distance: a row per 2048 points ------------------------------------------------------------------------------------------------
# (2, 513, 512) alone: 257 rows, the last of 1024 points.  The restatement takes about five seconds per occupancy of this size, so
# the shape of exactly 256 rows, (2, 512, 512), is left to the other two analyses.
DIST_SHAPE = (2, 513, 512)
DIST_BLOBS = {"two blobs": ((slice(None), slice(3, 10), slice(3, 10)), (slice(None), slice(505, 512), slice(3, 10))),
              "the second blob": ((slice(None), slice(505, 512), slice(3, 10)),),
              "a blob in the last row": ((slice(1, 2), slice(511, 513), slice(3, 10)),)}
DIST_COUNTS = {"two blobs": dict(points=196, max_inside=1, argmax_inside=1539, max_outside=313508, argmax_outside=132095),
               "the second blob": dict(points=98, max_inside=1, argmax_inside=258563, max_outside=507029, argmax_outside=511),
               "a blob in the last row": None}


@functools.lru_cache(maxsize=None)
def distance_case(name):
    occ = np.zeros(DIST_SHAPE, dtype=np.uint8)
    for blob in DIST_BLOBS[name]:
        occ[blob] = 1
    return occ, DR.separable(occ)


@pytest.mark.parametrize("name", list(DIST_BLOBS))
def test_distance_rows_pass_one_folded_row(res, name):
    """Two equal blobs: every inside point has D2 = 1, the first blob lies in row 0 and the second one's last points in row 256, so
    equal maxima meet only after the fold and the smaller index must win; the count of inside points needs both folded rows.  The
    second blob alone.  A blob that lies in row 256 alone: count and inside argmax come out of the second folded row."""
    nz, ny, nx = DIST_SHAPE
    assert -(-nz * ny * nx // 2048) == 257 and nz * ny * nx - 256 * 2048 == 1024
    occ, want = distance_case(name)
    counts = DR.counts(want)
    if DIST_COUNTS[name] is not None:
        assert counts == DIST_COUNTS[name]
    else:
        assert counts["points"] == 14 and counts["argmax_inside"] == 3 + nx * (511 + ny) >= 256 * 2048
    dist = res.distance_occupancy(occ)
    same_distance(dist, want, name)                                   # the five counts and the volume
    feats = dist.features(0, None)                                    # rm_dist_compose_kernel's rows, through the same path
    _, want_counts = DR.features(occ, 0, None, volume=want)
    print("features:", feats.counts)
    assert feats.counts == want_counts and feats.counts["core"] == counts["points"] and feats.counts["thin"] == 0


# ---- voxelisation: a row per 4096 cells ---------------------------------------------------------------------------------------------
# The lattices (nx, ny, nz).  With 64 or 65 points along x the box reaches past the lattice: its far crossings clamp to bit nx, and
# without its last face (x = 3.3) every row it crosses is open and no point inside.  With 128 points along x the whole box lies in
# the lattice.  (inside, open rows) of the closed box and of the open one.
VOX_CASES = [((64, 128, 128), 256, (60 * 6435, 0), (0, 6435)), ((65, 128, 128), 260, (392535, 0), (0, 6435)),
             ((128, 128, 64), 256, (752895, 0), (45045, 6435)), ((128, 128, 65), 260, (752895, 0), (45045, 6435))]


@functools.lru_cache(maxsize=None)
def voxel_mesh(closed):
    v, t = VR.box((3.3, 4.2, 5.1), (120.7, 121.6, 60.4))
    return v, (t if closed else t[:-2])


@pytest.mark.parametrize("closed", [True, False], ids=["closed box", "open box"])
@pytest.mark.parametrize("shape, rows, closed_counts, open_counts", VOX_CASES)
def test_voxel_rows_fill_and_pass_one_folded_row(res, shape, rows, closed_counts, open_counts, closed):
    nx, ny, nz = shape
    assert -(-nx * ny * nz // 4096) == rows
    v, t = voxel_mesh(closed)
    got = check_voxels(res, v, t, *UNIT, shape, "%s box %s" % ("closed" if closed else "open", shape))   # six counts, the bytes
    assert (got.counts["inside"], got.counts["open_rows"]) == (closed_counts if closed else open_counts)
