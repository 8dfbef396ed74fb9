"""The query kernels' LDS columns (rml::QueryLds, csrc/rm_lds_layout.h) at the sizes where the one launch path of the host ABI
changes what it does, bit for bit against the oracle and the numpy restatements.

A 256-thread workgroup takes 1024 bytes per slot: four wave columns of `slots` dwords per lane, behind the kernel's own static
LDS (0, 64 bytes for the traversal march, 4096 for the kernels that work a brick per workgroup).  The distance loop needs
spill_depth + 3 * transform levels slots, the leaf walk (ids) 2 * spill_depth + 3 * transform levels.  Above 64 KiB in all, a
launch has to raise the kernel's limit first; above what the device gives a workgroup (160 KiB on gfx950), the call is refused
with RM_ERR_TOO_LARGE.

What the decoder admits decides which of these can be reached: a value stack of 32 (spill_depth <= 30) under 8 transform
levels.  That is at most 54 slots (55 296 bytes) for the distance loop and 84 slots (86 016 bytes) for the walk:
  - no program reaches 160 KiB, so no call of this family can be refused for its LDS on this device, and rm_sample_grid,
    rm_mass_moments, rm_label_solid and the traversal march (distance loop only) never pass 64 KiB either, with or without
    their own 64 or 4096 bytes: there is no program to build such a case from;
  - the walk does pass 64 KiB: rm_query_points and the attribute pass of rm_trace_rays with ids (no static LDS), and
    rm_extract_mesh_sparse with ids, whose brick kernels run with the walk's columns behind their 4096 bytes.
The towers below -- a right-deep union of n spheres under k nested translations -- are chosen from rm_program_info's facts:
64 slots (65 536 bytes: exactly the limit without static LDS, above it with 4096), 65 slots (the first size above it for every
kernel) and the deepest program there is."""
import functools

import numpy as np
import pytest

import mass_ref as M
import scenes
import topology_ref as TOPO
import trace_ref as TR
from oracle import rm_oracle_np as onp
from ray_marching_amd import renderer
from test_gpu_query import same

pytestmark = pytest.mark.gpu

F = np.float32
LIM = (0.01, 100.0, 64)
KIB = 1024
OWN_BRICK = 4096
# name: (spheres, translations, walk slots)
TOWERS = {"at_64_kib": (22, 8, 64), "above_64_kib": (24, 7, 65), "deepest": (32, 8, 84)}
ORIGIN, STEP = (-3.0, -3.0, -3.0), (F(0.4), F(0.4), F(0.4))


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    r.set_limits(LIM)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def tower(name):
    """(cmd_count, words) of the tower, after checking on the decoder's facts that its columns have the size its name says."""
    from oracle import cbind
    n, k, walk_slots = TOWERS[name]
    t = scenes._Tab()
    prims = [t.sphere((0.15 * (i - (n - 1) / 2.0), 0.1 * (i % 3), 0.05 * (i % 2)), 0.5) for i in range(n)]
    root = prims[-1]
    for i in range(n - 2, -1, -1):
        root = t.op(scenes.UNION, prims[i], root)
    root = t.material(root, 1)
    for i in range(k):
        root = t.translation(root, (0.05 * (i + 1), -0.03, 0.02))
    cc, w = cbind.serialize(t.nodes, root)
    w = np.asarray(w, dtype=np.uint32)
    info = renderer.program_info(cc, w)
    assert info["is_chain"] == 0 and info["has_xforms"] == (1 if k else 0) and info["spill_depth"] == n - 2
    distance_slots, walk = info["spill_depth"] + 3 * k, 2 * info["spill_depth"] + 3 * k     # the general loop
    assert walk == walk_slots and distance_slots * KIB + OWN_BRICK <= 64 * KIB
    return int(cc), w


def test_the_towers_sit_on_either_side_of_the_launch_limit_and_at_the_decoder_s_limit(oracle):
    assert TOWERS["at_64_kib"][2] * KIB == 64 * KIB < TOWERS["at_64_kib"][2] * KIB + OWN_BRICK
    assert TOWERS["above_64_kib"][2] * KIB == 65 * KIB
    for name in TOWERS:
        tower(name)
    # one sphere more, or one translation more, and the decoder refuses the deepest tower
    n, k, _ = TOWERS["deepest"]
    t = scenes._Tab()
    prims = [t.sphere((0.1 * i, 0.0, 0.0), 0.5) for i in range(n + 1)]
    root = prims[-1]
    for i in range(n - 1, -1, -1):
        root = t.op(scenes.UNION, prims[i], root)
    assert renderer.validate_program(*oracle.serialize(t.nodes, root))[0] != 0
    t = scenes._Tab()
    root = t.sphere((0.0, 0.0, 0.0), 0.5)
    for i in range(k + 1):
        root = t.translation(root, (0.1, 0.0, 0.0))
    assert renderer.validate_program(*oracle.serialize(t.nodes, root))[0] != 0


@pytest.mark.parametrize("name", sorted(TOWERS))
def test_points_and_grid(res, name):
    """No static LDS: rm_query_points with the walk's columns, rm_sample_grid with the distance loop's."""
    cc, w = tower(name)
    res.set_program(cc, w)
    p = np.random.default_rng(1).uniform(-3, 3, (64, 3)).astype(F)
    q = res.query_points(p, normals=True)
    d, m = onp.map_scene(cc, w, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
    nx, ny, nz = TR.normals_at(cc, w, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2])
    assert same(q["distance"], d) and same(q["material"], m) and same(q["normal"], np.stack([nx, ny, nz], axis=1))
    assert set(int(x) for x in q["material"]) == {1} and len(set(int(x) for x in q["leaf"])) > 4
    g = res.sample_grid(ORIGIN, STEP, (8, 8, 8))
    k, j, i = np.meshgrid(*[np.arange(8, dtype=F)] * 3, indexing="ij")
    x, y, z = [F(ORIGIN[a]) + c.ravel() * STEP[a] for a, c in enumerate((i, j, k))]
    assert same(g.ravel(), onp.map_scene(cc, w, F(LIM[1]), x, y, z))


@pytest.mark.parametrize("name", sorted(TOWERS))
def test_trace_rays(res, name):
    """64 bytes of static LDS in the march (the distance loop's columns); the attribute pass with the walk's columns."""
    cc, w = tower(name)
    res.set_program(cc, w)
    rays = TR.standard_rays(64, seed=3)
    prm = TR.params(t_max=8.0, max_steps=64)
    got = res.trace_rays(rays, max_events=4, normals=True, ids=True, **dict(zip(TR.NAMES, [float(v) for v in prm])))
    want = TR.trace(cc, w, LIM[1], rays, prm, 4, normals=True, ids=True)
    for key in TR.KEYS:
        assert same(np.asarray(got[key]), want[key]), key
    assert int(got["stored"].sum()) > 16


@pytest.mark.parametrize("name", sorted(TOWERS))
def test_brick_kernels(res, name):
    """4096 bytes of static LDS: rm_mass_moments and rm_label_solid with the distance loop's columns, rm_extract_mesh_sparse
    with the walk's (ids) -- the same mesh as rm_extract_mesh, bit for bit."""
    cc, w = tower(name)
    res.set_program(cc, w)
    shape = (16, 16, 16)
    mass = res.mass_moments(ORIGIN, STEP, shape, 0.0)
    assert [int(x) for x in mass.moments] == M.lattice_moments(cc, w, ORIGIN, STEP, shape, 0.0, LIM[1]) and mass.moments[0] > 0
    topo = res.label_solid_grid(ORIGIN, STEP, shape, 0.0)
    want = TOPO.solid(cc, w, ORIGIN, STEP, shape, 0.0, LIM[1])
    assert topo.counts == want["counts"] and np.array_equal(topo.labels(), want["labels"]) and topo.counts["bodies"] == 1
    sparse = res.extract_mesh_grid_sparse(ORIGIN, STEP, shape, 0.0, True, True)
    dense = res.extract_mesh_grid(ORIGIN, STEP, shape, 0.0, True, True)
    assert len(sparse.vertices) > 64 and sparse.stats["bricks_kept"] > 0
    for a, b in ((sparse.vertices, dense.vertices), (sparse.triangles, dense.triangles), (sparse.normals, dense.normals),
                 (sparse.leaf, dense.leaf), (sparse.material, dense.material)):
        assert same(a, b)


def test_the_context_goes_on_with_a_shallow_program(res, oracle):
    """After the deepest program, g1 through rm_query_points: the launch state is the call's, nothing of it stays behind."""
    res.set_program(*tower("deepest"))
    p = np.random.default_rng(2).uniform(-2, 2, (64, 3)).astype(F)
    res.query_points(p)
    cc, w = oracle.serialize(*scenes.g1())
    res.set_program(cc, w)
    q = res.query_points(p)
    assert same(q["distance"], onp.map_scene(cc, w, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2]))
