"""Solid topology on the GPU (rm_label_solid, rm_label_occupancy, rm_read_topology): all nine counts, both
row tables and the whole label volume against the numpy restatement (tests/topology_ref.py) with ==; the brick statistics and
the summed body rows against rm_mass_moments on the same lattice; known topologies as literals; a body that winds through many
bricks; partial bricks; random occupancies around the percolation threshold; one lattice above 2^24 points with closed-form
answers; errors and isolation."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import mass_ref as M
import scenes
import test_sparse_mesh_cpu as T
import topology_ref as TR
from ray_marching_amd import _ffi, csg, renderer

pytestmark = pytest.mark.gpu

F = np.float32
LIM = (0.01, 100.0, 256)
BRICK_STATS = ("bricks", "bricks_kept", "bricks_inside", "evaluations")
SCENES_40 = ("g1", "g8", "g32", "g32_balanced", "g32s", "ext_mix", "xform_mix", "mat_mix")


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def box_lattice(shape, lo=-2.5, hi=2.5):
    """origin, step, shape of `shape` points over [lo, hi]^3 (label_solid's lattice)."""
    shape = (shape,) * 3 if isinstance(shape, int) else tuple(shape)
    lo_, step, n = renderer.RayMarchingResources._box_lattice(lo, hi, shape)
    return tuple(float(x) for x in lo_), tuple(F(x) for x in step), shape


def use(res, cc, w, limits=LIM):
    res.set_limits(limits)
    res.set_program(cc, w)


def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


def program(node):
    cc, w = csg.serialize(node)
    return int(cc), np.asarray(w, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def scene_program(name):
    from oracle import cbind
    cc, w = cbind.serialize(*T.ALL_SCENES[name]())
    return int(cc), np.asarray(w, dtype=np.uint32)


def summary(t):
    return t.bodies, t.cavities, t.euler, t.tunnels


def same(got, want, what=""):
    """Everything a Topology carries == the restatement's."""
    print("%s: counts %s; stats %s" % (what, got.counts, got.stats))
    assert got.counts == want["counts"], what
    assert got.body_moments.dtype == np.uint64 and got.body_moments.shape == (want["counts"]["bodies"], 16)
    assert got.cavity_moments.dtype == np.uint64 and got.cavity_moments.shape == (want["counts"]["cavities"], 16)
    assert [[int(x) for x in row] for row in got.body_moments] == want["body_rows"], what
    assert [[int(x) for x in row] for row in got.cavity_moments] == want["cavity_rows"], what
    lab = got.labels()
    assert lab.dtype == np.uint32 and lab.shape == want["labels"].shape
    assert np.array_equal(lab, want["labels"]), what
    assert got.stats["merge_passes"] == 1 and got.stats["scratch_bytes"] > 0   # a second pass would mean that a union was lost


def check_solid(res, cc, w, origin, step, shape, level=0.0, max_dist=LIM[1], what=""):
    """label_solid_grid == the restatement; its brick statistics and summed body rows == rm_mass_moments'."""
    got = res.label_solid_grid(origin, step, shape, level)
    same(got, TR.solid(cc, w, origin, step, shape, level, max_dist), "%s %s level %g" % (what, shape, level))
    mass = res.mass_moments(origin, step, shape, level)
    assert {k: got.stats[k] for k in BRICK_STATS} == {k: mass.stats[k] for k in BRICK_STATS}, what
    assert TR.combine_rows([[int(x) for x in row] for row in got.body_moments]) == [int(x) for x in mass.moments], what
    assert got.counts["points"] == int(mass.moments[0])
    return got


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES_40)
def test_named_scenes(res, name):
    cc, w = scene_program(name)
    use(res, cc, w)
    got = check_solid(res, cc, w, *box_lattice(40), what=name)
    assert got.bodies >= 1
    if name == "g32":
        assert got.bodies == 13
        fused = check_solid(res, cc, w, *box_lattice(40), level=0.1, what=name)
        assert fused.bodies == 9


# ---- known topology ---------------------------------------------------------------------------------------------------------------
def hollow_sphere():
    return program(csg.Subtraction(csg.Sphere((0.0, 0.0, 0.0), 1.8), csg.Sphere((0.1, 0.0, 0.0), 1.0)))


def box_ring():
    return program(csg.Subtraction(csg.Box((0.0, 0.0, 0.0), (1.5, 0.5, 1.5)), csg.Box((0.0, 0.0, 0.0), (0.7, 1.0, 0.7))))


@pytest.mark.parametrize("shape", [(40, 40, 40), (33, 20, 17)])
def test_hollow_sphere_has_one_cavity(res, shape):
    cc, w = hollow_sphere()
    use(res, cc, w)
    got = check_solid(res, cc, w, *box_lattice(shape), what="hollow sphere")
    assert summary(got) == (1, 1, 2, 0)
    assert got.cavity_moments[0][0] > 0
    props = got.body_properties(density=2.0)
    assert len(props) == 1 and props[0]["mass"] == pytest.approx(2.0 * props[0]["volume"])


def test_box_ring_has_one_tunnel(res):
    cc, w = box_ring()
    use(res, cc, w)
    got = check_solid(res, cc, w, *box_lattice(40), what="ring")
    assert summary(got) == (1, 0, 0, 1)


# ---- a component that winds through many bricks -----------------------------------------------------------------------------------
def serpentine():
    node = csg.Box((0.0, 0.0, 0.0), (2.2, 0.3, 2.2))
    for i in range(9):
        node = csg.Subtraction(node, csg.Box((-1.8 + 0.45 * i, 0.0, 0.5 if i % 2 == 0 else -0.5), (0.08, 1.0, 2.0)))
    return program(node)


def test_serpentine_is_one_body(res):
    """One body that crosses brick faces dozens of times: a lost union or a find that stops short splits it."""
    cc, w = serpentine()
    use(res, cc, w)
    got = check_solid(res, cc, w, *box_lattice((72, 9, 72)), what="serpentine")
    print("serpentine: merge_passes = %d" % got.stats["merge_passes"])
    assert (got.bodies, got.euler) == (1, 1)


# ---- partial bricks and tiny lattices -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 2), (9, 17, 10), (8, 8, 8), (16, 8, 8)])
def test_partial_bricks_and_tiny_lattices(res, shape):
    cc, w = scene_program("g8")
    use(res, cc, w)
    check_solid(res, cc, w, *box_lattice(shape, -1.5, 1.5), what="g8")
    cc, w = hollow_sphere()
    use(res, cc, w)
    check_solid(res, cc, w, *box_lattice(shape, -1.9, 1.9), what="hollow sphere")


# ---- random occupancies ---------------------------------------------------------------------------------------------------------
RANDOM_SUMMARIES = {0.2: (1017, 0, 1015, 2), 0.3116: (673, 0, 638, 35), 0.5: (156, 0, -536, 692), 0.9: (1, 93, 5, 89)}


DENSITIES = (0.2, 0.3116, 0.5, 0.9)                                          # 0.3116: near the site-percolation threshold


@functools.lru_cache(maxsize=None)
def random_occupancies(seed):
    """One occupancy per density, drawn one after the other from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    return {d: rng.random((17, 20, 33)) < d for d in DENSITIES}


def random_occupancy(seed, density):
    return random_occupancies(seed)[density]


@functools.lru_cache(maxsize=None)
def random_reference(seed, density):
    return TR.topology(random_occupancy(seed, density))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("seed,density", [(s, d) for s in (5, 6) for d in DENSITIES])
def test_random_occupancies(res, seed, density, device):
    occ = random_occupancy(seed, density)
    want = random_reference(seed, density)
    if device:
        import torch
        arg = torch.from_numpy(occ.astype(np.uint8) * 255).to("cuda:0")       # any nonzero byte is inside
    else:
        arg = occ
    got = res.label_occupancy(arg)
    same(got, want, "random %g seed %d %s" % (density, seed, "device" if device else "host"))
    assert {k: got.stats[k] for k in BRICK_STATS} == dict.fromkeys(BRICK_STATS, 0)
    if seed == 5:
        print("summary", summary(got))
        assert summary(got) == RANDOM_SUMMARIES[density]


# ---- above 2^24 points ------------------------------------------------------------------------------------------------------------
BIG = (264, 256, 256)                                                        # nx, ny, nz


def big_case():
    """Two interleaved combs and a buried hollow block on 264 x 256 x 256 points, built from disjoint index boxes [lo, hi) in
    (i, j, k): (boxes of body 0, of body 1, of body 2, the cavity's box).  Comb A: a spine at i in [2, 4) with 30 teeth toward
    +x; comb B: a spine at i in [258, 260) with 30 teeth toward -x between A's, two points away from them.  Both span
    k in [10, 100).  The block [40, 200) x [40, 200) x [120, 180) is hollow: [100, 140) x [90, 150) x [130, 170)."""
    teeth_a = [((4, 8 * t + 2, 10), (200, 8 * t + 4, 100)) for t in range(30)]
    comb_a = [((2, 2, 10), (4, 8 * 29 + 4, 100))] + teeth_a
    teeth_b = [((60, 8 * t + 6, 10), (258, 8 * t + 8, 100)) for t in range(30)]
    comb_b = [((258, 6, 10), (260, 8 * 29 + 8, 100))] + teeth_b
    hole = ((100, 90, 130), (140, 150, 170))
    (x0, y0, z0), (x1, y1, z1) = (40, 40, 120), (200, 200, 180)
    (a0, b0, c0), (a1, b1, c1) = hole
    block = [((x0, y0, z0), (x1, y1, c0)), ((x0, y0, c1), (x1, y1, z1)),          # below and above the hole in k
             ((x0, y0, c0), (x1, b0, c1)), ((x0, b1, c0), (x1, y1, c1)),          # then in j
             ((x0, b0, c0), (a0, b1, c1)), ((a1, b0, c0), (x1, b1, c1))]          # then in i
    return comb_a, comb_b, block, hole


def test_above_2_to_the_24_points(res):
    nx, ny, nz = BIG
    assert nx * ny * nz > 2 ** 24
    bodies = big_case()[:3]
    hole = big_case()[3]
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    want_lab = np.full((nz, ny, nx), TR.EXTERIOR, dtype=np.uint32)
    for b, boxes in enumerate(bodies):                                        # numbered by their first points: k = 10 (A before B), k = 120
        for lo, hi in boxes:
            assert not occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any()       # disjoint boxes: the rows add up
            occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = 1
            want_lab[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = b
    want_lab[hole[0][2]:hole[1][2], hole[0][1]:hole[1][1], hole[0][0]:hole[1][0]] = TR.CAVITY_BIT
    got = res.label_occupancy(occ)
    print(got.counts, got.stats)
    # closed forms: each comb and the block's shell are simply connected solids; the shell encloses one cavity
    assert summary(got) == (3, 1, 1 + 1 + 2, 0)
    volume = lambda boxes: sum((hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) for lo, hi in boxes)   # noqa: E731
    assert got.counts["points"] == sum(volume(b) for b in bodies)
    assert got.counts["exterior_points"] == nx * ny * nz - got.counts["points"] - volume([hole])
    a = occ.view(bool)
    assert got.counts["edges"] == int(np.count_nonzero(a[:, :, :-1] & a[:, :, 1:]) + np.count_nonzero(a[:, :-1] & a[:, 1:])
                                      + np.count_nonzero(a[:-1] & a[1:]))
    rows = [TR.combine_rows([M.box_moments(lo, hi) for lo, hi in boxes]) for boxes in bodies]
    assert [[int(x) for x in row] for row in got.body_moments] == rows
    assert [[int(x) for x in row] for row in got.cavity_moments] == [M.box_moments(*hole)]
    lab = got.labels()
    for k in (0, 9, 10, 55, 99, 100, 119, 120, 129, 130, 150, 169, 170, 179, 180, 255):
        assert np.array_equal(lab[k], want_lab[k]), k
    assert np.array_equal(lab[:, 100, :], want_lab[:, 100, :]) and np.array_equal(lab[:, :, 259], want_lab[:, :, 259])


# ---- contract edges -----------------------------------------------------------------------------------------------------------------
def test_the_empty_program(res):
    cc, w = 0, np.zeros(0, dtype=np.uint32)
    use(res, cc, w)
    origin, step, shape = box_lattice(37, -2.0, 2.0)
    got = check_solid(res, cc, w, origin, step, shape, 0.0, what="empty")
    assert summary(got) == (0, 0, 0, 0) and got.counts["exterior_points"] == 37 ** 3
    # a level above max_dist: one body fills the lattice, from the probes alone
    got = check_solid(res, cc, w, origin, step, shape, 1000.0, what="empty")
    assert summary(got) == (1, 0, 1, 0) and got.counts["points"] == 37 ** 3
    assert got.stats["bricks_kept"] == 0 and got.stats["evaluations"] == got.stats["bricks"] == 125
    assert [int(x) for x in got.body_moments[0]] == M.box_moments((0, 0, 0), shape)


def test_nan_is_outside(res):
    cc, w = words_of((204, [0.0]), (0, [0.2, 0.1, -0.1, 0.9]), (205, []))     # Scale by 0 around a sphere
    use(res, cc, w)
    origin, step, shape = box_lattice(20, -2.0, 2.0)
    assert not M.lattice_inside(cc, w, origin, step, shape, 0.0).any()
    got = check_solid(res, cc, w, origin, step, shape, what="scale 0")
    assert summary(got) == (0, 0, 0, 0) and got.counts["exterior_points"] == 20 ** 3


def lattice(o=(-2.0, -2.0, -2.0), s=(0.25, 0.25, 0.25)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


SENTINEL = 0x5A5A5A5A5A5A5A5A


def test_errors_leave_the_outputs_untouched():
    L = _ffi.hip_lib()
    r = renderer.RayMarchingResources(0)                                      # a context of its own: nothing labelled yet
    try:
        r.resize_command_buffer(65536)
        cc, w = scene_program("g8")
        use(r, cc, w)
        NC, NS = _ffi.RM_TOPO_COUNTS, _ffi.RM_TOPO_STATS
        counts, stats = (C.c_uint64 * NC)(*[SENTINEL] * NC), (C.c_uint64 * NS)(*[SENTINEL] * NS)
        untouched = lambda: all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in stats)   # noqa: E731
        buf = np.zeros(64, dtype=np.uint64)
        assert L.rm_read_topology(r._h, buf.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_ARG       # before any labelling
        assert L.rm_read_topology(None, buf.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_NULL
        o, s = lattice()
        solid = lambda h=r._h, o=o, s=s, n=(17, 17, 17), level=0.0, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_label_solid(h, o, s, n[0], n[1], n[2], level, counts, nc, stats, ns)   # noqa: E731
        assert solid(h=None) == _ffi.RM_ERR_NULL
        assert solid(counts=None) == _ffi.RM_ERR_NULL and solid(stats=None) == _ffi.RM_ERR_NULL
        assert solid(o=None) == _ffi.RM_ERR_NULL and solid(s=None) == _ffi.RM_ERR_NULL
        assert solid(nc=NC - 1) == _ffi.RM_ERR_ARG and solid(ns=NS - 1) == _ffi.RM_ERR_ARG
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2), (2, 65536, 2), (1024, 1024, 512)):
            assert solid(n=n) == _ffi.RM_ERR_RANGE, n
        for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
            assert solid(s=lattice(s=bad)[1]) == _ffi.RM_ERR_ARG, bad
        assert solid(o=lattice(o=(0.0, np.inf, 0.0))[0]) == _ffi.RM_ERR_ARG
        for level in (np.nan, np.inf):
            assert solid(level=level) == _ffi.RM_ERR_ARG
        occ = np.ones((4, 4, 4), dtype=np.uint8)
        occupancy = lambda h=r._h, n=(4, 4, 4), p=occ.ctypes.data, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_label_occupancy(h, n[0], n[1], n[2], p, 0, None, counts, nc, stats, ns)   # noqa: E731
        assert occupancy(h=None) == _ffi.RM_ERR_NULL and occupancy(p=None) == _ffi.RM_ERR_NULL
        assert occupancy(counts=None) == _ffi.RM_ERR_NULL and occupancy(stats=None) == _ffi.RM_ERR_NULL
        assert occupancy(nc=NC - 1) == _ffi.RM_ERR_ARG and occupancy(ns=NS - 1) == _ffi.RM_ERR_ARG
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2)):
            assert occupancy(n=n) == _ffi.RM_ERR_RANGE, n
        # an invalid program: the status a query gives
        r.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
        assert solid() == _ffi.RM_ERR_STACK_UNDERFLOW
        assert untouched()
        assert L.rm_read_topology(r._h, buf.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_ARG       # still nothing labelled
        with pytest.raises(ValueError):
            r.label_solid_grid((0, 0, 0), (0.1, 0.1, 0.1), (1, 4, 4))
        with pytest.raises(ValueError):
            r.label_occupancy(np.zeros((4, 4, 4), dtype=np.float32))
        use(r, cc, w)
        assert solid() == _ffi.RM_OK and not untouched()
        assert occupancy() == _ffi.RM_OK and counts[_ffi.RM_TOPO_BODIES] == 1 and counts[_ffi.RM_TOPO_POINTS] == 64
    finally:
        r.close()


def test_every_subset_of_the_outputs_on_host_and_device(res):
    import torch
    cc, w = hollow_sphere()
    use(res, cc, w)
    origin, step, shape = box_lattice((33, 20, 17))
    got = res.label_solid_grid(origin, step, shape)
    want = [got.body_moments.copy(), got.cavity_moments.copy(), got.labels().ravel()]
    assert want[0].shape == (1, 16) and want[1].shape == (1, 16)
    L = res._L
    for subset in itertools.product((False, True), repeat=3):
        if not any(subset):
            continue
        host = [np.full(x.shape, 0x5A, dtype=x.dtype) if on else None for x, on in zip(want, subset)]
        res._check(L.rm_read_topology(res._h, *[a.ctypes.data if a is not None else None for a in host], 0, None))
        for a, x in zip(host, want):
            assert a is None or np.array_equal(a, x), subset
        dev = [torch.full(x.shape, 0x5A, dtype=torch.int64 if x.dtype == np.uint64 else torch.int32, device="cuda:0") if on else None
               for x, on in zip(want, subset)]
        res.read_topology_device(*[t.data_ptr() if t is not None else 0 for t in dev], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for t, x in zip(dev, want):
            assert t is None or t.cpu().numpy().view(x.dtype).tobytes() == x.tobytes(), subset
    # a misaligned device array is refused
    t = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    assert L.rm_read_topology(res._h, C.c_void_p(t.data_ptr() + 4), None, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_topology(res._h, None, None, C.c_void_p(t.data_ptr() + 2), 1, None) == _ffi.RM_ERR_ARG


def test_two_runs_give_identical_words(res):
    cc, w = scene_program("g32")
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    a = res.label_solid_grid(origin, step, shape)
    la = a.labels()
    b = res.label_solid_grid(origin, step, shape)
    assert a.counts == b.counts and a.stats == b.stats
    assert a.body_moments.tobytes() == b.body_moments.tobytes() and a.cavity_moments.tobytes() == b.cavity_moments.tobytes()
    assert la.tobytes() == b.labels().tobytes()


def test_draws_meshes_and_slices_are_left_alone(res, oracle):
    cc, w = scene_program("xform_mix")
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    first = res.draw(W, H)
    origin, step, shape = box_lattice(40)
    mesh = res.extract_mesh_grid_sparse(origin, step, shape)
    slices = res.slice_contours((-2.5,) * 3, (2.5,) * 3, 40, heights=[0.0, 0.4])
    assert len(mesh.triangles) > 0 and len(slices.points) > 0
    infos = sorted(k for k in dir(_ffi) if k.startswith("RM_INFO_") and isinstance(getattr(_ffi, k), int))
    before = {k: res.info(getattr(_ffi, k)) for k in infos}
    got = res.label_solid_grid(origin, step, shape)
    assert got.bodies == 3
    assert res.label_occupancy(np.ones((9, 9, 9), dtype=bool)).bodies == 1
    assert {k: res.info(getattr(_ffi, k)) for k in infos} == before
    assert res.draw(W, H).tobytes() == first.tobytes()
    v, t = np.empty((len(mesh.vertices), 3), dtype=np.float32), np.empty((len(mesh.triangles), 3), dtype=np.uint32)
    res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, None, None, 0, None))
    assert v.tobytes() == mesh.vertices.tobytes() and t.tobytes() == mesh.triangles.tobytes()
    p = np.empty((len(slices.points), 3), dtype=np.float32)
    res._check(res._L.rm_read_slices(res._h, p.ctypes.data, None, None, None, None, 0, None))
    assert p.tobytes() == np.asarray(slices.points).tobytes()
