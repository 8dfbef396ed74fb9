"""Seeded random CSG programs (tests/fuzz_programs.py: one generator per record loop -- general, tree, chain) and constructed
tie / NaN programs through the entry points that stand on the query walk and the query launch's LDS sizing: rm_query_points,
rm_cast_rays, rm_draw_gbuffer, rm_draw_lit, rm_extract_mesh[_sparse] and rm_slice_contours, each against its reference
(oracle/rm_oracle_np.py, tests/gbuffer_ref.py, light_ref.py, mesh_ref.py, slice_ref.py), bit for bit with two NaNs equal.
What the inputs are is checked without a GPU in tests/test_query_fuzz_cpu.py.

RM_QUERY_FUZZ_SEEDS=N runs N seeds per class (default 8) from RM_QUERY_FUZZ_FIRST_SEED.

The material table of every case is random; a program without tags ignores it (the hit colour is the reference's constant,
as the C oracle has it), so the numpy references get the table only for tagged programs."""
import numpy as np
import pytest

import fuzz_programs as FP
import gbuffer_ref
import light_ref
import mesh_ref
import slice_ref
from oracle import rm_oracle_np as onp
from test_gpu_lit import NON_DEFAULT, set_light
from test_gpu_query import march_replay, oracle_taps_normal, same
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
W, H = FP.W, FP.H
CASES = [(cls, seed) for cls in FP.CLASSES for seed in FP.SEEDS]
LOOPS = {"chain": (1, 2), "tree": (3, 4), "general": (0, 5)}     # RM_INFO_INTERPRETER_LOOP
FORMS = (_ffi.RM_SAMPLE_ALL, _ffi.RM_SAMPLE_CENTER, 9)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_option(_ffi.RM_OPT_SPECIALIZE, 0)          # the interpreter kernel: the loop it reports is the loop the queries take
    yield r
    r.close()


def use(res, c):
    """The case on the context; the record loop its program takes is the one its class promises (a failure, not a skip).  A
    constructed program names its loop itself (fuzz_programs.loop_class)."""
    res.set_output_format(_ffi.RM_FORMAT_RGBA32F)
    res.set_materials(c.table)
    res.set_limits(c.limits)
    res.set_program(c.cc, c.words)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(c.u)))
    res.set_option(_ffi.RM_OPT_CULL, 0)
    res.draw(8, 8)
    loop = int(res.info(_ffi.RM_INFO_INTERPRETER_LOOP))
    res.set_option(_ffi.RM_OPT_CULL, 1)
    want = LOOPS[getattr(c, "loop", c.cls)]
    assert loop in want, "interpreter loop %d, expected one of %s: %s" % (loop, want, FP.describe(c))


def tagged(c):
    return 300 in FP.opcodes(c.cc, c.words)


def check(got, want, c, what, at=None):
    """got == want bit for bit (two NaNs equal); the message names the first element that differs and the input there."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s has shape %s, reference %s; %s" % (what, got.shape, want.shape, FP.describe(c))
    if same(got, want):
        return
    if got.dtype.kind == "f":
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    idx = np.argwhere(bad)
    i = tuple(int(x) for x in idx[0])
    where = "" if at is None else " input %s" % np.asarray(at)[i[0]].tolist()
    raise AssertionError("%s differs at %d elements, first %s: got %r, reference %r;%s %s" % (
        what, len(idx), i, got[i].tolist(), want[i].tolist(), where, FP.describe(c)))


# ---- points ----------------------------------------------------------------------------------------------------------------------
def check_points(res, c, p, every=7):
    mx = F(c.limits[1])
    q = res.query_points(p, normals=True)
    with np.errstate(all="ignore"):
        d, m = onp.map_scene(c.cc, c.words, mx, p[:, 0], p[:, 1], p[:, 2], want_material=True)
        leaf, _ = gbuffer_ref.leaf_and_material(c.cc, c.words, mx, p[:, 0], p[:, 1], p[:, 2])
        sub = p[::every]
        normal = oracle_taps_normal(c.cc, c.words, mx, sub)
    check(q["distance"], d, c, "rm_query_points distance", p)
    check(q["material"], m, c, "rm_query_points material", p)
    check(q["leaf"], leaf, c, "rm_query_points leaf", p)
    check(q["normal"][::every], normal, c, "rm_query_points normal", sub)
    return q


def check_point_outputs(res, c, p, full):
    """Every subset of the outputs on device memory gives the bits of the full query: with the ids the launch is sized for the
    walk's LDS layout, without them for the distance loop's."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(p)
    pt = torch.from_numpy(p).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for mask in range(1, 8):
        d = torch.full((n,), -1.0, device=dev) if mask & 1 else None
        nr = torch.full((n, 3), -1.0, device=dev) if mask & 2 else None
        ids = torch.full((n, 2), -7, dtype=torch.int32, device=dev) if mask & 4 else None
        res.query_points_device(n, pt.data_ptr(), d.data_ptr() if d is not None else 0, nr.data_ptr() if nr is not None else 0,
                                ids.data_ptr() if ids is not None else 0, stream=st)
        torch.cuda.synchronize()
        if d is not None:
            check(d.cpu().numpy(), full["distance"], c, "outputs %d: distance" % mask, p)
        if nr is not None:
            check(nr.cpu().numpy(), full["normal"], c, "outputs %d: normal" % mask, p)
        if ids is not None:
            got = ids.cpu().numpy().view(np.uint32)
            check(got[:, 0], full["leaf"], c, "outputs %d: leaf" % mask, p)
            check(got[:, 1], full["material"], c, "outputs %d: material" % mask, p)


@pytest.mark.parametrize("cls,seed", CASES)
def test_points(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    use(res, c)
    p = FP.points_of(c)
    assert len(p) % 64 != 0 and len(p) > 18000
    full = check_points(res, c, p)
    check_point_outputs(res, c, p, full)


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def check_rays(res, c, rays):
    mx = F(c.limits[1])
    hit = res.cast_rays(rays)
    kind, steps, t, pos = march_replay(c.cc, c.words, c.limits, rays)
    check(hit["kind"], kind, c, "rm_cast_rays kind", rays)
    check(hit["steps"], steps, c, "rm_cast_rays steps", rays)
    check(hit["t"], t, c, "rm_cast_rays t", rays)
    check(hit["position"], pos, c, "rm_cast_rays position", rays)
    with np.errstate(all="ignore"):
        rgb = onp.ray_march(c.cc, c.words, c.limits, *[rays[:, k].copy() for k in range(6)],
                            materials=c.table if tagged(c) else None)
    check(hit["rgb"], rgb.T, c, "rm_cast_rays rgb", rays)
    s = kind == _ffi.RM_HIT_SURFACE
    with np.errstate(all="ignore"):
        leaf, mat = gbuffer_ref.leaf_and_material(c.cc, c.words, mx, pos[s, 0], pos[s, 1], pos[s, 2])
        normal = oracle_taps_normal(c.cc, c.words, mx, pos[s])
    check(hit["leaf"][s], leaf, c, "rm_cast_rays leaf", rays[s])
    check(hit["material"][s], mat, c, "rm_cast_rays material", rays[s])
    check(hit["normal"][s], normal, c, "rm_cast_rays normal", rays[s])
    f = kind == _ffi.RM_HIT_FLOOR
    assert np.all(hit["normal"][f] == np.array([0, 1, 0], F)) and np.all(hit["diffuse"][~s] == 0), FP.describe(c)
    assert np.all(hit["leaf"][~s] == _ffi.RM_NO_ID) and np.all(hit["material"][~s] == _ffi.RM_NO_ID), FP.describe(c)
    return hit


def check_ray_outputs(res, c, rays, full):
    import torch
    dev = torch.device("cuda", 0)
    n = len(rays)
    rt = torch.from_numpy(rays).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for mask in range(1, 8):
        hit = torch.full((n, 8), -1.0, device=dev) if mask & 1 else None
        ids = torch.full((n, 4), -7, dtype=torch.int32, device=dev) if mask & 2 else None
        rgb = torch.full((n, 3), -1.0, device=dev) if mask & 4 else None
        res.cast_rays_device(n, rt.data_ptr(), hit.data_ptr() if hit is not None else 0, ids.data_ptr() if ids is not None else 0,
                             rgb.data_ptr() if rgb is not None else 0, stream=st)
        torch.cuda.synchronize()
        if hit is not None:
            h = hit.cpu().numpy()
            for k, part in (("t", h[:, 0]), ("position", h[:, 1:4]), ("normal", h[:, 4:7]), ("diffuse", h[:, 7])):
                check(part, full[k], c, "outputs %d: %s" % (mask, k), rays)
        if ids is not None:
            got = ids.cpu().numpy().view(np.uint32)
            for k, key in enumerate(("kind", "steps", "leaf", "material")):
                check(got[:, k], full[key], c, "outputs %d: %s" % (mask, key), rays)
        if rgb is not None:
            check(rgb.cpu().numpy(), full["rgb"], c, "outputs %d: rgb" % mask, rays)


@pytest.mark.parametrize("cls,seed", CASES)
def test_rays(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    use(res, c)
    rays = FP.rays_of(c)
    full = check_rays(res, c, rays)
    check_ray_outputs(res, c, rays, full)


# ---- G-buffer --------------------------------------------------------------------------------------------------------------------
def check_gbuffer(got, want, c, what):
    assert tuple(got) == gbuffer_ref.KEYS
    for k in gbuffer_ref.KEYS:
        check(got[k].reshape((-1,) + got[k].shape[2:]), want[k].reshape((-1,) + want[k].shape[2:]), c, "rm_draw_gbuffer %s: %s" % (what, k))


def reduced(records, ids, select, rows=H):
    return {k: v.reshape((rows, W) + v.shape[1:]) for k, v in gbuffer_ref.reduce(records, ids, select).items()}


@pytest.mark.parametrize("cls,seed", CASES)
def test_gbuffer(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    use(res, c)
    sel = (0, c.cc // 2)
    want, records = gbuffer_ref.render(c.ud, c.limits, c.cc, c.words, W, H, select=sel, detail=True)
    check_gbuffer(res.draw_gbuffer(W, H, select=sel), want, c, "all samples, select %s" % (sel,))
    for sample in FORMS[1:]:
        check_gbuffer(res.draw_gbuffer(W, H, sample=sample, select=sel),
                      gbuffer_ref.render(c.ud, c.limits, c.cc, c.words, W, H, sample=sample, select=sel), c, "sample %d" % sample)
    # an odd row band is those rows of the frame
    band = res.draw_gbuffer(W, H, 3, 5, select=sel)
    check_gbuffer(band, {k: v[3:8] for k, v in want.items()}, c, "rows 3..7")
    if seed == FP.SEEDS[0]:       # the selection of a graph node: the sub-tree of a random command
        node = int(np.random.default_rng(seed).integers(0, c.cc))
        sub = renderer.program_subtree(c.cc, c.words, node)
        check_gbuffer(res.draw_gbuffer(W, H, select=sub), reduced(records, list(range(16)), sub), c, "sub-tree %s of command %d" % (sub, node))


# ---- lit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,seed", CASES)
def test_lit(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    use(res, c)
    table = c.table if tagged(c) else None
    try:
        for what, named in (("default lighting", {}), ("shadow and occlusion, 3 shadow steps, no bias", NON_DEFAULT)):
            p = set_light(res, **named)
            ref = light_ref.render(c.ud, c.limits, c.cc, c.words, W, H, materials=table, light=p)[0]
            check(res.draw_lit(W, H).reshape(-1, 4), ref.reshape(-1, 4), c, "rm_draw_lit, " + what)
        set_light(res, **light_ref.IDENTITY)
        check(res.draw_lit(W, H).reshape(-1, 4), res.draw(W, H).reshape(-1, 4), c, "rm_draw_lit without shadow and occlusion against rm_draw")
    finally:
        set_light(res)


# ---- mesh and slices ---------------------------------------------------------------------------------------------------------------
MESH = ((-3.0,) * 3, (F(6.0) / F(23),) * 3, (24, 24, 24))
SLICE = ((-3.0, -3.0), (F(6.0) / F(39), F(6.0) / F(39)), (40, 40), [-0.4, 0.1, 0.75])


def grid_distances(c, p, shape):
    with np.errstate(all="ignore"):
        return np.asarray(onp.map_scene(c.cc, c.words, F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2]), dtype=F).reshape(shape)


@pytest.mark.parametrize("cls,seed", CASES)
def test_mesh_and_slices(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    use(res, c)
    origin, step, shape = MESH
    dist = grid_distances(c, mesh_ref.lattice_points(origin, step, shape), shape[::-1])
    v, t = mesh_ref.extract(dist, origin, step, 0.0)
    m = res.extract_mesh_grid(origin, step, shape)
    check(m.vertices, v, c, "rm_extract_mesh vertices")
    check(m.triangles, t, c, "rm_extract_mesh triangles")
    if len(v):
        q = res.query_points(m.vertices, normals=True)
        check(m.normals, q["normal"], c, "rm_extract_mesh normals against rm_query_points", m.vertices)
        check(m.leaf, q["leaf"], c, "rm_extract_mesh leaf against rm_query_points", m.vertices)
        check(m.material, q["material"], c, "rm_extract_mesh material against rm_query_points", m.vertices)
    sparse = res.extract_mesh_grid_sparse(origin, step, shape)
    for k in ("vertices", "triangles", "normals", "leaf", "material"):
        check(getattr(sparse, k), getattr(m, k), c, "rm_extract_mesh_sparse %s against the dense extraction" % k)
    o, s, n, heights = SLICE
    for axis in range(3):
        layers = [grid_distances(c, slice_ref.layer_points(axis, o, s, n, h), (n[1], n[0])) for h in heights]
        pts, con, lf = slice_ref.slice_contours(layers, axis, o, s, heights, 0.0)
        sl = res.slice_contours_grid(axis, o, s, n, heights, normals=True, ids=True)
        check(sl.points, pts, c, "rm_slice_contours axis %d points" % axis)
        check(sl.contours, con, c, "rm_slice_contours axis %d contours" % axis)
        check(sl.layer_first, lf, c, "rm_slice_contours axis %d layer_first" % axis)
        if len(pts):
            q = res.query_points(sl.points, normals=True)
            check(sl.normals, q["normal"], c, "rm_slice_contours axis %d normals against rm_query_points" % axis, sl.points)
            check(sl.leaf, q["leaf"], c, "rm_slice_contours axis %d leaf against rm_query_points" % axis, sl.points)
            check(sl.material, q["material"], c, "rm_slice_contours axis %d material against rm_query_points" % axis, sl.points)


# ---- constructed ties and NaN operands -----------------------------------------------------------------------------------------------
N_TIES = 36          # fuzz_programs.tie_cases (7 pairs x 5 places) and nan_case; tests/test_query_fuzz_cpu.py counts them


@pytest.mark.parametrize("k", range(N_TIES))
def test_ties_and_nan_operands(res, oracle, k):
    cases = FP.tie_cases(oracle) + [FP.nan_case(oracle)]
    assert len(cases) == N_TIES
    c = cases[k]
    use(res, c)
    p = FP.tie_point_set(c)
    full = check_points(res, c, p, every=1)
    check_point_outputs(res, c, p, full)
    check_rays(res, c, FP.tie_rays(c))
    # the second of the two tied operands selected: by the rule the first wins a tie, so the mask is the reference's -- and
    # with the first selected, the command right behind the selection is the second's primitive
    want, records = gbuffer_ref.render(c.ud, c.limits, c.cc, c.words, W, H, select=c.second, detail=True)
    assert want["surface_mask"].any(), c.name
    if c.cls == "tie" and "duplicates" in c.name and not c.name.startswith("subtraction"):
        assert not want["selected_mask"].any(), c.name          # every hit of a duplicated pair is a tie
    check_gbuffer(res.draw_gbuffer(W, H, select=c.second), want, c, c.name + ", second operand selected")
    first = reduced(records, list(range(16)), c.first)
    if c.cls == "tie" and not c.name.endswith("chain") and not c.name.startswith("subtraction"):
        assert first["selected_mask"].any(), c.name
    check_gbuffer(res.draw_gbuffer(W, H, select=c.first), first, c, c.name + ", first operand selected")


# ---- the shadow march's threshold ------------------------------------------------------------------------------------------------------
def test_a_shadow_step_at_exactly_min_dist_is_no_hit(res, oracle):
    """Floor points whose first shadow step returns exactly min_dist (fuzz_programs.shadow_threshold_case): `h < min_dist` ends a
    shadow march, `h == min_dist` does not."""
    c = FP.shadow_threshold_case(oracle)
    use(res, c)
    try:
        p = set_light(res, **c.light)
        ref = light_ref.render(c.ud, c.limits, c.cc, c.words, W, H, materials=None, light=p)[0]
        check(res.draw_lit(W, H).reshape(-1, 4), ref.reshape(-1, 4), c, "rm_draw_lit at the shadow threshold")
    finally:
        set_light(res)
