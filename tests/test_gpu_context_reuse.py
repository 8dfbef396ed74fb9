"""One context through every host-destination entry point at a small size, a larger one and the small one again, under three
programs whose record counts make the device copy of the program grow twice: every result is bit-identical to the same call
on a fresh context.  The scratch of a context (program copies, staging buffers of the draws and of the queries, the mesh and
slice buffers) only ever grows and is shared by all entry points; a call must neither depend on what an earlier, larger call
left there nor on where a buffer that just moved used to lie."""
import numpy as np
import pytest

from ray_marching_amd import _ffi, camera, csg, renderer

pytestmark = pytest.mark.gpu

F = np.float32
DRAWS = ((8, 8), (64, 48), (8, 8))
COUNTS = (1, 1000, 3)
GRIDS = ((2, 2, 2), (17, 9, 5), (2, 2, 2))


def chain(n):
    """A union of n spheres on a ring, every other one tagged with a material: n records (a chain's operators travel with
    their right operands) -> (cmd_count, words)."""
    words, cc = [], 0
    for i in range(n):
        a = 2.0 * np.pi * i / n
        sphere = np.array([1.5 * np.cos(a), 0.2 * np.sin(3.0 * a), 1.5 * np.sin(a), 0.35], dtype=F)
        words += [csg.CSGCommandType.Sphere] + [int(x) for x in sphere.view(np.uint32)]
        if i % 2:
            words += [csg.CSGCommandType.Material, i % 3]
        if i:
            words += [csg.CSGCommandType.Union]
        cc += 1 + i % 2 + (i > 0)
    return cc, np.asarray(words, dtype=np.uint32)


def fresh():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(32768)
    r.set_option(_ffi.RM_OPT_SPECIALIZE, 0)  # (the interpreter kernels: no compiler threads, and the same kernel in every context)
    r.set_materials([(0.4, 0.7, 0.1), (0.9, 0.15, 0.1), (0.1, 0.3, 0.9)])
    r.set_limits(renderer.RayMarchLimits(0.01, 100.0, 64))
    return r


def calls(r, cam, step, solids):
    """Every host-destination entry point at the sizes of `step` -> {name: array}."""
    W, H = DRAWS[step]
    n = COUNTS[step]
    u = renderer.prepare_uniforms((W, H), cam)
    r.set_uniforms(u)
    rng = np.random.default_rng(7 + step)
    pts = rng.uniform(-2.5, 2.5, (n, 3)).astype(F)
    rays = np.ascontiguousarray(r.camera_rays(W, H)[np.linspace(0, W * H - 1, n).astype(np.int64)])
    out = {"draw": r.draw(W, H), "strips": r.draw_strips(W, H, 8, 1 if H > 8 else 0, 2 if H > 8 else 1),
           "batch": r.draw_batch([u, u], W, H), "lit": r.draw_lit(W, H), "camera_rays": r.camera_rays(W, H),
           "grid": r.sample_grid((-2.0, -1.0, -2.0), (0.25, 0.25, 0.5), GRIDS[step])}
    for name, d in (("gbuffer", r.draw_gbuffer(W, H)), ("points", r.query_points(pts, normals=True)), ("rays", r.cast_rays(rays))):
        out.update({name + "." + k: v for k, v in d.items()})
    if solids:  # one dense mesh, one sparse mesh and one slice call on a 9^3 lattice
        for name, m in (("mesh", r.extract_mesh(-2.0, 2.0, 9)), ("sparse", r.extract_mesh_sparse(-2.0, 2.0, 9))):
            out.update({name + ".v": m.vertices, name + ".t": m.triangles, name + ".n": m.normals, name + ".leaf": m.leaf,
                        name + ".material": m.material})
        s = r.slice_contours(-2.0, 2.0, 9, layer_height=0.5, normals=True, ids=True)
        out.update({"slice.p": s.points, "slice.c": s.contours, "slice.first": s.layer_first, "slice.n": s.normals,
                    "slice.leaf": s.leaf, "slice.material": s.material})
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_a_reused_context_gives_what_a_fresh_one_gives():
    ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
    ctl.update(camera.Orbit([35.0, -25.0]))
    programs = [chain(20), chain(100), chain(700)]
    records = [renderer.program_info(cc, w)["records"] for cc, w in programs]
    # the device copy holds max(64, twice the records, their unit records and tree masks) of the program that made it grow:
    # under 64, over 64, and over six times that (a record has at most one unit record and one tree mask)
    assert records[0] < 64 < records[1] and records[2] > 6 * records[1], records
    cam = ctl.camera()
    shared = fresh()
    try:
        for p, (cc, w) in enumerate(programs):
            shared.set_program(cc, w)
            for step in range(3):
                got = calls(shared, cam, step, solids=step == 1)
                alone = fresh()
                try:
                    alone.set_program(cc, w)
                    want = calls(alone, cam, step, solids=step == 1)
                finally:
                    alone.close()
                assert got.keys() == want.keys()
                for k in want:
                    assert same(got[k], want[k]), (records[p], step, k)
                if step == 1:
                    assert got["draw"].any() and len(got["mesh.v"]) and len(got["slice.p"])  # (something was drawn, meshed and sliced)
    finally:
        shared.close()
