"""Ray traversal on the GPU (rm_trace_rays) against the numpy restatement of DESIGN.md section 18 (tests/trace_ref.py), bit for
bit with two NaNs equal: the three standard configurations on scenes of every record loop, random programs of each loop
class, the attributes against rm_query_points, every subset of the outputs, the edge cases of the parameters and sizes, the
device / torch path, every error status with the outputs untouched, and isolation from the draw state."""
import ctypes as C

import numpy as np
import pytest

import fuzz_programs as FP
import scenes
import trace_ref as TR
from test_gpu_query import commands, same
from test_gpu_query_fuzz import use
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
LIM = (0.01, 100.0, 128)
SCENES = ("g8", "xform_mix", "mat_mix", "g32s", "g32_balanced")     # chain, general (transforms; tags; smooth blends), tree
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    r.set_limits(LIM)
    yield r
    r.close()


def named(p):
    return dict(zip(TR.NAMES, [float(v) for v in p]))


def compare(got, want, what):
    assert tuple(got) == TR.KEYS
    for k in TR.KEYS:
        g = np.asarray(got[k])
        if not same(g, want[k]):
            bad = np.argwhere(~((g.view(np.uint32) == want[k].view(np.uint32)) | (np.isnan(g) & np.isnan(want[k])
                                                                                 if g.dtype.kind == "f" else False)))
            i = tuple(int(x) for x in bad[0])
            raise AssertionError("%s: %s differs at %d elements, first %s: got %r, reference %r" % (
                what, k, len(bad), i, g[i].tolist(), want[k][i].tolist()))


def check(res, cc, w, max_dist, rays, p, K, normals=True, ids=True, what=""):
    """The call on the host path against the reference; returns the GPU's result."""
    got = res.trace_rays(rays, max_events=K, normals=normals, ids=ids, **named(p))
    want = TR.trace(cc, w, max_dist, rays, p, K, normals=normals, ids=ids)
    compare(got, want, what)
    return got


def check_attributes_against_points(res, got, K):
    filled = np.arange(K)[None, :] < got["stored"][:, None]
    pos = np.ascontiguousarray(got["position"][filled])
    if len(pos):
        q = res.query_points(pos, normals=True)
        assert same(got["normal"][filled], q["normal"])
        assert np.array_equal(got["leaf"][filled], q["leaf"]) and np.array_equal(got["material"][filled], q["material"])
    return int(filled.sum())


def test_the_scenes_cover_the_three_record_loops(oracle):
    assert {FP.loop_class(*oracle.serialize(*ALL[name]())) for name in SCENES} == {"general", "tree", "chain"}


@pytest.mark.parametrize("config", sorted(TR.CONFIGS))
@pytest.mark.parametrize("name", SCENES)
def test_configurations_vs_reference(res, oracle, name, config):
    cc, w = oracle.serialize(*ALL[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    p, K = TR.config(config)
    rays = TR.standard_rays()
    got = check(res, cc, w, LIM[1], rays, p, K, what="%s %s" % (name, config))
    n_events = check_attributes_against_points(res, got, K)
    assert n_events > 500, (name, config, n_events)
    if config == "many_events":
        assert (got["events"] > K).any()
    if config == "out_of_steps":
        assert (got["flags"] & _ffi.RM_TRACE_OUT_OF_STEPS).any()


def fuzz_rays(c):
    """2001 rays for a random program: 1701 from origins in [-3, 3]^3 towards points near the centres of its primitives
    (random programs are small and scattered: unaimed rays mostly miss them) and, for the origins inside solids and the
    degenerate directions (zero, NaN, inf), the two ends of the case's own rays."""
    rng = np.random.default_rng(c.seed + 3)
    centres = np.asarray([p[:3] for _, op, p in commands(c.words, c.cc) if op in (0, 1, 10)] or [[0, 0, 0]], dtype=np.float64)
    o = rng.uniform(-3, 3, (1701, 3))
    d = centres[rng.integers(0, len(centres), 1701)] + rng.normal(0, 0.3, (1701, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    own = FP.rays_of(c)
    rays = np.ascontiguousarray(np.concatenate([np.concatenate([o, d], axis=1).astype(F), own[:150], own[-150:]]))
    assert len(rays) == 2001
    return rays


@pytest.mark.parametrize("cls,seed", [(cls, seed) for cls in FP.CLASSES for seed in list(FP.SEEDS)[:2]])
def test_random_programs(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 0)        # the interpreter kernel reports the loop the queries take
    try:
        use(res, c)                                  # the case on the context; asserts its loop class
        rays = fuzz_rays(c)
        p = TR.params(t_min=0.25, t_max=12.0, min_step=0.005, step_scale=1.0, level=0.0, max_steps=1024)
        got = check(res, c.cc, c.words, c.limits[1], rays, p, 8, what=FP.describe(c))
        # (1363..3045 stored events by the reference, except general seed 1, whose primitives sit inside transforms: 25)
        assert check_attributes_against_points(res, got, 8) > 20, FP.describe(c)
    finally:
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)
        res.set_materials(scenes.MATERIAL_TABLE)
        res.set_limits(LIM)


@pytest.mark.parametrize("name", ["g8", "mat_mix"])
def test_every_output_subset(res, oracle, name):
    """Each of the four arrays alone, events without ids and every other subset, under flags 0 / NORMALS / IDS / both, on
    device memory: what one array receives does not depend on which others were asked for."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    cc, w = oracle.serialize(*ALL[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    p, K = TR.config("level0")
    rays = TR.standard_rays()
    n = len(rays)
    full = res.trace_rays(rays, max_events=K, normals=True, ids=True, **named(p))
    rt = torch.from_numpy(rays).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    filled = np.arange(K)[None, :] < full["stored"][:, None]
    for flags in range(4):
        for mask in range(1, 16):
            ev = torch.full((n, K, 8), -1.0, device=dev) if mask & 1 else None
            eid = torch.full((n, K, 4), -7, dtype=torch.int32, device=dev) if mask & 2 else None
            cnt = torch.full((n, 4), -7, dtype=torch.int32, device=dev) if mask & 4 else None
            sp = torch.full((n, 4), -1.0, device=dev) if mask & 8 else None
            ptr = lambda t: t.data_ptr() if t is not None else 0
            res.trace_rays_device(n, rt.data_ptr(), p, K, flags, ptr(ev), ptr(eid), ptr(cnt), ptr(sp), stream=st)
            torch.cuda.synchronize()
            what = (name, flags, mask)
            if ev is not None:
                e = ev.cpu().numpy()
                assert same(e[:, :, 0], full["t"]) and same(e[:, :, 1:4], full["position"]) and same(e[:, :, 7], full["width"]), what
                want = full["normal"] if flags & _ffi.RM_MESH_NORMALS else np.zeros_like(full["normal"])
                assert same(e[:, :, 4:7], want), what
            if eid is not None:
                i = eid.cpu().numpy().view(np.uint32)
                assert np.array_equal(i[:, :, 0], full["kind"]) and np.array_equal(i[:, :, 1], full["step"]), what
                if flags & _ffi.RM_MESH_IDS:
                    assert np.array_equal(i[:, :, 2], full["leaf"]) and np.array_equal(i[:, :, 3], full["material"]), what
                else:
                    assert np.all(i[:, :, 2:] == _ffi.RM_NO_ID), what
            if cnt is not None:
                c4 = cnt.cpu().numpy().view(np.uint32)
                for k, key in enumerate(("events", "steps", "flags", "stored")):
                    assert np.array_equal(c4[:, k], full[key]), (what, key)
            if sp is not None:
                s4 = sp.cpu().numpy()
                for k, key in enumerate(("t_end", "length", "d_start", "d_end")):
                    assert same(s4[:, k], full[key]), (what, key)
    assert filled.any()


EDGES = {
    "t_min equals t_max": (dict(t_min=1.5, t_max=1.5), 8),
    "one step": (dict(max_steps=1), 8),
    "K = 1": (dict(), 1),
    "K = 64": (dict(level=-0.05), 64),
    "step scale 0.5": (dict(step_scale=0.5), 8),
    "two steps": (dict(max_steps=2), 8),
    "negative t_min": (dict(t_min=-3.0, t_max=3.0), 8),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_parameter_edges(res, oracle, edge):
    cc, w = oracle.serialize(*scenes.mat_mix())
    res.set_limits(LIM)
    res.set_program(cc, w)
    extra, K = EDGES[edge]
    p = TR.params(**dict(dict(TR.STANDARD, level=0.0, max_steps=4096), **extra))
    rays = TR.standard_rays()
    got = check(res, cc, w, LIM[1], rays, p, K, what=edge)
    if edge == "t_min equals t_max":             # one evaluation, no event
        assert np.all(got["steps"] == 1) and np.all(got["events"] == 0) and np.all(got["t_end"] == F(1.5)) and np.all(got["length"] == 0)
        assert not (got["flags"] & _ffi.RM_TRACE_OUT_OF_STEPS).any() and np.all(np.isposinf(got["t"]))
    if edge == "one step":
        assert np.all(got["steps"] == 1) and np.all(got["events"] == 0) and np.all((got["flags"] & _ffi.RM_TRACE_OUT_OF_STEPS) != 0)
    if edge == "K = 1":
        assert (got["events"] > 1).any() and got["stored"].max() == 1
    if edge == "K = 64":
        assert np.array_equal(got["stored"], got["events"]) and got["events"].max() > 2


def test_sizes_around_a_wave(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    res.set_limits(LIM)
    res.set_program(cc, w)
    p, K = TR.config("level0")
    rays = TR.standard_rays()
    for n in (1, 65):
        check(res, cc, w, LIM[1], rays[:n], p, K, what="n = %d" % n)
    # n = 0 writes nothing, on either path, whatever the pointers
    guard = np.full((1, 4), 7, np.uint32)
    pa = (C.c_float * 6)(*p)
    assert res._L.rm_trace_rays(res._h, 0, None, pa, 6, K, 0, None, None, guard.ctypes.data, None, 0, None) == _ffi.RM_OK
    assert np.all(guard == 7)
    empty = res.trace_rays(np.zeros((0, 6), F), max_events=K, **named(p))
    assert empty["events"].shape == (0,) and empty["t"].shape == (0, K)


def test_empty_program_and_nan_operands(res, oracle):
    p, K = TR.config("level0")
    rays = TR.standard_rays()
    res.set_limits(LIM)
    res.set_program(0, np.zeros(0, np.uint32))
    got = check(res, 0, np.zeros(0, np.uint32), LIM[1], rays, p, K, what="empty program")
    assert np.all(got["events"] == 0) and np.all(got["d_start"] == F(LIM[1])) and np.all(got["steps"] == 2)
    c = FP.nan_case(oracle)
    res.set_materials(c.table)
    try:
        res.set_limits(c.limits)
        res.set_program(c.cc, c.words)
        both = np.ascontiguousarray(np.concatenate([FP.tie_rays(c), rays[:1500]]))
        pn = TR.params(**dict(TR.STANDARD, level=0.0, max_steps=256))
        got = check(res, c.cc, c.words, c.limits[1], both, pn, K, what="scale by 0")
        assert got["stored"].sum() > 100
        # no finite Lipschitz bound: the wrapper refuses to choose the scale itself
        with pytest.raises(ValueError):
            res.trace_rays(both[:4], max_events=K)
        assert res.trace_rays(both[:4], max_events=K, step_scale=1.0)["events"].shape == (4,)
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
        res.set_limits(LIM)


def test_default_step_scale_is_the_lipschitz_bound(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    res.set_limits(LIM)
    res.set_program(cc, w)
    L = renderer.program_lipschitz(cc, w)
    assert np.isfinite(L)
    scale = F(1.0 / max(1.0, L))
    rays = TR.standard_rays()[:500]
    got = res.trace_rays(rays, t_max=6.0, min_step=0.005, max_events=4)
    p = TR.params(t_max=6.0, min_step=0.005, step_scale=scale)
    compare(got, TR.trace(cc, w, LIM[1], rays, p, 4, normals=False, ids=True), "default scale")


def test_device_path_equals_host_path(res, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    cc, w = oracle.serialize(*scenes.mat_mix())
    res.set_limits(LIM)
    res.set_program(cc, w)
    p, K = TR.config("level0")
    rays = TR.standard_rays()
    host = res.trace_rays(rays, max_events=K, normals=True, ids=True, **named(p))
    t = res.trace_rays(torch.from_numpy(rays).to(dev), max_events=K, normals=True, ids=True, **named(p))
    o = res.trace_rays(torch.from_numpy(rays[:, :3].copy()).to(dev), torch.from_numpy(rays[:, 3:].copy()).to(dev), max_events=K,
                       normals=True, ids=True, **named(p))
    torch.cuda.synchronize()
    for out in (t, o):
        assert out["t"].device == dev
        for k in TR.KEYS:
            g = out[k].cpu().numpy()
            assert same(g.view(np.uint32) if g.dtype == np.int32 else g, host[k]), k
    # the context's own stream
    cnt = torch.full((len(rays), 4), -7, dtype=torch.int32, device=dev)
    res.trace_rays_device(len(rays), torch.from_numpy(rays).to(dev).data_ptr(), p, K, counts_ptr=cnt.data_ptr(), stream=_ffi.RM_STREAM_OWN)
    res.sync_context()
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32)[:, 0], host["events"])


def test_error_statuses_leave_the_outputs_untouched(res, oracle):
    torch = pytest.importorskip("torch")
    L = res._L
    cc, w = oracle.serialize(*scenes.mat_mix())
    res.set_limits(LIM)
    res.set_program(cc, w)
    rays = TR.standard_rays()[:4].copy()
    K = 8
    ev, eid = np.full((4, K, 8), 7, F), np.full((4, K, 4), 7, np.uint32)
    cnt, sp = np.full((4, 4), 7, np.uint32), np.full((4, 4), 7, F)
    good = TR.params()

    def call(n=4, r=rays.ctypes.data, p=good, n_params=6, k=K, flags=3, outs=(ev, eid, cnt, sp)):
        pa = p if p is None else (C.c_float * len(p))(*[float(v) for v in p])
        return L.rm_trace_rays(res._h, n, r, pa, n_params, k, flags, *[o.ctypes.data if o is not None else None for o in outs], 0, None)

    assert call(outs=(None, None, None, None)) == _ffi.RM_ERR_NULL
    assert call(r=None) == _ffi.RM_ERR_NULL
    assert call(p=None) == _ffi.RM_ERR_NULL
    assert call(n_params=5) == _ffi.RM_ERR_ARG and call(n_params=7, p=list(good) + [0.0]) == _ffi.RM_ERR_ARG
    assert call(flags=4) == _ffi.RM_ERR_ARG and call(flags=0x80000001) == _ffi.RM_ERR_ARG
    assert call(k=0) == _ffi.RM_ERR_RANGE and call(k=65) == _ffi.RM_ERR_RANGE
    bad = {"t_min": [np.nan, np.inf, -np.inf, 101.0], "t_max": [np.nan, np.inf, -1.0], "min_step": [0.0, -1.0, np.inf, np.nan],
           "step_scale": [0.0, -0.5, 1.5, np.nan], "level": [np.nan, np.inf], "max_steps": [0.0, 1.5, 65537.0, np.nan, -1.0]}
    for key, values in bad.items():
        for v in values:
            assert call(p=TR.params(**{key: v})) == _ffi.RM_ERR_RANGE, (key, v)
    assert call(p=TR.params(max_steps=65536, t_max=0.0)) == _ffi.RM_OK       # the largest budget is accepted
    for o in (ev, eid, cnt, sp):
        o[...] = 7
    # the statuses of a query for the program and the limits
    res.set_limits((0.01, 100.0, 70000))
    assert call() == _ffi.RM_ERR_RANGE
    res.set_limits(LIM)
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())     # Union on an empty stack
    assert call() == _ffi.RM_ERR_STACK_UNDERFLOW
    with pytest.raises(ValueError):
        res.trace_rays(rays)                         # (the wrapper no longer knows the program: it cannot bound the step)
    res.set_program(cc, w)
    assert np.all(ev == 7) and np.all(eid == 7) and np.all(cnt == 7) and np.all(sp == 7)
    # device arrays off their alignment
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda:0")
    pa = (C.c_float * 6)(*good)
    b = buf.data_ptr()
    for args in ((b + 2, b + 512, None, None, None), (b, b + 512 + 4, None, None, None), (b, None, b + 512 + 8, None, None),
                 (b, None, None, b + 512 + 4, None), (b, None, None, None, b + 512 + 8)):
        assert L.rm_trace_rays(res._h, 1, args[0], pa, 6, 1, 0, args[1], args[2], args[3], args[4], 1, None) == _ffi.RM_ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    assert call() == _ffi.RM_OK and not np.all(cnt == 7)


def test_traversals_leave_the_draw_state_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits(LIM)
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_TIMING, 1)
    keys = (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP, _ffi.RM_INFO_PRUNED)
    try:
        first = res.draw(W, H)
        before = [res.info(k) for k in keys]
        ms = res.info(_ffi.RM_INFO_KERNEL_MS)
        assert ms > 0
        out = res.trace_rays(res.camera_rays(W, H), t_max=20.0, max_events=4, normals=True, ids=True)
        assert out["events"].any()
        assert [res.info(k) for k in keys] == before
        assert res.info(_ffi.RM_INFO_KERNEL_MS) == ms      # the traversal was not timed: nothing new to average
        assert res.draw(W, H).tobytes() == first.tobytes()
    finally:
        res.set_option(_ffi.RM_OPT_TIMING, 0)
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)
