"""Lit rendering on the GPU (rm_set_lighting / rm_draw_lit) against the lighting contract of DESIGN.md section 13: rm_draw
where the contract promises identity, tests/light_ref.py everywhere else.  Every comparison is bit for bit (two NaNs count
as equal) and covers every pixel of the frame it names."""
import ctypes as C

import numpy as np
import pytest

import light_ref
import scenes
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
SIZES = [(64, 48), (61, 37)]      # whole 2 x 2 blocks; odd in both directions


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def same(a, b):
    """Bit-identical, with any two NaNs equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def program(oracle, name):
    if name == "empty":
        return 0, np.zeros(0, dtype=np.uint32)
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    return cc, np.asarray(w, dtype=np.uint32)


def set_light(res, **named):
    """The defaults with the named parameters replaced, on the context; returns the same 13 values for light_ref."""
    full = dict(zip(light_ref.NAMES, light_ref.DEFAULTS))
    p = light_ref.params(**dict(named))
    full.update({k: float(v) for k, v in zip(light_ref.NAMES, p)})
    res.set_lighting(**full)
    assert list(res.lighting().values()) == [float(v) for v in p]
    return p


def setup(res, oracle, name, W, H, lim=None, **light):
    """Program, limits, still camera and lighting on the context -> (uniforms dict, limits, cc, words, materials, params)."""
    cc, w = program(oracle, name)
    lim = lim or scenes.LIMITS.get(name, (0.01, 100.0, 128))
    res.set_output_format(_ffi.RM_FORMAT_RGBA32F)
    res.set_limits(lim)
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    table = scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None
    return ud, lim, cc, w, table, set_light(res, **light)


def reference(ctx, W, H, row0=0, rows=None):
    ud, lim, cc, w, table, p = ctx
    return light_ref.render(ud, lim, cc, w, W, H, row0, rows, materials=table, light=p)[0]


# ---- identity: S = A = 0 is rm_draw ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", sorted(ALL_SCENES) + ["empty"])
def test_identity_equals_the_draw(res, oracle, name, W, H):
    setup(res, oracle, name, W, H, **light_ref.IDENTITY)
    img = res.draw(W, H)
    assert same(res.draw_lit(W, H), img), name
    r0, n = H // 5, H // 3 + 1                       # a row band that starts and ends on odd rows
    assert same(res.draw_lit(W, H, r0, n), img[r0:r0 + n]), name
    assert same(res.draw_lit(W, H, H - 1, 1), img[H - 1:]), name


def test_identity_equals_the_draw_at_1080p(res, oracle):
    W, H = 1920, 1080
    setup(res, oracle, "g32", W, H, **light_ref.IDENTITY)
    assert same(res.draw_lit(W, H), res.draw(W, H))


# ---- lit frames against the contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", sorted(ALL_SCENES) + ["empty"])
def test_defaults_equal_the_contract(res, oracle, name, W, H):
    ctx = setup(res, oracle, name, W, H)
    ref = reference(ctx, W, H)
    got = res.draw_lit(W, H)
    assert same(got, ref), (name, int(np.sum(np.any(got.view(np.uint32) != ref.view(np.uint32), axis=2))))
    r0, n = H // 5, H // 3 + 1
    assert same(res.draw_lit(W, H, r0, n), ref[r0:r0 + n]), name


NON_DEFAULT = dict(pos=(-3.0, -6.0, 1.0), shadow=0.5, ao=0.3, shadow_softness=2.0, shadow_steps=3, bias=0.0)


@pytest.mark.parametrize("taps", [1, 16])
@pytest.mark.parametrize("name", ["g8", "g32", "ext_mix", "xform_mix", "mat_mix"])
def test_non_default_parameters_equal_the_contract(res, oracle, name, taps):
    """A moved light, partial strengths, a wide penumbra, shadow marches that run out after 3 steps, no bias, 1 / 16 taps."""
    W, H = 64, 48
    ctx = setup(res, oracle, name, W, H, ao_taps=taps, **NON_DEFAULT)
    assert same(res.draw_lit(W, H), reference(ctx, W, H)), (name, taps)


@pytest.mark.parametrize("shadow,ao", [(1.0, 0.0), (0.0, 1.0)])
def test_one_term_alone_equals_the_contract(res, oracle, shadow, ao):
    """The kernels of (S > 0, A = 0) and (S = 0, A > 0), on the chain, tree and general loops."""
    W, H = 61, 37
    for name in ("g32", "g32_balanced", "mat_mix"):
        ctx = setup(res, oracle, name, W, H, shadow=shadow, ao=ao)
        assert same(res.draw_lit(W, H), reference(ctx, W, H)), name


@pytest.mark.parametrize("name", ["g8", "mat_mix"])
def test_primary_rays_that_run_out_fall_to_the_floor(res, oracle, name):
    W, H = 64, 48
    ctx = setup(res, oracle, name, W, H, lim=(0.01, 100.0, 6))
    ref = reference(ctx, W, H)
    full = light_ref.render(ctx[0], (0.01, 100.0, 128), ctx[2], ctx[3], W, H, materials=ctx[4], light=ctx[5])[0]
    assert not same(ref, full)                       # 6 steps are too few for part of the frame
    assert same(res.draw_lit(W, H), ref)


def deep_program():
    """8 nested translations around a right-deep union of 32 tagged spheres: a 32-deep value stack, whose leaf walk keeps a
    distance and a (leaf, material) pair per level plus 3 floats per transform level -- more than 64 LDS dwords per lane,
    i.e. more than 64 KB per 256-thread workgroup."""
    rng = np.random.default_rng(21)
    f = lambda *v: [int(x) for x in np.asarray(v, F).view(np.uint32)]   # noqa: E731
    words, cc = [], 0
    for lvl in range(8):
        words += [200] + f(0.04 * lvl, -0.02, 0.03); cc += 1
    for i in range(32):
        words += [0] + f(*rng.uniform(-1.6, 1.6, 3), rng.uniform(0.25, 0.6)) + [300, i % 6]; cc += 2
    words += [100] * 31; cc += 31
    words += [201] * 8; cc += 8
    return cc, np.asarray(words, dtype=np.uint32)


def test_a_program_deeper_than_64_kb_of_lds(res, oracle):
    W, H = 48, 36
    cc, w = deep_program()
    ctx = list(setup(res, oracle, "empty", W, H, lim=(0.01, 100.0, 96)))
    res.set_program(cc, w)
    assert res.info(_ffi.RM_INFO_PROGRAM_DEPTH) == 32 and renderer.program_info(cc, w)["has_xforms"] == 1
    ctx[2:5] = cc, w, scenes.MATERIAL_TABLE
    for light in (light_ref.params(), light_ref.params(**light_ref.IDENTITY)):
        ctx[5] = set_light(res, **dict(zip(light_ref.NAMES, light)))
        assert same(res.draw_lit(W, H), reference(ctx, W, H))


def test_random_pixels_at_1080p(res, oracle):
    W, H = 1920, 1080
    ud, lim, cc, w, table, p = setup(res, oracle, "g32", W, H)
    got = res.draw_lit(W, H)
    rng = np.random.default_rng(1080)
    at = rng.choice(W * H, 2000, replace=False)
    px, py = (at % W).astype(np.uint32), (at // W).astype(np.uint32)
    ref, _ = light_ref.render_pixels(px, py, ud, lim, cc, w, W, H, materials=table, light=p)
    assert same(got[py, px], ref)
    assert not np.isnan(got).any() and np.all(got[..., 3] == 1.0)


# ---- output and ordering ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_eight_bit_formats(res, oracle, W, H):
    ctx = setup(res, oracle, "mat_mix", W, H)
    ref = reference(ctx, W, H)
    try:
        for fmt, bgra in ((_ffi.RM_FORMAT_RGBA8_UNORM, False), (_ffi.RM_FORMAT_BGRA8_UNORM, True)):
            res.set_output_format(fmt)
            got = res.draw_lit(W, H)
            assert got.dtype == np.uint8 and same(got, oracle.quantize_unorm8(ref, bgra=bgra)), fmt
            assert same(res.draw_lit(W, H, 5, 9), oracle.quantize_unorm8(ref[5:14], bgra=bgra)), fmt
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)


def test_device_output_streams_and_program_order(res, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    W, H = 64, 48
    refs = {}
    for name in ("g8", "mat_mix"):
        refs[name] = reference(setup(res, oracle, name, W, H), W, H)
    a = torch.full((H, W, 4), -1.0, dtype=torch.float32, device=dev)
    b = torch.full((H, W, 4), -1.0, dtype=torch.float32, device=dev)
    band = torch.full((11, W, 4), -1.0, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream()
    # one caller stream: program A, lit draw, program B, lit draw -- each draw sees the program set right before it
    res.set_program(*program(oracle, "g8"))
    res.draw_lit_device(W, H, a.data_ptr(), stream=side.cuda_stream)
    res.set_program(*program(oracle, "mat_mix"))
    res.draw_lit_device(W, H, b.data_ptr(), stream=side.cuda_stream)
    # ... and a band on the context's own stream, ordered behind them
    res.draw_lit_device(W, H, band.data_ptr(), row0=7, rows=11, stream=_ffi.RM_STREAM_OWN)
    res.sync_context()
    side.synchronize()
    torch.cuda.synchronize()
    assert same(a.cpu().numpy(), refs["g8"]) and same(b.cpu().numpy(), refs["mat_mix"])
    assert same(band.cpu().numpy(), refs["mat_mix"][7:18])
    # the null stream, 8-bit pixels
    res.set_output_format(_ffi.RM_FORMAT_RGBA8_UNORM)
    try:
        q = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        res.draw_lit_device(W, H, q.data_ptr())
        torch.cuda.synchronize()
        assert same(q.cpu().numpy(), oracle.quantize_unorm8(refs["mat_mix"]))
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)


# ---- isolation from the draw state --------------------------------------------------------------------------------------------
def test_lit_draws_leave_the_draw_state_alone(res, oracle):
    W, H = 64, 48
    setup(res, oracle, "g32", W, H, lim=(0.01, 100.0, 128))
    keys = (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP, _ffi.RM_INFO_PRUNED)
    try:
        for spec in (0, 2):                          # the interpreter kernel (its loop is reported), then the specialised one
            res.set_option(_ffi.RM_OPT_SPECIALIZE, spec)
            res.set_option(_ffi.RM_OPT_TIMING, 1)
            first = res.draw(W, H)
            before = [res.info(k) for k in keys]
            ms = res.info(_ffi.RM_INFO_KERNEL_MS)
            assert ms > 0
            lit = res.draw_lit(W, H)
            res.draw_lit(W, H, 3, 17)
            set_light(res, **light_ref.IDENTITY)
            assert same(res.draw_lit(W, H), first)
            set_light(res)
            assert [res.info(k) for k in keys] == before
            assert res.info(_ffi.RM_INFO_KERNEL_MS) == ms          # the lit draws were not timed: nothing new to average
            assert res.draw(W, H).tobytes() == first.tobytes()
            assert same(res.draw_lit(W, H), lit)
    finally:
        res.set_option(_ffi.RM_OPT_TIMING, 0)
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)


# ---- errors -------------------------------------------------------------------------------------------------------------------
OUT_OF_RANGE = [("pos_x", np.inf), ("pos_y", np.nan), ("pos_z", -np.inf), ("shadow", -0.1), ("shadow", 1.5), ("shadow", np.nan),
                ("shadow_softness", 0.0), ("shadow_softness", -1.0), ("bias", -0.001), ("shadow_max_t", 0.0),
                ("shadow_steps", 0.0), ("shadow_steps", 1025.0), ("shadow_steps", 2.5), ("ao", -0.5), ("ao", 1.01),
                ("ao_step", 0.0), ("ao_falloff", 0.0), ("ao_falloff", 1.25), ("ao_scale", -1.0), ("ao_taps", 0.0),
                ("ao_taps", 17.0), ("ao_taps", 4.5), ("ao_taps", np.nan)]


def test_errors(res, oracle):
    L = res._L
    W, H = 64, 48
    setup(res, oracle, "mat_mix", W, H, shadow=0.75, ao_taps=3)
    frame = res.draw_lit(W, H)
    good = [float(v) for v in light_ref.params(shadow=0.75, ao_taps=3)]
    for key, value in OUT_OF_RANGE:
        p = list(good)
        p[light_ref.NAMES.index(key)] = value
        assert L.rm_set_lighting(res._h, (C.c_float * 13)(*p), 13) == _ffi.RM_ERR_RANGE, (key, value)
        with pytest.raises(_ffi.RmError) as e:
            res.set_lighting(**{key: value})
        assert e.value.status == _ffi.RM_ERR_RANGE and res.lighting()[key] == good[light_ref.NAMES.index(key)]
    assert same(res.draw_lit(W, H), frame)           # the failed calls changed nothing
    arr = (C.c_float * 16)(*(good + [0.0] * 3))
    for count in (0, 12, 14, 16):
        assert L.rm_set_lighting(res._h, arr, count) == _ffi.RM_ERR_ARG, count
    assert L.rm_set_lighting(res._h, None, 13) == _ffi.RM_ERR_NULL
    assert L.rm_set_lighting(None, arr, 13) == _ffi.RM_ERR_NULL
    out = np.zeros((H, W, 4), F)
    assert L.rm_draw_lit(res._h, W, H, 0, H, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_draw_lit(None, W, H, 0, H, out.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
    for args in ((W, H, H, 1), (W, H, 0, H + 1), (W, H, 0, 0), (0, H, 0, H), (70000, H, 0, H)):
        assert L.rm_draw_lit(res._h, *args, out.ctypes.data, 0, None) == _ffi.RM_ERR_RANGE, args
    assert same(res.draw_lit(W, H), frame)
    with pytest.raises(ValueError):
        res.set_lighting(brightness=2.0)
    res.set_materials(scenes.MATERIAL_TABLE[:2])     # mat_mix tags up to 5
    try:
        assert L.rm_draw_lit(res._h, W, H, 0, H, out.ctypes.data, 0, None) == _ffi.RM_ERR_MATERIAL
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
    res.set_limits((0.01, 100.0, 65537))
    assert L.rm_draw_lit(res._h, W, H, 0, H, out.ctypes.data, 0, None) == _ffi.RM_ERR_RANGE
    res.set_limits((0.01, 100.0, 128))
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    assert L.rm_draw_lit(res._h, W, H, 0, H, out.ctypes.data, 0, None) == _ffi.RM_ERR_STACK_UNDERFLOW
    res.set_program(*program(oracle, "mat_mix"))
    assert same(res.draw_lit(W, H), frame)


# ---- the offline orbit renderer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "ppm"])
def test_orbit_batch_lit_frames(tmp_path, oracle, fmt):
    """python -m ray_marching_amd.orbit_batch --lit: every frame is draw_lit of its camera, and the contract's frame."""
    pytest.importorskip("torch")
    from ray_marching_amd import camera, csg, orbit_batch
    a = orbit_batch.parse(["--out-dir", str(tmp_path / "lit"), "--frames", "3", "--width", "64", "--height", "40", "--scene", "g8",
                           "--max-iter", "64", "--format", fmt, "--slots", "2", "--writers", "1",
                           "--lit", "--shadow", "0.8", "--ao", "0.6", "--light", "1.5", "-4", "2"])
    s = orbit_batch.render_batch(a, rank=0, world=1, device=0)
    assert s["frames_rendered"] == 3
    W, H = a.width, a.height
    r = renderer.RayMarchingResources(0)
    try:
        r.set_limits((0.01, 100.0, a.max_iter))
        cc, w = csg.serialize(csg.scene("g8"))
        r.set_program(cc, w)
        p = set_light(r, pos=(1.5, -4.0, 2.0), shadow=0.8, ao=0.6)
        ctl = camera.OrbitCameraController.new([0.0, 0.0, 0.0], 5.0)
        for f in range(a.frames):
            ctl.set_angles(orbit_batch.orbit_yaw(f, a.frames), -0.25, 5.0)
            u = renderer.prepare_uniforms((float(W), float(H)), ctl.camera())
            r.set_uniforms(u)
            img = r.draw_lit(W, H)
            ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
            assert same(img, light_ref.render(ud, (0.01, 100.0, a.max_iter), cc, w, W, H, light=p)[0]), f
            data = open(orbit_batch.frame_path(a.out_dir, f, fmt), "rb").read()
            if fmt == "f32":
                assert data == img.tobytes(), f
            else:
                assert data[len(orbit_batch.ppm_header(W, H)):] == oracle.quantize_unorm8(img)[..., :3].tobytes(), f
            assert not same(img, r.draw(W, H))       # the frames are lit
    finally:
        r.close()
    assert orbit_batch.render_batch(a, rank=0, world=1, device=0)["frames_skipped"] == 3     # resumes
