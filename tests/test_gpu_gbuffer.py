"""The G-buffer draw on the GPU (rm_draw_gbuffer) against the contract of DESIGN.md section 14: the composition of
rm_camera_rays + rm_cast_rays per sample, reduced in numpy by section 14's rule, and tests/gbuffer_ref.py (numpy on the
oracle).  Every comparison is bit for bit (two NaNs count as equal) and covers all twelve named arrays of every pixel."""
import numpy as np
import pytest

import gbuffer_ref
import scenes
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
COMPOSED = ["g1", "g8", "g32", "g32_balanced", "g8x", "g32s", "ext_mix", "xform_mix", "mat_mix"]
FORMS = [_ffi.RM_SAMPLE_ALL, _ffi.RM_SAMPLE_CENTER, 9]
KEYS = gbuffer_ref.KEYS
BINARY = (100, 101, 102, 110)


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


def assert_same(got, want, what=""):
    assert tuple(got) == KEYS and tuple(want) == KEYS
    for k in KEYS:
        assert same(got[k], want[k]), (what, k)


def program(oracle, name):
    if name == "empty":
        return 0, np.zeros(0, dtype=np.uint32)
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    return cc, np.asarray(w, dtype=np.uint32)


def setup(res, oracle, name, W, H, lim=None):
    """Program, limits and the still camera on the context -> (uniforms dict, limits, cc, words)."""
    cc, w = program(oracle, name)
    lim = lim or scenes.LIMITS.get(name, (0.01, 100.0, 128))
    res.set_limits(lim)
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    return ud, lim, cc, w


def left_operand(cc, w):
    """The selection the composition tests use: the range of the root's left operand (the root itself when it is no
    binary operator), from rm_program_subtree."""
    if cc == 0:
        return (0, 0)
    first, count = renderer.program_subtree(cc, w, cc - 1)
    assert (first, count) == (0, cc)
    q = 0
    for _ in range(cc - 1):
        q += 1 + gbuffer_ref.NPARAM[int(w[q])]
    if int(w[q]) not in BINARY:
        return (0, cc)
    right_first, _ = renderer.program_subtree(cc, w, cc - 2)         # the command before the root ends its right operand
    sel = renderer.program_subtree(cc, w, right_first - 1)
    assert sel == (0, right_first)
    return sel


def cast_records(res, W, H, row0, rows, ids):
    """What the parent's entry points give: per sample, rm_camera_rays + rm_cast_rays over the band."""
    for s in ids:
        hit = res.cast_rays(res.camera_rays(W, H, 0, row0, W, rows, sample=s))
        rec = np.concatenate([hit["t"][:, None], hit["position"], hit["normal"], hit["diffuse"][:, None]], axis=1)
        yield {"kind": hit["kind"], "steps": hit["steps"], "leaf": hit["leaf"], "material": hit["material"],
               "hit": np.ascontiguousarray(rec, dtype=F)}


def composed(res, W, H, sample, select=None, row0=0, rows=None):
    rows = H - row0 if rows is None else rows
    ids = gbuffer_ref.sample_ids(sample)
    out = gbuffer_ref.reduce(cast_records(res, W, H, row0, rows, ids), ids, select)
    return {k: v.reshape((rows, W) + v.shape[1:]) for k, v in out.items()}


# ---- against the composition of rm_camera_rays and rm_cast_rays ----------------------------------------------------------------
@pytest.mark.parametrize("sample", FORMS)
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
@pytest.mark.parametrize("name", COMPOSED)
def test_equals_the_composition_of_camera_rays_and_cast_rays(res, oracle, name, W, H, sample):
    _, _, cc, w = setup(res, oracle, name, W, H)
    sel = left_operand(cc, w)
    got = res.draw_gbuffer(W, H, sample=sample, select=sel)
    assert_same(got, composed(res, W, H, sample, sel), (name, W, H, sample))
    assert got["surface_mask"].any() and (name == "g1" or sel[1] < cc)


# ---- against the numpy statement of section 14 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32", "xform_mix", "mat_mix"])
def test_equals_the_reference(res, oracle, name):
    W, H = 64, 48
    ud, lim, cc, w = setup(res, oracle, name, W, H, lim=(0.01, 100.0, 128))
    sel = (0, cc // 2)                                # the first half of the command stream
    want, records = gbuffer_ref.render(ud, lim, cc, w, W, H, select=sel, detail=True)
    # these inputs exercise the reduction: pixels whose samples disagree
    full = np.uint32(0xFFFF)
    partial_surface = (want["surface_mask"] != 0) & (want["surface_mask"] != full)
    partial_selected = (want["selected_mask"] != 0) & (want["selected_mask"] != want["surface_mask"])
    leaves = np.stack([np.where(r["kind"] == _ffi.RM_HIT_SURFACE, r["leaf"], _ffi.RM_NO_ID) for r in records]).astype(np.int64)
    lo = np.where(leaves == _ffi.RM_NO_ID, 1 << 40, leaves).min(axis=0)
    hi = np.where(leaves == _ffi.RM_NO_ID, -1, leaves).max(axis=0)
    several_leaves = (hi >= 0) & (lo != hi)
    print("%s: partial surface %d, several leaves %d, partially selected %d" % (
        name, partial_surface.sum(), several_leaves.sum(), partial_selected.sum()))
    assert partial_surface.any() and several_leaves.any() and partial_selected.any()
    assert_same(res.draw_gbuffer(W, H, select=sel), want, name)
    for sample in (_ffi.RM_SAMPLE_CENTER, 9):
        assert_same(res.draw_gbuffer(W, H, sample=sample, select=sel),
                    gbuffer_ref.render(ud, lim, cc, w, W, H, sample=sample, select=sel), (name, sample))


# ---- selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32", "mat_mix"])
def test_selection_edge_cases(res, oracle, name):
    W, H = 64, 48
    _, _, cc, w = setup(res, oracle, name, W, H)
    whole = res.draw_gbuffer(W, H, select=(0, cc))
    assert same(whole["selected_mask"], whole["surface_mask"]) and whole["surface_mask"].any()
    none = res.draw_gbuffer(W, H, select=(0, 0))
    assert not none["selected_mask"].any() and not res.draw_gbuffer(W, H, select=(cc, 0))["selected_mask"].any()
    assert not res.draw_gbuffer(W, H)["selected_mask"].any()
    for k in KEYS:
        if k != "selected_mask":
            assert same(whole[k], none[k]), k      # the selection changes nothing else
    # a single primitive: exactly the samples whose leaf is that primitive
    per_sample = list(cast_records(res, W, H, 0, H, range(16)))
    seen = np.unique(np.concatenate([r["leaf"][r["kind"] == _ffi.RM_HIT_SURFACE] for r in per_sample]))
    assert len(seen) >= 3
    for prim in (int(seen[0]), int(seen[len(seen) // 2]), int(seen[-1])):
        assert renderer.program_subtree(cc, w, prim) == (prim, 1)
        want = np.zeros(W * H, dtype=np.uint32)
        for s, r in enumerate(per_sample):
            want |= np.where((r["kind"] == _ffi.RM_HIT_SURFACE) & (r["leaf"] == prim), np.uint32(1 << s), np.uint32(0))
        got = res.draw_gbuffer(W, H, select=(prim, 1))["selected_mask"]
        assert want.any() and same(got, want.reshape(H, W)), prim


# ---- bands and sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [_ffi.RM_SAMPLE_ALL, _ffi.RM_SAMPLE_CENTER])
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29), (61, 37), (1, 1), (3, 70)])
def test_row_bands_and_odd_sizes(res, oracle, W, H, sample):
    _, _, cc, w = setup(res, oracle, "mat_mix", W, H)
    sel = left_operand(cc, w)
    full = res.draw_gbuffer(W, H, sample=sample, select=sel)
    assert_same(full, composed(res, W, H, sample, sel), (W, H))
    for row0, rows in ((0, 1), (5, 9), (H - 3, 3), (7, 2), (H - 1, 1), (1, H - 1)):
        if row0 < 0 or rows < 1 or row0 + rows > H:
            continue
        band = res.draw_gbuffer(W, H, row0, rows, sample=sample, select=sel)
        for k in KEYS:
            assert same(band[k], full[k][row0:row0 + rows]), (W, H, row0, rows, k)


def test_a_1080p_frame_equals_the_sixteen_casts(res, oracle):
    W, H = 1920, 1080
    _, _, cc, w = setup(res, oracle, "g32", W, H)
    sel = left_operand(cc, w)
    got = res.draw_gbuffer(W, H, select=sel)
    assert_same(got, composed(res, W, H, _ffi.RM_SAMPLE_ALL, sel), "1080p")
    assert not np.isnan(got["t"]).any()


# ---- output handling -----------------------------------------------------------------------------------------------------------
def device_draw(res, torch, W, H, mask, stream, row0=0, rows=None, sample=_ffi.RM_SAMPLE_ALL, select=None):
    """A device-destination draw of the outputs named by `mask` (1 geom, 2 ids, 4 masks) -> the tensors (None: not asked)."""
    rows = H - row0 if rows is None else rows
    dev = torch.device("cuda", 0)
    geom = torch.full((rows, W, 8), -1.0, dtype=torch.float32, device=dev) if mask & 1 else None
    ids = torch.full((rows, W, 4), -7, dtype=torch.int32, device=dev) if mask & 2 else None
    masks = torch.full((rows, W, 4), -7, dtype=torch.int32, device=dev) if mask & 4 else None
    res.draw_gbuffer_device(W, H, geom.data_ptr() if mask & 1 else 0, ids.data_ptr() if mask & 2 else 0,
                            masks.data_ptr() if mask & 4 else 0, row0, rows, sample, select, stream)
    return geom, ids, masks


def check_device(torch, tensors, want, what):
    geom, ids, masks = tensors
    torch.cuda.synchronize()
    if geom is not None:
        g = geom.cpu().numpy()
        for k, part in (("t", g[..., 0]), ("position", g[..., 1:4]), ("normal", g[..., 4:7]), ("diffuse", g[..., 7])):
            assert same(part, want[k]), (what, k)
    if ids is not None:
        i = ids.cpu().numpy().view(np.uint32)
        for n, k in enumerate(("kind", "sample", "leaf", "material")):
            assert same(i[..., n], want[k]), (what, k)
    if masks is not None:
        m = masks.cpu().numpy().view(np.uint32)
        for n, k in enumerate(("surface_mask", "floor_mask", "selected_mask", "steps")):
            assert same(m[..., n], want[k]), (what, k)


@pytest.mark.parametrize("name", ["g32", "g32_balanced", "mat_mix"])   # chain, tree and general loop
def test_every_output_combination(res, oracle, name):
    """Each subset of the outputs, on device memory, holds the bytes of the full draw: whether the taps or the walk run
    changes nothing in what the other outputs receive."""
    torch = pytest.importorskip("torch")
    W, H = 61, 37
    _, _, cc, w = setup(res, oracle, name, W, H, lim=(0.01, 100.0, 96))
    st = torch.cuda.current_stream().cuda_stream
    for sample in (_ffi.RM_SAMPLE_ALL, 9):
        for sel in (left_operand(cc, w), (0, 0)):        # (0, 0): with the ids not asked for either, no walk at all
            want = res.draw_gbuffer(W, H, sample=sample, select=sel)
            for mask in range(1, 8):
                check_device(torch, device_draw(res, torch, W, H, mask, st, sample=sample, select=sel), want, (name, sample, sel, mask))
    # the host path, one output at a time
    want = res.draw_gbuffer(W, H, select=(0, cc))
    n = W * H
    geom, ids, masks = np.empty((n, 8), F), np.empty((n, 4), np.uint32), np.empty((n, 4), np.uint32)
    L, h = res._L, res._h
    assert L.rm_draw_gbuffer(h, W, H, 0, H, _ffi.RM_SAMPLE_ALL, 0, cc, geom.ctypes.data, None, None, 0, None) == _ffi.RM_OK
    assert L.rm_draw_gbuffer(h, W, H, 0, H, _ffi.RM_SAMPLE_ALL, 0, cc, None, ids.ctypes.data, None, 0, None) == _ffi.RM_OK
    assert L.rm_draw_gbuffer(h, W, H, 0, H, _ffi.RM_SAMPLE_ALL, 0, cc, None, None, masks.ctypes.data, 0, None) == _ffi.RM_OK
    assert same(geom[:, 0].reshape(H, W), want["t"]) and same(geom[:, 4:7].reshape(H, W, 3), want["normal"])
    assert same(ids[:, 2].reshape(H, W), want["leaf"]) and same(masks[:, 2].reshape(H, W), want["selected_mask"])


def test_device_output_streams_and_program_order(res, oracle):
    torch = pytest.importorskip("torch")
    W, H = 64, 48
    wants = {}
    for name in ("g8", "mat_mix"):
        _, _, cc, w = setup(res, oracle, name, W, H)
        wants[name] = res.draw_gbuffer(W, H, select=(0, cc // 2))
        wants[name, "band"] = res.draw_gbuffer(W, H, 7, 11, sample=_ffi.RM_SAMPLE_CENTER, select=(0, cc // 2))
    side = torch.cuda.Stream()
    # one caller stream: program A, draw, program B, draw -- each draw sees the program set right before it
    ca, wa = program(oracle, "g8")
    cb, wb = program(oracle, "mat_mix")
    res.set_program(ca, wa)
    a = device_draw(res, torch, W, H, 7, side.cuda_stream, select=(0, ca // 2))
    res.set_program(cb, wb)
    b = device_draw(res, torch, W, H, 7, side.cuda_stream, select=(0, cb // 2))
    # ... and a band on the context's own stream, ordered behind them
    band = device_draw(res, torch, W, H, 7, _ffi.RM_STREAM_OWN, 7, 11, _ffi.RM_SAMPLE_CENTER, (0, cb // 2))
    res.sync_context()
    side.synchronize()
    check_device(torch, a, wants["g8"], "A")
    check_device(torch, b, wants["mat_mix"], "B")
    check_device(torch, band, wants["mat_mix", "band"], "band")
    check_device(torch, device_draw(res, torch, W, H, 7, None, select=(0, cb // 2)), wants["mat_mix"], "null stream")
    # misaligned device arrays: RM_ERR_ARG, nothing launched
    buf = torch.zeros(W * H * 8 + 64, dtype=torch.float32, device=torch.device("cuda", 0))
    L, h, p = res._L, res._h, buf.data_ptr()
    for args in ((p + 4, None, None), (None, p + 8, None), (None, None, p + 12), (p, p + 16 * W * H * 2, p + 4)):
        assert L.rm_draw_gbuffer(h, W, H, 0, 1, _ffi.RM_SAMPLE_ALL, 0, 0, *args, 1, None) == _ffi.RM_ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


def test_errors_and_empty_calls(res, oracle):
    W, H = 16, 12
    _, _, cc, w = setup(res, oracle, "mat_mix", W, H)
    L, h = res._L, res._h
    n = W * H
    geom, ids, masks = np.full((n, 8), -1, F), np.full((n, 4), 7, np.uint32), np.full((n, 4), 7, np.uint32)
    outs = (geom.ctypes.data, ids.ctypes.data, masks.ctypes.data)
    ALL = _ffi.RM_SAMPLE_ALL
    assert L.rm_draw_gbuffer(None, W, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, 0, 0, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_draw_gbuffer(h, W, H, 0, 0, ALL, 0, 0, *outs, 0, None) == _ffi.RM_OK            # W * rows = 0: nothing written
    assert L.rm_draw_gbuffer(h, 0, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_OK
    assert np.all(geom == -1) and np.all(ids == 7) and np.all(masks == 7)
    for band in ((H, 1), (0, H + 1), (H - 1, 2), (0xFFFFFFFF, 2)):
        assert L.rm_draw_gbuffer(h, W, H, *band, ALL, 0, 0, *outs, 0, None) == _ffi.RM_ERR_RANGE, band
    assert L.rm_draw_gbuffer(h, 70000, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_ERR_RANGE
    for sample in (18, 255, 0xFFFFFFFF):
        assert L.rm_draw_gbuffer(h, W, H, 0, H, sample, 0, 0, *outs, 0, None) == _ffi.RM_ERR_ARG, sample
    for sel in ((0, cc + 1), (cc, 1), (cc + 1, 0), (0xFFFFFFFF, 2), (1, 0xFFFFFFFF)):
        assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, *sel, *outs, 0, None) == _ffi.RM_ERR_ARG, sel
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, cc, 0, *outs, 0, None) == _ffi.RM_OK
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, cc - 1, 1, *outs, 0, None) == _ffi.RM_OK
    with pytest.raises(_ffi.RmError) as e:
        res.draw_gbuffer(W, H, select=(0, cc + 1))
    assert e.value.status == _ffi.RM_ERR_ARG
    res.set_limits((0.01, 100.0, 70000))
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_ERR_RANGE
    res.set_limits((0.01, 100.0, 128))
    res.set_materials(scenes.MATERIAL_TABLE[:2])   # mat_mix tags up to 5: no colour is asked for, so the draw works
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_OK
    res.set_materials(scenes.MATERIAL_TABLE)
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    assert L.rm_draw_gbuffer(h, W, H, 0, H, ALL, 0, 0, *outs, 0, None) == _ffi.RM_ERR_STACK_UNDERFLOW
    res.set_program(cc, w)


@pytest.mark.parametrize("sample", FORMS)
def test_an_empty_program_gives_floor_and_sky(res, oracle, sample):
    W, H = 40, 24
    ud, lim, cc, w = setup(res, oracle, "empty", W, H, lim=(0.01, 100.0, 64))
    got = res.draw_gbuffer(W, H, sample=sample)
    assert_same(got, gbuffer_ref.render(ud, lim, cc, w, W, H, sample=sample), sample)
    assert_same(got, composed(res, W, H, sample), sample)
    n = len(gbuffer_ref.sample_ids(sample))
    assert not got["surface_mask"].any() and not got["selected_mask"].any() and np.all(got["steps"] == 64 * n)
    assert got["floor_mask"].any() and (got["floor_mask"] == 0).any()
    assert set(np.unique(got["kind"])) == {_ffi.RM_HIT_NONE, _ffi.RM_HIT_FLOOR} and np.all(got["leaf"] == _ffi.RM_NO_ID)
    assert L_status(res, W, H, (0, 1)) == _ffi.RM_ERR_ARG     # nothing to select in an empty program


def L_status(res, W, H, sel):
    out = np.empty((W * H, 4), np.uint32)
    return res._L.rm_draw_gbuffer(res._h, W, H, 0, H, _ffi.RM_SAMPLE_ALL, sel[0], sel[1], None, None, out.ctypes.data, 0, None)


# ---- large programs ------------------------------------------------------------------------------------------------------------
def test_a_program_deeper_than_64_kb_of_lds(res, oracle):
    from test_gpu_lit import deep_program          # 8 transforms around a right-deep union of 32 tagged spheres
    W, H = 48, 36
    cc, w = deep_program()
    ud, lim, _, _ = setup(res, oracle, "empty", W, H, lim=(0.01, 100.0, 96))
    res.set_program(cc, w)
    assert res.info(_ffi.RM_INFO_PROGRAM_DEPTH) == 32 and renderer.program_info(cc, w)["has_xforms"] == 1
    sel = renderer.program_subtree(cc, w, 72 + 10)       # the union that spans the last 12 tagged spheres
    assert sel == (8 + 2 * 20, 2 * 12 + 11)
    for sample in FORMS:
        got = res.draw_gbuffer(W, H, sample=sample, select=sel)
        assert_same(got, composed(res, W, H, sample, sel), sample)
        assert got["surface_mask"].any()
    got = res.draw_gbuffer(W, H, select=sel)
    assert_same(got, gbuffer_ref.render(ud, lim, cc, w, W, H, select=sel), "deep")
    part = (got["selected_mask"] != 0) & (got["selected_mask"] != got["surface_mask"])
    assert part.any()


def lattice_program():
    """Nearly fills the 64 KB command buffer: a left-deep union of 2000 tagged spheres on a 20 x 10 x 10 lattice (16000 words;
    command indices up to 5998, i.e. leaves far beyond 8 bits)."""
    f = lambda *v: [int(x) for x in np.asarray(v, F).view(np.uint32)]   # noqa: E731
    words, cc, k = [], 0, 0
    for x in np.linspace(-2.4, 2.4, 20):
        for y in np.linspace(-1.0, 1.0, 10):
            for z in np.linspace(-1.2, 1.2, 10):
                words += [0] + f(x, y, z, 0.09) + [300, k % 6]
                cc += 2
                if k:
                    words += [100]
                    cc += 1
                k += 1
    return cc, np.asarray(words, dtype=np.uint32)


def test_a_program_in_a_grown_command_buffer(res, oracle):
    W, H = 48, 36
    cc, w = lattice_program()
    assert len(w) > 15900 and renderer.validate_program(cc, w)[0] == _ffi.RM_OK
    setup(res, oracle, "empty", W, H, lim=(0.01, 100.0, 64))
    res.set_program(cc, w)
    sel = (cc // 3, cc // 3)
    for sample in (_ffi.RM_SAMPLE_ALL, _ffi.RM_SAMPLE_CENTER):
        got = res.draw_gbuffer(W, H, sample=sample, select=sel)
        assert_same(got, composed(res, W, H, sample, sel), sample)
        leaves = np.unique(got["leaf"][got["kind"] == _ffi.RM_HIT_SURFACE])
        assert len(leaves) > 50 and leaves.max() > 4000 and got["selected_mask"].any()
        assert (got["selected_mask"] != got["surface_mask"]).any()


# ---- isolation from the draw state ---------------------------------------------------------------------------------------------
def test_gbuffer_draws_leave_the_draw_state_alone(res, oracle):
    W, H = 64, 48
    _, _, cc, w = setup(res, oracle, "g32", W, H, lim=(0.01, 100.0, 128))
    keys = (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP, _ffi.RM_INFO_PRUNED)
    try:
        for spec in (0, 2):                          # the interpreter kernel (its loop is reported), then the specialised one
            res.set_option(_ffi.RM_OPT_SPECIALIZE, spec)
            res.set_option(_ffi.RM_OPT_TIMING, 1)
            first = res.draw(W, H)
            before = [res.info(k) for k in keys]
            ms = res.info(_ffi.RM_INFO_KERNEL_MS)
            assert ms > 0
            g = res.draw_gbuffer(W, H, select=(0, cc // 2))
            res.draw_gbuffer(W, H, 3, 17, sample=_ffi.RM_SAMPLE_CENTER)
            assert [res.info(k) for k in keys] == before
            assert res.info(_ffi.RM_INFO_KERNEL_MS) == ms          # the G-buffer draws were not timed: nothing new to average
            assert res.draw(W, H).tobytes() == first.tobytes()
            assert [res.info(k) for k in keys] == before
            assert_same(res.draw_gbuffer(W, H, select=(0, cc // 2)), g, spec)
            # the frame and its G-buffer agree: a pixel is black exactly where no sample hit anything
            assert np.array_equal(np.all(first[..., :3] == 0, axis=-1), (g["surface_mask"] | g["floor_mask"]) == 0)
    finally:
        res.set_option(_ffi.RM_OPT_TIMING, 0)
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)


def test_gbuffer_draw_is_stream_capturable(oracle):
    """After its first call, a device-destination rm_draw_gbuffer issues nothing but its kernel launch on the caller's
    stream: it can be captured into a HIP graph and replayed."""
    torch = pytest.importorskip("torch")
    W, H = 96, 64
    r = renderer.RayMarchingResources(0)
    try:
        r.set_materials(scenes.MATERIAL_TABLE)
        _, _, cc, w = setup(r, oracle, "mat_mix", W, H, lim=(0.01, 100.0, 96))
        sel = (0, cc // 2)
        want = r.draw_gbuffer(W, H, select=sel)
        s = torch.cuda.Stream()
        outs = device_draw(r, torch, W, H, 7, s.cuda_stream, select=sel)      # warm: the program and its query form are uploaded
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            r.draw_gbuffer_device(W, H, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), select=sel, stream=s.cuda_stream)
            g.capture_end()
        for _ in range(3):
            for t in outs:
                t.zero_()
            g.replay()
            check_device(torch, outs, want, "replay")
    finally:
        r.close()
