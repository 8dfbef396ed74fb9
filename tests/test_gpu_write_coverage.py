"""Every draw writes all of its pixels and nothing else ("Write coverage").

The host path of a draw (out_is_device = 0) renders into the context's staging buffer, which survives from one draw to the
next: a pixel a draw fails to write comes back holding what the previous draw left there -- usually the right value, since
the suites draw the same frames over and over.  Here every case draws through the DEVICE path into sentinel-filled memory with
guard rows in front and behind (tests/write_coverage.py; tests/test_write_coverage_cpu.py shows that its check fails when it
should) and compares with the oracle's frame bit for bit: rmo_render, rmo_quantize_unorm8 for the 8-bit formats,
tests/light_ref.py for the lit draws.  The one exception is test_host_path_returns_this_draws_pixels, whose subject is the
staging buffer itself.

Oracle frames are computed once per (scene, camera, size, limits) and shared; a band's reference is a slice of the whole
frame's (the oracle works pixel by pixel)."""
import numpy as np
import pytest

import gbuffer_ref
import light_ref
import scenes
import write_coverage as WC
from ray_marching_amd import _ffi, renderer, shard

pytestmark = pytest.mark.gpu

F32, RGBA8, BGRA8 = _ffi.RM_FORMAT_RGBA32F, _ffi.RM_FORMAT_RGBA8_UNORM, _ffi.RM_FORMAT_BGRA8_UNORM
V5, V5_LDS, PIXEL = _ffi.RM_KERNEL_V5, _ffi.RM_KERNEL_V5_LDS, _ffi.RM_KERNEL_PIXEL
# a kernel as the tests name it: (RM_OPT_KERNEL, RM_OPT_SPECIALIZE, RM_OPT_PRUNE) -- those of test_miss_ray_culling_is_exact
KERNELS = {"v5": (V5, 0, 0), "v5_lds": (V5_LDS, 0, 0), "v5_spec": (V5_LDS, 2, 0), "v5_spec_prune": (V5_LDS, 2, 1), "pixel": (PIXEL, 0, 0)}
V5_KERNELS = ["v5", "v5_lds", "v5_spec", "v5_spec_prune"]

SIZES = [(1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (17, 65), (65, 17), (72, 48)]
FORMAT_SIZES = [(17, 65), (72, 48)]
LIM = (0.01, 100.0, 32)

# orbit events (1, dx, dy) turn the camera about the scene.  A is the suite's still camera; B looks from the far side and
# from higher up, so that other tiles are sky, floor and object (asserted on the oracle's frames in test_second_draw...);
# the rest are the frames of a batch.
CAMS = {"A": scenes.STILL_CAMERA_EVENTS, "B": [(1, 420.0, -110.0)], "C": [(1, 150.0, 40.0)], "D": [(1, -200.0, -60.0)],
        "E": [(1, 35.0, -25.0), (2, -40.0, 0.0)]}


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _defaults_afterwards(res):
    yield
    configure(res)
    res.set_materials([(0.4, 0.7, 0.1)])


def configure(res, kernel="v5_spec", cull=1, balance=3, wpt=0, fmt=F32, stats=0):
    k, spec, prune = KERNELS[kernel]
    for key, value in ((_ffi.RM_OPT_KERNEL, k), (_ffi.RM_OPT_SPECIALIZE, spec), (_ffi.RM_OPT_PRUNE, prune), (_ffi.RM_OPT_CULL, cull),
                       (_ffi.RM_OPT_BALANCE, balance), (_ffi.RM_OPT_WAVES_PER_TILE, wpt), (_ffi.RM_OPT_WAVE_STATS, stats)):
        res.set_option(key, value)
    res.set_output_format(fmt)


# ---- scenes, cameras, references ------------------------------------------------------------------------------------------------
def big_box():
    """The camera of every CAMS entry sits inside it: no ray can be cleared, every sample hits at its first step."""
    t = scenes._Tab()
    return t.nodes, t.box((0.0, 0.0, 0.0), (50.0, 50.0, 50.0))


PROGRAMS = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()) + [("big_box", big_box)])
_CACHE = {}


def program(oracle, name):
    if name == "empty":
        return 0, np.zeros(0, dtype=np.uint32)
    if ("prog", name) not in _CACHE:
        cc, w = oracle.serialize(*PROGRAMS[name]())
        _CACHE["prog", name] = (cc, np.asarray(w, dtype=np.uint32))
    return _CACHE["prog", name]


def camera(oracle, cam, W, H):
    return oracle.orbit_uniforms((float(W), float(H)), events=CAMS[cam])[0]


def ffi_u(u):
    return _ffi.Uniforms.from_buffer_copy(bytes(u))


def udict(u):
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


def frame(oracle, scene, cam, W, H, lim=LIM, fmt=F32):
    """The oracle's whole frame, read-only, in the pixel format `fmt`."""
    key = ("frame", scene, cam, W, H, lim)
    if key not in _CACHE:
        cc, w = program(oracle, scene)
        table = scenes.MATERIAL_TABLE if scene in scenes.MAT_SCENES else None
        _CACHE[key] = oracle.render(camera(oracle, cam, W, H), lim, cc, w, W, H, threads=16, materials=table)
        _CACHE[key].setflags(write=False)
    if fmt == F32:
        return _CACHE[key]
    if key + (fmt,) not in _CACHE:
        _CACHE[key + (fmt,)] = oracle.quantize_unorm8(_CACHE[key], bgra=fmt == BGRA8)
        _CACHE[key + (fmt,)].setflags(write=False)
    return _CACHE[key + (fmt,)]


def lit_frame(oracle, scene, cam, W, H, lim=LIM, fmt=F32):
    """tests/light_ref.py's whole frame under the default lighting."""
    key = ("lit", scene, cam, W, H, lim)
    if key not in _CACHE:
        cc, w = program(oracle, scene)
        table = scenes.MATERIAL_TABLE if scene in scenes.MAT_SCENES else None
        _CACHE[key] = light_ref.render(udict(camera(oracle, cam, W, H)), lim, cc, w, W, H, materials=table, light=light_ref.params())[0]
        _CACHE[key].setflags(write=False)
    return _CACHE[key] if fmt == F32 else oracle.quantize_unorm8(_CACHE[key], bgra=fmt == BGRA8)


def load(res, oracle, scene, cam, W, H, lim=LIM):
    res.set_limits(lim)
    res.set_program(*program(oracle, scene))
    res.set_materials(scenes.MATERIAL_TABLE if scene in scenes.MAT_SCENES else [(0.4, 0.7, 0.1)])
    res.set_uniforms(ffi_u(camera(oracle, cam, W, H)))


def bands(H):
    """Whole frame first, then the row bands (row0, rows) that fit: one row, a band inside the first tile row, one that starts
    on a tile's last row and ends inside the next but one, the frame's last row."""
    out = [(0, H)]
    for b in ((0, 1), (3, 5), (7, 11), (H - 1, 1)):
        if b[0] + b[1] <= H and b not in out:
            out.append(b)
    return out


def guard_rows(n_rows, W, fmt):
    """Float frames: at least 8 rows and 64 pixels.  8-bit frames: three times the region and 8 rows more behind it (and as
    much in front), so that a 16-byte store at ANY pixel index of the region would still land inside the allocation."""
    return max(8, -(-64 // W)) if fmt == F32 else 3 * n_rows + 8


def draw_checked(res, ref, fmt, what, call):
    """call(ptr) issues one device-path draw at ptr; the buffer around it is then held against ref."""
    ref = np.ascontiguousarray(ref)
    n_rows = int(np.prod(ref.shape[:-2]))
    g = guard_rows(n_rows, ref.shape[-2], fmt)
    buf = WC.guarded(ref.shape, ref.dtype, g)
    call(WC.region_ptr(buf, g))
    res.sync()
    WC.check(buf, ref, what)
    return buf[g:g + n_rows]


# ---- a. shapes at the tile grid's edges; b. formats ------------------------------------------------------------------------------
def sweep(res, oracle, kernel, wpts, sizes, scenes_, fmt):
    n = 0
    for W, H in sizes:
        for scene in scenes_:
            load(res, oracle, scene, "A", W, H)
            ref = frame(oracle, scene, "A", W, H, fmt=fmt)
            for wpt in wpts:
                for cull in (0, 1):
                    configure(res, kernel, cull=cull, wpt=wpt, fmt=fmt)
                    for row0, rows in bands(H):
                        what = "%s %s %dx%d rows [%d,+%d) wpt %d cull %d fmt %d" % (kernel, scene, W, H, row0, rows, wpt, cull, fmt)
                        draw_checked(res, ref[row0:row0 + rows], fmt, what,
                                     lambda p: res.draw_device(W, H, p, row0=row0, rows=rows))
                        n += 1
                    if kernel != "pixel":    # the kernel the case names is the kernel that drew
                        assert res.info(_ffi.RM_INFO_SPECIALIZED) == kernel.startswith("v5_spec"), (kernel, scene, wpt, res.jit_log())
    return n


@pytest.mark.parametrize("wpt", [1, 2, 4, 8])
@pytest.mark.parametrize("kernel", V5_KERNELS)
def test_frames_and_bands_at_the_tile_grids_edges(res, oracle, kernel, wpt):
    """rm_draw whole and in bands at sizes of one pixel, one tile, one tile and a column / a row, ragged in both directions, and
    several tiles each way; miss tests off and on."""
    assert [len(bands(H)) for H in (1, 8, 9, 17, 65)] == [1, 4, 4, 4, 5]
    sweep(res, oracle, kernel, [wpt], SIZES, ("g8", "g32"), F32)


def test_frames_and_bands_of_the_pixel_kernel(res, oracle):
    """RM_KERNEL_PIXEL (16 x 16 workgroups, reference node types, RGBA32F only) writes through its own bounds test."""
    sweep(res, oracle, "pixel", [0], SIZES, ("g8",), F32)


@pytest.mark.parametrize("fmt", [RGBA8, BGRA8], ids=["rgba8", "bgra8"])
@pytest.mark.parametrize("kernel", V5_KERNELS)
def test_eight_bit_frames_and_bands(res, oracle, kernel, fmt):
    """The 17x65 and 72x48 cases above with 4-byte pixels: the guards are in bytes, and a 16-byte store into such a frame
    lands behind the region (tests/test_write_coverage_cpu.py shows what that looks like)."""
    sweep(res, oracle, kernel, [1, 2, 4, 8], FORMAT_SIZES, ("g8", "g32"), fmt)


# ---- c. the second draw of a shape must not lean on the first ---------------------------------------------------------------------
def tile_classes(ref):
    """Per 8 x 8 tile of an oracle frame: 0 all sky (black), 1 no hit colour (sky and floor only), 2 some surface.  The floor's
    colours are grey-blue (r == g), a hit's (0.4, 0.7, 0.1) * k has r != g."""
    H, W = ref.shape[:2]
    out = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            t = ref[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            out[ty, tx] = 2 if np.any(t[..., 0] != t[..., 1]) else 1 if np.any(t[..., :3] != 0) else 0
    return out


@pytest.mark.parametrize("kernel", ["v5_lds", "v5_spec"])
@pytest.mark.parametrize("balance", [0, 1, 2, 3])
def test_second_draw_of_a_shape_does_not_lean_on_the_first(res, oracle, balance, kernel):
    """Frame A, frame B from the far side, frame A again -- same shape and program, each into a fresh sentinel-filled buffer.
    Under balance 3 the second and third draw are sorted by the durations the draw before them measured."""
    W, H, scene = 200, 120, "g32"
    a, b = frame(oracle, scene, "A", W, H), frame(oracle, scene, "B", W, H)
    ca, cb = tile_classes(a), tile_classes(b)
    assert np.mean(ca != cb) > 0.2 and all(np.any((ca == k) != (cb == k)) for k in (0, 1, 2)), "camera B must reclassify tiles"
    configure(res, kernel, balance=balance)
    for cam, ref in (("A", a), ("B", b), ("A", a)):
        load(res, oracle, scene, cam, W, H)
        draw_checked(res, ref, F32, "%s balance %d camera %s" % (kernel, balance, cam), lambda p: res.draw_device(W, H, p))


@pytest.mark.parametrize("kernel", ["v5_lds", "v5_spec"])
def test_durations_of_another_program(res, oracle, kernel):
    """g8, then g32 at the same shape under balance 3: the durations the sort reads belong to another scene."""
    W, H = 200, 120
    configure(res, kernel, balance=3)
    for scene in ("g8", "g32", "g8"):
        load(res, oracle, scene, "A", W, H)
        draw_checked(res, frame(oracle, scene, "A", W, H), F32, "%s after another program" % scene, lambda p: res.draw_device(W, H, p))


def shape_key(W, rows, n_frames, strip_rows=0, strip_first=0, strip_stride=0):
    """launch_v5_w's key of the launch the measured durations belong to, restated."""
    return (W << 40) ^ (rows << 20) ^ (strip_rows << 12) ^ (strip_first << 6) ^ strip_stride ^ (n_frames << 52) ^ 1


def test_two_launches_that_share_a_shape_key(res, oracle):
    """A 2-frame batch at W = 4160 and a 3-frame batch at W = 64, both 16 rows: 4160 << 40 = 2^52 + 2^46 and 2 << 52 = 2^53;
    64 << 40 = 2^46 and 3 << 52 = 2^53 + 2^52 -- the XOR of shifted fields gives both launches the key
    0x30400001000001, so the second sorts its 16 tiles per frame by what the first measured for other tiles of other
    frames.  The order never changes a pixel.  The larger launch goes first: the buffer of durations is then big enough, and
    the key is all that decides."""
    H, scene = 16, "g8"
    wide, narrow = (4160, ("A", "B")), (64, ("C", "D", "E"))
    assert shape_key(4160, H, 2) == shape_key(64, H, 3) == 0x30400001000001
    configure(res, "v5_spec", balance=3)
    for W, cams in (wide, narrow, wide):
        load(res, oracle, scene, cams[0], W, H)
        ref = np.stack([frame(oracle, scene, c, W, H) for c in cams])
        frames = [ffi_u(camera(oracle, c, W, H)) for c in cams]
        draw_checked(res, ref, F32, "%d-frame batch at %dx%d" % (len(cams), W, H), lambda p: res.draw_batch_device(frames, W, H, p))


# ---- d. the sort's batch boundaries ----------------------------------------------------------------------------------------------
SORT_LIM = (0.01, 100.0, 20)


@pytest.mark.parametrize("W,H", [(504, 1024), (512, 1024), (520, 1024)], ids=["8064", "8192", "8320"])
def test_tile_counts_around_one_sort_batch(res, oracle, W, H):
    """rm_tile_sort_v5 walks the tiles 8192 at a time (1024 threads x 8): frames of 8064, exactly 8192 and 8320 tiles, by
    pending pixels (balance 1) and by the durations of a first draw (balance 3, both draws checked)."""
    assert ((W + 7) // 8) * ((H + 7) // 8) == {504: 8064, 512: 8192, 520: 8320}[W]
    load(res, oracle, "g8", "A", W, H, SORT_LIM)
    ref = frame(oracle, "g8", "A", W, H, SORT_LIM)
    for balance, draws in ((1, 1), (3, 2)):
        configure(res, "v5_spec", balance=balance)
        for k in range(draws):
            draw_checked(res, ref, F32, "%dx%d balance %d draw %d" % (W, H, balance, k + 1), lambda p: res.draw_device(W, H, p))


def tiles_marched(res, n_frames, wpt):
    """(per frame: tiles the workgroups report, workgroups per frame) from the wave statistics, with the invariants every record
    must meet: end >= start, and one n_tiles_done per workgroup."""
    st = res.wave_stats()
    assert len(st) and len(st) % (n_frames * wpt) == 0, "%d records for %d frames of workgroups of %d waves" % (len(st), n_frames, wpt)
    st = st.reshape(n_frames, -1, wpt, 4)
    assert np.all(st[..., 1] >= st[..., 0]), "a wave ended before it started"
    done = (st[..., 2] >> np.uint64(32)).astype(np.int64)
    assert np.all(done == done[..., :1]), "the waves of a workgroup disagree on the tiles they worked on"
    return done[..., 0].sum(axis=1), st.shape[1]


@pytest.mark.parametrize("cull", [0, 1])
def test_every_tile_in_the_heaviest_bucket(res, oracle, cull):
    """Camera inside a large box: no tile can be settled, every tile has 64 pending pixels, and the sort's ballot shortcut for
    bucket 0 places all 8320 of them -- more than one batch."""
    W, H = 520, 1024
    load(res, oracle, "big_box", "A", W, H, SORT_LIM)
    configure(res, "v5_lds", cull=cull, balance=1, wpt=4, stats=1)
    draw_checked(res, frame(oracle, "big_box", "A", W, H, SORT_LIM), F32, "inside a box, cull %d" % cull, lambda p: res.draw_device(W, H, p))
    done, _ = tiles_marched(res, 1, 4)
    assert done.tolist() == [8320]


@pytest.mark.parametrize("W,H", [(72, 48), (520, 1024)])
def test_no_tile_on_the_work_list(res, oracle, W, H):
    """The empty program: the pre-pass settles every tile, the work list is empty, the march kernel claims nothing."""
    load(res, oracle, "empty", "A", W, H, SORT_LIM)
    for balance in (1, 3, 3):
        configure(res, "v5_lds", balance=balance, wpt=4, stats=1)
        draw_checked(res, frame(oracle, "empty", "A", W, H, SORT_LIM), F32, "empty program %dx%d balance %d" % (W, H, balance),
                     lambda p: res.draw_device(W, H, p))
        done, _ = tiles_marched(res, 1, 4)
        assert done.tolist() == [0]


# ---- e. strips and the gather ----------------------------------------------------------------------------------------------------
STRIP_W, STRIP_H = 72, 52        # 6.5 strips of 8 rows, 3.25 of 16: the last strip is ragged


def strips_ref(ref, strip_rows, rank, world):
    parts = [ref[r0:r0 + n] for r0, n in shard.strips_of_rank(ref.shape[0], rank, world, strip_rows)]
    return np.concatenate(parts) if parts else ref[:0]


def draw_rank(res, ref, fmt, strip_rows, rank, world):
    W, H = ref.shape[1], ref.shape[0]
    want = strips_ref(ref, strip_rows, rank, world)
    assert want.shape[0] == shard.strip_row_count(H, strip_rows, rank, world)
    got = []
    buf = draw_checked(res, want, fmt, "strips of %d rows, rank %d of %d" % (strip_rows, rank, world),
                       lambda p: got.append(res.draw_strips_device(W, H, strip_rows, rank, world, p)))
    assert got == [want.shape[0]]
    return buf


@pytest.mark.parametrize("fmt", [F32, RGBA8], ids=["float", "rgba8"])
@pytest.mark.parametrize("kernel", ["v5_lds", "v5_spec"])
@pytest.mark.parametrize("strip_rows", [8, 16])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_strips_of_every_rank(res, oracle, world, strip_rows, kernel, fmt):
    """rm_draw_strips: each rank into its own buffer of exactly its rows; a rank without a strip writes nothing at all."""
    W, H = STRIP_W, STRIP_H
    load(res, oracle, "g32", "A", W, H)
    configure(res, kernel, fmt=fmt)
    ref = frame(oracle, "g32", "A", W, H, fmt=fmt)
    empty = 0
    for rank in range(world):
        empty += draw_rank(res, ref, fmt, strip_rows, rank, world).shape[0] == 0
    assert empty == max(0, world - shard.n_strips(H, strip_rows))


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("strip_rows", [8, 16])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_gather_writes_a_ranks_rows_and_no_others(res, oracle, world, strip_rows, pinned):
    """rm_gather_strips into a sentinel-filled host image: rank r's gather alone changes rank r's rows only; all ranks
    together give the oracle's frame."""
    torch = pytest.importorskip("torch")
    W, H = STRIP_W, STRIP_H
    load(res, oracle, "g32", "A", W, H)
    configure(res, "v5_spec")
    ref = frame(oracle, "g32", "A", W, H)
    strips = [draw_rank(res, ref, F32, strip_rows, rank, world) for rank in range(world)]

    def host_image():
        img = torch.from_numpy(WC.sentinel_array((H, W, 4), np.float32).copy())
        img = img.pin_memory() if pinned else img
        assert img.is_pinned() == pinned
        return img

    everything = host_image()
    for rank in range(world):
        alone = host_image()
        for img in (alone, everything):
            res.gather_strips(W, H, strip_rows, rank, world, strips[rank].data_ptr(), img.data_ptr())
        res.sync()
        mine = np.zeros(H, dtype=bool)
        for r0, n in shard.strips_of_rank(H, rank, world, strip_rows):
            mine[r0:r0 + n] = True
        a = alone.numpy()
        assert np.array_equal(WC.written(a), np.broadcast_to(mine[:, None], (H, W))), "rank %d of %d" % (rank, world)
        assert WC.untouched(a[~mine]).all() and a[mine].tobytes() == ref[mine].tobytes(), "rank %d of %d" % (rank, world)
    WC.check(everything.numpy(), ref, "gather of %d ranks" % world)


# ---- f. batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, BGRA8], ids=["float", "bgra8"])
@pytest.mark.parametrize("n_frames", [1, 2, 5])
def test_batch_frames_lie_back_to_back(res, oracle, n_frames, fmt):
    """rm_draw_batch: frame f at f W H pixels of one buffer, each against the oracle's frame of its own camera."""
    cams = ["A", "B", "C", "D", "E"][:n_frames]
    for W, H in FORMAT_SIZES:
        ref = np.stack([frame(oracle, "g8", c, W, H, fmt=fmt) for c in cams])
        frames = [ffi_u(camera(oracle, c, W, H)) for c in cams]
        load(res, oracle, "g8", "A", W, H)
        for kernel in ("v5_lds", "v5_spec"):
            configure(res, kernel, fmt=fmt)
            draw_checked(res, ref, fmt, "%s batch of %d at %dx%d" % (kernel, n_frames, W, H),
                         lambda p: res.draw_batch_device(frames, W, H, p))


# ---- g. lit draws ----------------------------------------------------------------------------------------------------------------
LIT_CASES = [("g8", 17, 65), ("g8", 72, 48), ("mat_mix", 72, 48)]


@pytest.mark.parametrize("fmt", [F32, RGBA8], ids=["float", "rgba8"])
@pytest.mark.parametrize("scene,W,H", LIT_CASES, ids=["%s-%dx%d" % c for c in LIT_CASES])
def test_lit_frames_and_bands(res, oracle, scene, W, H, fmt):
    """rm_draw_lit (shadows and occlusion at their defaults) whole, as a band between odd rows, and as the last row."""
    load(res, oracle, scene, "A", W, H)
    res.set_lighting(**dict(zip(light_ref.NAMES, (float(v) for v in light_ref.params()))))
    configure(res, "v5_spec", fmt=fmt)
    ref = lit_frame(oracle, scene, "A", W, H, fmt=fmt)
    assert fmt != F32 or not np.array_equal(ref, frame(oracle, scene, "A", W, H)), "the frame must be lit"
    for row0, rows in ((0, H), (7, 11), (H - 1, 1)):
        draw_checked(res, ref[row0:row0 + rows], fmt, "lit %s %dx%d rows [%d,+%d)" % (scene, W, H, row0, rows),
                     lambda p: res.draw_lit_device(W, H, p, row0=row0, rows=rows))


# ---- h. the host path returns this draw's pixels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["draw", "strips", "batch", "lit"])
def test_host_path_returns_this_draws_pixels(res, oracle, entry):
    """The one case that goes through the staging buffer, because the staging buffer is its subject: a host draw of frame A
    leaves A there; the host draw of frame B (same shape, same bytes, another camera) must return B -- the bytes the device
    path writes into sentinel-filled memory, and the oracle's.  With A in the staging buffer a stale pixel is a wrong pixel."""
    W, H, scene = 72, 48, "g8" if entry == "lit" else "g32"     # (the lit reference of g8 is shared with the lit cases)
    configure(res, "v5_spec")
    res.set_lighting(**dict(zip(light_ref.NAMES, (float(v) for v in light_ref.params()))))
    if entry == "batch":
        cams_a, cams_b = ("A", "C"), ("B", "D")
        fa, fb = ([ffi_u(camera(oracle, c, W, H)) for c in cams] for cams in (cams_a, cams_b))
        ref_a, ref_b = (np.stack([frame(oracle, scene, c, W, H) for c in cams]) for cams in (cams_a, cams_b))
        host = lambda cam: res.draw_batch(fa if cam == "A" else fb, W, H)                  # noqa: E731
        device = lambda p: res.draw_batch_device(fb, W, H, p)                              # noqa: E731
    elif entry == "strips":
        cut = lambda ref: strips_ref(ref, 16, 1, 2)                                        # noqa: E731
        ref_a, ref_b = cut(frame(oracle, scene, "A", W, H)), cut(frame(oracle, scene, "B", W, H))
        host = lambda cam: res.draw_strips(W, H, 16, 1, 2)                                 # noqa: E731
        device = lambda p: res.draw_strips_device(W, H, 16, 1, 2, p)                       # noqa: E731
    elif entry == "lit":
        ref_a, ref_b = lit_frame(oracle, scene, "A", W, H), lit_frame(oracle, scene, "B", W, H)
        host = lambda cam: res.draw_lit(W, H)                                              # noqa: E731
        device = lambda p: res.draw_lit_device(W, H, p)                                    # noqa: E731
    else:
        ref_a, ref_b = frame(oracle, scene, "A", W, H), frame(oracle, scene, "B", W, H)
        host = lambda cam: res.draw(W, H)                                                  # noqa: E731
        device = lambda p: res.draw_device(W, H, p)                                        # noqa: E731
    assert ref_a.shape == ref_b.shape and np.mean(np.any(ref_a != ref_b, axis=-1)) > 0.3, "frame B must differ from frame A"
    load(res, oracle, scene, "A", W, H)
    host_a = host("A")
    load(res, oracle, scene, "B", W, H)
    host_b = host("B")
    dev_b = draw_checked(res, ref_b, F32, "%s: device draw of frame B" % entry, device).cpu().numpy().reshape(ref_b.shape)
    assert host_a.tobytes() == ref_a.tobytes(), "%s: host draw of frame A" % entry
    assert host_b.tobytes() == dev_b.tobytes(), "%s: the host path and the device path disagree on frame B" % entry
    assert host_b.tobytes() == ref_b.tobytes(), "%s: host draw of frame B" % entry


# ---- i. tiles marched, from the wave statistics -----------------------------------------------------------------------------------
STATS_LIM = (0.01, 100.0, 30)


def surface_tiles(oracle, cam, W, H):
    """Tiles with at least one sample that hits a surface, by the CPU reference of the G-buffer (tests/gbuffer_ref.py)."""
    key = ("surface", cam, W, H)
    if key not in _CACHE:
        cc, w = program(oracle, "g8")
        hit = gbuffer_ref.render(udict(camera(oracle, cam, W, H)), STATS_LIM, cc, w, W, H)["surface_mask"] != 0
        pad = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), dtype=bool)
        pad[:H, :W] = hit
        _CACHE[key] = int(pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).any(axis=(1, 3)).sum())
    return _CACHE[key]


@pytest.mark.parametrize("W,H", [(72, 48), (200, 120)])
@pytest.mark.parametrize("cams", [("A",), ("A", "B")], ids=["single", "batch2"])
@pytest.mark.parametrize("wpt", [4, 8])
@pytest.mark.parametrize("kernel", ["v5_lds", "v5_spec"])
def test_tiles_marched_by_the_wave_statistics(res, oracle, kernel, wpt, cams, W, H):
    """rm_render_v5_body writes one record per wave: start, end, n_tiles_done << 32 | n_iter, a fourth word.  Without miss
    tests (RM_OPT_CULL = 0) and with max_iter >= 1 the pre-pass has no tables and settles nothing -- do_tile's `clear` is
    max_iter == 0 then, and a tile verdict needs tables or max_iter == 0 --, so every tile is claimed exactly once: a dropped
    tile lowers the sum, a tile claimed twice raises it.  With miss tests the count can only fall, and never below the tiles
    in which some sample hits a surface: such a sample's ray cannot be cleared."""
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    n = len(cams)
    load(res, oracle, "g8", cams[0], W, H, STATS_LIM)
    frames = [ffi_u(camera(oracle, c, W, H)) for c in cams]
    ref = np.stack([frame(oracle, "g8", c, W, H, STATS_LIM) for c in cams])
    issue = (lambda p: res.draw_batch_device(frames, W, H, p)) if n > 1 else (lambda p: res.draw_device(W, H, p))
    cus = int(res.info(_ffi.RM_INFO_CU_COUNT))
    marched = {}
    for cull in (0, 1):
        configure(res, kernel, cull=cull, wpt=wpt, stats=1)
        draw_checked(res, ref if n > 1 else ref[0], F32, "%s wpt %d cull %d, %d frames" % (kernel, wpt, cull, n), issue)
        assert res.info(_ffi.RM_INFO_SPECIALIZED) == (kernel == "v5_spec")
        marched[cull], n_wg = tiles_marched(res, n, wpt)
        # a persistent grid: as many workgroups as tiles, or a whole number per compute unit (at most 24 waves of one launch)
        assert n_wg in {min(n_tiles, cus * k) for k in range(1, 24 // wpt + 1)}, (n_wg, n_tiles, cus)
    assert marched[0].tolist() == [n_tiles] * n
    floor = [surface_tiles(oracle, c, W, H) for c in cams]
    assert all(lo > 0 for lo in floor)
    assert all(lo <= m <= n_tiles for lo, m in zip(floor, marched[1].tolist())), (floor, marched[1].tolist(), n_tiles)
