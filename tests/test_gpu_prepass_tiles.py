"""The pre-pass's verdicts on whole tiles ("Pre-pass"): rm_selftest_cull_tiles runs tile_verdict_v5 -- the
cone of a tile's 32 x 32 sample directions against the miss-test tables, the sky rule and the one-cell rule on the rectangle of
its sample positions -- with the launch a draw would fill.  A tile with "clear" and "sky" or "one cell" is filled with one
constant without a look at its pixels, so each flag, when set, must hold for EVERY one of the tile's 1024 samples: against
binary64 geometry for the zones (tests/cull_ref.py, as tests/test_gpu_cull_bounds.py does for pixels) and against the numpy
oracle's binary32 rays and floor codes.  One-sided: how many tiles are settled is asserted once, on the metric frame.  Then
frames that are settled tile by tile, bit for bit against the oracle."""
import hashlib

import numpy as np
import pytest

import gbuffer_ref
import scenes
from prepass_ref import CELL, CLEAR, SKY, check_tiles, floor_codes, pick_tiles, program as _program, udict, with_frame_corners
from ray_marching_amd import _ffi, renderer, shard
from test_cull_tables_cpu import decode
from test_gpu_cull_bounds import MIN_DISTS, _ptr, set_case, table_zones
from test_gpu_parity import assert_same, orbit_frame_uniforms, setup

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


def probe_tiles(res, W, H, txy):
    txy = np.ascontiguousarray(txy, dtype=np.uint32)
    out = np.zeros((len(txy), 8), dtype=F)
    res._check(res._L.rm_selftest_cull_tiles(res._h, W, H, _ptr(txy), len(txy), _ptr(out)))
    return out


def _camera(oracle, name, W, H):
    if name.startswith("orbit"):
        return orbit_frame_uniforms(oracle, W, H, int(name[5:]))
    spec = {"still": dict(events=scenes.STILL_CAMERA_EVENTS),
            "horizon": dict(target=(0.0, -1.45, 0.0), events=[(1, 140.0, -1.0)]),      # grazing along the floor
            "below": dict(events=[(1, 30.0, -120.0)]),                                   # under the floor plane (y = -4.66)
            "inside": dict(radius=0.5, events=[(1, 20.0, -10.0)])}[name]                # inside g8's unit sphere
    return oracle.orbit_uniforms((float(W), float(H)), **spec)[0]


# (program, camera, W, H, index into MIN_DISTS)
CASES = [("g32", "still", 1920, 1080, 3), ("g32", "orbit100", 1920, 1080, 2), ("g32s", "orbit700", 640, 360, 3), ("g8", "horizon", 1920, 1080, 1),
         ("g8", "below", 640, 360, 4), ("g8", "inside", 640, 360, 3), ("plane", "still", 640, 360, 3), ("xform_mix", "still", 1920, 1080, 0),
         ("xform_mix", "horizon", 640, 360, 5), ("g32s", "still", 1920, 1080, 4), ("g32", "still", 64, 36, 3)]
_RESULTS = {}


def probe_case(res, oracle, name, prog, u, W, H, min_dist, seed, frame_corners=False, cone_expected=None, n_each=70, n_random=90):
    """One probe call under the prepared uniform block u and its assertions (prepass_ref.check_tiles); returns how often each flag
    was seen set and unset.  prog: a scene's name or (cmd_count, words)."""
    cc, w = _program(oracle, prog) if isinstance(prog, str) else prog
    w = np.asarray(w, dtype=np.uint32)
    d = decode(cc, w)
    set_case(res, cc, w, min_dist)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    ud = udict(u)
    ro64 = np.array([ud["inv_view"][12 + k] for k in range(3)], dtype=F).astype(np.float64)
    vetoed = bool(d["cull_veto"])
    zones = [] if vetoed else table_zones(d, ro64, min_dist)
    txy = pick_tiles(ud, W, H, zones, np.random.default_rng(seed), n_each=n_each, n_random=n_random)
    if frame_corners:
        txy = with_frame_corners(txy, W, H)
    out = probe_tiles(res, W, H, txy)
    stats = check_tiles(name, ud, W, H, txy, out, zones, check_zones=not vetoed, cone_expected=cone_expected)
    print("%s: %s" % (name, stats))
    return stats


def run_case(res, oracle, case):
    """One of CASES; cached."""
    if case in _RESULTS:
        return _RESULTS[case]
    prog, cam, W, H, k = case
    name = "%s / %s / %dx%d / min_dist %g" % (prog, cam, W, H, MIN_DISTS[k])
    _RESULTS[case] = probe_case(res, oracle, name, prog, _camera(oracle, cam, W, H), W, H, MIN_DISTS[k], 61000 + CASES.index(case),
                                cone_expected=W >= 100)
    return _RESULTS[case]


@pytest.mark.parametrize("case", CASES, ids=["%s-%s-%dx%d" % c[:4] for c in CASES])
def test_tile_verdicts_hold_for_every_sample(res, oracle, case):
    run_case(res, oracle, case)


def test_every_flag_is_seen_set_and_unset(res, oracle):
    total = {}
    for case in CASES:
        for k, v in run_case(res, oracle, case).items():
            if isinstance(v, tuple):
                total[k] = tuple(a + b for a, b in zip(total.get(k, (0, 0)), v))
    print("tile flags (set, unset): %s" % total)
    for k, (n_set, n_unset) in total.items():
        assert n_set > 20 and n_unset > 20, (k, total)


def test_half_of_the_metric_frame_is_settled_per_tile(res, oracle):
    """Not vacuous: a binary64 model that inflates every zone of the tables by twice the tile's angular radius settles 65.5 % of
    the tiles of the 1920x1080 metric frame (tools/prepass_tile_classes.py, profiles/r11_prepass_tile_classes.json); the kernel's
    slacks are orders of magnitude below a tile's size, so at least half must come back settled."""
    W, H = 1920, 1080
    cc, w = oracle.serialize(*scenes.g32())
    res.set_option(_ffi.RM_OPT_CULL, 1)
    res.set_limits((0.01, 100.0, 256))
    res.set_program(cc, np.asarray(w, dtype=np.uint32))
    u = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)[0]
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    tx, ty = np.meshgrid(np.arange(W // 8), np.arange(H // 8))
    flags = probe_tiles(res, W, H, np.stack([tx.ravel(), ty.ravel()], axis=1))[:, 5].view(np.uint32)
    settled = ((flags & CLEAR) != 0) & ((flags & (SKY | CELL)) != 0)
    print("metric frame: %d of %d tiles settled per tile (%.1f %%): %d sky, %d one cell; %d clear" % (
        settled.sum(), len(flags), 100.0 * settled.mean(), (settled & ((flags & SKY) != 0)).sum(), (settled & ((flags & CELL) != 0)).sum(),
        ((flags & CLEAR) != 0).sum()))
    assert settled.mean() >= 0.5


# ---- frames, bit for bit --------------------------------------------------------------------------------------------------------
METRIC_LIMITS = (0.01, 100.0, 256)


def _metric(res, oracle, W=1920, H=1080, limits=METRIC_LIMITS, cam="still"):
    cc, w = oracle.serialize(*scenes.g32())
    u = _camera(oracle, cam, W, H)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=limits)
    return cc, w, u


def _horizon_row(u, W, H):
    """First row of the frame's middle column whose centre ray reaches the floor."""
    py = np.arange(H, dtype=np.uint32)
    ro, d = gbuffer_ref.camera_rays(np.full(H, W // 2, np.uint32), py, _ffi.RM_SAMPLE_CENTER, udict(u), W, H)
    return int(np.argmax(floor_codes(np.array(ro, dtype=F)[:3], d) >= 0))


@pytest.mark.parametrize("band", ["sky", "horizon", "near floor", "objects", "unaligned"])
def test_bands_of_the_metric_frame(res, oracle, band):
    """64-row bands of the 1920x1080 metric frame, drawn on their own with row0 / rows (the tiles start at row0)."""
    W, H = 1920, 1080
    cc, w, u = _metric(res, oracle)
    hz = _horizon_row(u, W, H)
    assert 64 < hz < H - 128
    row0 = {"sky": 0, "horizon": (hz - 30) // 8 * 8, "near floor": H - 64, "objects": 504, "unaligned": hz - 27}[band]
    assert (row0 % 8 != 0) == (band == "unaligned")
    assert_same(res.draw(W, H, row0=row0, rows=64), oracle.render(u, METRIC_LIMITS, cc, w, W, H, row0=row0, rows=64, threads=16))


def test_ragged_frame_and_its_edge_tiles(res, oracle):
    """1918 x 1078: the last tile column and row hang over the frame; the tile verdict uses the whole 8 x 8 rectangle."""
    W, H = 1918, 1078
    cc, w, u = _metric(res, oracle, W, H)
    full = res.draw(W, H)
    hz = _horizon_row(u, W, H)
    for r0, rows in ((0, 16), (hz - 8, 16), (H - 22, 22)):
        assert_same(full[r0:r0 + rows], oracle.render(u, METRIC_LIMITS, cc, w, W, H, row0=r0, rows=rows, threads=16))


def test_strips_of_16_rows_and_heights_the_abi_refuses(res, oracle):
    """Interleaved 16-row strips (the multi-GPU partition): a tile's eight rows stay consecutive frame rows, so tiles are settled
    as in a whole frame, and the reassembled frame is the frame.  A strip height that is no multiple of 8 would break that; the ABI
    does not admit one."""
    W, H = 1920, 1080
    _metric(res, oracle)
    full = res.draw(W, H)
    img = np.zeros_like(full)
    for rank in range(3):
        shard.scatter_strips(img, res.draw_strips(W, H, 16, rank, 3), H, rank, 3, 16)
    assert hashlib.sha256(img.tobytes()).digest() == hashlib.sha256(full.tobytes()).digest()
    with pytest.raises(_ffi.RmError):
        res.draw_strips(W, H, 12, 0, 2)


def test_two_frame_batch(res, oracle):
    W, H = 640, 360
    cc, w, _ = _metric(res, oracle, W, H)
    frames = [_camera(oracle, cam, W, H) for cam in ("still", "orbit300")]
    batch = res.draw_batch([_ffi.Uniforms.from_buffer_copy(bytes(f)) for f in frames], W, H)
    hz = _horizon_row(frames[1], W, H)
    for i, f in enumerate(frames):
        res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(f)))
        assert batch[i].tobytes() == res.draw(W, H).tobytes()
    for r0, rows in ((0, 8), (hz - 8, 16), (H - 8, 8)):
        assert_same(batch[1][r0:r0 + rows], oracle.render(frames[1], METRIC_LIMITS, cc, w, W, H, row0=r0, rows=rows, threads=16))


def test_no_march_steps(res, oracle):
    """max_iter = 0: every ray is a miss, with or without tables; every tile is sky, one cell, or sampled."""
    W, H = 1920, 1080
    lim = (0.01, 100.0, 0)
    cc, w, u = _metric(res, oracle, limits=lim)
    hz = _horizon_row(u, W, H)
    for cull in (1, 0):
        res.set_option(_ffi.RM_OPT_CULL, cull)
        for r0 in (0, hz - 24, H - 64):
            assert_same(res.draw(W, H, row0=r0, rows=64), oracle.render(u, lim, cc, w, W, H, row0=r0, rows=64, threads=16))
    res.set_option(_ffi.RM_OPT_CULL, 1)


def test_8bit_output_of_settled_tiles(res, oracle):
    W, H = 1920, 1080
    cc, w, u = _metric(res, oracle)
    hz = _horizon_row(u, W, H)
    try:
        for r0 in (hz - 24, H - 64):
            ref = oracle.quantize_unorm8(oracle.render(u, METRIC_LIMITS, cc, w, W, H, row0=r0, rows=64, threads=16))
            res.set_output_format(_ffi.RM_FORMAT_RGBA8_UNORM)
            img = res.draw(W, H, row0=r0, rows=64)
            res.set_output_format(_ffi.RM_FORMAT_RGBA32F)
            assert img.dtype == np.uint8 and img.tobytes() == ref.tobytes()
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)


def test_camera_below_the_floor(res, oracle):
    """Nothing is assumed about the floor from below: no tile is sky or one cell, every pixel is still right."""
    W, H = 640, 360
    cc, w = oracle.serialize(*scenes.g8())
    u = _camera(oracle, "below", W, H)
    lim = (0.01, 100.0, 64)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=lim)
    tx, ty = np.meshgrid(np.arange(W // 8), np.arange(H // 8))
    flags = probe_tiles(res, W, H, np.stack([tx.ravel(), ty.ravel()], axis=1))[:, 5].view(np.uint32)
    assert not (flags & (SKY | CELL)).any()
    assert_same(res.draw(W, H), oracle.render(u, lim, cc, w, W, H, threads=16))
