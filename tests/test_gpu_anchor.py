"""The anchored first step of the march (rm_kernel_v5.h "Pruning", anchored first step) on the device.

(a) rm_selftest_anchor runs the two device functions the march calls around two interpreter evaluations, on the pairs of
    tests/test_anchor_cpu.py: the threshold bounds the device's own |F(q)| and the binary64 one; non-finite points never yield a
    finite threshold; the numbers are tests/anchor_ref.py's (one unit in the last place for the multiply-add's second rounding).
(b) frames, bit for bit against oracle.cbind.render: a skipped leaf that mattered changes a pixel.  Waves per tile 1, 2, 4, 8 (who
    takes which batch, and so which anchor meets which batch), interpreter and generated kernel, refill thresholds 1, 16, 64 (at
    less than 64 the anchor's lane is deeper into its march), partial tiles; scenes in which neighbouring batches see unrelated
    values; cameras whose rays do not take the shared step at all.
(c) the rule fires: leaves evaluated on g32 at 64x64, against the parent commit's count."""
import numpy as np
import pytest

import anchor_ref as A
import scene_f64
import scenes
from ray_marching_amd import _ffi, renderer
from test_cull_tables_cpu import decode
from test_gpu_cull_bounds import _ptr, set_case
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
N_PAIRS = 3000
LIM = (0.01, 100.0, 64)
SIZES = ((64, 64), (40, 24), (17, 9))


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.set_option(_ffi.RM_OPT_WAVE_STATS, 0)
    r.close()


def probe_anchor(res, ro, pr):
    ro, pr = np.ascontiguousarray(ro, dtype=F), np.ascontiguousarray(pr, dtype=F)
    out = np.zeros((len(pr), 4), dtype=F)
    res._check(res._L.rm_selftest_anchor(res._h, _ptr(ro), _ptr(pr), len(pr), _ptr(out)))
    return out


def _ulps(x, y):
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


# ---- (a) the device functions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.PAIR_PROGRAMS)
def test_device_threshold_bounds_the_value_at_q(res, oracle, name):
    cc, w, centre = A.program(oracle, name)
    scene_scale = decode(cc, w)["scene_scale"]
    set_case(res, cc, w, 0.01)
    rng = np.random.default_rng(2200 + A.PAIR_PROGRAMS.index(name))
    for radius in (5.0, 50.0):
        _, pos, _, _ = oracle.orbit_uniforms((64.0, 64.0), target=tuple(centre), radius=radius, events=scenes.STILL_CAMERA_EVENTS)
        ro = np.array(pos, dtype=F)
        ps = A.prune_scale(scene_scale, ro)
        f0 = float(scene_f64.map_scene(cc, w, 100.0, ro[None])[0])
        pr = A.pairs(ro, centre, abs(f0), rng, N_PAIRS)
        a, q = pr[:, 0], pr[:, 1]
        out = probe_anchor(res, ro, pr)
        aT, thr, fa, fq = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        assert np.all(np.isfinite(out)), name
        # the device's own value at q, and the real one with the evaluation error the derivation allows for
        k = int(np.argmin(thr - np.abs(fq)))
        assert np.all(thr >= np.abs(fq)), "%s: pair %d a %s q %s: thr %.9g < |F(q)| = %.9g on the device" % (
            name, k, a[k].tolist(), q[k].tolist(), thr[k], abs(fq[k]))
        f64q = scene_f64.map_scene(cc, w, 100.0, q)
        need = np.abs(f64q) + A.eval_error(ps, q)
        k = int(np.argmin(thr - need))
        assert np.all(thr.astype(np.float64) >= need), "%s: pair %d: thr %.9g < |F64(q)| + E = %.9g" % (name, k, thr[k], need[k])
        # (the device's values are within that error of binary64: what the CPU test assumes of F_a)
        assert np.all(np.abs(fa - scene_f64.map_scene(cc, w, 100.0, a)) <= A.eval_error(ps, a)), name
        # the restatement
        assert np.array_equal(aT, A.anchor_reach(a, fa, ps)), name
        assert _ulps(thr, A.threshold(q, a, fa, ps)).max() <= 1, name


def test_device_non_finite_points_never_give_a_finite_threshold(res, oracle):
    cc, w, centre = A.program(oracle, "g32")
    set_case(res, cc, w, 0.01)
    _, pos, _, _ = oracle.orbit_uniforms((64.0, 64.0), events=scenes.STILL_CAMERA_EVENTS)
    ro = np.array(pos, dtype=F)
    rng = np.random.default_rng(2221)
    bad = A.poisoned(A.pairs(ro, centre, 3.0, rng, 1200), rng)
    out = probe_anchor(res, ro, bad)
    assert not np.any(np.isfinite(out[:, 1])) and not np.any(out[:, 1] == -np.inf)
    # a NaN value at the anchor (a NaN coordinate there) makes the reach a NaN
    nan_a = np.isnan(bad[:, 0]).any(axis=1)
    assert nan_a.sum() > 100 and np.all(np.isnan(out[nan_a, 0]))
    L = res._L
    assert L.rm_selftest_anchor(res._h, _ptr(ro), _ptr(bad), 0, _ptr(out)) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_anchor(res._h, None, _ptr(bad), 4, _ptr(out)) == _ffi.RM_ERR_NULL
    assert L.rm_selftest_anchor(None, _ptr(ro), _ptr(bad), 4, _ptr(out)) == _ffi.RM_ERR_NULL


# ---- (b) frames -----------------------------------------------------------------------------------------------------------------
FRAME_PROGRAMS = ("g32", "g64", "g32_balanced", "tiny_sphere", "edge_on_box", "far")
# camera -> (orbit radius, limits): the still camera; inside the solid: f0 < min_dist, every ray starts as a hit at ro; f0 > max_dist:
# every ray ends at once; r = 50: a large f0, the start sphere passes through the scene's far side
CAMERAS = {"still": (5.0, LIM), "inside": (0.1, LIM), "beyond": (5.0, (0.01, 2.5, 64)), "r50": (50.0, LIM)}
INSIDE = (0.55, 0.15, 0.55)     # within g32's sphere of grid cell (2, 2): the "inside" camera orbits this point at 0.1
_REFS = {}


def _uniforms(oracle, name, cam, W, H):
    _, centre = A.PROGRAMS[name]
    events = A.EDGE_ON_EVENTS if name == "edge_on_box" else scenes.STILL_CAMERA_EVENTS
    target = tuple(np.add(centre, INSIDE)) if cam == "inside" else tuple(centre)
    return oracle.orbit_uniforms((float(W), float(H)), target=target, radius=CAMERAS[cam][0], events=events)[:2]


def reference(oracle, name, cam, W, H):
    """the oracle's frame, rendered once per (program, camera, size) and read-only after"""
    key = (name, cam, W, H)
    if key not in _REFS:
        cc, w, _ = A.program(oracle, name)
        u, pos = _uniforms(oracle, name, cam, W, H)
        img = oracle.render(u, CAMERAS[cam][1], cc, w, W, H, threads=16)
        img.setflags(write=False)
        _REFS[key] = (cc, w, u, np.array(pos, dtype=F), img)
    return _REFS[key]


def _configure(res, wpt, spec, refill):
    res.set_option(_ffi.RM_OPT_KERNEL, _ffi.RM_KERNEL_DEFAULT)
    res.set_option(_ffi.RM_OPT_CULL, 1)
    res.set_option(_ffi.RM_OPT_WAVES_PER_TILE, wpt)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, spec)
    res.set_option(_ffi.RM_OPT_PRUNE, 1)
    res.set_option(_ffi.RM_OPT_REFILL_MIN, refill)
    res.set_materials([(0.4, 0.7, 0.1)])


def _reset(res):
    res.set_option(_ffi.RM_OPT_WAVES_PER_TILE, 0)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_PRUNE, 0)
    res.set_option(_ffi.RM_OPT_REFILL_MIN, 0)


def _draw(res, oracle, name, cam, W, H):
    cc, w, u, pos, ref = reference(oracle, name, cam, W, H)
    res.set_limits(CAMERAS[cam][1])
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_program(cc, w)
    return res.draw(W, H), ref


@pytest.mark.parametrize("wpt", [1, 2, 4, 8])
@pytest.mark.parametrize("name", FRAME_PROGRAMS)
def test_frames_are_the_oracles(res, oracle, name, wpt):
    """one program, one number of waves per tile: interpreter and generated kernel x refill threshold x frame size, still camera"""
    try:
        for spec in (0, 2):
            for refill in (1, 16, 64):
                _configure(res, wpt, spec, refill)
                for W, H in SIZES:
                    img, ref = _draw(res, oracle, name, "still", W, H)
                    try:
                        assert_same(img, ref)
                    except AssertionError as e:
                        raise AssertionError("%s, %d waves per tile, specialize %d, refill %d, %dx%d: %s" % (name, wpt, spec, refill, W, H, e))
                if spec == 2:
                    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 1 and res.info(_ffi.RM_INFO_PRUNED) == 1, (name, wpt)
    finally:
        _reset(res)


def test_the_scenes_are_what_they_are_for(oracle):
    """the tiny sphere covers less than a 2x2 block of the 64x64 frame and is hit; the slab is a sliver at most three pixels wide inside one column of tiles; the
    cameras of CAMERAS start their rays the three ways"""
    cc, w, u, pos, ref = reference(oracle, "tiny_sphere", "still", 64, 64)
    green = ref[28:36, 28:36, 1] > ref[28:36, 28:36, 2]         # (the object's albedo (0.4, 0.7, 0.1) against floor and sky)
    assert 0 < green.sum() <= 4, int(green.sum())
    cc, w, u, pos, ref = reference(oracle, "edge_on_box", "still", 64, 64)
    assert abs(float(pos[0])) < 1e-3 and abs(float(pos[1])) < 1e-3, pos
    for y in (20, 32, 40):
        row = ref[y, :, 1] > ref[y, :, 2]
        assert 1 <= row.sum() <= 3 and row[32:40].sum() == row.sum(), row.astype(int).tolist()
    for name in ("g32", "far"):
        cc, w, _ = A.program(oracle, name)
        f0 = {}
        for cam in CAMERAS:
            p = np.array(_uniforms(oracle, name, cam, 64, 64)[1], dtype=F)
            f0[cam] = float(scene_f64.map_scene(cc, w, 100.0, p[None])[0])
        assert f0["inside"] < -0.01 and f0["beyond"] > CAMERAS["beyond"][1][1] and f0["r50"] > 40.0 and 0.01 < f0["still"] < 5.0, (name, f0)


@pytest.mark.parametrize("cam", ["inside", "beyond", "r50"])
@pytest.mark.parametrize("name", ["g32", "far"])
def test_cameras(res, oracle, name, cam):
    W, H = 40, 24
    try:
        for wpt in (1, 2, 4, 8):
            for spec in (0, 2):
                for refill in (1, 16, 64):
                    _configure(res, wpt, spec, refill)
                    img, ref = _draw(res, oracle, name, cam, W, H)
                    try:
                        assert_same(img, ref)
                    except AssertionError as e:
                        raise AssertionError("%s / %s, %d waves per tile, specialize %d, refill %d: %s" % (name, cam, wpt, spec, refill, e))
    finally:
        _reset(res)


@pytest.mark.parametrize("spec", [0, 2], ids=["interpreter", "generated"])
def test_consecutive_draws_and_a_batch_of_three(res, oracle, spec):
    try:
        for wpt in (1, 4):
            _configure(res, wpt, spec, 16)
            for _ in range(2):                                   # two draws on one context
                img, ref = _draw(res, oracle, "g32", "still", 64, 64)
                assert_same(img, ref)
            W, H = 32, 24
            cams = ("still", "r50", "inside")
            refs = [reference(oracle, "g32", cam, W, H) for cam in cams]
            res.set_limits(LIM)
            res.set_program(refs[0][0], refs[0][1])
            res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(refs[0][2])))
            batch = res.draw_batch([_ffi.Uniforms.from_buffer_copy(bytes(r[2])) for r in refs], W, H)
            for i, r in enumerate(refs):
                assert_same(batch[i], r[4])
    finally:
        _reset(res)


# ---- (c) the rule fires -------------------------------------------------------------------------------------------------------------
# Leaves evaluated by the pruned generated kernel on g32, 64x64, still camera, 4 waves per tile (RM_JIT_PRUNE_STATS=1: the kernel
# counts them per wave, RM_OPT_WAVE_STATS reads them back; tap phases evaluate without counting).  Which wave claims which batch
# varies from run to run, and with it which anchor a batch meets.  profiles/r22_first_step_anchor_ab.txt: the parent commit
# counts PARENT_LEAVES on this frame, this rule LEAVES_SEEN in five runs of the same job; the bound stands above the largest of the
# five by more than their spread and below the parent.
PARENT_LEAVES = (33240, 33445, 33518, 33297, 33925, 33273)       # two contexts, three draws each
LEAVES_SEEN = (29913, 30011, 29786, 30097, 30025)                 # first draws of five contexts; all fifteen draws: 29786 .. 30271
LEAVES_BOUND = 31500                                              # 30271 + 2.5 x (30271 - 29786); the parent's smallest - 1740


def count_leaves(res, oracle, monkeypatch):
    monkeypatch.setenv("RM_JIT_PRUNE_STATS", "1")
    _configure(res, 4, 2, 0)
    res.set_option(_ffi.RM_OPT_WAVE_STATS, 1)
    try:
        img, ref = _draw(res, oracle, "g32", "still", 64, 64)
        assert_same(img, ref)
        st = res.wave_stats()
    finally:
        res.set_option(_ffi.RM_OPT_WAVE_STATS, 0)
        _reset(res)
    return int((st[:, 3] >> np.uint64(32)).sum()), int((st[:, 2] & np.uint64(0xFFFFFFFF)).sum())


def test_the_rule_fires(res, oracle, monkeypatch):
    leaves, iters = count_leaves(res, oracle, monkeypatch)
    print("g32 64x64: %d leaves evaluated in %d iterations (parent %s, bound %s)" % (leaves, iters, PARENT_LEAVES, LEAVES_BOUND))
    assert leaves > 0 and iters > 0
    assert leaves <= LEAVES_BOUND
