"""The single-unit path of the generated march kernel (csrc/rm_jit.h "Single-unit steps", RM_JIT_UNIT_WALK) on the device: frames
drawn with the path (the default) and without it (RM_JIT_UNIT_WALK=0) are the same bits, and the oracle's.  A step that takes the
path returns a constant or one leaf's value in place of the whole straight-line code, so a unit classified wrongly -- +inf for a
leaf that mattered, a raw value where the operator would have dropped a NaN -- changes a pixel."""
import numpy as np
import pytest

import fuzz_programs as FZ
import golden_util as G
import scenes
from ray_marching_amd import _ffi, renderer
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

LIM = (0.01, 100.0, 64)
SIZES = ((64, 64), (40, 24))
IDX = G.index()


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.set_option(_ffi.RM_OPT_WAVE_STATS, 0)
    r.close()


def configure(res):
    res.set_option(_ffi.RM_OPT_KERNEL, _ffi.RM_KERNEL_DEFAULT)
    res.set_option(_ffi.RM_OPT_CULL, 1)
    res.set_option(_ffi.RM_OPT_WAVES_PER_TILE, 4)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_PRUNE, 1)
    res.set_materials([(0.4, 0.7, 0.1)])


def draw(res, monkeypatch, knob, cc, w, u, limits, W, H, pruned=True):
    """one frame by the pruned generated kernel; knob None: the default.  (The knob is read when set_program asks for the kernel.)"""
    if knob is None:
        monkeypatch.delenv("RM_JIT_UNIT_WALK", raising=False)
    else:
        monkeypatch.setenv("RM_JIT_UNIT_WALK", str(knob))
    configure(res)
    res.set_limits(limits)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_program(cc, w)
    img = res.draw(W, H)
    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 1 and (res.info(_ffi.RM_INFO_PRUNED) == 1 or not pruned), res.jit_log()
    return img


def both_are(res, monkeypatch, cc, w, u, limits, W, H, ref, what):
    for knob in (0, None):
        try:
            assert_same(draw(res, monkeypatch, knob, cc, w, u, limits, W, H), ref)
        except AssertionError as e:
            raise AssertionError("%s, %dx%d, RM_JIT_UNIT_WALK %s: %s" % (what, W, H, "0" if knob == 0 else "default", e))


def has_path(cc, w):
    return "map_scene_walk" in renderer.jit_source(cc, w, prune=True)


# ---- the scenes of the benchmark and the goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32", "g32_balanced", "g8", "g64"])
def test_scene_frames_are_the_oracles_with_and_without_the_path(res, oracle, monkeypatch, name):
    cc, w = oracle.serialize(*scenes.SCENES[name]())
    w = np.asarray(w, dtype=np.uint32)
    assert has_path(cc, w) == (name != "g32_balanced")            # (a tree whose units are not its first records keeps the straight-line code)
    for W, H in SIZES:
        u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
        ref = oracle.render(u, LIM, cc, w, W, H, threads=16)
        both_are(res, monkeypatch, cc, w, u, LIM, W, H, ref, name)


@pytest.mark.parametrize("name", ["g32_64", "g32_balanced_64", "g8_64", "g8_inside_56", "g64_48x40"])
def test_goldens_with_and_without_the_path(res, monkeypatch, name):
    """the committed frames (g8_inside: the camera inside the solid, every ray starts as a hit)"""
    e = IDX[name]
    both_are(res, monkeypatch, e["cmd_count"], G.words(e), G.uniforms_bytes(e), tuple(e["limits"]), e["W"], e["H"], G.load_image(e), name)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("cls", ["chain", "tree"])
def test_seeded_lattice_programs(res, oracle, monkeypatch, cls, seed):
    c = FZ.case(oracle, cls, seed)
    assert c.info["prunable"] == 1, FZ.describe(c)
    for W, H in SIZES:
        u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=c.events)
        ref = oracle.render(u, LIM, c.cc, c.words, W, H, threads=16)
        both_are(res, monkeypatch, c.cc, c.words, u, LIM, W, H, ref, FZ.describe(c))


# ---- one unit at a time ------------------------------------------------------------------------------------------------------------------
# S0 u B1 - S2 u B3 with the solids far apart, and a camera that orbits one primitive closely: its rays are near that primitive alone
# for most of their march, so the masks hold one bit -- the pushed first leaf (its raw value), the last leaf (through the Union's
# v_min_f32 with +inf).  The subtracted sphere carves a corner of B1; the camera at it sees steps that need B1, S2 or both.  A mask
# of S2 ALONE does not arise on the device: thr >= |F| >= the value of the nearest solid leaf, which is therefore always kept (the
# simulation met none either); that class -- +inf, nothing evaluated -- is held to the model in tests/test_jit_unit_walk_cpu.py.
CENTRES = ((-6.0, 0.0, 0.0), (-2.0, 0.0, 0.0), (-1.4, 0.5, 0.5), (6.0, 0.0, 0.0))


def spread_chain(radius2=0.7, extent3=(0.6, 0.5, 0.6)):
    t = scenes._Tab()
    a = t.op(scenes.UNION, t.sphere(CENTRES[0], 0.8), t.box(CENTRES[1], (0.6, 0.6, 0.6)))
    a = t.op(scenes.SUBTRACTION, a, t.sphere(CENTRES[2], radius2))
    return t.nodes, t.op(scenes.UNION, a, t.box(CENTRES[3], extent3))


def single_unit_evaluations(res):
    st = res.wave_stats()
    return int((st[:, 3] >> np.uint64(32)).sum()), int((st[:, 2] & np.uint64(0xFFFFFFFF)).sum())


@pytest.mark.parametrize("unit", [0, 2, 3], ids=["pushed_first_leaf", "subtracted_leaf", "last_leaf"])
def test_the_single_unit_is_each_kind_of_leaf_in_turn(res, oracle, monkeypatch, unit):
    cc, w = oracle.serialize(*spread_chain())
    w = np.asarray(w, dtype=np.uint32)
    assert has_path(cc, w)
    W, H = 64, 64
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), target=CENTRES[unit], radius=2.0, events=scenes.STILL_CAMERA_EVENTS)
    ref = oracle.render(u, LIM, cc, w, W, H, threads=16)
    both_are(res, monkeypatch, cc, w, u, LIM, W, H, ref, "unit %d" % unit)
    # ... and the path is what drew it: the statistics kernel (the same code with its counters) counts the evaluations that took it
    monkeypatch.setenv("RM_JIT_PRUNE_STATS", "5")
    res.set_option(_ffi.RM_OPT_WAVE_STATS, 1)
    try:
        assert_same(draw(res, monkeypatch, None, cc, w, u, LIM, W, H), ref)
        taken, iters = single_unit_evaluations(res)
    finally:
        res.set_option(_ffi.RM_OPT_WAVE_STATS, 0)
    print("unit %d: %d of %d wave-iterations took the single-unit path" % (unit, taken, iters))
    assert iters > 0 and (taken > 0 or unit == 2)


@pytest.mark.parametrize("what", ["nan_radius", "infinite_extent"])
def test_non_finite_parameters_draw_the_same_bits(res, oracle, monkeypatch, what):
    """a leaf whose value is NaN or -inf everywhere: the frame with the path is the frame without it"""
    nodes, root = spread_chain(radius2=float("nan")) if what == "nan_radius" else spread_chain(extent3=(0.6, float("inf"), 0.6))
    cc, w = oracle.serialize(nodes, root)
    w = np.asarray(w, dtype=np.uint32)
    for W, H in SIZES:
        for unit in (2, 3):
            u, *_ = oracle.orbit_uniforms((float(W), float(H)), target=CENTRES[unit], radius=2.0, events=scenes.STILL_CAMERA_EVENTS)
            off = draw(res, monkeypatch, 0, cc, w, u, LIM, W, H, pruned=False)
            on = draw(res, monkeypatch, None, cc, w, u, LIM, W, H, pruned=False)
            assert on.tobytes() == off.tobytes(), "%s, camera at unit %d, %dx%d: %d pixels differ" % (
                what, unit, W, H, int((on.view(np.uint32) != off.view(np.uint32)).any(axis=-1).sum()))


# ---- the path fires ------------------------------------------------------------------------------------------------------------------------
# Evaluations of g32 at 64x64 (still camera, 4 waves per tile) that took the single-unit path, counted by the statistics kernel
# (RM_JIT_PRUNE_STATS=5 + RM_OPT_WAVE_STATS).  Which wave claims which batch varies from run to run, and with it the anchors and the masks.
# profiles/r23_unit_walk_ab.txt: five contexts, three draws each gave TAKEN_SEEN; the floor stands a few spreads below the smallest.
TAKEN_SEEN = (2052, 2213)      # smallest and largest of the fifteen counts, of 7139 .. 7295 wave-iterations
TAKEN_FLOOR = 1650             # 2052 - 2.5 x (2213 - 2052)


def count_taken(res, oracle, monkeypatch, knob):
    cc, w = oracle.serialize(*scenes.g32())
    w = np.asarray(w, dtype=np.uint32)
    u, *_ = oracle.orbit_uniforms((64.0, 64.0), events=scenes.STILL_CAMERA_EVENTS)
    monkeypatch.setenv("RM_JIT_PRUNE_STATS", "5")
    res.set_option(_ffi.RM_OPT_WAVE_STATS, 1)
    try:
        draw(res, monkeypatch, knob, cc, w, u, LIM, 64, 64)
        return single_unit_evaluations(res)
    finally:
        res.set_option(_ffi.RM_OPT_WAVE_STATS, 0)


def test_the_path_fires(res, oracle, monkeypatch):
    taken, iters = count_taken(res, oracle, monkeypatch, None)
    print("g32 64x64: %d of %d wave-iterations took the single-unit path (seen %s, floor %d)" % (taken, iters, TAKEN_SEEN, TAKEN_FLOOR))
    assert iters > 0 and TAKEN_FLOOR > 0
    assert taken >= TAKEN_FLOOR


def test_without_the_path_the_counter_stays_zero(res, oracle, monkeypatch):
    taken, iters = count_taken(res, oracle, monkeypatch, 0)
    assert iters > 0 and taken == 0
