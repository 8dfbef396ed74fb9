"""The front end of a march step on the device (rm_kernel_v5.h: the unit table's float4 part, "Pruning", the position term along a
ray; DESIGN.md section 5, "The front end of a step").

(a) frames, bit for bit against oracle.cbind.render: a unit the mask skipped that mattered -- a wrong dword of the unit table, a
    threshold that fell short -- changes a pixel.  64x64 and 40x24 (partial tiles); g32, g64, the balanced tree, g8 and g32 a
    thousand units from the origin (where the position term is a hundred times the metric camera's); the still camera, a camera
    inside the solid and one beyond max_dist; 1, 2, 4 and 8 waves per tile, the generated kernel and the interpreter's masked
    loops, refill thresholds 1 and 64.
(b) leaves evaluated on g32 at 64x64 do not exceed the parent commit's: the bound on the threshold's position term makes the
    threshold larger by 1e-5 .. 1e-4, and that must not show (profiles/r25_step_front_end_ab.txt).
The functions themselves are held by tests/test_gpu_wave_reach.py and tests/test_gpu_anchor.py (rm_selftest_cull_waves reads the
unit table in its new arrangement; rm_selftest_anchor the untouched anchor functions), the arithmetic by
tests/test_step_thr_cpu.py, the arrangement by tests/test_unit_table_cpu.py."""
import numpy as np
import pytest

import anchor_ref as A
import scenes
from ray_marching_amd import _ffi, renderer
from test_gpu_anchor import CAMERAS, INSIDE, _configure, _reset, count_leaves
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = ((64, 64), (40, 24))
PROGRAMS = dict(A.PROGRAMS, g8=(scenes.g8, (0.0, 0.0, 0.0)))
FRAME_PROGRAMS = ("g32", "g64", "g32_balanced", "g8", "far")
REFILLS = (1, 64)
# RM_INFO_INTERPRETER_LOOP of the interpreter leg: the masked chain loop (2) for chains of a dozen leaves or more, the masked tree
# loop (4) for the balanced tree -- the two interpreter loops that read the unit table's float4 part and the new threshold.  g8 has
# four leaves and stays with the plain chain loop: its interpreter leg holds the staging of the table alone.
MASKED_LOOP = {"g32": 2, "g64": 2, "far": 2, "g32_balanced": 4}
_REFS = {}


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.set_option(_ffi.RM_OPT_WAVE_STATS, 0)
    r.close()


def reference(oracle, name, cam, W, H):
    """the oracle's frame, rendered once per (program, camera, size) and read-only after"""
    key = (name, cam, W, H)
    if key not in _REFS:
        scene, centre = PROGRAMS[name]
        cc, w = oracle.serialize(*scene())
        target = tuple(np.add(centre, INSIDE)) if cam == "inside" else tuple(centre)
        u = oracle.orbit_uniforms((float(W), float(H)), target=target, radius=CAMERAS[cam][0], events=scenes.STILL_CAMERA_EVENTS)[0]
        img = oracle.render(u, CAMERAS[cam][1], cc, np.asarray(w, dtype=np.uint32), W, H, threads=16)
        img.setflags(write=False)
        _REFS[key] = (cc, np.asarray(w, dtype=np.uint32), u, img)
    return _REFS[key]


def draw(res, oracle, name, cam, W, H):
    cc, w, u, ref = reference(oracle, name, cam, W, H)
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
            for refill in REFILLS:
                _configure(res, wpt, spec, refill)
                for W, H in SIZES:
                    img, ref = draw(res, oracle, name, "still", W, H)
                    try:
                        assert_same(img, ref)
                    except AssertionError as e:
                        raise AssertionError("%s, %d waves per tile, specialize %d, refill %d, %dx%d: %s" % (name, wpt, spec, refill, W, H, e))
                if spec == 2:
                    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 1 and res.info(_ffi.RM_INFO_PRUNED) == 1, (name, wpt)
                elif name in MASKED_LOOP:   # the interpreter leg ran the loop that calls the changed functions
                    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 0 and res.info(_ffi.RM_INFO_INTERPRETER_LOOP) == MASKED_LOOP[name], (name, wpt)
    finally:
        _reset(res)


@pytest.mark.parametrize("cam", ["inside", "beyond"])
@pytest.mark.parametrize("name", ["g32", "far"])
def test_cameras_whose_rays_do_not_take_the_shared_step(res, oracle, name, cam):
    try:
        for W, H in SIZES:
            for wpt in (1, 2, 4, 8):
                for spec in (0, 2):
                    for refill in REFILLS:
                        _configure(res, wpt, spec, refill)
                        img, ref = draw(res, oracle, name, cam, W, H)
                        try:
                            assert_same(img, ref)
                        except AssertionError as e:
                            raise AssertionError("%s / %s, %dx%d, %d waves per tile, specialize %d, refill %d: %s" % (name, cam, W, H, wpt, spec, refill, e))
    finally:
        _reset(res)


# Leaves evaluated by the pruned generated kernel on g32, 64x64, still camera, 4 waves per tile, as tests/test_gpu_anchor.py counts
# them (which wave claims which batch varies from draw to draw).  profiles/r25_step_front_end_ab.txt: the parent commit over fifteen
# draws (five contexts, three draws each) on the GPU that measured this change; this change's own fifteen draws are in the same file.
# The bound is the parent's largest count plus 2.5 times the parent's spread.
PARENT_LEAVES = (30345, 30330, 30450, 30178, 30291,
                 30221, 30537, 30203, 30209, 30173,
                 30129, 29905, 30144, 30195, 30097)
LEAVES_BOUND = 32117            # 30537 + 2.5 x (30537 - 29905)


def test_leaves_evaluated_do_not_exceed_the_parents(res, oracle, monkeypatch):
    leaves, iters = count_leaves(res, oracle, monkeypatch)
    print("g32 64x64: %d leaves evaluated in %d iterations (parent %d .. %d, bound %d)" % (
        leaves, iters, min(PARENT_LEAVES), max(PARENT_LEAVES), LEAVES_BOUND))
    assert LEAVES_BOUND == max(PARENT_LEAVES) + int(round(2.5 * (max(PARENT_LEAVES) - min(PARENT_LEAVES))))
    assert leaves > 0 and iters > 0
    assert leaves <= LEAVES_BOUND
