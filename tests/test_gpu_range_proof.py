"""The range proofs of the generated march kernel on the device (csrc/rm_interp.h "Range proofs"): a program whose facts make some
range guards of the square roots and divisions unnecessary runs a kernel compiled without them, every other program the guarded kernel
-- and the frames are the same bits either way, the oracle's.  RM_JIT_RANGE_PROOF=0 (read at every launch) forces the guarded kernel;
RM_INFO_RANGE_PROOF says which one ran."""
import numpy as np
import pytest

import golden_util as G
import scenes
from ray_marching_amd import _ffi, renderer
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

LIM = (0.01, 100.0, 64)
SIZES = ((64, 64), (48, 40))
IDX = G.index()


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


def configure(res, cc, w, u, limits, materials=((0.4, 0.7, 0.1),)):
    res.set_option(_ffi.RM_OPT_KERNEL, _ffi.RM_KERNEL_DEFAULT)
    res.set_option(_ffi.RM_OPT_CULL, 1)
    res.set_option(_ffi.RM_OPT_WAVES_PER_TILE, 4)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_PRUNE, 2)
    res.set_materials(list(materials))
    res.set_limits(limits)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_program(cc, np.asarray(w, dtype=np.uint32))


def draw(res, monkeypatch, forced_guarded, W, H):
    """one frame of the configured context -> (image, RM_INFO_RANGE_PROOF)"""
    if forced_guarded:
        monkeypatch.setenv("RM_JIT_RANGE_PROOF", "0")
    else:
        monkeypatch.delenv("RM_JIT_RANGE_PROOF", raising=False)
    img = res.draw(W, H)
    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 1, res.jit_log()
    return img, int(res.info(_ffi.RM_INFO_RANGE_PROOF))


def thin_boxes():
    """a lattice of sixteen boxes with half-extents 2^-23 .. 2^-20 around the origin, every fourth one subtracted"""
    t = scenes._Tab()
    prims = []
    for k in range(16):
        c = [((k % 4) - 1.5) * 3.0e-6, ((k // 4) % 2 - 0.5) * 2.0e-6, ((k // 8) - 0.5) * 3.0e-6]
        h = [2.0 ** -(23 - (k + a) % 4) for a in range(3)]
        prims.append(t.box(c, h))
    return t.nodes, scenes._fold_left(t, prims)


# ---- proved, forced guarded, oracle: the same bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32", "g64", "g32_balanced", "thin_boxes"])
def test_proved_and_guarded_kernels_draw_the_oracles_frame(res, oracle, monkeypatch, name):
    thin = name == "thin_boxes"
    cc, w = oracle.serialize(*(thin_boxes() if thin else scenes.SCENES[name]()))
    limits = (1.0e-8, 100.0, 64) if thin else LIM   # (the thin boxes would all be "hit" from anywhere near with min_dist = 0.01)
    cameras = [dict(target=(0, 0, 0), radius=1.2e-5), dict()] if thin else [dict()]
    for W, H in SIZES:
        for cam in cameras:
            u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS, **cam)
            ref = oracle.render(u, limits, cc, w, W, H, threads=16)
            configure(res, cc, w, u, limits)
            proved, ran = draw(res, monkeypatch, False, W, H)
            assert ran == 1, "%s: the variant did not run" % name
            guarded, ran0 = draw(res, monkeypatch, True, W, H)
            assert ran0 == 0
            assert_same(proved, ref)
            assert_same(guarded, ref)


# ---- hostile launches: the proved kernel equals the guarded one byte for byte, NaN payloads included -----------------
def poisoned(u, field, index, value):
    a = np.frombuffer(bytes(u), dtype=np.float32).copy()
    a[(4 if field == "inv_proj" else 20) + index] = value
    return a.tobytes()


@pytest.mark.parametrize("field,index,value", [("inv_proj", 0, np.nan), ("inv_proj", 13, np.inf), ("inv_proj", 5, -np.inf),
                                               ("inv_view", 1, np.nan), ("inv_view", 10, np.inf), ("inv_view", 15, np.nan),
                                               ("inv_view", 7, np.inf), ("inv_view", 12, np.nan), ("inv_view", 13, -np.inf)])
def test_non_finite_uniforms_leave_the_same_bytes(res, oracle, monkeypatch, field, index, value):
    W, H = 40, 24
    cc, w = oracle.serialize(*scenes.SCENES["g32"]())
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    configure(res, cc, w, poisoned(u, field, index, value), LIM)
    a, ran = draw(res, monkeypatch, False, W, H)
    b, ran0 = draw(res, monkeypatch, True, W, H)
    assert ran == 1 and ran0 == 0      # (nothing the variant relies on depends on the uniforms: it is the kernel's to survive them)
    assert a.tobytes() == b.tobytes()


def test_camera_inside_a_solid_leaves_the_same_bytes(res, oracle, monkeypatch):
    """every ray starts as a hit (START_HIT): the normal taps and the resolve alone"""
    W, H = 40, 24
    nodes, root = scenes.SCENES["g32"]()
    cc, w = oracle.serialize(nodes, root)
    centre = nodes[0][1][:3]                     # the first sphere of the grid (radius >= 0.35)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), target=tuple(centre), radius=0.05, events=scenes.STILL_CAMERA_EVENTS)
    ref = oracle.render(u, LIM, cc, w, W, H, threads=16)
    configure(res, cc, w, u, LIM)
    a, ran = draw(res, monkeypatch, False, W, H)
    b, ran0 = draw(res, monkeypatch, True, W, H)
    assert ran == 1 and ran0 == 0
    assert a.tobytes() == b.tobytes()
    assert_same(a, ref)
    assert float(a[..., :3].min()) > 0.0    # every pixel a lit surface: no sky


def test_an_infinite_colour_without_a_material_table(res, oracle, monkeypatch):
    """What the one upper guard the resolve keeps (on the green root) is for.  Four spheres of radius ~1e-30 sit exactly on the four
    tap positions of a hit at the camera (START_HIT: f0 < min_dist, every ray hits at ro): the tap values are -r_t, the normal's
    components a few 1e-30, their squares underflow, shade_hit divides by a zero root, and with the radii chosen so that every
    product of the dot has the same sign the code is +inf -- a colour outside the short root's range, from no material table."""
    W, H = 40, 24
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    F = np.float32
    ro = np.frombuffer(bytes(u), dtype=F)[20 + 12:20 + 15].copy()
    e = F(0.0001)
    taps = [(ro[0] + sx * e, ro[1] + sy * e, ro[2] + sz * e) for sx, sy, sz in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]   # wgsl:138-141
    want = np.sign(ro.astype(np.float64) - np.array([2.0, -5.0, 3.0]))          # the signs of pos - light_position
    import itertools
    for r in itertools.product((1, 2, 3, 4, 5), repeat=4):                     # f_t = -r_t: n = (f0-f1-f2+f3, -f0-f1+f2+f3, -f0+f1-f2+f3)
        n = np.array([-r[0] + r[1] + r[2] - r[3], r[0] + r[1] - r[2] - r[3], r[0] - r[1] + r[2] - r[3]])
        if np.all(n * want > 0):
            break
    else:
        raise AssertionError("no radii give the normal the light's signs")
    t = scenes._Tab()
    acc = scenes._fold_left(t, scenes._grid_prims(t, 4, 4, 0x5DF00020))
    for c, k in zip(taps, r):
        acc = t.op(scenes.UNION, acc, t.sphere([float(v) for v in c], k * 1.0e-30))
    cc, w = oracle.serialize(t.nodes, acc)
    ref = oracle.render(u, LIM, cc, w, W, H, threads=16)
    configure(res, cc, w, u, LIM)
    a, ran = draw(res, monkeypatch, False, W, H)
    b, ran0 = draw(res, monkeypatch, True, W, H)
    assert ran == 1 and ran0 == 0
    assert np.isposinf(ref[..., :3]).all(), "the program does not reach an infinite colour: %r" % (ref[0, 0],)
    assert a.tobytes() == b.tobytes()
    assert_same(a, ref)


# ---- the facts pick the kernel and never the frame ------------------------------------------------------------------------------------
# The variant rests on facts of the PROGRAM alone (box sizes, no material table): a box size outside the lemma keeps the guarded kernel.
# Coordinates of 3e18, a max_dist of 1e30 and uniforms in device memory are none of its business -- the kernel keeps the upper side of
# the leaves' guard, which is what such launches can trip -- so they run the variant, and it must draw them as the oracle does.
def grid_plus_box(centre=(0.3, 1.2, -0.4), half=(0.3, 0.25, 0.2)):
    """g32's primitives and one more box: ONE structure for every case below (the parameters alone differ)"""
    t = scenes._Tab()
    acc = scenes._fold_left(t, scenes._grid_prims(t, 4, 4, 0x5DF00020))
    return t.nodes, t.op(scenes.UNION, acc, t.box(centre, half))


CASES = {
    "sane": dict(ran=1),
    "box_half_extent_1e-9": dict(scene=dict(half=(1.0e-9, 0.25, 0.2)), ran=0),
    "box_half_extent_0": dict(scene=dict(half=(0.3, 0.0, 0.2)), ran=0),
    "box_half_extent_-1e-8": dict(scene=dict(half=(0.3, 0.25, -1.0e-8)), ran=0),
    "non_finite_parameter": dict(scene=dict(half=(0.3, float("inf"), 0.2)), ran=0),
    "coordinates_3e18": dict(scene=dict(centre=(3.0e18, 1.2, -0.4)), ran=1),
    "max_dist_1e30": dict(limits=(0.01, 1.0e30, 64), ran=1),
    "frames_batch": dict(batch=True, ran=1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_preconditions_pick_the_kernel_and_never_the_frame(res, oracle, monkeypatch, case):
    W, H = 48, 40
    spec = CASES[case]
    cc, w = oracle.serialize(*grid_plus_box(**spec.get("scene", {})))
    limits = spec.get("limits", LIM)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    ref = oracle.render(u, limits, cc, w, W, H, threads=16)
    configure(res, cc, w, u, limits)
    monkeypatch.delenv("RM_JIT_RANGE_PROOF", raising=False)
    if spec.get("batch"):
        img = res.draw_batch([_ffi.Uniforms.from_buffer_copy(bytes(u))], W, H)[0]   # uniforms in device memory
    else:
        img = res.draw(W, H)
    assert res.info(_ffi.RM_INFO_SPECIALIZED) == 1, res.jit_log()
    assert res.info(_ffi.RM_INFO_RANGE_PROOF) == spec["ran"], case
    assert_same(img, ref)
    if spec["ran"] and not spec.get("batch"):
        guarded, ran0 = draw(res, monkeypatch, True, W, H)
        assert ran0 == 0
        assert_same(guarded, ref)


def test_the_material_kernel_keeps_its_guards_and_its_golden_frame(res, monkeypatch):
    e = IDX["mat_mix_64x48"]
    configure(res, e["cmd_count"], G.words(e), G.uniforms_bytes(e), tuple(e["limits"]), materials=scenes.MATERIAL_TABLE)
    img, ran = draw(res, monkeypatch, False, e["W"], e["H"])
    assert ran == 0
    assert_same(img, G.load_image(e))
