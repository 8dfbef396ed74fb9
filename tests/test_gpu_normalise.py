"""The short normalisation of the march kernel and the pre-pass ("Short division"): rm_selftest_div on the
device, and whole frames against the oracle, bit for bit, under cameras that keep every wave on the short form, cameras that put
exact zeros into the ray directions, and uniform blocks that push rays across the guard's bounds or make them NaN -- with a numpy
restatement of the guard over the oracle's own ray arithmetic showing that both forms really ran."""
import ctypes as C

import numpy as np
import pytest

import div_ref as D
import prepass_ref as P
import scenes
from ray_marching_amd import _ffi, renderer, shard
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
F = np.float32
LIMITS = (0.01, 100.0, 96)
SIZES = [(64, 48), (40, 24)]
SCENES = ("g8", "g32", "mat_mix")
N_SEEDED, SEED = 1 << 20, 20261


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


# ---- (1) the primitives on the device -------------------------------------------------------------------------------------------
def special_pairs():
    sp = [0.0, -0.0, 1.0, -1.0, 3.0, 0.1, 1e-45, -1e-45, 1e-38, 1.17549435e-38, 3.4028235e38, np.inf, -np.inf, np.nan,
          2.0 ** -48, 2.0 ** -49, 2.0 ** 44, 2.0 ** 45, 2.0 ** -79, 2.0 ** -80, 2.0 ** 78, 2.0 ** 77, 1.9999999, 1.9999995, 0.99999994]
    a, b = np.meshgrid(np.array(sp, F), np.array(sp, F))
    rng = np.random.default_rng(77)
    v = rng.normal(size=(4096, 3)).astype(F) * F(2.0) ** rng.integers(-20, 21, (4096, 1)).astype(F)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return (np.ascontiguousarray(np.concatenate([a.ravel(), v[:, 0], v[:, 1], v[:, 2]]), F),
            np.ascontiguousarray(np.concatenate([b.ravel(), ln, ln, ln]), F))


def test_short_division_on_the_device(res):
    a, b = special_pairs()
    out = np.zeros(8, np.uint64)
    _ffi.check(res._h, _ffi.hip_lib().rm_selftest_div(res._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size,
                                                       SEED, N_SEEDED, out.ctypes.data_as(C.POINTER(C.c_uint64))))
    print("rm_selftest_div: %s" % [int(x) for x in out])
    assert out[0] == 0, "refined reciprocal differs from 1.0f / b, first at b = 0x%08x" % int(out[1])
    assert out[4] == 0, "short quotient differs from a / b, first at a = 0x%08x b = 0x%08x" % (int(out[5]) >> 32, int(out[5]) & 0xFFFFFFFF)
    # the only b of [2^-48, 2^44] on the generic form: the top four significands of each of its 92 binades
    assert out[3] == 0 and out[2] == 4 * 92
    sa, sb = D.seeded_pairs(SEED, N_SEEDED)
    slow_given, slow_seeded = int(D.guard_bad_np(a, b).sum()), int(D.guard_bad_np(sa, sb).sum())
    assert (int(out[6]), int(out[7])) == (slow_given, slow_seeded)
    assert 0.2 * N_SEEDED < slow_seeded < 0.8 * N_SEEDED and 0 < slow_given < a.size - 8192     # both forms were exercised


# ---- (2) frames --------------------------------------------------------------------------------------------------------------------
def ray_guard(u, W, H):
    """(slow, zero): per sample of the frame, whether gen_ray_at's normalisation falls outside the guard, and whether a
    numerator is an exact zero.  The oracle's ray arithmetic (gbuffer_ref.camera_rays) up to the normalisation."""
    ud = P.udict(u)
    ve = np.asarray(ud["viewport_extent"], F)
    ip, iv = np.asarray(ud["inv_proj"], F), np.asarray(ud["inv_view"], F)

    def matvec(m, x, y, z, w):
        return [((m[k] * x + m[4 + k] * y) + m[8 + k] * z) + m[12 + k] * w for k in range(4)]

    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    slow, zero = [], []
    with np.errstate(all="ignore"):
        ro = matvec(iv, F(0), F(0), F(0), F(1))
        sx = ((px.ravel().astype(F) + F(0.5)) / F(W)) * F(2) - F(1)
        sy = F(1) - ((py.ravel().astype(F) + F(0.5)) / F(H)) * F(2)
        for s in range(16):
            ox = ((F(s // 4) + F(0.5)) / F(4) - F(0.5)) / ve[0] * F(2)
            oy = ((F(s % 4) + F(0.5)) / F(4) - F(0.5)) / ve[1] * F(2)
            pw = matvec(iv, *matvec(ip, sx + ox, sy + oy, np.full(sx.size, F(-1)), np.full(sx.size, F(1))))
            e = [pw[k] - ro[k] for k in range(4)]
            rad = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]
            num = np.stack(e[:3], axis=-1)
            slow.append(D.guard_bad_np(num, np.sqrt(rad), rad))
            zero.append((num == 0).any(axis=-1))
    return np.concatenate(slow), np.concatenate(zero)


def axis_aligned(oracle, W, H):
    """A camera at (0, 0.2, 5) looking down -z with no rotation at all, its frustum shifted by a fraction of a pixel so that one
    sample column has pt_view.x = 0 exactly: those rays have a zero x component, and the boxes' faces give zero normal components."""
    u = P.clone(oracle.orbit_uniforms((float(W), float(H)))[0])
    M = np.eye(4)
    M[:3, 3] = (0.0, 0.2, 5.0)
    P.store_matrix(u.inv_view, M)
    m = P.perspective_inverse(oracle, W / H, 0.7853981633974483, 1.0)
    for i in range(16):
        u.inv_proj[i] = float(m[i])
    assert m[4] == 0 and m[8] == 0 and m[12] == 0
    sx = ((F(W // 2 + 3) + F(0.5)) / F(W)) * F(2) - F(1)
    ox = ((F(1) + F(0.5)) / F(4) - F(0.5)) / F(u.viewport_extent[0]) * F(2)
    u.inv_proj[12] = float(-(F(m[0]) * (sx + ox)))
    return u


def view_scaled(u, f, at_origin=False):
    """inv_view's rotation columns times f: |pt_world - ro| scales by f.  at_origin: the camera moves to the origin and row 3
    becomes (0, 0, 0, 1), without which a small f leaves only the cancellation noise of the translation."""
    v = P.clone(u)
    for i in range(12):
        v.inv_view[i] = float(F(v.inv_view[i]) * F(f))
    if at_origin:
        v.inv_view[12] = v.inv_view[13] = v.inv_view[14] = 0.0
        v.inv_view[15] = 1.0
    return v


def cameras(oracle, W, H):
    """[(name, block, kind)]; kind: 'fast' every sample on the short form, 'zeros' fast with exact zero numerators, 'mixed' both
    forms within the frame, 'slow' every sample on the generic form."""
    blocks = P.variants(oracle, W, H)
    still = blocks["still"]
    return [("metric", still, "fast"),
            ("axis_aligned", axis_aligned(oracle, W, H), "zeros"),
            ("view_scaled_3", blocks["view_scaled_3"], "fast"),
            # |pt_world - ro| straddles 2^-48 resp. 2^44 across the frame: rays on both sides of the guard's bounds in one frame
            ("view_tiny", view_scaled(still, 2.0 ** -48 * 0.9, at_origin=True), "mixed"),
            ("view_huge", view_scaled(still, 2.0 ** 44 * 0.9), "mixed"),
            ("view_denormal", view_scaled(still, 2.0 ** -70, at_origin=True), "slow"),
            ("nan_proj", blocks["nan_proj"], "slow"),
            ("nan_rays", blocks["nan_rays"], "fast")]


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "40x24"])
def test_the_cameras_take_the_paths_they_are_here_for(oracle, size):
    W, H = size
    seen = set()
    for name, u, kind in cameras(oracle, W, H):
        slow, zero = ray_guard(u, W, H)
        n_slow, n_fast, n_zero = int(slow.sum()), int((~slow).sum()), int((zero & ~slow).sum())
        print("%-14s %dx%d: %d samples on the short form (%d with a zero numerator), %d on the generic form" % (name, W, H, n_fast, n_zero, n_slow))
        if kind in ("fast", "zeros"):
            assert n_slow == 0
        if kind == "zeros":
            assert n_zero >= H
        if kind == "mixed":
            assert n_slow >= 100 and n_fast >= 100
        if kind == "slow":
            assert n_fast == 0
        seen.add(kind)
    assert seen == {"fast", "zeros", "mixed", "slow"}


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "40x24"])
@pytest.mark.parametrize("scene", SCENES)
def test_frames_match_the_oracle(res, oracle, scene, size):
    W, H = size
    cc, w = oracle.serialize(*{**scenes.SCENES, **scenes.MAT_SCENES}[scene]())
    mats = scenes.MATERIAL_TABLE if scene in scenes.MAT_SCENES else None
    res.set_limits(LIMITS)
    res.set_program(cc, np.asarray(w, dtype=np.uint32))
    try:
        for name, u, _ in cameras(oracle, W, H):
            ref = oracle.render(u, LIMITS, cc, w, W, H, threads=16, materials=mats)
            res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
            for spec in (2, 0):
                res.set_option(_ffi.RM_OPT_SPECIALIZE, spec)
                try:
                    assert_same(res.draw(W, H), ref)
                    img = np.zeros_like(ref)
                    for rank in range(2):
                        shard.scatter_strips(img, res.draw_strips(W, H, 8, rank, 2), H, rank, 2, 8)
                    assert_same(img, ref)
                except AssertionError as e:
                    raise AssertionError("%s / %s / %dx%d, specialise %d: %s" % (scene, name, W, H, spec, e)) from None
    finally:
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
