"""The short normalisation of the march kernel and the pre-pass ("Short division"): rm_selftest_div on the
device, and whole frames against the oracle, bit for bit, under cameras that keep every wave on the short form, cameras that put
exact zeros into the ray directions, and uniform blocks that push rays across the guard's bounds or make them NaN -- with a numpy
restatement of the guard over the oracle's own ray arithmetic showing that both forms really ran.  Part (3) does the same for
shade_hit's two normalisations: scenes whose tap-sum normals and light vectors lie on either side of the guard's bounds."""
import ctypes as C

import numpy as np
import pytest

import div_ref as D
import gbuffer_ref as G
import prepass_ref as P
import scenes
from oracle import rm_oracle_np as onp
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


# ---- (3) frames whose normals and light vectors leave the guard ---------------------------------------------------------------------
# Only a Plane has a gradient other than 1 (dot(p, n) + h, |n| free): behind it the four taps see the plane alone and their sum is
# about 4e-4 |n|.  Its value is huge in front of it, so the solids' distances drive the march and the rays step across the plane:
# the hits lie at varied depths behind it.  All scenes share one program structure (one specialised kernel).
K44 = 2.0 ** 44 / 4e-4                                         # |n| whose tap sum has length 2^44, the guard's upper bound
FAR_PLANE = ((0.0, 1.0, 0.0), 1000.0)                          # never the minimum: fills the second plane's slot


def _scaled(v, length):
    v = np.array(v, np.float64)
    return tuple(float(F(x)) for x in v / np.linalg.norm(v) * length)


def _wall(f):                                                  # solid behind z = -1.2, a little tilted; tap sums of length f 2^44
    return _scaled((0.10, 0.05, 1.0), K44 * f), float(F(1.2 * K44 * f))


def _side(f):                                                  # solid right of x = 1.8
    return _scaled((-1.0, 0.05, 0.1), K44 * f), float(F(1.8 * K44 * f))


def _program(oracle, planes, sphere=((-0.7, 0.0, 0.0), 0.8), box=((0.9, -0.4, 0.2), (0.5, 0.8, 0.5))):
    t = scenes._Tab()
    root = t.op(scenes.UNION, t.sphere(*sphere), t.box(*box))
    for n, h in planes:
        root = t.op(scenes.UNION, root, t.plane(n, h))
    return oracle.serialize(t.nodes, root)


def _large_block(oracle, still, S=2.0 ** 40, C=(2.0 ** 45 * 0.6, 2.0 ** 45 * 0.3, 2.0 ** 45 * 0.7)):
    """The still camera and the solids moved to C (magnitude 2^45) and scaled by S, max_dist with them.  A position there has an
    ulp of 2^22: the four taps coincide, the normal is exactly 0 (0 / 0: NaN) and the light vector is longer than 2^44.  A ray
    never converges onto a solid at that resolution; the hits come from a plane of |n| = 3, which the march oversteps."""
    u, C = P.clone(still), np.array(C)
    for k in range(3):
        u.inv_view[12 + k] = float(F(C[k] + S * still.inv_view[12 + k]))
    n = np.array(_scaled((0.10, 0.05, 1.0), 3.0), np.float64)
    h = float(F(-(n @ (C + S * np.array([0.0, 0.0, -1.2])))))
    sphere = (tuple(float(F(x)) for x in C + S * np.array([-0.7, 0.0, 0.0])), float(F(0.8 * S)))
    box = (tuple(float(F(x)) for x in C + S * np.array([0.9, -0.4, 0.2])), tuple(float(F(x * S)) for x in (0.5, 0.8, 0.5)))
    return u, _program(oracle, [(tuple(n), h), FAR_PLANE], sphere, box), (0.01, float(F(100.0 * S)), 96)


def shade_scenes(oracle, W, H):
    """[(name, uniform block, (cmd_count, words), limits, classes)]; classes: what the scene is there for, among 'n_in' (normals
    inside the guard within a binade of its upper bound), 'n_high' / 'n_low' / 'n_zero' (normals outside: radicand above 2^88,
    below 2^-96, exactly 0), 'mixed' (n_in and n_high within one 8 x 8 tile), 'l_out' (light vectors outside)."""
    still = P.variants(oracle, W, H)["still"]
    tiny = ((0.0, 0.0, 2.0 ** -40), 2.0 ** -40 * 1.2)
    out = [(name, still, _program(oracle, planes), LIMITS, classes) for name, planes, classes in (
        ("plane_under", [_wall(0.99), FAR_PLANE], ("n_in",)),
        ("plane_over", [_wall(1.01), FAR_PLANE], ("n_high",)),
        ("planes_mixed", [_wall(0.99), _side(1.01)], ("n_in", "n_high", "mixed")),
        ("plane_tiny", [tiny, FAR_PLANE], ("n_low",)))]
    u, prog, limits = _large_block(oracle, still)
    return out + [("large_block", u, prog, limits, ("n_zero", "l_out"))]


def hit_guard(u, W, H, cc, w, limits):
    """Per surface sample of the frame (all sixteen samples per pixel): its tile, the binary32 length of the raw tap sum, whether
    the normal and whether the light vector falls outside the guard.  The march and the taps are the numpy restatements
    (gbuffer_ref.cast's loop, the oracle's map_scene); nothing of the device."""
    ud = P.udict(u)
    py, px = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    px, py = px.ravel(), py.ravel()
    tile = (py // 8) * ((W + 7) // 8) + px // 8
    w = np.asarray(w, np.uint32)
    e, md = F(0.0001), F(limits[1])
    out = []
    with np.errstate(all="ignore"):
        for s in range(16):
            ro, (dx, dy, dz) = G.camera_rays(px, py, s, ud, W, H)
            r = G.cast(cc, w, limits, ro, dx, dy, dz)
            sf = np.nonzero(r["kind"] == G.RM_HIT_SURFACE)[0]
            x, y, z = r["hit"][sf, 1], r["hit"][sf, 2], r["hit"][sf, 3]
            f0, f1 = onp.map_scene(cc, w, md, x + e, y + -e, z + -e), onp.map_scene(cc, w, md, x + -e, y + -e, z + e)
            f2, f3 = onp.map_scene(cc, w, md, x + -e, y + e, z + -e), onp.map_scene(cc, w, md, x + e, y + e, z + e)
            n = np.stack([((f0 + -f1) + -f2) + f3, ((-f0 + -f1) + f2) + f3, ((-f0 + f1) + -f2) + f3], axis=-1)
            l = np.stack([x - F(2.0), y - F(-5.0), z - F(3.0)], axis=-1)
            sn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
            sl = (l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]
            out.append((tile[sf], np.sqrt(sn), D.guard_bad_np(n, np.sqrt(sn), sn), D.guard_bad_np(l, np.sqrt(sl), sl)))
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "40x24"])
def test_the_scenes_take_the_paths_they_are_here_for(oracle, size):
    W, H = size
    seen = set()
    for name, u, (cc, w), limits, classes in shade_scenes(oracle, W, H):
        tile, ln, n_out, l_out = hit_guard(u, W, H, cc, w, limits)
        sets = {"n_in": ~n_out & (ln > F(2.0 ** 43)), "n_high": n_out & (ln > F(2.0 ** 43)), "n_low": n_out & (ln > 0) & (ln < F(2.0 ** -48)),
                "n_zero": n_out & (ln == 0), "l_out": l_out}
        both = np.intersect1d(tile[sets["n_in"]], tile[sets["n_high"]]).size
        print("%-12s %dx%d: %d surface samples; %s; %d tiles with normals on both sides of 2^44" % (
            name, W, H, tile.size, ", ".join("%s %d" % (k, int(v.sum())) for k, v in sets.items()), both))
        for c in classes:
            if c == "mixed":
                assert both >= 1
            else:
                assert int(sets[c].sum()) >= 100, (name, c)
        if name == "plane_under":
            assert not n_out.any()
        if name != "large_block":
            assert not l_out.any()
        seen.update(classes)
    assert seen == {"n_in", "n_high", "n_low", "n_zero", "mixed", "l_out"}


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "40x24"])
def test_shaded_frames_match_the_oracle(res, oracle, size):
    W, H = size
    try:
        for name, u, (cc, w), limits, _ in shade_scenes(oracle, W, H):
            ref = oracle.render(u, limits, cc, w, W, H, threads=16)
            res.set_limits(limits)
            res.set_program(cc, np.asarray(w, dtype=np.uint32))
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
                    raise AssertionError("%s / %dx%d, specialise %d: %s" % (name, W, H, spec, e)) from None
    finally:
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
        res.set_limits(LIMITS)
