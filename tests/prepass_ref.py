"""What the tests of the pre-pass's tile verdicts share ("Pre-pass"), in numpy alone -- nothing here needs a
device: the oracle's rays and floor codes for every sample of a tile, the choice of tiles worth probing, the assertions on what
rm_selftest_cull_tiles reports, and the uniform blocks the verdicts are tested under (tests/test_gpu_prepass_tiles.py,
tests/test_gpu_prepass_uniforms.py, tests/test_prepass_uniforms_cpu.py).

The uniform block is three opaque blobs to the pipeline, so `variants` edits the still orbit camera's block into everything the
tile rules' proofs claim to cover: non-affine last rows, other near planes, extents of either sign and any size, rolled and tilted
cameras, asymmetric and mirrored frusta, scaled views, cameras on, just above and below the floor plane, far from the origin, and
with ro.w != 1.  Matrices are column-major: element row + 4 * col."""
import ctypes as C
import math

import numpy as np

import cull_ref as R
import gbuffer_ref
import scenes
from oracle import rm_oracle_np as onp

F = np.float32
CLEAR, SKY, CELL, USABLE = 1, 2, 4, 8
BASE_SIZE = (328, 200)          # 41 x 25 = 1025 tiles: 32 pre-pass workgroups of 32 tiles and one of a single tile
RAGGED_SIZE = (326, 198)        # the last tile column and row hang over the frame
SIZE_31 = (280, 168)            # 35 x 21 = 735 tiles = 22 * 32 + 31: the last workgroup lacks one tile
assert (BASE_SIZE[0] // 8) * (BASE_SIZE[1] // 8) % 32 == 1 and (SIZE_31[0] // 8) * (SIZE_31[1] // 8) % 32 == 31
# the pitch of look_down / look_up (radians about the camera's x axis): at -0.35 the floor fills the lower two thirds of the frame,
# near rows lie in one checker cell per tile and rows towards the horizon straddle cell edges (tests/test_prepass_uniforms_cpu.py
# asserts both)
LOOK_DOWN, LOOK_UP = -0.35, 0.25


def udict(u):
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


def floor_codes(ro, d):
    """The colour code of a miss ray as the oracle's ray_march decides it (rm_oracle_np.py, the miss branch): -1 black, else
    the checker bit.  d: (dx, dy, dz) binary32 arrays."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fd = (F(-1.5) - ro[1]) / d[1]
        on = fd > 0
        fx, fz = ro[0] + d[0] * fd, ro[2] + d[2] * fd
        ix, iz = onp.f2i(np.rint(fx + F(0.5))), onp.f2i(np.rint(fz + F(0.5)))
    return np.where(on, (ix ^ iz) & 1, -1)


def camera_rays(px, py, sample, ud, W, H):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return gbuffer_ref.camera_rays(px, py, sample, ud, W, H)


def tile_samples(ud, W, H, txy):
    """Every sample ray of the tiles' pixels inside the frame: ro (3,), directions (n, 3) binary32, tile index (n,)."""
    lane = np.arange(64)
    px = (txy[:, 0, None] * 8 + (lane & 7)[None, :]).ravel()
    py = (txy[:, 1, None] * 8 + (lane >> 3)[None, :]).ravel()
    owner = np.repeat(np.arange(len(txy)), 64)
    keep = (px < W) & (py < H)
    px, py, owner = px[keep].astype(np.uint32), py[keep].astype(np.uint32), owner[keep]
    dirs, ro = [], None
    for s in range(16):
        ro, d = camera_rays(px, py, s, ud, W, H)
        dirs.append(np.stack(d, axis=1))
    return np.array(ro, dtype=F)[:3], np.concatenate(dirs), np.tile(owner, 16)


def all_tiles(W, H):
    tx, ty = np.meshgrid(np.arange((W + 7) // 8), np.arange((H + 7) // 8))
    return np.stack([tx.ravel(), ty.ravel()], axis=1)


def pick_tiles(ud, W, H, zones, rng, n_each=70, n_random=90):
    """Tiles on silhouettes, on the horizon and on cell edges -- the centre rays of their four corner pixels disagree about a
    zone, about sky / floor or about the checker bit -- and random ones."""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    tx, ty = np.meshgrid(np.arange(tiles_x), np.arange(tiles_y))
    tx, ty = tx.ravel(), ty.ravel()
    meets, codes = [], []
    for cx, cy in ((0, 0), (7, 0), (0, 7), (7, 7)):
        px, py = np.minimum(tx * 8 + cx, W - 1).astype(np.uint32), np.minimum(ty * 8 + cy, H - 1).astype(np.uint32)
        ro, d = camera_rays(px, py, gbuffer_ref.RM_SAMPLE_CENTER, ud, W, H)
        ro = np.array(ro, dtype=F)[:3]
        d64 = np.stack(d, axis=1).astype(np.float64)
        m = np.zeros(len(px), dtype=bool)
        ok = np.isfinite(d64).all(axis=1) & (d64 != 0.0).any(axis=1)        # (a ray that is not a number meets nothing)
        for z in zones:
            if ok.any():
                m[ok] |= R.meets_zone(z, ro.astype(np.float64), d64[ok])
        meets.append(m)
        codes.append(floor_codes(ro, d))
    meets, codes = np.array(meets), np.array(codes)
    silhouette = np.flatnonzero(meets.any(axis=0) != meets.all(axis=0))
    sky = codes < 0
    horizon = np.flatnonzero(sky.any(axis=0) != sky.all(axis=0))
    edge = np.flatnonzero(~sky.any(axis=0) & (codes.min(axis=0) != codes.max(axis=0)))
    parts = [rng.permutation(k)[:n_each] for k in (silhouette, horizon, edge)] + [rng.integers(0, len(tx), n_random)]
    pick = np.unique(np.concatenate(parts))
    return np.stack([tx[pick], ty[pick]], axis=1)


def with_frame_corners(txy, W, H):
    """The picked tiles plus the four corner tiles of the frame; the frame's last tile is the last of them."""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    extra = np.array([(0, 0), (tiles_x - 1, 0), (0, tiles_y - 1), (tiles_x - 1, tiles_y - 1)])
    both = np.unique(np.concatenate([np.asarray(txy).reshape(-1, 2), extra]), axis=0)
    return both


def check_tiles(name, ud, W, H, txy, out, zones, check_zones=True, cone_expected=None):
    """The assertions on one rm_selftest_cull_tiles call, all one-sided and exact; returns how often each flag was seen set and
    unset.  out: the call's (n, 8) result for tiles txy; zones: the binary64 zones of the program's table entries (cull_ref);
    check_zones = False where the decoder vetoes culling (no table entry describes the scene then).  cone_expected: True / False
    when the caller knows whether the frame's tiles have a usable cone, None to assert only that every sample lies in a cone that
    is reported."""
    flags = out[:, 5].view(np.uint32)
    clear, sky, cell, usable = (flags & CLEAR) != 0, (flags & SKY) != 0, (flags & CELL) != 0, (flags & USABLE) != 0
    code = out[:, 4].astype(np.int64)
    c, rho = out[:, :3].astype(np.float64), out[:, 3].astype(np.float64)
    ro0, _ = camera_rays(np.zeros(1, np.uint32), np.zeros(1, np.uint32), 0, ud, W, H)
    ro64 = np.array(ro0, dtype=F)[:3].astype(np.float64)
    ro, e, owner = tile_samples(ud, W, H, txy)
    assert np.all(ro == np.array(ro0, dtype=F)[:3])
    assert not np.any(clear & ~usable), name
    assert not np.any(clear & np.isnan(rho)), name
    assert not np.any(sky & cell), name
    if cone_expected is False:
        assert np.isnan(rho).all() and not clear.any(), "%s: a tile of a tiny frame has no usable cone" % name
    else:
        e64 = e.astype(np.float64)
        if cone_expected:
            assert not np.isnan(rho).any(), name
            gap = rho[owner] - np.linalg.norm(e64 - c[owner], axis=1)       # (the oracle's direction as it is: of length 1)
            assert gap.min() >= 0.0, "%s: a sample direction lies %.3g outside its tile's cone" % (name, -gap.min())
        # The cone is one of half-lines, around the UNIT vector c.  The oracle's direction is xyz of a normalised vec4 (wgsl:62):
        # shorter than 1 wherever pt_world.w != ro.w (a non-affine inv_view, a near plane other than 1), so it is brought to
        # length 1 here, in binary64 -- its own binary32 rounding (6e-8 of its length per component) is what rho's 2e-6 is for.
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = rho[owner] - np.linalg.norm(e64 / np.linalg.norm(e64, axis=1, keepdims=True) - c[owner], axis=1)
        has = ~np.isnan(rho[owner])
        if has.any():
            assert not np.isnan(gap[has]).any(), "%s: a tile reports a cone although a sample direction is not a number" % name
            assert gap[has].min() >= 0.0, "%s: a sample direction lies %.3g outside its tile's cone" % (name, -gap[has].min())
    sel = clear[owner]
    if sel.any() and check_zones:
        for z in zones:
            hit = R.meets_zone(z, ro64, e[sel].astype(np.float64))
            assert not hit.any(), "%s: tile %s is reported clear but one of its samples meets the zone %s" % (
                name, txy[owner[sel][np.argmax(hit)]].tolist(), z)
    codes = floor_codes(ro, (e[:, 0], e[:, 1], e[:, 2]))
    bad = sky[owner] & (codes != -1)
    assert not bad.any(), "%s: tile %s is reported sky but a sample has floor code %d" % (name, txy[owner[np.argmax(bad)]].tolist(), codes[np.argmax(bad)])
    bad = cell[owner] & (codes != code[owner])
    assert not bad.any(), "%s: tile %s is reported cell %d but a sample has floor code %d" % (
        name, txy[owner[np.argmax(bad)]].tolist(), code[owner[np.argmax(bad)]], codes[np.argmax(bad)])
    # what is true of each probed tile, for the settled-versus-true record
    n = len(txy)
    lo, hi = np.full(n, 2), np.full(n, -2)
    np.minimum.at(lo, owner, codes)
    np.maximum.at(hi, owner, codes)
    true_sky, true_cell = (hi == -1), (lo == hi) & (lo >= 0)
    return {"clear": (int(clear.sum()), int((~clear).sum())), "sky": (int(sky.sum()), int((~sky).sum())), "cell": (int(cell.sum()), int((~cell).sum())),
            "code": (int((cell & (code == 1)).sum()), int((cell & (code == 0)).sum())), "settled": int((clear & (sky | cell)).sum()), "tiles": n,
            "flagged_sky": int(sky.sum()), "true_sky": int(true_sky.sum()), "flagged_cell": int(cell.sum()), "true_cell": int(true_cell.sum())}


def tile_truth(ud, W, H):
    """Per tile of the frame (row-major): whether all its samples inside the frame are sky (code -1), and the checker bit all of
    them share (-1 if they do not share one, or are not all on the floor)."""
    txy = all_tiles(W, H)
    ro, e, owner = tile_samples(ud, W, H, txy)
    codes = floor_codes(ro, (e[:, 0], e[:, 1], e[:, 2]))
    lo, hi = np.full(len(txy), 2), np.full(len(txy), -2)
    np.minimum.at(lo, owner, codes)
    np.maximum.at(hi, owner, codes)
    return hi == -1, np.where((lo == hi) & (lo >= 0), lo, -1)


def corner_samples_point_up(ud, W, H):
    """Per tile of the frame: whether its four extreme samples -- sample (0, 3) of its first pixel, (3, 3) of the last pixel of its
    first row, (0, 0) and (3, 0) of the first and last pixel of its last row; positive extents -- all have dy > 0.  Without
    rounding that would make every sample of the tile sky (dy is affine in the screen position)."""
    assert ud["viewport_extent"][0] > 0 and ud["viewport_extent"][1] > 0
    txy = all_tiles(W, H)
    up = np.ones(len(txy), dtype=bool)
    for cx, i in ((0, 0), (7, 3)):
        for cy, j in ((0, 3), (7, 0)):
            px, py = (txy[:, 0] * 8 + cx).astype(np.uint32), (txy[:, 1] * 8 + cy).astype(np.uint32)
            _, d = camera_rays(px, py, 4 * i + j, ud, W, H)
            up &= d[1] > 0
    return up


def horizon_tilt_rows(ud, W, H):
    """By how many rows the share of sky differs between the frame's first and last column (centre rays): 0 for an upright camera,
    H for a horizon that runs from top to bottom."""
    py = np.arange(H, dtype=np.uint32)
    n = []
    for x in (0, W - 1):
        ro, d = camera_rays(np.full(H, x, np.uint32), py, gbuffer_ref.RM_SAMPLE_CENTER, ud, W, H)
        n.append(int((floor_codes(np.array(ro, dtype=F)[:3], d) < 0).sum()))
    return abs(n[0] - n[1])


def plane_program(oracle):
    t = scenes._Tab()
    ground = t.plane((0.0, 2.0, 0.0), 2.4)
    return oracle.serialize(t.nodes, t.op(scenes.UNION, t.op(scenes.UNION, t.sphere((-0.7, 0.0, 0.0), 0.8), t.box((0.9, -0.4, 0.2), (0.5, 0.8, 0.5))), ground))


def program(oracle, name):
    if name == "plane":
        return plane_program(oracle)
    return oracle.serialize(*{**scenes.SCENES, **scenes.EXT_SCENES}[name]())


# ---- uniform blocks ---------------------------------------------------------------------------------------------------------------
def matrix(a):
    return np.array(list(a), dtype=np.float64).reshape(4, 4).T          # M[row, col] = a[row + 4 col]


def store_matrix(dst, M):
    flat = np.asarray(M, dtype=np.float64).T.ravel()
    for i in range(16):
        dst[i] = float(F(flat[i]))


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=np.float64)


def perspective_inverse(oracle, aspect, fov, znear, zfar=10000.0):
    m = np.zeros(16, F)
    oracle.lib().rmo_perspective_inverse(aspect, fov, znear, zfar, m.ctypes.data_as(C.POINTER(C.c_float)))
    return m


def clone(u):
    return type(u).from_buffer_copy(bytes(u))


VARIANT_NAMES = ("still", "short_dir_a2", "short_dir_am", "row3_x", "znear_0.5", "znear_1.5", "znear_3", "extent_small", "extent_huge",
                 "extent_negative", "nan_rays", "extent_negative_y", "extent_negative_xy", "roll30", "roll90", "look_down", "look_up",
                 "roll_down", "off_axis", "mirror_x", "view_scaled_3", "just_above_floor", "on_floor", "just_below_floor", "far_camera",
                 "ro_w_2", "nan_proj", "proj_roll30", "noisy_rolls")


def variants(oracle, W, H):
    """{name: uniform block} for a W x H frame, each an edit of the still orbit camera's block (`still` itself included).
    roll_down (a roll of -0.8 rad on top of look_down's pitch) is not in the list the tests were asked for: it is a third camera
    whose horizon crosses the frame obliquely with floor on both sides of the tilt.  Nor is nan_proj: under nan_rays (inv_proj = 0,
    carried over from test_culling_with_arbitrary_uniform_matrices) no ray is NaN -- pt_world is the zero vector, and the normalised
    vec4 (-ro.xyz, -ro.w) gives every sample the same finite direction -- so nan_proj is the block whose rays really are NaN.
    proj_roll30 puts roll30's rotation into inv_proj instead: pt_view.x and .y then each depend on both screen coordinates, and
    the chain of rounded operations from a position to pt_world.y is no longer monotone in each of them (with a diagonal
    inv_proj it is, and the corner samples then bound the others even without the rules' slacks).  noisy_rolls makes that
    count: a roll of -0.5 rad in inv_view, one of 1.0 rad in inv_proj, and 1e5 added to the z and w columns of inv_proj's first
    two rows, where z = -1 and w = 1 cancel it -- pt_view.xy is then quantised to 2^-7, several sample pitches, and there are
    tiles whose four extreme samples all point up while a sample between them points down (corner_samples_bound_the_sky;
    tests/test_prepass_uniforms_cpu.py).  Only the rules' slacks, which grow with the magnitudes that cancel, keep such a tile
    from being called sky."""
    import scenes as S
    base = oracle.orbit_uniforms((float(W), float(H)), events=S.STILL_CAMERA_EVENTS)[0]

    def view(idx, val):
        def edit(u):
            u.inv_view[idx] = val
        return edit

    def proj(znear):
        def edit(u):
            m = perspective_inverse(oracle, W / H, 0.7853981633974483, znear)
            for i in range(16):
                u.inv_proj[i] = float(m[i])
        return edit

    def extent(ex, ey):
        def edit(u):
            u.viewport_extent[0], u.viewport_extent[1] = ex, ey
        return edit

    def zero_proj(u):
        for i in range(16):
            u.inv_proj[i] = 0.0

    def view_times(M):
        def edit(u):
            store_matrix(u.inv_view, matrix(u.inv_view) @ M)
        return edit

    def nan_proj(u):
        u.inv_proj[5] = math.nan

    def proj_roll(u):
        store_matrix(u.inv_proj, rot_z(0.5) @ matrix(u.inv_proj))

    def noisy_rolls(u):
        store_matrix(u.inv_view, matrix(u.inv_view) @ rot_z(-0.5))
        store_matrix(u.inv_proj, rot_z(1.0) @ matrix(u.inv_proj))
        for i in (8, 9, 12, 13):
            u.inv_proj[i] += 1.0e5

    def off_axis(u):
        u.inv_proj[12] += 0.3
        u.inv_proj[13] -= 0.2

    def mirror_x(u):
        for i in range(4):
            u.inv_proj[i] = -u.inv_proj[i]

    def view_scaled(u):
        for i in range(12):
            u.inv_view[i] = u.inv_view[i] * 3.0

    def far_camera(u):
        u.inv_view[12], u.inv_view[13], u.inv_view[14] = 3000.0, 2000.0, 1000.0

    edits = {
        "still": lambda u: None,
        "short_dir_a2": view(11, 2.0),                      # pt_world.w = 1 - 2: |rd| ~ 0.45, same half-lines
        "short_dir_am": view(11, -0.6),
        "row3_x": view(3, 0.8),                             # pt_world.w varies across the screen
        "znear_0.5": proj(0.5),
        "znear_1.5": proj(1.5),
        "znear_3": proj(3.0),
        "extent_small": extent(W / 8.0, H / 8.0),           # AA offsets 8x the pixel pitch: a tile's rectangle reaches into its neighbours
        "extent_huge": extent(1e6, 1e6),                    # all 16 samples coincide with the pixel centre
        "extent_negative": extent(-float(W), float(H)),
        "nan_rays": zero_proj,                              # (every ray is -ro / |(ro, 1)|: finite, see above; no tile verdict)
        "extent_negative_y": extent(float(W), -float(H)),
        "extent_negative_xy": extent(-float(W), -float(H)),
        "roll30": view_times(rot_z(0.5)),
        "roll90": view_times(rot_z(math.pi / 2)),
        "look_down": view_times(rot_x(LOOK_DOWN)),
        "look_up": view_times(rot_x(LOOK_UP)),
        "roll_down": view_times(rot_x(LOOK_DOWN) @ rot_z(-0.8)),
        "off_axis": off_axis,                               # an asymmetric frustum
        "mirror_x": mirror_x,
        "view_scaled_3": view_scaled,
        "just_above_floor": view(13, -1.5 + 1e-3),
        "on_floor": view(13, -1.5),                         # C = 0: fd > 0 fails for every ray, every miss is black
        "just_below_floor": view(13, -1.5 - 1e-3),
        "far_camera": far_camera,
        "ro_w_2": view(15, 2.0),
        "nan_proj": nan_proj,
        "proj_roll30": proj_roll,
        "noisy_rolls": noisy_rolls,
    }
    assert tuple(edits) == VARIANT_NAMES
    out = {}
    for name, edit in edits.items():
        u = clone(base)
        edit(u)
        out[name] = u
    return out
