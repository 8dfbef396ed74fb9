"""The pre-pass's tile verdicts under arbitrary uniform blocks ("Pre-pass under arbitrary uniform blocks").

tile_verdict_v5 settles a whole 8 x 8 tile from the rectangle of its sample positions and writes one constant without a look at a
pixel; its proofs are worded for ANY matrices, and the uniform block is three opaque blobs.  tests/test_gpu_prepass_tiles.py runs it
under orbit cameras only, and the small frames of the other arbitrary-matrix tests have no usable tile cone.  Here: every uniform
block of prepass_ref.variants (rolled, tilted, mirrored, off-axis, scaled, non-affine, extents of either sign and any size, cameras
on / just above / below the floor, far away, ro.w = 2, NaN rays) at frame sizes whose tiles do have a cone -- 328 x 200 (1025 tiles:
the last pre-pass workgroup holds one), 326 x 198 (ragged) and 280 x 168 (the last workgroup lacks one tile) -- first through
rm_selftest_cull_tiles with the one-sided, exact assertions of prepass_ref.check_tiles, then whole frames through rm_draw,
rm_draw_strips and rm_draw_batch against the oracle, bit for bit; then random uniform blocks x random programs.
RM_FUZZ_SEEDS / RM_FUZZ_FIRST_SEED as in test_gpu_fuzz.py."""
import os

import numpy as np
import pytest

import prepass_ref as P
import scenes
from ray_marching_amd import _ffi, renderer, shard
from test_gpu_cull_bounds import MIN_DISTS
from test_gpu_fuzz import random_tree
from test_gpu_parity import assert_same
from test_gpu_prepass_tiles import probe_case, probe_tiles

pytestmark = pytest.mark.gpu

W, H = P.BASE_SIZE
LIMITS = (0.01, 100.0, 96)
# Variants with many truly-sky and truly-one-cell tiles (tests/test_prepass_uniforms_cpu.py) of which the tile rules legitimately
# settle none, and why; they are not counted by test_new_cases_are_not_vacuous.
CONSERVATIVE = {
    "just_below_floor": "C = -1.5 - ro.y > 0: both rules require the camera above the floor plane (rect_sky_v5: C < 0; rect_cell_v5: "
                        "C < -1e-20) -- seen from below, rays that point up reach the floor and rays that point down are black, "
                        "and nothing is assumed about that",
    "noisy_rolls": "inv_proj holds four entries of 1e5 that cancel, so mag >= 2e5 |inv_view row y| and the slacks 1e-5 mag (sky) and "
                   "4 * 4e-6 mag (one cell) exceed every |dy| of the frame (< 1.3): rightly so, the positions are quantised to "
                   "several sample pitches and the corner samples do not bound the others "
                   "(test_corner_samples_do_not_bound_a_tile_under_noisy_rolls); for the same reason cone_noise_v5 leaves no tile "
                   "and no pixel a usable cone (before it existed, samples lay 3e-3 outside the cones reported here)",
}


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)          # library defaults, but wait for the compiler: the specialised kernel is what is drawn
    r.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    r.resize_command_buffer(8192)
    yield r
    r.close()


@pytest.fixture(scope="module")
def blocks(oracle):
    return P.variants(oracle, W, H)


@pytest.fixture(scope="module")
def truth(blocks):
    """{variant: (truly-sky tiles, one-cell code per tile or -1)} at the base size, by the numpy reference."""
    return {name: P.tile_truth(P.udict(u), W, H) for name, u in blocks.items()}


def ffi_u(u):
    return _ffi.Uniforms.from_buffer_copy(bytes(u))


# ---- the probe under every variant ------------------------------------------------------------------------------------------------
PLANE_VARIANTS = ("roll30", "off_axis", "extent_small")
PROBE_CASES = [(v, prog, (2 * i + j) % len(MIN_DISTS)) for i, v in enumerate(P.VARIANT_NAMES) for j, prog in enumerate(("g32", "xform_mix"))]
PROBE_CASES += [(v, "plane", 3 + i) for i, v in enumerate(PLANE_VARIANTS)]
_STATS = {}


def run_probe(res, oracle, blocks, case):
    if case in _STATS:
        return _STATS[case]
    variant, prog, k = case
    name = "%s / %s / %dx%d / min_dist %g" % (prog, variant, W, H, MIN_DISTS[k])
    stats = probe_case(res, oracle, name, prog, blocks[variant], W, H, MIN_DISTS[k], 62000 + PROBE_CASES.index(case), frame_corners=True)
    assert stats["tiles"] <= 350
    n_set = {k: stats[k][0] for k in ("clear", "sky", "cell")}
    if variant in ("nan_rays", "nan_proj"):
        assert not any(n_set.values()), "%s: a flag is set although the block is no camera: %s" % (name, n_set)
    if variant in ("just_below_floor", "on_floor"):
        # (on_floor, C = 0: t = 0 / dy is never > 0, every miss is black -- the oracle would allow "sky" for any tile; that a
        # sky tile's samples are all black is asserted as everywhere)
        assert n_set["cell"] == 0, "%s: a tile is reported as one cell with the camera not above the floor" % name
    _STATS[case] = stats
    return stats


@pytest.mark.parametrize("case", PROBE_CASES, ids=["%s-%s" % c[:2] for c in PROBE_CASES])
def test_tile_verdicts_hold_under_the_variant(res, oracle, blocks, case):
    run_probe(res, oracle, blocks, case)


def test_no_flag_is_set_under_nan_rays(res, oracle, blocks):
    """Under nan_rays (inv_proj = 0) no ray is NaN: pt_world = 0, and wgsl:62 normalises the vec4 (0 - ro.xyz, 0 - ro.w), so every
    sample of the frame has the one direction -ro.xyz / |(ro.xyz, ro.w)|, finite and pointing up; the oracle paints every pixel black.
    A block that maps a whole tile onto one direction is no camera, and tile_verdict_v5 declines it (its four corners coincide): no
    flag on any tile, as for nan_proj, whose rays are NaN.  The per-pixel path draws the frame (test_frame_under_the_variant)."""
    n_set = {}
    for prog in ("g32", "xform_mix"):
        stats = run_probe(res, oracle, blocks, next(c for c in PROBE_CASES if c[:2] == ("nan_rays", prog)))
        n_set[prog] = {k: stats[k][0] for k in ("clear", "sky", "cell")}
    print("nan_rays, tiles with each flag set: %s" % n_set)
    assert not any(v for d in n_set.values() for v in d.values()), n_set


def test_new_cases_are_not_vacuous(res, oracle, blocks, truth):
    total, settled = {}, {}
    for case in PROBE_CASES:
        stats = run_probe(res, oracle, blocks, case)
        for k in ("clear", "sky", "cell", "code"):
            total[k] = tuple(a + b for a, b in zip(total.get(k, (0, 0)), stats[k]))
        settled[case[0]] = settled.get(case[0], 0) + stats["settled"]
    print("tile flags (set, unset) over the variants: %s" % total)
    for k in ("clear", "sky", "cell"):
        assert total[k][0] > 20 and total[k][1] > 20, (k, total)
    assert total["code"][0] > 0 and total["code"][1] > 0, total
    rich = [n for n, (t_sky, t_cell) in truth.items() if t_sky.sum() >= 20 and (t_cell >= 0).sum() >= 20]
    counted = [n for n in rich if n not in CONSERVATIVE]
    assert len(counted) >= 6 and {"roll30", "roll90", "roll_down", "off_axis", "look_down", "just_above_floor"} <= set(counted)
    for n in counted:
        assert settled[n] >= 1, "%s: no probed tile is settled per tile (clear and sky or one cell)" % n
    for n in CONSERVATIVE:
        assert settled[n] == 0, "%s settles tiles now: take it off the list of conservative variants" % n


def test_every_tile_of_the_frame_under_every_variant(res, oracle, blocks, truth):
    """All 1025 tiles under g32: a sky tile is truly sky, a one-cell tile truly lies in that cell (the reference's floor codes of all
    its samples).  Prints settled against true per variant, the record of DESIGN.md section 5."""
    cc, w = P.program(oracle, "g32")
    res.set_option(_ffi.RM_OPT_CULL, 1)
    res.set_limits(LIMITS)
    res.set_program(cc, np.asarray(w, dtype=np.uint32))
    txy = P.all_tiles(W, H)
    print("| variant | clear | sky: settled / flagged / true | one cell: settled / flagged / true |")
    for name, u in blocks.items():
        res.set_uniforms(ffi_u(u))
        out = probe_tiles(res, W, H, txy)
        flags = out[:, 5].view(np.uint32)
        clear, sky, cell = (flags & P.CLEAR) != 0, (flags & P.SKY) != 0, (flags & P.CELL) != 0
        t_sky, t_cell = truth[name]
        assert not (sky & ~t_sky).any() and not (cell & (t_cell != out[:, 4].astype(np.int64))).any(), name
        print("| `%s` | %d | %d / %d / %d | %d / %d / %d |" % (name, clear.sum(), (clear & sky).sum(), sky.sum(), t_sky.sum(),
                                                            (clear & cell).sum(), cell.sum(), (t_cell >= 0).sum()))


# ---- frames, bit for bit ----------------------------------------------------------------------------------------------------------
def load(res, cc, w, u, lim):
    res.set_limits(lim)
    res.set_uniforms(ffi_u(u))
    res.set_program(cc, np.asarray(w, dtype=np.uint32))


def assert_frames(res, oracle, cc, w, u, lim, fw, fh, what, specs=(2, 0), culls=(1, 0)):
    """rm_draw with culling on and off, with the library's default kernel and with the interpreter: each the oracle's frame."""
    ref = oracle.render(u, lim, cc, w, fw, fh, threads=16)
    load(res, cc, w, u, lim)
    try:
        for spec in specs:
            res.set_option(_ffi.RM_OPT_SPECIALIZE, spec)
            for cull in culls:
                res.set_option(_ffi.RM_OPT_CULL, cull)
                try:
                    assert_same(res.draw(fw, fh), ref)
                except AssertionError as e:
                    raise AssertionError("%s, specialise %d, cull %d: %s" % (what, spec, cull, e)) from None
    finally:
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
        res.set_option(_ffi.RM_OPT_CULL, 1)
    return ref


@pytest.mark.parametrize("variant", P.VARIANT_NAMES)
def test_frame_under_the_variant(res, oracle, blocks, variant):
    cc, w = P.program(oracle, "g32")
    assert_frames(res, oracle, cc, w, blocks[variant], LIMITS, W, H, variant)


@pytest.mark.parametrize("variant", ["roll30", "off_axis", "extent_negative_xy", "extent_small"])
@pytest.mark.parametrize("prog", ["xform_mix", "plane"])
def test_other_programs_under_the_variant(res, oracle, blocks, prog, variant):
    cc, w = P.program(oracle, prog)
    assert_frames(res, oracle, cc, w, blocks[variant], LIMITS, W, H, "%s / %s" % (prog, variant))


@pytest.mark.parametrize("variant", ["roll90", "off_axis"])
@pytest.mark.parametrize("size", [P.RAGGED_SIZE, P.SIZE_31], ids=["ragged", "31_of_32"])
def test_ragged_frame_and_a_last_workgroup_short_of_one_tile(res, oracle, size, variant):
    fw, fh = size
    cc, w = P.program(oracle, "g32")
    assert_frames(res, oracle, cc, w, P.variants(oracle, fw, fh)[variant], LIMITS, fw, fh, "%s at %dx%d" % (variant, fw, fh))


@pytest.mark.parametrize("variant", ["roll30", "extent_negative_y"])
def test_row_bands_and_strips(res, oracle, blocks, variant):
    """An unaligned row0 (the tiles start there) and 16-row strips of three ranks (rm_global_row maps a tile's rows)."""
    cc, w = P.program(oracle, "g32")
    u = blocks[variant]
    ref = oracle.render(u, LIMITS, cc, w, W, H, threads=16)
    load(res, cc, w, u, LIMITS)
    for row0 in (13, 91):
        assert row0 % 8 != 0
        assert_same(res.draw(W, H, row0=row0, rows=64), ref[row0:row0 + 64])
    img = np.zeros_like(ref)
    for rank in range(3):
        shard.scatter_strips(img, res.draw_strips(W, H, 16, rank, 3), H, rank, 3, 16)
    assert_same(img, ref)


def test_batch_of_three_variants(res, oracle, blocks):
    """Every frame of a batch from ITS uniform block (L.frames[blockIdx.z]) and its own verdicts, a frame of NaN rays in the middle."""
    cc, w = P.program(oracle, "g32")
    names = ("roll30", "nan_rays", "off_axis")
    load(res, cc, w, blocks[names[0]], LIMITS)
    batch = res.draw_batch([ffi_u(blocks[n]) for n in names], W, H)
    for i, n in enumerate(names):
        ref = oracle.render(blocks[n], LIMITS, cc, w, W, H, threads=16)
        res.set_uniforms(ffi_u(blocks[n]))
        assert_same(res.draw(W, H), ref)
        assert_same(batch[i], ref)
    assert batch[0].tobytes() != batch[2].tobytes()


@pytest.mark.parametrize("variant", ["roll90", "just_above_floor"])
def test_no_march_steps_under_the_variant(res, oracle, blocks, variant):
    cc, w = P.program(oracle, "g32")
    assert_frames(res, oracle, cc, w, blocks[variant], (0.01, 100.0, 0), W, H, "%s, max_iter 0" % variant, specs=(2,))


def test_8bit_output_under_off_axis(res, oracle, blocks):
    cc, w = P.program(oracle, "g32")
    u = blocks["off_axis"]
    ref = oracle.quantize_unorm8(oracle.render(u, LIMITS, cc, w, W, H, threads=16))
    load(res, cc, w, u, LIMITS)
    try:
        res.set_output_format(_ffi.RM_FORMAT_RGBA8_UNORM)
        img = res.draw(W, H)
        assert img.dtype == np.uint8 and img.tobytes() == ref.tobytes()
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)


# ---- random uniform blocks x random programs ---------------------------------------------------------------------------------------
SEEDS = range(int(os.environ.get("RM_FUZZ_FIRST_SEED", "0")), int(os.environ.get("RM_FUZZ_FIRST_SEED", "0")) + int(os.environ.get("RM_FUZZ_SEEDS", "24")))


def random_rotation(rng):
    """A rotation matrix from a uniformly random unit quaternion: any heading, pitch and roll."""
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def random_uniforms(rng, oracle):
    u = oracle.orbit_uniforms((float(W), float(H)))[0]
    M = np.eye(4)
    M[:3, :3] = random_rotation(rng)
    if rng.random() < 0.3:
        M[:3, :3] *= rng.uniform(0.3, 3.0)
    y = rng.uniform(-1.5 + 1e-3, 8.0) if rng.random() < 0.85 else rng.uniform(-6.0, -1.5 - 1e-3)     # else: below the floor
    M[:3, 3] = (rng.uniform(-6.0, 6.0), y, rng.uniform(-6.0, 6.0))
    P.store_matrix(u.inv_view, M)
    m = P.perspective_inverse(oracle, W / H, float(rng.uniform(0.3, 1.4)), float(rng.uniform(0.3, 3.0)))
    for i in range(16):
        u.inv_proj[i] = float(m[i])
    u.inv_proj[12] += float(rng.uniform(-0.4, 0.4))
    u.inv_proj[13] += float(rng.uniform(-0.4, 0.4))
    ex, ey = [(float(W), float(H)), (W / 4.0, H / 4.0), (1e6, 1e6)][int(rng.integers(0, 3))]
    u.viewport_extent[0], u.viewport_extent[1] = ex * rng.choice([-1.0, 1.0]), ey * rng.choice([-1.0, 1.0])
    return u


def random_valid_program(rng, oracle, lattice):
    for _ in range(20):
        t = scenes._Tab()
        root = random_tree(rng, t, int(rng.integers(3, 6)) if lattice else int(rng.integers(1, 5)),
                           allow_plane=bool(rng.random() < 0.3) and not lattice, tags=False, lattice=lattice)
        cc, w = oracle.serialize(t.nodes, root)
        rc, _ = oracle.validate(cc, w)
        prc, _ = renderer.validate_program(cc, w)
        assert rc == prc
        if rc == 0:         # (else e.g. nested more than 8 transforms deep: both sides agree, and another tree is drawn)
            return cc, np.asarray(w, dtype=np.uint32)
    raise AssertionError("no valid program in 20 draws")


@pytest.mark.parametrize("seed", SEEDS)
def test_random_uniform_blocks_and_programs(res, oracle, seed):
    rng = np.random.default_rng(515000 + seed)
    u = random_uniforms(rng, oracle)
    cc, w = random_valid_program(rng, oracle, lattice=seed % 2 == 1)
    lim = (0.01, 100.0, int(rng.choice([24, 64])))
    report = "seed %d; uniforms %s; limits %s; program: cmd_count %d words %s" % (seed, P.udict(u), lim, cc, [int(x) for x in w])
    ref = oracle.render(u, lim, cc, w, W, H, threads=16)
    load(res, cc, w, u, lim)
    res.set_option(_ffi.RM_OPT_CULL, 1)
    img = res.draw(W, H)
    if img.tobytes() != ref.tobytes():
        bad = np.argwhere((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1))
        raise AssertionError("the frame differs from the oracle at %d pixels (first %s); %s" % (len(bad), bad[:3].tolist(), report))
    try:
        probe_case(res, oracle, "seed %d" % seed, (cc, w), u, W, H, lim[0], 63000 + seed, frame_corners=True, n_each=35, n_random=40)
    except AssertionError as e:
        raise AssertionError("%s; %s" % (e, report)) from None
