"""Per-tile primitive masks ("Per-tile primitive masks"): the pre-pass keeps, per tile, one bit per entry of
the miss-test tables that the tile's cone does not provably clear; the per-pixel test of the pre-pass and the per-ray test of the
march kernel visit the set bits only.  rm_selftest_cull_tiles reports the mask (out[6]) and the number of entries (out[7]).

The miss tests are optional -- a ray they do not clear is marched and ends as the same miss -- so the one way a mask can change a
pixel is by dropping an entry that a sample ray of the tile meets.  Soundness is therefore tested directly: against cull_ref's
binary64 zones and the numpy oracle's binary32 sample rays, every one of the 1024 of a tile, in the style of
test_gpu_prepass_tiles.py.  Then that it IS a mask (not all ones under another name), and that every configuration in which the
mask is not in use, and silhouettes at several distances, still draw the oracle's frame bit for bit."""
import numpy as np
import pytest

import cull_ref as R
import scenes
import tile_mask_ref as TM
from prepass_ref import CLEAR, USABLE, all_tiles, pick_tiles, plane_program, udict, with_frame_corners
from ray_marching_amd import _ffi, renderer, shard
from test_cull_tables_cpu import decode
from test_gpu_cull_bounds import set_case, table_zones
from test_gpu_parity import assert_same, orbit_frame_uniforms, setup
from test_gpu_prepass_tiles import probe_tiles

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


def _camera(oracle, name, W, H):
    if name.startswith("orbit"):
        return orbit_frame_uniforms(oracle, W, H, int(name[5:]))
    return oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)[0]


def _edge_tiles(W, H):
    """Tiles along the four edges of the frame (every 9th), its corners included by with_frame_corners."""
    tx, ty = (W + 7) // 8, (H + 7) // 8
    xs, ys = np.arange(0, tx, 9), np.arange(0, ty, 9)
    return np.concatenate([np.stack([xs, np.zeros_like(xs)], 1), np.stack([xs, np.full_like(xs, ty - 1)], 1),
                           np.stack([np.zeros_like(ys), ys], 1), np.stack([np.full_like(ys, tx - 1), ys], 1)])


_PROBES = {}


def probe(res, oracle, scene, cam, W, H, min_dist, seed):
    """One probe call on ~300 tiles picked as pick_tiles does plus edge and corner tiles; cached.  Returns a dict: txy, mask, flags,
    n (entries the device reports), d (decoded program), met (E(tile), binary64), model (tile_mask_ref's mask)."""
    key = (scene, cam, W, H, min_dist)
    if key in _PROBES:
        return _PROBES[key]
    cc, w = oracle.serialize(*scenes.SCENES[scene]())
    w = np.asarray(w, dtype=np.uint32)
    d = decode(cc, w)
    assert not d["cull_veto"]
    u = _camera(oracle, cam, W, H)
    set_case(res, cc, w, min_dist)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    ud = udict(u)
    ro64 = np.array([ud["inv_view"][12 + k] for k in range(3)], dtype=F).astype(np.float64)
    zones, bits = table_zones(d, ro64, min_dist), TM.entry_bits(d)
    txy = pick_tiles(ud, W, H, zones, np.random.default_rng(seed))
    txy = with_frame_corners(np.unique(np.concatenate([txy, _edge_tiles(W, H)]), axis=0), W, H)
    out = probe_tiles(res, W, H, txy)
    _, model, met = TM.tile_truth(ud, W, H, txy, zones, bits)
    p = dict(txy=txy, mask=out[:, 6].view(np.uint32).astype(np.uint64), flags=out[:, 5].view(np.uint32), n=out[:, 7].view(np.uint32),
             rho=out[:, 3], d=d, met=met, model=model, name="%s / %s / %dx%d / min_dist %g" % key)
    _PROBES[key] = p
    return p


def check_sound_and_consistent(p):
    name, mask, flags, d = p["name"], p["mask"], p["flags"], p["d"]
    n = TM.n_entries(d)
    assert np.all(p["n"] == n), name
    usable = (flags & USABLE) != 0
    in_use = usable & ~np.isnan(p["rho"]) & (n <= 32)
    assert np.all(mask[~in_use] == TM.ALL), "%s: a mask that is not in use must be all ones" % name
    assert np.all((mask[usable] == 0) == ((flags[usable] & CLEAR) != 0)), "%s: mask == 0 and the CLEAR flag disagree" % name
    if n < 32:
        assert not np.any(mask[in_use] >> np.uint64(n)), "%s: a bit at or above n_cone + n_slab is set" % name
    dropped = p["met"] & ~mask
    bad = np.flatnonzero(dropped != 0)
    assert len(bad) == 0, "%s: tile %s: a sample ray meets entry bits %#x that the tile's mask %#x leaves out" % (
        name, p["txy"][bad[0]].tolist(), int(dropped[bad[0]]), int(mask[bad[0]]))
    return in_use


SMALL = [(s, c, m) for s in ("g32", "g64") for c in ("still", "orbit100") for m in (0.01, 0.1)]


@pytest.mark.parametrize("scene,cam,min_dist", SMALL, ids=["%s-%s-%g" % c for c in SMALL])
def test_no_sample_ray_meets_an_entry_the_mask_leaves_out(res, oracle, scene, cam, min_dist):
    p = probe(res, oracle, scene, cam, 640, 360, min_dist, 71100 + SMALL.index((scene, cam, min_dist)))
    in_use = check_sound_and_consistent(p)
    assert in_use.all(), "g32 has 13 entries, g64 25: every tile of a 640x360 frame has a mask"
    print("%s: %d tiles, %d touching, |E| %d, mask population %d" % (
        p["name"], len(p["txy"]), (p["met"] != 0).sum(), TM.popcount(p["met"]).sum(), TM.popcount(p["mask"]).sum()))


@pytest.mark.parametrize("W,H", [(1920, 1080), (1918, 1078)])
def test_masks_of_the_metric_frame(res, oracle, W, H):
    """~350 tiles of the metric frame: silhouettes, horizon, cell edges, random ones, the frame's edges and corners -- on the ragged
    1918x1078 frame the last tile column and row hang over the frame.  Sound, consistent, and a mask: it names every entry of
    E(tile), the entries some sample ray meets, and in total at most |E| plus one entry per touching tile -- the slack covers the
    cone's circumscription of the square tile.  (The binary64 model of the rule, tile_mask_ref.touch_mask, needs 137 for |E| = 105
    on 91 touching tiles of the 1920x1080 sample, inside the bound of 196.)"""
    p = probe(res, oracle, "g32", "still", W, H, 0.01, 71000)
    in_use = check_sound_and_consistent(p)
    assert in_use.all()
    txy, mask, met = p["txy"], p["mask"], p["met"]
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    touching = met != 0
    assert touching.sum() >= 60, "the sample must hold silhouette tiles"
    assert np.any((txy[:, 0] == tiles_x - 1) & (txy[:, 1] == tiles_y - 1)) and np.any(txy[:, 0] == 0) and np.any(txy[:, 1] == 0)
    pop, e_pop, model_pop = int(TM.popcount(mask).sum()), int(TM.popcount(met).sum()), int(TM.popcount(p["model"]).sum())
    print("%s: %d tiles, %d touching, |E| %d, model %d, device mask population %d (bound %d)" % (
        p["name"], len(txy), touching.sum(), e_pop, model_pop, pop, e_pop + touching.sum()))
    assert pop <= e_pop + int(touching.sum())


# ---- frames, bit for bit ----------------------------------------------------------------------------------------------------------
LIM = (0.01, 100.0, 64)


def _many_entries():
    """48 grid primitives, 37 of them with a table entry: more than a mask has bits for."""
    t = scenes._Tab()
    return t.nodes, scenes._fold_left(t, scenes._grid_prims(t, 8, 6, 0x5DF00060))


def _programs(oracle):
    return {
        "more than 32 entries": oracle.serialize(*_many_entries()),
        "plane (veto bit 1)": plane_program(oracle),
        "non-finite parameter (veto bit 0)": R.words_of((0, [0, 0, 0, 1.0]), (0, [np.inf, 0, 0, 1.0]), (100, [])),
        "transforms": oracle.serialize(*scenes.xform_mix()),
        "smooth union, bound walk": oracle.serialize(*scenes.g32s()),
    }


@pytest.mark.parametrize("name", ["more than 32 entries", "plane (veto bit 1)", "non-finite parameter (veto bit 0)", "transforms",
                                  "smooth union, bound walk"])
@pytest.mark.parametrize("specialize", [0, 2], ids=["interpreter", "generated"])
def test_programs_without_a_mask_draw_the_oracles_frame(res, oracle, name, specialize):
    W, H = 64, 48
    cc, w = _programs(oracle)[name]
    w = np.asarray(w, dtype=np.uint32)
    if name == "more than 32 entries":
        d = decode(cc, w)
        assert TM.n_entries(d) > 32
    u = _camera(oracle, "still", W, H)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=LIM)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, specialize)
    try:
        assert_same(res.draw(W, H), oracle.render(u, LIM, cc, w, W, H, threads=16))
    finally:
        res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_no_march_and_one_step(res, oracle, max_iter):
    W, H = 64, 48
    cc, w = oracle.serialize(*scenes.g32())
    u = _camera(oracle, "still", W, H)
    lim = (0.01, 100.0, max_iter)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=lim)
    assert_same(res.draw(W, H), oracle.render(u, lim, cc, w, W, H, threads=16))


def test_strips_of_16_rows_over_three_ranks(res, oracle):
    W, H = 64, 48
    cc, w = oracle.serialize(*scenes.g32())
    u = _camera(oracle, "still", W, H)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=LIM)
    ref = oracle.render(u, LIM, cc, w, W, H, threads=16)
    img = np.zeros_like(res.draw(W, H))
    for rank in range(3):
        shard.scatter_strips(img, res.draw_strips(W, H, 16, rank, 3), H, rank, 3, 16)
    assert_same(img, ref)


def test_two_frame_batch(res, oracle):
    W, H = 64, 48
    cc, w = oracle.serialize(*scenes.g32())
    frames = [_camera(oracle, cam, W, H) for cam in ("still", "orbit300")]
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(frames[0])), limits=LIM)
    batch = res.draw_batch([_ffi.Uniforms.from_buffer_copy(bytes(f)) for f in frames], W, H)
    for i, f in enumerate(frames):
        assert_same(batch[i], oracle.render(f, LIM, cc, w, W, H, threads=16))


def _at_distance(oracle, W, H, radius):
    return oracle.orbit_uniforms((float(W), float(H)), radius=radius, events=scenes.STILL_CAMERA_EVENTS)[0]


@pytest.mark.parametrize("scene", ["g8", "g32"])
@pytest.mark.parametrize("radius", [3.0, 6.0, 14.0])
@pytest.mark.parametrize("size", [64, 192])
def test_silhouettes_at_three_distances(res, oracle, scene, radius, size):
    """The camera near, at the usual distance and far: a tile holds one, a few, and most of the primitives.  At 64x64 a tile's
    cone is about as wide as the cone argument admits (rho < 0.05: tiles in the frame's middle have no mask, all ones); at
    192x192 every tile has one."""
    cc, w = oracle.serialize(*scenes.SCENES[scene]())
    w = np.asarray(w, dtype=np.uint32)
    u = _at_distance(oracle, size, size, radius)
    setup(res, cc=cc, words=w, u=_ffi.Uniforms.from_buffer_copy(bytes(u)), limits=LIM)
    out = probe_tiles(res, size, size, all_tiles(size, size))
    pop = TM.popcount(out[:, 6].view(np.uint32))
    print("%s at %g, %dx%d: mask populations %s" % (scene, radius, size, size, np.bincount(pop).tolist()))
    assert size == 64 or (pop < 32).all()
    assert_same(res.draw(size, size), oracle.render(u, LIM, cc, w, size, size, threads=16))
