"""Scene queries on the GPU (rm_query_points / rm_cast_rays / rm_camera_rays) against the oracle, bit for bit: distances,
materials, leaves, normals, ray casts, frames composed from cast sample rays against rm_draw, picking, the device / torch
path, the largest program the command buffer holds, isolation from the draw state, and the distances against a binary64
evaluation within the error bound sparse mesh extraction relies on."""
import numpy as np
import pytest

import scene_f64
import scenes
import test_mesh_bound_cpu as B
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
NPARAM = {0: 4, 1: 6, 2: 4, 10: 5, 100: 0, 101: 0, 102: 0, 110: 1, 200: 3, 201: 0, 202: 4, 203: 0, 204: 1, 205: 0, 300: 1}
PRIMS = (0, 1, 2, 10)
LIM = (0.01, 100.0, 256)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def same(a, b):
    """Bit-identical, with any two NaNs equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype.kind == "f":
        both_nan = np.isnan(a) & np.isnan(b)
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))
    return bool(np.array_equal(a, b))


def commands(words, cc):
    """(index, opcode, float parameters) of every command."""
    w = np.asarray(words, dtype=np.uint32)
    out, q = [], 0
    for i in range(cc):
        op = int(w[q])
        out.append((i, op, w[q + 1:q + 1 + NPARAM[op]].view(F)))
        q += 1 + NPARAM[op]
    return out


def tag_every_leaf(cc, words):
    """The program's own tags dropped, Material(ordinal % 256) after every primitive: (cmd_count, words, {command index of the
    primitive: ordinal})."""
    w = [int(x) for x in words]
    out, q, k, idx, ordinal, n = [], 0, 0, 0, {}, 0
    for _ in range(cc):
        op = w[q]
        if op == 300:
            q += 2
            continue
        out += w[q:q + 1 + NPARAM[op]]
        q += 1 + NPARAM[op]
        n += 1
        if op in PRIMS:
            ordinal[idx] = k % 256
            out += [300, k % 256]
            idx += 2
            k += 1
        else:
            idx += 1
    return n + k, np.asarray(out, dtype=np.uint32), ordinal


def sample_points(cc, words, n, seed):
    """Random points, near-surface points, exact primitive centres (sqrt(0)), 1e-20 offsets, |p| ~ 1e4, inf and NaN."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-4, 4, (n, 3)).astype(F)]
    centres, surf = [], []
    for _, op, p in commands(words, cc):
        if op in (0, 1, 10):
            c = p[:3]
            centres.append(c)
            r = p[3]
            for ax in range(3):
                e = np.zeros(3, dtype=F)
                e[ax] = r if op != 1 else p[3 + ax]
                surf += [c + e, c - e]
    if centres:
        c = np.asarray(centres, dtype=F)
        s = np.asarray(surf, dtype=F)
        parts += [c, c + F(1e-20), c - F(1e-20), np.repeat(s, 20, axis=0) + rng.normal(0, 1e-4, (len(s) * 20, 3)).astype(F)]
    parts += [rng.uniform(-1e4, 1e4, (200, 3)).astype(F),
              np.array([[np.inf, 0, 0], [0, -np.inf, 1], [np.nan, 0, 0], [1, 2, np.nan], [np.inf, np.inf, np.inf],
                        [0, 0, 0], [-0.0, -0.0, -0.0], [1e-30, -1e-30, 1e-38]], dtype=F)]
    return np.ascontiguousarray(np.concatenate(parts).astype(F))


def oracle_taps_normal(cc, words, max_dist, p):
    eps = F(0.0001)
    f = [onp.map_scene(cc, words, max_dist, p[:, 0] + F(kx) * eps, p[:, 1] + F(ky) * eps, p[:, 2] + F(kz) * eps)
         for kx, ky, kz in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx = ((f[0] + -f[1]) + -f[2]) + f[3]
        ny = ((-f[0] + -f[1]) + f[2]) + f[3]
        nz = ((-f[0] + f[1]) + -f[2]) + f[3]
        nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
        return np.stack([nx / nl, ny / nl, nz / nl], axis=1)


@pytest.mark.parametrize("name", sorted(ALL_SCENES) + ["empty"])
def test_points_vs_oracle(res, oracle, name):
    if name == "empty":
        cc, w = 0, np.zeros(0, dtype=np.uint32)
    else:
        cc, w = oracle.serialize(*ALL_SCENES[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    p = sample_points(cc, w, 100000, seed=len(name))
    q = res.query_points(p, normals=True)
    with np.errstate(all="ignore"):
        d, m = onp.map_scene(cc, w, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
    assert same(q["distance"], d), name
    assert same(q["material"], m), name
    if cc == 0:
        assert np.all(q["leaf"] == _ffi.RM_NO_ID) and np.all(q["distance"] == F(LIM[1]))
    sub = np.random.default_rng(1).choice(len(p), 300, replace=False)
    for i in sub:   # the C oracle on a subsample
        assert same(F(oracle.map_scene(cc, w, p[i], LIM)), q["distance"][i]), (name, p[i])
        assert oracle.map_scene_material(cc, w, p[i], LIM) == int(q["material"][i]), (name, p[i])
    nsub = p[::7]
    assert same(res.query_points(nsub, normals=True)["normal"], oracle_taps_normal(cc, w, F(LIM[1]), nsub)), name
    # without the normals (the distance + ids kernel): the same bits; every other combination: test_every_output_combination
    assert same(res.query_points(p)["distance"], q["distance"])


def real_value_programs(oracle):
    """The named scenes and four random programs: two with scaled plane normals and off-unit quaternions, the one with the
    largest error against its bound in tests/test_mesh_bound_cpu.py, and the first."""
    out = {name: oracle.serialize(*ALL_SCENES[name]()) for name in sorted(ALL_SCENES)}
    progs = B.random_programs(oracle)
    picks = [p for p in progs if "scaled" in p[0]][:2] + [p for p in progs if p[0] in ("seed 31000", "seed 31034")]
    assert len(picks) == 4
    out.update({label: (cc, w) for label, cc, w in picks})
    return out


@pytest.mark.parametrize("k", range(len(ALL_SCENES) + 4))
def test_sampled_distances_are_within_E_of_the_real_value(res, oracle, k):
    """|rm_query_points(p) - f(p)| <= E(1000) with f the binary64 evaluation (tests/scene_f64.py) and E rm_program_bound's error
    term: DESIGN.md section 15 "The evaluation error" on the kernel's own arithmetic, square root included."""
    progs = real_value_programs(oracle)
    label = list(progs)[k]
    cc, w = progs[label]
    L, E = B.program_bound(cc, w, 1000.0)
    assert np.isfinite(E), label
    p = np.random.default_rng(1000 + k).uniform(-1000.0, 1000.0, (20000, 3)).astype(F)
    res.set_limits(LIM)
    res.set_program(cc, w)
    res.set_materials(np.full((8, 3), 0.5, dtype=np.float32))                 # the random programs' tags name indices up to 7
    try:
        d = res.query_points(p)["distance"]
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
    err = np.abs(d.astype(np.float64) - scene_f64.map_scene(cc, w, LIM[1], p))
    print("%s: largest |gpu - f64| %.3g, E(1000) %.3g, ratio %.4f" % (label, float(err.max()), E, float(err.max() / E)))
    assert np.all(np.isfinite(err)), label
    assert np.all(err <= E), (label, float(err.max()), E)


@pytest.mark.parametrize("name", sorted(ALL_SCENES))
def test_leaves_carry_the_material_of_their_primitive(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    tc, tw, ordinal = tag_every_leaf(cc, w)
    res.set_limits(LIM)
    res.set_program(tc, tw)
    p = sample_points(tc, tw, 50000, seed=7)
    q = res.query_points(p)
    with np.errstate(all="ignore"):
        d, m = onp.map_scene(tc, tw, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
    assert same(q["material"], m)
    leaves = q["leaf"]
    assert set(np.unique(leaves)) <= set(ordinal), "a leaf that is not a primitive's command index"
    assert np.array_equal(np.array([ordinal[int(x)] for x in leaves], dtype=np.uint32), m)
    res.set_program(cc, w)  # the untagged program: the same leaves, shifted back to its command indices
    q0 = res.query_points(p)
    back = {idx: n for n, idx in enumerate(sorted(ordinal))}
    prim_idx = [i for i, op, _ in commands(w, cc) if op in PRIMS]
    assert np.array_equal(q0["leaf"], np.array([prim_idx[back[int(x)]] for x in leaves], dtype=np.uint32))


def march_replay(cc, words, limits, rays):
    """ray_march's loop, vectorised: kind, steps, t, position (RM_HIT_* conventions)."""
    mn, mx, it = F(limits[0]), F(limits[1]), int(limits[2])
    o, d = rays[:, :3], rays[:, 3:]
    n = len(rays)
    dist = np.zeros(n, F)
    kind = np.zeros(n, np.uint32)
    steps = np.full(n, it, np.uint32)
    t = np.full(n, np.inf, F)
    pos = np.zeros((n, 3), F)
    alive = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(it):
            if alive.size == 0:
                break
            pp = o[alive] + d[alive] * dist[alive][:, None]
            s = onp.map_scene(cc, words, mx, pp[:, 0], pp[:, 1], pp[:, 2])
            hit = s < mn
            esc = ~hit & (s > mx)
            h = alive[hit]
            kind[h], steps[h], t[h], pos[h] = 1, i + 1, dist[h], pp[hit]
            steps[alive[esc]] = i + 1
            cont = ~(hit | esc)
            dist[alive[cont]] = dist[alive[cont]] + s[cont]
            alive = alive[cont]
        miss = np.nonzero(kind == 0)[0]
        fd = (F(-1.5) - o[miss, 1]) / d[miss, 1]
        fl = miss[fd > 0]
        ft = fd[fd > 0]
        kind[fl], t[fl] = 2, ft
        pos[fl] = np.stack([o[fl, 0] + d[fl, 0] * ft, np.full(len(fl), F(-1.5)), o[fl, 2] + d[fl, 2] * ft], axis=1)
    return kind, steps, t, pos


def sample_rays(cc, words, n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-6, 6, (n, 3)).astype(F)
    d = rng.normal(0, 1, (n, 3)).astype(F)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    centres = np.asarray([p[:3] for _, op, p in commands(words, cc) if op in (0, 1, 10)] or [[0, 0, 0]], dtype=F)
    inside = np.concatenate([centres + F(0.01), centres * F(0.5)])                        # origins inside solids
    o[:len(inside)] = inside[:n]
    d[-6:] = np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, 0, 1e-30], [0, -1, 0], [0, 2.5, 0]], dtype=F)  # degenerate
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


@pytest.mark.parametrize("name", ["g1", "g8", "g32", "g32_balanced", "g8x", "g32s", "ext_mix", "xform_mix", "mat_mix"])
def test_cast_rays_vs_oracle(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    lim = (0.01, 100.0, 96)
    res.set_limits(lim)
    res.set_program(cc, w)
    rays = sample_rays(cc, w, 3000, seed=3)
    hit = res.cast_rays(rays)
    mats = scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None
    with np.errstate(all="ignore"):
        rgb = onp.ray_march(cc, w, lim, *[rays[:, k].copy() for k in range(6)], materials=mats)
    assert same(hit["rgb"], rgb.T), name
    kind, steps, t, pos = march_replay(cc, w, lim, rays)
    assert np.array_equal(hit["kind"], kind) and np.array_equal(hit["steps"], steps)
    assert same(hit["t"], t) and same(hit["position"], pos)
    s = kind == _ffi.RM_HIT_SURFACE
    assert same(hit["normal"][s], oracle_taps_normal(cc, w, F(lim[1]), pos[s]))
    f = kind == _ffi.RM_HIT_FLOOR
    assert np.all(hit["normal"][f] == np.array([0, 1, 0], F)) and np.all(hit["diffuse"][~s] == 0)
    assert np.all(hit["leaf"][~s] == _ffi.RM_NO_ID) and np.all(hit["material"][~s] == _ffi.RM_NO_ID)
    q = res.query_points(pos[s])
    assert np.array_equal(hit["leaf"][s], q["leaf"]) and np.array_equal(hit["material"][s], q["material"])
    for i in np.nonzero(s)[0][:20]:   # the C oracle on a few
        assert same(oracle.ray_march(cc, w, rays[i, :3], rays[i, 3:], lim), hit["rgb"][i]) or mats is not None


@pytest.mark.parametrize("name,W,H", [("g32", 64, 48), ("xform_mix", 64, 48), ("mat_mix", 64, 48), ("g32", 37, 29),
                                      ("mat_mix", 37, 29)])
def test_sample_rays_compose_the_drawn_image(res, oracle, name, W, H):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    lim = (0.01, 100.0, 128)
    res.set_limits(lim)
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_option(_ffi.RM_OPT_KERNEL, _ffi.RM_KERNEL_DEFAULT)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)     # the default kernel as it draws once its compiled form is ready
    img = res.draw(W, H)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 0)
    assert res.draw(W, H).tobytes() == img.tobytes()
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)
    total = np.zeros((H * W, 3), F)
    steps = 0
    for s in range(16):
        hit = res.cast_rays(res.camera_rays(W, H, sample=s))
        total = total + np.sqrt(hit["rgb"])
        steps += int(hit["steps"].astype(np.uint64).sum())
    resolved = (total / F(16)).reshape(H, W, 3)
    assert resolved.tobytes() == np.ascontiguousarray(img[..., :3]).tobytes(), name
    mats = scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None
    _, cnt = oracle.render(u, lim, cc, w, W, H, threads=4, want_counters=True, materials=mats)
    assert steps == cnt["march_steps"]
    # a block of the frame is the same rays as the whole frame's rows and columns
    blk = res.camera_rays(W, H, 5, 3, 11, 7, sample=9)
    assert blk.tobytes() == res.camera_rays(W, H, sample=9).reshape(H, W, 6)[3:10, 5:16].reshape(-1, 6).tobytes()


def test_pick(res, oracle):
    cc, w = oracle.serialize(*scenes.g1())
    W, H = 81, 61
    res.set_limits((0.01, 100.0, 64))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    h = res.pick(W, H, W // 2, H // 2)
    assert h["kind"] == _ffi.RM_HIT_SURFACE and h["leaf"] == 0 and h["material"] == 0
    assert abs(float(np.linalg.norm(h["position"])) - 1.0) < 0.02 and abs(float(np.linalg.norm(h["normal"])) - 1.0) < 1e-5
    rays = res.camera_rays(W, H)
    colours = [oracle.ray_march(cc, w, r[:3], r[3:], (0.01, 100.0, 64)) for r in rays[::7]]
    sky = [i * 7 for i, c in enumerate(colours) if not c.any()]
    floor = [i * 7 for i, c in enumerate(colours) if c[2] > c[1]]
    assert sky and floor
    hs = res.pick(W, H, sky[0] % W, sky[0] // W)
    assert hs["kind"] == _ffi.RM_HIT_NONE and hs["leaf"] == _ffi.RM_NO_ID and hs["material"] == _ffi.RM_NO_ID and hs["t"] == np.inf
    hf = res.pick(W, H, floor[0] % W, floor[0] // W)
    assert hf["kind"] == _ffi.RM_HIT_FLOOR and list(hf["normal"]) == [0.0, 1.0, 0.0] and hf["position"][1] == F(-1.5)
    # tagged: the material of the surface under the cursor (untagged surfaces carry 0; the table has 6 entries)
    res.set_program(cc + 1, np.concatenate([np.asarray(w, np.uint32), np.array([300, 3], np.uint32)]))
    ht = res.pick(W, H, W // 2, H // 2)
    assert ht["kind"] == _ffi.RM_HIT_SURFACE and ht["leaf"] == 0 and ht["material"] == 3
    assert same(ht["rgb"], np.asarray(scenes.MATERIAL_TABLE[3], F) * ht["diffuse"])


def test_device_path_and_torch(res, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    ca, wa = oracle.serialize(*scenes.g32())
    cb, wb = oracle.serialize(*scenes.mat_mix())
    res.set_limits(LIM)
    p = sample_points(ca, wa, 20000, seed=5)
    res.set_program(ca, wa)
    ha = res.query_points(p, normals=True)
    ra = res.cast_rays(sample_rays(ca, wa, 2000, seed=2))
    res.set_program(cb, wb)
    hb = res.query_points(p, normals=True)
    pt = torch.from_numpy(p).to(dev)
    # one stream: program A, query, program B, query -> A's answers, then B's
    res.set_program(ca, wa)
    qa = res.query_points(pt, normals=True)
    rt = res.cast_rays(torch.from_numpy(sample_rays(ca, wa, 2000, seed=2)).to(dev))
    res.set_program(cb, wb)
    qb = res.query_points(pt, normals=True)
    torch.cuda.synchronize()
    for h, q in ((ha, qa), (hb, qb)):
        assert q["distance"].device == dev
        for k in ("distance", "normal"):
            assert same(q[k].cpu().numpy(), h[k]), k
        for k in ("leaf", "material"):
            assert np.array_equal(q[k].cpu().numpy().view(np.uint32), h[k]), k
    for k in ("rgb", "t", "position", "normal", "diffuse"):
        assert same(rt[k].cpu().numpy(), ra[k]), k
    assert np.array_equal(rt["steps"].cpu().numpy().view(np.uint32), ra["steps"])
    for bad in (pt.to(torch.float64), pt[:, :2], pt.cpu()):
        with pytest.raises(ValueError):
            res.query_points(bad)
    # sizes around a wave and a workgroup; NULL outputs
    res.set_program(ca, wa)
    for n in (1, 63, 65, 100003):
        pn = sample_points(ca, wa, n, seed=n)[:n]
        full = res.query_points(pn, normals=True)
        t = torch.from_numpy(pn).to(dev)
        d = torch.empty(n, dtype=torch.float32, device=dev)
        res.query_points_device(n, t.data_ptr(), dist_ptr=d.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        ids = torch.empty((n, 2), dtype=torch.int32, device=dev)
        res.query_points_device(n, t.data_ptr(), ids_ptr=ids.data_ptr(), stream=_ffi.RM_STREAM_OWN)
        res.sync_context()
        torch.cuda.synchronize()
        assert same(d.cpu().numpy(), full["distance"]) and np.array_equal(ids.cpu().numpy().view(np.uint32)[:, 0], full["leaf"])
        rays = sample_rays(ca, wa, max(n, 8), seed=n)[:n]
        rgb_only = np.empty((n, 3), F)
        rc = res._L.rm_cast_rays(res._h, n, rays.ctypes.data, None, None, rgb_only.ctypes.data, 0, None)
        assert rc == _ffi.RM_OK and same(rgb_only, res.cast_rays(rays)["rgb"])
    cam = torch.empty((7 * 5, 6), dtype=torch.float32, device=dev)
    res.camera_rays(64, 48, 3, 4, 7, 5, sample=2, out=cam)
    torch.cuda.synchronize()
    assert cam.cpu().numpy().tobytes() == res.camera_rays(64, 48, 3, 4, 7, 5, sample=2).tobytes()
    # an `out` that cannot hold exactly the block, densely, is refused before anything is written
    guard = torch.full((40, 8), 7.0, dtype=torch.float32, device=dev)
    for bad in (torch.empty((1, 6), dtype=torch.float32, device=dev),        # too small for the default block
                torch.empty((7 * 5 + 1, 6), dtype=torch.float32, device=dev),
                guard[:35, :6],                                                # viewable as (n, 6) but not contiguous
                torch.empty((7 * 5, 6), dtype=torch.float64, device=dev),
                torch.empty((7 * 5, 6), dtype=torch.float32)):
        with pytest.raises(ValueError):
            res.camera_rays(64, 48, 3, 4, 7, 5, sample=2, out=bad)
    with pytest.raises(ValueError):
        res.camera_rays(1920, 1080, 960, 540, out=torch.empty((1, 6), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    # numpy: an array that is not (n, width) is refused, not reinterpreted (an (n, 6) ray array is no (2n, 3) point array)
    with pytest.raises(ValueError):
        res.query_points(np.zeros((4, 6), F))
    with pytest.raises(ValueError):
        res.cast_rays(np.zeros(12, F))
    assert res.query_points(np.zeros(3, F))["distance"].shape == (1,)
    # misaligned device arrays: RM_ERR_ARG, nothing launched
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    assert res._L.rm_query_points(res._h, 2, buf.data_ptr(), None, None, buf.data_ptr() + 36, 1, None) == _ffi.RM_ERR_ARG
    assert res._L.rm_cast_rays(res._h, 1, buf.data_ptr(), buf.data_ptr() + 68, None, None, 1, None) == _ffi.RM_ERR_ARG
    assert res._L.rm_cast_rays(res._h, 1, buf.data_ptr(), None, buf.data_ptr() + 40, None, 1, None) == _ffi.RM_ERR_ARG
    assert res._L.rm_query_points(res._h, 2, buf.data_ptr() + 2, buf.data_ptr(), None, None, 1, None) == _ffi.RM_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


@pytest.mark.parametrize("name", ["g32", "g32_balanced", "ext_mix", "mat_mix"])   # chain, tree, general loop (x2)
def test_every_output_combination(res, oracle, name):
    """Every kernel instance the entry points can pick: each subset of the outputs of rm_query_points and rm_cast_rays, on
    device memory, gives the bits of the full query."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    res.set_limits((0.01, 100.0, 96))
    res.set_program(cc, w)
    p = sample_points(cc, w, 5000, seed=13)
    full = res.query_points(p, normals=True)
    n = len(p)
    pt = torch.from_numpy(p).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for mask in range(1, 8):
        d = torch.full((n,), -1.0, device=dev) if mask & 1 else None
        nr = torch.full((n, 3), -1.0, device=dev) if mask & 2 else None
        ids = torch.full((n, 2), -7, dtype=torch.int32, device=dev) if mask & 4 else None
        res.query_points_device(n, pt.data_ptr(), d.data_ptr() if d is not None else 0, nr.data_ptr() if nr is not None else 0,
                                ids.data_ptr() if ids is not None else 0, stream=st)
        torch.cuda.synchronize()
        if d is not None:
            assert same(d.cpu().numpy(), full["distance"]), mask
        if nr is not None:
            assert same(nr.cpu().numpy(), full["normal"]), mask
        if ids is not None:
            got = ids.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:, 0], full["leaf"]) and np.array_equal(got[:, 1], full["material"]), mask
    rays = sample_rays(cc, w, 3000, seed=17)
    rfull = res.cast_rays(rays)
    rt = torch.from_numpy(rays).to(dev)
    for mask in range(1, 8):
        hit = torch.full((len(rays), 8), -1.0, device=dev) if mask & 1 else None
        ids = torch.full((len(rays), 4), -7, dtype=torch.int32, device=dev) if mask & 2 else None
        rgb = torch.full((len(rays), 3), -1.0, device=dev) if mask & 4 else None
        res.cast_rays_device(len(rays), rt.data_ptr(), hit.data_ptr() if hit is not None else 0,
                             ids.data_ptr() if ids is not None else 0, rgb.data_ptr() if rgb is not None else 0, stream=st)
        torch.cuda.synchronize()
        if hit is not None:
            h = hit.cpu().numpy()
            assert same(h[:, 0], rfull["t"]) and same(h[:, 1:4], rfull["position"]) and same(h[:, 4:7], rfull["normal"])
            assert same(h[:, 7], rfull["diffuse"]), mask
        if ids is not None:
            got = ids.cpu().numpy().view(np.uint32)
            for k, key in enumerate(("kind", "steps", "leaf", "material")):
                assert np.array_equal(got[:, k], rfull[key]), (mask, key)
        if rgb is not None:
            assert same(rgb.cpu().numpy(), rfull["rgb"]), mask


def test_errors_and_empty_calls(res, oracle):
    L = res._L
    cc, w = oracle.serialize(*scenes.mat_mix())
    res.set_program(cc, w)
    res.set_limits(LIM)
    x = np.zeros((4, 6), F)
    out = np.zeros((4, 8), F)
    assert L.rm_query_points(res._h, 4, x.ctypes.data, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_query_points(res._h, 4, None, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_cast_rays(res._h, 4, x.ctypes.data, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_query_points(res._h, 0, None, out.ctypes.data, None, None, 0, None) == _ffi.RM_OK
    assert L.rm_camera_rays(res._h, 8, 8, 0, 0, 0, 5, 0, None, 0, None) == _ffi.RM_OK
    for args in ((8, 8, 4, 0, 5, 1, 0), (8, 8, 0, 0, 1, 1, 17), (0, 8, 0, 0, 1, 1, 0), (70000, 8, 0, 0, 1, 1, 0)):
        assert L.rm_camera_rays(res._h, *args, out.ctypes.data, 0, None) == _ffi.RM_ERR_RANGE, args
    res.set_materials(scenes.MATERIAL_TABLE[:2])   # mat_mix tags up to 5: colours fail, everything else works
    rgb = np.zeros((4, 3), F)
    assert L.rm_cast_rays(res._h, 4, x.ctypes.data, None, None, rgb.ctypes.data, 0, None) == _ffi.RM_ERR_MATERIAL
    assert L.rm_cast_rays(res._h, 4, x.ctypes.data, out.ctypes.data, None, None, 0, None) == _ffi.RM_OK
    res.set_materials(scenes.MATERIAL_TABLE)
    res.set_limits((0.01, 100.0, 70000))
    assert L.rm_query_points(res._h, 4, x.ctypes.data, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_RANGE
    res.set_limits(LIM)
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    assert L.rm_query_points(res._h, 4, x.ctypes.data, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_STACK_UNDERFLOW
    res.set_program(cc, w)


def largest_program():
    """Fills the 64 KB command buffer: 8 nested translations around a right-deep union of 32 tagged spheres (a 32-deep
    stack), then a left-deep chain of tagged spheres and boxes up to the last word."""
    rng = np.random.default_rng(11)
    f = lambda *v: list(np.asarray(v, F).view(np.uint32))
    words, cc, k = [], 0, 0
    for lvl in range(8):
        words += [200] + f(0.05 * lvl, -0.03, 0.02); cc += 1
    for i in range(32):
        words += [0] + f(*rng.uniform(-2, 2, 3), rng.uniform(0.2, 0.6)) + [300, k % 256]; cc += 2; k += 1
    words += [100] * 31; cc += 31
    for lvl in range(8):
        words += [201]; cc += 1
    cap = 65536 // 4 - 1
    while True:
        if rng.random() < 0.5:
            item = [0] + f(*rng.uniform(-6, 6, 3), rng.uniform(0.05, 0.3))
        else:
            item = [1] + f(*rng.uniform(-6, 6, 3), *rng.uniform(0.05, 0.3, 3))
        item += [300, k % 256, 100 if rng.random() < 0.8 else 101]
        if len(words) + len(item) > cap:
            break
        words += item; cc += 3; k += 1
    return cc, np.asarray(words, dtype=np.uint32)


def test_largest_program(res, oracle):
    cc, w = largest_program()
    assert len(w) > 16300
    res.set_limits(LIM)
    res.set_program(cc, w)
    info = renderer.program_info(cc, w)
    assert info["has_xforms"] == 1
    p = sample_points(0, w, 3000, seed=4)
    q = res.query_points(p, normals=True)
    with np.errstate(all="ignore"):
        d, m = onp.map_scene(cc, w, F(LIM[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
    assert same(q["distance"], d) and same(q["material"], m)
    tags = {}
    for i, op, prm in commands(w, cc):
        if op == 300:
            tags[i - 1] = int(prm.view(np.uint32)[0])
    assert np.array_equal(np.array([tags[int(x)] for x in q["leaf"]], np.uint32), m)
    assert same(q["normal"][::10], oracle_taps_normal(cc, w, F(LIM[1]), p[::10]))


def test_queries_leave_the_draw_state_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_TIMING, 1)
    first = res.draw(W, H)
    before = [res.info(k) for k in (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP,
                                    _ffi.RM_INFO_PRUNED)]
    ms = res.info(_ffi.RM_INFO_KERNEL_MS)
    assert ms > 0
    res.query_points(sample_points(cc, w, 5000, seed=9), normals=True)
    res.cast_rays(res.camera_rays(W, H, sample=3))
    res.pick(W, H, 10, 10)
    after = [res.info(k) for k in (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP,
                                   _ffi.RM_INFO_PRUNED)]
    assert after == before
    assert res.info(_ffi.RM_INFO_KERNEL_MS) == ms      # the queries were not timed: nothing new to average
    assert res.draw(W, H).tobytes() == first.tobytes()
    res.set_option(_ffi.RM_OPT_TIMING, 0)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)
