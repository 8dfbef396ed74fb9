"""Ray traversal without a GPU: the numpy reference of DESIGN.md section 18 (tests/trace_ref.py) and its standard inputs on
their own -- the populations the GPU tests rely on, soundness of the reported intervals against the oracle's sign with no
tolerance, the identities between the outputs --, the host-only library calls (rm_trace_defaults, rm_trace_rays on a NULL
context), the scratch layout of the attribute pass (tests/cpp/trace_layout_check.cpp) and the tools of
ray_marching_amd.xray against a stand-in renderer backed by the reference."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gbuffer_ref
import scenes
import trace_ref as TR
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer, xray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MAX_DIST = 100.0
SCENES = ("g8", "xform_mix", "mat_mix")
ALL = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
_results = {}


def reference(oracle, name, config):
    """trace_ref.trace of the standard rays on scene `name` under configuration `config`, computed once: (program, rays,
    parameters, K, result)."""
    if (name, config) not in _results:
        cc, w = oracle.serialize(*ALL[name]())
        p, K = TR.config(config)
        rays = TR.standard_rays()
        _results[name, config] = (cc, np.asarray(w, dtype=np.uint32), rays, p, K, TR.trace(cc, w, MAX_DIST, rays, p, K))
    return _results[name, config]


def test_the_standard_rays_are_what_the_issue_measured():
    rays = TR.standard_rays()
    assert rays.shape == (2001, 6) and rays.dtype == F and len(rays) % 64 != 0
    assert np.all(np.abs(rays[:, :3]) <= F(1.2))
    assert np.allclose(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert TR.config("level0")[0].tolist() == [0.25, 6.0, F(0.005), 1.0, 0.0, 4096.0]


@pytest.mark.parametrize("name", SCENES)
def test_populations(oracle, name):
    """Every population the GPU comparison is meant to cover is there: rays that start inside, many events per ray, rays
    that exceed K, rays that run out of steps."""
    r = reference(oracle, name, "level0")[5]
    start_inside = int(((r["flags"] & TR.RM_TRACE_START_INSIDE) != 0).sum())
    hist = np.bincount(r["events"])
    print("%s level 0: %d start inside, events histogram %s, most steps %d" % (name, start_inside, hist.tolist(), int(r["steps"].max())))
    assert start_inside > 0 and start_inside < len(r["flags"])
    assert len(hist) - 1 >= 4 and int(r["steps"].max()) < 4096
    assert not np.any(r["flags"] & TR.RM_TRACE_OUT_OF_STEPS)
    over = reference(oracle, name, "many_events")
    n_over = int((over[5]["events"] > over[4]).sum())
    out = reference(oracle, name, "out_of_steps")[5]
    n_out = int(((out["flags"] & TR.RM_TRACE_OUT_OF_STEPS) != 0).sum())
    print("%s: %d rays exceed K = 2 at level -0.05; %d rays out of steps at level 0.1 with 24 steps" % (name, n_over, n_out))
    assert n_over > 0 and n_out > 0
    assert np.all(out["steps"][(out["flags"] & TR.RM_TRACE_OUT_OF_STEPS) != 0] == 24)


@pytest.mark.parametrize("config", sorted(TR.CONFIGS))
@pytest.mark.parametrize("name", SCENES)
def test_identities(oracle, name, config):
    cc, w, rays, p, K, r = reference(oracle, name, config)
    n = len(rays)
    for k in TR.KEYS:
        assert not (r[k].dtype.kind == "f" and np.isnan(r[k]).any()), k
    assert np.array_equal(r["stored"], np.minimum(r["events"], K))
    filled = np.arange(K)[None, :] < r["stored"][:, None]
    # unfilled slots
    assert np.all(np.isposinf(r["t"][~filled])) and np.all(r["position"][~filled] == 0) and np.all(r["width"][~filled] == 0)
    assert np.all(r["kind"][~filled] == 0) and np.all(r["step"][~filled] == 0)
    assert np.all(r["leaf"] == TR.RM_NO_ID) and np.all(r["material"] == TR.RM_NO_ID) and np.all(r["normal"] == 0)   # not asked for
    # kinds alternate, starting with ENTER iff the ray did not start inside; times do not decrease; steps increase
    start_inside = (r["flags"] & TR.RM_TRACE_START_INSIDE) != 0
    end_inside = (r["flags"] & TR.RM_TRACE_END_INSIDE) != 0
    want_kind = np.where((np.arange(K)[None, :] % 2 == 0) ^ start_inside[:, None], TR.RM_TRACE_ENTER, TR.RM_TRACE_EXIT)
    assert np.array_equal(r["kind"][filled], want_kind[filled])
    t = np.where(filled, r["t"], np.inf)
    assert np.all(t[:, 1:] >= t[:, :-1]) and np.all(r["t"][filled] >= p[0]) and np.all(r["t"][filled] <= r["t_end"][:, None].repeat(K, 1)[filled])
    st = np.where(filled, r["step"], np.iinfo(np.uint32).max).astype(np.int64)
    assert np.all(np.diff(st, axis=1)[filled[:, 1:]] > 0) and np.all(r["step"][filled] <= r["steps"][:, None].repeat(K, 1)[filled])
    assert np.all(r["width"][filled] > 0)
    # parity: every crossing flips the state
    assert np.array_equal((r["events"] % 2) == 1, start_inside ^ end_inside)
    # length, recomputed from the events in the stated order (rays whose events are all stored)
    whole = r["events"] <= K
    length = np.zeros(n, dtype=F)
    t_enter = np.full(n, p[0], dtype=F)
    for k in range(K):
        on = filled[:, k]
        enter = on & (r["kind"][:, k] == TR.RM_TRACE_ENTER)
        leave = on & (r["kind"][:, k] == TR.RM_TRACE_EXIT)
        length[leave] = length[leave] + (r["t"][leave, k] - t_enter[leave])
        t_enter[enter] = r["t"][enter, k]
    length[end_inside] = length[end_inside] + (r["t_end"][end_inside] - t_enter[end_inside])
    assert whole.sum() > n // 2
    assert np.array_equal(length[whole].view(np.uint32), r["length"][whole].view(np.uint32))
    assert np.all(r["length"] >= 0) and np.all(r["length"] <= r["t_end"] - p[0])
    # the ends
    assert np.all(r["t_end"] <= p[1]) and np.all((r["t_end"] == p[1]) | ((r["flags"] & TR.RM_TRACE_OUT_OF_STEPS) != 0))
    with np.errstate(all="ignore"):
        d0 = onp.map_scene(cc, w, F(MAX_DIST), *[rays[:, k] + rays[:, 3 + k] * p[0] for k in range(3)])
    assert np.array_equal(np.asarray(d0, F).view(np.uint32), r["d_start"].view(np.uint32))
    assert np.array_equal(r["d_start"] < p[4], start_inside) and np.array_equal(r["d_end"] < p[4], end_inside)


@pytest.mark.parametrize("name", SCENES)
def test_soundness_of_the_intervals(oracle, name):
    """Between consecutive reported times (T_MIN, the events, the final t) the oracle's sign at the midpoint is the state the
    events claim, for every interval longer than 4 MIN_STEP -- no tolerance.  The intervals of a ray past its K-th event are
    not known and count as left out; at least 95 % of all intervals must be covered."""
    cc, w, rays, p, K, r = reference(oracle, name, "level0")
    n = len(rays)
    filled = np.arange(K)[None, :] < r["stored"][:, None]
    times = np.concatenate([np.full((n, 1), p[0], F), np.where(filled, r["t"], F(0)), np.zeros((n, 1), F)], axis=1)
    whole = r["events"] <= K
    times[np.arange(n), r["stored"] + 1] = np.where(whole, r["t_end"], times[np.arange(n), r["stored"]])
    start_inside = (r["flags"] & TR.RM_TRACE_START_INSIDE) != 0
    total = int((r["events"].astype(np.int64) + 1).sum())
    covered = wrong = 0
    for j in range(K + 1):                          # interval j: after j events
        known = (j < r["stored"]) | ((j == r["stored"]) & whole)
        a, b = times[:, j], times[:, j + 1]
        use = known & ((b - a) > F(4) * p[2])
        m = (a[use] + b[use]) * F(0.5)
        with np.errstate(all="ignore"):
            d = onp.map_scene(cc, w, F(MAX_DIST), *[rays[use, k] + rays[use, 3 + k] * m for k in range(3)])
        claim = start_inside[use] ^ (j % 2 == 1)
        covered += int(use.sum())
        wrong += int(((np.asarray(d, F) < p[4]) != claim).sum())
    print("%s: %d of %d intervals covered (%.1f %%), %d wrong" % (name, covered, total, 100.0 * covered / total, wrong))
    assert covered >= 0.95 * total
    assert wrong == 0


def test_attributes_are_those_of_the_points(oracle):
    cc, w, rays, p, K, plain = reference(oracle, "mat_mix", "level0")
    r = TR.trace(cc, w, MAX_DIST, rays[:300], p, K, normals=True, ids=True)
    filled = np.arange(K)[None, :] < r["stored"][:, None]
    for k in ("t", "position", "width", "kind", "step"):
        assert np.array_equal(r[k], plain[k][:300]), k
    pos = r["position"][filled]
    assert len(pos) > 100
    with np.errstate(all="ignore"):
        leaf, mat = gbuffer_ref.leaf_and_material(cc, w, F(MAX_DIST), pos[:, 0], pos[:, 1], pos[:, 2])
    assert np.array_equal(r["leaf"][filled], leaf) and np.array_equal(r["material"][filled], mat)
    assert len(set(mat.tolist())) > 1
    nl = np.linalg.norm(r["normal"][filled].astype(np.float64), axis=1)
    assert np.all(np.abs(nl[np.isfinite(nl)] - 1.0) < 1e-5) and np.isfinite(nl).sum() > 100
    assert np.all(r["normal"][~filled] == 0) and np.all(r["leaf"][~filled] == TR.RM_NO_ID)


# ---- the host-only library calls (these need the feature) ------------------------------------------------------------------
def test_defaults_and_their_error_statuses():
    L = _ffi.hip_lib()
    out = (C.c_float * 8)(*([-1.0] * 8))
    assert L.rm_trace_defaults(out, 8) == _ffi.RM_OK
    assert [float(v) for v in out[:6]] == [float(F(v)) for v in TR.DEFAULTS] and out[6] == -1.0
    assert L.rm_trace_defaults(None, 6) == _ffi.RM_ERR_NULL
    assert L.rm_trace_defaults(out, 5) == _ffi.RM_ERR_ARG and out[6] == -1.0
    assert renderer.trace_defaults() == [float(F(v)) for v in TR.DEFAULTS]
    assert _ffi.TRACE_PARAM_NAMES == TR.NAMES and _ffi.RM_TRACE_PARAMS == len(TR.NAMES)
    assert renderer.RayMarchingResources.trace_defaults() == dict(zip(TR.NAMES, renderer.trace_defaults()))
    assert (_ffi.RM_TRACE_ENTER, _ffi.RM_TRACE_EXIT) == (TR.RM_TRACE_ENTER, TR.RM_TRACE_EXIT)
    assert (_ffi.RM_TRACE_START_INSIDE, _ffi.RM_TRACE_END_INSIDE, _ffi.RM_TRACE_OUT_OF_STEPS) == (1, 2, 4)


def test_null_context_is_an_error_not_a_crash():
    L = _ffi.hip_lib()
    rays = np.zeros((2, 6), F)
    p = (C.c_float * 6)(*TR.DEFAULTS)
    cnt = np.full((2, 4), 7, np.uint32)
    assert L.rm_trace_rays(None, 2, rays.ctypes.data, p, 6, 8, 0, None, None, cnt.ctypes.data, None, 0, None) == _ffi.RM_ERR_NULL
    assert np.all(cnt == 7)


def test_scratch_layout_of_the_attribute_pass(tmp_path):
    """tests/cpp/trace_layout_check.cpp under ASan + UBSan: rml::TraceScratch against offsets written out by hand."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "trace_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "trace_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "trace layout ok" in run.stdout


# ---- the tools, against a stand-in renderer backed by the reference ---------------------------------------------------------
class Stub:
    """camera_rays / trace_rays / trace_defaults of RayMarchingResources, computed by gbuffer_ref and trace_ref."""

    def __init__(self, cc, words, ud):
        self.cc, self.words, self.ud, self.calls = cc, np.asarray(words, np.uint32), ud, []

    @staticmethod
    def trace_defaults():
        return dict(zip(TR.NAMES, [float(F(v)) for v in TR.DEFAULTS]))

    def camera_rays(self, W, H):
        py, px = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
        with np.errstate(all="ignore"):
            ro, d = gbuffer_ref.camera_rays(px.ravel(), py.ravel(), gbuffer_ref.RM_SAMPLE_CENTER, self.ud, W, H)
        n = W * H
        return np.ascontiguousarray(np.stack([np.full(n, ro[0], F), np.full(n, ro[1], F), np.full(n, ro[2], F), d[0], d[1], d[2]], axis=1))

    def trace_rays(self, rays, directions=None, *, max_events=8, normals=False, ids=True, **named):
        assert directions is None
        named = {k: v for k, v in named.items() if v is not None}
        named.setdefault("step_scale", 1.0)          # a sphere: L = 1
        self.calls.append(dict(named, max_events=max_events, normals=normals, ids=ids))
        return TR.trace(self.cc, self.words, MAX_DIST, rays, TR.params(**named), max_events, normals=normals, ids=ids)


def sphere_stub(oracle, W, H):
    cc, w = oracle.serialize(*scenes.g1())           # the unit sphere at the origin
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    return Stub(cc, w, ud)


def test_thickness_image_of_a_sphere(oracle, tmp_path):
    W, H = 33, 21
    stub = sphere_stub(oracle, W, H)
    img = xray.thickness_image(stub, W, H, t_max=20.0)
    assert img.shape == (H, W) and img.dtype == F
    assert stub.calls[-1]["max_events"] == 1 and not stub.calls[-1]["ids"] and not stub.calls[-1]["normals"]
    # the centre pixel's ray runs along an axis of the sphere: through its centre
    centre = stub.camera_rays(W, H)[(H // 2) * W + W // 2].astype(np.float64)
    o, d = centre[:3], centre[3:]
    assert np.linalg.norm(o - d * (o @ d)) < 1e-5
    ev = stub.trace_rays(centre.astype(F)[None, :], max_events=2, ids=False, t_max=20.0)
    assert ev["kind"][0].tolist() == [TR.RM_TRACE_ENTER, TR.RM_TRACE_EXIT]
    tol = float(ev["width"][0, 0]) + float(ev["width"][0, 1])        # each event lies within its width of the true crossing
    got = float(img[H // 2, W // 2])
    print("thickness at the centre pixel %.9g, widths %s" % (got, ev["width"][0].tolist()))
    assert abs(got - 2.0) <= tol
    # (the widths are whole sphere-tracing steps here -- the first step from the camera lands on the surface --, so that bound is
    # loose.  Along a ray through the centre D(t) = |t - 5| - 1 is piecewise linear and the vertex rule exact up to rounding:
    # a few operations on values below 8, each within 2^-24 relative, say 16 ulp of 8 in all)
    assert abs(got - 2.0) <= 16 * 2.0 ** -21
    assert got == float(ev["length"][0]) and img.max() <= 2.0 + 16 * 2.0 ** -21 and img[0, 0] == 0 and (img > 0).sum() > 10
    # the files: float32 values and a 16-bit greyscale PNG scaled to the largest value
    npy, png = xray.write_thickness(img, str(tmp_path / "sphere"))
    assert np.array_equal(np.load(npy), img)
    data = open(png, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">IIBB", data[16:26]) == (W, H, 16, 0) and data.endswith(b"IEND\xaeB`\x82")
    n_idat = struct.unpack(">I", data[33:37])[0]
    rows = np.frombuffer(zlib.decompress(data[41:41 + n_idat]), np.uint8).reshape(H, 1 + 2 * W)
    px = rows[:, 1:].copy().view(">u2")
    assert np.all(rows[:, 0] == 0) and px.max() == 65535 and px[0, 0] == 0
    assert np.array_equal(px, np.rint(img.astype(np.float64) * (65535.0 / float(img.max()))).astype(">u2"))


def test_wall_thickness_of_a_sphere(oracle, capsys):
    stub = sphere_stub(oracle, 9, 9)
    rng = np.random.default_rng(5)
    nrm = rng.normal(0, 1, (257, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    mesh = type("M", (), {"vertices": nrm.copy(), "normals": nrm.copy()})()
    mesh.normals[7] = np.nan                         # a vertex without a normal
    thick, out = xray.wall_thickness(stub, mesh, t_max=5.0)
    assert stub.calls[-1]["t_min"] == pytest.approx(4 * 0.001) and thick.shape == (257,) and thick.dtype == F
    assert np.isnan(thick[7]) and np.isfinite(np.delete(thick, 7)).all()
    ok = np.delete(np.arange(257), 7)
    assert np.all((out["flags"][ok] & TR.RM_TRACE_START_INSIDE) != 0) and np.all(out["kind"][ok, 0] == TR.RM_TRACE_EXIT)
    # the chord through the centre is 2; the exit lies within its width of the true one, and the vertex and its direction
    # are rounded to binary32 (a few 2^-24 on a length of 2)
    assert np.all(np.abs(thick[ok].astype(np.float64) - 2.0) <= out["width"][ok, 0].astype(np.float64) + 1e-6)
    s = xray.summary(thick)
    assert s["vertices"] == 257 and s["no_normal"] == 1 and s["no_exit"] == 0 and abs(s["min"] - 2.0) < 0.01 and abs(s["p50"] - 2.0) < 0.01
    # a ray that finds no exit before t_max
    short, _ = xray.wall_thickness(stub, mesh, t_max=1.0)
    assert np.all(np.isposinf(np.delete(short, 7))) and xray.summary(short)["no_exit"] == 256
