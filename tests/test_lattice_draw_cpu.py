"""The lattice draw without a GPU: the two numpy restatements of the traversal agree with each other, on the
degenerate rays too, and with the exact hit cell in Fractions on generic rays; the window and the palette rule; the traversal the
kernels run (csrc/rm_lattice_walk.h), compiled for the host under ASan + UBSan, against itself without the brick jumps and against
the restatement, word for word; the enums of the three faces; the command line's image options up to the library call."""
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_cases as LC
import lattice_draw_ref as LR
from ray_marching_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(2, 2, 2), (3, 5, 7), (9, 8, 7), (17, 16, 15)]


def same_records(a, b):
    """Two traversals' (hit, t, axis, up, cell): the same rays hit, and the hits carry the same record, t bit for bit."""
    ha, ta, aa, ua, ca = a
    hb, tb, ab, ub, cb = b
    if not np.array_equal(ha, hb):
        return False
    h = ha
    faced = h & (aa != LR.NONE)
    return (np.array_equal(ta[h].view(np.uint32), tb[h].view(np.uint32)) and np.array_equal(aa[h], ab[h]) and np.array_equal(ca[h], cb[h])
            and np.array_equal(ua[faced], ub[faced]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", LC.CONTENTS)
def test_the_two_restatements_agree(shape, kind):
    cls = LC.contents(shape, kind, seed=sum(shape))
    rays = np.concatenate([LC.random_rays(shape, 240), LC.degenerate_rays(shape)])
    for window in [None] + LC.windows(shape)[:2]:
        a = LR.walk(cls, LC.ORIGIN, LC.STEP, rays, window)
        b = LR.merge(cls, LC.ORIGIN, LC.STEP, rays, window)
        assert same_records(a, b), (shape, kind, window)
        if kind == "full" and window is None:
            assert a[0].any() and not a[0].all()


def test_generic_rays_hit_the_exact_cell():
    """The hit cell of the binary32 walk is the hit cell of exact arithmetic wherever no two events lie closer than 2^-10 in t.
    Steps of 4 to 8 units keep the events apart: the oracle alone excludes at most 5 % of the rays."""
    shape, origin, step = (9, 7, 5), np.asarray([-16.0, 3.0, -11.0], dtype=F), np.asarray([4.0, 6.5, 8.0], dtype=F)
    cls = LC.contents(shape, "sparse", seed=5)
    cls[2:4, 3:5, 4:7] = 9
    rays = LC.random_rays(shape, 600, seed=7, origin=origin, step=step)
    hit, t, axis, up, cell = LR.walk(cls, origin, step, rays)
    generic = compared = 0
    for i, ray in enumerate(rays):
        g, h, c = LR.exact_cell(cls, origin, step, ray)
        if not g:
            continue
        generic += 1
        assert bool(hit[i]) == h, (i, ray)
        if h:
            compared += 1
            assert tuple(cell[i]) == c, (i, ray)
    assert generic >= 0.95 * len(rays), generic
    assert compared >= 100


def test_window_is_the_lattice_zeroed_outside_it():
    """For rays without ties at the window's faces -- random ones -- every word: a plane's t is a function of the plane alone, so
    a ray that walks to the window through emptied cells arrives with the record of one that is clipped to it.  (A ray through an
    edge or a vertex of the window's box is clipped by the window's rule, T0 < T1, and may pass outside: the degenerate rays are
    compared with the restatement, window and all, instead.)"""
    shape = (17, 16, 15)
    cls = LC.contents(shape, "random", seed=3)
    rays = LC.random_rays(shape, 600)
    for w in LC.windows(shape):
        cut = np.zeros_like(cls)
        cut[w[2]:w[5], w[1]:w[4], w[0]:w[3]] = cls[w[2]:w[5], w[1]:w[4], w[0]:w[3]]
        a = LR.cast(cls, LC.ORIGIN, LC.STEP, rays, LC.PALETTE, window=w)
        b = LR.cast(cut, LC.ORIGIN, LC.STEP, rays, LC.PALETTE)
        for key in ("ids", "hit", "rgb"):
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (w, key)
    assert (a["ids"][:, 0] == LR.RM_HIT_SURFACE).sum() > 20


def test_palette_rule():
    assert LR.palette_index([1, 4, 5, 255], 5).tolist() == [1, 4, 4, 4] and LR.palette_index([1, 200], 1).tolist() == [0, 0]
    cls = np.zeros((2, 2, 2), dtype=np.uint8)
    cls[0, 0, 0], cls[1, 1, 1] = 2, 200
    rays = np.asarray([[-3, 0, 0, 1, 0, 0], [4, 1, 1, -1, 0, 0]], dtype=F)
    out = LR.cast(cls, (0, 0, 0), (1, 1, 1), rays, LC.PALETTE)
    assert out["ids"][:, 2].tolist() == [2, 200] and out["ids"][:, 3].tolist() == [0, 1]           # faces -x and +x
    k = out["hit"][:, 7]
    assert np.array_equal(out["rgb"][0], np.asarray(LC.PALETTE[2], dtype=F) * k[0])
    assert np.array_equal(out["rgb"][1], np.asarray(LC.PALETTE[4], dtype=F) * k[1])                # min(200, 5 - 1)
    assert out["hit"][0, :4].tolist() == [2.5, -0.5, 0.0, 0.0] and out["hit"][0, 4:7].tolist() == [-1.0, 0.0, 0.0]
    # an origin inside a full cell: t = 0, no face, diffuse 0.02; a miss above the floor plane: the checker
    inside = LR.cast(cls, (0, 0, 0), (1, 1, 1), np.asarray([[0.25, 0.0, 0.125, 0, 1, 0], [0, 5, 0, 0, -1, 0.001]], dtype=F), LC.PALETTE)
    assert inside["ids"][0].tolist() == [LR.RM_HIT_SURFACE, 0, 2, LR.FACE_NONE] and inside["hit"][0].tolist() == [0, 0.25, 0, 0.125, 0, 0, 0, float(F(0.02))]
    assert inside["ids"][1].tolist() == [LR.RM_HIT_SURFACE, 0, 2, 3]                                  # the floor never occludes


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/cpp/lattice_layout_check.cpp under ASan + UBSan."""
    exe = tmp_path_factory.mktemp("lattice") / "lattice_layout_check"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"),
                            "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "lattice_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    return str(exe)


def test_lattice_layout_check(host_program):
    """rml::LatticeSlot against offsets written out by hand, the build kernel's indexing, and the traversal with the brick jumps
    against the one without, inside allocations of exactly the described sizes."""
    run = subprocess.run([host_program], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "lattice layout ok" in run.stdout


@pytest.mark.parametrize("shape,kind", [((3, 5, 7), "random"), ((17, 16, 15), "sparse"), ((17, 16, 15), "one_per_brick"),
                                        ((40, 33, 17), "hollow_brick"), ((40, 33, 17), "sparse"), ((130, 2, 2), "sparse")])
def test_the_kernels_traversal_is_the_restatement(host_program, tmp_path, shape, kind):
    """csrc/rm_lattice_walk.h as the kernels run it -- brick jumps included -- on the host: every record == the numpy walk."""
    cls = LC.contents(shape, kind, seed=11)
    rays = np.concatenate([LC.random_rays(shape, 900, seed=13), LC.degenerate_rays(shape)])
    for window in (None, LC.windows(shape)[3]):
        lo, hi = LR.window_of(shape, window)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.asarray(list(shape) + list(lo) + list(hi) + [len(rays)], dtype=np.uint32).tobytes())
            f.write(LC.ORIGIN.tobytes() + LC.STEP.tobytes() + cls.tobytes() + rays.tobytes())
        run = subprocess.run([host_program, "walk", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                             timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
        rec = np.fromfile(tmp_path / "out.bin", dtype=np.uint32).reshape(-1, 5)
        nx, ny = shape[0], shape[1]
        index = rec[:, 4].astype(np.int64)
        got = (rec[:, 0] != 0, rec[:, 1].copy().view(F), rec[:, 2].astype(np.int64), rec[:, 3] != 0,
               np.stack([index % nx, (index // nx) % ny, index // (nx * ny)], axis=1))
        want = LR.walk(cls, LC.ORIGIN, LC.STEP, rays, window)
        assert same_records(got, want), (shape, kind, window)
        assert want[0].any()


def test_enums_of_the_three_faces():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    names = re.findall(r"\b(RM_LAT_[A-Z_]+) = (\d+)", header)
    assert len(names) == 10
    for name, value in names:
        assert getattr(_ffi, name) == int(value), name
        assert re.search(r"\b%s: (c_int|u32) = %s;" % (name, value), rust), name
    assert re.search(r"#define RM_LAT_FACE_NONE 6u", header) and _ffi.RM_LAT_FACE_NONE == LR.FACE_NONE == 6
    assert len(_ffi.LAT_COUNT_NAMES) == _ffi.RM_LAT_COUNTS and len(_ffi.LAT_STAT_NAMES) == _ffi.RM_LAT_STATS
    for fn in ("rm_set_lattice", "rm_draw_lattice", "rm_cast_lattice"):
        assert re.search(r"\bint %s\(" % fn, header) and re.search(r"\bfn %s\(" % fn, rust), fn
        assert hasattr(_ffi.hip_lib(), fn)


def test_image_options():
    from ray_marching_amd import lattice_image as LI
    assert LI.parse_size("64x48") == (64, 48) and LI.parse_size("1920X1080") == (1920, 1080)
    for bad in ("64", "64x", "0x4", "axb", "64x48x3"):
        with pytest.raises(ValueError):
            LI.parse_size(bad)
    assert LI.parse_cut(None, (9, 8, 7)) is None
    assert LI.parse_cut("z:2:5", (9, 8, 7)) == (0, 0, 2, 9, 8, 5) and LI.parse_cut("X:0:9", (9, 8, 7)) == (0, 0, 0, 9, 8, 7)
    for bad in ("z:5:2", "z:0:8", "w:0:1", "z:1", "y:-1:3", "y:3:3"):
        with pytest.raises(ValueError):
            LI.parse_cut(bad, (9, 8, 7))
    cam = LI.box_camera((0, 0, 0), (0.5, 0.5, 0.5), (9, 9, 9))
    lo, hi = np.full(3, -0.25), np.full(3, 4.25)
    assert abs(np.linalg.norm(np.asarray(cam.position, dtype=np.float64)[:3] - 2.0) - 1.4 * np.linalg.norm(hi - lo)) < 1e-4          # aimed at the centre
    assert len(LI.LEGEND) == 5 and all(len(LI.LEGEND) >= len(v) for v in LI.LEGEND_NAMES.values())


class FakeResources:
    """RayMarchingResources up to the library: records what the command line asks of it."""
    device = 0

    def __init__(self, device=0):
        self.calls = []
        FakeResources.last = self

    def voxelize_mesh_box(self, vertices, triangles, resolution, margin):
        self.calls.append(("voxelize_mesh_box", len(vertices), len(triangles), resolution, margin))
        fake = self

        class Vox:
            counts = {n: 0 for n in _ffi.VOX_COUNT_NAMES}
            stats = {n: 0 for n in _ffi.VOX_STAT_NAMES}
            origin, step, shape = np.zeros(3, F), np.full(3, 0.25, F), (9, 8, 7)

            def occupancy_device(self):
                fake.calls.append(("occupancy_device",))
                return np.ones((7, 8, 9), dtype=np.uint8)
        return Vox()

    def set_lattice(self, classes, origin, step):
        self.calls.append(("set_lattice", classes.shape, tuple(float(x) for x in origin), tuple(float(x) for x in step)))

        class Lat:
            counts = {"points": int(np.count_nonzero(classes)), "bricks": 2}
            shape = classes.shape[::-1]
        Lat.origin, Lat.step = np.asarray(origin, F), np.asarray(step, F)
        return Lat()

    def set_materials(self, rgb):
        self.calls.append(("set_materials", len(rgb)))

    def set_uniforms(self, u):
        self.calls.append(("set_uniforms", tuple(u.viewport_extent)))

    def set_output_format(self, fmt):
        self.calls.append(("set_output_format", fmt))

    def draw_lattice(self, W, H, row0=0, rows=None, window=None):
        self.calls.append(("draw_lattice", W, H, window))
        img = np.zeros((H, W, 4), dtype=np.uint8)
        img[..., 0], img[..., 3] = np.arange(W, dtype=np.uint8)[None, :], 255
        return img

    def close(self):
        self.calls.append(("close",))


def test_voxelize_command_line_writes_an_image(tmp_path, monkeypatch, capsys):
    """python -m ray_marching_amd.voxelize part.stl --image out.png --size 40x30 --cut z:2:5, on a file round trip, up to the
    library: the device occupancy goes to set_lattice, the legend to set_materials, the cut to draw_lattice as a window, and the
    8-bit image comes back as a PNG of that size."""
    import json
    import struct
    import zlib
    import voxel_ref as VR
    from ray_marching_amd import mesh, renderer, voxelize
    v, t = VR.box((1, 1, 1), (3, 4, 5))
    part = tmp_path / "part.stl"
    mesh.write(mesh.Mesh(np.asarray(v, F), np.asarray(t, np.uint32)), str(part))
    monkeypatch.setattr(renderer, "RayMarchingResources", FakeResources)
    out = tmp_path / "out.png"
    assert voxelize.main([str(part), "--res", "16", "--image", str(out), "--size", "40x30", "--cut", "z:2:5"]) == 0
    report = json.loads(capsys.readouterr().out)
    assert report["image"] == {"file": str(out), "size": [40, 30], "window": [0, 0, 2, 9, 8, 5], "points": 504, "bricks": 2}
    calls = FakeResources.last.calls
    names = [c[0] for c in calls]
    assert names == ["voxelize_mesh_box", "occupancy_device", "occupancy_device", "set_lattice", "set_materials", "set_uniforms", "set_output_format", "draw_lattice",
                     "set_output_format", "close"]
    assert calls[3] == ("set_lattice", (7, 8, 9), (0.0, 0.0, 0.0), (0.25, 0.25, 0.25)) and calls[4] == ("set_materials", 5)
    assert calls[5] == ("set_uniforms", (40.0, 30.0)) and calls[6][1] == _ffi.RM_FORMAT_RGBA8_UNORM and calls[8][1] == _ffi.RM_FORMAT_RGBA32F
    assert calls[7] == ("draw_lattice", 40, 30, (0, 0, 2, 9, 8, 5))
    data = out.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (40, 30)
    n = struct.unpack(">I", data[33:37])[0]
    rows = np.frombuffer(zlib.decompress(data[41:41 + n]), dtype=np.uint8).reshape(30, 1 + 3 * 40)
    assert np.array_equal(rows[:, 1::3], np.tile(np.arange(40, dtype=np.uint8), (30, 1)))
    with pytest.raises(ValueError):
        voxelize.main([str(part), "--image", str(out), "--cut", "z:5:2"])
    with pytest.raises(SystemExit):
        voxelize.main([str(part), "--image"])


@pytest.mark.parametrize("module", ["thickness", "supports", "islands"])
def test_analysis_command_lines_take_the_image_options(module, capsys):
    import importlib
    m = importlib.import_module("ray_marching_amd." + module)
    with pytest.raises(SystemExit) as e:
        m.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--image" in text and "--size" in text and "--cut" in text
