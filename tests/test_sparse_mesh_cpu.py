"""Sparse mesh extraction without a GPU: the symbols and constants of the new entry points, rm_program_lipschitz on fixed
programs, its soundness on the numpy oracle (no pair of points may change the distance by more than L times their
separation), its tightness against the closed form, and the Python argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import scenes
import test_gpu_fuzz
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)


def rust_text():
    return open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


# ---- the C, Rust and Python faces ----------------------------------------------------------------------------------------------
def test_symbols_and_constants():
    text, rust, L = header_text(), rust_text(), _ffi.hip_lib()
    for name in ("rm_extract_mesh_sparse", "rm_program_lipschitz"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    body = re.search(r"enum\s+rm_meshstat\s*\{(.*?)\}", text, re.S).group(1)
    consts = {n: int(v) for n, v in re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)}
    assert consts == {"RM_MESH_STAT_VERTICES": 0, "RM_MESH_STAT_TRIANGLES": 1, "RM_MESH_STAT_BRICKS": 2, "RM_MESH_STAT_BRICKS_KEPT": 3,
                      "RM_MESH_STAT_EVALUATIONS": 4, "RM_MESH_STAT_SCRATCH_BYTES": 5, "RM_MESH_STATS": 6}
    for name, value in consts.items():
        assert getattr(_ffi, name) == value
        assert re.search(r"pub const %s: c_int = %d;" % (name, value), rust), name
    assert len(_ffi.MESH_STAT_NAMES) == _ffi.RM_MESH_STATS
    assert re.search(r"#define RM_ABI_VERSION 2\b", text) and L.rm_abi_version() == 2
    o, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    stats = (C.c_uint64 * _ffi.RM_MESH_STATS)()
    assert L.rm_extract_mesh_sparse(None, o, s, 4, 4, 4, 0.0, 0, stats, _ffi.RM_MESH_STATS) == _ffi.RM_ERR_NULL


def test_rust_wrapper_checks_its_slice():
    rust = rust_text()
    body = rust[rust.index("pub fn extract_mesh_sparse("):]
    body = body[:body.index("\n    }\n")]
    assert re.search(r"out_stats: &mut \[u64\]", body)
    assert body.index("assert!(out_stats.len() >= RM_MESH_STATS as usize") < body.index("rm_extract_mesh_sparse(")
    assert body.index("self.mesh.set(None)") < body.index("rm_extract_mesh_sparse(") < body.index("self.mesh.set(Some(")
    assert re.search(r"pub fn program_lipschitz\(cmd_count: u32, words: &\[u32\]\) -> Result<f64, c_int>", rust)


# ---- rm_program_lipschitz on fixed programs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_SCENES))
def test_lipschitz_of_the_named_scenes(oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    L = renderer.program_lipschitz(cc, w)
    if name == "ext_mix":
        assert 1.0198 <= L < 1.03, L
    else:
        assert 1.0 <= L < 1.001, L


def rotation_factor(q):
    w, a = float(q[0]), np.asarray(q[1:], dtype=np.float64)
    a2 = float(a @ a)
    return max(1.0, math.sqrt((1.0 - 2.0 * a2) ** 2 + 4.0 * w * w * a2))


def test_lipschitz_fixed_cases():
    assert renderer.program_lipschitz(0, []) == 0.0
    sphere = (0, [0.1, 0.2, 0.3, 0.5])
    assert renderer.program_lipschitz(*words_of(sphere)) == 1.0
    assert renderer.program_lipschitz(*words_of((0, [0, 0, 0, -0.3]))) == 1.0                    # negative radius
    assert renderer.program_lipschitz(*words_of((1, [0, 0, 0, 0.0, -1.0, 0.5]))) == 1.0          # degenerate extents
    assert math.isinf(renderer.program_lipschitz(*words_of((204, [0.0]), sphere, (205, []))))    # Scale 0
    assert math.isinf(renderer.program_lipschitz(*words_of((0, [0.1, np.nan, 0.3, 0.5]))))       # a NaN parameter
    assert math.isinf(renderer.program_lipschitz(*words_of(sphere, sphere, (110, [np.inf]))))
    assert renderer.program_lipschitz(*words_of((204, [-0.7]), sphere, (205, []))) == 1.0        # a negative scale: still 1
    assert renderer.program_lipschitz(*words_of((204, [1e-3]), sphere, (205, []))) == 1.0
    for q in ((2.0, 0.0, 0.0, 0.0), (1.3, 0.2, -0.4, 0.5), (0.5, 0.5, 0.5, 0.5), (0.3, 0.9, 0.1, -0.2)):
        L = renderer.program_lipschitz(*words_of((202, list(q)), sphere, (203, [])))
        qf = np.asarray(q, dtype=F)
        assert abs(L / rotation_factor(qf) - 1.0) < 1e-6, (q, L)
    assert renderer.program_lipschitz(*words_of((202, [2.0, 0.0, 0.0, 0.0]), sphere, (203, []))) == 1.0    # a = 0: the identity
    n = np.asarray([0.0, 1.0, 0.2], dtype=F).astype(np.float64)
    assert abs(renderer.program_lipschitz(*words_of((2, [0.0, 1.0, 0.2, 0.5]))) - math.sqrt(float(n @ n))) < 1e-12
    # operators take the larger operand's bound
    assert abs(renderer.program_lipschitz(*words_of(sphere, (2, [3.0, 0.0, 4.0, 0.5]), (110, [0.3]))) - 5.0) < 1e-12
    with pytest.raises(_ffi.RmError) as e:
        renderer.program_lipschitz(1, [100])
    assert e.value.status == _ffi.RM_ERR_STACK_UNDERFLOW
    assert _ffi.hip_lib().rm_program_lipschitz(0, None, 0, None) == _ffi.RM_ERR_NULL


# ---- soundness and tightness ---------------------------------------------------------------------------------------------------
def closed_form(nodes, root):
    """The product of the plane and rotation factors along the worst root-to-leaf path."""
    kind, params, lhs, rhs = nodes[root]
    if kind == scenes.PLANE:
        n = np.asarray(params[:3], dtype=F).astype(np.float64)
        return math.sqrt(float(n @ n))
    if kind in (scenes.SPHERE, scenes.BOX, scenes.CYLINDER):
        return 1.0
    if kind == scenes.ROTATION:
        return rotation_factor(np.asarray(params, dtype=F)) * closed_form(nodes, lhs)
    if kind in (scenes.TRANSLATION, scenes.SCALE, scenes.MATERIAL):
        return closed_form(nodes, lhs)
    return max(closed_form(nodes, lhs), closed_form(nodes, rhs))


def variants(rng, nodes):
    """The same tree with its planes' normals scaled to |n| in {0.5, 3} and its quaternions off the unit sphere."""
    out = []
    for kind, params, lhs, rhs in nodes:
        p = list(params)
        if kind == scenes.PLANE:
            f = float(rng.choice([0.5, 3.0]))
            p = [p[0] * f, p[1] * f, p[2] * f, p[3]]
        elif kind == scenes.ROTATION:
            f = float(rng.choice([0.8, 1.0, 1.25]))
            p = [x * f for x in p]
        out.append((kind, p, lhs, rhs))
    return out


def programs():
    for seed in range(60):
        rng = np.random.default_rng(5000 + seed)
        t = scenes._Tab()
        root = test_gpu_fuzz.random_tree(rng, t, int(rng.integers(2, 5)), allow_plane=bool(rng.random() < 0.6), tags=bool(rng.random() < 0.3))
        yield "seed %d" % seed, seed, t.nodes, root
        if any(k in (scenes.PLANE, scenes.ROTATION) for k, *_ in t.nodes):
            yield "seed %d, scaled planes and quaternions" % seed, seed, variants(rng, t.nodes), root


def point_pairs(rng, n):
    p = rng.uniform(-3.0, 3.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.01, 0.2, n) / np.linalg.norm(d, axis=1))[:, None]
    return p.astype(F), (p + d).astype(F)


def test_lipschitz_is_sound_and_tight(oracle):
    checked = scaled = 0
    worst = 0.0
    for label, seed, nodes, root in programs():
        cc, w = oracle.serialize(nodes, root)
        if oracle.validate(cc, w)[0] != 0:
            continue
        L = renderer.program_lipschitz(cc, w)
        assert math.isfinite(L) and L > 0.0, label
        expect = closed_form(nodes, root)
        assert L <= 1.05 * expect, (label, L, expect)
        p, q = point_pairs(np.random.default_rng(9000 + seed), 50000)
        with np.errstate(all="ignore"):
            dp = onp.map_scene(cc, w, F(100.0), p[:, 0], p[:, 1], p[:, 2]).astype(np.float64)
            dq = onp.map_scene(cc, w, F(100.0), q[:, 0], q[:, 1], q[:, 2]).astype(np.float64)
        sep = np.linalg.norm(p.astype(np.float64) - q.astype(np.float64), axis=1)
        excess = np.abs(dp - dq) - (L * sep * (1.0 + 1e-5) + 1e-5)
        assert np.all(np.isfinite(dp)) and np.all(np.isfinite(dq)), label
        assert np.all(excess <= 0.0), (label, L, float(excess.max()))
        worst = max(worst, float((np.abs(dp - dq) / sep).max() / L))
        checked += 1
        scaled += "scaled" in label
    assert checked >= 60 + scaled and scaled >= 15, (checked, scaled)
    print("largest |dd| / (L |dp|): %.7f over %d programs" % (worst, checked))


# ---- Python argument checks (raised before any device call) ----------------------------------------------------------------------
class _NoDevice(renderer.RayMarchingResources):
    def __init__(self):       # the argument checks only: no context
        self._L, self._h, self.device = _ffi.hip_lib(), None, 0


@pytest.mark.parametrize("lo, hi, res", [((-1, -1, -1), (1, 1, 1), 1), ((-1, -1, -1), (1, 1, 1), (8, 8, 1)),
                                         ((1, -1, -1), (1, 1, 1), 8), ((0, 0, 0), (-1, 1, 1), 8),
                                         ((-1, -1, -1), (1, 1, np.inf), 8), ((-1, -1, -1), (1, 1, 1), 2.5),
                                         ((-1, -1), (1, 1), 8)])
def test_extract_mesh_sparse_rejects_bad_boxes(lo, hi, res):
    with pytest.raises(ValueError):
        _NoDevice().extract_mesh_sparse(lo, hi, res)


@pytest.mark.parametrize("origin, step, shape", [((0, 0), (1, 1, 1), (4, 4, 4)), ((0, 0, 0), (1, 0, 1), (4, 4, 4)),
                                                 ((0, 0, 0), (1, -1, 1), (4, 4, 4)), ((0, np.nan, 0), (1, 1, 1), (4, 4, 4)),
                                                 ((0, 0, 0), (1, 1, 1), (4, 4)), ((0, 0, 0), (1, 1, 1), (4, 1, 4))])
def test_extract_mesh_grid_sparse_rejects_bad_lattices(origin, step, shape):
    with pytest.raises(ValueError):
        _NoDevice().extract_mesh_grid_sparse(origin, step, shape)


class _Recorder:
    """Stands in for the library: records the 3 floats behind each lattice pointer, then fails the call."""

    def __init__(self):
        self.calls = []

    def rm_extract_mesh_sparse(self, h, o, s, nx, ny, nz, level, flags, stats, n_stats):
        self.calls.append(([o[k] for k in range(3)], [s[k] for k in range(3)], (nx, ny, nz), level, flags, n_stats))
        return _ffi.RM_ERR_ARG


def test_scalar_and_broadcast_lattices_reach_the_library_as_three_values():
    r = _NoDevice()
    rec = r._L = _Recorder()
    with pytest.raises(_ffi.RmError):
        r.extract_mesh_sparse(-2.5, 2.5, 1024, level=0.25, normals=False)
    assert rec.calls[-1] == ([-2.5] * 3, [float(F(5.0) / F(1023.0))] * 3, (1024, 1024, 1024), 0.25, _ffi.RM_MESH_IDS, _ffi.RM_MESH_STATS)
    with pytest.raises(_ffi.RmError):
        r.extract_mesh_sparse((-1.0, -2.0, -3.0), 2.0, (9, 17, 33))
    assert rec.calls[-1][:3] == ([-1.0, -2.0, -3.0], [float(F(3.0) / F(8.0)), float(F(4.0) / F(16.0)), float(F(5.0) / F(32.0))],
                                 (9, 17, 33))
    view = np.broadcast_to(F(1.5), (3,))
    strided = np.arange(6, dtype=F)[::2] + F(0.25)
    with pytest.raises(_ffi.RmError):
        r.extract_mesh_grid_sparse(view, strided, (8, 8, 8))
    assert rec.calls[-1][:3] == ([1.5] * 3, [0.25, 2.25, 4.25], (8, 8, 8))


def test_cli_has_the_sparse_flag(capsys):
    from ray_marching_amd import mesh as M
    with pytest.raises(SystemExit):
        M.main(["--help"])
    assert "--sparse" in capsys.readouterr().out
