"""The lighting contract without a GPU: its numpy restatement (tests/light_ref.py) against both
oracles where the contract promises identity, against the committed lit fixtures, and the host-only pieces of the feature
(rm_lighting_defaults, the batch driver's flags and manifest)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import light_ref
import scenes
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, orbit_batch, renderer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_lit_golden as lit_golden  # noqa: E402

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))


def _udict(u):
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


@pytest.mark.parametrize("name", sorted(ALL_SCENES) + ["empty"])
def test_identity_is_the_oracles_frame(oracle, name):
    """S = A = 0: bit for bit oracle.rm_oracle_np.render and the C oracle's render."""
    W, H = 40, 30
    if name == "empty":
        cc, w = 0, np.zeros(0, dtype=np.uint32)
    else:
        cc, w = oracle.serialize(*ALL_SCENES[name]())
    lim = scenes.LIMITS.get(name, (0.01, 100.0, 128))
    table = scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    img, evals = light_ref.render(_udict(u), lim, cc, w, W, H, materials=table, light=light_ref.params(**light_ref.IDENTITY))
    assert img.tobytes() == onp.render(_udict(u), lim, cc, w, W, H, materials=table).tobytes()
    ref, cnt = oracle.render(u, lim, cc, w, W, H, threads=4, want_counters=True, materials=table)
    assert img.tobytes() == ref.tobytes()
    assert evals.shape == (H, W) and evals.min() >= 16       # every sample ray evaluates the scene at least once
    # a row band is the frame's rows
    band, _ = light_ref.render(_udict(u), lim, cc, w, W, H, row0=7, rows=5, materials=table, light=light_ref.params(**light_ref.IDENTITY))
    assert band.tobytes() == img[7:12].tobytes()


@pytest.mark.parametrize("name", lit_golden.LIT_SCENES)
def test_defaults_match_the_fixtures_and_only_darken(oracle, name):
    cc, w, ud, table = lit_golden.inputs(name)
    W, H = lit_golden.W, lit_golden.H
    img, evals = light_ref.render(ud, lit_golden.LIMITS, cc, w, W, H, materials=table)
    assert img.tobytes() == np.load(lit_golden.path(name), allow_pickle=False).tobytes()
    assert not np.isnan(img).any()
    unlit = onp.render(ud, lit_golden.LIMITS, cc, w, W, H, materials=table)
    assert np.all(img <= unlit)                               # every channel of every pixel
    darker = np.any(img[..., :3] < unlit[..., :3], axis=2)
    if name == "g8":
        assert darker.mean() >= 0.01, darker.mean()
    # chosen pixels are the frame's pixels
    rng = np.random.default_rng(5)
    px, py = rng.integers(0, W, 50), rng.integers(0, H, 50)
    sub, sub_evals = light_ref.render_pixels(px, py, ud, lit_golden.LIMITS, cc, w, W, H, materials=table)
    assert sub.tobytes() == img[py, px].tobytes() and np.array_equal(sub_evals, evals[py, px])


def test_lighting_defaults_are_the_table():
    L = _ffi.hip_lib()
    assert renderer.lighting_defaults() == [float(F(v)) for v in light_ref.DEFAULTS]
    assert _ffi.LIGHT_NAMES == light_ref.NAMES and len(light_ref.DEFAULTS) == _ffi.RM_LIGHT_PARAMS == 13
    out = (C.c_float * 16)(*([7.0] * 16))
    assert L.rm_lighting_defaults(out, 12) == _ffi.RM_ERR_ARG and list(out) == [7.0] * 16
    assert L.rm_lighting_defaults(None, 13) == _ffi.RM_ERR_NULL
    assert L.rm_lighting_defaults(out, 16) == _ffi.RM_OK and list(out)[13:] == [7.0] * 3
    assert L.rm_set_lighting(None, out, 13) == _ffi.RM_ERR_NULL
    assert L.rm_draw_lit(None, 4, 4, 0, 4, None, 0, None) == _ffi.RM_ERR_NULL


def test_header_enum_matches_the_names():
    """enum rm_light of include/rm_abi.h: RM_LIGHT_<NAME> = index, RM_LIGHT_PARAMS = 13."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rm_abi.h")).read(), flags=re.S)
    body = re.search(r"enum\s+rm_light\s*\{(.*?)\}", text, re.S).group(1)
    consts = {n: int(v) for n, v in re.findall(r"(RM_LIGHT_[A-Z0-9_]+)\s*=\s*(\d+)", body)}
    assert consts == dict([("RM_LIGHT_" + n.upper(), i) for i, n in enumerate(light_ref.NAMES)] + [("RM_LIGHT_PARAMS", 13)])


def test_orbit_batch_flags_and_manifest(tmp_path):
    a = orbit_batch.parse(["--out-dir", str(tmp_path / "lit"), "--lit", "--shadow", "0.5", "--ao", "0.25", "--light", "1", "-4", "2.5"])
    assert a.lit and a.shadow == 0.5 and a.ao == 0.25 and a.light == [1.0, -4.0, 2.5]
    assert orbit_batch.lighting_of(a) == {"lit": True, "shadow": 0.5, "ao": 0.25, "light": [1.0, -4.0, 2.5]}
    b = orbit_batch.parse(["--out-dir", str(tmp_path / "plain")])
    assert not b.lit and orbit_batch.lighting_of(b) is None
    # an unlit job's manifest is what it always was: exactly these keys, also for a Namespace that predates the flags
    for args in (b, argparse.Namespace(out_dir=str(tmp_path / "old"), frames=1024, width=3840, height=2160, scene="g32",
                                       max_iter=256, format="ppm")):
        os.makedirs(args.out_dir)
        orbit_batch.check_manifest(args)
        with open(os.path.join(args.out_dir, "orbit.json")) as fh:
            assert fh.read() == json.dumps({"frames": 1024, "width": 3840, "height": 2160, "scene": "g32", "max_iter": 256,
                                            "format": "ppm"})      # byte for byte
        orbit_batch.check_manifest(args)                     # resumes
    os.makedirs(a.out_dir)
    orbit_batch.check_manifest(a)
    with open(os.path.join(a.out_dir, "orbit.json")) as fh:
        have = json.load(fh)
    assert have["lit"] is True and have["shadow"] == 0.5 and have["ao"] == 0.25 and have["light"] == [1.0, -4.0, 2.5]
    with pytest.raises(SystemExit):                          # a lit directory refuses an unlit run, and other lighting
        orbit_batch.check_manifest(argparse.Namespace(**dict(vars(a), lit=False)))
    with pytest.raises(SystemExit):
        orbit_batch.check_manifest(argparse.Namespace(**dict(vars(a), shadow=1.0)))
