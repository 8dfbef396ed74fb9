"""Regenerates tests/golden/lit_*.npy: 64 x 48 lit frames (default lighting parameters) made by
tests/light_ref.py alone -- the numpy restatement of the lighting contract on top of the numpy oracle.  They pin
light_ref-version <-> light_ref-version; the GPU is compared with light_ref itself (tests/test_gpu_lit.py).

    python tests/golden/make_lit_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import light_ref  # noqa: E402
import scenes  # noqa: E402
from oracle import cbind  # noqa: E402

W, H = 64, 48
LIMITS = (0.01, 100.0, 128)
LIT_SCENES = ("g8", "mat_mix", "ext_mix", "xform_mix")


def inputs(name):
    """(cmd_count, words, uniforms dict, material table or None) of a fixture."""
    cc, words = cbind.serialize(*{**scenes.SCENES, **scenes.EXT_SCENES, **scenes.MAT_SCENES}[name]())
    u, *_ = cbind.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    ud = {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}
    return cc, words, ud, scenes.MATERIAL_TABLE if name in scenes.MAT_SCENES else None


def path(name):
    return os.path.join(HERE, "lit_%s_%dx%d.npy" % (name, W, H))


def main():
    for name in LIT_SCENES:
        cc, words, ud, table = inputs(name)
        img, evals = light_ref.render(ud, LIMITS, cc, words, W, H, materials=table)
        np.save(path(name), img)
        print(name, "mean evaluations per pixel %.1f" % evals.mean())


if __name__ == "__main__":
    main()
