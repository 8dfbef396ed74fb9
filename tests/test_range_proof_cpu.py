"""The range proofs of the generated march kernel without a GPU (csrc/rm_interp.h "Range proofs"): the stand-alone program
tests/cpp/range_proof_check.cpp under ASan + UBSan (the decoder's verdict on box sizes, the box lemma over every binade, the
numerator lemma over every significand), the box lemma again in numpy, and how the variant is wired: a compile definition in front
of an unchanged translation unit, taken only by kernels that have the variant."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ray_marching_amd import _ffi, csg, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("range_proof") / "range_proof_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(out),
                            os.path.join(ROOT, "tests", "cpp", "range_proof_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_facts_and_lemmas_in_the_stand_alone_program(exe):
    out = run(exe)
    assert "range proofs ok" in out and "box lemma:" in out, out


@pytest.mark.parametrize("half,normal", [((0.3, 0.25, 0.2), 1), ((2.0 ** -23, 0.25, 0.2), 1), ((1.0e-9, 0.25, 0.2), 0), ((0.3, 0.0, 0.2), 0),
                                         ((0.3, 0.25, -1.0e-8), 0), ((0.3, float("inf"), 0.2), 0), ((0.3, 0.25, float("nan")), 0),
                                         ((-0.3, -0.25, -0.2), 1)])
def test_the_decoder_says_which_box_sizes_the_lemma_covers(exe, half, normal):
    assert int(run(exe, *half).split()[-1]) == normal


def test_the_box_lemma_in_binary32_arrays():
    """m = max(fl(t - r), 0) is 0 or >= 2^-46 for |r| >= 2^-23: every binade, t within 64 ulp of r, 2 r and the binade edges"""
    e = np.arange(-23, 128)
    sig = np.array([0, 1, 2, 0x155555, 0x400000, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)
    r = (((e + 127).astype(np.uint32) << np.uint32(23))[:, None] | sig[None, :]).reshape(-1).view(F)
    d = np.arange(-64, 65, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for anchor in (r, F(2.0) * r, np.exp2(np.floor(np.log2(r.astype(np.float64)))).astype(F), np.exp2(np.floor(np.log2(r.astype(np.float64))) + 1).astype(F)):
            ok = np.isfinite(anchor)
            tb = anchor[ok].view(np.uint32).astype(np.int64)[:, None] + d[None, :]
            keep = (tb >= 0) & (tb < 0x7F800000)
            t = np.where(keep, tb, 0).astype(np.uint32).view(F)
            for sign in (F(1.0), F(-1.0)):
                q = (t - (sign * r[ok])[:, None]).astype(F)
                m = np.maximum(q, F(0.0))
                sq = (m * m).astype(F)
                assert np.all((m == 0) | (m >= F(2.0 ** -46)) | ~keep)
                assert np.all((sq == 0) | (sq >= F(2.0 ** -92)) | ~keep)
    # ... and not below 2^-23
    r0 = F(2.0 ** -50)
    q0 = F(np.nextafter(r0, F(1.0)) - r0)
    assert 0 < F(q0 * q0) < F(2.0 ** -96)


def test_the_variant_is_a_definition_in_front_of_the_same_translation_unit():
    cc, w = csg.serialize(csg.scene("g32"))
    guarded = renderer.jit_source(cc, w, 4, prune=True)
    proved = renderer.jit_source(cc, w, 4 | _ffi.RM_JIT_RANGE_PROVED, prune=True)
    assert "RM_JIT_RANGE_PROOF" not in guarded
    assert proved.replace("#define RM_JIT_RANGE_PROOF 1\n", "", 1) == guarded and proved != guarded
    # kernels without the variant take no notice: no culling (g8 unpruned), blends (g32s), a material phase (mat_mix)
    for name, prune in (("g8", False), ("g32", False), ("g32s", True), ("mat_mix", True)):
        cc, w = csg.serialize(csg.scene(name))
        assert renderer.jit_source(cc, w, 4 | _ffi.RM_JIT_RANGE_PROVED, prune=prune) == renderer.jit_source(cc, w, 4, prune=prune), name
