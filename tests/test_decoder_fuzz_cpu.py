"""The upload-time decoder (ray-marching_amd/csrc/rm_decode.h) under AddressSanitizer + UndefinedBehaviorSanitizer: it is the one
place where bytes from the host application are interpreted.  tests/cpp/decode_fuzz.cpp feeds it well-formed random programs
(every node type, transform scopes, material tags, NaN / inf parameters), the same with words flipped, tails cut and command
counts off by a few, and pure noise; every stream must be rejected with a status or decode into records that satisfy the
invariants the kernels rely on (table slots within their tables, flags only where they mean something, depths within the
machine's limits).  CPU only: GPU sanitizers are not available on this pool."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decoder_survives_random_and_damaged_programs(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "decode_fuzz"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "decode_fuzz.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), "30000"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "decoder fuzz ok" in run.stdout


def test_masked_tree_loop_equals_the_whole_program_with_the_unneeded_leaves_at_infinity(tmp_path):
    """tests/cpp/tree_keep_model.cpp: the interpreter's masked tree loop (rm_kernel_v5.h tree_keep, rm_interp.h
    map_scene_tree_masked) as a CPU model over the decoder's real per-record tables and the decision functions the kernel
    itself uses (rm_device.h rm_tree_*): for random trees, masks and leaf values, the records a mask leaves give the value of
    the whole program with the other leaves at +inf, bit for bit, on a stack one slot deeper than the program's own."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "tree_keep_model"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "tree_keep_model.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "tree keep model ok" in run.stdout


def test_elf_reader_of_the_specialiser_survives_damaged_code_objects(tmp_path):
    """tests/cpp/elf_scratch_fuzz.cpp: rm_jit.h code_object_scratch_bytes -- the reader that decides whether a register-capped kernel is
    kept, and that sees files from the on-disk kernel cache -- on a synthetic ELF64, every truncation of it, every byte damaged and
    20 000 noisy variants, under ASan + UBSan: a value or UINT32_MAX, never a read outside the buffer."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    gen = os.path.join(ROOT, "ray-marching_amd", "csrc", "generated", "rm_jit_sources.inc")
    if not os.path.exists(gen):
        from ray_marching_amd import build
        build.generate_jit_sources()
    exe = tmp_path / "elf_scratch_fuzz"
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "elf_scratch_fuzz.cpp"), "-ldl", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "elf reader fuzz ok" in run.stdout


def test_scratch_layouts_of_the_host_abi_match_the_hand_written_offsets(tmp_path):
    """tests/cpp/abi_layout_check.cpp: rm_abi_layout.h -- where the typed arrays of the host ABI's device allocations lie (dense
    and sparse mesh scratch, the three slicing layouts, the slice attributes, the mesh result) -- against the chained align16
    offsets written out by hand: regions in declaration order, 16-byte aligned, disjoint and inside the total, at the shapes
    where a count is no multiple of 4 or crosses a scan block; and strip_row_count against a direct loop over the rows."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "abi_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "abi_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "abi layout ok" in run.stdout


def test_lds_layouts_match_the_hand_written_offsets_and_the_boundary_frames_straddle_their_edges(tmp_path, oracle):
    """tests/cpp/lds_layout_check.cpp: rm_lds_layout.h -- where the arrays of the kernels' dynamic LDS lie (the miss-test tables
    of the pre-pass and the culling self-tests, the march workgroup, kernel v1) -- against the sums the host and the kernels
    wrote out before it existed, which the march kernel still writes out for its launch-dependent offsets: regions in order,
    16-byte aligned, disjoint, ending at the total; the choice of waves per tile and program placement against launch_v5's
    former formulas, and never below the launch that follows.  The programs of test_gpu_parity.LAYOUT_BOUNDARY_FRAMES go
    through the decoder and the chooser: each must come out with the waves per tile the list gives it, so that consecutive
    entries do straddle an edge of the layout."""
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    import scenes
    from test_gpu_parity import LAYOUT_BOUNDARY_FRAMES
    for (n0, wpt0, _), (n1, wpt1, _) in zip(LAYOUT_BOUNDARY_FRAMES[0::2], LAYOUT_BOUNDARY_FRAMES[1::2]):
        assert n1 == n0 + 1 and wpt1 < wpt0
    progs = tmp_path / "boundary_programs.txt"
    with open(progs, "w") as f:
        for n, wpt, in_lds in LAYOUT_BOUNDARY_FRAMES:
            cc, w = oracle.serialize(*scenes.right_deep(n))
            f.write("%d %d %d %d %d %s\n" % (n, wpt, in_lds, cc, len(w), " ".join(str(int(x)) for x in w)))
    exe = tmp_path / "lds_layout_check"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "lds_layout_check.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), str(progs)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "lds layout ok" in run.stdout and "%d programs)" % len(LAYOUT_BOUNDARY_FRAMES) in run.stdout
