"""The union-find of the topology merge pass (csrc/rm_topo_union.h) run on CPU threads:
tests/cpp/topo_union_model.cpp includes the header the kernels include and unites random occupancies with 8 threads, then
requires after ONE merge pass that no adjacent same-class pair has different roots and that every root is the smallest index of
its component.  Built plain, under ThreadSanitizer (a stand-alone binary, nothing preloaded), and once with a deliberately torn
minimum, which must fail: the model can see a lost union.  No GPU."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "topo_union_model.cpp")
OK_LINE = "topo union model ok: 40 seeds x 4 densities x 2 modes on 33 x 20 x 17 points, 8 threads, one merge pass each"


def build_and_run(tmp_path, name, flags, fixed_addresses=False):
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path / name
    build = subprocess.run([cxx, "-std=c++17", "-pthread", *flags, "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe), SOURCE],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    setarch = shutil.which("setarch") if fixed_addresses else None
    if setarch:                                                               # this process alone, no setting of the machine's
        run = subprocess.run([setarch, platform.machine(), "-R", str(exe)], capture_output=True, text=True, timeout=600)
        if "setarch" not in run.stderr:
            return run
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)


def test_one_merge_pass_unites_everything(tmp_path):
    run = build_and_run(tmp_path, "topo_union_model", ["-O2"])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.strip().splitlines()[-1] == OK_LINE


def test_one_merge_pass_under_thread_sanitizer(tmp_path):
    """ThreadSanitizer keeps its shadow memory at fixed addresses.  A kernel that randomises 32 bits of every mapping places the
    program inside them now and then, and the runtime gives up before main(); so the program runs with address randomisation off
    where setarch can do that.  Where the runtime still cannot start, nothing was tested: skipped, with its message."""
    run = build_and_run(tmp_path, "topo_union_model_tsan", ["-O1", "-g", "-fsanitize=thread"], fixed_addresses=True)
    if run.returncode == 66 and "ThreadSanitizer: unexpected memory mapping" in run.stderr and not run.stdout:
        pytest.skip("ThreadSanitizer cannot start here: " + run.stderr.strip()[-200:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ThreadSanitizer" not in run.stderr
    assert run.stdout.strip().splitlines()[-1] == OK_LINE


def test_the_model_sees_a_torn_minimum(tmp_path):
    """-DTOPO_MODEL_TORN_MIN: the model's own minimum becomes load / yield / conditional store; the shared header is the same."""
    run = build_and_run(tmp_path, "topo_union_model_torn", ["-O2", "-DTOPO_MODEL_TORN_MIN"])
    print(run.stdout[-500:])
    assert run.returncode == 1, (run.stdout + run.stderr)[-3000:]
    assert "FAILED: seed" in run.stdout and "ok" not in run.stdout
