"""The unit table of wave-level culling as it is staged in LDS (ray-marching_amd/csrc/rm_kernel_v5.h stage_units), without a GPU:
tests/cpp/unit_table_probe.cpp runs the staging loop of every thread of a workgroup with the mapping the kernel itself uses
(rm_device.h rm_unit_table_source) over unit records whose dword j of unit u holds 100 u + j.

the arrangement   dwords [0, 4 n) hold one float4 per unit -- fields 0 .. 3 of RmDecoded::units[u].p, the record's dwords 1 .. 4:
                  what wave_cull_lattice and unit_bounds read with one 16-byte read at 4 * lane;
                  rows 4 .. 6 hold fields 4 .. 6 (the record's dwords 5 .. 7) at f n + u, row 7 the record's first word at 7 n + u:
                  what unit_bounds, tree_keep's base (8 n) and map_scene_units (row 7) read, where they always were.
the staging       every dword of the table is written exactly once, whatever the number of threads (one wave of the self-test,
                  1, 2, 4 and 8 waves per tile of the march), and nothing outside it.
n_units 1, 16, 17, 32, 63 and 64: one unit, the metric scene's 16, a count that is no multiple of 4 or of a row of 16 lanes, and
the two ends of the last row of the mask."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_UNITS = (1, 16, 17, 32, 63, 64)
N_THREADS = (64, 128, 256, 512)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("unit_table") / "unit_table_probe"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ray-marching_amd", "csrc"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "cpp", "unit_table_probe.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    text = "".join("%d %d\n" % (n, t) for n in N_UNITS for t in N_THREADS)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert [(d["n_units"], d["n_threads"]) for d in out] == [(n, t) for n in N_UNITS for t in N_THREADS]
    return out


def test_fields_0_to_3_stand_together_one_float4_per_unit(tables):
    for d in tables:
        n, t = d["n_units"], d["table"]
        for u in range(n):
            assert t[4 * u:4 * u + 4] == [100 * u + 1 + f for f in range(4)], (n, d["n_threads"], u)


def test_rows_4_to_7_are_where_they_were(tables):
    for d in tables:
        n, t = d["n_units"], d["table"]
        for f in (4, 5, 6):
            assert t[f * n:(f + 1) * n] == [100 * u + 1 + f for u in range(n)], (n, d["n_threads"], f)
        assert t[7 * n:8 * n] == [100 * u for u in range(n)], (n, d["n_threads"])       # the record's first word: first | last << 16


def test_every_dword_is_written_once_and_the_table_is_a_permutation_of_the_records(tables):
    for d in tables:
        n = d["n_units"]
        assert len(d["table"]) == 8 * n and d["writes"] == [1] * (8 * n), (n, d["n_threads"])
        assert sorted(d["table"]) == sorted(100 * u + j for u in range(n) for j in range(8)), (n, d["n_threads"])
