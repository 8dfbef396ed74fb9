"""--mesh-out of the command lines on the GPU: supports on a small overhang scene writes the supports as a
mesh file that reads back with two triangles per counted face, closed, and the report carries the counts; the file name is checked
before any work."""
import json

import numpy as np
import pytest

from ray_marching_amd import _ffi, lattice_mesh, mesh, supports

pytestmark = pytest.mark.gpu


def run(capsys, *args):
    status = supports.main(list(args))
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    return status, json.loads(lines[0])


@pytest.mark.parametrize("ext", lattice_mesh.FORMATS)
def test_supports_mesh_out(capsys, tmp_path, ext):
    path = str(tmp_path / ("supports." + ext))
    args = ("--scene", "g8", "--res", "48", "--up", "+z")
    status, r = run(capsys, *args, "--mesh-out", path)
    m = r["mesh"]
    assert status == 0 and m["file"] == path and m["classes"] == [3, 4] and set(_ffi.CMESH_COUNT_NAMES) <= set(m)
    assert r["support_on_plate"] + r["support_on_part"] > 0 and m["faces"] > 0 and m["triangles"] == 2 * m["faces"]
    assert m["open_edges"] == 0                                                  # against every other class: closed
    got = mesh.read(path)
    assert len(got.triangles) == 2 * m["faces"]
    if ext == "stl":                                                             # an STL file is a soup: welded by position here
        v, inverse = np.unique(got.vertices, axis=0, return_inverse=True)
        got = mesh.Mesh(v, inverse.reshape(-1)[got.triangles.astype(np.int64)].astype(np.uint32))
    assert len(got.vertices) == m["vertices"] and got.is_closed()
    lo, hi = np.asarray(got.vertices).min(axis=0), np.asarray(got.vertices).max(axis=0)
    assert np.all(lo >= -2.5 - r["step"][0]) and np.all(hi <= 2.5 + r["step"][0])
    _, plain = run(capsys, *args)
    del r["mesh"]
    assert plain == r                                                            # nothing else in the report changes


def test_a_bad_file_name_is_refused_before_any_work(capsys):
    with pytest.raises(SystemExit) as e:
        supports.main(["--scene", "g8", "--res", "48", "--mesh-out", "supports.vtk"])
    assert "--mesh-out" in str(e.value)
