"""Retained results: what a producing call leaves in the context for rm_read_*, and the Python result objects
that read it on demand.  rm_read_* copies the size of the context's LAST result, so an object that stands for an earlier one must
refuse to read: with a strictly larger second lattice the library would otherwise write past the first one's arrays.  Also here:
a failed call leaves the serial alone, the two serials of a distance volume and its mask, absent outputs on both destinations of
the eager readers, and the refusals of the six rm_read_* around the read path they share, message for message.

That the device and the host destination of extract_mesh* and slice_contours* give the same words with every output present is
asserted by test_gpu_mesh.py::test_attributes_are_those_of_the_point_query,
test_gpu_sparse_mesh.py::test_sparse_and_dense_share_the_context_mesh_and_leave_draws_alone and test_gpu_slice.py::test_device_reads;
the case here is the one with outputs left out."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_topology import scene_program, use
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

SMALL, LARGE = (2, 3, 4), (8, 8, 8)                 # (nz, ny, nx): a first lattice of 4 x 3 x 2 points, a second of 8 x 8 x 8
UP, R2 = "+z", 1


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    use(r, *scene_program("g8"))
    yield r
    r.close()


@pytest.fixture(scope="module")
def occupancies():
    rng = np.random.default_rng(24)
    return {shape: np.ascontiguousarray(rng.random(shape) < 0.4).view(np.uint8) for shape in (SMALL, LARGE)}


# per family: the call, the readers of its result object, and the raw read of the context's last result in the readers' order
def raw_topology(res, got):
    out = np.full(got.shape[::-1], 0x5A5A5A5A, np.uint32)
    res._check(res._L.rm_read_topology(res._h, None, None, out.ctypes.data, 0, None))
    return [out]


def raw_distance(res, got):
    out = np.full(got.shape[::-1], 0x5A5A5A5A, np.uint32)
    res._check(res._L.rm_read_distance(res._h, out.ctypes.data, None, 0, None))
    return [out]


def raw_support(res, got):
    out = [np.full(got.shape[::-1], 0x5A, np.uint8), np.full((got.layers, 4), 0x5A5A5A5A, np.uint32)]
    res._check(res._L.rm_read_support(res._h, out[0].ctypes.data, out[1].ctypes.data, 0, None))
    return out


def raw_islands(res, got):
    R = got.counts["regions"]
    out = [np.full(R * _ffi.RM_ISL_ROW_WORDS, 0x5A5A5A5A, np.uint32).view(renderer.ISL_ROW_DTYPE),
           np.full(got.shape[::-1], 0x5A5A5A5A, np.uint32), np.full(got.shape[::-1], 0x5A, np.uint8),
           np.full((got.layers, 4), 0x5A5A5A5A, np.uint32)]
    res._check(res._L.rm_read_islands(res._h, out[0].ctypes.data if R else None, R, *[a.ctypes.data for a in out[1:]], 0, None))
    return out


FAMILIES = {
    "topology": (lambda res, occ: res.label_occupancy(occ), ("labels",), raw_topology),
    "distance": (lambda res, occ: res.distance_occupancy(occ), ("d2",), raw_distance),
    "support": (lambda res, occ: res.support_occupancy(occ, up=UP, r2=R2), ("mask", "profile"), raw_support),
    "islands": (lambda res, occ: res.islands_occupancy(occ, up=UP, r2=R2), ("rows", "labels", "mask", "profile"), raw_islands),
}


def read_all(got, readers):
    return [getattr(got, name)() for name in readers]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_result_replaced_by_a_larger_one_refuses_to_read(res, occupancies, family):
    call, readers, raw = FAMILIES[family]
    a = call(res, occupancies[SMALL])
    first = read_all(a, readers)
    assert all(same(x, y) for x, y in zip(first, raw(res, a)))
    b = call(res, occupancies[LARGE])
    for name in readers + (("features",) if family == "distance" else ()):
        with pytest.raises(ValueError) as e:
            getattr(a, name)()
        assert type(a).__name__ in str(e.value) and "_occupancy" in str(e.value), str(e.value)   # the object and the newer call
    got = read_all(b, readers)
    assert b.shape == LARGE[::-1] and [x.shape for x in got] != [x.shape for x in first]
    assert all(same(x, y) for x, y in zip(got, raw(res, b)))
    assert all(not np.all(x.view(np.uint8) == 0x5A) for x in got if x.size)                       # every array was written


@pytest.mark.parametrize("family", FAMILIES)
def test_a_refused_call_leaves_the_serial_alone(res, occupancies, family):
    call, readers, _ = FAMILIES[family]
    a = call(res, occupancies[SMALL])
    first = read_all(a, readers)
    with pytest.raises(_ffi.RmError) as e:
        call(res, np.zeros((2, 2, 1025), np.uint8))                                              # nx = 1025: a lattice out of range
    assert e.value.status == _ffi.RM_ERR_RANGE
    assert all(same(x, y) for x, y in zip(read_all(a, readers), first))


def test_the_mask_has_a_serial_of_its_own(res, occupancies):
    d = res.distance_occupancy(occupancies[LARGE])
    f1 = d.features(r2_wall=1)
    f2 = d.features(r2_wall=4)
    with pytest.raises(ValueError) as e:
        f1.mask()
    assert "DistanceFeatures" in str(e.value) and "rm_distance_features" in str(e.value), str(e.value)
    raw = np.full(LARGE, 0x5A, np.uint8)
    res._check(res._L.rm_read_distance(res._h, None, raw.ctypes.data, 0, None))
    assert same(f2.mask(), raw) and set(np.unique(raw)) <= {0, 1, 2}
    assert same(d.d2(), raw_distance(res, d)[0])                                                 # the volume's serial has not moved
    res.distance_occupancy(occupancies[SMALL])
    for stale in (f1, f2):
        with pytest.raises(ValueError):
            stale.mask()
    with pytest.raises(ValueError):
        d.features(r2_wall=1)


def test_both_destinations_of_the_eager_readers_with_outputs_left_out(res):
    import torch

    def words(x):
        return None if x is None else (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).tobytes()

    origin, step = (-2.0, -2.0, -2.0), (0.5, 0.5, 0.6)
    for normals, ids in ((True, False), (False, True)):
        host = res.extract_mesh_grid(origin, step, (9, 8, 7), normals=normals, ids=ids)
        dev = res.extract_mesh_grid(origin, step, (9, 8, 7), normals=normals, ids=ids, device=True)
        torch.cuda.synchronize()
        assert len(host.triangles) > 0 and dev.vertices.device.type == "cuda" and dev.triangles.dtype == torch.int32
        assert (host.normals is None) == (not normals) and (host.leaf is None) == (not ids)
        for name in ("vertices", "triangles", "normals", "leaf", "material"):
            assert words(getattr(dev, name)) == words(getattr(host, name)), name
        args = (1, (-2.0, -2.0), (0.25, 0.25), (17, 17), [-0.5, 0.0, 0.5])
        host = res.slice_contours_grid(*args, normals=normals, ids=ids)
        dev = res.slice_contours_grid(*args, normals=normals, ids=ids, device=True)
        torch.cuda.synchronize()
        assert len(host.points) > 0 and len(host.layer_first) == 4 and dev.contours.dtype == torch.int32
        for name in ("points", "contours", "layer_first", "normals", "leaf", "material"):
            assert words(getattr(dev, name)) == words(getattr(host, name)), name


# ---- the refusals of the six rm_read_*: status and message, word for word --------------------------------------------------------
# (the call with `p` for the output that carries the alignment, nothing has been produced, a device destination off its alignment)
READS = {
    "rm_read_mesh": (lambda L, h, p, d: L.rm_read_mesh(h, p, None, None, None, d, None),
                     "rm_read_mesh: no mesh has been extracted",
                     "rm_read_mesh: device arrays need 4-byte alignment (out_ids: 8-byte)"),
    "rm_read_slices": (lambda L, h, p, d: L.rm_read_slices(h, p, None, None, None, None, d, None),
                       "rm_read_slices: nothing has been sliced",
                       "rm_read_slices: device arrays need 4-byte alignment (out_contours: 16-byte, out_ids: 8-byte)"),
    "rm_read_topology": (lambda L, h, p, d: L.rm_read_topology(h, None, None, p, d, None),
                         "rm_read_topology: nothing has been labelled",
                         "rm_read_topology: device arrays need 8-byte alignment (out_labels: 4-byte)"),
    "rm_read_distance": (lambda L, h, p, d: L.rm_read_distance(h, p, None, d, None),
                         "rm_read_distance: no distance volume has been computed",
                         "rm_read_distance: a device out_d2 needs 4-byte alignment"),
    "rm_read_support": (lambda L, h, p, d: L.rm_read_support(h, None, p, d, None),
                        "rm_read_support: no support call has been made",
                        "rm_read_support: a device out_profile needs 4-byte alignment"),
    "rm_read_islands": (lambda L, h, p, d: L.rm_read_islands(h, None, 0, p, None, None, d, None),
                        "rm_read_islands: no islands call has been made",
                        "rm_read_islands: device out_rows, out_labels and out_profile need 4-byte alignment"),
}


def last_error(r):
    return (r._L.rm_last_error(r._h) or b"").decode()


def test_reads_before_any_result_are_refused():
    fresh = renderer.RayMarchingResources(0)
    try:
        host = np.full(64, 0x5A5A5A5A, np.uint32)
        for name, (read, nothing, _) in READS.items():
            assert read(fresh._L, fresh._h, host.ctypes.data, 0) == _ffi.RM_ERR_ARG, name
            assert last_error(fresh) == nothing
        assert np.all(host == 0x5A5A5A5A)
    finally:
        fresh.close()


def test_misaligned_device_destinations_are_refused(res, occupancies):
    import torch
    res.extract_mesh_grid((-2.0, -2.0, -2.0), (0.5, 0.5, 0.6), (9, 8, 7))
    res.slice_contours_grid(1, (-2.0, -2.0), (0.25, 0.25), (17, 17), [0.0])
    for call, _, _ in FAMILIES.values():
        call(res, occupancies[SMALL])
    dev = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda:0")  # room for any output of these results
    for name, (read, _, misaligned) in READS.items():
        assert read(res._L, res._h, C.c_void_p(dev.data_ptr() + 1), 1) == _ffi.RM_ERR_ARG, name
        assert last_error(res) == misaligned
    torch.cuda.synchronize()
    assert bool((dev == 0x5A).all())
