"""The front end the eight lattice analyses share (rm_label_*, rm_distance_*, rm_support_*, rm_islands_*, each as _solid and as
_occupancy): with two faults in one call the earlier check answers, and a call that fails leaves the previous
result of its family readable, word for word.  Results, shapes and single faults are the family tests' business."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_topology import scene_program, use
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

NX, NY, NZ = 9, 17, 10
N = NX * NY * NZ
UP, NH = _ffi.RM_UP_POS_Z, NZ                      # the layers of the directed families run along z
AUTO = _ffi.RM_SUPPORT_PLATE_AUTO
UNDERFLOW = np.array([1, 100], np.uint32)          # one command: a Union on an empty stack


class Family:
    def __init__(self, name, n_counts, n_stats, directed):
        self.name, self.n_counts, self.n_stats, self.directed = name, n_counts, n_stats, directed


FAMILIES = {f.name: f for f in (Family("label", _ffi.RM_TOPO_COUNTS, _ffi.RM_TOPO_STATS, False),
                                Family("distance", _ffi.RM_DIST_COUNTS, _ffi.RM_DIST_STATS, False),
                                Family("support", _ffi.RM_SUP_COUNTS, _ffi.RM_SUP_STATS, True),
                                Family("islands", _ffi.RM_ISL_COUNTS, _ffi.RM_ISL_STATS, True))}
ENTRIES = [(name, kind) for name in FAMILIES for kind in ("solid", "occupancy")]
ids = lambda e: "rm_%s_%s" % e  # noqa: E731


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    use(r, *scene_program("g8"))
    yield r
    r.close()


@pytest.fixture(scope="module")
def occupancy():
    return np.ascontiguousarray(np.random.default_rng(23).random((NZ, NY, NX)) < 0.4).view(np.uint8)


def call(res, entry, occ, *, n=(NX, NY, NZ), step=(0.5, 0.25, 0.4), level=0.0, up=UP, r2=1, plate=AUTO, counts=True, stats=True,
         short_counts=0, short_stats=0):
    """One call of an entry point with everything right but what is named: its status, the message, the counts."""
    fam, kind = FAMILIES[entry[0]], entry[1]
    fn = getattr(res._L, "rm_%s_%s" % entry)
    out_counts, out_stats = (C.c_uint64 * fam.n_counts)(), (C.c_uint64 * fam.n_stats)()
    direction = (up, r2, plate) if fam.directed else ()
    outputs = (out_counts if counts else None, fam.n_counts - short_counts, out_stats if stats else None, fam.n_stats - short_stats)
    if kind == "solid":
        rc = fn(res._h, (C.c_float * 3)(-2.0, -2.0, -2.0), (C.c_float * 3)(*step), n[0], n[1], n[2], level, *direction, *outputs)
    else:
        rc = fn(res._h, n[0], n[1], n[2], occ.ctypes.data, 0, None, *direction, *outputs)
    return rc, (res._L.rm_last_error(res._h) or b"").decode(), [int(x) for x in out_counts]


# (the two faults, the entries they apply to, the status of the earlier check, what its message names)
SOLID, DIRECTED = (lambda e: e[1] == "solid"), (lambda e: FAMILIES[e[0]].directed)
PAIRS = [
    ("NULL out_stats, short n_counts", dict(stats=False, short_counts=1), lambda e: True, _ffi.RM_ERR_NULL, "is NULL"),
    ("short n_stats, non-finite step", dict(short_stats=1, step=(0.5, np.inf, 0.4)), SOLID, _ffi.RM_ERR_ARG, "n_stats"),
    ("non-finite level, nx = 1", dict(level=np.nan, n=(1, NY, NZ)), SOLID, _ffi.RM_ERR_ARG, "level"),
    ("up = 6, nx = 1025", dict(up=6, n=(1025, NY, NZ)), DIRECTED, _ffi.RM_ERR_ARG, "up 6"),
    ("r2 = 256, plate out of range", dict(r2=256, plate=NH), DIRECTED, _ffi.RM_ERR_RANGE, "r2 256"),
    ("bad lattice, empty program", dict(n=(NX, 1, NZ), underflow=True), SOLID, _ffi.RM_ERR_RANGE, "lattice"),
]


@pytest.mark.parametrize("entry", ENTRIES, ids=ids)
def test_the_earlier_of_two_faults_answers(res, occupancy, entry):
    for what, faults, applies, status, names in PAIRS:
        if not applies(entry):
            continue
        faults = dict(faults)
        try:
            if faults.pop("underflow", False):
                res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, UNDERFLOW.tobytes())
                assert call(res, entry, occupancy)[0] == _ffi.RM_ERR_STACK_UNDERFLOW, what   # (the later fault is one)
            rc, message, _ = call(res, entry, occupancy, **faults)
        finally:
            use(res, *scene_program("g8"))
        print("%s: %s -> %d %r" % (ids(entry), what, rc, message))
        assert rc == status, what
        assert message.startswith(ids(entry) + ":") and names in message, (what, message)


def read(res, family, counts):
    """The words rm_read_* gives for the family's last result (counts: those of the call that made it)."""
    L, h = res._L, res._h
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    if family == "label":
        out = [np.full((counts[_ffi.RM_TOPO_BODIES], 16), 0x5A, np.uint64), np.full((counts[_ffi.RM_TOPO_CAVITIES], 16), 0x5A, np.uint64),
               np.full(N, 0x5A, np.uint32)]
        rc = L.rm_read_topology(h, p(out[0]), p(out[1]), p(out[2]), 0, None)
    elif family == "distance":
        out = [np.full(N, 0x5A, np.uint32)]
        rc = L.rm_read_distance(h, p(out[0]), None, 0, None)
    elif family == "support":
        out = [np.full(N, 0x5A, np.uint8), np.full(NH * 4, 0x5A, np.uint32)]
        rc = L.rm_read_support(h, p(out[0]), p(out[1]), 0, None)
    else:
        R = counts[_ffi.RM_ISL_REGIONS]
        out = [np.full((R, _ffi.RM_ISL_ROW_WORDS), 0x5A, np.uint32), np.full(N, 0x5A, np.uint32), np.full(N, 0x5A, np.uint8),
               np.full(NH * 4, 0x5A, np.uint32)]
        rc = L.rm_read_islands(h, p(out[0]), R, p(out[1]), p(out[2]), p(out[3]), 0, None)
    assert rc == _ffi.RM_OK, (family, rc)
    return out


@pytest.mark.parametrize("entry", ENTRIES, ids=ids)
def test_a_failed_call_leaves_the_previous_result_readable(res, occupancy, entry):
    family = entry[0]
    rc, message, counts = call(res, (family, "occupancy"), occupancy)
    assert rc == _ffi.RM_OK, message
    first = read(res, family, counts)
    assert all(not np.all(a == 0x5A) for a in first if a.size)                                    # every array was written
    failures = [("a lattice out of range", dict(n=(1025, NY, NZ)), _ffi.RM_ERR_RANGE)]
    if entry[1] == "solid":
        failures.append(("an invalid program", dict(), _ffi.RM_ERR_STACK_UNDERFLOW))
    for what, faults, status in failures:
        try:
            if status == _ffi.RM_ERR_STACK_UNDERFLOW:
                res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, UNDERFLOW.tobytes())
            assert call(res, entry, occupancy, **faults)[0] == status, what
        finally:
            use(res, *scene_program("g8"))
        again = read(res, family, counts)
        assert len(again) == len(first) and all(np.array_equal(a, b) for a, b in zip(again, first)), what
