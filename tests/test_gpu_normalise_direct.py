"""normalize3, the ray's four-term normalisation and shade_hit run directly on the device (rm_selftest_normalise: the functions
the march kernels call, not copies) on both sides of every bound of the DivGuard, against a numpy binary32 reference that shares
nothing with the device: the radicand in the contract's order, np.sqrt, x / len, each quotient cross-checked once in binary64;
shade_hit through the oracle's fmax.  For every record: the short form as the kernels run it (whole-wave fall-back included),
the generic form and the guard's verdict for the lane equal the reference, bit for bit.  The families and what each is there
for: tests/normalise_inputs.py; tests/test_normalise_inputs_cpu.py shows without a GPU that the families reach the edges they
name.  DESIGN.md section 5, "Direct tests"."""
import ctypes as C

import numpy as np
import pytest

import normalise_inputs as N
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    yield r
    r.close()


def run(res, mode, recs):
    """-> (short (n, 3), generic (n, 3), verdict (n,)) of rm_selftest_normalise."""
    recs = np.ascontiguousarray(recs, F)
    assert recs.shape[1] == 8 and len(recs) % 64 == 0
    out = np.full((len(recs), 8), 0xDEADBEEF, U)
    _ffi.check(res._h, _ffi.hip_lib().rm_selftest_normalise(res._h, recs.ctypes.data_as(C.c_void_p), len(recs), mode,
                                                             out.ctypes.data_as(C.c_void_p)))
    assert (out[:, 7] == 0).all()
    return out[:, 0:3].copy().view(F), out[:, 3:6].copy().view(F), out[:, 6].copy()


def check(res, cases):
    """All cases of one mode in one launch (every case is whole waves).  -> per case, the waves wholly inside the guard for
    every vector of the record, i.e. the waves on which the short form is what ran."""
    mode = cases[0].mode
    assert all(c.mode == mode for c in cases)
    recs = np.concatenate([c.recs for c in cases])
    short, generic, verdict = run(res, mode, recs)
    want, want_verdict = N.reference(mode, recs)
    if mode != 2:
        assert N.same_bits(want, N.quotients_in_binary64(mode, recs)).all()
    ok_v = verdict == want_verdict
    ok_s = N.same_bits(short, want).all(axis=1)
    ok_g = N.same_bits(generic, want).all(axis=1)
    if not (ok_v & ok_s & ok_g).all():
        i = int(np.nonzero(~(ok_v & ok_s & ok_g))[0][0])
        first = np.cumsum([len(c.recs) for c in cases])
        c = cases[int(np.searchsorted(first, i, side="right"))]
        raise AssertionError("mode %d, %d records differ (verdict %d, short form %d, generic form %d); first: record %d, lane %d of '%s': "
                             "input %s, verdict %d want %d, short %s generic %s want %s" % (
                                 mode, int((~(ok_v & ok_s & ok_g)).sum()), int((~ok_v).sum()), int((~ok_s).sum()), int((~ok_g).sum()),
                                 i, i % 64, c.name, ["%08x" % x for x in recs[i].view(U)], verdict[i], want_verdict[i],
                                 ["%08x" % x for x in short[i].view(U)], ["%08x" % x for x in generic[i].view(U)],
                                 ["%08x" % x for x in want[i].view(U)]))
    whole, at = [], 0
    for c in cases:
        v = want_verdict[at:at + len(c.recs)]
        N.check_population(c, v)
        whole.append(int((v.reshape(-1, 64) == 0).all(axis=1).sum()))
        at += len(c.recs)
    return whole


def test_in_range_runs_the_short_form(res):
    c = N.in_range()[0]
    whole = check(res, [c])[0]
    print("in_range: %d records, %d of %d waves wholly on the short form" % (len(c.recs), whole, len(c.recs) // 64))
    assert len(c.recs) == 1 << 20 and whole >= 0.999 * (len(c.recs) // 64)


@pytest.mark.parametrize("family", ["radicand_bounds", "numerator_bounds", "top_significands"])
def test_bounds_of_the_guard(res, family):
    cases = getattr(N, family)()
    whole = check(res, cases)
    n_in = sum(1 for c in cases if c.expect == "in")
    print("%s: %d cases, %d records; %d waves wholly on the short form" % (family, len(cases), sum(len(c.recs) for c in cases), sum(whole)))
    for c, w in zip(cases, whole):
        if c.expect == "in" and not N.top_four(c.recs, 0).any():
            assert w == len(c.recs) // 64, c.name                  # the short form is what computed these
        if c.expect == "out":
            assert w == 0
    assert n_in >= 10


def test_rounding_boundaries(res):
    c, d = N.rounding_boundaries()
    whole = check(res, [c])[0]
    print("rounding boundaries: %d quotients %.3g .. %.3g ulp from a midpoint, %d of %d waves wholly on the short form" % (
        len(d), d[0], d[-1], whole, len(c.recs) // 64))
    assert whole >= 60


def test_one_lane_sends_the_wave_to_the_generic_form(res):
    cases = N.wave_fallback()
    assert len(cases) == 24 and check(res, cases) == [0] * 24        # check_population: exactly that lane is outside


def test_ray_form(res):
    cases = N.ray_form()
    whole = dict(zip([c.name for c in cases], check(res, cases)))
    print("ray form: %s" % whole)
    for c in cases:
        assert whole[c.name] >= (len(c.recs) // 64 - 1 if c.expect == "in" else 0) and (c.expect == "in" or whole[c.name] == 0)


def test_shade_hit(res):
    cases = N.shade_cases()
    check(res, cases)
    combos = np.zeros((2, 2), np.int64)
    for c in cases:
        n_in, n_out, l_in, l_out = N.check_population(c, N.reference(2, c.recs)[1])
        for a, n_w in enumerate((n_in, n_out)):
            for b, l_w in enumerate((l_in, l_out)):
                combos[a, b] += int((n_w & l_w).sum())
    print("shade_hit: %d records; whole waves (normal in, out) x (light in, out) = %s" % (sum(len(c.recs) for c in cases), combos.tolist()))
    assert (combos >= 64).all()


def test_arguments_are_checked(res):
    L, r, o = _ffi.hip_lib(), np.zeros((64, 8), F), np.zeros((64, 8), U)
    p, q = r.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    assert L.rm_selftest_normalise(res._h, p, 63, 0, q) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_normalise(res._h, p, 0, 0, q) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_normalise(res._h, p, 64, 3, q) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_normalise(res._h, None, 64, 0, q) == _ffi.RM_ERR_NULL
    assert L.rm_selftest_normalise(None, p, 64, 0, q) == _ffi.RM_ERR_NULL
