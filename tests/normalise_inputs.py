"""Inputs and the numpy reference for rm_selftest_normalise (include/rm_abi.h): the families of DESIGN.md section 5, "Direct
tests".  TEST INFRASTRUCTURE shared by tests/test_normalise_inputs_cpu.py (the integer model of div_ref on a subsample) and
tests/test_gpu_normalise_direct.py (the device on all of it).  Nothing here looks at the device.

A Case is a block of whole waves (64 consecutive records each) of one mode with one expectation:
  "in"     every record inside the guard, except those whose root has one of the top four significands
  "out"    every record outside the guard
  "lanes"  every wave has exactly the lanes `lanes` outside, the other lanes inside
  "any"    no claim (the reference decides per record)
Mode 2 carries two expectations, for the normal and for the light vector.

The reference is plain binary32 numpy: the radicand in the contract's order, np.sqrt, one division per component."""
import functools
from collections import namedtuple

import numpy as np

import div_ref as D
from gbuffer_ref import _normalize3
from oracle import rm_oracle_np as onp

F = np.float32
U = np.uint32
LIGHT = (F(2.0), F(-5.0), F(3.0))
Case = namedtuple("Case", "name mode recs expect lanes")


def p2(e):
    return F(np.ldexp(1.0, e))


def up(x, k=1):
    """k binary32 steps away from x, towards +inf (k > 0) or -inf (k < 0); x positive."""
    return (np.asarray(x, F).view(U) + U(k & 0xFFFFFFFF)).view(F) if k else np.asarray(x, F)


def recs(x, y, z, w=0.0, px=0.0, py=0.0, pz=0.0):
    x, y, z, w, px, py, pz = np.broadcast_arrays(*[np.asarray(v, F) for v in (x, y, z, w, px, py, pz)])
    r = np.zeros((x.size, 8), F)
    for k, v in enumerate((x, y, z, w, px, py, pz)):
        r[:, k] = v.ravel()
    return r


def whole_waves(r):
    """r cycled up to a multiple of 64 records."""
    n = -(-len(r) // 64) * 64
    return np.ascontiguousarray(r[np.arange(n) % len(r)])


def case(name, mode, r, expect, lanes=()):
    return Case(name, mode, whole_waves(np.asarray(r, F)), expect, tuple(lanes))


def spread(v):
    """(k, 3) vectors -> the same vectors under the six axis permutations and a sign pattern per record: 64 records per wave
    keep their radicand (one addition rounds when at most two components are non-zero; callers check s where it matters)."""
    perms = [(0, 1, 2), (1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0), (2, 0, 1)]
    v = whole_waves(np.asarray(v, F).reshape(-1, 3))
    out = np.empty_like(v)
    for i in range(len(v)):
        sg = [F(-1.0) if (i >> b) & 1 else F(1.0) for b in (0, 1, 2)]
        out[i] = [v[i, perms[i % 6][k]] * sg[k] for k in range(3)]
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def radicand(r, mode):
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    s = (x * x + y * y) + z * z
    return s + r[:, 3] * r[:, 3] if mode == 1 else s


def reference(mode, r):
    """-> (result (n, 3) float32 -- mode 2: column 0 alone --, verdict (n,) uint32) as rm_selftest_normalise defines them."""
    r = np.asarray(r, F)
    out = np.zeros((len(r), 3), F)
    with np.errstate(all="ignore"):
        x, y, z = r[:, 0], r[:, 1], r[:, 2]
        s = radicand(r, mode)
        ln = np.sqrt(s)
        bad = D.guard_bad_np(r[:, :3], ln, s).astype(U)
        if mode != 2:
            out[:, 0], out[:, 1], out[:, 2] = x / ln, y / ln, z / ln
            return out, bad
        nx, ny, nz = _normalize3(x, y, z)
        lx, ly, lz = r[:, 4] - LIGHT[0], r[:, 5] - LIGHT[1], r[:, 6] - LIGHT[2]
        sl = (lx * lx + ly * ly) + lz * lz
        bad |= D.guard_bad_np(np.stack([lx, ly, lz], axis=-1), np.sqrt(sl), sl).astype(U) << U(1)
        lx, ly, lz = _normalize3(lx, ly, lz)
        out[:, 0] = onp.fmax(F(0.02), (nx * lx + ny * ly) + nz * lz)
        return out, bad


def quotients_in_binary64(mode, r):
    """The cross-check of the quotients: float32(float64(x) / float64(len)), len the binary32 root.  Double rounding is harmless
    for a quotient of two binary32 values (it is never within 2^-29 ulp of a midpoint without being exact)."""
    with np.errstate(all="ignore"):
        ln = np.sqrt(radicand(r, mode)).astype(np.float64)
        return (r[:, :3].astype(np.float64) / ln[:, None]).astype(F)


def top_four(r, mode):
    with np.errstate(all="ignore"):
        return (np.sqrt(radicand(r, mode)).view(U) & U(0x7FFFFF)) >= U(D.K_MANT)


def light_vectors(r):
    """pos - light of mode 2 records, as records of mode 0."""
    with np.errstate(all="ignore"):
        return recs(r[:, 4] - LIGHT[0], r[:, 5] - LIGHT[1], r[:, 6] - LIGHT[2])


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))


# ---- building blocks ----------------------------------------------------------------------------------------------------------------
def directions(rng, n, kmin=-47, kmax=43):
    """n random directions of length 2^k (1 + u), k uniform in [kmin, kmax], u in [0, 1).  (Unit vectors times 2^k would not do:
    the binary32 length of one is within an ulp or two of a power of two, and every other one has a top significand.)"""
    v = rng.normal(size=(n, 3))
    v *= ((1.0 + rng.random(n) * 0.999) / np.sqrt((v * v).sum(axis=1)))[:, None]
    return (v * np.ldexp(1.0, rng.integers(kmin, kmax + 1, n))[:, None]).astype(F)


def with_radicand(target, n=64):
    """Up to n vectors (x, y, 0) whose radicand, formed in binary32, is exactly `target`: a search over the neighbours of
    sqrt(target) and small second components."""
    t = float(target)
    x0 = F(np.sqrt(t))
    xs = up(x0, 0).view(U).astype(np.int64)[None] + np.arange(-6, 7)[:, None]
    xs = xs.astype(U).view(F).ravel()
    ys = np.concatenate([[0.0], (np.sqrt(t) * np.ldexp(1.0, -np.arange(9, 14))[:, None] * (1.0 + np.arange(32) / 32.0)[None, :]).ravel()]).astype(F)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    with np.errstate(all="ignore"):
        hit = (X * X + Y * Y) == F(target)
    v = np.stack([X[hit], Y[hit], np.zeros(int(hit.sum()), F)], axis=-1)
    assert len(v) > 0, "no vector with radicand %r" % target
    return v[:n]


def with_root_significand(rng, e, frac, n=64):
    """n general vectors whose binary32 root is 2^e (1 + frac 2^-23): random directions scaled onto the target length in
    binary64 and kept when the binary32 arithmetic lands on it."""
    want = (U((e + 127) << 23) | U(frac)).view(F)
    keep = np.zeros((0, 3), F)
    while len(keep) < n:
        v = rng.normal(size=(4096, 3))
        v = (v * (float(want) / np.sqrt((v * v).sum(axis=1)))[:, None]).astype(F)
        ok = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) == want
        keep = np.concatenate([keep, v[ok]])
    return keep[:n]


# ---- the families (mode 0 and 1) -----------------------------------------------------------------------------------------------------
def in_range():
    return [case("in_range", 0, recs(*directions(np.random.default_rng(5101), 1 << 20).T), "in")]


def radicand_bounds():
    out = []
    lo, hi = p2(-96), p2(88)
    for name, s in (("s=2^-96", lo), ("s=2^-96+1ulp", up(lo, 1)), ("s=2^-96-1ulp", up(lo, -1)),
                    ("s=2^88", hi), ("s=2^88+1ulp", up(hi, 1)), ("s=2^88+2ulp", up(hi, 2)), ("s=2^88-1ulp", up(hi, -1)),
                    ("s denormal, 2^-130", p2(-130)), ("s denormal, 3 2^-149", up(F(0), 3))):
        out.append(case(name, 0, recs(*spread(with_radicand(s)).T), "any"))
    # every exponent of s inside the range, odd and even (root_of's >> 1), and the two binades just outside
    rng = np.random.default_rng(5102)
    v = directions(rng, 1 << 18, -49, 44)
    ex = np.frexp(radicand(recs(*v.T), 0))[1] - 1
    for e in range(-97, 89):
        pick = np.nonzero(ex == e)[0][:64]
        assert len(pick) == 64
        out.append(case("exponent of s %d" % e, 0, recs(*v[pick].T), "in" if -96 <= e <= 87 else "out"))
    z = np.zeros(64, F)
    out.append(case("s = 0", 0, recs(z, z, z) * np.where(np.arange(64) & 1, F(-1), F(1))[:, None], "out"))
    out.append(case("s = +inf (2^64)", 0, recs(*spread(recs(p2(64), p2(64) * F(1.25), p2(10))[:, :3]).T), "out"))
    out.append(case("s underflows to 0 (2^-75)", 0, recs(*spread(np.array([[p2(-75), 0, 0], [p2(-75), p2(-76), p2(-78)]], F)).T), "out"))
    return out


def numerator_bounds():
    rng = np.random.default_rng(5103)
    out = []
    big = (rng.random((64, 2)) + 0.25).astype(F)
    big *= np.where(rng.random((64, 2)) < 0.5, F(-1), F(1))
    for name, a, expect in (("numerator 2^-79", p2(-79), "in"), ("numerator 2^-79-1ulp", up(p2(-79), -1), "out"),
                            ("numerator denormal", p2(-140), "out"), ("numerator smallest denormal", up(F(0), 1), "out"),
                            ("numerator +0", F(0.0), "in"), ("numerator -0", F(-0.0), "in")):
        for pos in range(3):
            v = np.insert(big, pos, a, axis=1)
            if a != 0:
                v[1::2, pos] = -v[1::2, pos]
            out.append(case("%s at %s" % (name, "xyz"[pos]), 0, recs(*v.T), expect))
    # corners of the proof: b at the lower bound's side with a mid significand, b just below 2^44; |a| at 2^-79 and at b
    b_lo, tiny = F(1.5) * p2(-48), p2(-79)
    k = np.arange(5, 69)
    b_hi, b_top = up(np.full(64, p2(44)), 0).view(U) - k.astype(U), (p2(44).view(U) - U(1) - np.arange(4, dtype=U))
    b_hi, b_top = b_hi.view(F), b_top.view(F)
    sg = np.where(np.arange(64) & 1, F(-1), F(1))
    out += [case("b=1.5 2^-48, a=b", 0, recs(*spread(np.array([[b_lo, 0, 0]], F)).T), "in"),
            case("b=1.5 2^-48, a=2^-79", 0, recs(*spread(np.array([[b_lo, tiny, -tiny], [b_lo, tiny, 0]], F)).T), "in"),
            case("b=2^44-k ulp, a=b", 0, recs(b_hi * sg, 0, 0), "in"),
            case("b=2^44-k ulp, a=2^-79", 0, recs(b_hi, tiny * sg, -tiny), "in"),
            case("b=2^44-k ulp, k<=4, a=2^-79", 0, recs(b_top, tiny, -tiny), "out"),
            case("b=2^44, a=b", 0, recs(*spread(np.array([[p2(44), 0, 0]], F)).T), "in"),
            case("b=2^44, a=2^-79", 0, recs(*spread(np.array([[p2(44), tiny, -tiny]], F)).T), "in"),
            case("b=2^44+1ulp", 0, recs(*spread(np.array([[up(p2(44), 1), 0, 0], [up(p2(44), 1), tiny, -tiny]], F)).T), "out"),
            case("b=2^-48", 0, recs(*spread(np.array([[p2(-48), 0, 0]], F)).T), "in"),
            case("b=2^-48-1ulp", 0, recs(*spread(np.array([[up(p2(-48), -1), 0, 0]], F)).T), "out")]
    return out


TOP_BINADES = (-47, -30, -10, -1, 0, 7, 25, 43)


def top_significands():
    rng = np.random.default_rng(5104)
    out = []
    for frac in range(0x7FFFFB, 0x800000):
        for e in TOP_BINADES:
            b = (U((e + 127) << 23) | U(frac)).view(F)
            expect = "in" if frac < D.K_MANT else "out"
            out.append(case("root 2^%d sig %06X, axis" % (e, frac), 0, recs(*spread(np.array([[b, 0, 0]], F)).T), expect))
            out.append(case("root 2^%d sig %06X, general" % (e, frac), 0, recs(*with_root_significand(rng, e, frac).T), expect))
    return out


@functools.lru_cache(maxsize=None)
def rounding_boundaries(n_pool=1 << 24, keep=4096):
    """-> (Case, distances in ulp of the kept quotients from the nearest midpoint of two floats, ascending).  Random vectors
    with normal components; x / len ranked in binary64 (53 bits: the distance is resolved to 2^-29 ulp)."""
    rng = np.random.default_rng(5105)
    best_v, best_d = np.zeros((0, 3), F), np.zeros(0)
    for _ in range(n_pool >> 20):
        v = rng.normal(size=(1 << 20, 3)).astype(F)
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float64)
        m, _e = np.frexp(np.abs(v[:, 0].astype(np.float64)) / ln)
        t = m * 16777216.0
        d = np.abs((t - np.floor(t)) - 0.5)
        best_v, best_d = np.concatenate([best_v, v]), np.concatenate([best_d, d])
        order = np.argsort(best_d, kind="stable")[:keep]
        best_v, best_d = best_v[order], best_d[order]
    return case("rounding_boundaries", 0, recs(*best_v.T), "in"), best_d


BAD_LANES = (("low s", (p2(-50), 0, 0)), ("high s", (p2(45), 0, 0)), ("top significand", (up(F(2), -1), 0, 0)),
             ("small numerator", (1.0, p2(-90), 0.5)), ("NaN", (np.nan, 1.0, 1.0)), ("inf", (np.inf, 1.0, 1.0)))


def wave_fallback():
    rng = np.random.default_rng(5106)
    out = []
    for name, bad in BAD_LANES:
        for lane in (0, 31, 32, 63):
            v = directions(rng, 64)
            v[lane] = bad
            out.append(case("one lane %d: %s" % (lane, name), 0, recs(*v.T), "lanes", (lane,)))
    return out


def ray_form():
    rng = np.random.default_rng(5107)
    v, g = directions(rng, 4096), directions(rng, 4096, -46, 40)      # g: room for a fourth term of up to six times |g|
    out = [case("ray ew=0", 1, recs(*v.T, 0.0), "in"),
           case("ray ew=-0", 1, recs(*v[:256].T, -0.0), "in"),
           case("ray general", 1, recs(*g.T, (rng.normal(size=4096) * np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))).astype(F)), "in")]
    w = (np.ldexp(1.0 + rng.random(1024), 40) * np.where(rng.random(1024) < 0.5, -1, 1)).astype(F)
    out.append(case("ray ew dominating", 1, recs(*directions(rng, 1024, -60, -60).T, w), "in"))
    t = p2(-79)
    w = (np.ldexp(1.5 + 0.5 * rng.random(64), 43)).astype(F)
    w[0] = F(2.0 ** 43.9)
    sg = [np.where((np.arange(64) >> b) & 1, F(-1), F(1)) for b in range(3)]
    out.append(case("ray four-term corner", 1, recs(t * sg[0], t * sg[1], t * sg[2], w), "in"))
    out.append(case("ray four-term corner, 2^-79-1ulp", 1, recs(up(t, -1) * sg[0], t * sg[1], t * sg[2], w), "out"))
    for name, e in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        out.append(case("ray ew %s" % name, 1, recs(*v[:64].T, e), "out"))
    return out


def mode0_cases(full=True):
    """full=False: the big in-range family cut to 64 waves and the boundaries to 16 (what mode 2 crosses with positions)."""
    a, b = in_range()[0], rounding_boundaries()[0]
    if not full:
        a, b = a._replace(recs=a.recs[:64 * 64]), b._replace(recs=b.recs[:16 * 64])
    return [a] + radicand_bounds() + numerator_bounds() + top_significands() + [b] + wave_fallback()


# ---- shade_hit (mode 2) ---------------------------------------------------------------------------------------------------------------
def positions(kind, rng, n):
    """n hit positions of one class -> ((n, 3) float32, the expectation for the light vector pos - (2, -5, 3))."""
    light = np.array(LIGHT, F)
    if kind == "ordinary":
        return (rng.random((n, 3)) * 10.0 - 5.0).astype(F), "in"
    if kind == "near light":                               # each component 1..8 steps from the light's, either side
        steps = rng.integers(1, 9, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1, 1)
        return (np.abs(light).view(U).astype(np.int64) + steps).astype(U).view(F).reshape(n, 3) * np.sign(light), "in"
    if kind == "at light":
        return np.broadcast_to(light, (n, 3)).copy(), "out"
    if kind in ("2^43", "2^45", "2^70"):
        return directions(rng, n, int(kind[2:]), int(kind[2:])), {"2^43": "in", "2^45": "out", "2^70": "out"}[kind]
    assert kind == "NaN"
    p = (rng.random((n, 3)) * 10.0 - 5.0).astype(F)
    p[np.arange(n), rng.integers(0, 3, n)] = np.nan
    return p, "out"


POSITION_KINDS = ("ordinary", "near light", "at light", "2^43", "2^45", "2^70", "NaN")


def shade_cases():
    rng = np.random.default_rng(5108)
    out = []
    for c in mode0_cases(full=False):
        for kind in POSITION_KINDS:
            pos, expect_l = positions(kind, rng, len(c.recs))
            r = c.recs.copy()
            r[:, 4:7] = pos
            out.append(Case("shade %s | pos %s" % (c.name, kind), 2, r, (c.expect, expect_l), c.lanes))
    return out


def all_cases():
    return mode0_cases() + ray_form() + shade_cases()


# ---- populations ---------------------------------------------------------------------------------------------------------------------
def check_population(c, verdict):
    """Asserts that the verdicts (the reference's, bit 0 the normal / only vector, bit 1 the light) are the ones the case is
    there for; -> per wave (normal wholly in, normal wholly out, light wholly in, light wholly out)."""
    verdict = np.asarray(verdict, U)
    expects = c.expect if c.mode == 2 else (c.expect,)
    waves = []
    for bit, expect in enumerate(expects):
        bad = ((verdict >> U(bit)) & U(1)).astype(bool)
        if expect == "in":
            top = top_four(c.recs if bit == 0 else light_vectors(c.recs), c.mode if c.mode != 2 else 0)
            assert not (bad & ~top).any(), "%s: %d records outside the guard for another reason than a top significand" % (c.name, int((bad & ~top).sum()))
        elif expect == "out":
            assert bad.all(), "%s: %d records inside the guard" % (c.name, int((~bad).sum()))
        elif expect == "lanes":
            want = np.isin(np.arange(len(bad)) % 64, c.lanes)
            assert (bad == want).all(), "%s: the lanes outside the guard are not %r" % (c.name, c.lanes)
        w = bad.reshape(-1, 64)
        waves += [~w.any(axis=1), w.all(axis=1)]
    return waves
