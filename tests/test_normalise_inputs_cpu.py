"""The inputs of tests/test_gpu_normalise_direct.py without a GPU ("Direct tests"): every family's
accept / reject populations are the ones it is there for, and on a subsample of every family the integer model of
tests/div_ref.py -- the radicand in the contract's order, the exact root, the guard on the radicand, the short reciprocal and
quotients for EVERY value v_rcp_f32 may return -- gives RN(x / len) wherever the guard accepts.  It also ties the numpy
reference of that test to the integer model: radicand, root and quotients agree bit for bit on every finite sampled record."""
import numpy as np
import pytest

import div_ref as D
import normalise_inputs as N

F, U = np.float32, np.uint32
PER_CASE = {"in_range": 1500, "rounding_boundaries": 600}     # records of the subsample; every other case: 6


def subsample(c, rng):
    k = PER_CASE.get(c.name, 6)
    idx = np.unique(np.concatenate([[0, len(c.recs) - 1], rng.integers(0, len(c.recs), k - 2)]))
    if c.expect == "lanes":
        idx = np.unique(np.concatenate([idx, np.array(c.lanes)]))
    return idx


def model_vector(comps, extra=()):
    """comps: bit patterns of (x, y, z); extra: further squares of the radicand.  -> (s, b, accepted) with every quotient of an
    accepted vector checked against div for every reciprocal candidate; None when an operand or the radicand is not finite."""
    if not all(D.is_finite(v) for v in tuple(comps) + tuple(extra)):
        return None
    s = None
    for v in tuple(comps) + tuple(extra):
        sq = D.mul(v, v)
        if not D.is_finite(sq) or (s is not None and not D.is_finite(s)):
            return None
        s = sq if s is None else D.add(s, sq)
    if not D.is_finite(s):
        return None
    if s == 0:
        assert D.guard_bad(list(comps), 0, s)
        return s, None, False
    b = D.sqrt(s)
    if D.guard_bad(list(comps), b, s):
        return s, b, False
    want_r = D.div(D.ONE, b)
    cands = D.rcp_candidates(b)
    assert want_r in cands and len(cands) >= 2
    for r0 in cands:
        r = D.rcp_refined(b, r0)
        assert r == want_r, "reciprocal of 0x%08x from r0 = 0x%08x: 0x%08x, want 0x%08x" % (b, r0, r, want_r)
        for a in comps:
            q = D.div_short(a, b, r)
            assert q == D.div(a, b), "0x%08x / 0x%08x from r0 = 0x%08x: 0x%08x, want 0x%08x" % (a, b, r0, q, D.div(a, b))
    return s, b, True


def check_case(c, rng):
    ref, verdict = N.reference(c.mode, c.recs)
    N.check_population(c, verdict)
    if c.mode != 2:                                           # the reference's quotients, once more in binary64
        assert N.same_bits(ref, N.quotients_in_binary64(c.mode, c.recs)).all(), c.name
    n_model = 0
    for i in subsample(c, rng):
        r = c.recs[i]
        ub = [int(x) for x in r.view(U)]
        vectors = [(ub[:3], ub[3:4] if c.mode == 1 else [])]
        if c.mode == 2:
            with np.errstate(all="ignore"):
                l = np.array([r[4] - N.LIGHT[0], r[5] - N.LIGHT[1], r[6] - N.LIGHT[2]], F)
            if all(D.is_finite(int(p)) for p in r[4:7].view(U)):          # pos - light in the model: one rounded addition each
                want = [D.add(int(p), D.neg(int(q))) for p, q in zip(r[4:7].view(U), np.array(N.LIGHT, F).view(U))]
                assert [int(x) for x in l.view(U)] == want
            vectors.append(([int(x) for x in l.view(U)], []))
        for bit, (comps, extra) in enumerate(vectors):
            m = model_vector(comps, extra)
            bad = bool((verdict[i] >> bit) & 1)
            if m is None:
                assert bad, "%s record %d: a non-finite vector inside the guard" % (c.name, i)
                continue
            s, b, accepted = m
            assert accepted == (not bad), "%s record %d: the scalar guard and guard_bad_np disagree" % (c.name, i)
            # the numpy reference against the model: radicand, root, quotients
            v = np.array(comps, U).view(F)
            with np.errstate(all="ignore"):
                rec = np.zeros((1, 8), F)
                rec[0, :3] = v
                if extra:
                    rec[0, 3] = np.array(extra, U).view(F)[0]
                s_np = N.radicand(rec, 1 if extra else 0)
                assert int(s_np.view(U)[0]) == s, "%s record %d: radicand" % (c.name, i)
                if b is not None:
                    ln = np.sqrt(s_np)
                    assert int(ln.view(U)[0]) == b, "%s record %d: root" % (c.name, i)
                    assert [int(x) for x in (v / ln).view(U)] == [D.div(a, b) for a in comps], "%s record %d: quotients" % (c.name, i)
            n_model += 1
    return n_model


FAMILIES = {"in_range": N.in_range, "radicand_bounds": N.radicand_bounds, "numerator_bounds": N.numerator_bounds,
            "top_significands": N.top_significands, "rounding_boundaries": lambda: [N.rounding_boundaries()[0]],
            "wave_fallback": N.wave_fallback, "ray_form": N.ray_form}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_populations_and_model(family):
    rng = np.random.default_rng(61)
    cases = FAMILIES[family]()
    n_rec = sum(len(c.recs) for c in cases)
    n_model = sum(check_case(c, rng) for c in cases)
    print("%s: %d cases, %d records, %d vectors through the integer model" % (family, len(cases), n_rec, n_model))
    assert n_model >= 3 * len(cases)


def test_in_range_keeps_the_waves_on_the_short_form():
    c = N.in_range()[0]
    _, verdict = N.reference(0, c.recs)
    whole_in = N.check_population(c, verdict)[0]
    print("in_range: %d records outside the guard (top significands), %d of %d waves wholly inside" % (int(verdict.sum()), int(whole_in.sum()), len(whole_in)))
    assert len(c.recs) == 1 << 20 and whole_in.mean() >= 0.999


def test_named_bounds_are_on_the_side_the_guard_puts_them():
    """The cases whose expectation is left to the reference ("any"), pinned here: which side of the radicand's bounds."""
    want = {"s=2^-96": 0, "s=2^-96+1ulp": 0, "s=2^-96-1ulp": 1, "s=2^88": 0, "s=2^88+1ulp": 0, "s=2^88+2ulp": 1, "s=2^88-1ulp": 1,
            "s denormal, 2^-130": 1, "s denormal, 3 2^-149": 1}
    seen = {}
    for c in N.radicand_bounds():
        if c.name in want:
            s = N.radicand(c.recs, 0)
            assert len(np.unique(s.view(U))) == 1                                  # the wave really has that one radicand
            _, verdict = N.reference(0, c.recs)
            assert (verdict == want[c.name]).all(), c.name
            seen[c.name] = int(s.view(U)[0])
    assert set(seen) == set(want)
    assert seen["s=2^-96"] == D.K_S_LO and seen["s=2^-96-1ulp"] == D.K_S_LO - 1 and seen["s=2^88+2ulp"] == 0x6B800002
    # (2^88 + 1 ulp is inside: its root rounds to 2^44, and root_of's shift drops the last bit of the radicand;  2^88 - 1 ulp is
    # outside although its radicand is in range: its root is 2^44 - 1 ulp, the all-ones significand)


def test_top_significands_reach_every_binade():
    seen = set()
    for c in N.top_significands():
        b = np.sqrt(N.radicand(c.recs, 0)).view(U)
        assert len(np.unique(b)) == 1
        seen.add((int(b[0] >> 23) - 127, int(b[0] & 0x7FFFFF), "axis" in c.name))
    assert seen == {(e, f, a) for e in N.TOP_BINADES for f in range(0x7FFFFB, 0x800000) for a in (True, False)}


def test_rounding_boundaries_are_close():
    c, d = N.rounding_boundaries()
    print("rounding boundaries: %d quotients, midpoint distance %.3g .. %.3g ulp" % (len(d), d[0], d[-1]))
    assert len(c.recs) == 4096 and d[-1] < 2.0 ** -11 and d[0] < 1e-6
    # the ranking is the quotient's own: recompute two of them exactly
    for i in (0, 1):
        x, s = int(c.recs[i, 0:1].view(U)[0]), None
        for v in c.recs[i, :3].view(U):
            sq = D.mul(int(v), int(v))
            s = sq if s is None else D.add(s, sq)
        b = D.sqrt(s)
        _, mx, ex = D.decode(x)
        _, mb, eb = D.decode(b)
        q = D.div(x, b)
        _, mq, eq = D.decode(q)
        # |x / b - (q +- half an ulp)| in ulp of q, for the nearer midpoint, in exact integers scaled by mb
        sh = ex - eb - eq + 1
        num = (mx << (sh + 40)) if sh + 40 >= 0 else mx >> -(sh + 40)
        dist = min(abs(num - ((2 * mq + t) * mb << 40)) for t in (-1, 1)) / float(2 * mb << 40)
        assert abs(dist - d[i]) <= 2.0 ** -28, (dist, d[i])


def test_shade_populations():
    """Mode 2: each of the four combinations (normal in / out) x (light in / out) has at least 64 whole waves."""
    combos = np.zeros((2, 2), np.int64)
    rng = np.random.default_rng(62)
    n_model = 0
    for c in N.shade_cases():
        _, verdict = N.reference(2, c.recs)
        n_in, n_out, l_in, l_out = N.check_population(c, verdict)
        for a, n_w in enumerate((n_in, n_out)):
            for b, l_w in enumerate((l_in, l_out)):
                combos[a, b] += int((n_w & l_w).sum())
        if rng.random() < 0.05:
            n_model += check_case(c, rng)
    print("shade_hit: whole waves (normal in, out) x (light in, out) = %s; %d vectors through the integer model" % (combos.tolist(), n_model))
    assert (combos >= 64).all() and n_model >= 300
