"""The short division ("Short division") in exact integer arithmetic, no GPU: for every input the
guard accepts, and for every value v_rcp_f32 may return (RN(1/b) and those of its two neighbours within one ulp of 1/b), the
refined reciprocal is RN(1/b) and the short quotient is RN(a/b), sign of zero included; and the guard accepts what a
normalisation ordinarily sees, so the generic path stays the exception."""
import numpy as np
import pytest

import div_ref as D

F = np.float32


def bits(x):
    return int(np.array([x], F).view(np.uint32)[0])


def check_pair(a, b, s=None, must_accept=False):
    """-> True when the guard accepted.  Asserts the accepted result for every reciprocal candidate."""
    if D.guard_bad([a], b, s):
        assert not must_accept, "guard rejects a = 0x%08x  b = 0x%08x" % (a, b)
        return False
    want_r, want_q = D.div(D.ONE, b), D.div(a, b)
    cands = D.rcp_candidates(b)
    assert want_r in cands and len(cands) >= 2
    for r0 in cands:
        r = D.rcp_refined(b, r0)
        assert r == want_r, "reciprocal of 0x%08x from r0 = 0x%08x: 0x%08x, want 0x%08x" % (b, r0, r, want_r)
        q = D.div_short(a, b, r)
        assert q == want_q, "0x%08x / 0x%08x from r0 = 0x%08x: 0x%08x, want 0x%08x" % (a, b, r0, q, want_q)
    return True


def test_random_pairs_are_accepted_and_exact():
    rng = np.random.default_rng(1201)
    n = 6000
    eb = rng.integers(127 - 20, 127 + 21, n)
    ea = eb - rng.integers(0, 24, n)                       # |a| up to 2^-23 of b's binade, and a few a > b
    ea[::7] = eb[::7] + rng.integers(0, 3, n)[::7]
    fa, fb = rng.integers(0, 1 << 23, n), rng.integers(0, (1 << 23) - 4, n)
    sa = rng.integers(0, 2, n)
    for k in range(n):
        check_pair(int(sa[k]) << 31 | int(ea[k]) << 23 | int(fa[k]), int(eb[k]) << 23 | int(fb[k]), must_accept=True)


def test_components_over_their_own_length_are_accepted_and_exact():
    """What gen_ray_at (four squares) and shade_hit (three) do: s in the contract's order, b = RN(sqrt(s)), the guard on s."""
    rng = np.random.default_rng(1202)
    for k in range(2000):
        dims = 3 + (k & 1)
        v = (rng.normal(size=dims) * 2.0 ** int(rng.integers(-20, 21))).astype(F)
        vb = [bits(x) for x in v]
        sq = [D.mul(x, x) for x in vb]
        s = D.add(D.add(sq[0], sq[1]), sq[2])
        if dims == 4:
            s = D.add(s, sq[3])
        b = D.sqrt(s)
        if (b & 0x7FFFFF) >= D.K_MANT:
            continue                                       # (a 1 in 2^21 chance per vector; none with this seed)
        for a in vb[:3]:
            check_pair(a, b, s, must_accept=True)


def test_powers_of_two_and_top_significands():
    rng = np.random.default_rng(1203)
    for E in (79, 80, 100, 126, 127, 128, 150, 170):
        for k in range(40):
            a = int(rng.integers(0, 2)) << 31 | (E - int(rng.integers(0, 20))) << 23 | int(rng.integers(0, 1 << 23))
            assert check_pair(a, E << 23)                  # b a power of two
            assert check_pair(a, E << 23 | 0x7FFFFB)       # the last significand below the rejected four
            for top in range(4):                            # all ones minus 0..3: always the generic form
                assert not check_pair(a, E << 23 | (0x7FFFFF - top))


def test_markstein_exception_is_real():
    """Why the guard looks at the significand at all: with all ones some admissible r0 refines to the wrong reciprocal."""
    b = 127 << 23 | 0x7FFFFF
    want = D.div(D.ONE, b)
    assert any(D.rcp_refined(b, r0) != want for r0 in D.rcp_candidates(b))


def test_zero_numerators_keep_their_sign():
    rng = np.random.default_rng(1204)
    for k in range(200):
        b = int(rng.integers(79, 171)) << 23 | int(rng.integers(0, (1 << 23) - 4))
        for a in (0x00000000, 0x80000000):
            assert check_pair(a, b)
            r = D.rcp_refined(b, D.div(D.ONE, b))
            assert D.div_short(a, b, r) == a
    # without the sign transfer -0 / b would come out +0
    b = bits(3.0)
    r = D.div(D.ONE, b)
    q = D.mul(0x80000000, r)
    assert q == 0x80000000 and D.fma(D.fma(D.neg(q), b, 0x80000000), r, q) == 0


def test_bounds_of_the_guard():
    rng = np.random.default_rng(1205)
    top_b = D.K_B_LO + D.K_B_SPAN                         # 2^44
    for k in range(300):
        fb = int(rng.integers(0, (1 << 23) - 4))
        sign = int(rng.integers(0, 2)) << 31
        for b in (D.K_B_LO | fb, (top_b - (1 << 23)) | fb, top_b, 127 << 23 | fb):
            # numerators just above / below 2^-79 and 2^78: the quotient and the remainder stay normal just inside
            assert check_pair(sign | D.K_A_LO, b) and check_pair(sign | (D.K_A_LO + 1 + fb), b)
            assert not check_pair(sign | (D.K_A_LO - 1), b) and not check_pair(sign | (D.K_A_LO - 1 - fb), b)
            assert check_pair(sign | (D.K_A_HI - 1), b) and not check_pair(sign | D.K_A_HI, b)
            assert not check_pair(sign | 1, b) and not check_pair(sign | 0x007FFFFF, b)      # denormal numerators
        a = sign | 100 << 23 | fb
        # denominators just outside [2^-48, 2^44], zero, denormal
        for b in (D.K_B_LO - 1, top_b + 1, 0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x80000000 | 127 << 23):
            assert not check_pair(a, b)
    # the radicand form: s in [2^-96, 2^88] accepted, its neighbours outside rejected; b itself is then not looked at
    b1 = bits(1.0)
    assert not D.guard_bad([b1], b1, D.K_S_LO) and D.guard_bad([b1], b1, D.K_S_LO - 1)
    assert not D.guard_bad([b1], b1, 0x6B800000) and D.guard_bad([b1], b1, 0x6B800002)
    assert D.guard_bad([b1], b1, 0) and D.guard_bad([b1], b1, 0x7F800000) and D.guard_bad([b1], b1, 0x7FC00000)
    assert D.sqrt(0x6B800001) == top_b and D.sqrt(D.K_S_LO) == D.K_B_LO


@pytest.mark.parametrize("special", [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001])
def test_nan_and_infinity_are_rejected(special):
    one = bits(1.0)
    assert D.guard_bad([special], one) and D.guard_bad([one], special)
    assert D.guard_bad([one, special, one], one) and D.guard_bad([one], one, special)


def test_numpy_guard_is_the_scalar_guard():
    a, b = D.seeded_pairs(7, 4096)
    got = D.guard_bad_np(a, b)
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    want = np.array([D.guard_bad([int(x)], int(y)) for x, y in zip(ua, ub)])
    assert (got == want).all() and 0.2 < want.mean() < 0.8
    ok = np.nonzero(~want)[0][:1500]
    for k in ok:                                           # and the seeded pairs of rm_selftest_div are exact where accepted
        check_pair(int(ua[k]), int(ub[k]), must_accept=True)
