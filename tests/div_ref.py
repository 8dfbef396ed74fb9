"""The short division of csrc/rm_interp.h (rcp_rn_fast, div_rn_fast, DivGuard) restated for the tests: an exact model on
Python integers (binary32 values as bit patterns, every operation rounded once, to nearest even), the guard on bit patterns
both scalar and in numpy, and the seeded pair generator of rm_selftest_div.  DESIGN.md section 2, "Short division"."""
from math import isqrt

import numpy as np

# DivGuard's constants (bit patterns)
K_B_LO, K_B_SPAN = 0x27800000, 0x2E000000   # 2^-48; bits(2^44) - bits(2^-48)
K_S_LO = 0x0F800000                         # 2^-96
K_MANT = 0x7FFFFC                           # the top four significands
K_A_LO, K_A_HI = 0x18000000, 0x66800000     # 2^-79, 2^78
M32 = 0xFFFFFFFF


# ---- exact binary32 arithmetic on integers (finite operands) ---------------------------------
def decode(bits):
    """bits -> (sign, m, e): the value is (-1)^sign m 2^e.  Finite values only."""
    s, E, f = bits >> 31, (bits >> 23) & 0xFF, bits & 0x7FFFFF
    assert E != 0xFF
    return (s, f, -149) if E == 0 else (s, f | 0x800000, E - 150)


def is_finite(bits):
    return (bits >> 23) & 0xFF != 0xFF


def round_ratio(sign, n, d, e):
    """RN((-1)^sign n / d 2^e) as a bit pattern; n >= 0, d > 0 integers.  Ties to even, gradual underflow, overflow to inf."""
    if n == 0:
        return sign << 31
    k = n.bit_length() - d.bit_length() + e        # 2^(k-1) < value < 2^(k+1)
    if (n << max(0, -(k - e))) < (d << max(0, k - e)):   # value < 2^k
        k -= 1
    t = max(k - 23, -149)                           # exponent of the result's last place
    sh = e - t
    nn, dd = (n << sh, d) if sh >= 0 else (n, d << -sh)
    q, r = divmod(nn, dd)
    if 2 * r > dd or (2 * r == dd and (q & 1)):
        q += 1
    if q == 1 << 24:
        q, t = q >> 1, t + 1
    if q < 1 << 23:
        return (sign << 31) | q                     # denormal (or zero after rounding)
    E = t + 150
    if E >= 0xFF:
        return (sign << 31) | 0x7F800000
    return (sign << 31) | (E << 23) | (q - (1 << 23))


def fma(a, b, c):
    """RN(a * b + c) on bit patterns."""
    sa, ma, ea = decode(a)
    sb, mb, eb = decode(b)
    sc, mc, ec = decode(c)
    sp, mp, ep = sa ^ sb, ma * mb, ea + eb
    if mp == 0 and mc == 0:
        return (sp << 31) if sp == sc else 0
    e = min(ep, ec)
    v = (-1) ** sp * (mp << (ep - e)) + (-1) ** sc * (mc << (ec - e))
    if v == 0:
        return 0                                    # exact cancellation: +0 in round-to-nearest
    return round_ratio(1 if v < 0 else 0, abs(v), 1, e)


def mul(a, b):
    sa, ma, ea = decode(a)
    sb, mb, eb = decode(b)
    return round_ratio(sa ^ sb, ma * mb, 1, ea + eb)


def add(a, b):
    return fma(a, 0x3F800000, b)


def div(a, b):
    """RN(a / b), b != 0."""
    sa, ma, ea = decode(a)
    sb, mb, eb = decode(b)
    return round_ratio(sa ^ sb, ma, mb, ea - eb)


def sqrt(a):
    """RN(sqrt(a)), a > 0."""
    _, m, e = decode(a)
    if e & 1:
        m, e = m << 1, e - 1
    m, e = m << 60, e - 60                          # 30 more bits of root than the result keeps
    r = isqrt(m)
    if r * r != m:
        r = 2 * r + 1                               # sticky bit: the root is irrational here, never a tie
        e -= 2
    return round_ratio(0, r, 1, e // 2)


def neg(a):
    return a ^ 0x80000000


ONE = 0x3F800000


def rcp_candidates(b):
    """What v_rcp_f32 may return for b (1 ulp accuracy): RN(1/b) and those of its two neighbours within one ulp of 1/b."""
    r = div(ONE, b)
    _, mb, eb = decode(b)
    out = []
    for c in (r - 1, r, r + 1):                     # neighbouring bit patterns of a positive normal value
        _, mc, ec = decode(c)
        # |c - 1/b| <= ulp(1/b)  <=>  |c b - 1| <= ulp b, with ulp taken in the binade of r (the larger, at a binade edge)
        _, _, er = decode(r)
        e = min(ec + eb, 0, er + eb)
        lhs = abs((mc * mb << (ec + eb - e)) - (1 << -e))
        if lhs <= mb << (er + eb - e):
            out.append(c)
    return out


def rcp_refined(b, r0):
    return fma(fma(neg(b), r0, ONE), r0, r0)


def div_short(a, b, r):
    q = mul(a, r)
    q1 = fma(fma(neg(q), b, a), r, q)
    return (q1 & 0x7FFFFFFF) | (q & 0x80000000)


# ---- the guard ----------------------------------------------------------------------------------
def guard_bad(a_list, b, s=None):
    """DivGuard::bad() after denominator(b) (or root_of(s, b) when the radicand s is given) and numerator(a) for each a."""
    d_hi = ((s - K_S_LO) & M32) >> 1 if s is not None else (b - K_B_LO) & M32
    bad = d_hi > K_B_SPAN or (b & 0x7FFFFF) >= K_MANT
    for a in a_list:
        ua = a & 0x7FFFFFFF
        bad = bad or ((ua - 1) & M32) < K_A_LO - 1 or ua >= K_A_HI
    return bad


def guard_bad_np(a, b, s=None):
    """The same on numpy arrays of float32 (a: (..., k) numerators sharing b: (...))."""
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    if s is None:
        d_hi = b - np.uint32(K_B_LO)
    else:
        d_hi = (np.ascontiguousarray(s, np.float32).view(np.uint32) - np.uint32(K_S_LO)) >> np.uint32(1)
    bad = (d_hi > np.uint32(K_B_SPAN)) | ((b & np.uint32(0x7FFFFF)) >= np.uint32(K_MANT))
    ua = a & np.uint32(0x7FFFFFFF)
    bad_a = ((ua - np.uint32(1)) < np.uint32(K_A_LO - 1)) | (ua >= np.uint32(K_A_HI))
    return bad | (bad_a if bad_a.ndim == bad.ndim else bad_a.any(axis=-1))


# ---- rm_selftest_div's seeded pairs ----------------------------------------------------------------
def _mix(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return x


def seeded_pairs(seed, n):
    """selftest_div_pair(seed, j), j < n, as two float32 arrays."""
    j = np.arange(n, dtype=np.uint32)
    g = np.uint32(0x9E3779B9)
    with np.errstate(over="ignore"):
        h1 = _mix(np.uint32(seed) ^ (np.uint32(3) * j) * g)
        h2 = _mix(np.uint32(seed) ^ (np.uint32(3) * j + np.uint32(1)) * g)
        h3 = _mix(np.uint32(seed) ^ (np.uint32(3) * j + np.uint32(2)) * g)
    mode = j & np.uint32(3)
    eb = np.uint32(107) + (h3 & np.uint32(0xFF)) % np.uint32(41)
    span = np.where(mode == 1, 4, np.where(mode == 2, 40, 110)).astype(np.uint32)
    drop = ((h3 >> np.uint32(8)) & np.uint32(0xFF)) % span
    ea = np.where(eb > drop, eb - drop, 0).astype(np.uint32)
    b = (eb << np.uint32(23)) | (h2 & np.uint32(0x7FFFFF))
    a = (h1 & np.uint32(0x80000000)) | (ea << np.uint32(23)) | (h1 & np.uint32(0x7FFFFF))
    a = np.where(((h3 >> np.uint32(16)) & np.uint32(31)) == 0, a & np.uint32(0x80000000), a)
    b = np.where(((h3 >> np.uint32(21)) & np.uint32(63)) == 0, b | np.uint32(0x7FFFFC), b)
    raw = mode == 0
    a = np.where(raw, h1, a).astype(np.uint32)
    b = np.where(raw, h2 & np.uint32(0x7FFFFFFF), b).astype(np.uint32)
    return a.view(np.float32), b.view(np.float32)
