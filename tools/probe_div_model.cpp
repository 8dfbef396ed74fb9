// probe_div_model.cpp -- host-side evidence for the short reciprocal and quotient of csrc/rm_interp.h (DESIGN.md
// section 2, "Short division").  Plain C++, no GPU:  c++ -O2 -march=native -o probe_div_model tools/probe_div_model.cpp
//
// Everything scales by powers of two while nothing under- or overflows (the guard's job), so significands suffice.
//
// 1. Reciprocal, exhaustive: for every significand B in [2^23, 2^24) and each binary32 value r0 within one ulp of
//    1/B (RN(1/B) and those of its two neighbours that are), is r = fma(fma(-B, r0, 1), r0, r0) the correctly rounded
//    1/B?  Prints every failing significand (expected: all ones alone, Markstein's exception).
// 2. Quotient, exhaustive over the hard cases: with r = RN(1/B), q = RN(A r), rem = RN(A - q B) and V = q + rem r
//    (before the last rounding), |V - A/B| < 2^-22 ulp(A/B) (DESIGN.md derives it).  So q' = RN(V) can differ from
//    RN(A/B) only if A/B lies that close to a rounding boundary, i.e. |A 2^26 - N B| <= 34 for an integer N.  For
//    every B these A are the solutions of 69 congruences; all of them are run through the sequence.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static uint64_t inv_mod(uint64_t a, uint64_t m) {  // a^-1 mod m, gcd(a, m) = 1
    int64_t t = 0, nt = 1, r = (int64_t)m, nr = (int64_t)(a % m);
    while (nr) {
        const int64_t q = r / nr, x = t - q * nt, y = r - q * nr;
        t = nt; nt = x; r = nr; nr = y;
    }
    return (uint64_t)(t < 0 ? t + (int64_t)m : t);
}

static bool quotient_ok(float a, float b) {
    const float r = 1.0f / b;
    const float q = a * r;
    const float q1 = fmaf(fmaf(-q, b, a), r, q);
    const float want = a / b;
    return memcmp(&q1, &want, 4) == 0;
}

int main() {
    // ---- 1 ----
    uint64_t bad_r = 0;
    uint32_t lowest_bad = 0xFFFFFFFFu;
    for (uint32_t B = 1u << 23; B < (1u << 24); B++) {
        const float b = (float)B, want = 1.0f / b;
        const float cand[3] = {nextafterf(want, 0.0f), want, nextafterf(want, 1.0f)};
        bool bad = false;
        for (float r0 : cand) {
            // within one ulp of the exact 1/B: ulp(1/B) = 2^-47 below 2^-23, and r0 B is exact in binary64
            if (std::fabs((double)r0 * (double)b - 1.0) > std::ldexp((double)b, -47)) continue;
            const float r = fmaf(fmaf(-b, r0, 1.0f), r0, r0);
            bad = bad || memcmp(&r, &want, 4) != 0;
        }
        if (bad) {
            bad_r++;
            if (B < lowest_bad) lowest_bad = B;
            printf("reciprocal not correctly rounded for significand 0x%06x (all ones minus %u)\n", B & 0x7FFFFFu, 0xFFFFFFu - B);
        }
    }
    printf("reciprocal: %llu failing significands, lowest 0x%06x\n", (unsigned long long)bad_r, lowest_bad & 0x7FFFFFu);

    // ---- 2 ----
    uint64_t tried = 0, bad_q = 0;
    for (uint64_t B = 1u << 23; B < (1u << 24); B++) {
        const uint64_t g = B & (~B + 1u);  // gcd(2^26, B)
        const uint64_t Bp = B / g;
        const uint64_t inv = Bp == 1u ? 0u : inv_mod(((uint64_t)1 << 26) / g % Bp, Bp);
        for (int64_t c = -34; c <= 34; c++) {
            if (c % (int64_t)g) continue;
            const int64_t cg = c / (int64_t)g;
            const uint64_t c_mod = (uint64_t)((cg % (int64_t)Bp + (int64_t)Bp) % (int64_t)Bp);
            uint64_t A = Bp == 1u ? 0u : (unsigned __int128)c_mod * inv % Bp;
            for (; A < (1u << 24); A += Bp) {
                if (A < (1u << 23)) continue;
                tried++;
                if (!quotient_ok((float)A, (float)B)) {
                    if (bad_q++ < 20) printf("quotient wrong: A = 0x%06llx  B = 0x%06llx\n", (unsigned long long)A, (unsigned long long)B);
                }
            }
        }
    }
    printf("quotient: %llu hard cases tried, %llu wrong\n", (unsigned long long)tried, (unsigned long long)bad_q);
    return bad_q != 0;
}
