// rm_lattice_walk.h -- the traversal of the lattice draw (rm_lattice.h): a ray through the bit words of a
// lattice, cell by cell or over empty bricks, to the record of its hit cell.  Included by rm_lattice.h for the kernels, and by
// tests/cpp/lattice_layout_check.cpp for a host program that runs the same functions on the CPU under ASan + UBSan -- the
// jumping traversal against the plain one, and both against the numpy restatement: the two functions below are the only lines
// that differ between the two.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
namespace rmk {
RM_DEV float lat_fmax(float a, float b) { return fmax_(a, b); }
RM_DEV float lat_fmin(float a, float b) { return fmin_(a, b); }
}  // namespace rmk
#else
// The host: no HIP.  v_max_f32 and v_min_f32 written out: -0 < +0 (no operand is NaN here).
#define RM_DEV inline
namespace rmk {
inline float lat_fmax(float a, float b) { return a > b || (a == b && __builtin_signbit(b)) ? a : b; }
inline float lat_fmin(float a, float b) { return a < b || (a == b && __builtin_signbit(a)) ? a : b; }
}  // namespace rmk
#endif

namespace rmk {

RM_DEV int lat_imax(int a, int b) { return a > b ? a : b; }
RM_DEV int lat_imin(int a, int b) { return a < b ? a : b; }

// The retained lattice and the window of a call, as the kernels see them.
struct LatGrid {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz;
    uint32_t row_words;  // u32 words of a row of nx bits
    uint32_t bx, by;     // bricks along x and y
    uint32_t lox, loy, loz, hix, hiy, hiz;
    const uint8_t* cls;
    const uint32_t* bits;
    const uint32_t* bricks;
    const float* materials;  // four floats an entry (r, g, b, unused)
    uint32_t n_materials;
};


// ---- traversal -----------------------------------------------------------------------------------------------------------------
// One axis of a ray in index space: e = (O - o) / s, r = 1 / (D / s); the window [lo, hi) and the cell i.
struct LatAxis {
    float e, r;
    int i, lo, hi;
    bool par, up;  // parallel: never steps; up: r > 0
};
RM_DEV float lat_t(const LatAxis& A, int m) { return (((float)m - 0.5f) - A.e) * A.r; }

// false: the ray misses the lattice for this axis alone (a non-finite e or g; a parallel axis outside the window)
RM_DEV bool lat_axis(LatAxis& A, float O, float D, float o, float s, uint32_t lo, uint32_t hi) {
    const float g = D / s;
    A.e = (O - o) / s;
    A.r = 1.0f / g;
    A.lo = (int)lo; A.hi = (int)hi;
    A.i = (int)lo;
    A.up = A.r > 0.0f;
    A.par = g == 0.0f || __builtin_isinf(A.r);
    if (!__builtin_isfinite(A.e) || !__builtin_isfinite(g)) return false;
    if (A.par) {
        if (!(A.e >= (float)A.lo - 0.5f && A.e < (float)A.hi - 0.5f)) return false;
        int m = (int)__builtin_floorf(A.e + 0.5f);  // off by one at most: e + 0.5f is rounded
        if ((float)m - 0.5f > A.e) m--;
        else if (A.e >= (float)m + 0.5f) m++;
        A.i = m;
    }
    return true;
}
// The planes ahead of the first one, k = 1..: lo + k (up) or hi - k; how many of the first `most` have t <= T.
RM_DEV int lat_first_count(const LatAxis& A, float T) {
    int L = 0, R = A.hi - A.lo - 1;
    while (L < R) {
        const int mid = (L + R + 1) >> 1;
        if (lat_t(A, A.up ? A.lo + mid : A.hi - mid) <= T) L = mid;
        else R = mid - 1;
    }
    return L;
}
// The planes ahead of cell i, k = 1..most: i + k (up) or i + 1 - k; how many have t <= T (or_equal) or t < T.
RM_DEV int lat_ahead_count(const LatAxis& A, int most, float T, bool or_equal) {
    int L = 0, R = most;
#pragma unroll
    for (int it = 0; it < 3; it++) {  // most <= 7
        if (L < R) {
            const int mid = (L + R + 1) >> 1;
            const float t = lat_t(A, A.up ? A.i + mid : A.i + 1 - mid);
            if (or_equal ? t <= T : t < T) L = mid;
            else R = mid - 1;
        }
    }
    return L;
}

struct LatRecord {
    bool hit;
    float t;
    uint32_t axis;  // 0..2, 3: none (the origin is inside)
    uint32_t index;
    bool up;  // of the record's axis
};

// (t, a) < (best, best_a) with x < y < z on ties; best_a == 3: nothing yet
#define RM_LAT_OFFER(A, a_, t_)                      \
    if (!A.par) {                                    \
        const float tt = (t_);                       \
        if (best_a == 3u || tt < best) { best = tt; best_a = a_; } \
    }

template <bool SKIP>
RM_DEV LatRecord lat_traverse(const LatGrid& G, float Ox, float Oy, float Oz, float Dx, float Dy, float Dz) {
    LatRecord rec;
    rec.hit = false; rec.t = 0.0f; rec.axis = 3u; rec.index = 0u; rec.up = false;
    LatAxis X, Y, Z;
    bool ok = lat_axis(X, Ox, Dx, G.ox, G.sx, G.lox, G.hix);
    ok = lat_axis(Y, Oy, Dy, G.oy, G.sy, G.loy, G.hiy) && ok;
    ok = lat_axis(Z, Oz, Dz, G.oz, G.sz, G.loz, G.hiz) && ok;
    if (!ok) return rec;
    // entry
    const float inf = __builtin_inff();
    float T0 = 0.0f, T1 = inf;
    float tinx = 0.0f, tiny = 0.0f, tinz = 0.0f;
    if (!X.par) { tinx = lat_t(X, X.up ? X.lo : X.hi); T0 = lat_fmax(T0, tinx); T1 = lat_fmin(T1, lat_t(X, X.up ? X.hi : X.lo)); }
    if (!Y.par) { tiny = lat_t(Y, Y.up ? Y.lo : Y.hi); T0 = lat_fmax(T0, tiny); T1 = lat_fmin(T1, lat_t(Y, Y.up ? Y.hi : Y.lo)); }
    if (!Z.par) { tinz = lat_t(Z, Z.up ? Z.lo : Z.hi); T0 = lat_fmax(T0, tinz); T1 = lat_fmin(T1, lat_t(Z, Z.up ? Z.hi : Z.lo)); }
    if (!(T0 < T1)) return rec;
    if (!X.par) { const int c = lat_first_count(X, T0); X.i = X.up ? X.lo + c : X.hi - 1 - c; }
    if (!Y.par) { const int c = lat_first_count(Y, T0); Y.i = Y.up ? Y.lo + c : Y.hi - 1 - c; }
    if (!Z.par) { const int c = lat_first_count(Z, T0); Z.i = Z.up ? Z.lo + c : Z.hi - 1 - c; }
    float t = T0;
    uint32_t axis = 3u;
    if (!X.par && tinx == T0) axis = 0u;
    if (!Y.par && tiny == T0) axis = 1u;
    if (!Z.par && tinz == T0) axis = 2u;
    // walk: every iteration moves at least one cell on, so at most nx + ny + nz of them
    for (;;) {
        const uint32_t ix = (uint32_t)X.i, iy = (uint32_t)Y.i, iz = (uint32_t)Z.i;
        bool single = true;
        if constexpr (SKIP) {
            const uint32_t b = ((iz >> 3) * G.by + (iy >> 3)) * G.bx + (ix >> 3);
            single = ((G.bricks[b >> 5] >> (b & 31u)) & 1u) != 0u;
        }
        float best = 0.0f;
        uint32_t best_a = 3u;
        if (single) {
            const uint32_t word = G.bits[(size_t)(iz * G.ny + iy) * G.row_words + (ix >> 5)];
            if ((word >> (ix & 31u)) & 1u) {
                rec.hit = true;
                break;
            }
            RM_LAT_OFFER(X, 0u, lat_t(X, X.up ? X.i + 1 : X.i))
            RM_LAT_OFFER(Y, 1u, lat_t(Y, Y.up ? Y.i + 1 : Y.i))
            RM_LAT_OFFER(Z, 2u, lat_t(Z, Z.up ? Z.i + 1 : Z.i))
            if (best_a == 3u) return rec;  // no axis steps: the walk is its first cell
            if (best_a == 0u) { if ((X.up ? X.i + 1 : X.i) == (X.up ? X.hi : X.lo)) return rec; X.i += X.up ? 1 : -1; }
            else if (best_a == 1u) { if ((Y.up ? Y.i + 1 : Y.i) == (Y.up ? Y.hi : Y.lo)) return rec; Y.i += Y.up ? 1 : -1; }
            else { if ((Z.up ? Z.i + 1 : Z.i) == (Z.up ? Z.hi : Z.lo)) return rec; Z.i += Z.up ? 1 : -1; }
        } else {
            // the empty brick's part of the window, [l, h) per axis, and its leaving planes
            const int xl = lat_imax(X.lo, X.i & ~7), xh = lat_imin(X.hi, (X.i & ~7) + 8);
            const int yl = lat_imax(Y.lo, Y.i & ~7), yh = lat_imin(Y.hi, (Y.i & ~7) + 8);
            const int zl = lat_imax(Z.lo, Z.i & ~7), zh = lat_imin(Z.hi, (Z.i & ~7) + 8);
            RM_LAT_OFFER(X, 0u, lat_t(X, X.up ? xh : xl))
            RM_LAT_OFFER(Y, 1u, lat_t(Y, Y.up ? yh : yl))
            RM_LAT_OFFER(Z, 2u, lat_t(Z, Z.up ? zh : zl))
            if (best_a == 3u) return rec;
            // the other axes: their planes inside the brick that come before the leaving event -- t < T, or t == T on a lower axis
            if (!X.par && best_a != 0u) { const int c = lat_ahead_count(X, X.up ? xh - 1 - X.i : X.i - xl, best, true); X.i += X.up ? c : -c; }
            if (!Y.par && best_a != 1u) { const int c = lat_ahead_count(Y, Y.up ? yh - 1 - Y.i : Y.i - yl, best, best_a > 1u); Y.i += Y.up ? c : -c; }
            if (!Z.par && best_a != 2u) { const int c = lat_ahead_count(Z, Z.up ? zh - 1 - Z.i : Z.i - zl, best, false); Z.i += Z.up ? c : -c; }
            if (best_a == 0u) { if ((X.up ? xh : xl) == (X.up ? X.hi : X.lo)) return rec; X.i = X.up ? xh : xl - 1; }
            else if (best_a == 1u) { if ((Y.up ? yh : yl) == (Y.up ? Y.hi : Y.lo)) return rec; Y.i = Y.up ? yh : yl - 1; }
            else { if ((Z.up ? zh : zl) == (Z.up ? Z.hi : Z.lo)) return rec; Z.i = Z.up ? zh : zl - 1; }
        }
        t = best;
        axis = best_a;
    }
    rec.t = t;
    rec.axis = axis;
    rec.up = axis == 0u ? X.up : axis == 1u ? Y.up : Z.up;
    rec.index = (uint32_t)X.i + G.nx * ((uint32_t)Y.i + G.ny * (uint32_t)Z.i);
    return rec;
}
#undef RM_LAT_OFFER

}  // namespace rmk
