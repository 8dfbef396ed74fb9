// rm_distance.h -- the exact squared Euclidean distance transform of the occupancy lattice {d < level} (rm_distance_solid,
// rm_distance_occupancy) and the thin walls and narrow gaps it gives (rm_distance_features).  Included by rm_abi.hip alone, after
// rm_topology.h, whose probe and occupancy kernels fill the occupancy.  DESIGN.md section 20 is the contract; every output is an
// integer defined by a minimum or a count, so no order of execution changes a word, and no atomic decides one.
//
// One u32 per point holds BOTH transforms: the inside's (distance to the nearest outside point, the surrounding layer included)
// and the outside's (distance to the nearest inside point).  At every point one of the two is 0 -- the point is a source of the
// other class's transform --, so the word holds the point's own class's running value and kDistInside tells which.  The passes,
// each a launch of its own (no workgroup reads what another one of the same launch wrote):
//   rows     one wave per row of x: the row's class bits by ballot into LDS (16 words at most), then per point the nearest
//            bit of the other class to the left and to the right, word by word (clz / ctz): D = min(dl, dr)^2.
//   columns  y, then z: f(p) = min_q g(q) + (p - q)^2 along the column, g(q) the word of a point of p's class and 0 for a point of
//            the other.  A workgroup stages a tile of 16..64 adjacent columns in LDS (rml::DistColumnLds: adjacent lanes hold
//            adjacent x in both passes), and every point searches a WINDOW around itself: q = p already gives g(p), and a row at
//            offset d cannot give less than gmin + d^2 (gmin the column's smallest g), so the search ends at the first d with
//            gmin + d^2 >= the best so far; an outside point starts at the first row that holds a value at all.  Exact for
//            every input; the cost per point is about the distance it finds, in points (section 20 has the worst case).  In
//            place: a workgroup reads and writes its own columns only, and reads them all before it writes.
//   maxima   per 2048 points one row of 16 words (rm_reduce.h): the inside points, and max of (D2 << 32 | ~index) per
//            class -- the largest D2 and the smallest index that attains it, whatever the order.
// The features run the same row and column kernels from a core mask {class c, D2 > r2}: one class, no layer, values capped at
// r2 + 1 (a window never reaches past sqrt(r2)); a compose kernel marks the points of class c farther than r2 from every core
// point and counts.
#pragma once
#include "rm_lds_layout.h"
#include "rm_reduce.h"

namespace rmk {

constexpr uint32_t kDistInside = 0x80000000u, kDistNone = 0x7FFFFFFFu;  // RM_DIST_INSIDE_BIT, RM_DIST_NONE (and the value's mask)
constexpr uint32_t kDistBlock = 2048u;                                  // points per row of the reductions
enum : int { DIST_FROM_OCCUPANCY = 0, DIST_FROM_WALL_CORE = 1, DIST_FROM_GAP_CORE = 2 };

// ---- rows -------------------------------------------------------------------------------------------------------------------
// SRC = DIST_FROM_OCCUPANCY: bit = inside (occ); both classes, the inside's sees the layer points at -1 and nx.
// Otherwise bit = a core point of the distance volume `vol` (class inside / outside with D2 > r2): a core point gets kDistInside | 0,
// every other point min(its squared distance to the nearest core point of the row, r2 + 1).
template <int SRC>
__global__ __launch_bounds__(256) void rm_dist_row_kernel(uint32_t nx, uint32_t n_rows, const uint8_t* __restrict__ occ,
                                                          const uint32_t* __restrict__ vol, uint32_t r2, uint32_t* __restrict__ out) {
    __shared__ unsigned long long s_bits[4][16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * 4u + wave;
    const bool live = row < n_rows;  // uniform over the wave
    const uint32_t base = row * nx;  // (< 2^28 when live)
    const uint32_t words = (nx + 63u) >> 6;
    for (uint32_t w = 0; w < words; w++) {
        const uint32_t x = w * 64u + lane;
        bool b = false;
        if (live && x < nx) {
            if (SRC == DIST_FROM_OCCUPANCY) {
                b = occ[base + x] != 0u;
            } else {
                const uint32_t v = vol[base + x];
                b = (v >> 31) == (SRC == DIST_FROM_WALL_CORE ? 1u : 0u) && (v & kDistNone) > r2;
            }
        }
        const unsigned long long m = __ballot(b);
        if (lane == 0u) s_bits[wave][w] = m;
    }
    __syncthreads();
    if (!live) return;
    const uint32_t tail = nx & 63u;
    for (uint32_t w = 0; w < words; w++) {
        const uint32_t x = w * 64u + lane;
        if (x >= nx) continue;
        const bool c = (s_bits[wave][w] >> lane) & 1ull;
        if (SRC != DIST_FROM_OCCUPANCY && c) {
            out[base + x] = kDistInside;
            continue;
        }
        // the points of the other class in word ww (its bits past the row's end cleared)
        const auto other = [&](uint32_t ww) -> unsigned long long {
            const unsigned long long bits = s_bits[wave][ww];
            const unsigned long long valid = (ww + 1u == words && tail != 0u) ? (1ull << tail) - 1ull : ~0ull;
            return (c ? ~bits : bits) & valid;
        };
        const bool layer = SRC == DIST_FROM_OCCUPANCY && c;
        uint32_t ww = w;
        unsigned long long o = other(ww) & ((1ull << lane) - 1ull);
        while (o == 0ull && ww > 0u) o = other(--ww);
        const uint32_t dl = o != 0ull ? x - (ww * 64u + 63u - (uint32_t)__builtin_clzll(o)) : layer ? x + 1u : 0xFFFFFFFFu;
        ww = w;
        o = lane == 63u ? 0ull : other(ww) & (~0ull << (lane + 1u));
        while (o == 0ull && ww + 1u < words) o = other(++ww);
        const uint32_t dr = o != 0ull ? ww * 64u + (uint32_t)__builtin_ctzll(o) - x : layer ? nx - x : 0xFFFFFFFFu;
        const uint32_t d = min(dl, dr);  // (<= 1024 or none)
        if (SRC == DIST_FROM_OCCUPANCY)
            out[base + x] = (c ? kDistInside : 0u) | (d == 0xFFFFFFFFu ? kDistNone : d * d);
        else
            out[base + x] = d == 0xFFFFFFFFu ? r2 + 1u : min(d * d, r2 + 1u);
    }
}

// ---- columns ----------------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): the columns x = bx * xt + [0, xt) of slab `by`; point q of column x is vol[by * outer + x + q * stride].
// The y pass: stride nx, outer nx * ny (by = k); the z pass: stride nx * ny, outer nx (by = j).
// SINGLE (the features): only the words without kDistInside are transformed, towards those with it, and `none` = r2 + 1 is
// their largest value; otherwise both classes, `none` = kDistNone, and the inside's transform sees g = 0 at q = -1 and q = n.
template <bool SINGLE>
__global__ __launch_bounds__(256) void rm_dist_column_kernel(uint32_t nx, uint32_t n, uint32_t stride, uint32_t outer, uint32_t xt_log2,
                                                             uint32_t none, uint32_t* vol) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // per column: for the outside's transform the smallest g, the first and the last row that hold a value below `none`; for the
    // inside's the smallest g.  (LDS atomics of min and max: the result is the same in every order.)
    __shared__ uint32_t s_meta[rml::kDistMaxColumns][4];
    const uint32_t xt = 1u << xt_log2;
    uint32_t* s_col = smem + rml::DistColumnLds(xt, n).col / 4u;
    const uint32_t lx = threadIdx.x & (xt - 1u), r0 = threadIdx.x >> xt_log2, rstep = 256u >> xt_log2;
    const uint32_t x = blockIdx.x * xt + lx;
    const bool live = x < nx;
    const uint32_t base = blockIdx.y * outer + x;  // (below 2^28 when live)
    if (threadIdx.x < xt) {
        s_meta[threadIdx.x][0] = 0xFFFFFFFFu;
        s_meta[threadIdx.x][1] = 0xFFFFFFFFu;
        s_meta[threadIdx.x][2] = 0u;
        s_meta[threadIdx.x][3] = 0xFFFFFFFFu;
    }
    __syncthreads();
    uint32_t gmin0 = 0xFFFFFFFFu, first = 0xFFFFFFFFu, last = 0u, gmin1 = 0xFFFFFFFFu;
    for (uint32_t q = r0; q < n; q += rstep) {
        const uint32_t v = live ? vol[base + q * stride] : none;
        s_col[q * xt + lx] = v;
        const uint32_t val = v & kDistNone;
        const uint32_t g0 = (v >> 31) ? 0u : val, g1 = (v >> 31) ? val : 0u;  // what the outside's and the inside's transform see
        if (g0 < none) {
            gmin0 = min(gmin0, g0);
            first = min(first, q);
            last = max(last, q);
        }
        gmin1 = min(gmin1, g1);
    }
    if (live && r0 < n) {
        if (first != 0xFFFFFFFFu) {
            atomicMin(&s_meta[lx][0], gmin0);
            atomicMin(&s_meta[lx][1], first);
            atomicMax(&s_meta[lx][2], last);
        }
        atomicMin(&s_meta[lx][3], gmin1);
    }
    __syncthreads();
    if (!live) return;
    const uint32_t m0 = s_meta[lx][0], lo = s_meta[lx][1], hi = s_meta[lx][2], m1 = s_meta[lx][3];
    for (uint32_t p = r0; p < n; p += rstep) {
        const uint32_t w = s_col[p * xt + lx];
        const uint32_t cls = w >> 31;
        if (SINGLE && cls != 0u) continue;  // a core point stays as it is
        uint32_t best = w & kDistNone;
        const uint32_t below = p, above = n - 1u - p;  // points of the column on either side
        uint32_t gmin, d, dmax;
        if (cls == 0u) {
            if (lo == 0xFFFFFFFFu) continue;  // no row of this column holds a value: this one stays `none`
            // rows nearer than the first one with a value cannot give less than `none`; rows past the last one neither
            gmin = m0;
            d = p < lo ? lo - p : p > hi ? p - hi : 1u;
            dmax = max(p > lo ? p - lo : 0u, hi > p ? hi - p : 0u);
        } else {
            // the layer's points at -1 and n (g = 0), then the column's rows
            best = min(best, min((below + 1u) * (below + 1u), (above + 1u) * (above + 1u)));
            gmin = m1;
            d = 1u;
            dmax = max(below, above);
        }
        // a row at offset d or more cannot give less than gmin + d^2
        for (; d <= dmax && gmin + d * d < best; d++) {
            const uint32_t dd = d * d;
            if (d <= below) {
                const uint32_t u = s_col[(p - d) * xt + lx];
                best = min(best, ((u >> 31) != cls ? 0u : u & kDistNone) + dd);  // (at most 2^31 + 2^20)
            }
            if (d <= above) {
                const uint32_t u = s_col[(p + d) * xt + lx];
                best = min(best, ((u >> 31) != cls ? 0u : u & kDistNone) + dd);
            }
        }
        vol[base + p * stride] = (cls << 31) | min(best, none);
    }
}

// ---- maxima and counts ------------------------------------------------------------------------------------------------------
// rows[16 b]: entry 0 the inside points among the points [2048 b, 2048 (b + 1)), entry 13 the largest (D2 << 32 | ~index) over
// them, entry 14 the same over the outside points (0: no such point; D2 >= 1 otherwise).
__global__ __launch_bounds__(256) void rm_dist_max_kernel(uint32_t n, const uint32_t* __restrict__ vol, unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[12];
    unsigned long long cnt = 0ull, kin = 0ull, kout = 0ull;
#pragma unroll
    for (uint32_t m = 0; m < kDistBlock / 256u; m++) {
        const uint32_t p = blockIdx.x * kDistBlock + m * 256u + threadIdx.x;
        if (p >= n) continue;
        const uint32_t v = vol[p];
        const unsigned long long key = (unsigned long long)(v & kDistNone) << 32 | (unsigned long long)(~p);
        if (v >> 31) {
            cnt++;
            kin = key > kin ? key : kin;
        } else {
            kout = key > kout ? key : kout;
        }
    }
    block_row<32, 32>(cnt, kin, kout, wred, rows);  // (a workgroup counts at most 2048)
}

// ---- features ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_dist_mask_init_kernel(uint32_t n, const uint32_t* __restrict__ vol, uint8_t* __restrict__ mask) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) mask[p] = (uint8_t)(vol[p] >> 31);
}

// feat: the transform towards the core {class CLS, D2 > r2} (a core point: kDistInside).  A point of class CLS farther than r2
// from every core point gets MARK in the mask.  rows[16 b]: entry 0 the core points, entry 1 the marked ones.
template <uint32_t CLS, uint32_t MARK>
__global__ __launch_bounds__(256) void rm_dist_compose_kernel(uint32_t n, const uint32_t* __restrict__ vol, const uint32_t* __restrict__ feat,
                                                              uint32_t r2, uint8_t* __restrict__ mask, unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[4];
    unsigned long long sums = 0ull;
#pragma unroll
    for (uint32_t m = 0; m < kDistBlock / 256u; m++) {
        const uint32_t p = blockIdx.x * kDistBlock + m * 256u + threadIdx.x;
        if (p >= n) continue;
        if ((vol[p] >> 31) != CLS) continue;
        const uint32_t f = feat[p];
        if (f >> 31) {
            sums += 1ull;
        } else if (f > r2) {
            mask[p] = (uint8_t)MARK;
            sums += 1ull << 32;
        }
    }
    block_row<32, 32>(sums, wred, rows);  // (two counts of at most 2048)
}

}  // namespace rmk
