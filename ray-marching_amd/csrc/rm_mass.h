// rm_mass.h -- mass properties (rm_mass_moments): integer moments of the occupancy lattice {d < level}, exact and independent
// of any order.  Included by rm_abi.hip alone, after rm_mesh_sparse.h.  DESIGN.md section 17 is the contract.
//
// The lattice is cut into the bricks of rm_mesh_sparse.h and section 15's rule decides, on the same tile of up to 9 x 9 x 9
// points, which bricks are kept.  A brick's own points (up to 8 x 8 x 8) are a subset of its tile, so a cleared brick's own
// points all lie on the side of `level` its probe lies on: with v < level the brick is INSIDE and contributes the closed-form
// moments of its index box, otherwise nothing.  The passes:
//   probe    one lane per brick: the decision of sparse_probe_brick (the mesh's, expression for expression); the keep flag for
//            rm_sparse_compact_kernel; block sums with the kept bricks in the low half and the inside bricks in the high half
//            (rm_block_scan_kernel scans both); the inside bricks' moments, reduced to ONE row of 16 u64 per workgroup.
//   count    one workgroup per kept brick, two own points per thread: query_distance, moments in brick-local coordinates 0..7
//            (every local sum is below 2^15: two to a 32-bit word), reduced by shuffles and across the waves through LDS,
//            shifted to lattice coordinates once in u64; one row per kept brick.  No tile, no distance goes to memory.
//   reduce   rm_rows_reduce_kernel (rm_reduce.h, whose row protocol this is), one workgroup: the rows of both -> 16 u64.
// The one atomic adds up a statistic (evaluations), as in section 15.
#pragma once
#include "rm_mesh_sparse.h"
#include "rm_reduce.h"

namespace rmk {

// sum of i and of i^2 over [i0, i0 + n), n in 1..8, i0 < 4096: below 2^27
RM_DEV void mass_axis_sums(uint32_t i0, uint32_t n, unsigned long long& s1, unsigned long long& s2) {
    const unsigned long long a = i0, t1 = n * (n - 1u) / 2u, t2 = (n - 1u) * n * (2u * n - 1u) / 6u;
    s1 = n * a + t1;
    s2 = n * a * a + 2ull * a * t1 + t2;
}

// ---- probe ------------------------------------------------------------------------------------------------------------------
// keep[] and block_sums as rm_sparse_probe_kernel writes them (the inside bricks counted in the high half); rows[16 * block]:
// the moments of the block's inside bricks.
template <int LOOP>
__global__ __launch_bounds__(256) void rm_mass_probe_kernel(QueryLaunch Q, SparseGrid g, float level, double L, double err2,
                                                            uint32_t* __restrict__ keep, unsigned long long* __restrict__ block_sums,
                                                            unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wsum[4];
    __shared__ unsigned long long wrow[4][kRowWords];
    static_assert(sizeof wsum + sizeof wrow <= rml::kQueryOwnBrick, "the static LDS the host counts in front of the query columns");
    const uint32_t b = blockIdx.x * 256u + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t k = 0u, in = 0u;
    unsigned long long m[kRowWords];
#pragma unroll
    for (uint32_t e = 0; e < kRowWords; e++) m[e] = row_identity(e);
    if (b < g.nb) {
        const SparseBrick B = sparse_brick(g, b);
        float v;
        k = sparse_probe_brick<LOOP>(Q, query_spill(Q.slots), g, B, level, L, err2, v) ? 1u : 0u;
        in = (k == 0u && v < level) ? 1u : 0u;
        if (in) {
            // the brick's OWN box: [i0, i0 + ex) with ex = min(8, n - i0)
            const uint32_t ex = min(kBrick, g.nx - B.i0), ey = min(kBrick, g.ny - B.j0), ez = min(kBrick, g.nz - B.k0);
            unsigned long long x1, x2, y1, y2, z1, z2;
            mass_axis_sums(B.i0, ex, x1, x2);
            mass_axis_sums(B.j0, ey, y1, y2);
            mass_axis_sums(B.k0, ez, z1, z2);
            m[0] = ex * ey * ez;
            m[1] = x1 * (ey * ez); m[2] = y1 * (ex * ez); m[3] = z1 * (ex * ey);
            m[4] = x2 * (ey * ez); m[5] = y2 * (ex * ez); m[6] = z2 * (ex * ey);
            m[7] = x1 * y1 * ez; m[8] = y1 * z1 * ex; m[9] = x1 * z1 * ey;  // < 2^27 * 2^27 * 2^3
            m[10] = B.i0; m[11] = B.j0; m[12] = B.k0;
            m[13] = B.i0 + ex - 1u; m[14] = B.j0 + ey - 1u; m[15] = B.k0 + ez - 1u;
        }
    }
    if (b <= g.nb) keep[b] = k;
    if (__ballot(in) != 0ull) {  // wave-uniform: most waves hold no inside brick
#pragma unroll
        for (uint32_t e = 0; e < kRowWords; e++)
            m[e] = wave_reduce<64>(m[e], [e](unsigned long long a, unsigned long long b) { return row_combine(e, a, b); });
    }
    if (lane == 0u) {
#pragma unroll
        for (uint32_t e = 0; e < kRowWords; e++) wrow[wave][e] = m[e];
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>((unsigned long long)k | (unsigned long long)in << 32, wsum, total);  // (its barriers order wrow)
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
    if (threadIdx.x < kRowWords) {
        const uint32_t e = threadIdx.x;
        unsigned long long r = wrow[0][e];
#pragma unroll
        for (uint32_t w = 1; w < 4u; w++) r = row_combine(e, r, wrow[w][e]);
        rows[(size_t)blockIdx.x * kRowWords + e] = r;
    }
}

// ---- count ------------------------------------------------------------------------------------------------------------------
template <int LOOP>
__global__ __launch_bounds__(256) void rm_mass_count_kernel(QueryLaunch Q, SparseGrid g, float level, const uint32_t* __restrict__ klist,
                                                            unsigned long long* __restrict__ rows,
                                                            unsigned long long* __restrict__ evaluations) {
    __shared__ uint32_t wred[4][8];
    static_assert(sizeof wred <= rml::kQueryOwnBrick, "the static LDS the host counts in front of the query columns");
    const uint32_t c = blockIdx.x, b = klist[c], wave = threadIdx.x >> 6;
    const SparseBrick B = sparse_brick(g, b);
    const uint32_t ex = min(kBrick, g.nx - B.i0), ey = min(kBrick, g.ny - B.j0), ez = min(kBrick, g.nz - B.k0);  // its own points
    float* spill = query_spill(Q.slots);
    // this thread's two points: (il, jl, wave) and (il, jl, wave + 4)
    const uint32_t il = threadIdx.x & 7u, jl = (threadIdx.x >> 3) & 7u;
    uint32_t cnt = 0u, sn = 0u, snn = 0u, kbits = 0u;
    if (il < ex && jl < ey) {
        const float x = grid_coord(g.ox, B.i0 + il, g.sx), y = grid_coord(g.oy, B.j0 + jl, g.sy);
#pragma unroll
        for (uint32_t half = 0; half < 2u; half++) {
            const uint32_t kl = wave + 4u * half;
            if (kl < ez) {
                const float d = query_distance<LOOP>(Q, spill, x, y, grid_coord(g.oz, B.k0 + kl, g.sz));
                const uint32_t in = d < level ? 1u : 0u;  // NaN is outside
                cnt += in;
                sn += kl * in;
                snn += kl * kl * in;
                kbits |= in << (16u + kl);
            }
        }
    }
    // local sums, two to a word: over the brick each stays below 2^15 (count <= 512, first moments <= 7 * 512, second <= 49 * 512)
    uint32_t w0 = cnt | (il * cnt) << 16;               // count, sum l
    uint32_t w1 = (jl * cnt) | sn << 16;                // sum m, sum n
    uint32_t w2 = (il * il * cnt) | (jl * jl * cnt) << 16;  // sum l^2, sum m^2
    uint32_t w3 = snn | (il * jl * cnt) << 16;          // sum n^2, sum l m
    uint32_t w4 = (jl * sn) | (il * sn) << 16;          // sum m n, sum l n
    uint32_t w5 = kbits | (cnt ? (1u << il) | (1u << (8u + jl)) : 0u);  // which l, m, n occur: bits 0-7, 8-15, 16-23
    w0 = wave_sum(w0); w1 = wave_sum(w1); w2 = wave_sum(w2); w3 = wave_sum(w3); w4 = wave_sum(w4);
    w5 = wave_or(w5);
    if ((threadIdx.x & 63u) == 0u) {
        wred[wave][0] = w0; wred[wave][1] = w1; wred[wave][2] = w2; wred[wave][3] = w3; wred[wave][4] = w4; wred[wave][5] = w5;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        w0 = wred[0][0] + wred[1][0] + wred[2][0] + wred[3][0];
        w1 = wred[0][1] + wred[1][1] + wred[2][1] + wred[3][1];
        w2 = wred[0][2] + wred[1][2] + wred[2][2] + wred[3][2];
        w3 = wred[0][3] + wred[1][3] + wred[2][3] + wred[3][3];
        w4 = wred[0][4] + wred[1][4] + wred[2][4] + wred[3][4];
        w5 = wred[0][5] | wred[1][5] | wred[2][5] | wred[3][5];
        // to lattice coordinates, once, in u64: sum (i0 + l) = i0 c + sum l; sum (i0 + l)^2 = i0^2 c + 2 i0 sum l + sum l^2;
        // sum (i0 + l)(j0 + m) = i0 j0 c + i0 sum m + j0 sum l + sum l m
        const unsigned long long n = w0 & 0xFFFFu, sl = w0 >> 16, sm = w1 & 0xFFFFu, sN = w1 >> 16, sll = w2 & 0xFFFFu, smm = w2 >> 16,
                                 sNN = w3 & 0xFFFFu, slm = w3 >> 16, smn = w4 & 0xFFFFu, sln = w4 >> 16;
        const unsigned long long i0 = B.i0, j0 = B.j0, k0 = B.k0;
        unsigned long long* row = rows + (size_t)c * kRowWords;
        row[0] = n;
        row[1] = i0 * n + sl;
        row[2] = j0 * n + sm;
        row[3] = k0 * n + sN;
        row[4] = i0 * i0 * n + 2ull * i0 * sl + sll;
        row[5] = j0 * j0 * n + 2ull * j0 * sm + smm;
        row[6] = k0 * k0 * n + 2ull * k0 * sN + sNN;
        row[7] = i0 * j0 * n + i0 * sm + j0 * sl + slm;
        row[8] = j0 * k0 * n + j0 * sN + k0 * sm + smn;
        row[9] = i0 * k0 * n + i0 * sN + k0 * sl + sln;
        const uint32_t bl = w5 & 0xFFu, bm = (w5 >> 8) & 0xFFu, bn = (w5 >> 16) & 0xFFu;
        const bool any = n != 0ull;  // (then all three sets have a member)
        row[10] = any ? i0 + (uint32_t)__builtin_ctz(bl | 0x100u) : kMassNoMin;
        row[11] = any ? j0 + (uint32_t)__builtin_ctz(bm | 0x100u) : kMassNoMin;
        row[12] = any ? k0 + (uint32_t)__builtin_ctz(bn | 0x100u) : kMassNoMin;
        row[13] = any ? i0 + (31u - (uint32_t)__builtin_clz(bl | 1u)) : 0ull;
        row[14] = any ? j0 + (31u - (uint32_t)__builtin_clz(bm | 1u)) : 0ull;
        row[15] = any ? k0 + (31u - (uint32_t)__builtin_clz(bn | 1u)) : 0ull;
        atomicAdd(evaluations, (unsigned long long)(ex * ey * ez));  // a statistic: nothing depends on it
    }
}

}  // namespace rmk
