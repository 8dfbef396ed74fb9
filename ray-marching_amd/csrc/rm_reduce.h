// rm_reduce.h -- the reductions the lattice analyses share, under no feature's name: sums, minima and maxima over a wave, scans
// over a workgroup and over a launch's block sums (rm_block_scan_kernel), and the ROW protocol by which the workgroups of a launch
// hand a few counts to the host: 16 u64 per workgroup (block_row), folded 256 to a workgroup (rm_rows_fold_kernel) and reduced by
// one (rm_rows_reduce_kernel).  Rows plus a reducer instead of 64-bit atomics: nothing to zero, no contention, and no atomic
// decides a result.
#pragma once
#include "rm_kernels.h"

namespace rmk {

// ---- a wave -----------------------------------------------------------------------------------------------------------------
// The xor butterfly over each aligned group of LANES lanes (a power of two; 64: the wave): every lane gets the result, and every
// lane must take part.
template <int LANES, class T, class F>
RM_DEV T wave_reduce(T x, F op) {
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) x = op(x, __shfl_xor(x, o, 64));
    return x;
}
template <int LANES = 64, class T> RM_DEV T wave_sum(T x) { return wave_reduce<LANES>(x, [](T a, T b) { return a + b; }); }
template <int LANES = 64, class T> RM_DEV T wave_or(T x) { return wave_reduce<LANES>(x, [](T a, T b) { return a | b; }); }
template <int LANES = 64, class T> RM_DEV T wave_min(T x) { return wave_reduce<LANES>(x, [](T a, T b) { return a < b ? a : b; }); }
template <int LANES = 64, class T> RM_DEV T wave_max(T x) { return wave_reduce<LANES>(x, [](T a, T b) { return a > b ? a : b; }); }

// ---- scans ------------------------------------------------------------------------------------------------------------------
// Inclusive scan across the 64 lanes of a wave (__shfl_up: the compiler places the cross-lane moves and their waits).
template <class T>
RM_DEV T wave_inclusive_sum(T x) {
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// Exclusive scan across a workgroup of WAVES waves; `total` gets the sum of all.  wsum: WAVES words of LDS.  Ends with a
// barrier, so wsum may be reused by the next call.
template <int WAVES, class T>
RM_DEV T block_exclusive_sum(T v, T* wsum, T& total) {
    const T inc = wave_inclusive_sum(v);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wsum[w] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < WAVES; q++) {
        const T s = wsum[q];
        before += (uint32_t)q < w ? s : (T)0;
        all += s;
    }
    total = all;
    __syncthreads();
    return before + inc - v;
}

// Block sums packed lo | hi << 32 -> exclusive offsets in place (each half modulo 2^32), by one 1024-thread workgroup; the
// two totals as 64-bit numbers, so that a sum that does not fit 32 bits is seen.
__global__ __launch_bounds__(1024) void rm_block_scan_kernel(unsigned long long* __restrict__ block_sums, uint32_t n_blocks,
                                                             unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long wsum[16];
    const uint32_t per = (n_blocks + 1023u) / 1024u, b0 = min(threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    unsigned long long lo = 0, hi = 0;
    for (uint32_t b = b0; b < b1; b++) {
        const unsigned long long v = block_sums[b];
        lo += v & 0xFFFFFFFFull;
        hi += v >> 32;
    }
    unsigned long long tlo, thi;
    unsigned long long olo = block_exclusive_sum<16>(lo, wsum, tlo);
    unsigned long long ohi = block_exclusive_sum<16>(hi, wsum, thi);
    for (uint32_t b = b0; b < b1; b++) {
        const unsigned long long v = block_sums[b];
        block_sums[b] = (olo & 0xFFFFFFFFull) | (ohi << 32);
        olo += v & 0xFFFFFFFFull;
        ohi += v >> 32;
    }
    if (threadIdx.x == 0) {
        totals[0] = tlo;
        totals[1] = thi;
    }
}

// ---- rows -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRowWords = 16u;                       // RM_MOMENTS: one row
constexpr unsigned long long kMassNoMin = 0xFFFFFFFFull;  // the minimum of an empty set (the maximum is 0)

// An entry of a row: 0-9 sums, 10-12 minima, 13-15 maxima.
RM_DEV unsigned long long row_combine(uint32_t e, unsigned long long a, unsigned long long b) {
    return e < 10u ? a + b : e < 13u ? (a < b ? a : b) : (a > b ? a : b);
}
RM_DEV unsigned long long row_identity(uint32_t e) { return e >= 10u && e < 13u ? kMassNoMin : 0ull; }

// This workgroup's row (4 waves), rows[16 blockIdx.x + e]: entries 0, 1, ... the workgroup's sums of the fields of `packed`
// (W... bits each, from bit 0), entries 13 and 14 the maxima of key_a and key_b when KEYS, every other entry its identity.
// THE CALLER BOUNDS THE SUMS: the sum over the whole workgroup of each field must fit the field's width, or it carries into the
// next one.  wred: 4 words of LDS, 12 when KEYS.  Every thread of the workgroup calls it.
template <bool KEYS, uint32_t... W>
RM_DEV void block_row_write(unsigned long long packed, unsigned long long key_a, unsigned long long key_b, unsigned long long* wred,
                            unsigned long long* __restrict__ rows) {
    static_assert((W + ... + 0u) <= 64u && ((W > 0u) && ...) && sizeof...(W) <= 10u, "fields of one packed word, for the summed entries");
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // (wave_sum and two wave_max in one loop: three loops cost rm_dist_max_kernel two registers)
        packed += __shfl_xor(packed, o, 64);
        if (KEYS) {
            const unsigned long long a = __shfl_xor(key_a, o, 64), b = __shfl_xor(key_b, o, 64);
            key_a = a > key_a ? a : key_a;
            key_b = b > key_b ? b : key_b;
        }
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        wred[wave] = packed;
        if (KEYS) wred[4u + wave] = key_a, wred[8u + wave] = key_b;
    }
    __syncthreads();
    if (threadIdx.x < kRowWords) {
        const uint32_t e = threadIdx.x;
        unsigned long long v = row_identity(e);
        if (e < sizeof...(W)) {
            constexpr uint32_t width[] = {W...};
            const unsigned long long all = wred[0] + wred[1] + wred[2] + wred[3];
#pragma unroll
            for (uint32_t f = 0, shift = 0; f < sizeof...(W); shift += width[f++])
                if (e == f) v = (all >> shift) & (~0ull >> (64u - width[f]));
        } else if (KEYS && (e == 13u || e == 14u)) {
            const unsigned long long* k = wred + (e == 13u ? 4u : 8u);
            v = k[0];
#pragma unroll
            for (uint32_t q = 1; q < 4u; q++) v = k[q] > v ? k[q] : v;
        }
        rows[(size_t)blockIdx.x * kRowWords + e] = v;
    }
}
template <uint32_t... W>
RM_DEV void block_row(unsigned long long packed, unsigned long long* wred, unsigned long long* __restrict__ rows) {
    block_row_write<false, W...>(packed, 0ull, 0ull, wred, rows);
}
template <uint32_t... W>
RM_DEV void block_row(unsigned long long packed, unsigned long long key_a, unsigned long long key_b, unsigned long long* wred,
                      unsigned long long* __restrict__ rows) {
    block_row_write<true, W...>(packed, key_a, key_b, wred, rows);
}

// The rows of a launch, kRowsFold to a workgroup, combined entry by entry into folded[16 block]: rm_rows_reduce_kernel (one
// workgroup) then reads one row per 256.  Thread t takes entry t & 15 of the rows t >> 4, + 16, ... as there.
constexpr uint32_t kRowsFold = 256u;
constexpr uint32_t rows_folded(uint32_t n_rows) { return (n_rows + kRowsFold - 1u) / kRowsFold; }
__global__ __launch_bounds__(256) void rm_rows_fold_kernel(const unsigned long long* __restrict__ rows, uint32_t n_rows,
                                                           unsigned long long* __restrict__ folded) {
    __shared__ unsigned long long part[16][kRowWords];
    const uint32_t e = threadIdx.x & 15u, grp = threadIdx.x >> 4, r0 = blockIdx.x * kRowsFold, r1 = min(r0 + kRowsFold, n_rows);
    unsigned long long acc = row_identity(e);
    for (uint32_t r = r0 + grp; r < r1; r += 16u) acc = row_combine(e, acc, rows[(size_t)r * kRowWords + e]);
    part[grp][e] = acc;
    __syncthreads();
    if (threadIdx.x < kRowWords) {
        unsigned long long r = part[0][e];
#pragma unroll
        for (uint32_t q = 1; q < 16u; q++) r = row_combine(e, r, part[q][e]);
        folded[(size_t)blockIdx.x * kRowWords + e] = r;
    }
}

// out[16] = the rows a[0, na) and b[0, nb) combined entry by entry.  Thread t takes entry t & 15 of the rows t >> 4, + 16, ...
// (16 threads read one row: 128 contiguous bytes).
__global__ __launch_bounds__(256) void rm_rows_reduce_kernel(const unsigned long long* __restrict__ a, uint32_t na,
                                                             const unsigned long long* __restrict__ b, uint32_t nb,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[16][kRowWords];
    const uint32_t e = threadIdx.x & 15u, grp = threadIdx.x >> 4;
    unsigned long long sum = 0ull, lo = kMassNoMin, hi = 0ull;
    for (uint32_t r = grp; r < na; r += 16u) {
        const unsigned long long v = a[(size_t)r * kRowWords + e];
        sum += v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    for (uint32_t r = grp; r < nb; r += 16u) {
        const unsigned long long v = b[(size_t)r * kRowWords + e];
        sum += v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    part[grp][e] = e < 10u ? sum : e < 13u ? lo : hi;
    __syncthreads();
    if (threadIdx.x < kRowWords) {
        unsigned long long r = part[0][e];
#pragma unroll
        for (uint32_t q = 1; q < 16u; q++) r = row_combine(e, r, part[q][e]);
        out[e] = r;
    }
}

}  // namespace rmk
