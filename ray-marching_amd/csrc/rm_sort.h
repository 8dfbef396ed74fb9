// rm_sort.h -- a stable device sort of (u64 key, u32 value) pairs by the low `bits` bits of the key, under no feature's name: LSD
// radix sort with 8-bit digits, sort_passes(bits) passes between two buffers.  Included by rm_abi.hip alone.  A pass is
//   count    one workgroup per tile of rml::kSortTile pairs: how many pairs of the tile have each digit, table[digit][tile]
//   scan     the table, digit-major, into exclusive sums in place (block sums, rm_block_scan_kernel, the blocks' own scans): the
//            entry of (digit, tile) becomes the output position of the tile's first pair with that digit
//   scatter  the tile again: every pair goes to its digit's position plus its rank among the tile's pairs with that digit
// The rank is the order of the input: a tile is kSortRounds rounds of 64 pairs (rml::SortLds), a pair's rank within its round is
// the number of lower lanes with its digit (eight ballots), and the rounds before it add their counts (LDS, one writer per word).
// No atomic anywhere: equal keys keep their input order, and two runs write identical buffers.  Bits of the key above `bits` are
// carried along and never looked at.
#pragma once
#include "rm_abi_layout.h"
#include "rm_lds_layout.h"
#include "rm_reduce.h"

namespace rmk {

static_assert(rml::kSortRounds * 64u == rml::kSortTile && rml::kSortLdsDigits == rml::kSortDigits && rml::kSortWaves * 64u == 256u,
              "a tile is kSortRounds rounds of one wave each, kSortWaves at a time");
constexpr uint32_t kSortIts = rml::kSortRounds / rml::kSortWaves;  // passes of the workgroup over its tile

// The lanes of the wave whose pair is valid and has this lane's digit.  Every lane of the wave calls it.
RM_DEV unsigned long long sort_match(uint32_t digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const bool bit = ((digit >> b) & 1u) != 0u;
        const unsigned long long s = __ballot(bit);
        m &= bit ? s : ~s;
    }
    return m;
}
RM_DEV uint32_t sort_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

RM_DEV void sort_clear_rows(uint32_t* rows) {
#pragma unroll
    for (uint32_t q = 0; q < rml::kSortRounds; q++) rows[q * rml::kSortLdsDigits + threadIdx.x] = 0u;
    __syncthreads();
}

// table[d * n_tiles + tile] = the pairs of tile blockIdx.x whose digit (key >> shift) & mask is d (mask: 255, or the bits that are
// left of the key's significant ones in the last pass)
__global__ __launch_bounds__(256) void rm_sort_count_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t mask,
                                                            uint32_t n_tiles, uint32_t* __restrict__ table) {
    constexpr rml::SortLds L;
    __shared__ uint32_t rows[L.bytes / 4u];
    sort_clear_rows(rows);
    const uint32_t lane = sort_lane(), wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t it = 0; it < kSortIts; it++) {
        const size_t idx = (size_t)blockIdx.x * rml::kSortTile + it * 256u + threadIdx.x;
        const bool valid = idx < (size_t)n;
        const uint32_t digit = valid ? (uint32_t)(keys[idx] >> shift) & mask : 0u;
        const unsigned long long m = sort_match(digit, valid);
        if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) rows[(it * rml::kSortWaves + wave) * rml::kSortLdsDigits + digit] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t r = 0; r < rml::kSortRounds; r++) sum += rows[r * rml::kSortLdsDigits + threadIdx.x];
    table[(size_t)threadIdx.x * n_tiles + blockIdx.x] = sum;
}

// The table's scan: the sum of each block of kSortTile entries (lo half of the packed word rm_block_scan_kernel takes), and the
// block's own exclusive scan on top of its offset, in place.
__global__ __launch_bounds__(256) void rm_sort_table_sum_kernel(const uint32_t* __restrict__ table, uint32_t n_entries,
                                                                unsigned long long* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    uint32_t s = 0u;
#pragma unroll
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t idx = blockIdx.x * rml::kSortTile + it * 256u + threadIdx.x;
        if (idx < n_entries) s += table[idx];
    }
    uint32_t total;
    (void)block_exclusive_sum<4>(s, wsum, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void rm_sort_table_scan_kernel(uint32_t* __restrict__ table, uint32_t n_entries,
                                                                 const unsigned long long* __restrict__ offsets) {
    __shared__ uint32_t wsum[4];
    uint32_t carry = (uint32_t)offsets[blockIdx.x];
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t idx = blockIdx.x * rml::kSortTile + it * 256u + threadIdx.x;
        const uint32_t v = idx < n_entries ? table[idx] : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_exclusive_sum<4>(v, wsum, total);
        if (idx < n_entries) table[idx] = ex;
        carry += total;
    }
}

// One pass's scatter; `table` holds the scanned counts.
__global__ __launch_bounds__(256) void rm_sort_scatter_kernel(const unsigned long long* __restrict__ keys_in, const uint32_t* __restrict__ values_in,
                                                              uint32_t n, uint32_t shift, uint32_t mask, uint32_t n_tiles,
                                                              const uint32_t* __restrict__ table,
                                                              unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ values_out) {
    constexpr rml::SortLds L;
    __shared__ uint32_t rows[L.bytes / 4u];
    sort_clear_rows(rows);
    const uint32_t lane = sort_lane(), wave = threadIdx.x >> 6;
    unsigned long long key[kSortIts];
    uint32_t value[kSortIts], rank[kSortIts];  // rank: bit 31 the pair is valid, bits 8.. its rank in the round, bits 0-7 its digit
#pragma unroll
    for (uint32_t it = 0; it < kSortIts; it++) {
        const size_t idx = (size_t)blockIdx.x * rml::kSortTile + it * 256u + threadIdx.x;
        const bool valid = idx < (size_t)n;
        key[it] = valid ? keys_in[idx] : 0ull;
        value[it] = valid ? values_in[idx] : 0u;
        const uint32_t digit = (uint32_t)(key[it] >> shift) & mask;
        const unsigned long long m = sort_match(digit, valid);
        const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid && below == 0u) rows[(it * rml::kSortWaves + wave) * rml::kSortLdsDigits + digit] = (uint32_t)__popcll(m);
        rank[it] = (valid ? 0x80000000u : 0u) | below << 8 | digit;
    }
    __syncthreads();
    {   // thread d: the rounds' counts of digit d -> the position of each round's first pair with it
        uint32_t pos = table[(size_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (uint32_t r = 0; r < rml::kSortRounds; r++) {
            const uint32_t cnt = rows[r * rml::kSortLdsDigits + threadIdx.x];
            rows[r * rml::kSortLdsDigits + threadIdx.x] = pos;
            pos += cnt;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < kSortIts; it++) {
        const uint32_t pos = rows[(it * rml::kSortWaves + wave) * rml::kSortLdsDigits + (rank[it] & 255u)] + ((rank[it] >> 8) & 63u);
        if ((rank[it] >> 31) != 0u && pos < n) {  // (pos < n always: the positions are a permutation)
            keys_out[pos] = key[it];
            values_out[pos] = value[it];
        }
    }
}

}  // namespace rmk

namespace rml {

// Where a sort left its result: the caller's arrays after an even number of passes, the scratch's after an odd one.
struct SortedPairs {
    unsigned long long* keys;
    uint32_t* values;
    uint32_t passes;
};

// Queues the sort of the n pairs (keys[i], values[i]) by the low `bits` bits (1..64) of the keys on `stream`; `scratch` holds
// SortScratch(n).bytes bytes.  Both the caller's arrays and the scratch's are overwritten.  The launches are not checked here:
// the caller asks hipGetLastError() as after its own.
inline SortedPairs sort_pairs(hipStream_t stream, unsigned long long* keys, uint32_t* values, uint32_t n, uint32_t bits, char* scratch) {
    const SortScratch S(n);
    const uint32_t passes = sort_passes(bits), n_tiles = sort_tiles(n), n_entries = n_tiles * kSortDigits, nb = sort_table_blocks(n);
    SortedPairs in{keys, values, passes}, out{S.keys.at(scratch), S.values.at(scratch), passes};
    if (n == 0u) return in;
    uint32_t* table = S.table.at(scratch);
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t left = bits - 8u * p, mask = left >= 8u ? 255u : (1u << left) - 1u;  // the last digit may be short
        hipLaunchKernelGGL(rmk::rm_sort_count_kernel, dim3(n_tiles), dim3(256), 0, stream, in.keys, n, 8u * p, mask, n_tiles, table);
        hipLaunchKernelGGL(rmk::rm_sort_table_sum_kernel, dim3(nb), dim3(256), 0, stream, table, n_entries, S.bsums.at(scratch));
        hipLaunchKernelGGL(rmk::rm_block_scan_kernel, dim3(1), dim3(1024), 0, stream, S.bsums.at(scratch), nb, S.btot.at(scratch));
        hipLaunchKernelGGL(rmk::rm_sort_table_scan_kernel, dim3(nb), dim3(256), 0, stream, table, n_entries, S.bsums.at(scratch));
        hipLaunchKernelGGL(rmk::rm_sort_scatter_kernel, dim3(n_tiles), dim3(256), 0, stream, in.keys, in.values, n, 8u * p, mask, n_tiles, table,
                           out.keys, out.values);
        const SortedPairs t = in;
        in = out;
        out = t;
    }
    return in;
}

}  // namespace rml
