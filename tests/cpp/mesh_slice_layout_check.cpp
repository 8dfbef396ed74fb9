// mesh_slice_layout_check.cpp -- the layouts of the device sort and of rm_slice_mesh on the CPU, under ASan + UBSan
// (tests/test_mesh_slice_cpu.py): rml::SortScratch, rml::MeshSliceScratch and rml::MeshSliceItems (ray-marching_amd/csrc/
// rm_abi_layout.h) and the sort's static LDS rml::SortLds (rm_lds_layout.h).  The regions lie in declaration order, start on
// 16-byte boundaries, do not overlap and end inside the total; the offsets equal the chained align16 formula written out here; and
// the sort's indexing -- count, table scan and scatter restated thread by thread, with the rounds, rows and table entries where the
// kernels put them -- stays inside real allocations of exactly the described sizes, writes every output slot once and sorts stably.
#include "rm_abi_layout.h"
#include "rm_lds_layout.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <numeric>
#include <vector>

namespace {

int g_checks = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

size_t a16(size_t b) { return (b + 15u) & ~(size_t)15u; }

struct Span { size_t offset, bytes; };
template <class T>
Span span(const rml::Region<T>& r) { return Span{r.offset, r.bytes}; }

void check_regions(std::initializer_list<Span> regions, size_t total) {
    size_t end = 0;
    for (const Span& r : regions) {
        CHECK(r.offset % 16u == 0u);
        CHECK(r.offset >= end);
        end = r.offset + r.bytes;
        CHECK(end >= r.offset && end <= total);
    }
}

void offsets() {
    static_assert(rml::kSortTile == 1024u && rml::kSortDigits == 256u && rml::kSortRounds * 64u == rml::kSortTile, "the tile");
    constexpr rml::SortLds L;
    static_assert(L.rows == 0u && L.bytes == 16u * 256u * 4u, "one row of 256 words per round");
    CHECK(rml::sort_passes(1) == 1u && rml::sort_passes(8) == 1u && rml::sort_passes(9) == 2u && rml::sort_passes(64) == 8u);
    for (uint32_t n : {1u, 63u, 1023u, 1024u, 1025u, 4096u, 1050000u, 0xFFFFFFFFu}) {
        const uint32_t tiles = (uint32_t)(((uint64_t)n + 1023u) / 1024u), blocks = (uint32_t)(((uint64_t)tiles * 256u + 1023u) / 1024u);
        CHECK(rml::sort_tiles(n) == tiles && rml::sort_table_blocks(n) == blocks);
        const rml::SortScratch S(n);
        const size_t values_o = a16((size_t)n * 8u), table_o = values_o + a16((size_t)n * 4u), bsums_o = table_o + a16((size_t)tiles * 1024u),
                     btot_o = bsums_o + a16((size_t)blocks * 8u);
        CHECK(S.keys.offset == 0u && S.values.offset == values_o && S.table.offset == table_o && S.bsums.offset == bsums_o && S.btot.offset == btot_o);
        CHECK(S.bytes == btot_o + 16u);
        check_regions({span(S.keys), span(S.values), span(S.table), span(S.bsums), span(S.btot)}, S.bytes);
    }
    struct Case { uint32_t nv, nt, nl, hv, ht; };
    for (const Case& c : {Case{3, 1, 1, 3, 1}, Case{8, 12, 4, 8, 12}, Case{642, 1280, 40, 0, 0}, Case{1u << 20, 1u << 21, 65536, 0, 0},
                          Case{5, 1u << 28, 7, 0, 0}}) {
        const uint32_t H = 3u * c.nt, hb = (H + 255u) / 256u;
        const rml::MeshSliceScratch S(c.nv, c.nt, c.nl, c.hv, c.ht);
        const size_t p2_o = a16((size_t)c.nv * 12u), hkeys_o = p2_o + a16((size_t)c.nl * 4u), hvals_o = hkeys_o + a16((size_t)H * 8u),
                     mate_o = hvals_o + a16((size_t)H * 4u), estart_o = mate_o + a16((size_t)H * 4u), k0_o = estart_o + a16(((size_t)H + 1u) * 4u),
                     bsums_o = k0_o + a16((size_t)H * 4u), btot_o = bsums_o + a16((size_t)((H + 1023u) / 1024u) * 8u), rows_o = btot_o + 16u,
                     folded_o = rows_o + (size_t)hb * 128u, result_o = folded_o + (size_t)((hb + 255u) / 256u) * 128u, xyz_o = result_o + 128u,
                     idx_o = xyz_o + a16((size_t)c.hv * 12u), sort_o = idx_o + a16((size_t)c.ht * 12u);
        CHECK(S.vq.offset == 0u && S.p2.offset == p2_o && S.hkeys.offset == hkeys_o && S.hvals.offset == hvals_o && S.mate.offset == mate_o);
        CHECK(S.estart.offset == estart_o && S.k0.offset == k0_o && S.bsums.offset == bsums_o && S.btot.offset == btot_o && S.rows.offset == rows_o);
        CHECK(S.folded.offset == folded_o && S.result.offset == result_o && S.xyz.offset == xyz_o && S.idx.offset == idx_o && S.sort == sort_o);
        CHECK(S.bytes == sort_o + rml::SortScratch(H).bytes);
        check_regions({span(S.vq), span(S.p2), span(S.hkeys), span(S.hvals), span(S.mate), span(S.estart), span(S.k0), span(S.bsums), span(S.btot),
                       span(S.rows), span(S.folded), span(S.result), span(S.xyz), span(S.idx)}, S.sort);
    }
    for (uint32_t N : {1u, 255u, 256u, 257u, 70000u, 0xFFFFFFFFu}) {
        for (uint32_t nl : {1u, 300u, 65536u}) {
            const rml::MeshSliceItems I(N, nl);
            const uint32_t vb = (uint32_t)(((uint64_t)N + 255u) / 256u);
            const size_t ivals_o = a16((size_t)N * 8u), inv_o = ivals_o + a16((size_t)N * 4u), vh_o = inv_o + a16((size_t)N * 4u),
                         base_o = vh_o + a16((size_t)N * 4u), totals_o = base_o + a16(((size_t)nl + 1u) * 4u), rows_o = totals_o + 16u;
            CHECK(I.ikeys.offset == 0u && I.ivals.offset == ivals_o && I.inv.offset == inv_o && I.vh.offset == vh_o && I.layer_base.offset == base_o);
            CHECK(I.totals.offset == totals_o && I.rows.offset == rows_o);
            CHECK(I.rows.bytes == (size_t)vb * 128u && I.folded.bytes == (size_t)((vb + 255u) / 256u) * 128u);
            CHECK(I.bytes == I.sort + rml::SortScratch(N).bytes);
            check_regions({span(I.ikeys), span(I.ivals), span(I.inv), span(I.vh), span(I.layer_base), span(I.totals), span(I.rows), span(I.folded),
                           span(I.result)}, I.sort);
        }
    }
}

// One pass of the sort as the kernels index it: workgroup `tile`, thread t (wave t >> 6, lane t & 63), pass `it` over the tile.
void sort_pass(const std::vector<unsigned long long>& kin, const std::vector<uint32_t>& vin, uint32_t shift, uint32_t mask,
               std::vector<unsigned long long>& kout, std::vector<uint32_t>& vout) {
    const uint32_t n = (uint32_t)kin.size(), tiles = rml::sort_tiles(n), entries = tiles * rml::kSortDigits, blocks = rml::sort_table_blocks(n);
    constexpr rml::SortLds L;
    std::vector<uint32_t> table((size_t)tiles * rml::kSortDigits);
    const uint32_t its = rml::kSortRounds / rml::kSortWaves;
    // count
    for (uint32_t tile = 0; tile < tiles; tile++) {
        std::vector<uint32_t> rows(L.bytes / 4u, 0u);
        for (uint32_t it = 0; it < its; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const size_t idx = (size_t)tile * rml::kSortTile + it * 256u + t;
                if (idx >= n) continue;
                const uint32_t digit = (uint32_t)(kin[idx] >> shift) & mask, round = it * rml::kSortWaves + (t >> 6);
                rows[round * rml::kSortLdsDigits + digit]++;  // (the wave's leader writes the ballot's count: the same number)
            }
        for (uint32_t d = 0; d < 256u; d++) {
            uint32_t sum = 0;
            for (uint32_t r = 0; r < rml::kSortRounds; r++) sum += rows[r * rml::kSortLdsDigits + d];
            table[(size_t)d * tiles + tile] = sum;
        }
    }
    // scan: block sums, their exclusive scan, the blocks' own scans on top
    std::vector<unsigned long long> bsums(blocks);
    for (uint32_t b = 0; b < blocks; b++) {
        unsigned long long s = 0;
        for (uint32_t q = 0; q < rml::kSortTile; q++)
            if (b * rml::kSortTile + q < entries) s += table[b * rml::kSortTile + q];
        bsums[b] = s;
    }
    unsigned long long run = 0;
    for (uint32_t b = 0; b < blocks; b++) {
        const unsigned long long v = bsums[b];
        bsums[b] = run;
        run += v;
    }
    CHECK(run == n);
    for (uint32_t b = 0; b < blocks; b++) {
        uint32_t carry = (uint32_t)bsums[b];
        for (uint32_t q = 0; q < rml::kSortTile; q++) {
            const uint32_t idx = b * rml::kSortTile + q;
            if (idx >= entries) break;
            const uint32_t v = table[idx];
            table[idx] = carry;
            carry += v;
        }
    }
    // scatter
    std::vector<uint8_t> written(n, 0);
    for (uint32_t tile = 0; tile < tiles; tile++) {
        std::vector<uint32_t> rows(L.bytes / 4u, 0u), rank((size_t)its * 256u, 0u);
        for (uint32_t it = 0; it < its; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const size_t idx = (size_t)tile * rml::kSortTile + it * 256u + t;
                if (idx >= n) continue;
                const uint32_t digit = (uint32_t)(kin[idx] >> shift) & mask, round = it * rml::kSortWaves + (t >> 6);
                rank[it * 256u + t] = rows[round * rml::kSortLdsDigits + digit]++;  // the lower lanes of the wave with this digit
            }
        for (uint32_t d = 0; d < 256u; d++) {
            uint32_t pos = table[(size_t)d * tiles + tile];
            for (uint32_t r = 0; r < rml::kSortRounds; r++) {
                const uint32_t cnt = rows[r * rml::kSortLdsDigits + d];
                rows[r * rml::kSortLdsDigits + d] = pos;
                pos += cnt;
            }
        }
        for (uint32_t it = 0; it < its; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const size_t idx = (size_t)tile * rml::kSortTile + it * 256u + t;
                if (idx >= n) continue;
                const uint32_t digit = (uint32_t)(kin[idx] >> shift) & mask, round = it * rml::kSortWaves + (t >> 6);
                const uint32_t pos = rows[round * rml::kSortLdsDigits + digit] + rank[it * 256u + t];
                CHECK(pos < n && !written[pos]);
                written[pos] = 1;
                kout[pos] = kin[idx];
                vout[pos] = vin[idx];
            }
    }
}

void sort_indexing() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (uint32_t n : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 1023u, 1024u, 1025u, 5000u}) {
        for (uint32_t bits : {1u, 8u, 9u, 16u, 40u, 64u}) {
            std::vector<unsigned long long> k(n), k2(n);
            std::vector<uint32_t> v(n), v2(n);
            for (uint32_t i = 0; i < n; i++) k[i] = next() >> (i % 3u == 0u ? 0u : 58u), v[i] = i;
            const std::vector<unsigned long long> k0 = k;
            const unsigned long long mask = bits == 64u ? ~0ull : (1ull << bits) - 1ull;
            std::vector<uint32_t> want(n);
            std::iota(want.begin(), want.end(), 0u);
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return (k0[a] & mask) < (k0[b] & mask); });
            for (uint32_t p = 0; p < rml::sort_passes(bits); p++) {
                const uint32_t left = bits - 8u * p;  // the last digit may be short: bits above `bits` never take part
                sort_pass(k, v, 8u * p, left >= 8u ? 255u : (1u << left) - 1u, k2, v2);
                k.swap(k2);
                v.swap(v2);
            }
            for (uint32_t i = 0; i < n; i++) CHECK(v[i] == want[i] && k[i] == k0[want[i]]);
        }
    }
}

}  // namespace

int main() {
    offsets();
    sort_indexing();
    std::printf("mesh_slice_layout_check: ok (%d checks)\n", g_checks);
    return 0;
}
