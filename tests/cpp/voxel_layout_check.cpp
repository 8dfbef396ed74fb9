// voxel_layout_check.cpp -- the layouts of rm_voxelize_mesh on the CPU, under ASan + UBSan (tests/test_voxelize_cpu.py):
// rml::VoxScratch (ray-marching_amd/csrc/rm_abi_layout.h) and the fill's staging rml::VoxFillLds (rm_lds_layout.h).  The regions
// lie in declaration order, start on 16-byte boundaries, do not overlap and end inside the total; every offset equals the chained
// align16 formula written out here; the counters and the bit volume form one span; and the fill kernel's indexing -- restated here
// thread by thread -- stays inside real allocations of exactly the described sizes for every nx of 2..1024, visits every byte of
// the occupancy once and gives the prefix parities of the rows' bits.
#include "rm_abi_layout.h"
#include "rm_lds_layout.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
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

struct Case { uint32_t nt, nv_host, nt_host, nx, ny, nz; };

void offsets() {
    for (const Case& c : {Case{1, 0, 0, 2, 2, 2}, Case{20, 12, 20, 20, 18, 16}, Case{257, 771, 0, 33, 20, 17}, Case{1u << 20, 0, 0, 1024, 512, 512},
                          Case{12, 8, 12, 2, 1024, 1024}, Case{5000, 15000, 0, 31, 3, 1024}}) {
        const uint32_t n = c.nx * c.ny * c.nz, nb = (c.nt + 255u) / 256u, W = rml::vox_row_words(c.nx), nw = c.ny * c.nz * W;
        const uint32_t ng = (n + rml::kVoxFillCells - 1u) / rml::kVoxFillCells, nf = (ng + 255u) / 256u;
        CHECK(W == (c.nx + 1u + 31u) / 32u);  // a row of nx + 1 bits
        const rml::VoxScratch S(c.nt, nb, nw, ng, nf, c.nv_host, c.nt_host);
        const size_t starts_o = a16((size_t)c.nt * 48u), bsums_o = starts_o + a16((size_t)c.nt * 4u), btot_o = bsums_o + a16((size_t)nb * 8u),
                     counters_o = btot_o + 16u, bits_o = counters_o + 64u, rows_o = bits_o + a16((size_t)nw * 4u), folded_o = rows_o + (size_t)ng * 128u,
                     result_o = folded_o + (size_t)nf * 128u, xyz_o = result_o + 128u, idx_o = xyz_o + a16((size_t)c.nv_host * 12u);
        CHECK(S.tris.offset == 0u && S.starts.offset == starts_o && S.bsums.offset == bsums_o && S.btot.offset == btot_o);
        CHECK(S.counters.offset == counters_o && S.bits.offset == bits_o && S.rows.offset == rows_o && S.folded.offset == folded_o);
        CHECK(S.result.offset == result_o && S.xyz.offset == xyz_o && S.idx.offset == idx_o);
        CHECK(S.bytes == idx_o + a16((size_t)c.nt_host * 12u));
        CHECK(S.xyz.bytes == (size_t)c.nv_host * 12u && S.idx.bytes == (size_t)c.nt_host * 12u && S.bits.bytes == (size_t)nw * 4u);
        check_regions({span(S.tris), span(S.starts), span(S.bsums), span(S.btot), span(S.counters), span(S.bits), span(S.rows), span(S.folded),
                       span(S.result), span(S.xyz), span(S.idx)}, S.bytes);
        // one memset clears the counters and the bit volume, and nothing else
        CHECK(S.clear_offset() == counters_o && S.clear_offset() + S.clear_bytes() == bits_o + (size_t)nw * 4u);
        CHECK(S.clear_offset() + S.clear_bytes() <= S.rows.offset);
    }
}

void staging() {
    constexpr rml::VoxFillLds L;
    CHECK(L.raw == 0u && L.prefix == a16(rml::kVoxFillMaxWords * 4u) && L.bytes == L.prefix + rml::kVoxFillMaxWords * 4u);
    CHECK(L.bytes + 1024u <= rml::kLdsLaunchLimit);
    uint32_t most = 0u;
    for (uint32_t nx = 2u; nx <= 1024u; nx++) {
        const uint32_t w = rml::vox_fill_rows(nx) * rml::vox_row_words(nx);
        most = w > most ? w : most;
        // the rows any kVoxFillCells consecutive cells lie in
        for (uint32_t p0 : {0u, nx - 1u, 3u * nx + 1u}) {
            const uint32_t r0 = p0 / nx, r1 = (p0 + rml::kVoxFillCells - 1u) / nx;
            CHECK(r1 - r0 + 1u <= rml::vox_fill_rows(nx));
        }
    }
    CHECK(most == rml::kVoxFillMaxWords);
}

uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// rm_vox_fill_kernel, thread by thread, on random bits: every index inside the staged arrays, every byte written once
void fill_walk() {
    constexpr rml::VoxFillLds L;
    uint32_t seed = 27u;
    for (const Case& c : {Case{0, 0, 0, 2, 70, 33}, Case{0, 0, 0, 3, 41, 37}, Case{0, 0, 0, 31, 9, 17}, Case{0, 0, 0, 32, 9, 17}, Case{0, 0, 0, 33, 20, 17},
                          Case{0, 0, 0, 63, 5, 14}, Case{0, 0, 0, 64, 5, 14}, Case{0, 0, 0, 65, 7, 10}, Case{0, 0, 0, 1023, 3, 3}, Case{0, 0, 0, 1024, 3, 2},
                          Case{0, 0, 0, 20, 18, 16}}) {
        const uint32_t nx = c.nx, rows = c.ny * c.nz, n = nx * rows, W = rml::vox_row_words(nx);
        std::vector<uint32_t> bits((size_t)rows * W, 0u);
        for (uint32_t r = 0; r < rows; r++)
            for (uint32_t k = 0; k < 5u; k++) {
                const uint32_t t = rnd(seed) % (nx + 1u);
                bits[(size_t)r * W + (t >> 5)] ^= 1u << (t & 31u);
            }
        std::vector<uint8_t> occ(n, 0xEEu);
        std::vector<uint32_t> written(n, 0u);
        uint64_t inside = 0u, open = 0u;
        const uint32_t groups = (n + rml::kVoxFillCells - 1u) / rml::kVoxFillCells;
        for (uint32_t g = 0; g < groups; g++) {
            std::vector<char> lds(L.bytes);
            uint32_t* s_raw = reinterpret_cast<uint32_t*>(lds.data() + L.raw);
            uint32_t* s_pre = reinterpret_cast<uint32_t*>(lds.data() + L.prefix);
            const uint32_t p0 = g * rml::kVoxFillCells, p1 = p0 + rml::kVoxFillCells < n ? p0 + rml::kVoxFillCells : n;
            const uint32_t r0 = p0 / nx, r1 = (p1 - 1u) / nx, nw = (r1 - r0 + 1u) * W;
            CHECK(nw <= rml::kVoxFillMaxWords && (size_t)r0 * W + nw <= bits.size());
            for (uint32_t t = 0; t < 256u; t++)
                for (uint32_t x = t; x < nw; x += 256u) s_raw[x] = bits[(size_t)r0 * W + x];
            for (uint32_t t = 0; t < 256u; t++)
                for (uint32_t x = t; x < nw; x += 256u) {
                    const uint32_t rl = x / W, w = x - rl * W;
                    uint32_t before = 0u;
                    for (uint32_t y = x - w; y < x; y++) before ^= s_raw[y];
                    uint32_t v = s_raw[x];
                    v ^= v << 1, v ^= v << 2, v ^= v << 4, v ^= v << 8, v ^= v << 16;
                    if (__builtin_popcount(before) & 1) v = ~v;
                    s_pre[x] = v;
                    if (w == W - 1u && (size_t)(r0 + rl) * nx >= p0) open += (v >> (nx & 31u)) & 1u;
                }
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t p = p0 + t * 16u;
                if (p >= p1) continue;
                uint32_t rl = p / nx, i = p - rl * nx;
                rl -= r0;
                for (uint32_t e = 0; e < 16u && p + e < p1; e++) {
                    CHECK(rl * W + (i >> 5) < nw);
                    const uint32_t b = (s_pre[rl * W + (i >> 5)] >> (i & 31u)) & 1u;
                    occ[p + e] = (uint8_t)b;
                    written[p + e]++;
                    inside += b;
                    if (++i == nx) i = 0u, rl++;
                }
            }
        }
        uint64_t want_inside = 0u, want_open = 0u;
        for (uint32_t r = 0; r < rows; r++) {
            uint32_t parity = 0u;
            for (uint32_t t = 0; t <= nx; t++) {
                parity ^= (bits[(size_t)r * W + (t >> 5)] >> (t & 31u)) & 1u;
                if (t < nx) {
                    CHECK(written[r * nx + t] == 1u && occ[r * nx + t] == parity);
                    want_inside += parity;
                }
            }
            want_open += parity;
        }
        CHECK(inside == want_inside && open == want_open);
    }
}

}  // namespace

int main() {
    offsets();
    staging();
    fill_walk();
    std::printf("voxel layout ok (%d checks)\n", g_checks);
    return 0;
}
