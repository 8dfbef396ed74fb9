// surface_layout_check.cpp -- the layouts of rm_surface_solid / rm_surface_classes on the CPU, under ASan + UBSan
// (tests/test_surface_cpu.py): rml::SurfScratch (ray-marching_amd/csrc/rm_abi_layout.h) and the tile rml::SurfTileLds
// (rm_lds_layout.h).  The regions lie in declaration order, start on 16-byte boundaries, do not overlap and end inside the total;
// every offset equals the chained align16 formula written out here; and a walk over the tiles as rm_surf_count_kernel indexes them
// stays inside real allocations of `bytes` bytes, reads every lattice point as an owner exactly once, and finds every pair of the
// padded lattice exactly once.
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

struct Lattice { uint32_t nx, ny, nz; };

uint32_t groups_of(const Lattice& l) {
    const uint32_t tiles = rml::surf_tiles(l.nx, rml::kSurfTileX) * rml::surf_tiles(l.ny, rml::kSurfTileY) * rml::surf_tiles(l.nz, rml::kSurfTileZ);
    return tiles < rml::kSurfMaxGroups ? tiles : rml::kSurfMaxGroups;
}

void offsets() {
    CHECK(rml::kSurfRowWords == 840u && rml::kSurfCounts == 840u && rml::kSurfCounts == 8u + 8u * 8u * 13u);
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{3, 5, 7}, Lattice{65, 33, 17}, Lattice{1024, 2, 2}, Lattice{2, 1024, 2}, Lattice{2, 2, 1024},
                             Lattice{264, 256, 256}, Lattice{1024, 1024, 256}, Lattice{1024, 513, 511}}) {
        const uint32_t n = l.nx * l.ny * l.nz, nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u), np = (nb + 255u) / 256u;
        const uint32_t groups = groups_of(l);
        CHECK(groups >= 1u && groups <= 1024u);
        const rml::SurfScratch S(n, nb, np, groups);
        const size_t cls_o = a16(n), psums_o = cls_o + a16(nb), ptot_o = psums_o + a16((size_t)np * 8u), evals_o = ptot_o + 16u,
                     rows_o = evals_o + 16u, result_o = rows_o + a16((size_t)groups * 840u * 4u);
        CHECK(S.occ.offset == 0u && S.cls.offset == cls_o && S.psums.offset == psums_o && S.ptot.offset == ptot_o && S.evals.offset == evals_o);
        CHECK(S.rows.offset == rows_o && S.result.offset == result_o && S.bytes == result_o + 840u * 8u && S.n_groups == groups);
        CHECK(S.occ.bytes == n && S.rows.bytes == (size_t)groups * 3360u && S.result.bytes == 6720u);
        check_regions({span(S.occ), span(S.cls), span(S.psums), span(S.ptot), span(S.evals), span(S.rows), span(S.result)}, S.bytes);
        // a workgroup's 32-bit bins hold the owners of all its tiles
        const uint64_t tiles = (uint64_t)rml::surf_tiles(l.nx, 64u) * rml::surf_tiles(l.ny, 16u) * rml::surf_tiles(l.nz, 8u);
        CHECK((tiles + groups - 1u) / groups * 8192u < (1ull << 32));
    }
}

void tile() {
    constexpr rml::SurfTileLds T;
    CHECK(rml::kSurfTileX == 64u && rml::kSurfTileY == 16u && rml::kSurfTileZ == 8u);
    CHECK(T.pitch == 65u && T.rows_y == 18u && T.rows_z == 10u && T.cls == 0u && T.counts == 11712u && T.bytes == 11712u + 3360u && T.bytes == 15072u);
    CHECK(T.counts % 16u == 0u && T.counts >= 65u * 18u * 10u && T.bytes + 1024u <= rml::kLdsLaunchLimit);
    CHECK(rml::surf_tiles(2u, 64u) == 1u && rml::surf_tiles(62u, 64u) == 1u && rml::surf_tiles(63u, 64u) == 2u && rml::surf_tiles(1024u, 64u) == 17u);
    CHECK(rml::surf_tiles(14u, 16u) == 1u && rml::surf_tiles(15u, 16u) == 2u && rml::surf_tiles(6u, 8u) == 1u && rml::surf_tiles(7u, 8u) == 2u);
}

const int kDir[13][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1},  {1, 1, 0}, {1, -1, 0}, {1, 0, 1},  {1, 0, -1},
                         {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};

// the kernel's staging and pair loops, with a class of 1 everywhere in the lattice: every read in real allocations of exactly
// `bytes` bytes (the sanitizer watches their ends)
void walk() {
    constexpr rml::SurfTileLds T;
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{3, 5, 7}, Lattice{62, 14, 6}, Lattice{63, 15, 7}, Lattice{64, 16, 8}, Lattice{65, 33, 17},
                             Lattice{130, 2, 3}, Lattice{2, 3, 40}}) {
        const uint32_t n = l.nx * l.ny * l.nz;
        std::vector<unsigned char> lattice(n, 1u);
        std::vector<uint32_t> owned(n, 0u);
        std::vector<unsigned char> lds(T.bytes);
        unsigned char* s_cls = lds.data() + T.cls;
        const uint32_t tx = rml::surf_tiles(l.nx, 64u), ty = rml::surf_tiles(l.ny, 16u), tz = rml::surf_tiles(l.nz, 8u);
        uint64_t pairs[13] = {}, inner[13] = {};
        for (uint32_t tile_i = 0; tile_i < tx * ty * tz; tile_i++) {
            const uint32_t ti = tile_i % tx, r = tile_i / tx, tj = r % ty, tk = r / ty;
            const int x0 = (int)(ti * 64u) - 1, y0 = (int)(tj * 16u) - 1, z0 = (int)(tk * 8u) - 1;
            for (uint32_t row = 0; row < T.rows_y * T.rows_z; row++) {
                const uint32_t cz = row / T.rows_y, cy = row - cz * T.rows_y;
                const int gy = y0 - 1 + (int)cy, gz = z0 - 1 + (int)cz;
                for (uint32_t cx = 0; cx <= 64u; cx++) {
                    const int gx = x0 + (int)cx;
                    unsigned char v = 0u;
                    if ((uint32_t)gx < l.nx && (uint32_t)gy < l.ny && (uint32_t)gz < l.nz) {
                        const uint32_t at = ((uint32_t)gz * l.ny + (uint32_t)gy) * l.nx + (uint32_t)gx;
                        CHECK(at < n);
                        v = lattice[at];
                    }
                    s_cls[row * T.pitch + cx] = v;
                }
            }
            for (uint32_t row = 0; row < 16u * 8u; row++) {
                const uint32_t lz = row / 16u, ly = row - lz * 16u;
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const unsigned char* own = s_cls + ((lz + 1u) * T.rows_y + ly + 1u) * T.pitch + lane;
                    const int gx = x0 + (int)lane, gy = y0 + (int)ly, gz = z0 + (int)lz;
                    if (own[0] != 0u) {
                        CHECK((uint32_t)gx < l.nx && (uint32_t)gy < l.ny && (uint32_t)gz < l.nz);
                        owned[((uint32_t)gz * l.ny + (uint32_t)gy) * l.nx + (uint32_t)gx]++;
                    }
                    for (int d = 0; d < 13; d++) {
                        const unsigned char b = own[(kDir[d][2] * (int)T.rows_y + kDir[d][1]) * (int)T.pitch + kDir[d][0]];
                        if (own[0] != 0u || b != 0u) pairs[d]++;
                        if (own[0] != 0u && b != 0u) inner[d]++;
                    }
                }
            }
        }
        for (uint32_t p = 0; p < n; p++) CHECK(owned[p] == 1u);
        // a full lattice: along nu the pairs inside are prod(n - |nu|), and every point has one pair with the padding on either side
        for (int d = 0; d < 13; d++) {
            const uint64_t in = (uint64_t)(l.nx - (uint32_t)std::abs(kDir[d][0])) * (l.ny - (uint32_t)std::abs(kDir[d][1])) * (l.nz - (uint32_t)std::abs(kDir[d][2]));
            CHECK(inner[d] == in);
            CHECK(pairs[d] == in + 2u * ((uint64_t)n - in));
        }
    }
}

}  // namespace

int main() {
    offsets();
    tile();
    walk();
    std::printf("surface layout ok (%d checks)\n", g_checks);
    return 0;
}
