// distance_layout_check.cpp -- the layouts of rm_distance_solid / rm_distance_occupancy / rm_distance_features on the CPU, under
// ASan + UBSan (tests/test_distance_cpu.py): rml::DistScratch and rml::DistFeatureScratch (ray-marching_amd/csrc/rm_abi_layout.h)
// and the column tile rml::DistColumnLds (rm_lds_layout.h).  The regions lie in declaration order, start on 16-byte boundaries, do
// not overlap and end inside the total; every offset equals the chained align16 formula written out here; the tile's width is the
// power of two the comment promises; and a walk over the regions and the tile as the kernels index them stays inside a real
// allocation of `bytes` bytes.
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

void sizes(const Lattice& l, uint32_t& n, uint32_t& nb, uint32_t& n_pblocks, uint32_t& n_rblocks, uint32_t& n_fblocks) {
    n = l.nx * l.ny * l.nz;
    nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u);
    n_pblocks = (nb + 255u) / 256u;
    n_rblocks = (n + 2047u) / 2048u;
    n_fblocks = (n_rblocks + 255u) / 256u;
}

void offsets() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{264, 256, 256}, Lattice{1024, 1024, 256},
                             Lattice{2, 2, 1024}, Lattice{1024, 513, 511}}) {
        uint32_t n, nb, np, nr, nf;
        sizes(l, n, nb, np, nr, nf);
        const rml::DistScratch S(n, nb, np, nr, nf);
        const size_t cls_o = a16(n), psums_o = cls_o + a16(nb), rows_o = psums_o + a16((size_t)np * 8u), folded_o = rows_o + (size_t)nr * 128u,
                     ptot_o = folded_o + (size_t)nf * 128u, evals_o = ptot_o + 16u, result_o = evals_o + 16u;
        CHECK(S.occ.offset == 0u && S.cls.offset == cls_o && S.psums.offset == psums_o && S.rows.offset == rows_o);
        CHECK(S.folded.offset == folded_o && S.ptot.offset == ptot_o && S.evals.offset == evals_o && S.result.offset == result_o);
        CHECK(S.bytes == result_o + 128u);
        CHECK(S.occ.bytes == n && S.cls.bytes == nb && S.rows.bytes == (size_t)nr * 128u && S.folded.bytes == (size_t)nf * 128u);
        check_regions({span(S.occ), span(S.cls), span(S.psums), span(S.rows), span(S.folded), span(S.ptot), span(S.evals), span(S.result)},
                      S.bytes);
        // about 1.1 bytes per point beside the distance volume
        CHECK(S.bytes <= (size_t)n + (size_t)n / 15u + (size_t)nb * 2u + 1024u);

        const rml::DistFeatureScratch F(n, nr, nf);
        const size_t frows_o = a16((size_t)n * 4u), ffolded_o = frows_o + (size_t)nr * 128u, fresult_o = ffolded_o + (size_t)nf * 128u;
        CHECK(F.feat.offset == 0u && F.rows.offset == frows_o && F.folded.offset == ffolded_o && F.result.offset == fresult_o);
        CHECK(F.bytes == fresult_o + 128u && F.feat.bytes == (size_t)n * 4u);
        check_regions({span(F.feat), span(F.rows), span(F.folded), span(F.result)}, F.bytes);
    }
}

// the column tile: 16..64 columns, a power of two, within 32 KB unless 16 columns of the axis are more; never above the launch limit
void tiles() {
    for (uint32_t n = 2u; n <= rml::kDistMaxAxis; n++) {
        const uint32_t l = rml::dist_columns_log2(n), xt = 1u << l;
        CHECK(xt >= rml::kDistMinColumns && xt <= rml::kDistMaxColumns);
        CHECK(xt == rml::kDistMinColumns || xt * n <= rml::kDistTileWords);
        CHECK(xt == rml::kDistMaxColumns || 2u * xt * n > rml::kDistTileWords);
        CHECK(256u % xt == 0u);  // whole rows of the tile per pass of the workgroup's 256 threads
        const rml::DistColumnLds L(xt, n);
        CHECK(L.col == 0u && L.bytes == xt * n * 4u && L.bytes <= rml::kLdsLaunchLimit);
    }
    CHECK(rml::dist_columns_log2(128u) == 6u && rml::dist_columns_log2(129u) == 5u && rml::dist_columns_log2(256u) == 5u);
    CHECK(rml::dist_columns_log2(257u) == 4u && rml::dist_columns_log2(1024u) == 4u);
    CHECK(rml::DistColumnLds(16u, 1024u).bytes == 65536u);
}

// every element the kernels touch, in real allocations of exactly `bytes` bytes (the sanitizer watches their ends)
void walk() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{65, 3, 2}}) {
        uint32_t n, nb, np, nr, nf;
        sizes(l, n, nb, np, nr, nf);
        const rml::DistScratch S(n, nb, np, nr, nf);
        std::vector<char> buf(S.bytes);
        char* b = buf.data();
        for (uint32_t p = 0; p < n; p++) S.occ.at(b)[p] = 1u;
        for (uint32_t k = 0; k < nb; k++) S.cls.at(b)[k] = 2u;
        for (uint32_t k = 0; k < np; k++) S.psums.at(b)[k] = k;
        for (uint32_t k = 0; k < nr; k++)
            for (int e = 0; e < 16; e++) S.rows.at(b)[(size_t)k * 16u + e] = k;
        for (uint32_t k = 0; k < nf; k++)
            for (int e = 0; e < 16; e++) S.folded.at(b)[(size_t)k * 16u + e] = k;
        for (int k = 0; k < 2; k++) S.ptot.at(b)[k] = S.evals.at(b)[k] = 0ull;
        for (int e = 0; e < 16; e++) S.result.at(b)[e] = 0ull;
        CHECK(S.occ.at(b)[n - 1u] == 1u && S.rows.at(b)[(size_t)nr * 16u - 1u] == nr - 1u);

        const rml::DistFeatureScratch F(n, nr, nf);
        std::vector<char> fbuf(F.bytes);
        for (uint32_t p = 0; p < n; p++) F.feat.at(fbuf.data())[p] = p;
        for (uint32_t k = 0; k < nr * 16u; k++) F.rows.at(fbuf.data())[k] = k;
        for (uint32_t k = 0; k < nf * 16u; k++) F.folded.at(fbuf.data())[k] = k;
        for (int e = 0; e < 16; e++) F.result.at(fbuf.data())[e] = 0ull;
        CHECK(F.feat.at(fbuf.data())[n - 1u] == n - 1u);

        // the column kernel's staging of the y and the z pass: thread t holds column t & (xt - 1), rows t >> log2(xt), + 256 / xt, ...
        const uint32_t axes[2][3] = {{l.ny, l.nx, l.nx * l.ny}, {l.nz, l.nx * l.ny, l.nx}}, slabs[2] = {l.nz, l.ny};
        std::vector<uint32_t> vol(n, 0u);
        for (int a = 0; a < 2; a++) {
            const uint32_t len = axes[a][0], xl = rml::dist_columns_log2(len), xt = 1u << xl;
            const rml::DistColumnLds L(xt, len);
            std::vector<char> lds(L.bytes);
            uint32_t* col = reinterpret_cast<uint32_t*>(lds.data() + L.col);
            for (uint32_t by = 0; by < slabs[a]; by++)
                for (uint32_t bx = 0; bx < (l.nx + xt - 1u) / xt; bx++)
                    for (uint32_t t = 0; t < 256u; t++) {
                        const uint32_t lx = t & (xt - 1u), x = bx * xt + lx;
                        for (uint32_t q = t >> xl; q < len; q += 256u >> xl) {
                            col[q * xt + lx] = x < l.nx ? vol[by * axes[a][2] + x + q * axes[a][1]] : 0u;
                            if (x < l.nx) vol[by * axes[a][2] + x + q * axes[a][1]] += 1u;
                        }
                    }
        }
        for (uint32_t p = 0; p < n; p++) CHECK(vol[p] == 2u);  // both passes visit every point exactly once
    }
}

}  // namespace

int main() {
    offsets();
    tiles();
    walk();
    std::printf("distance layout ok (%d checks)\n", g_checks);
    return 0;
}
