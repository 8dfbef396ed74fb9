// topology_layout_check.cpp -- the scratch and result layouts of rm_label_solid / rm_label_occupancy (rml::TopoScratch and
// rml::TopoRows in ray-marching_amd/csrc/rm_abi_layout.h) on the CPU, under ASan + UBSan (tests/test_topology_cpu.py).  The
// regions lie in declaration order, start on 16-byte boundaries, do not overlap and end inside the total; every offset equals the
// chained align16 formula written out here; the cavities' rows follow the bodies' without a gap (the rows kernel indexes both from
// one base); and a walk over the regions as the kernels index them stays inside a real allocation of `bytes` bytes.
#include "rm_abi_layout.h"

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

void sizes(const Lattice& l, uint32_t& n, uint32_t& nb, uint32_t& n_pblocks, uint32_t& n_rblocks) {
    n = l.nx * l.ny * l.nz;
    nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u);
    n_pblocks = (nb + 255u) / 256u;
    n_rblocks = (n + 2047u) / 2048u;
}

void offsets() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{264, 256, 256}, Lattice{1024, 1024, 256},
                             Lattice{2, 2, 1024}, Lattice{1024, 513, 511}}) {
        uint32_t n, nb, np, nr;
        sizes(l, n, nb, np, nr);
        const rml::TopoScratch S(n, nb, np, nr);
        const size_t occ_o = a16((size_t)n * 4u), ext_o = occ_o + a16(n), cls_o = ext_o + a16(n), rows_o = cls_o + a16(nb),
                     folded_o = rows_o + (size_t)nb * 128u, psums_o = folded_o + (size_t)np * 128u, rsums_o = psums_o + a16((size_t)np * 8u),
                     ptot_o = rsums_o + a16((size_t)nr * 8u), rtot_o = ptot_o + 16u, evals_o = rtot_o + 16u, result_o = evals_o + 16u;
        CHECK(S.parent.offset == 0u && S.occ.offset == occ_o && S.ext.offset == ext_o && S.cls.offset == cls_o && S.rows.offset == rows_o);
        CHECK(S.folded.offset == folded_o && S.psums.offset == psums_o && S.rsums.offset == rsums_o && S.ptot.offset == ptot_o);
        CHECK(S.rtot.offset == rtot_o && S.evals.offset == evals_o && S.result.offset == result_o && S.bytes == result_o + 128u);
        CHECK(S.parent.bytes == (size_t)n * 4u && S.occ.bytes == n && S.ext.bytes == n && S.cls.bytes == nb);
        CHECK(S.rows.bytes == (size_t)nb * 128u && S.folded.bytes == (size_t)np * 128u && S.result.bytes == 128u);
        check_regions({span(S.parent), span(S.occ), span(S.ext), span(S.cls), span(S.rows), span(S.folded), span(S.psums), span(S.rsums),
                       span(S.ptot), span(S.rtot), span(S.evals), span(S.result)}, S.bytes);
        // about 6.3 bytes per point beside the label volume, whatever the shape of the partial bricks
        CHECK(S.bytes <= (size_t)n * 6u + (size_t)nb * 130u + (size_t)nr * 8u + 1024u);
    }
    for (uint64_t B : {0ull, 1ull, 13ull, 1017ull, 1ull << 27})
        for (uint64_t C : {0ull, 1ull, 93ull, 1ull << 27}) {
            const rml::TopoRows R(B, C);
            CHECK(R.bodies.offset == 0u && R.bodies.bytes == B * 128u);
            CHECK(R.cavities.offset == B * 128u && R.cavities.bytes == C * 128u);  // one table of B + C rows
            CHECK(R.bytes == (B + C) * 128u);
        }
}

// every element the kernels touch, in a real allocation of exactly `bytes` bytes (the sanitizer watches its ends)
void walk() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}}) {
        uint32_t n, nb, np, nr;
        sizes(l, n, nb, np, nr);
        const rml::TopoScratch S(n, nb, np, nr);
        std::vector<char> buf(S.bytes);
        char* b = buf.data();
        for (uint32_t p = 0; p < n; p++) {
            S.parent.at(b)[p] = p;
            S.occ.at(b)[p] = 1u;
            S.ext.at(b)[p] = 0u;
        }
        for (uint32_t k = 0; k < nb; k++) {
            S.cls.at(b)[k] = 2u;
            for (int e = 0; e < 16; e++) S.rows.at(b)[(size_t)k * 16u + e] = k;
        }
        for (uint32_t k = 0; k < np; k++) {
            S.psums.at(b)[k] = k;
            for (int e = 0; e < 16; e++) S.folded.at(b)[(size_t)k * 16u + e] = k;
        }
        for (uint32_t k = 0; k < nr; k++) S.rsums.at(b)[k] = k;
        for (int k = 0; k < 2; k++) S.ptot.at(b)[k] = S.rtot.at(b)[k] = S.evals.at(b)[k] = 0ull;
        for (int e = 0; e < 16; e++) S.result.at(b)[e] = 0ull;
        CHECK(S.parent.at(b)[n - 1u] == n - 1u && S.rows.at(b)[(size_t)nb * 16u - 1u] == nb - 1u);
        const rml::TopoRows R(3, 2);
        std::vector<char> rows(R.bytes);
        for (int r = 0; r < 5; r++)
            for (int e = 0; e < 16; e++) R.bodies.at(rows.data())[r * 16 + e] = (unsigned long long)r;  // cavity c is row B + c
        CHECK(R.cavities.at(rows.data())[0] == 3ull && R.cavities.at(rows.data())[31] == 4ull);
    }
}

}  // namespace

int main() {
    offsets();
    walk();
    std::printf("topology layout ok (%d checks)\n", g_checks);
    return 0;
}
