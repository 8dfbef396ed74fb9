// class_mesh_layout_check.cpp -- the layouts of rm_mesh_classes on the CPU, under ASan + UBSan (tests/test_class_mesh_cpu.py):
// rml::ClassMeshScratch and rml::ClassMeshSlot (ray-marching_amd/csrc/rm_abi_layout.h).  The regions lie in declaration order,
// start on 16-byte boundaries, do not overlap and end inside the total; every offset equals the chained align16 formula written out
// here; a walk over the words as the kernels index them (word -> corner, corner -> word) stays inside real allocations of `bytes`
// bytes and visits every corner of the corner lattice exactly once, in the order of L; and the bounds the kernels' packed fields
// rely on hold at the lattice limits.
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

void offsets() {
    CHECK(rml::kCmeshGroupWords == 16u);
    CHECK(rml::cmesh_row_words(2u) == 1u && rml::cmesh_row_words(63u) == 1u && rml::cmesh_row_words(64u) == 2u && rml::cmesh_row_words(127u) == 2u &&
          rml::cmesh_row_words(128u) == 3u && rml::cmesh_row_words(1024u) == 17u);
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{3, 5, 7}, Lattice{63, 3, 4}, Lattice{64, 3, 4}, Lattice{65, 33, 17}, Lattice{1024, 2, 2},
                             Lattice{2, 1024, 2}, Lattice{2, 2, 1024}, Lattice{256, 256, 256}, Lattice{1024, 1024, 256}, Lattice{2, 1024, 1024}}) {
        const size_t n = (size_t)l.nx * l.ny * l.nz;
        const uint32_t wpr = (l.nx + 64u) / 64u, words = wpr * (l.ny + 1u) * (l.nz + 1u), groups = (words + 15u) / 16u;
        const rml::ClassMeshScratch S(l.nx, l.ny, l.nz);
        const size_t bits_o = a16(n), before_o = bits_o + a16((size_t)words * 8u), bsums_o = before_o + a16((size_t)words * 4u),
                     btot_o = bsums_o + a16((size_t)groups * 8u), rows_o = btot_o + 16u, folded_o = rows_o + (size_t)groups * 256u,
                     result_o = folded_o + (size_t)((2u * groups + 255u) / 256u) * 128u;
        CHECK(S.n_words == words && S.n_groups == groups && rml::cmesh_words(l.nx, l.ny, l.nz) == words);
        CHECK(S.cls.offset == 0u && S.bits.offset == bits_o && S.before.offset == before_o && S.bsums.offset == bsums_o && S.btot.offset == btot_o);
        CHECK(S.rows.offset == rows_o && S.folded.offset == folded_o && S.result.offset == result_o && S.bytes == result_o + 128u);
        CHECK(S.cls.bytes == n && S.bits.bytes == (size_t)words * 8u && S.before.bytes == (size_t)words * 4u && S.rows.bytes == (size_t)groups * 256u);
        check_regions({span(S.cls), span(S.bits), span(S.before), span(S.bsums), span(S.btot), span(S.rows), span(S.folded), span(S.result)}, S.bytes);
        // what the packed fields rely on: words and groups fit 32 bits with room, vertices and faces stay below 2^32
        const uint64_t corners = (uint64_t)(l.nx + 1u) * (l.ny + 1u) * (l.nz + 1u);
        const uint64_t faces = 3u * (uint64_t)n + (uint64_t)l.ny * l.nz + (uint64_t)l.nx * l.nz + (uint64_t)l.nx * l.ny;
        CHECK((uint64_t)words * 64u >= corners && words < (1u << 24) && corners < (1ull << 32) && 2u * faces < (1ull << 32) && 2u * faces <= 9u * (uint64_t)n);
    }
    for (const uint64_t V : {0ull, 1ull, 8ull, 26ull, 1000003ull}) {
        const uint64_t T = 2u * V + (V & 1u);
        const rml::ClassMeshSlot M(V, T);
        const size_t tri_o = a16((size_t)V * 12u), ids_o = tri_o + a16((size_t)T * 12u);
        CHECK(M.vertices.offset == 0u && M.triangles.offset == tri_o && M.ids.offset == ids_o && M.bytes == ids_o + a16((size_t)T * 8u));
        CHECK(M.vertices.bytes == V * 12u && M.triangles.bytes == T * 12u && M.ids.bytes == T * 8u);
        check_regions({span(M.vertices), span(M.triangles), span(M.ids)}, M.bytes);
    }
}

// the kernels' index arithmetic: word w, lane -> corner; corner -> word, bit; every access inside real allocations
void walk() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{3, 5, 7}, Lattice{62, 2, 3}, Lattice{63, 3, 2}, Lattice{64, 2, 2}, Lattice{65, 4, 3}, Lattice{127, 2, 2},
                             Lattice{128, 2, 3}}) {
        const rml::ClassMeshScratch S(l.nx, l.ny, l.nz);
        std::vector<char> scratch(S.bytes);
        unsigned long long* bits = S.bits.at(scratch.data());
        uint32_t* before = S.before.at(scratch.data());
        unsigned long long* bsums = S.bsums.at(scratch.data());
        const uint32_t cx = l.nx + 1u, cy = l.ny + 1u, cz = l.nz + 1u, wpr = rml::cmesh_row_words(l.nx);
        uint64_t next = 0;
        for (uint32_t g = 0; g < S.n_groups; g++) {
            for (uint32_t slot = 0; slot < rml::kCmeshGroupWords; slot++) {
                const uint32_t w = g * rml::kCmeshGroupWords + slot;
                if (w >= S.n_words) continue;
                bits[w] = 0ull;
                before[w] = slot;
                const uint32_t wx = w % wpr, r = w / wpr, cj = r % cy, ck = r / cy;
                CHECK(ck < cz);
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const uint32_t ci = wx * 64u + lane;
                    if (ci >= cx) continue;
                    CHECK((uint64_t)ci + (uint64_t)cx * (cj + (uint64_t)cy * ck) == next);  // the order of L
                    next++;
                    const uint32_t back = (ck * cy + cj) * wpr + (ci >> 6);
                    CHECK(back == w && (ci & 63u) == lane);
                    bits[back] |= 1ull << lane;
                }
            }
            bsums[g] = g;
        }
        CHECK(next == (uint64_t)cx * cy * cz);
        for (uint32_t w = 0; w < S.n_words; w++) CHECK(bits[w] != 0ull && before[w] == w % rml::kCmeshGroupWords && bsums[w / rml::kCmeshGroupWords] == w / 16u);
    }
}

}  // namespace

int main() {
    offsets();
    walk();
    std::printf("class mesh layout ok (%d checks)\n", g_checks);
    return 0;
}
