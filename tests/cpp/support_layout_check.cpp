// support_layout_check.cpp -- the layouts of rm_support_solid / rm_support_occupancy on the CPU, under ASan + UBSan
// (tests/test_support_cpu.py): rml::SupportScratch and rml::SupportProfile (ray-marching_amd/csrc/rm_abi_layout.h) and the
// overhang tile rml::SupCoverLds (rm_lds_layout.h).  The regions lie in declaration order, start on 16-byte boundaries, do not
// overlap and end inside the total; every offset equals the chained align16 formula written out here; the tile gives every thread
// of a workgroup at most one word and stays far below the launch limit; and a walk over the planes and the tile as the kernels
// index them, for all three frames, stays inside real allocations of `bytes` bytes and visits every word and point exactly once.
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

// the canonical frame of rm_abi.hip's sup_frame, written out again: points along the bit axis, the row axis and the up axis,
// and the strides of the three in the caller's array
struct Frame { uint32_t nu, nv, nh, nw, su, sv, sh; };
Frame frame(const Lattice& l, uint32_t axis) {
    Frame f = axis == 0u   ? Frame{l.ny, l.nz, l.nx, 0u, l.nx, l.nx * l.ny, 1u}
              : axis == 1u ? Frame{l.nx, l.nz, l.ny, 0u, 1u, l.nx * l.ny, l.nx}
                           : Frame{l.nx, l.ny, l.nz, 0u, 1u, l.nx, l.nx * l.ny};
    f.nw = (f.nu + 63u) / 64u;
    return f;
}

void offsets() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{65, 3, 2}, Lattice{264, 256, 256},
                             Lattice{1024, 1024, 256}, Lattice{2, 2, 1024}, Lattice{1024, 513, 511}})
        for (uint32_t axis = 0; axis < 3u; axis++) {
            const Frame f = frame(l, axis);
            const uint32_t n = l.nx * l.ny * l.nz, nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u), np = (nb + 255u) / 256u;
            const uint32_t words = f.nh * f.nv * f.nw;
            const rml::SupportScratch S(n, nb, np, words);
            const size_t cls_o = a16(n), psums_o = cls_o + a16(nb), ptot_o = psums_o + a16((size_t)np * 8u), evals_o = ptot_o + 16u,
                         ins_o = evals_o + 16u, plane = a16((size_t)words * 8u), plate_o = ins_o + 4u * plane;
            CHECK(S.occ.offset == 0u && S.cls.offset == cls_o && S.psums.offset == psums_o && S.ptot.offset == ptot_o && S.evals.offset == evals_o);
            CHECK(S.ins.offset == ins_o && S.ov.offset == ins_o + plane && S.sup.offset == ins_o + 2u * plane && S.plt.offset == ins_o + 3u * plane);
            CHECK(S.plate.offset == plate_o && S.plate.bytes == 16u && S.bytes == plate_o + 16u);
            CHECK(S.occ.bytes == n && S.ins.bytes == (size_t)words * 8u && S.plt.bytes == (size_t)words * 8u);
            check_regions({span(S.occ), span(S.cls), span(S.psums), span(S.ptot), span(S.evals), span(S.ins), span(S.ov), span(S.sup), span(S.plt),
                           span(S.plate)},
                          S.bytes);
            // the planes hold every point, and at most two words where one would do (a 65th point along the bit axis)
            CHECK((size_t)words * 64u >= n && (size_t)words * 64u <= (size_t)n * 64u);
            if (f.nu % 64u == 0u) CHECK((size_t)words * 64u == n);  // then four planes are half a byte per point
            const rml::SupportProfile P(f.nh);
            CHECK(P.profile.offset == 0u && P.profile.bytes == (size_t)f.nh * 16u && P.extra.offset == a16((size_t)f.nh * 16u));
            CHECK(P.extra.bytes == (size_t)f.nh * 8u && P.bytes == P.extra.offset + a16((size_t)f.nh * 8u));
            check_regions({span(P.profile), span(P.extra)}, P.bytes);
        }
}

// the overhang tile: at most one word per thread, at most 64 rows, the halo of the widest disc on either side
void tiles() {
    CHECK(rml::kSupMaxReach * rml::kSupMaxReach <= rml::kSupMaxR2 && (rml::kSupMaxReach + 1u) * (rml::kSupMaxReach + 1u) > rml::kSupMaxR2);
    CHECK(rml::kSupMaxWords * 64u == 1024u);
    uint32_t worst = 0u;
    for (uint32_t nw = 1u; nw <= rml::kSupMaxWords; nw++) {
        const uint32_t tv = rml::sup_tile_rows(nw);
        CHECK(tv >= 1u && tv <= rml::kSupMaxRows && tv * nw <= 256u);
        CHECK(tv == rml::kSupMaxRows || (tv + 1u) * nw > 256u);
        for (uint32_t reach = 0u; reach <= rml::kSupMaxReach; reach++) {
            const rml::SupCoverLds L(tv, reach, nw);
            CHECK(L.rows == 0u && L.bytes == (tv + 2u * reach) * nw * 8u && L.bytes % 8u == 0u);
            worst = L.bytes > worst ? L.bytes : worst;
        }
    }
    CHECK(worst == (16u + 30u) * 16u * 8u && worst == 5888u && worst + 1024u <= rml::kLdsLaunchLimit);
    CHECK(rml::sup_tile_rows(1u) == 64u && rml::sup_tile_rows(4u) == 64u && rml::sup_tile_rows(5u) == 51u && rml::sup_tile_rows(16u) == 16u);
}

// every element the kernels touch, in real allocations of exactly `bytes` bytes (the sanitizer watches their ends)
void walk() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{65, 3, 2}, Lattice{3, 130, 2}, Lattice{2, 3, 70}})
        for (uint32_t axis = 0; axis < 3u; axis++)
            for (uint32_t neg = 0; neg < 2u; neg++) {
                const Frame f = frame(l, axis);
                const uint32_t n = l.nx * l.ny * l.nz, nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u), np = (nb + 255u) / 256u;
                const uint32_t words = f.nh * f.nv * f.nw, ncw = f.nv * f.nw;
                const rml::SupportScratch S(n, nb, np, words);
                std::vector<char> buf(S.bytes);
                char* b = buf.data();
                for (uint32_t p = 0; p < n; p++) S.occ.at(b)[p] = 0u;
                for (uint32_t k = 0; k < nb; k++) S.cls.at(b)[k] = 2u;
                for (uint32_t k = 0; k < np; k++) S.psums.at(b)[k] = k;
                for (int k = 0; k < 2; k++) S.ptot.at(b)[k] = S.evals.at(b)[k] = 0ull;
                for (int k = 0; k < 4; k++) S.plate.at(b)[k] = 0xFFFFFFFFu;
                for (uint32_t w = 0; w < words; w++) S.ins.at(b)[w] = S.ov.at(b)[w] = S.sup.at(b)[w] = S.plt.at(b)[w] = 0ull;
                // pack and compose: every bit of a plane is one point of the caller's array, and every point is one bit
                for (uint32_t h = 0; h < f.nh; h++)
                    for (uint32_t v = 0; v < f.nv; v++)
                        for (uint32_t w = 0; w < f.nw; w++)
                            for (uint32_t bit = 0; bit < 64u && w * 64u + bit < f.nu; bit++) {
                                const uint32_t hh = neg ? f.nh - 1u - h : h;
                                const uint32_t at = (w * 64u + bit) * f.su + v * f.sv + hh * f.sh;
                                CHECK(at < n);
                                S.occ.at(b)[at] += 1u;
                                S.ins.at(b)[(h * f.nv + v) * f.nw + w] |= 1ull << bit;
                            }
                for (uint32_t p = 0; p < n; p++) CHECK(S.occ.at(b)[p] == 1u);
                uint64_t bits = 0;
                for (uint32_t w = 0; w < words; w++) bits += (uint64_t)__builtin_popcountll(S.ins.at(b)[w]);
                CHECK(bits == n);
                // the overhang kernel's staging and its tile, for the narrowest and the widest disc
                const uint32_t tv = rml::sup_tile_rows(f.nw);
                for (uint32_t reach : {0u, 1u, rml::kSupMaxReach}) {
                    const rml::SupCoverLds L(tv, reach, f.nw);
                    std::vector<char> lds(L.bytes);
                    unsigned long long* rows = reinterpret_cast<unsigned long long*>(lds.data() + L.rows);
                    std::vector<uint32_t> written(words, 0u);
                    for (uint32_t h = 1; h < f.nh; h++)
                        for (uint32_t bx = 0; bx < (f.nv + tv - 1u) / tv; bx++) {
                            const uint32_t v0 = bx * tv, n_stage = (tv + 2u * reach) * f.nw;
                            for (uint32_t t = 0; t < 256u; t++)
                                for (uint32_t q = t; q < n_stage; q += 256u) {
                                    const uint32_t r = q / f.nw, c = q - r * f.nw;
                                    const int vv = (int)v0 - (int)reach + (int)r;
                                    rows[q] = vv >= 0 && vv < (int)f.nv ? S.ins.at(b)[(h - 1u) * ncw + (uint32_t)vv * f.nw + c] : 0ull;
                                }
                            for (uint32_t t = 0; t < 256u; t++) {
                                const uint32_t lv = t / f.nw, wu = t - lv * f.nw, v = v0 + lv;
                                if (lv >= tv || v >= f.nv) continue;
                                unsigned long long cover = 0ull;
                                for (uint32_t d = 0; d <= 2u * reach; d++) cover |= rows[(lv + d) * f.nw + wu];
                                written[h * ncw + v * f.nw + wu] += 1u + (uint32_t)(cover & 0ull);
                            }
                        }
                    for (uint32_t w = ncw; w < words; w++) CHECK(written[w] == 1u);  // every word above layer 0, once
                }
            }
}

}  // namespace

int main() {
    offsets();
    tiles();
    walk();
    std::printf("support layout ok (%d checks)\n", g_checks);
    return 0;
}
