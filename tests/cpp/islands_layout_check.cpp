// islands_layout_check.cpp -- the layouts of rm_islands_solid / rm_islands_occupancy on the CPU, under ASan + UBSan
// (tests/test_islands_cpu.py): rml::IslandsScratch and rml::IslandsRows (ray-marching_amd/csrc/rm_abi_layout.h), the labelling
// tile rml::IslTileLds and the links tile rml::IslLinkLds (rm_lds_layout.h).  The regions lie in declaration order, start on
// 16-byte boundaries, do not overlap and end inside the total; every offset equals the chained align16 formula written out here;
// a walk over the tiles as the kernels index them, for all three frames, stays inside real allocations of `bytes` bytes and
// visits every point exactly once; and within a layer the canonical order (v, then u) is the order of the caller's linear index
// in all six directions, which is what makes numbering the roots in canonical order number the regions by (h, FIRST).
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

// the canonical frame of rm_abi.hip's sup_frame, written out again
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
            const uint32_t words = f.nh * f.nv * f.nw, nr = (n + 255u) / 256u;
            const rml::IslandsScratch S(n, nb, np, words, nr, f.nh);
            const size_t cls_o = a16(n), psums_o = cls_o + a16(nb), ptot_o = psums_o + a16((size_t)np * 8u), evals_o = ptot_o + 16u,
                         ins_o = evals_o + 16u, plane = a16((size_t)words * 8u), parent_o = ins_o + 2u * plane, vol = a16((size_t)n * 4u),
                         rsums_o = parent_o + 2u * vol, rtot_o = rsums_o + a16((size_t)nr * 8u), lbase_o = rtot_o + 16u,
                         plate_o = lbase_o + a16(((size_t)f.nh + 1u) * 4u);
            CHECK(S.occ.offset == 0u && S.cls.offset == cls_o && S.psums.offset == psums_o && S.ptot.offset == ptot_o && S.evals.offset == evals_o);
            CHECK(S.ins.offset == ins_o && S.ov.offset == ins_o + plane && S.parent.offset == parent_o && S.lab.offset == parent_o + vol);
            CHECK(S.rsums.offset == rsums_o && S.rtot.offset == rtot_o && S.lbase.offset == lbase_o && S.plate.offset == plate_o);
            CHECK(S.totals.offset == plate_o + 16u && S.bytes == plate_o + 32u);
            CHECK(S.occ.bytes == n && S.ins.bytes == (size_t)words * 8u && S.parent.bytes == (size_t)n * 4u && S.lab.bytes == (size_t)n * 4u);
            check_regions({span(S.occ), span(S.cls), span(S.psums), span(S.ptot), span(S.evals), span(S.ins), span(S.ov), span(S.parent),
                           span(S.lab), span(S.rsums), span(S.rtot), span(S.lbase), span(S.plate), span(S.totals)},
                          S.bytes);
        }
    CHECK(rml::kIslRowWords == 12u);
    for (uint64_t regions : {0ull, 1ull, 3ull, 297ull, 1ull << 27}) {
        const rml::IslandsRows T(regions);
        CHECK(T.rows.offset == 0u && T.rows.bytes == regions * 48u && T.bytes == a16(regions * 48u));
    }
}

void tiles() {
    constexpr rml::IslTileLds T;
    CHECK(rml::kIslTile == 64u && T.words == 0u && T.parent == 512u && T.bytes == 512u + 64u * 64u * 4u && T.bytes == 16896u);
    CHECK(T.parent % 16u == 0u && T.bytes + 1024u <= rml::kLdsLaunchLimit);
    uint32_t worst = 0u;
    for (uint32_t reach = 0u; reach <= rml::kSupMaxReach; reach++) {
        const rml::IslLinkLds L(reach);
        CHECK(L.labels == 0u && L.pitch == 64u + 2u * reach && L.rows == rml::kIslLinkRows + 2u * reach && L.bytes == L.rows * L.pitch * 4u);
        worst = L.bytes > worst ? L.bytes : worst;
    }
    CHECK(rml::kIslLinkRows == 16u && worst == 46u * 94u * 4u && worst == 17296u && worst + 1024u <= rml::kLdsLaunchLimit);
}

// every element the kernels touch, in real allocations of exactly `bytes` bytes (the sanitizer watches their ends)
void walk() {
    for (const Lattice& l : {Lattice{2, 2, 2}, Lattice{9, 17, 10}, Lattice{33, 20, 17}, Lattice{65, 3, 2}, Lattice{3, 130, 2}, Lattice{2, 3, 70},
                             Lattice{66, 67, 3}})
        for (uint32_t axis = 0; axis < 3u; axis++)
            for (uint32_t neg = 0; neg < 2u; neg++) {
                const Frame f = frame(l, axis);
                const uint32_t n = l.nx * l.ny * l.nz, nb = ((l.nx + 7u) / 8u) * ((l.ny + 7u) / 8u) * ((l.nz + 7u) / 8u), np = (nb + 255u) / 256u;
                const uint32_t words = f.nh * f.nv * f.nw, nr = (n + 255u) / 256u;
                const rml::IslandsScratch S(n, nb, np, words, nr, f.nh);
                std::vector<char> buf(S.bytes);
                char* b = buf.data();
                for (uint32_t k = 0; k < nr; k++) S.rsums.at(b)[k] = k;
                for (uint32_t k = 0; k <= f.nh; k++) S.lbase.at(b)[k] = k;
                for (int k = 0; k < 4; k++) S.plate.at(b)[k] = S.totals.at(b)[k] = 0u;
                for (int k = 0; k < 2; k++) S.rtot.at(b)[k] = 0ull;
                for (uint32_t p = 0; p < n; p++) S.parent.at(b)[p] = S.lab.at(b)[p] = 0u;
                // the canonical index p = (h nv + v) nu + u names every point of the caller's array once, and within a layer
                // it grows with the caller's linear index
                std::vector<uint32_t> seen(n, 0u);
                for (uint32_t h = 0; h < f.nh; h++) {
                    uint32_t last = 0u;
                    for (uint32_t v = 0; v < f.nv; v++)
                        for (uint32_t u = 0; u < f.nu; u++) {
                            const uint32_t p = (h * f.nv + v) * f.nu + u, hh = neg ? f.nh - 1u - h : h;
                            const uint32_t at = u * f.su + v * f.sv + hh * f.sh;
                            CHECK(p < n && at < n);
                            seen[at]++;
                            CHECK((v == 0u && u == 0u) || at > last);
                            last = at;
                            // ... and the compose kernel's way back from the caller's point
                            const uint32_t i = at % l.nx, r = at / l.nx, j = r % l.ny, k = r / l.ny;
                            const uint32_t cu = axis == 0u ? j : i, cv = axis == 2u ? j : k, ch = axis == 0u ? i : axis == 1u ? j : k;
                            CHECK(cu == u && cv == v && (neg ? f.nh - 1u - ch : ch) == h);
                        }
                }
                for (uint32_t p = 0; p < n; p++) CHECK(seen[p] == 1u);
                // the labelling tile: lane `lane` of workgroup (w, tile, h) holds row 64 tile + lane; row r, bit b writes one parent
                {
                    constexpr rml::IslTileLds T;
                    std::vector<char> lds(T.bytes);
                    unsigned long long* s_word = reinterpret_cast<unsigned long long*>(lds.data() + T.words);
                    uint32_t* s_par = reinterpret_cast<uint32_t*>(lds.data() + T.parent);
                    for (uint32_t h = 0; h < f.nh; h++)
                        for (uint32_t tile = 0; tile < (f.nv + 63u) / 64u; tile++)
                            for (uint32_t w = 0; w < f.nw; w++) {
                                for (uint32_t lane = 0; lane < 64u; lane++) {
                                    s_word[lane] = tile * 64u + lane < f.nv ? ~0ull >> (w * 64u + 64u <= f.nu ? 0u : 64u - (f.nu - w * 64u)) : 0ull;
                                    for (uint32_t bit = 0; bit < 64u; bit++) s_par[lane * 64u + bit] = lane * 64u + bit;
                                }
                                for (uint32_t r = 0; r < 64u; r++)
                                    for (uint32_t lane = 0; lane < 64u; lane++) {
                                        if (((s_word[r] >> lane) & 1ull) == 0ull) continue;
                                        const uint32_t p = (h * f.nv + tile * 64u + r) * f.nu + w * 64u + lane;
                                        CHECK(p < n);
                                        S.parent.at(b)[p] += 1u;
                                    }
                            }
                    for (uint32_t p = 0; p < n; p++) CHECK(S.parent.at(b)[p] == 1u);
                }
                // the links tile: staging and the gather of the widest and the narrowest disc stay inside the tile, and the tiles
                // of a layer visit every point above layer 0 once
                for (uint32_t reach : {0u, 1u, rml::kSupMaxReach}) {
                    const rml::IslLinkLds L(reach);
                    std::vector<char> lds(L.bytes);
                    uint32_t* s_lab = reinterpret_cast<uint32_t*>(lds.data() + L.labels);
                    for (uint32_t p = 0; p < n; p++) S.lab.at(b)[p] = 0u;
                    for (uint32_t h = 1; h < f.nh; h++)
                        for (uint32_t bv = 0; bv < (f.nv + rml::kIslLinkRows - 1u) / rml::kIslLinkRows; bv++)
                            for (uint32_t w = 0; w < f.nw; w++) {
                                const int u0 = (int)(w * 64u) - (int)reach, vb = (int)(bv * rml::kIslLinkRows) - (int)reach;
                                for (uint32_t q = 0; q < L.rows * L.pitch; q++) {
                                    const uint32_t rr = q / L.pitch, cc = q - rr * L.pitch;
                                    const int vv = vb + (int)rr, uu = u0 + (int)cc;
                                    const bool in = vv >= 0 && vv < (int)f.nv && uu >= 0 && uu < (int)f.nu;
                                    if (in) CHECK(((h - 1u) * f.nv + (uint32_t)vv) * f.nu + (uint32_t)uu < n);
                                    s_lab[q] = in ? 1u : 0u;
                                }
                                for (uint32_t t = 0; t < 256u; t++)
                                    for (uint32_t lv = t >> 6; lv < rml::kIslLinkRows; lv += 4u) {
                                        const uint32_t lu = t & 63u, v = bv * rml::kIslLinkRows + lv, u = w * 64u + lu;
                                        if (v >= f.nv || u >= f.nu) continue;
                                        uint32_t found = 0u;
                                        for (uint32_t d = 0; d <= 2u * reach; d++) {
                                            const uint32_t* row = s_lab + (lv + d) * L.pitch + lu + reach;
                                            for (int du = -(int)reach; du <= (int)reach; du++) found += row[du];
                                        }
                                        CHECK(found >= 1u);  // (at least the point directly below)
                                        S.lab.at(b)[(h * f.nv + v) * f.nu + u] += 1u;
                                    }
                            }
                    for (uint32_t p = f.nv * f.nu; p < n; p++) CHECK(S.lab.at(b)[p] == 1u);
                }
            }
}

}  // namespace

int main() {
    offsets();
    tiles();
    walk();
    std::printf("islands layout ok (%d checks)\n", g_checks);
    return 0;
}
