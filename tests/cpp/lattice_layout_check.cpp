// lattice_layout_check.cpp -- the lattice draw on the CPU, under ASan + UBSan (tests/test_lattice_draw_cpu.py): the retained slot
// rml::LatticeSlot (ray-marching_amd/csrc/rm_abi_layout.h) against offsets written out by hand; the build kernel's indexing --
// restated here word by word -- inside real allocations of exactly the described sizes; and the traversal itself, the functions
// of rm_lattice_walk.h that the kernels run: the one that jumps over empty bricks against the one that visits every cell, record
// for record, on random and degenerate rays, every read inside those allocations.
//
//   lattice_layout_check                 the checks above
//   lattice_layout_check walk IN OUT     the jumping traversal (plain IN OUT: the one without jumps) of the rays in file IN, five u32 words a ray to file OUT (hit, the
//                                        bits of t, axis, up, linear index), for the comparison with the numpy restatement.
//                                        IN: u32 nx, ny, nz, window[6], n; f32 origin[3], step[3]; nx ny nz class bytes; n x 6 f32.
#include "rm_abi_layout.h"
#include "rm_lattice_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <random>
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

void offsets() {
    struct Case { uint32_t nx, ny, nz; };
    for (const Case& c : {Case{2, 2, 2}, Case{3, 5, 7}, Case{9, 8, 7}, Case{65, 33, 17}, Case{1024, 2, 2}, Case{2, 1024, 2}, Case{2, 2, 1024},
                          Case{1024, 512, 512}, Case{31, 3, 1024}}) {
        const rml::LatticeSlot S(c.nx, c.ny, c.nz);
        const size_t n = (size_t)c.nx * c.ny * c.nz, W = (c.nx + 31u) / 32u;
        const size_t nb = (size_t)((c.nx + 7u) / 8u) * ((c.ny + 7u) / 8u) * ((c.nz + 7u) / 8u);
        CHECK(rml::lat_row_words(c.nx) == W && rml::lat_bricks(c.nx) == (c.nx + 7u) / 8u);
        const size_t bits_o = a16(n), bricks_o = bits_o + a16((size_t)c.ny * c.nz * W * 4u), counters_o = bricks_o + a16((nb + 31u) / 32u * 4u);
        CHECK(S.classes.offset == 0u && S.classes.bytes == n);
        CHECK(S.bits.offset == bits_o && S.bits.bytes == (size_t)c.ny * c.nz * W * 4u);
        CHECK(S.bricks.offset == bricks_o && S.bricks.bytes == (nb + 31u) / 32u * 4u);
        CHECK(S.counters.offset == counters_o && S.counters.bytes == 16u && S.bytes == counters_o + 16u);
        CHECK(S.clear_offset() == bricks_o && S.clear_offset() + S.clear_bytes() == S.bytes);  // one memset: bricks and counters
        CHECK(nb <= (1u << 19) || n > (1u << 28));                                          // 64 KiB of brick bits at the most
    }
}

// A lattice in allocations of exactly the slot's region sizes: what rm_lat_pack_kernel writes, one "lane" per word.
struct Lattice {
    uint32_t nx, ny, nz;
    std::vector<uint8_t> cls;
    std::vector<uint32_t> bits, bricks;
    uint64_t points = 0, n_bricks = 0;
    Lattice(uint32_t nx_, uint32_t ny_, uint32_t nz_, std::vector<uint8_t> bytes) : nx(nx_), ny(ny_), nz(nz_), cls(std::move(bytes)) {
        const rml::LatticeSlot S(nx, ny, nz);
        CHECK(cls.size() == S.classes.bytes);
        bits.assign(S.bits.bytes / 4u, 0xFFFFFFFFu);
        bricks.assign(S.bricks.bytes / 4u, 0u);
        const uint32_t row_words = rml::lat_row_words(nx), n_words = ny * nz * row_words, bx = rml::lat_bricks(nx), by = rml::lat_bricks(ny);
        for (uint32_t w = 0; w < n_words; w++) {
            const uint32_t row = w / row_words, x0 = (w - row * row_words) * 32u;
            const uint32_t count = nx - x0 < 32u ? nx - x0 : 32u;
            uint32_t word = 0u;
            for (uint32_t x = 0; x < count; x++) word |= (cls.at((size_t)row * nx + x0 + x) != 0u ? 1u : 0u) << x;
            bits.at(w) = word;
            points += (uint32_t)__builtin_popcount(word);
            if (word == 0u) continue;
            const uint32_t j = row % ny, k = row / ny, base = ((k >> 3) * by + (j >> 3)) * bx + (x0 >> 3);
            for (uint32_t q = 0; q < 4u; q++) {
                if (((word >> (8u * q)) & 0xFFu) == 0u) continue;
                const uint32_t b = base + q, bit = 1u << (b & 31u);
                if ((bricks.at(b >> 5) & bit) == 0u) n_bricks++;
                bricks.at(b >> 5) |= bit;
            }
        }
    }
    rmk::LatGrid grid(const float* origin, const float* step, const uint32_t* window) const {
        rmk::LatGrid G{};
        G.ox = origin[0]; G.oy = origin[1]; G.oz = origin[2];
        G.sx = step[0]; G.sy = step[1]; G.sz = step[2];
        G.nx = nx; G.ny = ny; G.nz = nz;
        G.row_words = rml::lat_row_words(nx);
        G.bx = rml::lat_bricks(nx); G.by = rml::lat_bricks(ny);
        G.lox = window ? window[0] : 0u; G.loy = window ? window[1] : 0u; G.loz = window ? window[2] : 0u;
        G.hix = window ? window[3] : nx; G.hiy = window ? window[4] : ny; G.hiz = window ? window[5] : nz;
        G.cls = cls.data(); G.bits = bits.data(); G.bricks = bricks.data();
        G.materials = nullptr; G.n_materials = 0u;
        return G;
    }
};

// The words against the definition: a point's bit, a brick's bit, the two counts.
void pack(const Lattice& L) {
    const uint32_t bx = rml::lat_bricks(L.nx), by = rml::lat_bricks(L.ny), bz = rml::lat_bricks(L.nz), W = rml::lat_row_words(L.nx);
    std::vector<uint8_t> brick((size_t)bx * by * bz, 0);
    uint64_t points = 0;
    for (uint32_t k = 0; k < L.nz; k++)
        for (uint32_t j = 0; j < L.ny; j++)
            for (uint32_t i = 0; i < L.nx; i++) {
                const bool full = L.cls[i + (size_t)L.nx * (j + (size_t)L.ny * k)] != 0u;
                CHECK(((L.bits[(size_t)(k * L.ny + j) * W + (i >> 5)] >> (i & 31u)) & 1u) == (full ? 1u : 0u));
                if (full) { points++; brick[((size_t)(k >> 3) * by + (j >> 3)) * bx + (i >> 3)] = 1; }
            }
    uint64_t n_bricks = 0;
    for (size_t b = 0; b < brick.size(); b++) {
        CHECK(((L.bricks[b >> 5] >> (b & 31u)) & 1u) == brick[b]);
        n_bricks += brick[b];
    }
    for (uint32_t w = 0; w < L.ny * L.nz * W; w++)  // no bit beyond a row's end
        if ((w % W) == W - 1u && (L.nx & 31u)) CHECK((L.bits[w] >> (L.nx & 31u)) == 0u);
    CHECK(points == L.points && n_bricks == L.n_bricks);
}

bool same(const rmk::LatRecord& a, const rmk::LatRecord& b) {
    if (a.hit != b.hit) return false;
    if (!a.hit) return true;
    uint32_t ta, tb;
    std::memcpy(&ta, &a.t, 4); std::memcpy(&tb, &b.t, 4);
    return ta == tb && a.axis == b.axis && a.index == b.index && (a.axis == 3u || a.up == b.up);
}

std::vector<uint8_t> contents(uint32_t nx, uint32_t ny, uint32_t nz, int kind, std::mt19937& rng) {
    std::vector<uint8_t> c((size_t)nx * ny * nz, 0);
    auto at = [&](uint32_t i, uint32_t j, uint32_t k) -> uint8_t& { return c[i + (size_t)nx * (j + (size_t)ny * k)]; };
    if (kind == 0) return c;                                                          // empty
    if (kind == 1) { for (auto& v : c) v = 1 + rng() % 255; return c; }               // full
    if (kind == 2) { at(0, 0, 0) = 1; at(nx - 1, ny - 1, nz - 1) = 255; return c; }   // corners
    if (kind == 3) { for (auto& v : c) v = rng() % 10u == 0u ? 1 + rng() % 255 : 0; return c; }  // 10 % sparse
    if (kind == 4) {                                                                   // one point per brick
        for (uint32_t k = 0; k < nz; k += 8) for (uint32_t j = 0; j < ny; j += 8) for (uint32_t i = 0; i < nx; i += 8)
            at(std::min(nx - 1u, i + (uint32_t)(rng() % 8u)), std::min(ny - 1u, j + (uint32_t)(rng() % 8u)), std::min(nz - 1u, k + (uint32_t)(rng() % 8u))) = 7;
        return c;
    }
    for (auto& v : c) v = 3;                                                           // solid, one empty brick inside
    for (uint32_t k = 8; k < std::min(nz, 16u); k++) for (uint32_t j = 8; j < std::min(ny, 16u); j++) for (uint32_t i = 8; i < std::min(nx, 16u); i++) at(i, j, k) = 0;
    return c;
}

void traversal() {
    std::mt19937 rng(28);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    struct Shape { uint32_t nx, ny, nz; };
    uint64_t rays = 0, hits = 0;
    for (const Shape& sh : {Shape{2, 2, 2}, Shape{3, 5, 7}, Shape{9, 8, 7}, Shape{17, 16, 15}, Shape{40, 33, 17}, Shape{130, 2, 2}, Shape{2, 2, 130}}) {
        for (int kind = 0; kind < 6; kind++) {
            const Lattice L(sh.nx, sh.ny, sh.nz, contents(sh.nx, sh.ny, sh.nz, kind, rng));
            pack(L);
            const float origin[3] = {-1.25f, 0.5f, 2.0f}, step[3] = {0.25f, 0.5f, 0.375f};
            const float n[3] = {(float)sh.nx, (float)sh.ny, (float)sh.nz};
            for (int win = 0; win < 2; win++) {
                uint32_t w[6] = {0, 0, 0, sh.nx, sh.ny, sh.nz};
                if (win) for (int a = 0; a < 3; a++) { w[a] = rng() % (w[3 + a] - 1u); w[3 + a] = w[a] + 1u + rng() % (w[3 + a] - w[a]); }
                const rmk::LatGrid G = L.grid(origin, step, w);
                for (int r = 0; r < 600; r++) {
                    float O[3], D[3];
                    const int mode = r % 6;
                    for (int a = 0; a < 3; a++) {
                        const float lo = origin[a] - 0.5f * step[a], len = n[a] * step[a];
                        O[a] = mode == 0 ? lo + len * U(rng)                       // inside the box
                                         : lo + len * (3.0f * U(rng) - 1.0f);      // around it
                        D[a] = (r / 6) % 3 ? (lo + len * U(rng)) - O[a] : 2.0f * U(rng) - 1.0f;  // two in three aim at the box
                    }
                    if (mode == 2) D[rng() % 3] = 0.0f;                            // parallel to an axis plane
                    if (mode == 3) { D[rng() % 3] = 0.0f; D[rng() % 3] = 0.0f; }   // axis-parallel
                    if (mode == 4) {                                               // through lattice vertices: ties at every step
                        for (int a = 0; a < 3; a++) { O[a] = origin[a] + ((float)(rng() % 4) - 2.5f) * step[a]; D[a] = (r & (8 << a) ? -1.0f : 1.0f) * step[a]; }
                    }
                    if (mode == 5) {                                               // in a plane between cells; tiny and huge components
                        const int a = rng() % 3;
                        O[a] = origin[a] + ((float)(rng() % sh.nx) - 0.5f) * step[a];
                        D[(a + 1) % 3] = r & 8 ? 1e-30f : std::numeric_limits<float>::denorm_min();
                        if (r & 16) O[(a + 2) % 3] = 1e8f;
                    }
                    const rmk::LatRecord a = rmk::lat_traverse<true>(G, O[0], O[1], O[2], D[0], D[1], D[2]);
                    const rmk::LatRecord b = rmk::lat_traverse<false>(G, O[0], O[1], O[2], D[0], D[1], D[2]);
                    if (!same(a, b)) {
                        std::fprintf(stderr, "lattice %ux%ux%u kind %d window %d ray %d (%a %a %a | %a %a %a): jump (%d %a %u %u) walk (%d %a %u %u)\n", sh.nx,
                                     sh.ny, sh.nz, kind, win, r, O[0], O[1], O[2], D[0], D[1], D[2], a.hit, a.t, a.axis, a.index, b.hit, b.t, b.axis, b.index);
                        std::exit(1);
                    }
                    g_checks++;
                    rays++;
                    hits += a.hit;
                }
            }
        }
    }
    std::printf("%llu rays, %llu hits\n", (unsigned long long)rays, (unsigned long long)hits);
    CHECK(hits > rays / 10u && hits < rays);  // the comparison saw both outcomes
    // non-finite components miss, whatever the lattice holds
    const Lattice L(4, 4, 4, std::vector<uint8_t>(64, 1));
    const float origin[3] = {0, 0, 0}, step[3] = {1, 1, 1};
    const rmk::LatGrid G = L.grid(origin, step, nullptr);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float bad : {nan, inf, -inf}) {
        CHECK(!rmk::lat_traverse<true>(G, bad, 1, 1, 1, 0, 0).hit && !rmk::lat_traverse<true>(G, -2, 1, 1, bad, 0, 0).hit);
        CHECK(!rmk::lat_traverse<true>(G, 1, 1, bad, 0, 0, 1).hit && !rmk::lat_traverse<true>(G, 1, 1, -2, 0, bad, 1).hit);
    }
    CHECK(rmk::lat_traverse<true>(G, 1, 1, 1, 0, 0, 0).hit && rmk::lat_traverse<true>(G, 1, 1, 1, 0, 0, 0).axis == 3u);  // a zero direction inside
    CHECK(!rmk::lat_traverse<true>(G, 9, 1, 1, 0, 0, 0).hit);
}

int walk_file(const char* in, const char* out, bool jumps) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    uint32_t head[10];
    float os[6];
    if (std::fread(head, 4, 10, f) != 10 || std::fread(os, 4, 6, f) != 6) return 2;
    const uint32_t nx = head[0], ny = head[1], nz = head[2], n = head[9];
    std::vector<uint8_t> bytes((size_t)nx * ny * nz);
    std::vector<float> rays((size_t)n * 6u);
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size() || std::fread(rays.data(), 4, rays.size(), f) != rays.size()) return 2;
    std::fclose(f);
    const Lattice L(nx, ny, nz, bytes);
    const rmk::LatGrid G = L.grid(os, os + 3, head + 3);
    std::vector<uint32_t> rec((size_t)n * 5u);
    for (uint32_t i = 0; i < n; i++) {
        const float* r = &rays[6u * i];
        const rmk::LatRecord a = jumps ? rmk::lat_traverse<true>(G, r[0], r[1], r[2], r[3], r[4], r[5]) : rmk::lat_traverse<false>(G, r[0], r[1], r[2], r[3], r[4], r[5]);
        uint32_t t;
        std::memcpy(&t, &a.t, 4);
        rec[5u * i] = a.hit; rec[5u * i + 1u] = t; rec[5u * i + 2u] = a.axis; rec[5u * i + 3u] = a.up; rec[5u * i + 4u] = a.index;
    }
    f = std::fopen(out, "wb");
    if (!f || std::fwrite(rec.data(), 4, rec.size(), f) != rec.size()) return 2;
    std::fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "walk") == 0) return walk_file(argv[2], argv[3], true);
    if (argc == 4 && std::strcmp(argv[1], "plain") == 0) return walk_file(argv[2], argv[3], false);
    offsets();
    traversal();
    std::printf("lattice layout ok (%d checks)\n", g_checks);
    return 0;
}
