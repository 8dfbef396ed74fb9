// trace_layout_check.cpp -- the scratch layout of rm_trace_rays' attribute pass (rml::TraceScratch in
// ray-marching_amd/csrc/rm_abi_layout.h) on the CPU, under ASan + UBSan (tests/test_trace_cpu.py).  Its regions lie in
// declaration order, start on 16-byte boundaries, do not overlap and end inside the total; every offset equals the chained
// align16 formula written out here; the list holds K entries per ray; the event copy exists only when asked for; and a walk
// over the regions as the kernels index them stays inside a real allocation of `bytes` bytes.
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

struct Pair { uint32_t x, y; };  // the kernels' uint2

void offsets() {
    static_assert(sizeof(Pair) == 8, "stand-in of the kernels' type");
    for (uint64_t n64 : {1ull, 65ull, 256ull, 257ull, 2001ull, (1ull << 32) - 1ull})
        for (uint32_t K : {1u, 2u, 8u, 64u})
            for (int own = 0; own < 2; own++) {
                const uint32_t n = (uint32_t)n64, nb = (uint32_t)((n64 + 255u) / 256u);
                const rml::TraceScratch<Pair> S(n, nb, K, own != 0);
                const size_t sums_o = a16((size_t)n * 4u), totals_o = sums_o + a16((size_t)nb * 8u), list_o = totals_o + 16u,
                             events_o = list_o + a16((size_t)n * K * 8u), bytes = events_o + (own ? a16((size_t)n * K * 32u) : 0u);
                CHECK(S.stored.offset == 0u && S.sums.offset == sums_o && S.totals.offset == totals_o && S.list.offset == list_o &&
                      S.events.offset == events_o);
                CHECK(S.stored.bytes == (size_t)n * 4u && S.sums.bytes == (size_t)nb * 8u && S.totals.bytes == 16u);
                CHECK(S.list.bytes == (size_t)n * K * 8u);
                CHECK(S.events.bytes == (own ? (size_t)n * K * 32u : 0u));
                CHECK(S.bytes == bytes);
                check_regions({span(S.stored), span(S.sums), span(S.totals), span(S.list), span(S.events)}, S.bytes);
            }
}

// every element the kernels touch, in a real allocation of exactly `bytes` bytes (the sanitizer watches its ends)
void walk() {
    for (uint32_t n : {1u, 65u, 257u})
        for (uint32_t K : {1u, 5u, 64u}) {
            const uint32_t nb = (n + 255u) / 256u;
            const rml::TraceScratch<Pair> S(n, nb, K, true);
            std::vector<char> buf(S.bytes);
            for (uint32_t i = 0; i < n; i++) S.stored.at(buf.data())[i] = K;
            for (uint32_t b = 0; b < nb; b++) S.sums.at(buf.data())[b] = (unsigned long long)b * 256u * K;
            for (int k = 0; k < 4; k++) S.totals.at(buf.data())[k] = 0u;
            for (size_t e = 0; e < (size_t)n * K; e++) {
                S.list.at(buf.data())[e] = Pair{(uint32_t)(e / K), (uint32_t)(e % K)};
                for (int k = 0; k < 8; k++) S.events.at(buf.data())[8u * e + k] = 0.0f;
            }
            CHECK(S.list.at(buf.data())[(size_t)n * K - 1u].x == n - 1u);
        }
}

}  // namespace

int main() {
    offsets();
    walk();
    std::printf("trace layout ok (%d checks)\n", g_checks);
    return 0;
}
