// hatch_layout_check.cpp -- the layouts and the index arithmetic of rm_hatch_slices on the CPU, under ASan + UBSan
// (tests/test_hatch_cpu.py): rml::HatchScratch, rml::HatchItems and rml::HatchSlot (ray-marching_amd/csrc/rm_abi_layout.h) lie in
// declaration order on 16-byte boundaries, without overlap, at the chained align16 offsets written out here; the host's bounds
// (2^32 crossings, the sort key's bits) answer as the contract says; and the count, scan, items, pair and emit kernels of
// rm_hatch.h, restated thread by thread with their blocks, passes and binary searches, stay inside real allocations of exactly the
// described sizes, write every output slot once and give what a plain per-line walk gives.
#include "rm_abi_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
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
    static_assert(rml::kHatchMaxLines == 1u << 24, "j is exact in binary32 and j * spacing in binary64");
    for (uint32_t P : {0u, 1u, 1023u, 1024u, 1025u, 2400000u, 0xFFFFFFFFu})
        for (uint32_t nl : {1u, 300u, 65536u}) {
            const rml::HatchScratch S(P, nl);
            const uint32_t pb = (uint32_t)(((uint64_t)P + 1023u) / 1024u);
            const size_t cstart_o = a16((size_t)nl * 16u), j0_o = cstart_o + a16(((size_t)P + 1u) * 4u), bsums_o = j0_o + a16((size_t)P * 4u),
                         btot_o = bsums_o + a16((size_t)pb * 8u), rows_o = btot_o + 16u, folded_o = rows_o + (size_t)pb * 128u,
                         result_o = folded_o + (size_t)((pb + 255u) / 256u) * 128u;
            CHECK(S.lines.offset == 0u && S.cstart.offset == cstart_o && S.j0.offset == j0_o && S.bsums.offset == bsums_o && S.btot.offset == btot_o);
            CHECK(S.rows.offset == rows_o && S.folded.offset == folded_o && S.result.offset == result_o && S.bytes == result_o + 128u);
            check_regions({span(S.lines), span(S.cstart), span(S.j0), span(S.bsums), span(S.btot), span(S.rows), span(S.folded), span(S.result)}, S.bytes);
        }
    for (uint32_t N : {1u, 1023u, 1024u, 1025u, 70000u, 0xFFFFFFFFu}) {
        const rml::HatchItems I(N);
        const uint32_t nb = (uint32_t)(((uint64_t)N + 1023u) / 1024u);
        const size_t ivals_o = a16((size_t)N * 8u), xs_o = ivals_o + a16((size_t)N * 4u), hstart_o = xs_o + a16((size_t)N * 8u),
                     bsums_o = hstart_o + a16(((size_t)N + 1u) * 4u), btot_o = bsums_o + a16((size_t)nb * 8u), rows_o = btot_o + 16u,
                     folded_o = rows_o + (size_t)nb * 128u, result_o = folded_o + (size_t)((nb + 255u) / 256u) * 128u;
        CHECK(I.ikeys.offset == 0u && I.ivals.offset == ivals_o && I.xs.offset == xs_o && I.hstart.offset == hstart_o && I.bsums.offset == bsums_o);
        CHECK(I.btot.offset == btot_o && I.rows.offset == rows_o && I.folded.offset == folded_o && I.result.offset == result_o);
        CHECK(I.sort == result_o + 128u && I.bytes == I.sort + rml::SortScratch(N).bytes);
        check_regions({span(I.ikeys), span(I.ivals), span(I.xs), span(I.hstart), span(I.bsums), span(I.btot), span(I.rows), span(I.folded),
                       span(I.result)}, I.sort);
    }
    for (uint64_t H : {0ull, 1ull, 5ull, 1ull << 31})
        for (uint32_t nl : {1u, 4u, 65536u}) {
            const rml::HatchSlot T(H, nl);
            const size_t line_o = a16((size_t)H * 16u), lf_o = line_o + a16((size_t)H * 4u);
            CHECK(T.segments.offset == 0u && T.line.offset == line_o && T.layer_first.offset == lf_o && T.bytes == lf_o + a16(((size_t)nl + 1u) * 4u));
            check_regions({span(T.segments), span(T.line), span(T.layer_first)}, T.bytes);
        }
}

// The host's bounds.  The count pass's block sums are 64-bit numbers; rm_block_scan_kernel adds their halves up separately.
void bounds() {
    CHECK(rml::hatch_crossings_fit(0u, 0u) && rml::hatch_crossings_fit(0xFFFFFFFFull, 0u));
    CHECK(!rml::hatch_crossings_fit(1ull << 32, 0u));       // many blocks whose low halves add up to 2^32
    CHECK(!rml::hatch_crossings_fit(0u, 1u));               // one block of 1024 segments of 2^22 crossings each: its sum is 2^32
    CHECK(!rml::hatch_crossings_fit(5u, 3u) && !rml::hatch_crossings_fit(1ull << 53, 1ull << 20));
    {   // the halves of the block sums of 4 blocks of 1024 segments crossing 2^24 lines each
        unsigned long long lo = 0, hi = 0;
        for (int b = 0; b < 4; b++) {
            const unsigned long long sum = 1024ull << 24;
            lo += sum & 0xFFFFFFFFull, hi += sum >> 32;
        }
        CHECK(lo == 0u && hi == 16u && !rml::hatch_crossings_fit(lo, hi));
    }
    CHECK(rml::hatch_key_bits(1u) == 32u && rml::hatch_key_bits(2u) == 33u && rml::hatch_key_bits(3u) == 34u && rml::hatch_key_bits(256u) == 40u);
    CHECK(rml::hatch_key_bits(90000u) == 49u && rml::hatch_key_bits(1ull << 16) == 48u && rml::hatch_key_bits((1ull << 16) + 1u) == 49u);
    CHECK(rml::hatch_key_bits(1ull << 32) == 64u && rml::sort_passes(rml::hatch_key_bits(90000u)) == 7u);
}

// ---- the kernels of rm_hatch.h, thread by thread -----------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };  // a contour record: first point, count, layer, closed
struct Frame { uint32_t u, v, n_points, n_contours, n_lines; };

uint32_t contour_of(const U4* contours, uint32_t n, uint32_t i) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        CHECK(mid < n);
        if (contours[mid].x > i) hi = mid;
        else lo = mid + 1u;
    }
    CHECK(lo >= 1u);
    return lo - 1u;
}
double s_of(const float* p, const Frame& f, double dx, double dy) { return (double)p[f.v] * dx - (double)p[f.u] * dy; }
double c_of(uint32_t j, double offset, double spacing) { return offset + (double)j * spacing; }
uint32_t lower(double s, double offset, double spacing, uint32_t n_lines) {
    uint32_t lo = 0u, hi = n_lines;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (c_of(mid, offset, spacing) >= s) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
struct Seg { uint32_t layer, a, b; double sa, sb, dx, dy, offset, spacing; };
bool segment(const Frame& f, const float* points, const U4* contours, const float* lines, uint32_t i, Seg& g) {
    const U4 c = contours[contour_of(contours, f.n_contours, i)];
    const uint32_t at = i - c.x;
    CHECK(at < c.y);
    if (c.w == 0u && at + 1u >= c.y) return false;
    const uint32_t h = c.x + (at + 1u == c.y ? 0u : at + 1u);
    CHECK(h < f.n_points);
    const float* l = lines + (size_t)c.z * 4u;
    g.layer = c.z, g.dx = l[0], g.dy = l[1], g.offset = l[2], g.spacing = l[3];
    const double st = s_of(points + (size_t)i * 3u, f, g.dx, g.dy), sh = s_of(points + (size_t)h * 3u, f, g.dx, g.dy);
    const bool tail_first = st < sh;
    g.a = tail_first ? i : h, g.b = tail_first ? h : i, g.sa = tail_first ? st : sh, g.sb = tail_first ? sh : st;
    return true;
}
uint32_t item_segment(const uint32_t* cstart, uint32_t n, uint32_t i) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cstart[mid] > i) hi = mid;
        else lo = mid + 1u;
    }
    CHECK(lo >= 1u);
    return lo - 1u;
}
uint32_t key_lower(const unsigned long long* keys, uint32_t n, unsigned long long x) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] >= x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
uint32_t key32(float r) {
    uint32_t b;
    std::memcpy(&b, &r, 4);
    return b ^ ((b >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u);
}

// rm_block_scan_kernel and rm_mslice_scan_kernel on block sums of 1024 entries: start[] in place, start[n] = the total.
void scan_in_place(uint32_t* start, uint32_t n, unsigned long long* bsums, uint32_t nb) {
    unsigned long long run = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const unsigned long long v = bsums[b];
        bsums[b] = run;
        run += v;
    }
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t carry = (uint32_t)bsums[b];
        for (uint32_t it = 0; it < 4u; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t h = b * 1024u + it * 256u + t;
                if (h >= n) continue;
                const uint32_t v = start[h];
                start[h] = carry;
                if (h + 1u == n) start[n] = carry + v;
                carry += v;
            }
    }
}

struct Result {
    std::vector<float> segments;
    std::vector<uint32_t> line, layer_first;
    uint64_t segments_in = 0, crossings = 0, lines_hit = 0, odd_lines = 0;
};

Result by_kernels(uint32_t axis, const std::vector<float>& pts, const std::vector<U4>& cons, const std::vector<float>& lines_in, uint32_t n_layers,
                  uint32_t n_lines, bool zigzag) {
    Result R;
    const uint32_t P = (uint32_t)(pts.size() / 3u), pb = (P + 1023u) / 1024u;
    Frame f{(axis + 1u) % 3u, (axis + 2u) % 3u, P, (uint32_t)cons.size(), n_lines};
    const rml::HatchScratch S(P, n_layers);
    char* sc = static_cast<char*>(std::malloc(S.bytes));
    std::memcpy(S.lines.at(sc), lines_in.data(), (size_t)n_layers * 16u);
    const float* lines = S.lines.at(sc);
    uint32_t* cstart = S.cstart.at(sc);
    uint32_t* j0 = S.j0.at(sc);
    unsigned long long* bsums = S.bsums.at(sc);
    // count: workgroup b, pass it, thread t
    for (uint32_t b = 0; b < pb; b++) {
        unsigned long long total = 0;
        for (uint32_t it = 0; it < 4u; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t i = b * 1024u + it * 256u + t;
                if (i >= P) continue;
                uint32_t cnt = 0, first = 0;
                Seg g;
                if (segment(f, pts.data(), cons.data(), lines, i, g)) {
                    R.segments_in++;
                    if (g.sa < g.sb && g.sa - g.sa == 0.0 && g.sb - g.sb == 0.0) {
                        first = lower(g.sa, g.offset, g.spacing, n_lines);
                        cnt = lower(g.sb, g.offset, g.spacing, n_lines) - first;
                    }
                }
                cstart[i] = cnt, j0[i] = first, total += cnt;
            }
        bsums[b] = total;
    }
    unsigned long long lo = 0, hi = 0;
    for (uint32_t b = 0; b < pb; b++) lo += bsums[b] & 0xFFFFFFFFull, hi += bsums[b] >> 32;
    CHECK(rml::hatch_crossings_fit(lo, hi));
    const uint32_t N = (uint32_t)lo;
    R.crossings = N;
    R.layer_first.assign((size_t)n_layers + 1u, 0u);
    if (N == 0u) {
        std::free(sc);
        return R;
    }
    scan_in_place(cstart, P, bsums, pb);
    CHECK(cstart[P] == N);
    const rml::HatchItems I(N);
    char* ic = static_cast<char*>(std::malloc(I.sort));  // (the sort's own scratch: mesh_slice_layout_check.cpp)
    unsigned long long* keys = I.ikeys.at(ic);
    uint32_t* values = I.ivals.at(ic);
    float* xs = I.xs.at(ic);
    uint32_t* hstart = I.hstart.at(ic);
    // items: one thread per crossing
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t seg = item_segment(cstart, P, i);
        CHECK(seg < P && cstart[seg] <= i && i < cstart[seg + 1u]);
        const uint32_t j = j0[seg] + (i - cstart[seg]);
        CHECK(j < n_lines);
        Seg g;
        CHECK(segment(f, pts.data(), cons.data(), lines, seg, g));
        const double cj = c_of(j, g.offset, g.spacing), t = (cj - g.sa) / (g.sb - g.sa);
        CHECK(g.sa <= cj && cj < g.sb);
        const float* A = pts.data() + (size_t)g.a * 3u;
        const float* B = pts.data() + (size_t)g.b * 3u;
        const float xu = (float)((double)A[f.u] + t * ((double)B[f.u] - (double)A[f.u])), xv = (float)((double)A[f.v] + t * ((double)B[f.v] - (double)A[f.v]));
        const float r = (float)((double)xu * g.dx + (double)xv * g.dy);
        keys[i] = ((unsigned long long)g.layer * n_lines + j) << 32 | key32(r);
        values[i] = i;
        xs[2u * i] = xu, xs[2u * i + 1u] = xv;
    }
    {   // (the sort)
        std::vector<uint32_t> order(N);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        std::vector<unsigned long long> k(N);
        for (uint32_t q = 0; q < N; q++) k[q] = keys[order[q]];
        for (uint32_t q = 0; q < N; q++) keys[q] = k[q], values[q] = order[q];
    }
    // pair
    const uint32_t nb = (N + 1023u) / 1024u;
    unsigned long long* hsums = I.bsums.at(ic);
    for (uint32_t b = 0; b < nb; b++) {
        unsigned long long heads = 0;
        for (uint32_t it = 0; it < 4u; it++)
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t q = b * 1024u + it * 256u + t;
                if (q >= N) continue;
                const unsigned long long L = keys[q] >> 32;
                const uint32_t rank = q - key_lower(keys, q, L << 32);
                const bool partner = q + 1u < N && (keys[q + 1u] >> 32) == L, even = (rank & 1u) == 0u;
                hstart[q] = even && partner ? 1u : 0u;
                heads += hstart[q];
                R.lines_hit += rank == 0u, R.odd_lines += even && !partner;
            }
        hsums[b] = heads;
    }
    scan_in_place(hstart, N, hsums, nb);
    const uint32_t H = hstart[N];
    CHECK(2ull * H <= N);
    const rml::HatchSlot T(H, n_layers);
    char* hb = static_cast<char*>(std::malloc(T.bytes));
    float* segments = T.segments.at(hb);
    uint32_t* line = T.line.at(hb);
    uint32_t* layer_first = T.layer_first.at(hb);
    std::vector<uint8_t> written(H, 0), lf_written((size_t)n_layers + 1u, 0);
    // emit: one thread per sorted crossing and per layer
    const uint32_t threads = ((std::max(N, n_layers + 1u) + 255u) / 256u) * 256u;
    for (uint32_t q = 0; q < threads; q++) {
        if (q <= n_layers) {
            const unsigned long long first_line = (unsigned long long)q * n_lines;
            CHECK(q == n_layers || first_line < (1ull << 32));
            layer_first[q] = q == n_layers ? hstart[N] : hstart[key_lower(keys, N, first_line << 32)];
            lf_written[q]++;
        }
        if (q >= N) continue;
        uint32_t pos = hstart[q];
        if (hstart[q + 1u] == pos) continue;
        const unsigned long long L = keys[q] >> 32;
        CHECK(values[q] < N && values[q + 1u] < N);
        float a[2] = {xs[2u * values[q]], xs[2u * values[q] + 1u]}, b2[2] = {xs[2u * values[q + 1u]], xs[2u * values[q + 1u] + 1u]};
        if (zigzag && ((uint32_t)(L % n_lines) & 1u) != 0u) {
            const uint32_t q0 = key_lower(keys, q, L << 32), q1 = L == 0xFFFFFFFFull ? N : key_lower(keys, N, (L + 1ull) << 32);
            const uint32_t base = hstart[q0], m = hstart[q1] - base;
            CHECK(pos >= base && pos - base < m);
            pos = base + (m - 1u - (pos - base));
            std::swap(a[0], b2[0]), std::swap(a[1], b2[1]);
        }
        CHECK(pos < H && !written[pos]);
        written[pos] = 1;
        segments[4u * pos] = a[0], segments[4u * pos + 1u] = a[1], segments[4u * pos + 2u] = b2[0], segments[4u * pos + 3u] = b2[1];
        line[pos] = (uint32_t)L;
    }
    for (uint8_t w : written) CHECK(w == 1);
    for (uint8_t w : lf_written) CHECK(w == 1);
    R.segments.assign(segments, segments + 4u * (size_t)H);
    R.line.assign(line, line + H);
    R.layer_first.assign(layer_first, layer_first + n_layers + 1u);
    std::free(hb);
    std::free(ic);
    std::free(sc);
    return R;
}

// The contract walked line by line: every segment against every line.
Result by_walk(uint32_t axis, const std::vector<float>& pts, const std::vector<U4>& cons, const std::vector<float>& lines, uint32_t n_layers,
               uint32_t n_lines, bool zigzag) {
    Result R;
    const uint32_t u = (axis + 1u) % 3u, v = (axis + 2u) % 3u;
    struct X { uint32_t key; uint32_t order; float xu, xv; };
    std::map<unsigned long long, std::vector<X>> by_line;
    uint32_t order = 0;
    for (const U4& c : cons)
        for (uint32_t at = 0; at < c.y; at++) {
            if (c.w == 0u && at + 1u == c.y) continue;
            R.segments_in++;
            const float* l = &lines[(size_t)c.z * 4u];
            const double dx = l[0], dy = l[1];
            const float* T = &pts[(size_t)(c.x + at) * 3u];
            const float* Hd = &pts[(size_t)(c.x + (at + 1u) % c.y) * 3u];
            const double st = (double)T[v] * dx - (double)T[u] * dy, sh = (double)Hd[v] * dx - (double)Hd[u] * dy;
            if (!(std::isfinite(st) && std::isfinite(sh)) || st == sh) continue;
            const float* A = st < sh ? T : Hd;
            const float* B = st < sh ? Hd : T;
            const double sa = std::min(st, sh), sb = std::max(st, sh);
            for (uint32_t j = 0; j < n_lines; j++) {
                const double cj = (double)l[2] + (double)j * (double)l[3];
                if (!(sa <= cj && cj < sb)) continue;
                const double t = (cj - sa) / (sb - sa);
                X x;
                x.xu = (float)((double)A[u] + t * ((double)B[u] - (double)A[u])), x.xv = (float)((double)A[v] + t * ((double)B[v] - (double)A[v]));
                x.key = key32((float)((double)x.xu * dx + (double)x.xv * dy)), x.order = order++;
                by_line[(unsigned long long)c.z * n_lines + j].push_back(x);
                R.crossings++;
            }
        }
    R.layer_first.assign((size_t)n_layers + 1u, 0u);
    for (auto& e : by_line) {
        std::vector<X>& xs = e.second;
        std::stable_sort(xs.begin(), xs.end(), [](const X& a, const X& b) { return a.key < b.key; });
        R.lines_hit++, R.odd_lines += xs.size() & 1u;
        const size_t m = xs.size() / 2u;
        const bool back = zigzag && ((e.first % n_lines) & 1u) != 0u;
        for (size_t i = 0; i < m; i++) {
            const size_t p = back ? m - 1u - i : i;
            const X& a = xs[2u * p + (back ? 1u : 0u)];
            const X& b = xs[2u * p + (back ? 0u : 1u)];
            R.segments.insert(R.segments.end(), {a.xu, a.xv, b.xu, b.xv});
            R.line.push_back((uint32_t)e.first);
        }
        for (uint32_t k = (uint32_t)(e.first / n_lines) + 1u; k <= n_layers; k++) R.layer_first[k] += (uint32_t)m;
    }
    return R;
}

void index_arithmetic() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    auto coord = [&]() { return (float)((double)(next() % 4001u) / 16.0 - 125.0); };  // multiples of 1 / 16: lines through vertices happen
    struct Case { uint32_t n_layers, contours_per_layer, max_points, n_lines; float dx, dy, offset, spacing; };
    for (const Case& c : {Case{1, 1, 4, 12, 1.0f, 0.0f, 0.5f, 1.0f}, Case{3, 2, 9, 40, 0.0f, 1.0f, -120.0f, 6.25f},
                          Case{5, 7, 40, 300, 3.0f, -4.0f, -900.0f, 6.0f}, Case{4, 3, 300, 1000, 0.8660254f, 0.5f, -180.0f, 0.25f},
                          Case{2, 1, 3, 1u << 15, 1.0f, 1.0f, -250.0f, 0.015625f}})
        for (uint32_t axis = 0; axis < 3u; axis++)
            for (int zig = 0; zig < 2; zig++) {
                std::vector<float> pts, lines;
                std::vector<U4> cons;
                for (uint32_t k = 0; k < c.n_layers; k++) {
                    lines.insert(lines.end(), {c.dx, c.dy, c.offset + (float)k, c.spacing});
                    if (k == 1u) continue;  // an empty layer between full ones
                    for (uint32_t q = 0; q < c.contours_per_layer; q++) {
                        const uint32_t n = 1u + (uint32_t)(next() % c.max_points), closed = (uint32_t)(next() % 4u != 0u);
                        cons.push_back(U4{(uint32_t)(pts.size() / 3u), n, k, closed});
                        for (uint32_t i = 0; i < n; i++) pts.insert(pts.end(), {coord(), coord(), coord()});
                    }
                }
                const Result a = by_kernels(axis, pts, cons, lines, c.n_layers, c.n_lines, zig != 0);
                const Result b = by_walk(axis, pts, cons, lines, c.n_layers, c.n_lines, zig != 0);
                CHECK(a.segments_in == b.segments_in && a.crossings == b.crossings && a.lines_hit == b.lines_hit && a.odd_lines == b.odd_lines);
                CHECK(a.segments.size() == b.segments.size() && a.line == b.line && a.layer_first == b.layer_first);
                CHECK(a.segments.empty() || std::memcmp(a.segments.data(), b.segments.data(), a.segments.size() * 4u) == 0);
                CHECK(c.n_layers < 2u || a.layer_first[1] == a.layer_first[2]);
            }
}

}  // namespace

int main() {
    offsets();
    bounds();
    index_arithmetic();
    std::printf("hatch_layout_check: ok (%d checks)\n", g_checks);
    return 0;
}
