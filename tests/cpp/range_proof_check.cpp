// The facts behind the range proofs of the generated march kernel (csrc/rm_interp.h "Range proofs"), on the CPU: the decoder's
// verdict on box sizes (RmDecoded::box_sizes_normal), the box lemma it feeds and the numerator lemma of normalize3_guard.
// Plain C++, built with sanitizers by tests/test_range_proof_cpu.py.
//   no arguments      everything
//   <rx> <ry> <rz>    prints box_sizes_normal of a program of one box with those half-extents, for the Python test
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

struct float4 { float x, y, z, w; };  // rm_device.h names the HIP vector type in RmLaunch; this is a host-only build
#include "rm_abi.h"
#include "rm_decode.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (failures++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                  \
    } while (0)

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// box_sizes_normal of "sphere; box(half); Union"
static bool sizes_normal(float rx, float ry, float rz) {
    std::vector<uint32_t> w;
    auto f = [&](float v) { w.push_back(bits_of(v)); };
    w.push_back(RM_CMD_SPHERE); f(0.0f); f(0.0f); f(0.0f); f(1.0f);
    w.push_back(RM_CMD_BOX); f(0.5f); f(0.25f); f(-0.5f); f(rx); f(ry); f(rz);
    w.push_back(RM_CMD_UNION);
    RmDecoded d;
    const int rc = rm_decode_program(3u, w.data(), (uint32_t)w.size(), &d);
    CHECK(rc == RM_OK, "decode: %d", rc);
    return d.box_sizes_normal;
}
static void box_sizes() {
    const float lim = std::ldexp(1.0f, -23), inf = INFINITY, nan = NAN;
    CHECK(sizes_normal(0.3f, 0.25f, 0.2f), "ordinary sizes");
    CHECK(sizes_normal(lim, -lim, 3.0e38f), "2^-23 on both signs, and the largest finite sizes");
    for (int axis = 0; axis < 3; axis++)
        for (float bad : {std::nextafterf(lim, 0.0f), 1.0e-9f, 0.0f, -0.0f, -1.0e-8f, inf, -inf, nan, 1.0e-45f}) {
            float r[3] = {0.3f, 0.25f, 0.2f};
            r[axis] = bad;
            CHECK(!sizes_normal(r[0], r[1], r[2]), "axis %d half-extent %g", axis, (double)bad);
        }
    // a program without boxes has nothing to refuse
    std::vector<uint32_t> w = {RM_CMD_SPHERE, 0u, 0u, 0u, bits_of(1.0e-30f)};
    RmDecoded d;
    CHECK(rm_decode_program(1u, w.data(), (uint32_t)w.size(), &d) == RM_OK && d.box_sizes_normal, "spheres alone");
}

// m = max(fl(t - r), 0) is 0 or >= 2^-46, its square 0 or >= 2^-92, and the radicand with it >= 2^-96 -- for r in every binade
// from 2^-23 up and t within 64 ulp of r, of 2 r and of the edges of their binades, both signs of r
static void box_lemma() {
    const float lim_m = std::ldexp(1.0f, -46), lim_sq = std::ldexp(1.0f, -92), lim_rad = std::ldexp(1.0f, -96);
    unsigned long long n = 0;
    for (int e = -23; e <= 127; e++) {
        const uint32_t base = (uint32_t)(e + 127) << 23;
        const uint32_t sigs[] = {0u, 1u, 2u, 0x155555u, 0x400000u, 0x6DB6DBu, 0x7FFFFEu, 0x7FFFFFu};
        for (uint32_t sg : sigs) {
            for (int neg = 0; neg < 2; neg++) {
                const float r = from_bits(base | sg | (neg ? 0x80000000u : 0u));
                const float ar = std::fabs(r);
                const float anchors[] = {ar, 2.0f * ar, std::ldexp(1.0f, e), std::ldexp(1.0f, e + 1), std::ldexp(1.0f, e + 2 > 127 ? 127 : e + 2), 0.0f};
                for (float a : anchors) {
                    if (!(a < INFINITY)) continue;
                    for (int d = -64; d <= 64; d++) {
                        const int64_t tb = (int64_t)bits_of(a) + d;
                        if (tb < 0 || tb >= 0x7F800000) continue;
                        const float t = from_bits((uint32_t)tb);  // t = |p - c| >= 0
                        volatile float q = t - r;
                        const float mx = q > 0.0f ? (float)q : 0.0f;  // fmax_(q, 0)
                        volatile float sq = mx * mx;
                        volatile float rad = (sq + 0.0f) + 0.0f;   // the other two axes inside their slabs
                        n++;
                        if (mx == 0.0f) { CHECK(rad == 0.0f, "r %a t %a", (double)r, (double)t); continue; }
                        CHECK(mx >= lim_m, "r %a t %a: m %a", (double)r, (double)t, (double)mx);
                        CHECK(sq >= lim_sq || sq == INFINITY, "r %a t %a: m^2 %a", (double)r, (double)t, (double)sq);
                        CHECK(rad >= lim_rad, "r %a t %a: radicand %a", (double)r, (double)t, (double)rad);
                    }
                }
            }
        }
    }
    // the lemma needs |r| >= 2^-23: just below it, a radicand under the guard's limit exists
    {
        const float r = std::ldexp(1.0f, -50), t = std::nextafterf(r, 1.0f);
        volatile float q = t - r;
        volatile float sq = q * q;
        CHECK(sq > 0.0f && sq < lim_rad, "2^-50: m^2 %a", (double)sq);
    }
    std::printf("box lemma: %llu (r, t) pairs\n", n);
}

// every numerator a of a normalisation has fl(a a) <= s, hence |a| <= sqrt(s) (1 + 2^-23): over every significand (the set
// tools/probe_div_model.cpp walks; powers of two scale a, s and the root together), with the root correctly rounded; and at the
// top of what DivGuard::root_of lets through (s <= 2^88 (1 + 2^-23)) that is below the numerator limit 2^78
static void numerator_lemma() {
    const double slack = 1.0 + std::ldexp(1.0, -23);
    for (uint32_t A = 1u << 23; A < (1u << 24); A++) {
        const float a = (float)A;
        volatile float s = a * a;          // the smallest radicand a can sit in: the other terms are >= 0 and rounding is monotone
        const float b = std::sqrt((float)s);
        CHECK((double)a <= (double)b * slack, "significand 0x%06x: a %a, root %a", A & 0x7FFFFFu, (double)a, (double)b);
        volatile float s2 = (float)s + a * a;  // ... and with a second equal term
        CHECK((double)a <= (double)std::sqrt((float)s2) * slack, "significand 0x%06x, two terms", A & 0x7FFFFFu);
    }
    const float s_top = from_bits(0x0F800000u + 2u * 0x2E000000u + 1u);  // the largest s with ((bits - kSLo) >> 1) <= kBSpan
    CHECK(s_top == std::ldexp(1.0f, 88) * (1.0f + std::ldexp(1.0f, -23)), "s_top %a", (double)s_top);
    CHECK((double)std::sqrt(s_top) * slack < std::ldexp(1.0, 78), "the largest numerator against 2^78");
    CHECK((double)std::sqrt(s_top) * slack < std::ldexp(1.0, 44) * 1.000001, "the largest numerator against 2^44 * 1.000001");
}

int main(int argc, char** argv) {
    if (argc == 4) {
        std::printf("%d\n", sizes_normal(std::strtof(argv[1], nullptr), std::strtof(argv[2], nullptr), std::strtof(argv[3], nullptr)) ? 1 : 0);
        return failures ? 1 : 0;
    }
    box_sizes();
    box_lemma();
    numerator_lemma();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("range proofs ok\n");
    return 0;
}
