// lds_layout_check.cpp -- the dynamic-LDS layouts of the kernels (ray-marching_amd/csrc/rm_lds_layout.h) on the CPU, under
// ASan + UBSan (tests/test_decoder_fuzz_cpu.py).  Every region offset and total of rml::CullLds, rml::MarchLds,
// rml::PixelLds and rml::QueryLds equals the expression the host and the kernels used before the layouts existed -- and
// the march kernel still writes out for the offsets that depend on the launch --, written out here by hand; regions lie in declaration
// order, do not overlap, start on 16-byte boundaries and end at `bytes`; rml::choose_march returns what launch_v5's
// formulas returned, and never sizes a workgroup below what the launch that follows takes.
//   lds_layout_check                 the sweeps
//   lds_layout_check FILE            ... and the programs of FILE, one per line: `n waves_per_tile in_lds cmd_count n_words
//                                    word ...` (decimal): decoded, launched as a 24 x 16 frame would be, the chooser must
//                                    give that line's waves per tile and program placement
#include "rm_lds_layout.h"

struct float4 { float x, y, z, w; };  // rm_device.h names the HIP vector type in RmLaunch; this is a host-only build
#include "rm_decode.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <initializer_list>
#include <sstream>
#include <string>
#include <vector>

namespace {

long long g_checks = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Span { size_t offset, bytes; };

// in declaration order, 16-byte aligned, disjoint, the last one ends at `total`
void check_regions(std::initializer_list<Span> regions, size_t total) {
    size_t end = 0;
    for (const Span& r : regions) {
        CHECK(r.offset % 16u == 0u);
        CHECK(r.offset >= end);
        end = r.offset + r.bytes;
    }
    CHECK(end == total);
}

const uint32_t kCounts[] = {0u, 1u, 2u, 3u, 5u, 16u, 17u, 63u, 64u, 100u, 255u, 256u};                       // n_cone, n_slab
const uint32_t kRecords[] = {0u, 1u, 2u, 7u, 8u, 64u, 65u, 128u, 129u, 255u, 256u, 257u, 1000u, 2730u, 6000u};  // n_rec, n_grp, n_tree

void cull_tables() {
    for (uint32_t n_cone = 0; n_cone <= 256u; n_cone++)
        for (uint32_t n_slab = 0; n_slab <= 256u; n_slab++)
            for (int aux = 0; aux < 2; aux++) {
                const rml::CullLds T(n_cone, n_slab, aux != 0);
                // rm_tile_pre_v5 and the self-tests: smem, smem + 4 dwords, + n_cone float4, + 3 n_slab float4
                CHECK(T.veto == 0u && T.cone == 16u && T.slab == 16u + 16u * n_cone && T.aux == 16u + 16u * n_cone + 48u * n_slab);
                const size_t host = 16u + (size_t)n_cone * 16u + (size_t)n_slab * 48u + (aux ? (size_t)(n_cone + n_slab) * 8u : 0u);
                CHECK(T.bytes == host);
                check_regions({{T.veto, 16u}, {T.cone, 16u * n_cone}, {T.slab, 48u * n_slab}, {T.aux, aux ? 8u * (n_cone + n_slab) : 0u}}, T.bytes);
            }
}

void wave_buffers() {
    using W = rml::MarchWaveLds;
    // rm_render_v5_body, in dwords from the wave's base: wbase, + V5_RQ, + 4 V5_RQ, + V5_SQ, + 4 V5_SQ, + V5_HQ, + 3 V5_HQ, + 16
    CHECK(rml::V5_RQ == 64u && rml::V5_SQ == 64u && rml::V5_HQ == 128u && rml::V5_POOL == 1024u);
    CHECK(W::rq_rid == 0u && W::rq_d == 4u * 64u && W::sq_rid == 4u * 256u && W::sq_v == 4u * 320u && W::hq_rid == 4u * 512u);
    CHECK(W::hq_v == 4u * 640u && W::wxy == 4u * 1024u && W::tn == 4u * 1040u && W::bytes == 4u * 1232u);
    CHECK(rml::V5_TN_DWORDS == 192u && rml::V5_WAVE_DWORDS == 1232u);
    check_regions({{W::rq_rid, 4u * 64u}, {W::rq_d, 12u * 64u}, {W::sq_rid, 4u * 64u}, {W::sq_v, 12u * 64u}, {W::hq_rid, 4u * 128u},
                   {W::hq_v, 12u * 128u}, {W::wxy, 64u}, {W::tn, 768u}}, W::bytes);
    CHECK(W::tn == 4u * (rml::V5_WAVE_DWORDS - rml::V5_TN_DWORDS));  // the normals are last: a wave without them ends there
}

void march_one(uint32_t wpt, uint32_t wd, uint32_t depth, uint32_t n_cone, uint32_t n_slab, bool lds, uint32_t n_rec, uint32_t n_grp,
               uint32_t n_tree, bool tagged) {
    const rml::MarchLds M(wpt, wd, depth, n_cone, n_slab, lds, n_rec, n_grp, n_tree, tagged);
    // rm_render_v5_body's pointers, as byte offsets from smem
    const size_t wbase0 = 4u * (size_t)1024u, after = 4u * ((size_t)1024u + (size_t)wpt * wd);
    const size_t t_cone = after + 4u * ((size_t)wpt * depth * 64u), t_slab = t_cone + 16u * (size_t)n_cone, lprog = t_slab + 16u * (3u * (size_t)n_slab);
    const size_t lunits = lprog + 4u * (8u * (size_t)n_rec), ltree = lunits + 4u * (8u * (size_t)n_grp);
    const size_t s_next = lprog + 4u * (lds ? ((size_t)n_rec + n_grp + n_tree) * 8u : 0u);
    CHECK(M.pool == 0u && M.waves == wbase0 && M.wave_bytes == 4u * (size_t)wd && M.spill == after);
    CHECK(M.cone == t_cone && M.slab == t_slab && M.prog == lprog && M.ctl == s_next);
    if (lds) CHECK(M.units == lunits && M.tree == ltree);
    else CHECK(M.units == lprog && M.tree == lprog);
    CHECK(M.off == s_next + 4u * 4u && M.rmat == s_next + 4u * 36u);
    // launch_v5_w's shmem
    const size_t cull_bytes = (size_t)n_cone * 16u + (size_t)n_slab * 48u;
    const size_t shmem = (size_t)(1024u + wpt * wd) * 4u + (size_t)depth * 64u * wpt * 4u + cull_bytes +
                         (lds ? (size_t)(n_rec + n_grp + n_tree) * 32u : 0u) + (16u + 144u) + (tagged ? 1024u : 0u);
    CHECK(M.bytes == shmem);
    check_regions({{M.pool, 4096u}, {M.waves, (size_t)wpt * M.wave_bytes}, {M.spill, (size_t)wpt * depth * 256u}, {M.cone, 16u * (size_t)n_cone},
                   {M.slab, 48u * (size_t)n_slab}, {M.prog, lds ? 32u * (size_t)n_rec : 0u}, {M.units, lds ? 32u * (size_t)n_grp : 0u},
                   {M.tree, lds ? 32u * (size_t)n_tree : 0u}, {M.ctl, 16u}, {M.off, 128u}, {M.rmat, tagged ? 1024u : 0u}, {M.pad, 16u}}, M.bytes);
    CHECK(M.wave_bytes % 16u == 0u);  // every wave's buffers start on a 16-byte boundary
}

// launch_v5's formulas before the layouts existed
struct OldChoice { bool lds; int wpt; size_t bytes; };
OldChoice old_choice(bool lds, int wpt, uint32_t spill_depth, uint32_t mat_depth, bool tagged, uint32_t n_cone, uint32_t n_slab, uint32_t n_rec,
                     uint32_t n_grp, size_t tree_size) {
    const size_t cull_bytes = n_rec <= 256u ? (size_t)n_cone * 16u + (size_t)n_slab * 48u : 0u;
    const size_t prog_bytes = (size_t)(n_rec + n_grp + tree_size) * 32u;
    const size_t depth = std::max<size_t>(spill_depth + (tree_size == 0u ? 0u : 1u), tagged ? mat_depth : 0u);
    const size_t per_wave = 1232u * 4u + depth * 256u;
    const size_t fixed = 4096u + cull_bytes + (16u + 144u) + (tagged ? 1024u : 0u);
    if (lds && fixed + prog_bytes + per_wave > 60u * 1024u) lds = false;
    const size_t fixed_all = fixed + (lds ? prog_bytes : 0u);
    while (wpt > 1 && fixed_all + (size_t)wpt * per_wave > 48u * 1024u) wpt /= 2;
    return OldChoice{lds, wpt, fixed_all + (size_t)wpt * per_wave};
}

void chooser_one(uint32_t spill_depth, uint32_t mat_depth, bool tagged, uint32_t n_cone, uint32_t n_slab, uint32_t n_rec, uint32_t n_grp,
                 uint32_t tree_size) {
    for (int want = 0; want < 2; want++)
        for (uint32_t wpt : {1u, 2u, 4u, 8u}) {
            const OldChoice o = old_choice(want != 0, (int)wpt, spill_depth, mat_depth, tagged, n_cone, n_slab, n_rec, n_grp, tree_size);
            const rml::MarchChoice m = rml::choose_march(want != 0, wpt, spill_depth, tagged ? mat_depth : 0u, tagged, n_cone, n_slab, n_rec, n_grp, tree_size);
            CHECK(m.prog_in_lds == o.lds && (int)m.wpt == o.wpt && m.bytes == o.bytes);
            // The launch that follows (plan_v5, launch_v5_w): tables only with culling (n_rec <= 256), the tree table and its
            // spill slot only in the masked tree loop, no spill columns and no tree table under a generated kernel, the
            // material stack unless that kernel walks the materials itself, the partial normals unless it takes four taps at once.
            for (int cull = 0; cull < 2; cull++)
                for (int tree = 0; tree < 2; tree++)
                    for (int spec = 0; spec < 2; spec++)
                        for (int walk = 0; walk < 2; walk++)
                            for (int taps4 = 0; taps4 < 2; taps4++) {
                                if ((cull && n_rec > 256u) || (tree && (!m.prog_in_lds || tree_size == 0u)) || ((walk || taps4) && !spec)) continue;
                                uint32_t n_tree = tree ? tree_size : 0u, depth = spill_depth + (n_tree != 0u ? 1u : 0u);
                                if (spec) { depth = 0u; n_tree = 0u; }
                                if (tagged && !(spec && walk)) depth = std::max(depth, mat_depth);
                                const uint32_t wd = rml::V5_WAVE_DWORDS - ((spec && taps4 && !tagged) ? rml::V5_TN_DWORDS : 0u);
                                const rml::MarchLds exact(m.wpt, wd, depth, cull ? n_cone : 0u, cull ? n_slab : 0u, m.prog_in_lds, n_rec, n_grp, n_tree, tagged);
                                CHECK(exact.bytes <= m.bytes);
                            }
        }
}

void march_and_chooser() {
    // every spill depth, wave count and wave size against a few programs ...
    for (uint32_t depth = 0; depth <= 260u; depth++)
        for (uint32_t wpt : {1u, 2u, 4u, 8u})
            for (uint32_t wd : {rml::V5_WAVE_DWORDS, rml::V5_WAVE_DWORDS - rml::V5_TN_DWORDS})
                for (int lds = 0; lds < 2; lds++)
                    for (int tagged = 0; tagged < 2; tagged++)
                        for (uint32_t n : {0u, 1u, 31u, 256u, 6000u}) march_one(wpt, wd, depth, n % 257u, (7u * n) % 257u, lds != 0, n, n / 2u, n, tagged != 0);
    // ... every table size ...
    for (uint32_t n_cone = 0; n_cone <= 256u; n_cone++)
        for (uint32_t n_slab = 0; n_slab <= 256u; n_slab++) {
            march_one(4u, rml::V5_WAVE_DWORDS, n_cone % 33u, n_cone, n_slab, true, n_cone + n_slab, n_cone, 0u, (n_slab & 1u) != 0u);
            chooser_one(n_slab % 33u, n_cone % 90u, (n_cone & 1u) != 0u, n_cone, n_slab, n_cone + n_slab, std::min(n_cone + n_slab, 64u), (n_cone + n_slab) % 129u);
        }
    // ... and the program sizes against each other
    for (uint32_t n_rec : kRecords)
        for (uint32_t n_grp : {0u, 1u, 64u, 65u, 6000u})
            for (uint32_t n_tree : {0u, 1u, 128u, 129u, 6000u})
                for (uint32_t n_cone : kCounts)
                    for (uint32_t n_slab : {0u, 1u, 100u, 256u})
                        for (uint32_t depth : {0u, 1u, 31u, 55u, 260u}) {
                            for (int lds = 0; lds < 2; lds++)
                                for (int tagged = 0; tagged < 2; tagged++)
                                    march_one(n_rec % 2u ? 8u : 2u, depth % 2u ? rml::V5_WAVE_DWORDS : rml::V5_WAVE_DWORDS - rml::V5_TN_DWORDS, depth, n_cone,
                                              n_slab, lds != 0, n_rec, n_grp, n_tree, tagged != 0);
                            chooser_one(depth, (depth * 7u) % 87u, (n_grp & 1u) != 0u, n_cone, n_slab, n_rec, n_grp, n_tree);
                            chooser_one(depth, 260u - depth, true, n_cone, n_slab, n_rec, n_grp, n_tree);
                        }
}

void pixel_kernel() {
    for (uint32_t n_rec : kRecords)
        for (uint32_t depth = 0; depth <= 260u; depth++) {
            const rml::PixelLds P(n_rec, depth);
            CHECK(P.prog == 0u && P.spill == (size_t)n_rec * 8u * 4u);  // rm_render_pixel: smem, smem + n_rec * 8 dwords
            CHECK(P.bytes == (size_t)n_rec * 32u + (size_t)depth * 256u * sizeof(float));
            check_regions({{P.prog, 32u * (size_t)n_rec}, {P.spill, 1024u * (size_t)depth}}, P.bytes);
        }
}

// The query kernels' columns: what query_begin, rm_trace_rays and brick_lattice wrote out before the layout existed -- `slots * 64
// * 4 * 4` bytes, refused when that (+ 64 for the traversal march, + 4096 for a brick kernel) exceeds the device's LDS per
// workgroup, opted in above 64 KiB -- and query_spill's stride of slots * 64 floats per wave.  slots: everything a program of
// the largest command buffer (16384 words) can decode to, 2 * spill depth + 3 floats per transform level of the walk at the most.
void query_columns() {
    const uint32_t max_slots = 2u * 16384u + 3u * RM_MAX_XFORM_DEPTH;
    const size_t caps[] = {64u * 1024u, 160u * 1024u};
    CHECK(rml::kQueryOwnTrace == 64u && rml::kQueryOwnBrick == 4096u && rml::kQueryWaves == 4u && rml::kQueryLanes == 64u);
    for (uint32_t own : {0u, rml::kQueryOwnTrace, rml::kQueryOwnBrick})
        for (uint32_t slots = 0; slots <= max_slots; slots++) {
            const rml::QueryLds L(slots, own);
            const size_t shmem = (size_t)slots * 64u * 4u * 4u;
            CHECK(L.slots == slots && L.own == own && L.dynamic == shmem && L.bytes == shmem + own);
            CHECK(L.stride == (size_t)slots * 64u * sizeof(float) && 4u * (size_t)L.stride == L.dynamic);  // wave w at qsmem + w * slots * 64
            check_regions({{0u, L.stride}, {L.stride, L.stride}, {2u * (size_t)L.stride, L.stride}, {3u * (size_t)L.stride, L.stride}}, L.dynamic);
            CHECK(L.needs_opt_in() == (shmem + own > 64u * 1024u));
            for (size_t cap : caps) CHECK(L.fits(cap) == !(shmem + own > cap));
            const rml::QueryLds B = L.behind(rml::kQueryOwnBrick);
            CHECK(B.slots == slots && B.dynamic == L.dynamic && B.bytes == shmem + 4096u);
        }
    // the boundary: workgroups of cap - 1 and of cap bytes fit, one of cap + 1 does not (columns are whole KiB: `own` gives the rest)
    for (size_t cap : caps)
        for (uint32_t own : {0u, rml::kQueryOwnTrace, rml::kQueryOwnBrick}) {
            const uint32_t slots = (uint32_t)((cap - own) / 1024u);  // the most that fit behind `own`
            CHECK(rml::QueryLds(slots, own).fits(cap) == true && rml::QueryLds(slots + 1u, own).fits(cap) == false);
            for (int delta = -1; delta <= 1; delta++) {
                const rml::QueryLds L(slots - 1u, (uint32_t)(cap + delta - (size_t)(slots - 1u) * 1024u));
                CHECK(L.bytes == cap + delta && L.fits(cap) == (delta <= 0));
                CHECK(L.fits(cap - 1u) == (delta < 0) && L.fits(cap + 1u) == true);
            }
        }
    CHECK(rml::QueryLds(64u, 0u).needs_opt_in() == false && rml::QueryLds(64u, 1u).needs_opt_in() == true);
    CHECK(rml::QueryLds(63u, rml::kQueryOwnBrick).needs_opt_in() == true && rml::QueryLds(60u, rml::kQueryOwnBrick).needs_opt_in() == false);
}

// The programs of the GPU test "frames at the layout's decision boundaries": what launch_v5 decides for each, from the decoder's
// own numbers as fill_launch reads them, for a launch of few enough tiles to start from eight waves per tile.
int boundary_programs(const char* path) {
    std::ifstream in(path);
    CHECK(in.good());
    std::string line;
    int n_prog = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        uint32_t n = 0, want_wpt = 0, want_lds = 0, cc = 0, nw = 0;
        if (!(s >> n >> want_wpt >> want_lds >> cc >> nw)) continue;
        std::vector<uint32_t> words(nw);
        for (uint32_t& w : words) CHECK(static_cast<bool>(s >> w));
        RmDecoded d;
        CHECK(rm_decode_program(cc, words.data(), nw, &d) == RM_OK);
        const bool tagged = !d.mrec.empty();
        const rml::MarchChoice m = rml::choose_march(true, 8u, d.spill_depth + 3u * d.xform_depth, tagged ? 2u * d.mat_spill_depth + 3u * d.mat_xform_depth : 0u,
                                                     tagged, d.n_sphere, d.n_box, (uint32_t)d.rec.size(), (uint32_t)d.units.size(), (uint32_t)d.tree.size());
        std::printf("right_deep(%u): %u records, %u units, tree table %u, spill depth %u -> %s, %u waves per tile, %u bytes\n", n, (unsigned)d.rec.size(),
                    (unsigned)d.units.size(), (unsigned)d.tree.size(), d.spill_depth, m.prog_in_lds ? "LDS" : "scalar cache", m.wpt, m.bytes);
        CHECK(m.wpt == want_wpt && m.prog_in_lds == (want_lds != 0u));
        CHECK(m.bytes <= rml::kLdsLaunchLimit);  // drawable
        n_prog++;
    }
    return n_prog;
}

}  // namespace

int main(int argc, char** argv) {
    cull_tables();
    wave_buffers();
    march_and_chooser();
    pixel_kernel();
    query_columns();
    const int n_prog = argc > 1 ? boundary_programs(argv[1]) : 0;
    std::printf("lds layout ok (%lld checks, %d programs)\n", g_checks, n_prog);
    return 0;
}
