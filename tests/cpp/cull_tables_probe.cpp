// What the decoder (ray-marching_amd/csrc/rm_decode.h) hands the culling rules of the march, made readable for the tests (CPU,
// built by tests/test_cull_tables_cpu.py): the unit records, the world-space bounding spheres, scene_scale, smooth_slack, the
// vetoes and each record's place in the miss-test tables.  Reads any number of programs from standard input, each as
// cmd_count, n_words and the words (decimal u32), and prints one line of JSON per program.  Every binary32 number is printed
// as its bit pattern (NaN and infinities survive, nothing is rounded by printing), smooth_slack as the bits of the double.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct float4 { float x, y, z, w; };  // rm_device.h names the HIP vector type in RmLaunch; this is a host-only build
#include "rm_abi.h"
#include "rm_decode.h"

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
    unsigned long long cc = 0, nw = 0;
    while (std::scanf("%llu %llu", &cc, &nw) == 2) {
        if (nw > (1ull << 20) || cc > 0xFFFFFFFFull) return 2;
        std::vector<uint32_t> words((size_t)nw);
        for (auto& x : words) {
            unsigned long long v;
            if (std::scanf("%llu", &v) != 1 || v > 0xFFFFFFFFull) return 2;
            x = (uint32_t)v;
        }
        RmDecoded d;
        const int rc = rm_decode_program((uint32_t)cc, words.data(), (uint32_t)words.size(), &d);
        if (rc != RM_OK) {
            std::printf("{\"rc\": %d}\n", rc);
            continue;
        }
        unsigned long long slack_bits;
        std::memcpy(&slack_bits, &d.smooth_slack, 8);
        std::printf("{\"rc\": 0, \"unit_mode\": %u, \"unit_kmax\": %u, \"scene_scale\": %u, \"smooth_slack\": %llu, \"cull_veto\": %d, "
                    "\"bound_walk\": %d, \"has_xforms\": %d, \"prunable\": %d, \"n_sphere\": %u, \"n_box\": %u, \"n_plane\": %u, \"spill_depth\": %u, ",
                    d.unit_mode, fbits(d.unit_kmax), fbits(d.scene_scale), slack_bits, (int)d.cull_veto, (int)d.bound_walk,
                    (int)d.has_xforms, (int)d.prunable, d.n_sphere, d.n_box, d.n_plane, d.spill_depth);
        std::printf("\"units\": [");
        for (size_t i = 0; i < d.units.size(); i++) {  // kind, first record, last record, p[0..5]
            const RmRecord& g = d.units[i];
            std::printf("%s[%u, %u, %u", i ? ", " : "", fbits(g.p[6]), g.op & 0xFFFFu, g.op >> 16);
            for (int k = 0; k < 6; k++) std::printf(", %u", fbits(g.p[k]));
            std::printf("]");
        }
        std::printf("], \"bounds\": [");
        for (size_t i = 0; i < d.bounds.size(); i++) std::printf("%s%u", i ? ", " : "", fbits(d.bounds[i]));
        std::printf("], \"rec\": [");
        for (size_t i = 0; i < d.rec.size(); i++) {  // kind, mode, RM_OP_NOCULL, table slot, unit + 1, command index, p[0..5]
            const RmRecord& r = d.rec[i];
            std::printf("%s[%u, %u, %u, %u, %u, %u", i ? ", " : "", RM_OP_KIND(r.op), RM_OP_MODE(r.op), (r.op & RM_OP_NOCULL) ? 1u : 0u,
                        fbits(r.p[6]), RM_OP_UNIT(r.op), d.rec_cmd[i]);
            for (int k = 0; k < 6; k++) std::printf(", %u", fbits(r.p[k]));
            std::printf("]");
        }
        std::printf("]}\n");
    }
    return 0;
}
