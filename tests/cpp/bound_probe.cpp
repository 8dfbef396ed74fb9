// rm_program_bound (ray-marching_amd/csrc/rm_mesh_bound.h) for the tests (CPU, built by tests/test_mesh_bound_cpu.py): the C ABI
// returns only L (rm_program_lipschitz, at P = 1); the sparse mesh extraction also relies on E, and on both at the lattice's P.
// Reads from standard input: cmd_count, n_words, the words (decimal u32), then any number of P values.  Prints one line per P:
// the status, L and E with 17 significant digits (inf as "inf").
#include <cstdint>
#include <cstdio>
#include <vector>

struct float4 { float x, y, z, w; };  // rm_device.h names the HIP vector type in RmLaunch; this is a host-only build
#include "rm_abi.h"
#include "rm_mesh_bound.h"

int main() {
    unsigned long long cc = 0, nw = 0;
    if (std::scanf("%llu %llu", &cc, &nw) != 2 || nw > (1ull << 24)) return 2;
    std::vector<uint32_t> words((size_t)nw);
    for (auto& x : words) {
        unsigned long long v;
        if (std::scanf("%llu", &v) != 1 || v > 0xFFFFFFFFull) return 2;
        x = (uint32_t)v;
    }
    double P;
    while (std::scanf("%lf", &P) == 1) {
        RmProgramBound b;
        const int rc = rm_program_bound((uint32_t)cc, words.data(), (uint32_t)words.size(), P, &b);
        std::printf("%d %.17g %.17g\n", rc, b.L, b.E);
    }
    return 0;
}
