// The unit table of wave-level culling as a workgroup stages it in LDS (rm_kernel_v5.h stage_units), on the CPU with the mapping
// the kernel itself uses (rm_device.h rm_unit_table_source).  Reads pairs "n_units n_threads" from standard input; the unit
// records hold the word 100 u + j at dword j of unit u; every thread of the workgroup runs stage_units' loop.  Prints one line
// of JSON per pair: the table, and how often each of its dwords was written.  (Built by tests/test_unit_table_cpu.py.)
#include <cstdint>
#include <cstdio>
#include <vector>

struct float4 { float x, y, z, w; };  // rm_device.h names the HIP vector type in RmLaunch; this is a host-only build
#include "rm_abi.h"
#include "rm_device.h"

int main() {
    unsigned n_units = 0, n_threads = 0;
    while (std::scanf("%u %u", &n_units, &n_threads) == 2) {
        if (n_units == 0 || n_units > 64 || n_threads == 0 || n_threads > 1024) return 2;
        std::vector<uint32_t> src(8u * n_units), table(8u * n_units, 0xFFFFFFFFu), writes(8u * n_units, 0u);
        for (uint32_t u = 0; u < n_units; u++)
            for (uint32_t j = 0; j < 8u; j++) src[8u * u + j] = 100u * u + j;
        for (uint32_t tid = 0; tid < n_threads; tid++)
            for (uint32_t k = tid; k < 8u * n_units; k += n_threads) {
                table.at(k) = src.at(rm_unit_table_source(k, n_units));
                writes[k]++;
            }
        std::printf("{\"n_units\": %u, \"n_threads\": %u, \"table\": [", n_units, n_threads);
        for (size_t k = 0; k < table.size(); k++) std::printf("%s%u", k ? ", " : "", table[k]);
        std::printf("], \"writes\": [");
        for (size_t k = 0; k < writes.size(); k++) std::printf("%s%u", k ? ", " : "", writes[k]);
        std::printf("]}\n");
    }
    return 0;
}
