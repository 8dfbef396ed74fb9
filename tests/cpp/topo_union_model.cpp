// topo_union_model.cpp -- the union-find of the topology merge pass (csrc/rm_topo_union.h: topo_find, topo_unite,
// topo_for_preceding, the very functions the kernels call) run by 8 CPU threads on random occupancies, and checked after ONE merge
// pass and a flatten: no adjacent same-class pair with different roots (what rm_topo_verify_kernel counts), and every root the
// smallest index of its component (a serial union-find below).  Stand-alone: g++ -std=c++17 -pthread, nothing from HIP; built
// plain and with -fsanitize=thread by tests/test_topology_union_cpu.py.
//
// Two modes per occupancy:
//   global  parent[p] = p, every point united with all its preceding same-class neighbours: no local pass has done any work, so
//           every union goes through the shared structure (the hardest case for it);
//   bricks  parent[p] = the smallest index of p's component inside its 8^3 brick (a serial labelling: what rm_topo_local_kernel
//           leaves), then the body of rm_topo_merge_kernel as it stands: the early-out for points whose preceding neighbours all
//           lie in their own brick, the same-brick skip, the skip of a neighbour whose parent equals the previous one's.
// Points are interleaved over the threads, and before each memory primitive a thread calls sched_yield() with a small seeded
// probability.
//
// -DTOPO_MODEL_TORN_MIN replaces this file's minimum by load / yield / conditional store, a lost update; the shared header is the
// same.  That build must FAIL: it shows that the two checks see a union that was lost.
//
// What this does not cover: x86 orders memory more strongly than the GPU does, and the primitives here are the host's, not
// __hip_atomic_load and atomicMin.  The model checks the algorithm under many interleavings of its primitives; it says nothing
// about the device's memory model or about the primitives' device implementations.
#include <sched.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <vector>

namespace model {
// One generator per thread, seeded per run: xorshift32.
thread_local uint32_t rng_state = 1u;
inline uint32_t rng_next() {
    uint32_t x = rng_state;
    x ^= x << 13; x ^= x >> 17; x ^= x << 5;
    return rng_state = x;
}
inline void maybe_yield() {
    if ((rng_next() & 63u) == 0u) sched_yield();
}
}  // namespace model

#define RM_TOPO_HOST_HOOK() model::maybe_yield()
#ifdef TOPO_MODEL_TORN_MIN
#define RM_TOPO_HOST_FETCH_MIN
namespace rmk {
// NOT a minimum: another thread's smaller value, stored between the load and the store, is overwritten.
inline uint32_t topo_fetch_min(uint32_t* p, uint32_t v) {
    const uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    sched_yield();
    if (v < cur) __atomic_store_n(p, v, __ATOMIC_RELAXED);
    return cur;
}
}  // namespace rmk
#endif
#include "rm_topo_union.h"

namespace {

constexpr uint32_t NX = 33, NY = 20, NZ = 17, N = NX * NY * NZ, THREADS = 8;
constexpr int SEEDS = 40;
const double DENSITIES[4] = {0.2, 0.3116, 0.5, 0.9};

struct Lattice {
    rmk::SparseGrid g;
    std::vector<uint8_t> occ;
};
inline uint32_t index_of(uint32_t i, uint32_t j, uint32_t k) { return i + NX * (j + NY * k); }

// splitmix64 for the occupancies: one stream per seed, the four densities drawn one after the other.
struct SplitMix {
    uint64_t s;
    double next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
    }
};

// ---- the serial yardstick: union by smaller index, no concurrency --------------------------------------------------------------
uint32_t serial_find(std::vector<uint32_t>& parent, uint32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
}
void serial_unite(std::vector<uint32_t>& parent, uint32_t a, uint32_t b) {
    a = serial_find(parent, a);
    b = serial_find(parent, b);
    if (a == b) return;
    if (a < b) parent[b] = a; else parent[a] = b;
}
// Roots of the components of the whole lattice (same_brick_only = false) or of each brick's part of them (true).
std::vector<uint32_t> serial_roots(const Lattice& L, bool same_brick_only) {
    std::vector<uint32_t> parent(N);
    std::iota(parent.begin(), parent.end(), 0u);
    for (uint32_t k = 0; k < NZ; k++)
        for (uint32_t j = 0; j < NY; j++)
            for (uint32_t i = 0; i < NX; i++) {
                const uint32_t p = index_of(i, j, k);
                const bool c = L.occ[p] != 0u;
                rmk::topo_for_preceding(L.g, i, j, k, c, [&](uint32_t qi, uint32_t qj, uint32_t qk) {
                    if (same_brick_only && (((qi ^ i) | (qj ^ j) | (qk ^ k)) >> 3) != 0u) return;
                    const uint32_t q = index_of(qi, qj, qk);
                    if ((L.occ[q] != 0u) == c) serial_unite(parent, p, q);
                });
            }
    for (uint32_t p = 0; p < N; p++) parent[p] = serial_find(parent, p);
    return parent;
}

// ---- the merge pass, one thread's share: the body of rm_topo_merge_kernel ----------------------------------------------------------
void merge_share(const Lattice& L, uint32_t* parent, uint32_t thread, bool bricks, uint32_t seed) {
    model::rng_state = (seed * 2654435761u) ^ (thread * 0x9E3779B9u) ^ 0x5bd1e995u;
    if (model::rng_state == 0u) model::rng_state = 1u;
    const uint32_t bound = N;
    for (uint32_t p = thread; p < N; p += THREADS) {
        const uint32_t i = p % NX, j = (p / NX) % NY, k = p / (NX * NY);
        const uint32_t il = i & 7u, jl = j & 7u, kl = k & 7u;
        if (bricks && il != 0u && il != 7u && jl != 0u && jl != 7u && kl != 0u) continue;  // every preceding neighbour is in this brick
        const bool c = L.occ[p] != 0u;
        uint32_t mine = p, last = 0xFFFFFFFFu;
        rmk::topo_for_preceding(L.g, i, j, k, c, [&](uint32_t qi, uint32_t qj, uint32_t qk) {
            if (bricks && (((qi ^ i) | (qj ^ j) | (qk ^ k)) >> 3) == 0u) return;  // the same brick: the local pass has united them
            const uint32_t q = index_of(qi, qj, qk);
            if ((L.occ[q] != 0u) != c) return;
            const uint32_t up = rmk::topo_load(parent + q);
            if (up == last) return;
            last = up;
            mine = rmk::topo_find<true>(parent, mine, bound);
            rmk::topo_unite(parent, mine, up, bound);
        });
    }
}
// rm_topo_flatten_kernel: others walk through p meanwhile.
void flatten_share(uint32_t* parent, uint32_t thread, uint32_t seed) {
    model::rng_state = (seed * 40503u) ^ (thread * 0x85EBCA6Bu) ^ 0x27d4eb2fu;
    if (model::rng_state == 0u) model::rng_state = 1u;
    for (uint32_t p = thread; p < N; p += THREADS) {
        const uint32_t r = rmk::topo_find<false>(parent, p, N);
        __atomic_store_n(parent + p, r, __ATOMIC_RELAXED);
    }
}

template <class Fn>
void on_threads(Fn fn) {
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < THREADS; t++) pool.emplace_back(fn, t);
    for (auto& th : pool) th.join();
}

// What rm_topo_verify_kernel counts: the pairs (p, preceding same-class neighbour) whose roots differ.
uint64_t verify(const Lattice& L, const std::vector<uint32_t>& parent) {
    uint64_t bad = 0;
    for (uint32_t p = 0; p < N; p++) {
        const uint32_t i = p % NX, j = (p / NX) % NY, k = p / (NX * NY);
        const bool c = L.occ[p] != 0u;
        rmk::topo_for_preceding(L.g, i, j, k, c, [&](uint32_t qi, uint32_t qj, uint32_t qk) {
            const uint32_t q = index_of(qi, qj, qk);
            if ((L.occ[q] != 0u) == c && parent[q] != parent[p]) bad++;
        });
    }
    return bad;
}

bool run(const Lattice& L, const std::vector<uint32_t>& want, bool bricks, int seed, double density) {
    std::vector<uint32_t> parent(N);
    if (bricks) parent = serial_roots(L, true);
    else std::iota(parent.begin(), parent.end(), 0u);
    uint32_t* P = parent.data();
    on_threads([&](uint32_t t) { merge_share(L, P, t, bricks, (uint32_t)seed * 8u + (bricks ? 1u : 0u)); });  // ONE pass
    on_threads([&](uint32_t t) { flatten_share(P, t, (uint32_t)seed); });
    const uint64_t bad = verify(L, parent);
    uint64_t wrong = 0;
    for (uint32_t p = 0; p < N; p++) wrong += parent[p] != want[p];
    if (bad != 0 || wrong != 0) {
        std::printf("FAILED: seed %d density %g mode %s: %llu adjacent same-class pairs with different roots, %llu points whose root is "
                    "not the smallest index of their component\n", seed, density, bricks ? "bricks" : "global",
                    (unsigned long long)bad, (unsigned long long)wrong);
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int seeds = argc > 1 ? std::atoi(argv[1]) : SEEDS;
    for (int seed = 0; seed < seeds; seed++) {
        SplitMix rng{0x746F706Full + (uint64_t)seed * 0x100000001B3ull};
        for (double density : DENSITIES) {
            Lattice L;
            L.g.nx = NX; L.g.ny = NY; L.g.nz = NZ;
            L.occ.resize(N);
            for (uint32_t p = 0; p < N; p++) L.occ[p] = rng.next() < density ? 1u : 0u;
            const std::vector<uint32_t> want = serial_roots(L, false);
            for (uint32_t p = 0; p < N; p++)
                if (want[p] > p || want[want[p]] != want[p]) { std::printf("FAILED: the serial yardstick, seed %d\n", seed); return 3; }
            for (int bricks = 0; bricks < 2; bricks++)
                if (!run(L, want, bricks != 0, seed, density)) return 1;
        }
    }
    std::printf("topo union model ok: %d seeds x 4 densities x 2 modes on %u x %u x %u points, %u threads, one merge pass each\n", seeds, NX, NY,
                NZ, THREADS);
    return 0;
}
