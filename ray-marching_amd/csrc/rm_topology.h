// rm_topology.h -- solid topology (rm_label_solid, rm_label_occupancy): the connected components of the occupancy lattice
// {d < level} -- bodies under 6-adjacency, voids under 26-adjacency, cavities the voids that do not reach the border --, their
// canonical numbers, sixteen moments per component and the Euler characteristic.  Included by rm_abi.hip alone.
// DESIGN.md section 19 is the contract; every output is an integer that no order of execution changes.
//
// The lattice is cut into the bricks of rm_mesh_sparse.h.  The passes:
//   probe      one lane per brick: the decision of sparse_probe_brick (the mesh's and the mass pass's, expression for expression);
//              a class byte per brick (outside / inside / kept) and block sums (kept low, inside high) for the statistics.
//   occupancy  one workgroup per brick, two own points per thread: one BYTE per point (0 outside, 1 inside).  A brick proven clear
//              stores its probe's side, a kept brick evaluates query_distance.  A byte, not a bit: every later pass reads single
//              neighbours at arbitrary offsets (up to 26 per point), and a caller's occupancy (rm_label_occupancy) arrives as bytes.
//   local      one workgroup per brick, occupancy and labels in LDS: both classes at once, union by smaller index with pointer
//              jumping until nothing changes; parent[p] = the smallest point of p's component INSIDE its brick.
//   merge      every point unites with its same-class neighbours in OTHER bricks (the 3 or 13 that precede it): a union-find in
//              global memory in which a parent is always a strictly smaller index (no cycles, every find terminates), unions by
//              atomicMin on the current root, retried from the value returned; find halves its path, again by atomicMin; every
//              other access a relaxed agent-scope atomic load.  No workgroup waits for another; a stale parent is still a smaller
//              member of the same component.
//   flatten    parent[p] = its root.   verify: per brick the adjacent same-class pairs whose roots differ (a row per brick, folded
//              and reduced as rm_reduce.h has it); the host repeats merge and flatten while that count is not zero
//              (expected: never).
//   exterior   every outside point on the lattice's border marks its root's byte (plain stores of the same value).
//   number     roots in linear order: block sums, rm_block_scan_kernel, ranks -> the label of each root in the label volume.
//   rows       per point its root's label into the label volume; the moments reduced over the lanes of a wave that share a root,
//              then one 64-bit integer atomic per entry per root per wave (integer and commutative: no word depends on arrival
//              order); V, E, F, K and the exterior's points from the occupancy alone, one row per brick + the row reducer.
#pragma once
#include "rm_mesh_sparse.h"
#include "rm_reduce.h"
#include "rm_topo_union.h"

namespace rmk {

constexpr uint32_t kTopoExterior = 0xFFFFFFFFu, kTopoCavityBit = 0x80000000u;  // RM_TOPO_EXTERIOR, RM_TOPO_CAVITY_BIT
constexpr uint32_t kTopoBrickPoints = kBrick * kBrick * kBrick;
constexpr uint32_t kTopoRankPer = 8u, kTopoRankBlock = 256u * kTopoRankPer;  // numbering: 2048 points per workgroup
enum : uint8_t { TOPO_BRICK_OUTSIDE = 0, TOPO_BRICK_INSIDE = 1, TOPO_BRICK_KEPT = 2 };

// This thread's two points of brick B: (il, jl, wave) and (il, jl, wave + 4); a wave holds one plane of 8 x 8 points at a time.
struct TopoPoint {
    uint32_t il, jl, kl;
    uint32_t i, j, k;
    uint32_t p;  // linear index (valid only)
    bool valid;  // inside the lattice
};
RM_DEV TopoPoint topo_point(const SparseGrid& g, const SparseBrick& B, uint32_t half) {
    TopoPoint t;
    t.il = threadIdx.x & 7u;
    t.jl = (threadIdx.x >> 3) & 7u;
    t.kl = (threadIdx.x >> 6) + 4u * half;
    t.i = B.i0 + t.il; t.j = B.j0 + t.jl; t.k = B.k0 + t.kl;
    t.valid = t.i < g.nx && t.j < g.ny && t.k < g.nz;
    t.p = t.i + g.nx * (t.j + g.ny * t.k);
    return t;
}
RM_DEV uint32_t topo_index(const SparseGrid& g, uint32_t i, uint32_t j, uint32_t k) { return i + g.nx * (j + g.ny * k); }

// ---- probe ------------------------------------------------------------------------------------------------------------------
template <int LOOP>
__global__ __launch_bounds__(256) void rm_topo_probe_kernel(QueryLaunch Q, SparseGrid g, float level, double L, double err2,
                                                            uint8_t* __restrict__ cls, unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    static_assert(sizeof wsum <= rml::kQueryOwnBrick, "the static LDS the host counts in front of the query columns");
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    uint32_t k = 0u, in = 0u;
    if (b < g.nb) {
        float v;
        k = sparse_probe_brick<LOOP>(Q, query_spill(Q.slots), g, sparse_brick(g, b), level, L, err2, v) ? 1u : 0u;
        in = (k == 0u && v < level) ? 1u : 0u;
        cls[b] = k ? TOPO_BRICK_KEPT : in ? TOPO_BRICK_INSIDE : TOPO_BRICK_OUTSIDE;
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>((unsigned long long)k | (unsigned long long)in << 32, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// ---- occupancy --------------------------------------------------------------------------------------------------------------
template <int LOOP>
__global__ __launch_bounds__(256) void rm_topo_occupancy_kernel(QueryLaunch Q, SparseGrid g, float level, const uint8_t* __restrict__ cls,
                                                                uint8_t* __restrict__ occ, unsigned long long* __restrict__ evaluations) {
    const uint32_t b = blockIdx.x;
    const SparseBrick B = sparse_brick(g, b);
    const uint32_t cl = cls[b];  // uniform over the workgroup
    float* spill = query_spill(Q.slots);
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const TopoPoint t = topo_point(g, B, half);
        if (!t.valid) continue;
        uint32_t in = cl;
        if (cl == TOPO_BRICK_KEPT) {
            const float d = query_distance<LOOP>(Q, spill, grid_coord(g.ox, t.i, g.sx), grid_coord(g.oy, t.j, g.sy), grid_coord(g.oz, t.k, g.sz));
            in = d < level ? 1u : 0u;  // NaN is outside
        }
        occ[t.p] = (uint8_t)in;
    }
    if (cl == TOPO_BRICK_KEPT && threadIdx.x == 0) {
        const uint32_t ex = min(kBrick, g.nx - B.i0), ey = min(kBrick, g.ny - B.j0), ez = min(kBrick, g.nz - B.k0);
        atomicAdd(evaluations, (unsigned long long)(ex * ey * ez));  // a statistic: nothing depends on it
    }
}

// ---- local labelling --------------------------------------------------------------------------------------------------------
// The smallest label among the same-class neighbours of local point (il, jl, kl) inside the brick: 6 for an inside point, 26 for
// an outside one.  s_cls: 0 outside, 1 inside, 2 beyond the lattice (never matches: such points are not visited).
RM_DEV uint32_t topo_local_min(const uint8_t* s_cls, const uint32_t* s_lab, uint32_t il, uint32_t jl, uint32_t kl, uint32_t c, uint32_t m) {
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int faces = (dx != 0) + (dy != 0) + (dz != 0);
                if (faces == 0) continue;
                const uint32_t qi = il + (uint32_t)dx, qj = jl + (uint32_t)dy, qk = kl + (uint32_t)dz;  // (wraps past 0: >= 8)
                if (qi >= kBrick || qj >= kBrick || qk >= kBrick) continue;
                const uint32_t q = qi + kBrick * (qj + kBrick * qk);
                if (s_cls[q] == c && (faces == 1 || c == 0u)) m = min(m, s_lab[q]);
            }
    return m;
}

// parent[p] = the smallest linear index of p's component within its brick.  Local indices l = il + 8 (jl + 8 kl) order the brick's
// points as their linear indices do, so the smallest local label is the smallest linear index.
__global__ __launch_bounds__(256) void rm_topo_local_kernel(SparseGrid g, const uint8_t* __restrict__ occ, uint32_t* __restrict__ parent) {
    __shared__ uint8_t s_cls[kTopoBrickPoints];
    __shared__ uint32_t s_lab[kTopoBrickPoints];
    const SparseBrick B = sparse_brick(g, blockIdx.x);
    TopoPoint t[2];
    uint32_t l[2], c[2];
#pragma unroll
    for (uint32_t h = 0; h < 2u; h++) {
        t[h] = topo_point(g, B, h);
        l[h] = t[h].il + kBrick * (t[h].jl + kBrick * t[h].kl);
        c[h] = t[h].valid ? (occ[t[h].p] != 0u ? 1u : 0u) : 2u;
        s_cls[l[h]] = (uint8_t)c[h];
        s_lab[l[h]] = l[h];
    }
    __syncthreads();
    // Every label is a member of the same component with an index <= its point's, so the labels form a forest.  A round that
    // changes anything lowers at least one label, and a component's smallest label travels at least one point per round: at
    // most kTopoBrickPoints rounds.
    for (uint32_t round = 0; round < kTopoBrickPoints; round++) {
        int changed = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
            if (c[h] == 2u) continue;
            const uint32_t cur = s_lab[l[h]];
            const uint32_t m = topo_local_min(s_cls, s_lab, t[h].il, t[h].jl, t[h].kl, c[h], cur);
            if (m < cur) {
                atomicMin(&s_lab[cur], m);  // hook the tree of `cur` below the smaller neighbour
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
        // pointer jumping: every label to the root of its tree (a root stays one during this phase; a label read while another
        // thread replaces it is the old or the new ancestor)
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
            if (c[h] == 2u) continue;
            uint32_t r = s_lab[l[h]];
            for (uint32_t n = 0; n < kTopoBrickPoints; n++) {
                const uint32_t up = s_lab[r];
                if (up == r) break;
                r = up;
            }
            s_lab[l[h]] = r;
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t h = 0; h < 2u; h++) {
        if (c[h] == 2u) continue;
        const uint32_t r = s_lab[l[h]];
        parent[t[h].p] = topo_index(g, B.i0 + (r & 7u), B.j0 + ((r >> 3) & 7u), B.k0 + (r >> 6));
    }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------
// topo_find, topo_unite and topo_for_preceding live in rm_topo_union.h (included above), written in two memory primitives --
// topo_load, a relaxed agent-scope load, and topo_fetch_min, atomicMin returning the old value -- so that the same three functions
// also run on CPU threads in tests/cpp/topo_union_model.cpp.
__global__ __launch_bounds__(256) void rm_topo_merge_kernel(SparseGrid g, const uint8_t* __restrict__ occ, uint32_t* parent) {
    const SparseBrick B = sparse_brick(g, blockIdx.x);
    const uint32_t bound = g.nx * g.ny * g.nz;
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const TopoPoint t = topo_point(g, B, half);
        if (!t.valid) continue;
        if (t.il != 0u && t.il != 7u && t.jl != 0u && t.jl != 7u && t.kl != 0u) continue;  // every preceding neighbour is in this brick
        const bool c = occ[t.p] != 0u;
        // Most of a point's neighbours across a face hang below one parent (their brick's local root): two neighbours with the
        // same parent -- read whenever -- are in one component, so the second union would change nothing and is not attempted.
        uint32_t mine = t.p, last = kTopoExterior;  // (no index: indices stay below 2^28)
        topo_for_preceding(g, t.i, t.j, t.k, c, [&](uint32_t qi, uint32_t qj, uint32_t qk) {
            if ((((qi ^ t.i) | (qj ^ t.j) | (qk ^ t.k)) >> 3) == 0u) return;  // the same brick: the local pass has united them
            const uint32_t q = topo_index(g, qi, qj, qk);
            if ((occ[q] != 0u) != c) return;
            const uint32_t up = topo_load(parent + q);
            if (up == last) return;
            last = up;
            mine = topo_find<true>(parent, mine, bound);  // (an ancestor of t.p: the walk continues where the last one ended)
            topo_unite(parent, mine, up, bound);
        });
    }
}

// ---- flatten and verify -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_topo_flatten_kernel(uint32_t n, uint32_t* parent) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = topo_find<false>(parent, p, n);
    __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (others walk through p meanwhile)
}

// rows[16 b + 4]: the pairs (p, preceding same-class neighbour) of brick b's points whose roots differ, after flatten.
__global__ __launch_bounds__(256) void rm_topo_verify_kernel(SparseGrid g, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                                             unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[4];
    const SparseBrick B = sparse_brick(g, blockIdx.x);
    uint32_t bad = 0u;
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const TopoPoint t = topo_point(g, B, half);
        if (!t.valid) continue;
        const bool c = occ[t.p] != 0u;
        const uint32_t r = parent[t.p];
        topo_for_preceding(g, t.i, t.j, t.k, c, [&](uint32_t qi, uint32_t qj, uint32_t qk) {
            const uint32_t q = topo_index(g, qi, qj, qk);
            if ((occ[q] != 0u) == c && parent[q] != r) bad++;
        });
    }
    block_row<12, 12, 12, 12, 16>((unsigned long long)bad << 48, wred, rows);  // entry 4, the 16-bit field: at most 13 x 512 per brick
}

// ---- exterior ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_topo_exterior_kernel(SparseGrid g, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                                               uint8_t* __restrict__ ext) {
    const SparseBrick B = sparse_brick(g, blockIdx.x);
    if (B.bi != 0u && B.bj != 0u && B.bk != 0u && B.bi + 1u != g.bx && B.bj + 1u != g.by && B.bk + 1u != g.bz) return;
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const TopoPoint t = topo_point(g, B, half);
        if (!t.valid) continue;
        const bool border = t.i == 0u || t.j == 0u || t.k == 0u || t.i + 1u == g.nx || t.j + 1u == g.ny || t.k + 1u == g.nz;
        if (border && occ[t.p] == 0u) ext[parent[t.p]] = 1u;
    }
}

// ---- numbering --------------------------------------------------------------------------------------------------------------
// 1 for the root of a body, 1 << 32 for the root of a cavity, 0 otherwise.
RM_DEV unsigned long long topo_root_flag(uint32_t p, uint32_t n, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                         const uint8_t* __restrict__ ext) {
    if (p >= n || parent[p] != p) return 0ull;
    return occ[p] != 0u ? 1ull : ext[p] != 0u ? 0ull : 1ull << 32;
}
__global__ __launch_bounds__(256) void rm_topo_root_sum_kernel(uint32_t n, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                                               const uint8_t* __restrict__ ext, unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    unsigned long long s = 0ull;
#pragma unroll
    for (uint32_t m = 0; m < kTopoRankPer; m++) s += topo_root_flag(blockIdx.x * kTopoRankBlock + m * 256u + threadIdx.x, n, occ, parent, ext);
    unsigned long long total;
    (void)block_exclusive_sum<4>(s, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
// labels[root] = its body's number, kTopoCavityBit | its cavity's number, or kTopoExterior.
__global__ __launch_bounds__(256) void rm_topo_rank_kernel(uint32_t n, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                                           const uint8_t* __restrict__ ext, const unsigned long long* __restrict__ block_offsets,
                                                           uint32_t* __restrict__ labels) {
    __shared__ unsigned long long wsum[4];
    unsigned long long off = block_offsets[blockIdx.x];
    for (uint32_t m = 0; m < kTopoRankPer; m++) {  // 8 rounds of 256 consecutive points
        const uint32_t p = blockIdx.x * kTopoRankBlock + m * 256u + threadIdx.x;
        const unsigned long long f = topo_root_flag(p, n, occ, parent, ext);
        unsigned long long total;
        const unsigned long long before = off + block_exclusive_sum<4>(f, wsum, total);
        if (p < n && parent[p] == p)
            labels[p] = f == 1ull ? (uint32_t)before : f != 0ull ? kTopoCavityBit | (uint32_t)(before >> 32) : kTopoExterior;
        off += total;
    }
}

// ---- rows and counts --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_topo_rows_init_kernel(uint32_t n_rows, unsigned long long* __restrict__ rows) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_rows * kRowWords) rows[w] = row_identity(w & 15u);
}

// comp_rows: the bodies' rows, then the cavities' (n_bodies rows before them).  count_rows[16 b]: V, E, F, K and the exterior's
// points among brick b's points.
__global__ __launch_bounds__(256) void rm_topo_rows_kernel(SparseGrid g, const uint8_t* __restrict__ occ, const uint32_t* __restrict__ parent,
                                                           uint32_t* labels, uint32_t n_bodies, unsigned long long* comp_rows,
                                                           unsigned long long* __restrict__ count_rows) {
    __shared__ unsigned long long wred[4];
    const SparseBrick B = sparse_brick(g, blockIdx.x);
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long counts = 0ull;
#pragma unroll 1
    for (uint32_t half = 0; half < 2u; half++) {
        const TopoPoint t = topo_point(g, B, half);  // (t.kl and t.k are uniform over the wave)
        uint32_t lab = kTopoExterior;
        if (t.valid) {
            const uint32_t root = parent[t.p];
            lab = labels[root];  // roots hold their labels since the rank pass; only other points are written here
            if (root != t.p) labels[t.p] = lab;
            const auto at = [&](uint32_t di, uint32_t dj, uint32_t dk) -> uint32_t {
                const uint32_t qi = t.i + di, qj = t.j + dj, qk = t.k + dk;
                return qi < g.nx && qj < g.ny && qk < g.nz && occ[topo_index(g, qi, qj, qk)] != 0u ? 1u : 0u;
            };
            const uint32_t c = at(0, 0, 0);
            if (c) {
                const uint32_t x = at(1, 0, 0), y = at(0, 1, 0), z = at(0, 0, 1);
                const uint32_t xy = x & y & at(1, 1, 0), yz = y & z & at(0, 1, 1), xz = x & z & at(1, 0, 1);
                const uint32_t cube = xy & yz & xz & at(1, 1, 1);
                counts += 1ull | (unsigned long long)(x + y + z) << 12 | (unsigned long long)(xy + yz + xz) << 24 | (unsigned long long)cube << 36;
            } else if (lab == kTopoExterior) {
                counts += 1ull << 48;
            }
        }
        // the moments of this plane's points, per distinct label: brick-local sums (each below 2^16: at most 64 points with
        // coordinates 0..7), two to a word, shifted to lattice coordinates once in u64
        bool active = lab != kTopoExterior;
        unsigned long long pending = __ballot(active);
        while (pending != 0ull) {  // at most 64 rounds: each retires its leader
            const uint32_t key = __shfl(lab, (int)__builtin_ctzll(pending), 64);
            const bool mine = active && lab == key;
            const uint32_t cnt = mine ? 1u : 0u;
            uint32_t w0 = cnt | (t.il * cnt) << 16;                        // count, sum l
            uint32_t w1 = (t.jl * cnt) | (t.il * t.il * cnt) << 16;        // sum m, sum l^2
            uint32_t w2 = (t.jl * t.jl * cnt) | (t.il * t.jl * cnt) << 16;  // sum m^2, sum l m
            uint32_t w3 = mine ? (1u << t.il) | (1u << (8u + t.jl)) : 0u;   // which l, m occur
            w0 = wave_sum(w0); w1 = wave_sum(w1); w2 = wave_sum(w2);
            w3 = wave_or(w3);
            if (lane < kRowWords) {  // lane e: entry e of the row
                const unsigned long long n = w0 & 0xFFFFu, sl = w0 >> 16, sm = w1 & 0xFFFFu, sll = w1 >> 16, smm = w2 & 0xFFFFu, slm = w2 >> 16;
                const unsigned long long i0 = B.i0, j0 = B.j0, k = t.k;
                const unsigned long long sx = i0 * n + sl, sy = j0 * n + sm;
                const uint32_t bl = w3 & 0xFFu, bm = (w3 >> 8) & 0xFFu;
                unsigned long long v;
                switch (lane) {
                    case 0: v = n; break;
                    case 1: v = sx; break;
                    case 2: v = sy; break;
                    case 3: v = k * n; break;
                    case 4: v = i0 * i0 * n + 2ull * i0 * sl + sll; break;
                    case 5: v = j0 * j0 * n + 2ull * j0 * sm + smm; break;
                    case 6: v = k * k * n; break;
                    case 7: v = i0 * j0 * n + i0 * sm + j0 * sl + slm; break;
                    case 8: v = k * sy; break;
                    case 9: v = k * sx; break;
                    case 10: v = i0 + (uint32_t)__builtin_ctz(bl | 0x100u); break;
                    case 11: v = j0 + (uint32_t)__builtin_ctz(bm | 0x100u); break;
                    case 13: v = i0 + (31u - (uint32_t)__builtin_clz(bl | 1u)); break;
                    case 14: v = j0 + (31u - (uint32_t)__builtin_clz(bm | 1u)); break;
                    default: v = k; break;  // 12, 15
                }
                const size_t row = (key & kTopoCavityBit) ? (size_t)n_bodies + (key & ~kTopoCavityBit) : (size_t)key;
                unsigned long long* dst = comp_rows + row * kRowWords + lane;
                if (lane < 10u) atomicAdd(dst, v);
                else if (lane < 13u) atomicMin(dst, v);
                else atomicMax(dst, v);
            }
            active = active && !mine;
            pending = __ballot(active);
        }
    }
    // a brick has 512 points, each counted at most 1, 3, 3 and 1 time in the fields of 12 bits and once in the last, of 16
    block_row<12, 12, 12, 12, 16>(counts, wred, count_rows);
}

}  // namespace rmk
