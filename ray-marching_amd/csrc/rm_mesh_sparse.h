// rm_mesh_sparse.h -- sparse mesh extraction (rm_extract_mesh_sparse): the mesh of rm_mesh.h, bit for bit and in the same
// order, evaluated only in the bricks the surface can reach.  Included by rm_abi.hip alone, after rm_mesh.h.
//
// The lattice is cut into bricks of 8 x 8 x 8 points.  A brick OWNS the edges that start at its points and the cells anchored
// there, so it READS a tile of 9 x 9 x 9 points (one layer of its neighbours; less at the lattice's border).  DESIGN.md
// section 15 proves the skipping rule; the passes:
//   probe    one lane per brick: map_scene at the tile's centre; the brick is kept unless |v - level| exceeds
//            L * radius + 2 E (L: the program's Lipschitz bound, E: the bound on the binary32 evaluation's error), in
//            which case every point of the tile is on the same side of `level`.  Block sums of the keep flags.
//   scan     rm_block_scan_kernel (rm_reduce.h), one workgroup: block sums -> offsets, the totals as 64-bit numbers.
//   compact  the kept bricks in linear order (klist), and for every brick the number of kept bricks before it (boff).
//   count    one workgroup per kept brick: the tile's distances (query_distance, the bit patterns the dense path computes)
//            into LDS and into the brick's tile in device memory; per row segment (the 8 points of the brick that share
//            j and k) one word: the crossing flags of its points (3 bits each) and its triangle count.
//   segment scans   the words lie in the order the dense mesh has -- k, then j, then i: within a slab of bricks (same bz) by
//            (k in brick, by, j in brick, bx) -- so a plain scan over them gives every segment's first vertex and triangle.
//   emit     one workgroup per kept brick, from the stored tile: the vertices of its points, and its cells' triangles; a
//            vertex on an edge that starts in a neighbour brick is looked up through that brick's segment words.
// Every order is fixed by the lattice.  The one atomic adds up a statistic (evaluations) and decides nothing.
#pragma once
#include "rm_mesh.h"
#include "rm_reduce.h"

namespace rmk {

constexpr uint32_t kBrick = 8u, kTile = kBrick + 1u, kTilePoints = kTile * kTile * kTile, kBrickSegs = kBrick * kBrick;
constexpr uint32_t kSegPer = 8u, kSegBlock = 256u * kSegPer;  // the segment scans: 2048 words per workgroup

struct SparseGrid {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz;
    uint32_t bx, by, bz;  // bricks per axis: ceil(n / 8)
    uint32_t nb;          // bx * by * bz (< 2^32 - 1)
};

// Where a kept brick's 64 segment words lie: word (kl, jl) at base + kl * stride_k + jl * stride_j.
struct SparseSegMap {
    uint32_t base, stride_k, stride_j, brick;
};

struct SparseBrick {
    uint32_t bi, bj, bk;  // the brick's coordinates
    uint32_t i0, j0, k0;  // its first point
    uint32_t ex, ey, ez;  // the tile's extent in points (<= 9: up to the lattice's last point)
};
RM_DEV SparseBrick sparse_brick(const SparseGrid& g, uint32_t b) {
    SparseBrick B;
    B.bi = b % g.bx;
    const uint32_t r = b / g.bx;
    B.bj = r % g.by;
    B.bk = r / g.by;
    B.i0 = B.bi * kBrick; B.j0 = B.bj * kBrick; B.k0 = B.bk * kBrick;
    B.ex = min(kTile, g.nx - B.i0); B.ey = min(kTile, g.ny - B.j0); B.ez = min(kTile, g.nz - B.k0);
    return B;
}

// ---- probe ------------------------------------------------------------------------------------------------------------------
// keep[b] (as a u32, scanned in place later) for the bricks [0, nb) and 0 for the extra entry nb; block sums of 256 entries.
// margin_scale = L, err2 = 2 E: both +inf when the program has no bound.
// The decision for brick b (< g.nb): true when it is kept; v is map_scene at the tile's centre.  Shared by the mesh's probe and
// the mass probe (rm_mass.h), so that both keep the same bricks.
template <int LOOP>
RM_DEV bool sparse_probe_brick(const QueryLaunch& Q, float* spill, const SparseGrid& g, const SparseBrick& B, float level, double L,
                               double err2, float& v) {
    // Lattice coordinates are monotone in the index (one rounded product, one rounded sum, step > 0), so every point of
    // the tile lies in the box of its first and last point as they are computed
    const float x0 = grid_coord(g.ox, B.i0, g.sx), x1 = grid_coord(g.ox, B.i0 + B.ex - 1u, g.sx);
    const float y0 = grid_coord(g.oy, B.j0, g.sy), y1 = grid_coord(g.oy, B.j0 + B.ey - 1u, g.sy);
    const float z0 = grid_coord(g.oz, B.k0, g.sz), z1 = grid_coord(g.oz, B.k0 + B.ez - 1u, g.sz);
    const float cx = x0 + (x1 - x0) * 0.5f, cy = y0 + (y1 - y0) * 0.5f, cz = z0 + (z1 - z0) * 0.5f;  // any point serves
    v = query_distance<LOOP>(Q, spill, cx, cy, cz);
    // the radius about the probe as it was computed, in binary64 (differences of binary32 numbers: exact or 2^-53 off)
    const double hx = fmax((double)x1 - (double)cx, (double)cx - (double)x0), hy = fmax((double)y1 - (double)cy, (double)cy - (double)y0),
                 hz = fmax((double)z1 - (double)cz, (double)cz - (double)z0);
    const double r = sqrt(hx * hx + hy * hy + hz * hz), reach = L * r;
    const double margin = (reach + err2) * (1.0 + 1.0e-9);
    // skipped only when proven clear: a NaN probe, an infinite bound, or an error term that is not small against
    // L * radius (steps near the coordinates' ulp) all keep the brick
    const bool clear = fabs((double)v - (double)level) > margin && err2 <= 0.5 * reach;
    return !clear;
}

template <int LOOP>
__global__ __launch_bounds__(256) void rm_sparse_probe_kernel(QueryLaunch Q, SparseGrid g, float level, double L, double err2,
                                                              uint32_t* __restrict__ keep, unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    static_assert(sizeof wsum <= rml::kQueryOwnBrick, "the static LDS the host counts in front of the query columns");
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    uint32_t k = 0u;
    if (b < g.nb) {
        float v;
        k = sparse_probe_brick<LOOP>(Q, query_spill(Q.slots), g, sparse_brick(g, b), level, L, err2, v) ? 1u : 0u;
    }
    if (b <= g.nb) keep[b] = k;
    unsigned long long total;
    (void)block_exclusive_sum<4>((unsigned long long)k, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// keep[] -> boff[] in place (kept bricks before b; entry nb: all of them) and the list of the kept bricks.
__global__ __launch_bounds__(256) void rm_sparse_compact_kernel(uint32_t n_entries, const unsigned long long* __restrict__ block_offsets,
                                                                uint32_t* __restrict__ boff, uint32_t* __restrict__ klist) {
    __shared__ uint32_t wsum[4];
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    const uint32_t k = b < n_entries ? boff[b] : 0u;
    uint32_t total;
    const uint32_t c = (uint32_t)block_offsets[blockIdx.x] + block_exclusive_sum<4>(k, wsum, total);
    if (b < n_entries) boff[b] = c;
    if (k) klist[c] = b;
}

// ---- the order of the segments ------------------------------------------------------------------------------------------------
// Kept brick c = boff[b].  With [s0, s1) the kept bricks of its slab (same bk) and [r0, r1) those of its row (same bj, bk),
// both contiguous in klist: the slab's words start at 64 s0; within the slab they are ordered by kl (8 (s1 - s0) words each),
// then by row (8 (r1 - r0) words each, the rows before it hold 8 (r0 - s0)), then by jl (r1 - r0 words each), then by brick.
RM_DEV SparseSegMap sparse_segmap(const SparseGrid& g, const uint32_t* __restrict__ boff, uint32_t b, uint32_t c) {
    const uint32_t row = b / g.bx, slab = row / g.by, per_slab = g.bx * g.by;
    const uint32_t r0 = boff[row * g.bx], r1 = boff[(row + 1u) * g.bx];
    const uint32_t s0 = boff[slab * per_slab], s1 = boff[(slab + 1u) * per_slab];
    SparseSegMap m;
    m.base = kBrickSegs * s0 + kBrick * (r0 - s0) + (c - r0);
    m.stride_k = kBrick * (s1 - s0);
    m.stride_j = r1 - r0;
    m.brick = b;
    return m;
}

// The flags (bits 0-2: crossing edges along x, y, z; bit 3: inside) and the cell's case entry of the brick's point
// (il, jl, kl), from the tile in LDS.  A point beyond the lattice has neither.
RM_DEV uint32_t sparse_point(const SparseGrid& g, const SparseBrick& B, const float* tile, float level, uint32_t il, uint32_t jl,
                             uint32_t kl, unsigned long long& entry) {
    entry = 0ull;
    if (B.i0 + il >= g.nx || B.j0 + jl >= g.ny || B.k0 + kl >= g.nz) return 0u;
    const uint32_t t = il + kTile * (jl + kTile * kl);
    const bool ex = B.i0 + il + 1u < g.nx, ey = B.j0 + jl + 1u < g.ny, ez = B.k0 + kl + 1u < g.nz;
    const bool in = tile[t] < level;
    uint32_t f = in ? (uint32_t)kMeshInside : 0u;
    f |= (ex && (tile[t + 1u] < level) != in) ? 1u : 0u;
    f |= (ey && (tile[t + kTile] < level) != in) ? 2u : 0u;
    f |= (ez && (tile[t + kTile * kTile] < level) != in) ? 4u : 0u;
    if (ex && ey && ez) {
        uint32_t cs = 0;
#pragma unroll
        for (uint32_t c = 0; c < 8u; c++)
            cs |= (tile[t + (c & 1u) + ((c >> 1) & 1u) * kTile + (c >> 2) * kTile * kTile] < level ? 1u : 0u) << c;
        entry = kMeshCases.c[cs];
    }
    return f;
}

// ---- count ------------------------------------------------------------------------------------------------------------------
// A segment's word: bits 3 il + a the crossing edge of point il along axis a; bits 24-31 the triangles of its 8 cells (<= 40).
template <int LOOP>
__global__ __launch_bounds__(256) void rm_sparse_count_kernel(QueryLaunch Q, SparseGrid g, float level, const uint32_t* __restrict__ boff,
                                                              const uint32_t* __restrict__ klist, float* __restrict__ tiles,
                                                              SparseSegMap* __restrict__ maps, uint32_t* __restrict__ seg_words,
                                                              unsigned long long* __restrict__ evaluations) {
    __shared__ float tile[kTilePoints];
    static_assert(sizeof tile <= rml::kQueryOwnBrick, "the static LDS the host counts in front of the query columns");
    const uint32_t c = blockIdx.x, b = klist[c];
    const SparseBrick B = sparse_brick(g, b);
    float* spill = query_spill(Q.slots);
    for (uint32_t t = threadIdx.x; t < kTilePoints; t += 256u) {
        const uint32_t ti = t % kTile, tj = (t / kTile) % kTile, tk = t / (kTile * kTile);
        float d = 0.0f;  // beyond the lattice: never read
        if (ti < B.ex && tj < B.ey && tk < B.ez)
            d = query_distance<LOOP>(Q, spill, grid_coord(g.ox, B.i0 + ti, g.sx), grid_coord(g.oy, B.j0 + tj, g.sy),
                                     grid_coord(g.oz, B.k0 + tk, g.sz));
        tile[t] = d;
        tiles[(size_t)c * kTilePoints + t] = d;
    }
    __syncthreads();
    const SparseSegMap m = sparse_segmap(g, boff, b, c);
    if (threadIdx.x == 0) {
        maps[c] = m;
        atomicAdd(evaluations, (unsigned long long)(B.ex * B.ey * B.ez));  // a statistic: no order depends on it
    }
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const uint32_t l = threadIdx.x + 256u * half, il = l & 7u, jl = (l >> 3) & 7u, kl = l >> 6;
        unsigned long long entry;
        const uint32_t f = sparse_point(g, B, tile, level, il, jl, kl, entry);
        uint32_t w = (f & 7u) << (3u * il) | (uint32_t)(entry & 15ull) << 24;  // disjoint fields: the sum is the union
        w = wave_sum<8>(w);
        if (il == 0u) seg_words[m.base + kl * m.stride_k + jl * m.stride_j] = w;
    }
}

// ---- segment scans ------------------------------------------------------------------------------------------------------------
RM_DEV unsigned long long sparse_seg_counts(uint32_t w) {
    return (unsigned long long)__builtin_popcount(w & 0xFFFFFFu) | (unsigned long long)(w >> 24) << 32;
}
__global__ __launch_bounds__(256) void rm_sparse_seg_sum_kernel(uint32_t n, const uint32_t* __restrict__ seg_words,
                                                                unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t m = 0; m < kSegPer; m++) {  // lane-strided: coalesced
        const uint32_t p = blockIdx.x * kSegBlock + m * 256u + threadIdx.x;
        if (p < n) s += sparse_seg_counts(seg_words[p]);
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>(s, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
// seg_first[p] = (vertices, triangles) before segment p
__global__ __launch_bounds__(256) void rm_sparse_seg_scan_kernel(uint32_t n, const uint32_t* __restrict__ seg_words,
                                                                 const unsigned long long* __restrict__ block_offsets,
                                                                 uint2* __restrict__ seg_first) {
    __shared__ unsigned long long wsum[4];
    const unsigned long long off = block_offsets[blockIdx.x];
    uint32_t v0 = (uint32_t)off, t0 = (uint32_t)(off >> 32);
    for (uint32_t m = 0; m < kSegPer; m++) {  // 8 rounds of 256 consecutive segments
        const uint32_t p = blockIdx.x * kSegBlock + m * 256u + threadIdx.x;
        const unsigned long long cnt = p < n ? sparse_seg_counts(seg_words[p]) : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_exclusive_sum<4>(cnt, wsum, total);
        if (p < n) seg_first[p] = make_uint2(v0 + (uint32_t)ex, t0 + (uint32_t)(ex >> 32));
        v0 += (uint32_t)total;
        t0 += (uint32_t)(total >> 32);
    }
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_sparse_emit_kernel(SparseGrid g, float level, uint32_t n_kept, const uint32_t* __restrict__ boff,
                                                             const uint32_t* __restrict__ klist, const float* __restrict__ tiles,
                                                             const SparseSegMap* __restrict__ maps, const uint32_t* __restrict__ seg_words,
                                                             const uint2* __restrict__ seg_first, float* __restrict__ vertices,
                                                             uint32_t* __restrict__ triangles) {
    __shared__ float tile[kTilePoints];
    __shared__ uint32_t s_word[kBrickSegs];
    __shared__ uint2 s_first[kBrickSegs];
    const uint32_t c = blockIdx.x, b = klist[c];
    const SparseBrick B = sparse_brick(g, b);
    const SparseSegMap m = maps[c];
    for (uint32_t t = threadIdx.x; t < kTilePoints; t += 256u) tile[t] = tiles[(size_t)c * kTilePoints + t];
    if (threadIdx.x < kBrickSegs) {
        const uint32_t p = m.base + (threadIdx.x >> 3) * m.stride_k + (threadIdx.x & 7u) * m.stride_j;
        s_word[threadIdx.x] = seg_words[p];
        s_first[threadIdx.x] = seg_first[p];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t half = 0; half < 2u; half++) {
        const uint32_t l = threadIdx.x + 256u * half, il = l & 7u, jl = (l >> 3) & 7u, kl = l >> 6, seg = l >> 3;
        unsigned long long entry;
        const uint32_t f = sparse_point(g, B, tile, level, il, jl, kl, entry);
        const uint32_t nt = (uint32_t)(entry & 15ull);
        // triangles before this cell within its segment: a scan over the 8 lanes of the segment
        uint32_t before = nt;
#pragma unroll
        for (uint32_t o = 1; o < 8u; o <<= 1) {
            const uint32_t y = __shfl_up(before, o, 8);
            if (il >= o) before += y;
        }
        before -= nt;
        if (f & 7u) {
            size_t v = (size_t)s_first[seg].x + (size_t)__builtin_popcount(s_word[seg] & ((1u << (3u * il)) - 1u));
            const uint32_t i = B.i0 + il, j = B.j0 + jl, k = B.k0 + kl, t = il + kTile * (jl + kTile * kl);
            const float x = grid_coord(g.ox, i, g.sx), y = grid_coord(g.oy, j, g.sy), z = grid_coord(g.oz, k, g.sz);
            const float da = tile[t];
            if (f & 1u) {
                const float tt = (da - level) / (da - tile[t + 1u]), xb = grid_coord(g.ox, i + 1u, g.sx);
                vertices[3u * v] = x + tt * (xb - x); vertices[3u * v + 1u] = y; vertices[3u * v + 2u] = z;
                v++;
            }
            if (f & 2u) {
                const float tt = (da - level) / (da - tile[t + kTile]), yb = grid_coord(g.oy, j + 1u, g.sy);
                vertices[3u * v] = x; vertices[3u * v + 1u] = y + tt * (yb - y); vertices[3u * v + 2u] = z;
                v++;
            }
            if (f & 4u) {
                const float tt = (da - level) / (da - tile[t + kTile * kTile]), zb = grid_coord(g.oz, k + 1u, g.sz);
                vertices[3u * v] = x; vertices[3u * v + 1u] = y; vertices[3u * v + 2u] = z + tt * (zb - z);
                v++;
            }
        }
        size_t tri = (size_t)s_first[seg].y + before;
        for (uint32_t n = 0; n < 3u * nt; n++) {
            const uint32_t e = (uint32_t)(entry >> (4u + 4u * n)) & 15u, a = e >> 2, lo = e & 1u, hi = (e >> 1) & 1u;
            // the edge's start point in the tile: offsets on the lower and the higher of the two other axes
            const uint32_t qi = il + (a == 0u ? 0u : lo), qj = jl + (a == 0u ? lo : a == 1u ? 0u : hi), qk = kl + (a == 2u ? 0u : hi);
            uint32_t word, first;
            if ((qi | qj | qk) < kBrick) {
                word = s_word[qk * kBrick + qj];
                first = s_first[qk * kBrick + qj].x;
            } else {
                // a neighbour's point: that brick holds a crossing edge, so it was kept (section 15); were it not, the index
                // written is 0xFFFFFFFF and nothing is read out of bounds
                const uint32_t nb = (B.bi + (qi >> 3)) + g.bx * ((B.bj + (qj >> 3)) + g.by * (B.bk + (qk >> 3)));
                const uint32_t nc = boff[nb];
                word = 0u;
                first = 0xFFFFFFFFu;
                if (nc < n_kept) {
                    const SparseSegMap nm = maps[nc];
                    if (nm.brick == nb) {
                        const uint32_t p = nm.base + (qk & 7u) * nm.stride_k + (qj & 7u) * nm.stride_j;
                        word = seg_words[p];
                        first = seg_first[p].x;
                    }
                }
            }
            triangles[3u * tri + n] = first + (uint32_t)__builtin_popcount(word & ((1u << (3u * (qi & 7u) + a)) - 1u));
        }
    }
}

}  // namespace rmk
