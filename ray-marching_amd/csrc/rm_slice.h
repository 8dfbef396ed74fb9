// rm_slice.h -- slicing (rm_slice_contours): the level set of the scene in a stack of parallel planes, as ordered contour
// loops.  Included by rm_abi.hip alone, after rm_mesh.h: neither the draw kernels nor the specialiser's embedded headers
// change.
//
// The contract pins every bit of the output, so a CPU restatement can compare arrays exactly:
//   point (i, j) of layer k lies at (ou + (float)i * su, ov + (float)j * sv) on the in-plane axes u = (w + 1) % 3 and
//   v = (w + 2) % 3 and at heights[k] on the slicing axis w; its value is query_distance; inside iff d < level (NaN
//   outside); one vertex per in-plane lattice edge whose ends differ, at t = (da - level) / (da - db), ordered by (layer,
//   i + nu * j, axis); per cell the directed segments of the case table below (the inside on the left seen from +w); the
//   segments chain into contours, an open one started at the vertex no segment ends at, a closed one at its lowest
//   vertex; contours ordered by layer and then by their first vertex.
// A batch of layers is processed as: distances, count + scan (a vertex base per point), links (next / prev per vertex),
// two list rankings by pointer doubling (the lowest vertex of each loop; then first vertex and rank of every vertex), a
// compaction of the first vertices (the contours), a scan of their lengths (the point offsets), and a last pass over the
// lattice that computes each vertex and writes it where its contour and rank put it.  Every order is fixed by the
// lattice and every slot has one writer: no atomics, identical runs.
#pragma once
#include "rm_mesh.h"

namespace rmk {

// ---- the square case table (host and device) ---------------------------------------------------------------------------
// Corner c (0..3) of a cell sits at (c & 1, c >> 1) in (u, v).  Edge e (0..3) runs along in-plane axis e >> 1 from the
// corner with 0 on it; e & 1 is its offset on the other axis: 0 bottom, 1 top, 2 left, 3 right.  Case = sum of
// inside(c) << c.  Two crossing edges give one segment; four (the diagonal cases 6 and 9) one segment around each inside
// corner, so inside corners are never joined across a cell.  A segment is directed so that its inside corner lies on its
// left seen from +w ((u, v, w) is right-handed: u to the right, v up).  Words per case: [0] the segment count, then
// (tail edge, head edge) pairs ordered by tail edge, 0xFFFFFFFF after the last.
constexpr int kSliceCaseWords = 5;
struct SliceCaseTable {
    uint32_t w[16 * kSliceCaseWords];
    bool ok;  // every segment had its inside corner strictly on one side
};

// corner index of end `end` (0 or 1) of edge e
constexpr int slice_edge_corner(int e, int end) {
    const int a = e >> 1;
    return (end << a) | ((e & 1) << (1 - a));
}
// doubled coordinate of the midpoint of edge e on in-plane axis f
constexpr int slice_edge_mid2(int e, int f) { return (e >> 1) == f ? 1 : 2 * (e & 1); }

constexpr SliceCaseTable make_slice_case_table() {
    SliceCaseTable T{};
    T.ok = true;
    for (int cs = 0; cs < 16; cs++) {
        uint32_t* out = T.w + cs * kSliceCaseWords;
        for (int k = 0; k < kSliceCaseWords; k++) out[k] = 0xFFFFFFFFu;
        int ce[4] = {}, nc = 0;  // crossing edges
        for (int e = 0; e < 4; e++)
            if (((cs >> slice_edge_corner(e, 0)) & 1) != ((cs >> slice_edge_corner(e, 1)) & 1)) ce[nc++] = e;
        int seg[2][3] = {};  // (edge, edge, an inside corner the segment bounds)
        int ns = 0;
        for (int c = 0; c < 4 && nc > 0; c++) {
            if (!((cs >> c) & 1)) continue;
            if (nc == 2) {
                seg[0][0] = ce[0]; seg[0][1] = ce[1]; seg[0][2] = c;
                ns = 1;
                break;
            }
            // four crossings: the two edges at this inside corner
            int at[2] = {}, na = 0;
            for (int q = 0; q < 4; q++)
                if (slice_edge_corner(ce[q], 0) == c || slice_edge_corner(ce[q], 1) == c) at[na++] = ce[q];
            if (na != 2 || ns == 2) { T.ok = false; break; }
            seg[ns][0] = at[0]; seg[ns][1] = at[1]; seg[ns][2] = c;
            ns++;
        }
        if (ns != nc / 2) T.ok = false;
        int tail[2] = {}, head[2] = {};
        for (int q = 0; q < ns; q++) {
            const int ax = slice_edge_mid2(seg[q][0], 0), ay = slice_edge_mid2(seg[q][0], 1);
            const int bx = slice_edge_mid2(seg[q][1], 0), by = slice_edge_mid2(seg[q][1], 1);
            const int px = 2 * (seg[q][2] & 1), py = 2 * (seg[q][2] >> 1);
            const int side = (bx - ax) * (py - ay) - (by - ay) * (px - ax);  // > 0: the corner is on the left of a -> b
            if (side == 0) T.ok = false;
            tail[q] = side > 0 ? seg[q][0] : seg[q][1];
            head[q] = side > 0 ? seg[q][1] : seg[q][0];
        }
        if (ns == 2 && tail[1] < tail[0]) {
            const int t = tail[0], h = head[0];
            tail[0] = tail[1]; head[0] = head[1];
            tail[1] = t; head[1] = h;
        }
        if (ns == 2 && (tail[0] == tail[1] || head[0] == head[1])) T.ok = false;
        out[0] = (uint32_t)ns;
        for (int q = 0; q < ns; q++) {
            out[1 + 2 * q] = (uint32_t)tail[q];
            out[2 + 2 * q] = (uint32_t)head[q];
        }
    }
    return T;
}

// The device's form: one word per case, the count in bits 0-1, then 2 bits each for tail and head of the segments.
struct SliceCasesPacked { uint32_t c[16]; };
constexpr SliceCasesPacked pack_slice_cases(const SliceCaseTable& T) {
    SliceCasesPacked P{};
    for (int cs = 0; cs < 16; cs++) {
        const uint32_t* w = T.w + cs * kSliceCaseWords;
        uint32_t v = w[0];
        for (uint32_t k = 0; k < 2u * w[0]; k++) v |= w[1 + k] << (2 + 2 * k);
        P.c[cs] = v;
    }
    return P;
}

constexpr SliceCaseTable kSliceCaseTable = make_slice_case_table();
static_assert(kSliceCaseTable.ok, "the case-table rule must orient every segment");
__constant__ SliceCasesPacked kSliceCases = pack_slice_cases(kSliceCaseTable);

// ---- lattice -------------------------------------------------------------------------------------------------------------
// Lattice points a batch of layers may hold (whole layers; a layer has at most 2^26): the scratch per point is 8 bytes
// (distance, packed vertex base), so a batch's point scratch stays within 1 GiB whatever the number of layers.
constexpr uint32_t kSliceBatchPoints = 1u << 27;
constexpr uint32_t kSliceNil = 0xFFFFFFFFu;
// The packed word of a point: bits 0-27 the id (within the batch) of its first vertex -- a batch has fewer than 2^28 --,
// bit 28 / 29 whether its edge along u / v carries one, bit 30 inside.
constexpr uint32_t kSliceBaseMask = (1u << 28) - 1u;
constexpr uint32_t kSliceBlock = 1024u;  // elements per workgroup of the scans: 4 per lane, 256 apart (coalesced)

struct SliceGrid {
    float ou, ov, su, sv;
    uint32_t nu, nv, n2;  // n2 = nu * nv <= 2^26
    uint32_t axis;        // w: 0, 1 or 2
    uint32_t k0;          // first layer of the batch
    uint32_t n;           // lattice points of the batch: layers * n2 <= kSliceBatchPoints
};

struct SlicePoint { uint32_t layer, i, j; };
RM_DEV SlicePoint slice_point(const SliceGrid& g, uint32_t p) {
    SlicePoint s;
    s.layer = p / g.n2;
    const uint32_t q = p - s.layer * g.n2;
    s.j = q / g.nu;
    s.i = q - s.j * g.nu;
    return s;
}

// map_scene at every lattice point of the batch, one lane per point: rm_grid_dist_kernel with the position permuted
template <int LOOP>
__global__ __launch_bounds__(256) void rm_slice_dist_kernel(QueryLaunch Q, SliceGrid g, const float* __restrict__ heights,
                                                            float* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.n) return;
    float* spill = query_spill(Q.slots);
    const SlicePoint s = slice_point(g, p);
    const float cu = grid_coord(g.ou, s.i, g.su), cv = grid_coord(g.ov, s.j, g.sv), h = heights[g.k0 + s.layer];
    const float x = g.axis == 0u ? h : g.axis == 1u ? cv : cu;
    const float y = g.axis == 0u ? cu : g.axis == 1u ? h : cv;
    const float z = g.axis == 0u ? cv : g.axis == 1u ? cu : h;
    out[p] = query_distance<LOOP>(Q, spill, x, y, z);
}

// bit 0 / 1: the edge from p along u / v carries a vertex; bit 2: p is inside.  p < g.n.
RM_DEV uint32_t slice_crossings(const SliceGrid& g, float level, const float* __restrict__ dist, uint32_t p) {
    const SlicePoint s = slice_point(g, p);
    const bool in = dist[p] < level;
    uint32_t f = in ? 4u : 0u;
    if (s.i + 1u < g.nu && (dist[p + 1u] < level) != in) f |= 1u;
    if (s.j + 1u < g.nv && (dist[p + g.nu] < level) != in) f |= 2u;
    return f;
}

// ---- scans ---------------------------------------------------------------------------------------------------------------
// A scan of n values is three launches: the sum of each block of kSliceBlock values, rm_slice_scan_kernel over the block
// sums, and the block's own scan redone on top of its offset.
template <class F>
RM_DEV void slice_block_sum(uint32_t n, uint32_t* __restrict__ sums, uint32_t* wsum, F value) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t idx = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        if (idx < n) s += value(idx);
    }
    uint32_t total;
    (void)block_exclusive_sum<4>(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
template <class F, class G>
RM_DEV void slice_block_scan(uint32_t n, const uint32_t* __restrict__ offsets, uint32_t* wsum, F value, G emit) {
    uint32_t carry = offsets[blockIdx.x];
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t idx = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        const uint32_t v = idx < n ? value(idx) : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_exclusive_sum<4>(v, wsum, total);
        if (idx < n) emit(idx, ex);
        carry += total;
    }
}

// The block sums -> exclusive offsets, in place, by one 1024-thread workgroup; *total = the sum of all.
__global__ __launch_bounds__(1024) void rm_slice_scan_kernel(uint32_t* __restrict__ sums, uint32_t n_blocks,
                                                             uint32_t* __restrict__ total_out) {
    __shared__ uint32_t wsum[16];
    const uint32_t per = (n_blocks + 1023u) / 1024u, b0 = min(threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    uint32_t s = 0;
    for (uint32_t b = b0; b < b1; b++) s += sums[b];
    uint32_t total;
    uint32_t off = block_exclusive_sum<16>(s, wsum, total);
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t v = sums[b];
        sums[b] = off;
        off += v;
    }
    if (threadIdx.x == 0) *total_out = total;
}

// ---- vertices: count, scan, pack -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_slice_count_kernel(SliceGrid g, float level, const float* __restrict__ dist,
                                                             uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    slice_block_sum(g.n, sums, wsum, [&](uint32_t p) { return (uint32_t)__builtin_popcount(slice_crossings(g, level, dist, p) & 3u); });
}

__global__ __launch_bounds__(256) void rm_slice_pack_kernel(SliceGrid g, float level, const float* __restrict__ dist,
                                                            const uint32_t* __restrict__ offsets, uint32_t* __restrict__ packed) {
    __shared__ uint32_t wsum[4];
    uint32_t carry = offsets[blockIdx.x];
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t p = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        const uint32_t f = p < g.n ? slice_crossings(g, level, dist, p) : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_exclusive_sum<4>((uint32_t)__builtin_popcount(f & 3u), wsum, total);
        if (p < g.n) packed[p] = ex | f << 28;
        carry += total;
    }
}

// out[l] = the id of the first vertex of layer l of the batch (l < layers); out[layers] = the batch's vertex count
__global__ __launch_bounds__(256) void rm_slice_layer_base_kernel(const uint32_t* __restrict__ packed, uint32_t n2, uint32_t layers,
                                                                  const uint32_t* __restrict__ n_vertices, uint32_t* __restrict__ out) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l < layers) out[l] = packed[l * n2] & kSliceBaseMask;
    else if (l == layers) out[l] = *n_vertices;
}

// ---- links -----------------------------------------------------------------------------------------------------------------
// One lane per cell: next[tail] = head and prev[head] = tail for each segment of its case.  Both arrays come filled with
// kSliceNil; every slot has one writer (a vertex is the tail of at most one segment and the head of at most one).
__global__ __launch_bounds__(256) void rm_slice_link_kernel(SliceGrid g, const uint32_t* __restrict__ packed,
                                                            uint32_t* __restrict__ next, uint32_t* __restrict__ prev) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.n) return;
    const SlicePoint s = slice_point(g, p);
    if (s.i + 1u >= g.nu || s.j + 1u >= g.nv) return;  // no cell: a corner would be off the layer
    const uint32_t w00 = packed[p], w10 = packed[p + 1u], w01 = packed[p + g.nu], w11 = packed[p + g.nu + 1u];
    const uint32_t cs = ((w00 >> 30) & 1u) | ((w10 >> 30) & 1u) << 1 | ((w01 >> 30) & 1u) << 2 | ((w11 >> 30) & 1u) << 3;
    const uint32_t tab = kSliceCases.c[cs], cnt = tab & 3u;
    if (cnt == 0u) return;
    // the vertex on each edge of the cell: bottom, top (the u-edges of (i, j) and (i, j + 1)), left, right (the v-edges of
    // (i, j) and (i + 1, j), behind the point's u-edge vertex when it has one)
    const uint32_t ev[4] = {w00 & kSliceBaseMask, w01 & kSliceBaseMask, (w00 & kSliceBaseMask) + ((w00 >> 28) & 1u),
                            (w10 & kSliceBaseMask) + ((w10 >> 28) & 1u)};
#pragma unroll
    for (uint32_t q = 0; q < 2u; q++) {
        if (q < cnt) {
            const uint32_t te = (tab >> (2u + 4u * q)) & 3u, he = (tab >> (4u + 4u * q)) & 3u;
            const uint32_t t = te == 0u ? ev[0] : te == 1u ? ev[1] : te == 2u ? ev[2] : ev[3];
            const uint32_t h = he == 0u ? ev[0] : he == 1u ? ev[1] : he == 2u ? ev[2] : ev[3];
            next[t] = h;
            prev[h] = t;
        }
    }
}

// ---- ranking by pointer doubling -------------------------------------------------------------------------------------------
// Pass 1, state (jump, low) per vertex: jump = next applied 2^r times (kSliceNil once the chain has ended), low = the lowest
// id among the vertex and the 2^r - 1 that follow it.  After rounds with 2^r >= the longest chain, a vertex of a closed
// loop holds the loop's lowest id and a vertex of an open chain has jump = kSliceNil.  Each round reads one buffer and
// writes the other.
__global__ __launch_bounds__(256) void rm_slice_low_init_kernel(const uint32_t* __restrict__ next, uint32_t n_vertices,
                                                                uint2* __restrict__ out) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n_vertices) out[v] = make_uint2(next[v], v);
}
__global__ __launch_bounds__(256) void rm_slice_low_round_kernel(const uint2* __restrict__ in, uint32_t n_vertices,
                                                                 uint2* __restrict__ out) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    uint2 a = in[v];
    if (a.x != kSliceNil) {
        const uint2 b = in[a.x];
        a.y = min(a.y, b.y);
        a.x = b.x;
    }
    out[v] = a;
}
// The cut: a closed loop is opened before its lowest vertex.  start[v]: bit 0 the vertex is the first of its contour, bit 1
// the contour is closed.  Pass 2 starts from (first known ancestor, distance to it) = (prev, 1), or (v, 0) for a first vertex.
__global__ __launch_bounds__(256) void rm_slice_cut_kernel(const uint2* __restrict__ low, const uint32_t* __restrict__ prev,
                                                           uint32_t n_vertices, uint32_t* __restrict__ start, uint2* __restrict__ rank) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    const uint2 a = low[v];
    const uint32_t pv = prev[v];
    const bool closed = a.x != kSliceNil, first = closed ? a.y == v : pv == kSliceNil;
    start[v] = (first ? 1u : 0u) | (closed ? 2u : 0u);
    rank[v] = first ? make_uint2(v, 0u) : make_uint2(pv, 1u);
}
// Pass 2, state (ancestor, distance): a first vertex is its own ancestor at distance 0, so a round needs no end test.
__global__ __launch_bounds__(256) void rm_slice_rank_round_kernel(const uint2* __restrict__ in, uint32_t n_vertices,
                                                                  uint2* __restrict__ out) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    const uint2 a = in[v], b = in[a.x];
    out[v] = make_uint2(b.x, a.y + b.y);
}

// ---- contours --------------------------------------------------------------------------------------------------------------
// The first vertices compacted in id order: start[v] becomes (first vertices below v) << 2 | its two bits, which for a
// first vertex is its contour's index in the batch.
__global__ __launch_bounds__(256) void rm_slice_start_count_kernel(const uint32_t* __restrict__ start, uint32_t n_vertices,
                                                                   uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    slice_block_sum(n_vertices, sums, wsum, [&](uint32_t v) { return start[v] & 1u; });
}
__global__ __launch_bounds__(256) void rm_slice_start_scan_kernel(uint32_t* __restrict__ start, uint32_t n_vertices,
                                                                  const uint32_t* __restrict__ offsets) {
    __shared__ uint32_t wsum[4];
    slice_block_scan(n_vertices, offsets, wsum, [&](uint32_t v) { return start[v] & 1u; },
                     [&](uint32_t v, uint32_t ex) { start[v] = ex << 2 | (start[v] & 3u); });
}
// The last vertex of each chain (nothing follows it, or its contour's first vertex does) supplies the length.
__global__ __launch_bounds__(256) void rm_slice_length_kernel(const uint2* __restrict__ rank, const uint32_t* __restrict__ next,
                                                              const uint32_t* __restrict__ start, uint32_t n_vertices,
                                                              uint32_t* __restrict__ length) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    const uint2 r = rank[v];
    const uint32_t nx = next[v];
    if (nx == kSliceNil || nx == r.x) length[start[r.x] >> 2] = r.y + 1u;
}
__global__ __launch_bounds__(256) void rm_slice_length_count_kernel(const uint32_t* __restrict__ length, uint32_t n_contours,
                                                                    uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    slice_block_sum(n_contours, sums, wsum, [&](uint32_t c) { return length[c]; });
}
__global__ __launch_bounds__(256) void rm_slice_length_scan_kernel(const uint32_t* __restrict__ length, uint32_t n_contours,
                                                                   const uint32_t* __restrict__ offsets, uint32_t* __restrict__ first_point) {
    __shared__ uint32_t wsum[4];
    slice_block_scan(n_contours, offsets, wsum, [&](uint32_t c) { return length[c]; },
                     [&](uint32_t c, uint32_t ex) { first_point[c] = ex; });
}
// layer_first[k0 + l] = contour_base + the contours of the batch's layers below l (l <= layers): the first vertices below
// the layer's first vertex id.
__global__ __launch_bounds__(256) void rm_slice_layer_first_kernel(const uint32_t* __restrict__ layer_base, uint32_t layers,
                                                                   uint32_t n_vertices, const uint32_t* __restrict__ start,
                                                                   uint32_t n_contours, uint32_t contour_base,
                                                                   uint32_t* __restrict__ layer_first) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l > layers) return;
    const uint32_t vb = l < layers ? layer_base[l] : n_vertices;
    layer_first[l] = contour_base + (vb < n_vertices ? start[vb] >> 2 : n_contours);
}

// One lane per lattice point: the vertices on its two edges, by the mesh's rule, each written where its contour and rank
// put it; a contour's first vertex also writes the contour's record (first point, points, layer, closed).
__global__ __launch_bounds__(256) void rm_slice_emit_kernel(SliceGrid g, float level, const float* __restrict__ dist,
                                                            const float* __restrict__ heights, const uint32_t* __restrict__ packed,
                                                            const uint2* __restrict__ rank, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ length, const uint32_t* __restrict__ first_point,
                                                            uint32_t point_base, uint32_t contour_base, float* __restrict__ points,
                                                            uint4* __restrict__ contours) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.n) return;
    const uint32_t w = packed[p];
    if (((w >> 28) & 3u) == 0u) return;
    const SlicePoint s = slice_point(g, p);
    const float cu = grid_coord(g.ou, s.i, g.su), cv = grid_coord(g.ov, s.j, g.sv), h = heights[g.k0 + s.layer];
    const float da = dist[p];
    uint32_t vid = w & kSliceBaseMask;
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++) {
        if (((w >> (28u + a)) & 1u) == 0u) continue;
        float pu = cu, pv = cv;
        if (a == 0u) {
            const float t = (da - level) / (da - dist[p + 1u]), ub = grid_coord(g.ou, s.i + 1u, g.su);
            pu = cu + t * (ub - cu);
        } else {
            const float t = (da - level) / (da - dist[p + g.nu]), vb = grid_coord(g.ov, s.j + 1u, g.sv);
            pv = cv + t * (vb - cv);
        }
        const uint2 r = rank[vid];
        const uint32_t c = start[r.x] >> 2, fp = first_point[c];
        float* o = points + 3u * ((size_t)point_base + fp + r.y);
        o[0] = g.axis == 0u ? h : g.axis == 1u ? pv : pu;
        o[1] = g.axis == 0u ? pu : g.axis == 1u ? h : pv;
        o[2] = g.axis == 0u ? pv : g.axis == 1u ? pu : h;
        if (r.y == 0u) contours[(size_t)contour_base + c] = make_uint4(point_base + fp, length[c], g.k0 + s.layer, (start[vid] >> 1) & 1u);
        vid++;
    }
}

}  // namespace rmk
