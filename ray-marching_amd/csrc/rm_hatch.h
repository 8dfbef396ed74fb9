// rm_hatch.h -- hatching (rm_hatch_slices): the retained slices filled, layer by layer, with parallel lines under the even-odd rule.
// Included by rm_abi.hip alone, after rm_mesh_slice.h (whose scan and item search run here as they are) and rm_sort.h.  DESIGN.md
// section 31 is the contract.  A SEGMENT is a contour segment, numbered by its tail point; a CROSSING is a (segment, line) pair
// with sA <= c_j < sB; crossings are enumerated by (segment, j) and sorted by (layer * n_lines + j, position along the line).
//   count    one lane per point: its contour by binary search, s of the segment's two ends, the lines [lb(sA), lb(sB)) by two
//            binary searches on c_j = offset + j * spacing (evaluated, never inverted); the block sums of the counts (64 bits: the
//            total may exceed 2^32, which the host refuses) and SEGMENTS_IN in rows
//   (scan)   rm_block_scan_kernel, rm_mslice_scan_kernel: cstart[i] = the crossings before segment i's own
//   items    one lane per crossing: its segment by binary search over cstart, the point, (key, value) = (L << 32 | key32, item)
//   (sort)   by key, stably
//   pair     one lane per sorted crossing: its rank in its line by a lower-bound search for L << 32 in the sorted keys; an even
//            rank with a partner is a HEAD (hstart = 1, to be scanned); LINES_HIT and ODD_LINES in rows
//   (scan)   as above: hstart[q] = the hatch segments before q's own, hstart[N] = H
//   emit     one lane per sorted crossing: a head writes its segment and line where hstart (and, zigzag, its line's range) puts it;
//            one lane per layer writes layer_first from the keys' boundaries
// Every slot has one writer and no atomic is used: identical runs.
#pragma once
#include "rm_abi_layout.h"
#include "rm_mesh_slice.h"
#include "rm_reduce.h"

namespace rmk {

struct HatchFrame {
    uint32_t u, v;  // the in-plane axes of the slices
    uint32_t n_points, n_contours, n_lines;
};

// The contour that holds point i: the last c with contours[c].x <= i (contours lie in the order of their first points; n > 0).
RM_DEV uint32_t hatch_contour(const uint4* __restrict__ contours, uint32_t n, uint32_t i) {
    uint32_t lo = 0u, hi = n;  // the first c in [0, n] with first point > i, never 0
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (contours[mid].x > i) hi = mid;
        else lo = mid + 1u;
    }
    return lo - 1u;
}

RM_DEV double hatch_s(const float* __restrict__ p, uint32_t u, uint32_t v, double dx, double dy) {
    return (double)p[v] * dx - (double)p[u] * dy;  // exact products, one rounded difference
}
RM_DEV double hatch_c(uint32_t j, double offset, double spacing) { return offset + (double)j * spacing; }  // exact product (j < 2^24)

// the first j in [0, n_lines] with c_j >= s (c is non-decreasing)
RM_DEV uint32_t hatch_lower(double s, double offset, double spacing, uint32_t n_lines) {
    uint32_t lo = 0u, hi = n_lines;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (hatch_c(mid, offset, spacing) >= s) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// Segment i: false when point i is the tail of none (the last point of an open contour); else its layer, the ends A (the smaller
// s) and B, and their s.  sA < sB is NOT checked here.
struct HatchSegment {
    uint32_t layer, a, b;
    double sa, sb, dx, dy, offset, spacing;
};
RM_DEV bool hatch_segment(const HatchFrame& f, const float* __restrict__ points, const uint4* __restrict__ contours,
                          const float4* __restrict__ lines, uint32_t i, HatchSegment& g) {
    const uint4 c = contours[hatch_contour(contours, f.n_contours, i)];  // (first, count, layer, closed)
    const uint32_t at = i - c.x;
    if (c.w == 0u && at + 1u >= c.y) return false;
    const uint32_t h = c.x + (at + 1u == c.y ? 0u : at + 1u);
    const float4 l = lines[c.z];
    g.layer = c.z, g.dx = (double)l.x, g.dy = (double)l.y, g.offset = (double)l.z, g.spacing = (double)l.w;
    const double st = hatch_s(points + (size_t)i * 3u, f.u, f.v, g.dx, g.dy), sh = hatch_s(points + (size_t)h * 3u, f.u, f.v, g.dx, g.dy);
    const bool tail_first = st < sh;
    g.a = tail_first ? i : h, g.b = tail_first ? h : i;
    g.sa = tail_first ? st : sh, g.sb = tail_first ? sh : st;
    return true;
}

// cstart[i] = the crossings of segment i (to be scanned), j0[i] = its first line; sums[block] = the block's sum over its kSliceBlock
// points, as a 64-bit number (lo | hi << 32 with hi = sum >> 32: what rm_block_scan_kernel adds up half by half); rows: entry 0
// SEGMENTS_IN.
__global__ __launch_bounds__(256) void rm_hatch_count_kernel(HatchFrame f, const float* __restrict__ points, const uint4* __restrict__ contours,
                                                             const float4* __restrict__ lines, uint32_t* __restrict__ cstart,
                                                             uint32_t* __restrict__ j0, unsigned long long* __restrict__ sums,
                                                             unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wsum[4];
    unsigned long long s_all = 0ull, tails = 0ull;
#pragma unroll 1
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t i = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        if (i >= f.n_points) continue;
        uint32_t cnt = 0u, first = 0u;
        HatchSegment g;
        if (hatch_segment(f, points, contours, lines, i, g)) {
            tails++;
            if (g.sa < g.sb && g.sa - g.sa == 0.0 && g.sb - g.sb == 0.0) {  // both finite (NaN compares false, inf - inf is NaN)
                first = hatch_lower(g.sa, g.offset, g.spacing, f.n_lines);
                cnt = hatch_lower(g.sb, g.offset, g.spacing, f.n_lines) - first;
            }
        }
        cstart[i] = cnt;
        j0[i] = first;
        s_all += cnt;
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>(s_all, wsum, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
    block_row<16>(tails, wsum, rows);  // (at most kSliceBlock tails to a workgroup)
}

RM_DEV uint32_t hatch_key32(float r) {
    const uint32_t b = __float_as_uint(r);
    return b ^ ((b >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u);
}

// keys[i], values[i] = i, xs[i] = (X_u, X_v) of crossing i.
__global__ __launch_bounds__(256) void rm_hatch_items_kernel(HatchFrame f, uint32_t n_items, const float* __restrict__ points,
                                                             const uint4* __restrict__ contours, const float4* __restrict__ lines,
                                                             const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ j0,
                                                             unsigned long long* __restrict__ keys, uint32_t* __restrict__ values,
                                                             float2* __restrict__ xs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t seg = mslice_item_edge(cstart, f.n_points, i), j = j0[seg] + (i - cstart[seg]);
    HatchSegment g;
    (void)hatch_segment(f, points, contours, lines, seg, g);  // (a segment with crossings is one)
    const double t = (hatch_c(j, g.offset, g.spacing) - g.sa) / (g.sb - g.sa);
    const float* A = points + (size_t)g.a * 3u;
    const float* B = points + (size_t)g.b * 3u;
    const float xu = (float)((double)A[f.u] + t * ((double)B[f.u] - (double)A[f.u]));
    const float xv = (float)((double)A[f.v] + t * ((double)B[f.v] - (double)A[f.v]));
    const float r = (float)((double)xu * g.dx + (double)xv * g.dy);
    const unsigned long long L = (unsigned long long)g.layer * f.n_lines + j;
    keys[i] = L << 32 | hatch_key32(r);
    values[i] = i;
    xs[i] = make_float2(xu, xv);
}

// the first q in [0, n] with keys[q] >= x
RM_DEV uint32_t hatch_key_lower(const unsigned long long* __restrict__ keys, uint32_t n, unsigned long long x) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] >= x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// keys: sorted.  hstart[q] = 1 for a head; sums as rm_mslice_count_kernel's; rows: entry 0 LINES_HIT, entry 1 ODD_LINES.
__global__ __launch_bounds__(256) void rm_hatch_pair_kernel(uint32_t n_items, const unsigned long long* __restrict__ keys,
                                                            uint32_t* __restrict__ hstart, unsigned long long* __restrict__ sums,
                                                            unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[4];
    __shared__ uint32_t wsum[4];
    uint32_t heads = 0u;
    unsigned long long packed = 0ull;
#pragma unroll 1
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t q = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        if (q >= n_items) continue;
        const unsigned long long L = keys[q] >> 32;
        const uint32_t rank = q - hatch_key_lower(keys, q, L << 32);  // (the line's first crossing lies at or before q)
        const bool partner = q + 1u < n_items && (keys[q + 1u] >> 32) == L, even = (rank & 1u) == 0u;
        const uint32_t head = even && partner ? 1u : 0u;
        hstart[q] = head;
        heads += head;
        packed += (rank == 0u ? 1ull : 0ull) + (even && !partner ? 1ull << 16 : 0ull);
    }
    uint32_t total;
    (void)block_exclusive_sum<4>(heads, wsum, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
    block_row<16, 16>(packed, wred, rows);
}

// hstart: scanned, hstart[n_items] = H.  Lane q < n_items: the segment of a head; lane k <= n_layers: layer_first[k].
__global__ __launch_bounds__(256) void rm_hatch_emit_kernel(uint32_t n_items, uint32_t n_layers, uint32_t n_lines, uint32_t zigzag,
                                                            const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ values,
                                                            const float2* __restrict__ xs, const uint32_t* __restrict__ hstart,
                                                            float4* __restrict__ segments, uint32_t* __restrict__ line,
                                                            uint32_t* __restrict__ layer_first) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q <= n_layers) {
        // k * n_lines < 2^32 for k < n_layers; the layer begins at the first crossing of its first line or any later one
        const unsigned long long first_line = (unsigned long long)q * n_lines;
        layer_first[q] = q == n_layers ? hstart[n_items] : hstart[hatch_key_lower(keys, n_items, first_line << 32)];
    }
    if (q >= n_items) return;
    uint32_t pos = hstart[q];
    if (hstart[q + 1u] == pos) return;  // no head
    const unsigned long long L = keys[q] >> 32;
    float2 a = xs[values[q]], b = xs[values[q + 1u]];
    if (zigzag != 0u && (((uint32_t)(L % n_lines)) & 1u) != 0u) {
        // the line's segments [base, base + m) in reverse, ends swapped
        const uint32_t q0 = hatch_key_lower(keys, q, L << 32);
        const uint32_t q1 = L == 0xFFFFFFFFull ? n_items : hatch_key_lower(keys, n_items, (L + 1ull) << 32);
        const uint32_t base = hstart[q0], m = hstart[q1] - base;
        pos = base + (m - 1u - (pos - base));
        const float2 x = a;
        a = b;
        b = x;
    }
    segments[pos] = make_float4(a.x, a.y, b.x, b.y);
    line[pos] = (uint32_t)L;
}

}  // namespace rmk
