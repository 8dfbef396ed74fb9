// rm_mesh_slice.h -- mesh slicing (rm_slice_mesh): the outlines of an indexed triangle mesh in a stack of parallel planes, as the
// ordered contour loops of rm_slice.h.  Included by rm_abi.hip alone, after rm_slice.h, rm_voxel.h and rm_sort.h.  DESIGN.md
// section 30 is the contract.  Vertices are snapped as the voxeliser snaps them (vox_snap: even positions in units of 1 / 128 of
// a step), planes sit at odd positions P2, so no vertex lies on a plane and everything up to the points is exact in integers.
//   snap     one lane per vertex: its snapped coordinates, or kMsliceBad
//   keys     one lane per half-edge h = 3 t + s (from tri[t][s] to tri[t][(s + 1) % 3]): the key lo << b | hi of its unordered
//            index pair, 0 for a half-edge of a rejected triangle (an accepted one has lo < hi, so its key is not 0)
//   (sort)   by key, stably: the half-edges of an edge lie side by side, lowest h first
//   groups   one lane per sorted half-edge: its mate if its group is two half-edges of opposite direction, else kSliceNil; the
//            counts PAIRED, BORDER, BRANCH (per group) and REJECTED (per triangle) in rows
//   count    one lane per half-edge: the planes strictly between the ends of a CANONICAL half-edge (no mate, or the lower of the
//            two) -- a contiguous range [k0, k0 + cnt) by binary search, P2 increasing -- and the block sums of cnt
//   scan     estart[h] = the vertices before h's own in edge-major order (an ITEM is a vertex in that order)
//   items    one lane per item: its half-edge by binary search over estart, its plane; (key, value) = (plane, item)
//   (sort)   by plane, stably: the place of an item is its vertex ID, ordered by (plane, canonical half-edge)
//   ids      one lane per id: inv[item] = id, vh[id] = the half-edge, and the first id of every layer
//   link     one lane per id: in the triangle of its half-edge, and in that of the mate, the plane crosses one more half-edge; the
//            segment runs from the half-edge going down to the one going up: next[id] or prev[id] = the other's id
//   (rank)   rm_slice.h's pointer doubling, cut, start and length scans and layer_first, as they are
//   emit     one lane per id: the point, written where contour and rank put it; the contour records; OPEN contours in rows
// Every slot has one writer and no atomic is used: identical runs.
#pragma once
#include "rm_abi_layout.h"
#include "rm_reduce.h"
#include "rm_slice.h"
#include "rm_sort.h"
#include "rm_voxel.h"

namespace rmk {

struct MsliceFrame {
    double o[3], s[3];  // the caller's floats, converted exactly
    uint32_t axis;      // w
    uint32_t n_layers;
};

__global__ __launch_bounds__(256) void rm_mslice_snap_kernel(MsliceFrame f, uint32_t n_vertices, const float* __restrict__ xyz,
                                                             int32_t* __restrict__ vq) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    const float* p = xyz + (size_t)v * 3u;
    int q[3] = {0, 0, 0};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) ok = vox_snap(p[a], f.o[a], f.s[a], q[a]) && ok;
    int32_t* o = vq + (size_t)v * 3u;
    o[0] = ok ? q[0] : rml::kMsliceBad;
    o[1] = q[1];
    o[2] = q[2];
}

// The corners of triangle t; false for a rejected one: an index beyond the vertices, two equal indices, a corner that did not snap.
RM_DEV bool mslice_tri(const uint32_t* __restrict__ tris, uint32_t t, uint32_t n_vertices, const int32_t* __restrict__ vq, uint32_t (&v)[3]) {
#pragma unroll
    for (int e = 0; e < 3; e++) v[e] = tris[(size_t)t * 3u + e];
    if (v[0] >= n_vertices || v[1] >= n_vertices || v[2] >= n_vertices || v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return false;
    return vq[(size_t)v[0] * 3u] != rml::kMsliceBad && vq[(size_t)v[1] * 3u] != rml::kMsliceBad && vq[(size_t)v[2] * 3u] != rml::kMsliceBad;
}
RM_DEV uint32_t mslice_next(uint32_t s) { return s == 2u ? 0u : s + 1u; }
// the canonical half-edge of the edge of h (of an accepted triangle)
RM_DEV uint32_t mslice_canonical(const uint32_t* __restrict__ mate, uint32_t h) {
    const uint32_t m = mate[h];
    return m == kSliceNil || h < m ? h : m;
}

__global__ __launch_bounds__(256) void rm_mslice_keys_kernel(uint32_t n_vertices, uint32_t n_half, uint32_t b, const uint32_t* __restrict__ tris,
                                                             const int32_t* __restrict__ vq, unsigned long long* __restrict__ keys,
                                                             uint32_t* __restrict__ values) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n_half) return;
    const uint32_t t = h / 3u, s = h - 3u * t;
    uint32_t v[3];
    unsigned long long key = 0ull;
    if (mslice_tri(tris, t, n_vertices, vq, v)) {
        const uint32_t a = v[s], e = v[mslice_next(s)];
        key = (unsigned long long)min(a, e) << b | (unsigned long long)max(a, e);
    }
    keys[h] = key;
    values[h] = h;
}

// whether half-edge h runs from its lower index to its higher one
RM_DEV bool mslice_ascending(const uint32_t* __restrict__ tris, uint32_t h) {
    const uint32_t t = h / 3u, s = h - 3u * t;
    return tris[(size_t)t * 3u + s] < tris[(size_t)t * 3u + mslice_next(s)];
}

// rows: entry 0 PAIRED, 1 BORDER, 2 BRANCH, 3 REJECTED
__global__ __launch_bounds__(256) void rm_mslice_groups_kernel(uint32_t n_half, const uint32_t* __restrict__ tris,
                                                               const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ values,
                                                               uint32_t* __restrict__ mate, unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long packed = 0ull;
    if (i < n_half) {
        const unsigned long long key = keys[i];
        const uint32_t h = values[i];
        uint32_t m = kSliceNil;
        if (key == 0ull) {
            packed = h % 3u == 0u ? 1ull << 48 : 0ull;
        } else {
            const bool prev = i > 0u && keys[i - 1u] == key, next = i + 1u < n_half && keys[i + 1u] == key;
            if (!prev && !next) {
                packed = 1ull << 16;
            } else if (!prev) {
                const bool more = i + 2u < n_half && keys[i + 2u] == key;
                const uint32_t h2 = values[i + 1u];
                if (!more && mslice_ascending(tris, h) != mslice_ascending(tris, h2)) m = h2, packed = 1ull;
                else packed = 1ull << 32;
            } else if (!next && !(i >= 2u && keys[i - 2u] == key)) {
                const uint32_t h1 = values[i - 1u];
                if (mslice_ascending(tris, h) != mslice_ascending(tris, h1)) m = h1;
            }
        }
        mate[h] = m;
    }
    block_row<16, 16, 16, 16>(packed, wred, rows);
}

// the first k in [0, n) with p2[k] > x
RM_DEV uint32_t mslice_upper(const int32_t* __restrict__ p2, uint32_t n, int32_t x) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p2[mid] > x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// estart[h] = cnt (to be scanned), k0[h]; sums[block] = the block's sum of cnt over its kSliceBlock half-edges
__global__ __launch_bounds__(256) void rm_mslice_count_kernel(MsliceFrame f, uint32_t n_vertices, uint32_t n_half, const uint32_t* __restrict__ tris,
                                                              const int32_t* __restrict__ vq, const int32_t* __restrict__ p2,
                                                              const uint32_t* __restrict__ mate, uint32_t* __restrict__ estart,
                                                              uint32_t* __restrict__ k0, unsigned long long* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    uint32_t s_all = 0u;
#pragma unroll 1
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t h = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        if (h >= n_half) continue;
        const uint32_t t = h / 3u, s = h - 3u * t;
        uint32_t v[3], cnt = 0u, first = 0u;
        if (mslice_tri(tris, t, n_vertices, vq, v) && mslice_canonical(mate, h) == h) {
            const int32_t za = vq[(size_t)v[s] * 3u + f.axis], zb = vq[(size_t)v[mslice_next(s)] * 3u + f.axis];
            const int32_t lo = 2 * min(za, zb), hi = 2 * max(za, zb);  // even; the planes are odd
            first = mslice_upper(p2, f.n_layers, lo);
            cnt = mslice_upper(p2, f.n_layers, hi) - first;
        }
        estart[h] = cnt;
        k0[h] = first;
        s_all += cnt;
    }
    uint32_t total;
    (void)block_exclusive_sum<4>(s_all, wsum, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// estart in place: the exclusive scan on top of the block's offset; estart[n_half] = the total (modulo 2^32: the host has the sum)
__global__ __launch_bounds__(256) void rm_mslice_scan_kernel(uint32_t n_half, const unsigned long long* __restrict__ offsets,
                                                             uint32_t* __restrict__ estart) {
    __shared__ uint32_t wsum[4];
    uint32_t carry = (uint32_t)offsets[blockIdx.x];
    for (uint32_t it = 0; it < 4u; it++) {
        const uint32_t h = blockIdx.x * kSliceBlock + it * 256u + threadIdx.x;
        const uint32_t v = h < n_half ? estart[h] : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_exclusive_sum<4>(v, wsum, total);
        if (h < n_half) {
            estart[h] = ex;
            if (h + 1u == n_half) estart[n_half] = ex + v;
        }
        carry += total;
    }
}

// the half-edge whose items hold item i: the last h with estart[h] <= i (estart[n_half] = n_items > i)
RM_DEV uint32_t mslice_item_edge(const uint32_t* __restrict__ estart, uint32_t n_half, uint32_t i) {
    uint32_t lo = 0u, hi = n_half;  // the first h in [0, n_half] with estart[h] > i, never 0
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (estart[mid] > i) hi = mid;
        else lo = mid + 1u;
    }
    return lo - 1u;
}

__global__ __launch_bounds__(256) void rm_mslice_items_kernel(uint32_t n_items, uint32_t n_half, const uint32_t* __restrict__ estart,
                                                              const uint32_t* __restrict__ k0, unsigned long long* __restrict__ keys,
                                                              uint32_t* __restrict__ values) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t h = mslice_item_edge(estart, n_half, i);
    keys[i] = (unsigned long long)(k0[h] + (i - estart[h]));
    values[i] = i;
}

// keys / values: the items sorted by plane.  layer_base[l] = the first id of layer l, layer_base[n_layers] = n_items.
__global__ __launch_bounds__(256) void rm_mslice_ids_kernel(uint32_t n_items, uint32_t n_half, uint32_t n_layers, const uint32_t* __restrict__ estart,
                                                            const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ values,
                                                            uint32_t* __restrict__ inv, uint32_t* __restrict__ vh, uint32_t* __restrict__ layer_base) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n_items) return;
    const uint32_t i = values[id], k = (uint32_t)keys[id];
    if (i < n_items) inv[i] = id;
    vh[id] = mslice_item_edge(estart, n_half, i);
    // the layers that begin here: those above the previous id's, up to this id's
    const uint32_t from = id == 0u ? 0u : (uint32_t)keys[id - 1u] + 1u;
    for (uint32_t l = from; l <= k && l < n_layers; l++) layer_base[l] = id;
    if (id + 1u == n_items)
        for (uint32_t l = k + 1u; l <= n_layers; l++) layer_base[l] = n_items;
}

// next and prev come filled with kSliceNil.
__global__ __launch_bounds__(256) void rm_mslice_link_kernel(MsliceFrame f, uint32_t n_items, const uint32_t* __restrict__ tris,
                                                             const int32_t* __restrict__ vq, const int32_t* __restrict__ p2,
                                                             const uint32_t* __restrict__ mate, const uint32_t* __restrict__ estart,
                                                             const uint32_t* __restrict__ k0, const unsigned long long* __restrict__ keys,
                                                             const uint32_t* __restrict__ vh, const uint32_t* __restrict__ inv,
                                                             uint32_t* __restrict__ next, uint32_t* __restrict__ prev) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n_items) return;
    const uint32_t c = vh[id], k = (uint32_t)keys[id];
    const int32_t P2 = p2[k];
    for (uint32_t side = 0; side < 2u; side++) {
        const uint32_t x = side == 0u ? c : mate[c];
        if (x == kSliceNil) break;
        const uint32_t t = x / 3u, s = x - 3u * t, s1 = mslice_next(s), s2 = mslice_next(s1);
        const uint32_t va = tris[(size_t)t * 3u + s], vb = tris[(size_t)t * 3u + s1], vc = tris[(size_t)t * 3u + s2];
        const bool a_up = 2 * vq[(size_t)va * 3u + f.axis] > P2, b_up = 2 * vq[(size_t)vb * 3u + f.axis] > P2,
                   c_up = 2 * vq[(size_t)vc * 3u + f.axis] > P2;
        // x runs a -> b across the plane; the third corner is on b's side: c -> a crosses, else b -> c does
        const uint32_t y = 3u * t + (c_up == b_up ? s2 : s1), cy = mslice_canonical(mate, y);
        const uint32_t item = estart[cy] + (k - k0[cy]);
        if (item >= n_items) continue;  // (never: the plane lies between the ends of y)
        const uint32_t other = inv[item];
        if (a_up && !b_up) next[id] = other;  // x goes down: the segment starts here
        else prev[id] = other;
    }
}

// The point of vertex `id` where its contour and rank put it, the record of a contour at its first vertex, and in rows entry 0 the
// vertices no segment ends at (the open contours).
__global__ __launch_bounds__(256) void rm_mslice_emit_kernel(MsliceFrame f, uint32_t n_items, const uint32_t* __restrict__ tris,
                                                             const int32_t* __restrict__ vq, const int32_t* __restrict__ p2,
                                                             const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vh,
                                                             const uint32_t* __restrict__ prev, const uint2* __restrict__ rank,
                                                             const uint32_t* __restrict__ start, const uint32_t* __restrict__ length,
                                                             const uint32_t* __restrict__ first_point, float* __restrict__ points,
                                                             uint4* __restrict__ contours, unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[4];
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    unsigned long long open = 0ull;
    if (id < n_items) {
        const uint32_t c = vh[id], k = (uint32_t)keys[id], t = c / 3u, s = c - 3u * t, w = f.axis, u = w == 2u ? 0u : w + 1u, v = u == 2u ? 0u : u + 1u;
        uint32_t ia = tris[(size_t)t * 3u + s], ib = tris[(size_t)t * 3u + mslice_next(s)];
        if (vq[(size_t)ia * 3u + w] > vq[(size_t)ib * 3u + w]) {
            const uint32_t x = ia;
            ia = ib;
            ib = x;
        }
        const int32_t* A = vq + (size_t)ia * 3u;
        const int32_t* B = vq + (size_t)ib * 3u;
        const int32_t P2 = p2[k];
        const long long num = (long long)P2 - 2ll * A[w], den = 2ll * ((long long)B[w] - A[w]);  // 0 < num < den
        const double gu = (double)A[u] + (double)((long long)(B[u] - A[u]) * num) / (double)den;
        const double gv = (double)A[v] + (double)((long long)(B[v] - A[v]) * num) / (double)den;
        const double gw = (double)P2 / 2.0;
        // (x, y, z) = (w, u, v), (v, w, u) or (u, v, w) for w = 0, 1, 2
        const double gx = w == 0u ? gw : w == 1u ? gv : gu, gy = w == 0u ? gu : w == 1u ? gw : gv, gz = w == 0u ? gv : w == 1u ? gu : gw;
        const uint2 r = rank[id];
        const uint32_t cn = start[r.x] >> 2, fp = first_point[cn];
        float* o = points + 3u * ((size_t)fp + r.y);
        o[0] = (float)(f.o[0] + gx / 64.0 * f.s[0]);
        o[1] = (float)(f.o[1] + gy / 64.0 * f.s[1]);
        o[2] = (float)(f.o[2] + gz / 64.0 * f.s[2]);
        if (r.y == 0u) contours[cn] = make_uint4(fp, length[cn], k, (start[id] >> 1) & 1u);
        open = prev[id] == kSliceNil ? 1ull : 0ull;
    }
    block_row<16>(open, wred, rows);
}

}  // namespace rmk
