// rm_mesh.h -- mesh export (rm_sample_grid, rm_extract_mesh): the scene's distance on a lattice, and its level surface as
// an indexed triangle mesh.  Included by rm_abi.hip alone, after rm_query.h: neither the draw kernels nor the specialiser's
// embedded headers change.
//
// The contract pins every bit of the output, so a CPU restatement can compare arrays exactly:
//   lattice point (i, j, k) = (ox + (float)i * sx, ...), linear index i + nx * (j + ny * k); its value is query_distance;
//   inside iff d < level (NaN outside); one vertex per lattice edge whose ends differ, at t = (da - level) / (da - db) along
//   the edge, ordered by (start point, axis); triangles per cell (anchored at its lowest corner) from the case table below,
//   ordered by cell and then by table order.
// Extraction is count, scan, emit: rm_mesh_count_kernel sums the vertices and triangles of each 2048-point block,
// rm_mesh_scan_kernel turns the block sums into offsets (one workgroup, no inter-workgroup flags), and the two emit kernels
// redo their block's local scan on top of that offset.  Every order is fixed by the lattice: no atomics, identical runs.
#pragma once
#include "rm_query.h"
#include "rm_reduce.h"

namespace rmk {

// ---- the cube case table (host and device) ------------------------------------------------------------------------------
// Corner c (0..7) sits at (c & 1, c >> 1 & 1, c >> 2 & 1).  Edge e (0..11) runs along axis a = e >> 2, from the corner with
// 0 on that axis to the one with 1; bit 0 of e & 3 is its offset on the lower of the two other axes, bit 1 on the higher.
// On each face the crossing edges pair up into segments (4 crossings: one segment around each inside corner, so inside
// corners are never joined across a face), oriented so that, seen from outside the cube, the inside corners lie on the
// right; the segments chain head to tail into loops, each started at its lowest edge, taken in that order and cut into fans
// (l0, lk, lk+1).  Case = sum of inside(c) << c.  Words per case: [0] the triangle count, then 3 edges per triangle,
// 0xFFFFFFFF after the last.
constexpr int kMeshCaseWords = 16;
struct MeshCaseTable {
    uint32_t w[256 * kMeshCaseWords];
    bool ok;  // every case chained into closed loops of at most 5 triangles
};

constexpr int mesh_edge_lo_axis(int a) { return a == 0 ? 1 : 0; }
constexpr int mesh_edge_hi_axis(int a) { return a == 2 ? 1 : 2; }
// the coordinate of edge e on axis f != its own axis
constexpr int mesh_edge_offset(int e, int f) {
    return f == mesh_edge_lo_axis(e >> 2) ? (e & 1) : ((e >> 1) & 1);
}
// corner index of end `end` (0 or 1) of edge e
constexpr int mesh_edge_corner(int e, int end) {
    const int a = e >> 2, lo = mesh_edge_lo_axis(a), hi = mesh_edge_hi_axis(a);
    return (end << a) | ((e & 1) << lo) | (((e >> 1) & 1) << hi);
}

constexpr MeshCaseTable make_mesh_case_table() {
    MeshCaseTable T{};
    T.ok = true;
    for (int cs = 0; cs < 256; cs++) {
        uint32_t* out = T.w + cs * kMeshCaseWords;
        for (int k = 0; k < kMeshCaseWords; k++) out[k] = 0xFFFFFFFFu;
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        bool crossing[12] = {};
        for (int e = 0; e < 12; e++)
            crossing[e] = ((cs >> mesh_edge_corner(e, 0)) & 1) != ((cs >> mesh_edge_corner(e, 1)) & 1);
        for (int f = 0; f < 3; f++)
            for (int s = 0; s < 2; s++) {
                int fe[4] = {}, nf = 0;  // crossing edges of this face
                for (int e = 0; e < 12; e++)
                    if ((e >> 2) != f && mesh_edge_offset(e, f) == s && crossing[e]) fe[nf++] = e;
                if (nf == 0) continue;
                int seg[2][3] = {};  // (edge, edge, inside corner on the right)
                int ns = 0;
                for (int c = 0; c < 8; c++) {
                    if (((c >> f) & 1) != s || !((cs >> c) & 1)) continue;
                    if (nf == 2) {
                        seg[0][0] = fe[0]; seg[0][1] = fe[1]; seg[0][2] = c;
                        ns = 1;
                        break;
                    }
                    // 4 crossings: the two face edges at this inside corner
                    int a2[2] = {}, na = 0;
                    for (int q = 0; q < 4; q++)
                        if (mesh_edge_corner(fe[q], 0) == c || mesh_edge_corner(fe[q], 1) == c) a2[na++] = fe[q];
                    if (na != 2) T.ok = false;
                    seg[ns][0] = a2[0]; seg[ns][1] = a2[1]; seg[ns][2] = c;
                    ns++;
                }
                if (ns != (nf == 2 ? 1 : 2)) T.ok = false;
                for (int q = 0; q < ns; q++) {
                    // positions doubled: edge midpoints and the corner on integer coordinates
                    int A[3] = {}, B[3] = {}, P[3] = {}, n[3] = {};
                    for (int x = 0; x < 3; x++) {
                        A[x] = x == (seg[q][0] >> 2) ? 1 : 2 * mesh_edge_offset(seg[q][0], x);
                        B[x] = x == (seg[q][1] >> 2) ? 1 : 2 * mesh_edge_offset(seg[q][1], x);
                        P[x] = 2 * ((seg[q][2] >> x) & 1);
                    }
                    n[f] = s ? 1 : -1;  // outward normal of the face
                    const int d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
                    const int r[3] = {d[1] * n[2] - d[2] * n[1], d[2] * n[0] - d[0] * n[2], d[0] * n[1] - d[1] * n[0]};  // d x n: right
                    const int side = r[0] * (P[0] - A[0]) + r[1] * (P[1] - A[1]) + r[2] * (P[2] - A[2]);
                    const int from = side > 0 ? seg[q][0] : seg[q][1], to = side > 0 ? seg[q][1] : seg[q][0];
                    if (side == 0 || next[from] != -1) T.ok = false;
                    else next[from] = to;
                }
            }
        bool seen[12] = {};
        int ntri = 0;
        for (int e0 = 0; e0 < 12; e0++) {
            if (!crossing[e0] || seen[e0]) continue;
            int loop[12] = {}, len = 0;
            for (int e = e0; e >= 0 && !seen[e]; e = next[e]) {
                seen[e] = true;
                loop[len++] = e;
            }
            if (len < 3 || next[loop[len - 1]] != e0) { T.ok = false; break; }
            for (int k = 1; k + 1 < len; k++) {
                if (ntri == 5) { T.ok = false; break; }
                out[1 + 3 * ntri] = (uint32_t)loop[0];
                out[2 + 3 * ntri] = (uint32_t)loop[k];
                out[3 + 3 * ntri] = (uint32_t)loop[k + 1];
                ntri++;
            }
        }
        for (int e = 0; e < 12; e++)
            if (crossing[e] && !seen[e]) T.ok = false;
        out[0] = (uint32_t)ntri;
    }
    return T;
}

// The device's form: one word per case, the triangle count in bits 0-3 and the edge of vertex v of the case's triangles
// (v = 3t + m) in bits 4 + 4v (at most 5 triangles: 15 edges, 64 bits).
struct MeshCasesPacked { unsigned long long c[256]; };
constexpr MeshCasesPacked pack_mesh_cases(const MeshCaseTable& T) {
    MeshCasesPacked P{};
    for (int cs = 0; cs < 256; cs++) {
        const uint32_t* w = T.w + cs * kMeshCaseWords;
        unsigned long long v = w[0];
        for (uint32_t k = 0; k < 3u * w[0]; k++) v |= (unsigned long long)w[1 + k] << (4 + 4 * k);
        P.c[cs] = v;
    }
    return P;
}

constexpr MeshCaseTable kMeshCaseTable = make_mesh_case_table();
static_assert(kMeshCaseTable.ok, "the case-table rule must chain every case into loops of at most 5 triangles");
__constant__ MeshCasesPacked kMeshCases = pack_mesh_cases(kMeshCaseTable);

// ---- lattice ---------------------------------------------------------------------------------------------------------
struct MeshGrid {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz;
    uint32_t n;  // nx * ny * nz (extraction: <= 2^28)
};

RM_DEV float grid_coord(float o, uint32_t i, float s) { return o + (float)i * s; }

// map_scene at every lattice point, one lane per point (up to 2^31 points)
template <int LOOP>
__global__ __launch_bounds__(256) void rm_grid_dist_kernel(QueryLaunch Q, float ox, float oy, float oz, float sx, float sy,
                                                           float sz, uint32_t nx, uint32_t ny, uint64_t n,
                                                           float* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float* spill = query_spill(Q.slots);
    const uint32_t i = p % nx, r = p / nx, j = r % ny, k = r / ny;
    out[p] = query_distance<LOOP>(Q, spill, grid_coord(ox, i, sx), grid_coord(oy, j, sy), grid_coord(oz, k, sz));
}

// ---- extraction: count, scan, emit ---------------------------------------------------------------------------------------
// (wave_inclusive_sum and block_exclusive_sum: rm_reduce.h)
// Each 256-thread workgroup owns kMeshBlock consecutive lattice points, each thread kMeshPer of them in a row.
constexpr uint32_t kMeshPer = 8, kMeshBlock = 256u * kMeshPer;
constexpr uint8_t kMeshInside = 8u;  // flags byte: bits 0-2 the crossing edges along x, y, z from this point; bit 3 inside

// The lattice position of this thread's first point and whether each of its points has an edge / a cell.
struct MeshRun {
    uint32_t p0;
    uint32_t i, j, k;
};
RM_DEV MeshRun mesh_run(const MeshGrid& g) {
    MeshRun r;
    r.p0 = blockIdx.x * kMeshBlock + threadIdx.x * kMeshPer;
    r.i = r.p0 % g.nx;
    const uint32_t q = r.p0 / g.nx;
    r.j = q % g.ny;
    r.k = q / g.ny;
    return r;
}
RM_DEV void mesh_step(const MeshGrid& g, uint32_t& i, uint32_t& j, uint32_t& k) {
    if (++i == g.nx) {
        i = 0;
        if (++j == g.ny) { j = 0; ++k; }
    }
}
// inside(d) of the 9 points p0 .. p0 + 8 past `off` (bit m); points past the lattice read as outside (never used)
RM_DEV uint32_t mesh_inside_row(const float* __restrict__ dist, uint32_t n, uint32_t first, float level) {
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t m = 0; m <= kMeshPer; m++) {
        const uint32_t p = first + m;
        const float d = p < n ? dist[p] : 0.0f;
        bits |= (p < n && d < level ? 1u : 0u) << m;
    }
    return bits;
}

// Per block: (vertices, triangles) of its points, packed v | t << 32 (the sums of the whole lattice fit 32 bits each).
__global__ __launch_bounds__(256) void rm_mesh_count_kernel(MeshGrid g, float level, const float* __restrict__ dist,
                                                            unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    const MeshRun r = mesh_run(g);
    const uint32_t nxy = g.nx * g.ny;
    uint32_t nv = 0, nt = 0;
    if (r.p0 < g.n) {
        const uint32_t b0 = mesh_inside_row(dist, g.n, r.p0, level), b1 = mesh_inside_row(dist, g.n, r.p0 + g.nx, level),
                       b2 = mesh_inside_row(dist, g.n, r.p0 + nxy, level), b3 = mesh_inside_row(dist, g.n, r.p0 + nxy + g.nx, level);
        uint32_t i = r.i, j = r.j, k = r.k;
        for (uint32_t m = 0; m < kMeshPer && r.p0 + m < g.n; m++) {
            const uint32_t in = (b0 >> m) & 1u;
            const bool ex = i + 1u < g.nx, ey = j + 1u < g.ny, ez = k + 1u < g.nz;
            nv += (ex && ((b0 >> (m + 1u)) & 1u) != in) + (ey && ((b1 >> m) & 1u) != in) + (ez && ((b2 >> m) & 1u) != in);
            if (ex && ey && ez) {
                const uint32_t cs = ((b0 >> m) & 3u) | ((b1 >> m) & 3u) << 2 | ((b2 >> m) & 3u) << 4 | ((b3 >> m) & 3u) << 6;
                nt += (uint32_t)(kMeshCases.c[cs] & 15ull);
            }
            mesh_step(g, i, j, k);
        }
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>((unsigned long long)nv | (unsigned long long)nt << 32, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// The block sums -> exclusive offsets, in place, by one 1024-thread workgroup (each thread a run of consecutive blocks);
// totals[0] = vertices, totals[1] = triangles.
__global__ __launch_bounds__(1024) void rm_mesh_scan_kernel(unsigned long long* __restrict__ block_sums, uint32_t n_blocks,
                                                            uint32_t* __restrict__ totals) {
    __shared__ unsigned long long wsum[16];
    const uint32_t per = (n_blocks + 1023u) / 1024u, b0 = min(threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    unsigned long long s = 0;
    for (uint32_t b = b0; b < b1; b++) s += block_sums[b];
    unsigned long long total;
    unsigned long long off = block_exclusive_sum<16>(s, wsum, total);
    for (uint32_t b = b0; b < b1; b++) {
        const unsigned long long v = block_sums[b];
        block_sums[b] = off;
        off += v;
    }
    if (threadIdx.x == 0) {
        totals[0] = (uint32_t)total;
        totals[1] = (uint32_t)(total >> 32);
    }
}

// Vertices: each point's crossing edges (x, y, z in that order) at vbase[point] on; the flags byte per point.
__global__ __launch_bounds__(256) void rm_mesh_vertex_kernel(MeshGrid g, float level, const float* __restrict__ dist,
                                                             const unsigned long long* __restrict__ block_offsets,
                                                             uint32_t* __restrict__ vbase, uint8_t* __restrict__ flags,
                                                             float* __restrict__ vertices) {
    __shared__ uint32_t wsum[4];
    const MeshRun r = mesh_run(g);
    const uint32_t nxy = g.nx * g.ny;
    float d0[kMeshPer + 1], dy[kMeshPer], dz[kMeshPer];
    uint32_t fl[kMeshPer];
    uint32_t nv = 0;
#pragma unroll
    for (uint32_t m = 0; m <= kMeshPer; m++) {
        const uint32_t p = r.p0 + m;
        d0[m] = p < g.n ? dist[p] : 0.0f;
        if (m == kMeshPer) break;
        dy[m] = p + g.nx < g.n ? dist[p + g.nx] : 0.0f;
        dz[m] = p + nxy < g.n ? dist[p + nxy] : 0.0f;
    }
    {
        uint32_t i = r.i, j = r.j, k = r.k;
#pragma unroll
        for (uint32_t m = 0; m < kMeshPer; m++) {
            uint32_t f = 0;
            if (r.p0 + m < g.n) {
                const bool in = d0[m] < level;
                f = in ? kMeshInside : 0u;
                f |= (i + 1u < g.nx && (d0[m + 1] < level) != in) ? 1u : 0u;
                f |= (j + 1u < g.ny && (dy[m] < level) != in) ? 2u : 0u;
                f |= (k + 1u < g.nz && (dz[m] < level) != in) ? 4u : 0u;
            }
            fl[m] = f;
            nv += __builtin_popcount(f & 7u);
            mesh_step(g, i, j, k);
        }
    }
    uint32_t total;
    uint32_t v = (uint32_t)block_offsets[blockIdx.x] + block_exclusive_sum<4>(nv, wsum, total);
    uint32_t i = r.i, j = r.j, k = r.k;
#pragma unroll
    for (uint32_t m = 0; m < kMeshPer; m++) {
        const uint32_t p = r.p0 + m;
        if (p < g.n) {
            vbase[p] = v;
            flags[p] = (uint8_t)fl[m];
        }
        if (fl[m] & 7u) {
            const float x = grid_coord(g.ox, i, g.sx), y = grid_coord(g.oy, j, g.sy), z = grid_coord(g.oz, k, g.sz);
            const float da = d0[m];
            if (fl[m] & 1u) {
                const float t = (da - level) / (da - d0[m + 1]), xb = grid_coord(g.ox, i + 1u, g.sx);
                vertices[3u * (size_t)v] = x + t * (xb - x); vertices[3u * (size_t)v + 1u] = y; vertices[3u * (size_t)v + 2u] = z;
                v++;
            }
            if (fl[m] & 2u) {
                const float t = (da - level) / (da - dy[m]), yb = grid_coord(g.oy, j + 1u, g.sy);
                vertices[3u * (size_t)v] = x; vertices[3u * (size_t)v + 1u] = y + t * (yb - y); vertices[3u * (size_t)v + 2u] = z;
                v++;
            }
            if (fl[m] & 4u) {
                const float t = (da - level) / (da - dz[m]), zb = grid_coord(g.oz, k + 1u, g.sz);
                vertices[3u * (size_t)v] = x; vertices[3u * (size_t)v + 1u] = y; vertices[3u * (size_t)v + 2u] = z + t * (zb - z);
                v++;
            }
        }
        mesh_step(g, i, j, k);
    }
}

// Triangles: the case of each cell from the inside bits of its corners' flags, its table entry, and the index of each
// vertex: vbase[q] + the crossing edges of q on lower axes, q the start point of the vertex's edge.
__global__ __launch_bounds__(256) void rm_mesh_triangle_kernel(MeshGrid g, const unsigned long long* __restrict__ block_offsets,
                                                               const uint32_t* __restrict__ vbase, const uint8_t* __restrict__ flags,
                                                               uint32_t* __restrict__ triangles) {
    __shared__ uint32_t wsum[4];
    const MeshRun r = mesh_run(g);
    const uint32_t nxy = g.nx * g.ny;
    unsigned long long tab[kMeshPer];
    uint32_t nt = 0;
    {
        uint32_t i = r.i, j = r.j, k = r.k;
#pragma unroll
        for (uint32_t m = 0; m < kMeshPer; m++) {
            const uint32_t p = r.p0 + m;
            unsigned long long e = 0;
            if (p < g.n && i + 1u < g.nx && j + 1u < g.ny && k + 1u < g.nz) {  // a cell: all 8 corners are on the lattice
                uint32_t cs = 0;
#pragma unroll
                for (uint32_t c = 0; c < 8u; c++) {
                    const uint32_t q = p + (c & 1u) + ((c >> 1) & 1u) * g.nx + (c >> 2) * nxy;
                    cs |= ((uint32_t)(flags[q] >> 3) & 1u) << c;
                }
                e = kMeshCases.c[cs];
            }
            tab[m] = e;
            nt += (uint32_t)(e & 15ull);
            mesh_step(g, i, j, k);
        }
    }
    uint32_t total;
    size_t t = (size_t)((uint32_t)(block_offsets[blockIdx.x] >> 32) + block_exclusive_sum<4>(nt, wsum, total));
#pragma unroll
    for (uint32_t m = 0; m < kMeshPer; m++) {
        const uint32_t p = r.p0 + m, cnt = (uint32_t)(tab[m] & 15ull);
        for (uint32_t v = 0; v < 3u * cnt; v++) {
            const uint32_t e = (uint32_t)(tab[m] >> (4u + 4u * v)) & 15u, a = e >> 2;
            // the start point: offsets (bits 0, 1 of e) on the lower and the higher of the two other axes
            const uint32_t s_lo = a == 0u ? g.nx : 1u, s_hi = a == 2u ? g.nx : nxy;
            const uint32_t q = p + (e & 1u) * s_lo + ((e >> 1) & 1u) * s_hi;
            triangles[3u * t + v] = vbase[q] + (uint32_t)__builtin_popcount((uint32_t)flags[q] & ((1u << a) - 1u));
        }
        t += cnt;
    }
}

}  // namespace rmk
