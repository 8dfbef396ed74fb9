// rm_voxel.h -- mesh voxelisation (rm_voxelize_mesh): a triangle mesh into the occupancy of a lattice, by the even-odd rule along
// +x.  Included by rm_abi.hip alone.  DESIGN.md section 27 is the contract; every output is an integer that no order of execution
// changes: the crossings toggle bits by XOR, the counts are sums.
//
// A vertex is snapped to index space with 6 fractional bits (vox_snap: three correctly rounded binary64 operations, then
// rint); everything after that is exact in int64.  A triangle crosses the row (j, k) iff its three edge functions admit the
// point (64 j, 64 k) of the y-z plane (vox_admits: the tie rule is antisymmetric in the edge's direction); the crossing toggles
// bit t = ceil(x / 64) of the row, clamped to [0, nx], and the occupancy of point i is the XOR of the row's bits 0..i.
//   setup   one lane per triangle: gather, snap, reject, orient, the box of lattice rows its projection can reach and the number
//           of work items of 64 rows in it; a box of at most kVoxSmallRows rows is finished by the lane itself (no items).  The
//           record (12 words) and the items before the triangle in its block of 256; the block's sum for the scan
//           (rm_block_scan_kernel); TRIANGLES, REJECTED, EDGE_ON and the lanes' crossings by one atomic add per wave.
//   raster  one wave per work item, found by binary search over the blocks' offsets and then the block's 256 entries; one lane
//           per row of the box.  The 64-bit divide runs in admitted lanes only.
//   fill    a workgroup makes kVoxFillCells consecutive bytes of the occupancy: the bit words of the rows they lie in staged
//           in LDS (rml::VoxFillLds), each word's inclusive prefix XOR and the parity of the row's words before it, then 16
//           bytes per lane.  INSIDE and OPEN_ROWS into one row of 16 words per workgroup (rm_reduce.h).
// No kernel reads what another workgroup of its launch wrote; the atomics only accumulate and are read by the next launch.
#pragma once
#include "rm_device.h"
#include "rm_lds_layout.h"
#include "rm_reduce.h"

namespace rmk {

static_assert(rml::vox_fill_rows(2u) * rml::vox_row_words(2u) == rml::kVoxFillMaxWords, "the fill's staged words at nx = 2");

constexpr uint32_t kVoxFrac = 6u;                 // fractional bits of index space: lattice point i at 64 i
constexpr double kVoxMaxQ = 131072.0;             // |q| <= 2^17: 2048 points from the origin
constexpr uint32_t kVoxTriWords = 12u;            // a triangle's record: 9 coordinates, j0 | k0 << 16, nj | nk << 16, 0
constexpr uint32_t kVoxSmallRows = 4u;            // a box of at most this many rows is finished in the setup lane
constexpr uint32_t kVoxBlock = 256u;              // triangles of a setup workgroup = entries of one block of the item table
enum { VOX_N_TRIANGLES = 0, VOX_N_REJECTED = 1, VOX_N_EDGE_ON = 2, VOX_N_CROSSINGS = 3, VOX_N_COUNTERS = 8 };

// The lattice in binary64 (float origin and step, converted exactly) and the words of a row of nx + 1 bits.
struct VoxLattice {
    double ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz, row_words;
};

// q = rint((v - o) / s * 64): each operation rounded once (the build forbids contraction).  False for a coordinate that is not
// finite or lies beyond 2^17.
RM_DEV bool vox_snap(float v, double o, double s, int& q) {
    const double d = ((double)v - o) / s;
    const double r = rint(d * 64.0);
    if (!(fabs(r) <= kVoxMaxQ)) return false;  // (NaN fails, too)
    q = (int)r;
    return true;
}

// Whether the directed edge u -> v admits the point (Y, Z); E is its edge function there.
RM_DEV long long vox_edge(int uy, int uz, int dy, int dz, int Y, int Z) {
    return (long long)dy * (long long)(Z - uz) - (long long)dz * (long long)(Y - uy);
}
RM_DEV bool vox_admits(long long E, int dy, int dz) { return E > 0 || (E == 0 && (dy > 0 || (dy == 0 && dz > 0))); }

// The triangle (oriented: A2 > 0) on the row (j, k) of the lattice: toggles the bit of its crossing, if there is one.
RM_DEV bool vox_cross_row(const int (&q)[9], long long A2, uint32_t j, uint32_t k, const VoxLattice& g, uint32_t* __restrict__ bits) {
    const int Y = (int)(j << kVoxFrac), Z = (int)(k << kVoxFrac);
    const int ay = q[1], az = q[2], by = q[4], bz = q[5], cy = q[7], cz = q[8];
    const long long Ea = vox_edge(by, bz, cy - by, cz - bz, Y, Z);
    const long long Eb = vox_edge(cy, cz, ay - cy, az - cz, Y, Z);
    const long long Ec = vox_edge(ay, az, by - ay, bz - az, Y, Z);
    if (!(vox_admits(Ea, cy - by, cz - bz) && vox_admits(Eb, ay - cy, az - cz) && vox_admits(Ec, by - ay, bz - az))) return false;
    const long long num = Ea * q[0] + Eb * q[3] + Ec * q[6], den = A2 << kVoxFrac;  // |num| < 2^54, den nx < 2^53
    uint32_t t = 0u;
    if (num > 0) t = num > den * (long long)(g.nx - 1u) ? g.nx : (uint32_t)(((unsigned long long)num + (unsigned long long)den - 1ull) / (unsigned long long)den);
    atomicXor(bits + (size_t)(j + g.ny * k) * g.row_words + (t >> 5), 1u << (t & 31u));
    return true;
}

// ---- setup ----------------------------------------------------------------------------------------------------------------
// indices == nullptr: a soup, triangle t has the vertices 3 t, 3 t + 1, 3 t + 2.
__global__ __launch_bounds__(256) void rm_vox_setup_kernel(VoxLattice g, uint32_t n_vertices, const float* __restrict__ xyz, uint32_t n_triangles,
                                                           const uint32_t* __restrict__ indices, uint32_t* __restrict__ tris,
                                                           uint32_t* __restrict__ starts, unsigned long long* __restrict__ block_sums,
                                                           uint32_t* __restrict__ bits, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t wsum[4];
    const uint32_t t = blockIdx.x * kVoxBlock + threadIdx.x;
    const bool live = t < n_triangles;
    bool ok = live, edge_on = false;
    int q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        size_t v[3];
#pragma unroll
        for (int e = 0; e < 3; e++) {
            v[e] = indices ? (size_t)indices[(size_t)t * 3u + e] : (size_t)t * 3u + e;
            ok = ok && v[e] < (size_t)n_vertices;
        }
        if (ok) {
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const float* p = xyz + v[e] * 3u;
                const bool sx = vox_snap(p[0], g.ox, g.sx, q[3 * e]), sy = vox_snap(p[1], g.oy, g.sy, q[3 * e + 1]),
                           sz = vox_snap(p[2], g.oz, g.sz, q[3 * e + 2]);
                ok = ok && sx && sy && sz;
            }
        }
    }
    uint32_t items = 0u, crossings = 0u, j0 = 0u, k0 = 0u, nj = 0u, nk = 0u;
    if (ok) {
        long long A2 = (long long)(q[4] - q[1]) * (long long)(q[8] - q[2]) - (long long)(q[5] - q[2]) * (long long)(q[7] - q[1]);
        edge_on = A2 == 0;
        if (A2 < 0) {
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const int x = q[3 + e];
                q[3 + e] = q[6 + e];
                q[6 + e] = x;
            }
            A2 = -A2;
        }
        if (!edge_on) {
            // the rows 64 j in [min y, max y], 64 k in [min z, max z], clamped to the lattice (>> of a negative int: floor)
            const int ylo = min(q[1], min(q[4], q[7])), yhi = max(q[1], max(q[4], q[7]));
            const int zlo = min(q[2], min(q[5], q[8])), zhi = max(q[2], max(q[5], q[8]));
            const int ja = max((ylo + 63) >> kVoxFrac, 0), jb = min(yhi >> kVoxFrac, (int)g.ny - 1);
            const int ka = max((zlo + 63) >> kVoxFrac, 0), kb = min(zhi >> kVoxFrac, (int)g.nz - 1);
            if (ja <= jb && ka <= kb) {
                j0 = (uint32_t)ja, k0 = (uint32_t)ka, nj = (uint32_t)(jb - ja + 1), nk = (uint32_t)(kb - ka + 1);
                const uint32_t rows = nj * nk;  // <= 2^20
                if (rows <= kVoxSmallRows) {
                    for (uint32_t r = 0; r < rows; r++) crossings += vox_cross_row(q, A2, j0 + r % nj, k0 + r / nj, g, bits) ? 1u : 0u;
                } else {
                    items = (rows + 63u) >> 6;
                }
            }
        }
    }
    if (live) {
        uint4* rec = reinterpret_cast<uint4*>(tris + (size_t)t * kVoxTriWords);
        rec[0] = make_uint4((uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3]);
        rec[1] = make_uint4((uint32_t)q[4], (uint32_t)q[5], (uint32_t)q[6], (uint32_t)q[7]);
        rec[2] = make_uint4((uint32_t)q[8], j0 | k0 << 16, nj | nk << 16, 0u);
    }
    uint32_t total;
    const uint32_t before = block_exclusive_sum<4>(items, wsum, total);
    if (live) starts[t] = before;
    if (threadIdx.x == 0u) block_sums[blockIdx.x] = total;
    // the counts: one add per wave and count
    const uint32_t n_live = (uint32_t)__popcll(__ballot(live)), n_rej = (uint32_t)__popcll(__ballot(live && !ok)),
                   n_edge = (uint32_t)__popcll(__ballot(edge_on)), n_cross = wave_sum(crossings);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_live) atomicAdd(counters + VOX_N_TRIANGLES, (unsigned long long)n_live);
        if (n_rej) atomicAdd(counters + VOX_N_REJECTED, (unsigned long long)n_rej);
        if (n_edge) atomicAdd(counters + VOX_N_EDGE_ON, (unsigned long long)n_edge);
        if (n_cross) atomicAdd(counters + VOX_N_CROSSINGS, (unsigned long long)n_cross);
    }
}

// ---- raster ---------------------------------------------------------------------------------------------------------------
// Wave w of the launch takes work item w < n_items: block_offsets (the scanned block sums, low halves) and starts (the items
// before a triangle in its block) name its triangle and which 64 rows of the box.
__global__ __launch_bounds__(256) void rm_vox_raster_kernel(VoxLattice g, uint32_t n_triangles, uint32_t n_items, const uint32_t* __restrict__ tris,
                                                            const uint32_t* __restrict__ starts,
                                                            const unsigned long long* __restrict__ block_offsets, uint32_t* __restrict__ bits,
                                                            unsigned long long* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (item >= n_items) return;
    // the last block whose offset is <= item, then the last of its triangles whose start is <= what is left: neither is empty
    const uint32_t n_blocks = (n_triangles + kVoxBlock - 1u) / kVoxBlock;
    uint32_t lo = 0u, hi = n_blocks;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t)block_offsets[mid] <= item) lo = mid;
        else hi = mid;
    }
    const uint32_t local = item - (uint32_t)block_offsets[lo], t0 = lo * kVoxBlock;
    lo = 0u, hi = min(kVoxBlock, n_triangles - t0);
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[t0 + mid] <= local) lo = mid;
        else hi = mid;
    }
    const uint32_t t = t0 + lo, m = local - starts[t];
    const uint4* rec = reinterpret_cast<const uint4*>(tris + (size_t)t * kVoxTriWords);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const int q[9] = {(int)r0.x, (int)r0.y, (int)r0.z, (int)r0.w, (int)r1.x, (int)r1.y, (int)r1.z, (int)r1.w, (int)r2.x};
    const uint32_t j0 = r2.y & 0xFFFFu, k0 = r2.y >> 16, nj = r2.z & 0xFFFFu, nk = r2.z >> 16;
    const uint32_t row = m * 64u + lane;
    bool crossed = false;
    if (row < nj * nk) {
        const long long A2 = (long long)(q[4] - q[1]) * (long long)(q[8] - q[2]) - (long long)(q[5] - q[2]) * (long long)(q[7] - q[1]);
        const uint32_t dk = row / nj;
        crossed = vox_cross_row(q, A2, j0 + (row - dk * nj), k0 + dk, g, bits);
    }
    const uint32_t n_cross = (uint32_t)__popcll(__ballot(crossed));
    if (lane == 0u && n_cross) atomicAdd(counters + VOX_N_CROSSINGS, (unsigned long long)n_cross);
}

// ---- fill -----------------------------------------------------------------------------------------------------------------
// Workgroup b: the bytes [4096 b, 4096 b + 4096) of the n of the occupancy.  rows[16 b]: {inside points, open rows it owns (a row
// belongs to the workgroup that holds its first point), 0 ...}.
__global__ __launch_bounds__(256) void rm_vox_fill_kernel(uint32_t nx, uint32_t n, const uint32_t* __restrict__ bits, uint8_t* __restrict__ occ,
                                                          unsigned long long* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vox_smem[];
    __shared__ unsigned long long wred[4];
    constexpr rml::VoxFillLds L;
    uint32_t* s_raw = reinterpret_cast<uint32_t*>(vox_smem + L.raw);
    uint32_t* s_pre = reinterpret_cast<uint32_t*>(vox_smem + L.prefix);
    const uint32_t t = threadIdx.x, W = rml::vox_row_words(nx);
    const uint32_t p0 = blockIdx.x * rml::kVoxFillCells, p1 = min(p0 + rml::kVoxFillCells, n);
    const uint32_t r0 = p0 / nx, r1 = (p1 - 1u) / nx, nw = (r1 - r0 + 1u) * W;  // nw <= rml::kVoxFillMaxWords
    for (uint32_t x = t; x < nw; x += 256u) s_raw[x] = bits[(size_t)r0 * W + x];
    __syncthreads();
    uint32_t open = 0u, inside = 0u;
    for (uint32_t x = t; x < nw; x += 256u) {
        const uint32_t rl = x / W, w = x - rl * W;
        uint32_t before = 0u;
        for (uint32_t y = x - w; y < x; y++) before ^= s_raw[y];
        uint32_t v = s_raw[x];  // the inclusive prefix XOR of the word's bits, then the parity of the words before it
        v ^= v << 1;
        v ^= v << 2;
        v ^= v << 4;
        v ^= v << 8;
        v ^= v << 16;
        if (__popc(before) & 1u) v = ~v;
        s_pre[x] = v;
        // bit nx: the parity of all the row's crossings
        if (w == W - 1u && (size_t)(r0 + rl) * nx >= p0) open += (v >> (nx & 31u)) & 1u;
    }
    __syncthreads();
    const uint32_t p = p0 + t * 16u;
    if (p < p1) {
        uint32_t rl = p / nx, i = p - rl * nx;
        rl -= r0;
        uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t e = 0; e < 16u; e++) {
            if (p + e < p1) {
                const uint32_t b = (s_pre[rl * W + (i >> 5)] >> (i & 31u)) & 1u;
                out[e >> 2] |= b << (8u * (e & 3u));
                inside += b;
                if (++i == nx) i = 0u, rl++;
            }
        }
        if (p + 16u <= p1) {
            *reinterpret_cast<uint4*>(occ + p) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            for (uint32_t e = 0; p + e < p1; e++) occ[p + e] = (uint8_t)(out[e >> 2] >> (8u * (e & 3u)));
        }
    }
    block_row<32, 32>((unsigned long long)inside | (unsigned long long)open << 32, wred, rows);  // (4096 cells: far below 2^32 each)
}

}  // namespace rmk
