// rm_surface.h -- surface measures of a lattice of classes (rm_surface_solid, rm_surface_classes): how many ordered pairs of
// neighbouring points hold which two classes, for each of 13 directions.  Included by rm_abi.hip alone.  DESIGN.md section 25 is
// the contract; every output is a count, so no order of execution changes a word.
//
// Every point of the lattice has a class 0..7; the lattice counts as surrounded by one layer of class-0 points (the PADDED
// lattice, coordinates -1 .. n per axis).  PAIR[a][b][nu] counts the pairs (p, p + nu) of the padded lattice with class(p) = a and
// class(p + nu) = b; the pair belongs to p, its OWNER.  Every direction's first nonzero component is +1, so an owner reaches one
// point further on +x and one on either side in y and z.  A point beyond the lattice has class 0, and a pair with a point beyond
// the PADDED lattice can only be a pair of two class-0 points, which is not counted: the kernel needs no test for the padded
// lattice's own border, only the index test that makes a point beyond the lattice class 0.
//   count   a workgroup walks tiles of 64 x 16 x 8 owners of the padded lattice (rml::SurfTileLds): the tile's class bytes and
//           their halo staged in LDS, each byte of the lattice read from memory for one tile as an owner (and for up to seven
//           more as halo, from the cache); a wave takes a row of 64 owners at a time, a lane forms its 13 pairs from LDS.  Counts
//           go into the workgroup's table in LDS by 32-bit atomics -- one from one lane when the bin is the same in all 64 lanes
//           (the bulk: a wave inside one class), one per lane otherwise.  The workgroup writes its table as one row.
//   reduce  the rows summed in u64, eight bins to a workgroup.
#pragma once
#include "rm_device.h"
#include "rm_lds_layout.h"

namespace rmk {

constexpr uint32_t kSurfClasses = 8u, kSurfDirs = 13u, kSurfPairs = 8u;  // RM_SURF_CLASSES, RM_SURF_DIRS, the first pair bin
static_assert(rml::kSurfCounts == kSurfPairs + kSurfClasses * kSurfClasses * kSurfDirs, "8 point bins, 8 x 8 x 13 pair bins");

// The 13 directions in rm_surface_directions' order: axes, face diagonals, space diagonals.
struct SurfDir {
    int x, y, z;
};
__host__ __device__ constexpr SurfDir surf_dir(uint32_t d) {
    constexpr SurfDir dirs[kSurfDirs] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1},  {1, 1, 0}, {1, -1, 0}, {1, 0, 1},  {1, 0, -1},
                                         {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
    return dirs[d];
}

// One count per lane into `bin` of the table, for the lanes with `live`; all 64 lanes of the wave are here.  (`live` is a function
// of the bin, so it is uniform where the bin is.)
RM_DEV void surf_add(uint32_t* s_cnt, uint32_t bin, bool live, uint32_t lane) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
    if (__all(bin == first)) {
        if (live && lane == 0u) atomicAdd(s_cnt + first, 64u);
    } else if (live) {
        atomicAdd(s_cnt + bin, 1u);
    }
}

// The class of the point (gx, gy, gz): min(byte, 7) inside the lattice, 0 beyond it (negative coordinates wrap to large ones).
RM_DEV uint32_t surf_class(const uint8_t* __restrict__ cls, uint32_t nx, uint32_t ny, uint32_t nz, int gx, int gy, int gz) {
    if ((uint32_t)gx >= nx || (uint32_t)gy >= ny || (uint32_t)gz >= nz) return 0u;
    return min((uint32_t)cls[((uint32_t)gz * ny + (uint32_t)gy) * nx + (uint32_t)gx], kSurfClasses - 1u);
}

// ---- count --------------------------------------------------------------------------------------------------------------------
// Workgroup g: the tiles g, g + gridDim.x, ... of the tx x ty x tz tiles of the padded lattice; rows[g]: its table.
__global__ __launch_bounds__(256) void rm_surf_count_kernel(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t tx, uint32_t ty, uint32_t n_tiles,
                                                            const uint8_t* __restrict__ cls, uint32_t* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char surf_smem[];
    constexpr rml::SurfTileLds L;
    uint8_t* s_cls = surf_smem + L.cls;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(surf_smem + L.counts);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t b = t; b < rml::kSurfCounts; b += 256u) s_cnt[b] = 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t ti = tile % tx, r = tile / tx, tj = r % ty, tk = r / ty;
        const int x0 = (int)(ti * rml::kSurfTileX) - 1, y0 = (int)(tj * rml::kSurfTileY) - 1, z0 = (int)(tk * rml::kSurfTileZ) - 1;
        __syncthreads();  // the table is zero / the last tile's bytes have been read
        for (uint32_t row = wave; row < L.rows_y * L.rows_z; row += 4u) {
            const uint32_t cz = row / L.rows_y, cy = row - cz * L.rows_y;
            const int gy = y0 - 1 + (int)cy, gz = z0 - 1 + (int)cz;
            s_cls[row * L.pitch + lane] = (uint8_t)surf_class(cls, nx, ny, nz, x0 + (int)lane, gy, gz);
            if (lane == 0u) s_cls[row * L.pitch + rml::kSurfTileX] = (uint8_t)surf_class(cls, nx, ny, nz, x0 + (int)rml::kSurfTileX, gy, gz);
        }
        __syncthreads();
        for (uint32_t row = wave; row < rml::kSurfTileY * rml::kSurfTileZ; row += 4u) {
            const uint32_t lz = row / rml::kSurfTileY, ly = row - lz * rml::kSurfTileY;
            const uint8_t* own = s_cls + ((lz + 1u) * L.rows_y + ly + 1u) * L.pitch + lane;
            const uint32_t a = own[0];
            surf_add(s_cnt, a, a != 0u, lane);  // (POINTS[0] is what the other seven leave of the lattice: the reducer's)
#pragma unroll
            for (uint32_t d = 0; d < kSurfDirs; d++) {
                const SurfDir nu = surf_dir(d);
                const uint32_t b = own[(nu.z * (int)L.rows_y + nu.y) * (int)L.pitch + nu.x];
                const uint32_t key = a * kSurfClasses + b;
                surf_add(s_cnt, kSurfPairs + key * kSurfDirs + d, key != 0u, lane);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = t; b < rml::kSurfCounts; b += 256u) rows[(size_t)blockIdx.x * rml::kSurfCounts + b] = s_cnt[b];
}

// ---- reduce -------------------------------------------------------------------------------------------------------------------
// Workgroup w: the bins 8 w .. 8 w + 7 (kSurfCounts / 8 workgroups); thread t: bin 8 w + (t & 7) of the rows (t >> 3) + 32 k.
// result[0] = n_points - the points of the classes 1..7 is left to the host, which has all eight words.
__global__ __launch_bounds__(256) void rm_surf_reduce_kernel(const uint32_t* __restrict__ rows, uint32_t n_rows, unsigned long long* __restrict__ result) {
    __shared__ unsigned long long part[256];
    const uint32_t t = threadIdx.x, bin = blockIdx.x * 8u + (t & 7u);
    unsigned long long sum = 0ull;
    for (uint32_t g = t >> 3; g < n_rows; g += 32u) sum += rows[(size_t)g * rml::kSurfCounts + bin];
    part[t] = sum;
    __syncthreads();
    for (uint32_t s = 128u; s >= 8u; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t < 8u) result[bin] = part[t];
}
static_assert(rml::kSurfCounts % 8u == 0u, "the reducer's workgroups take eight bins each");

}  // namespace rmk
