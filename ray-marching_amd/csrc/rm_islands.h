// rm_islands.h -- layer regions and islands of the occupancy lattice {d < level} for one of the six axis directions as the build
// direction (rm_islands_solid, rm_islands_occupancy).  Included by rm_abi.hip alone, after rm_support.h, whose pack and overhang
// kernels give the bit planes `ins` and `ov` in the canonical frame (h, v, u) described there.  DESIGN.md section 22 is the
// contract; every output is a bit, a count, a sum of small integers, a minimum or a maximum, so no order of execution changes a
// word.
//
// A REGION is a 4-connected component of the inside points of one layer at or above the plate.  The point (h, v, u) has the
// canonical index p = (h * nv + v) * nu + u.  Within a layer that order, v then u, is the order of the caller's linear index for
// every direction (up z: (u, v) = (x, y); up y: (x, z); up x: (y, z); a negative direction turns only h), so the smallest
// canonical index of a region is its FIRST point, and numbering the roots of a min-root union-find in canonical order numbers the
// regions by (h, FIRST).  A = u and B = v in the region table.  The passes, each a launch of its own:
//   local     one wave per tile of 64 rows x one word column of one layer: a union-find over the tile's RUNS of set bits in LDS
//             (rml::IslTileLds), a run's representative its first bit, the smaller index the root; one parent per inside point
//   border    one lane per word: bit 63 with bit 0 of the next word, and the first row of a tile with the row before it, one
//             union per common run, by topo_unite (rm_topo_union.h) in device memory.  Never across layers
//   roots     every inside point at or above the plate is hung below its root; block sums of the root flags
//   scan      rm_block_scan_kernel; the host reads REGIONS and allocates the table
//   rank      the roots' numbers into `lab`, LAYER and FIRST into their rows, and per layer the regions before it
//   spread    lab[p] = lab[root of p], 0 for every other point
//   rows      one lane per word, a step per run: POINTS, SUPPORTED, the sums and the box by 32-bit integer atomics; per layer
//             the inside points
//   links     BELOW_MIN / BELOW_MAX: per point with a clear overhang bit the smallest and largest label of the disc in the
//             layer below, gathered from a tile of labels staged in LDS (rml::IslLinkLds), folded by atomicMin / atomicMax
//   finish    per region: no link -> BELOW_MIN = 0; islands and island points per layer, the merges; per layer its regions
//   compose   labels and mask in the caller's frame (with pack, the only pass that knows it)
#pragma once
#include "rm_lds_layout.h"
#include "rm_reduce.h"
#include "rm_support.h"

namespace rmk {

constexpr uint32_t kIslRowWords = 12u;  // RM_ISL_ROW_WORDS
constexpr uint32_t kIslLayer = 0u, kIslFirst = 1u, kIslPoints = 2u, kIslSupported = 3u, kIslSumA = 4u, kIslSumB = 5u, kIslMinA = 6u,
                   kIslMaxA = 7u, kIslMinB = 8u, kIslMaxB = 9u, kIslBelowMin = 10u, kIslBelowMax = 11u;  // RM_ISL_ROW_*
constexpr uint32_t kIslNone = 0xFFFFFFFFu;  // a minimum nothing has lowered yet

// The first bit of the run of set bits of `w` that holds bit b.
RM_DEV uint32_t isl_run_start(unsigned long long w, uint32_t b) {
    const unsigned long long low = ~w & ((1ull << b) - 1ull);
    return low != 0ull ? 64u - (uint32_t)__clzll((long long)low) : 0u;
}

// The canonical point p: its coordinates, and whether it is an inside point at or above the plate.
struct IslPoint {
    uint32_t h, v, u;
    bool live;
};
RM_DEV IslPoint isl_point(const SupFrame& f, uint32_t p, uint32_t n, uint32_t h0, const unsigned long long* __restrict__ ins) {
    IslPoint q;
    const uint32_t lp = f.nv * f.nu;
    q.h = p / lp;
    const uint32_t r = p - q.h * lp;
    q.v = r / f.nu;
    q.u = r - q.v * f.nu;
    q.live = p < n && q.h >= h0 && ((ins[(q.h * f.nv + q.v) * f.nw + (q.u >> 6)] >> (q.u & 63u)) & 1ull) != 0ull;
    return q;
}

// ---- local ------------------------------------------------------------------------------------------------------------------
// Workgroup (w, tile, h), one wave: lane l holds the word w of row v = 64 tile + l.
__global__ __launch_bounds__(64) void rm_isl_local_kernel(SupFrame f, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                          const unsigned long long* __restrict__ ins, uint32_t* __restrict__ parent) {
    extern __shared__ __attribute__((aligned(16))) unsigned char isl_smem[];
    constexpr rml::IslTileLds L;
    unsigned long long* s_word = reinterpret_cast<unsigned long long*>(isl_smem + L.words);
    uint32_t* s_par = reinterpret_cast<uint32_t*>(isl_smem + L.parent);
    const uint32_t lane = threadIdx.x, w = blockIdx.x, v0 = blockIdx.y * rml::kIslTile, h = blockIdx.z;
    if (h < sup_plate(plate, h0w)) return;  // under the plate: no regions (uniform over the workgroup)
    const uint32_t v = v0 + lane;
    const unsigned long long word = v < f.nv ? ins[(h * f.nv + v) * f.nw + w] : 0ull;
    s_word[lane] = word;
    for (unsigned long long m = word & ~(word << 1); m != 0ull; m &= m - 1ull) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m);
        s_par[lane * 64u + b] = lane * 64u + b;
    }
    __syncthreads();
    if (lane > 0u) {
        const unsigned long long above = s_word[lane - 1u], both = word & above;
        for (unsigned long long m = both & ~(both << 1); m != 0ull; m &= m - 1ull) {  // one union per common run
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            topo_unite(s_par, lane * 64u + isl_run_start(word, b), (lane - 1u) * 64u + isl_run_start(above, b), 4096u);
        }
    }
    __syncthreads();
    const uint32_t u = w * 64u + lane;
    for (uint32_t r = 0; r < rml::kIslTile; r++) {  // row r of the tile, lane l its bit l: 64 consecutive parents
        const unsigned long long wr = s_word[r];
        if (((wr >> lane) & 1ull) == 0ull) continue;  // (rows past nv and bits past nu are zero)
        const uint32_t root = topo_find<false>(s_par, r * 64u + isl_run_start(wr, lane), 4096u);
        parent[(h * f.nv + v0 + r) * f.nu + u] = (h * f.nv + v0 + (root >> 6)) * f.nu + w * 64u + (root & 63u);
    }
}

// ---- border -----------------------------------------------------------------------------------------------------------------
// Thread W: the word (h, v, w) of the plane.
__global__ __launch_bounds__(256) void rm_isl_border_kernel(SupFrame f, uint32_t n_words, uint32_t n, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                            const unsigned long long* __restrict__ ins, uint32_t* parent) {
    const uint32_t W = blockIdx.x * 256u + threadIdx.x;
    if (W >= n_words) return;
    const uint32_t w = W % f.nw, r = W / f.nw, v = r % f.nv, h = r / f.nv;
    if (h < sup_plate(plate, h0w)) return;
    const unsigned long long cur = ins[W];
    if (cur == 0ull) return;
    const uint32_t base = r * f.nu + w * 64u;  // the canonical index of bit 0
    if (w + 1u < f.nw && (cur >> 63) != 0ull && (ins[W + 1u] & 1ull) != 0ull) topo_unite(parent, base + 63u, base + 64u, n);
    if (v != 0u && (v & (rml::kIslTile - 1u)) == 0u) {
        const unsigned long long both = cur & ins[W - f.nw];
        for (unsigned long long m = both & ~(both << 1); m != 0ull; m &= m - 1ull) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            topo_unite(parent, base + b, base - f.nu + b, n);
        }
    }
}

// ---- roots, rank, spread ----------------------------------------------------------------------------------------------------
// Thread p: the canonical point p.
__global__ __launch_bounds__(256) void rm_isl_roots_kernel(SupFrame f, uint32_t n, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                           const unsigned long long* __restrict__ ins, uint32_t* parent,
                                                           unsigned long long* __restrict__ block_sums) {
    __shared__ unsigned long long wsum[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const IslPoint q = isl_point(f, p, n, sup_plate(plate, h0w), ins);
    unsigned long long flag = 0ull;
    if (q.live) {
        // (another thread's find may read this parent meanwhile: the old one and the root are both ancestors)
        const uint32_t root = topo_find<false>(parent, p, n);
        parent[p] = root;
        flag = root == p ? 1ull : 0ull;
    }
    unsigned long long total;
    (void)block_exclusive_sum<4>(flag, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// lab[root] = its region's number; LAYER and FIRST of its row; lbase[h] = the regions before layer h.
__global__ __launch_bounds__(256) void rm_isl_rank_kernel(SupFrame f, uint32_t n, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                          const unsigned long long* __restrict__ ins, const uint32_t* __restrict__ parent,
                                                          const unsigned long long* __restrict__ block_offsets, uint32_t* __restrict__ lab,
                                                          uint32_t* __restrict__ rows, uint32_t* __restrict__ lbase) {
    __shared__ unsigned long long wsum[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const IslPoint q = isl_point(f, p, n, sup_plate(plate, h0w), ins);
    const bool root = q.live && parent[p] == p;
    unsigned long long total;
    const uint32_t before = (uint32_t)(block_offsets[blockIdx.x] + block_exclusive_sum<4>(root ? 1ull : 0ull, wsum, total));
    if (p < n && q.v == 0u && q.u == 0u) lbase[q.h] = before;
    if (root) {
        lab[p] = before + 1u;
        uint32_t* row = rows + (size_t)before * kIslRowWords;
        row[kIslLayer] = q.h;
        row[kIslFirst] = q.u * f.su + q.v * f.sv + (f.neg ? f.nh - 1u - q.h : q.h) * f.sh;
    }
}

// (Only a root's entry is read here, and the rank pass wrote it; a root reads and writes its own.)
__global__ __launch_bounds__(256) void rm_isl_spread_kernel(SupFrame f, uint32_t n, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                            const unsigned long long* __restrict__ ins, const uint32_t* __restrict__ parent,
                                                            uint32_t* lab) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const IslPoint q = isl_point(f, p, n, sup_plate(plate, h0w), ins);
    lab[p] = q.live ? lab[parent[p]] : 0u;
}

__global__ __launch_bounds__(256) void rm_isl_rows_init_kernel(uint32_t n_words, uint32_t* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t k = i % kIslRowWords;
    rows[i] = k == kIslMinA || k == kIslMinB || k == kIslBelowMin ? kIslNone : 0u;
}

// ---- rows -------------------------------------------------------------------------------------------------------------------
// Workgroup (bx, h): 256 words of layer h, a lane per word and a step per run.  profile[4 h] (zero before the launch): the
// inside points of layer h.
__global__ __launch_bounds__(256) void rm_isl_rows_kernel(SupFrame f, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                          const unsigned long long* __restrict__ ins, const unsigned long long* __restrict__ ov,
                                                          const uint32_t* __restrict__ lab, uint32_t* rows, uint32_t* profile) {
    const uint32_t ncw = f.nv * f.nw, cw = blockIdx.x * 256u + threadIdx.x, h = blockIdx.y;
    const uint32_t h0 = sup_plate(plate, h0w);
    unsigned long long word = 0ull, over = 0ull;
    if (cw < ncw) {
        word = ins[h * ncw + cw];
        over = ov[h * ncw + cw];
    }
    uint32_t inside = (uint32_t)__popcll(word);
    inside = wave_sum(inside);
    if ((threadIdx.x & 63u) == 0u && inside != 0u) atomicAdd(profile + 4u * h, inside);
    if (h < h0) return;
    const uint32_t v = cw / f.nw, w = cw - v * f.nw;
    const uint32_t base = (h * f.nv + v) * f.nu + w * 64u;
    for (unsigned long long m = word; m != 0ull;) {
        const uint32_t s = (uint32_t)__builtin_ctzll(m);
        const unsigned long long run = m & ~(m + (1ull << s));  // (the carry clears the run; past bit 63 it falls away)
        m &= ~run;
        const uint32_t len = (uint32_t)__popcll(run), a0 = w * 64u + s;
        uint32_t* row = rows + (size_t)(lab[base + s] - 1u) * kIslRowWords;
        atomicAdd(row + kIslPoints, len);
        const uint32_t supported = h == h0 ? len : (uint32_t)__popcll(run & ~over);
        if (supported != 0u) atomicAdd(row + kIslSupported, supported);
        atomicAdd(row + kIslSumA, len * a0 + len * (len - 1u) / 2u);
        atomicAdd(row + kIslSumB, len * v);
        atomicMin(row + kIslMinA, a0);
        atomicMax(row + kIslMaxA, a0 + len - 1u);
        atomicMin(row + kIslMinB, v);
        atomicMax(row + kIslMaxB, v);
    }
}

// ---- links ------------------------------------------------------------------------------------------------------------------
// Workgroup (w, bv, h): the rows v = 16 bv + [0, 16) of the word column w of layer h; thread t the column 64 w + (t & 63) of the
// rows (t >> 6) + 4 k.  A minimum / maximum only ever falls / rises, so the plain read before an atomic only spares atomics.
__global__ __launch_bounds__(256) void rm_isl_links_kernel(SupFrame f, uint32_t r2, uint32_t reach, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                           const unsigned long long* __restrict__ ins, const unsigned long long* __restrict__ ov,
                                                           const uint32_t* __restrict__ lab, uint32_t* rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char isl_smem[];
    __shared__ uint32_t s_w[rml::kSupMaxReach + 1u];            // the half width of the disc at row offset d
    __shared__ unsigned long long s_cov[rml::kIslLinkRows];     // the tile's points that are no overhang
    const rml::IslLinkLds L(reach);
    uint32_t* s_lab = reinterpret_cast<uint32_t*>(isl_smem + L.labels);
    const uint32_t t = threadIdx.x, w = blockIdx.x, v0 = blockIdx.y * rml::kIslLinkRows, h = blockIdx.z;
    if (h <= sup_plate(plate, h0w)) return;  // on the plate or under it: no links (uniform over the workgroup)
    unsigned long long cov = 0ull;
    if (t < rml::kIslLinkRows) {
        const uint32_t v = v0 + t;
        if (v < f.nv) {
            const uint32_t at = (h * f.nv + v) * f.nw + w;
            cov = ins[at] & ~ov[at];
        }
        s_cov[t] = cov;
    }
    if (t <= reach) {
        uint32_t hw = 0u;
        while ((hw + 1u) * (hw + 1u) + t * t <= r2) hw++;
        s_w[t] = hw;
    }
    if (__syncthreads_or(cov != 0ull) == 0) return;  // nothing of this tile rests on the layer below
    const int u0 = (int)(w * 64u) - (int)reach, vb = (int)v0 - (int)reach;
    for (uint32_t q = t; q < L.rows * L.pitch; q += 256u) {
        const uint32_t rr = q / L.pitch, cc = q - rr * L.pitch;
        const int vv = vb + (int)rr, uu = u0 + (int)cc;
        s_lab[q] = vv >= 0 && vv < (int)f.nv && uu >= 0 && uu < (int)f.nu ? lab[((h - 1u) * f.nv + (uint32_t)vv) * f.nu + (uint32_t)uu] : 0u;
    }
    __syncthreads();
    const uint32_t lu = t & 63u;
    for (uint32_t lv = t >> 6; lv < rml::kIslLinkRows; lv += 4u) {
        if (((s_cov[lv] >> lu) & 1ull) == 0ull) continue;
        uint32_t mn = kIslNone, mx = 0u;  // mn: the smallest label - 1 (no label: 0 - 1, the largest word)
        for (uint32_t d = 0; d <= 2u * reach; d++) {
            const uint32_t hw = s_w[d < reach ? reach - d : d - reach];
            const uint32_t* row = s_lab + (lv + d) * L.pitch + lu + reach;
            for (int du = -(int)hw; du <= (int)hw; du++) {
                const uint32_t l = row[du];
                mn = min(mn, l - 1u);
                mx = max(mx, l);
            }
        }
        uint32_t* row = rows + (size_t)(lab[(h * f.nv + v0 + lv) * f.nu + w * 64u + lu] - 1u) * kIslRowWords;
        if (mn + 1u < __hip_atomic_load(row + kIslBelowMin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(row + kIslBelowMin, mn + 1u);
        if (mx > __hip_atomic_load(row + kIslBelowMax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(row + kIslBelowMax, mx);
    }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------
// Thread i: region i + 1, and layer i.  totals[0]: the merges (zero before the launch).
__global__ __launch_bounds__(256) void rm_isl_finish_kernel(uint32_t n_regions, uint32_t nh, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                            const uint32_t* __restrict__ lbase, uint32_t* rows, uint32_t* profile,
                                                            uint32_t* totals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t h0 = sup_plate(plate, h0w);
    if (i < nh) profile[4u * i + 1u] = (i + 1u < nh ? lbase[i + 1u] : n_regions) - lbase[i];
    if (i >= n_regions) return;
    uint32_t* row = rows + (size_t)i * kIslRowWords;
    const uint32_t h = row[kIslLayer];
    if (row[kIslBelowMin] == kIslNone) {
        row[kIslBelowMin] = 0u;
        if (h > h0) {
            atomicAdd(profile + 4u * h + 2u, 1u);
            atomicAdd(profile + 4u * h + 3u, row[kIslPoints]);
        }
    } else if (row[kIslBelowMin] != row[kIslBelowMax]) {
        atomicAdd(totals, 1u);
    }
}

// ---- compose ----------------------------------------------------------------------------------------------------------------
// Thread q: the point q of the caller's array.  (axis: 0, 1, 2 for x, y, z up.)
__global__ __launch_bounds__(256) void rm_isl_compose_kernel(SupFrame f, uint32_t axis, uint32_t nx, uint32_t ny, uint32_t n, uint32_t plate,
                                                             const uint32_t* __restrict__ h0w, const unsigned long long* __restrict__ ins,
                                                             const uint32_t* __restrict__ lab, const uint32_t* __restrict__ rows,
                                                             uint32_t* __restrict__ labels, uint8_t* __restrict__ mask) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t i = q % nx, r = q / nx, j = r % ny, k = r / ny;
    const uint32_t u = axis == 0u ? j : i, v = axis == 2u ? j : k, hh = axis == 0u ? i : axis == 1u ? j : k;
    const uint32_t h = f.neg ? f.nh - 1u - hh : hh;
    const bool inside = ((ins[(h * f.nv + v) * f.nw + (u >> 6)] >> (u & 63u)) & 1ull) != 0ull;
    const uint32_t l = inside ? lab[(h * f.nv + v) * f.nu + u] : 0u;  // (0 under the plate)
    labels[q] = l;
    uint8_t m = inside ? 1u : 0u;
    if (l != 0u && h > sup_plate(plate, h0w) && rows[(size_t)(l - 1u) * kIslRowWords + kIslBelowMin] == 0u) m = 2u;
    mask[q] = m;
}

}  // namespace rmk
