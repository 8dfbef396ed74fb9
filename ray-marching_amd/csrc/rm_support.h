// rm_support.h -- overhangs and supports of the occupancy lattice {d < level} for one of the six axis directions as the build
// direction (rm_support_solid, rm_support_occupancy).  Included by rm_abi.hip alone, after rm_topology.h, whose probe and
// occupancy kernels fill the occupancy.  DESIGN.md section 21 is the contract; every output is a bit, a count or a minimum, so no
// order of execution changes a word.
//
// One bit per point is all the analysis needs, so the work runs on BIT PLANES in one canonical frame, whatever the direction:
//   h  the height (the up axis, turned round for a negative direction), nh layers
//   v  the in-layer axis that indexes the bit rows, nv rows per layer
//   u  the in-layer axis whose points are the bits of a row: nw = ceil(nu / 64) u64 words, bit b of word w is u = 64 w + b,
//      and the bits past nu are zero
// word (h, v, w) of a plane lies at (h * nv + v) * nw + w.  Up = +-z: (u, v, h) = (x, y, z); up = +-y: (x, z, y); up = +-x:
// (y, z, x).  The overhang disc du^2 + dv^2 <= r2 is symmetric, so which in-layer axis becomes the bits is free.  Only the first
// and the last pass know the caller's frame: they exist twice, for x in the layer (a wave turns 64 consecutive bytes into one
// word by a ballot, and back) and for x up (a lane holds the word of its own x, that is of its own layer, and walks the 64 bytes
// of its bits with the wave's lanes on consecutive x), so both read and write the byte arrays in whole lines.  Between them one
// set of kernels serves all six directions.  The passes, each a launch of its own (no workgroup reads what another one of the same
// launch wrote):
//   pack      occupancy bytes -> the plane `ins`; with an automatic plate, the lowest height that holds a bit by atomicMin (a
//             minimum: the same in every order)
//   overhang  ov(h) = ins(h) & ~cover, cover the layer below dilated by the disc: the OR over the row offset d of the row v + d
//             dilated along u by w(d) = floor(sqrt(r2 - d^2)), by shifts with the carries of the neighbouring words.  The rows
//             a tile of rows can see are staged in LDS once (rml::SupCoverLds)
//   columns   one lane carries the 64 columns of a word: top-down sup = F & ~ins, F = sup | ov (F: the first inside point above
//             is an overhang); bottom-up plt = sup & P, P &= ~ins (P: no inside point since the plate)
//   count     per layer the popcounts of the profile, the runs and the landings, by integer atomics
//   compose   the four planes -> the mask's bytes
#pragma once
#include "rm_lds_layout.h"
#include "rm_reduce.h"
#include "rm_topology.h"

namespace rmk {

constexpr uint32_t kSupPlateAuto = 0xFFFFFFFFu;  // RM_SUPPORT_PLATE_AUTO
constexpr uint32_t kSupWordsPerWave = 4u;        // pack and compose with x in the layer: words a wave handles
// The column pass has one thread per 64 columns, 1024 threads at 256^3, and each walks every layer twice: what it waits for is
// the latency of its loads.  One wave per workgroup spreads those few waves over as many CUs as there are.
constexpr uint32_t kSupColumnThreads = 64u;

// The canonical frame of a call.  A point (u, v, h) lies at u * su + v * sv + (neg ? nh - 1 - h : h) * sh of the caller's array.
struct SupFrame {
    uint32_t nu, nv, nh, nw;
    uint32_t su, sv, sh;
    uint32_t neg;
};

// The plate's height: the caller's, or the minimum the pack pass found (nothing found: 0).
RM_DEV uint32_t sup_plate(uint32_t plate, const uint32_t* __restrict__ h0w) {
    if (plate != kSupPlateAuto) return plate;
    const uint32_t h = *h0w;
    return h == kSupPlateAuto ? 0u : h;
}

RM_DEV void sup_note_height(uint32_t* h0w, uint32_t h) {
    // (the plain read only spares atomics: the word never grows, so a height at or above it cannot lower it)
    if (h < __hip_atomic_load(h0w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(h0w, h);
}

// ---- pack -------------------------------------------------------------------------------------------------------------------
// XUP = false (su = 1): wave g takes the words [4 g, 4 g + 4) of the plane, a ballot each.
// XUP = true (sh = 1, u = y): wave g takes one (v, w) and 64 consecutive x; lane l builds the word of layer x = 64 c + l.
template <bool XUP>
__global__ __launch_bounds__(256) void rm_sup_pack_kernel(SupFrame f, uint32_t n_tasks, uint32_t plate, const uint8_t* __restrict__ occ,
                                                          unsigned long long* __restrict__ ins, uint32_t* h0w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (!XUP) {
        // the four bytes first, so that their loads are in flight together; then the ballots
        uint8_t byte[kSupWordsPerWave];
        uint32_t height[kSupWordsPerWave];
#pragma unroll
        for (uint32_t k = 0; k < kSupWordsPerWave; k++) {
            const uint32_t W = g * kSupWordsPerWave + k;  // (uniform over the wave)
            const uint32_t w = W % f.nw, r = W / f.nw, v = r % f.nv, h = r / f.nv;
            const uint32_t u = w * 64u + lane, hh = f.neg ? f.nh - 1u - h : h;
            height[k] = h;
            byte[k] = W < n_tasks && u < f.nu ? occ[u + v * f.sv + hh * f.sh] : (uint8_t)0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kSupWordsPerWave; k++) {
            const uint32_t W = g * kSupWordsPerWave + k;
            const unsigned long long m = __ballot(byte[k] != 0u);
            if (lane == 0u && W < n_tasks) {
                ins[W] = m;
                if (plate == kSupPlateAuto && m != 0ull) sup_note_height(h0w, height[k]);
            }
        }
    } else {
        if (g >= n_tasks) return;
        const uint32_t n_chunks = (f.nh + 63u) >> 6;
        const uint32_t c = g % n_chunks, r = g / n_chunks, w = r % f.nw, v = r / f.nw;
        const uint32_t x = c * 64u + lane;
        const bool live = x < f.nh;
        const uint32_t h = f.neg ? f.nh - 1u - x : x;
        const uint32_t bits = min(64u, f.nu - w * 64u);
        unsigned long long word = 0ull;
        if (live) {
            const uint8_t* p = occ + x + v * f.sv + w * 64u * f.su;
            for (uint32_t b = 0; b < bits; b++) word |= (unsigned long long)(p[b * f.su] != 0u) << b;
            ins[(h * f.nv + v) * f.nw + w] = word;
        }
        if (plate == kSupPlateAuto) {
            uint32_t hm = live && word != 0ull ? h : kSupPlateAuto;
            hm = wave_min(hm);
            if (lane == 0u && hm != kSupPlateAuto) sup_note_height(h0w, hm);
        }
    }
}

// ---- overhang ---------------------------------------------------------------------------------------------------------------
// Workgroup (bx, h): the rows v = bx * tv + [0, tv) of layer h, thread t the word (t / nw, t % nw) of the tile (tv * nw <= 256).
// reach = floor(sqrt(r2)) <= 15.
__global__ __launch_bounds__(256) void rm_sup_overhang_kernel(uint32_t nv, uint32_t nw, uint32_t tv, uint32_t r2, uint32_t reach, uint32_t plate,
                                                              const uint32_t* __restrict__ h0w, const unsigned long long* __restrict__ ins,
                                                              unsigned long long* __restrict__ ov) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sup_smem[];
    __shared__ uint32_t s_w[rml::kSupMaxReach + 1u];  // w(d): the half width of the disc at row offset d
    unsigned long long* s_rows = sup_smem + rml::SupCoverLds(tv, reach, nw).rows / 8u;
    const uint32_t h = blockIdx.y, v0 = blockIdx.x * tv, ncw = nv * nw;
    const uint32_t t = threadIdx.x, lv = t / nw, wu = t - lv * nw, v = v0 + lv;
    const bool own = lv < tv && v < nv;
    const uint32_t at = h * ncw + v * nw + wu;  // (read and written only when own)
    if (h <= sup_plate(plate, h0w)) {           // under the plate or on it: nothing overhangs (uniform over the workgroup)
        if (own) ov[at] = 0ull;
        return;
    }
    if (t <= reach) {
        uint32_t w = 0u;
        while ((w + 1u) * (w + 1u) + t * t <= r2) w++;
        s_w[t] = w;
    }
    const uint32_t n_stage = (tv + 2u * reach) * nw;
    for (uint32_t q = t; q < n_stage; q += 256u) {
        const uint32_t r = q / nw, c = q - r * nw;
        const int vv = (int)v0 - (int)reach + (int)r;
        s_rows[q] = vv >= 0 && vv < (int)nv ? ins[(h - 1u) * ncw + (uint32_t)vv * nw + c] : 0ull;
    }
    __syncthreads();
    if (!own) return;
    unsigned long long cover = 0ull;
    for (uint32_t d = 0; d <= 2u * reach; d++) {
        const uint32_t w = s_w[d < reach ? reach - d : d - reach];
        const unsigned long long* row = s_rows + (lv + d) * nw;
        const unsigned long long cur = row[wu], prev = wu > 0u ? row[wu - 1u] : 0ull, next = wu + 1u < nw ? row[wu + 1u] : 0ull;
        unsigned long long acc = cur;
        for (uint32_t s = 1; s <= w; s++) acc |= (cur << s) | (prev >> (64u - s)) | (cur >> s) | (next << (64u - s));
        cover |= acc;
    }
    ov[at] = ins[at] & ~cover;
}

// ---- columns ----------------------------------------------------------------------------------------------------------------
// Thread cw: the 64 columns of word cw of every layer (16 layers' loads in flight at a time).
__global__ __launch_bounds__(kSupColumnThreads) void rm_sup_columns_kernel(uint32_t ncw, uint32_t nh, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                             const unsigned long long* __restrict__ ins, const unsigned long long* __restrict__ ov,
                                                             unsigned long long* __restrict__ sup, unsigned long long* __restrict__ plt) {
    const uint32_t cw = blockIdx.x * kSupColumnThreads + threadIdx.x;
    if (cw >= ncw) return;
    const uint32_t h0 = sup_plate(plate, h0w);
    unsigned long long F = 0ull;  // columns whose first inside point above is an overhang
#pragma unroll 16
    for (uint32_t h = nh; h-- > h0;) {
        const uint32_t at = h * ncw + cw;
        const unsigned long long s = F & ~ins[at];
        sup[at] = s;
        F = s | ov[at];
    }
    unsigned long long P = ~0ull;  // columns with no inside point since the plate
#pragma unroll 16
    for (uint32_t h = h0; h < nh; h++) {
        const uint32_t at = h * ncw + cw;
        plt[at] = sup[at] & P;
        P &= ~ins[at];
    }
    for (uint32_t h = 0; h < h0; h++) sup[h * ncw + cw] = plt[h * ncw + cw] = 0ull;
}

// ---- count ------------------------------------------------------------------------------------------------------------------
// Workgroup (bx, h): 256 words of layer h.  profile[4 h + 0..3]: inside, overhang, support on the plate, support on the part;
// extra[2 h + 0..1]: the support points of layer h directly below an overhang point, and those whose point below is inside.
// Both arrays are zero before the launch.
__global__ __launch_bounds__(256) void rm_sup_count_kernel(uint32_t ncw, uint32_t nh, uint32_t plate, const uint32_t* __restrict__ h0w,
                                                           const unsigned long long* __restrict__ ins, const unsigned long long* __restrict__ ov,
                                                           const unsigned long long* __restrict__ sup, const unsigned long long* __restrict__ plt,
                                                           uint32_t* profile, uint32_t* extra) {
    __shared__ uint32_t s_red[4][6];
    const uint32_t cw = blockIdx.x * 256u + threadIdx.x, h = blockIdx.y;
    const uint32_t h0 = sup_plate(plate, h0w);
    uint32_t c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (cw < ncw) {
        const uint32_t at = h * ncw + cw;
        const unsigned long long i = ins[at], s = sup[at], p = plt[at];
        c[0] = __popcll(i);
        c[1] = __popcll(ov[at]);
        c[2] = __popcll(p);
        c[3] = __popcll(s & ~p);
        if (h >= h0 && h + 1u < nh) c[4] = __popcll(ov[at + ncw] & ~i);
        if (h > h0) c[5] = __popcll(s & ins[at - ncw]);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        c[k] = wave_sum(c[k]);
        if ((threadIdx.x & 63u) == 0u) s_red[threadIdx.x >> 6][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 6u) {
        const uint32_t k = threadIdx.x, sum = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
        if (sum != 0u) atomicAdd(k < 4u ? profile + 4u * h + k : extra + 2u * h + (k - 4u), sum);
    }
}

// ---- compose ----------------------------------------------------------------------------------------------------------------
RM_DEV uint8_t sup_class(unsigned long long i, unsigned long long o, unsigned long long s, unsigned long long p, uint32_t b) {
    if ((i >> b) & 1ull) return (o >> b) & 1ull ? 2u : 1u;
    if ((s >> b) & 1ull) return (p >> b) & 1ull ? 3u : 4u;
    return 0u;
}

// The tasks of a wave are the pack kernel's.
template <bool XUP>
__global__ __launch_bounds__(256) void rm_sup_compose_kernel(SupFrame f, uint32_t n_tasks, const unsigned long long* __restrict__ ins,
                                                             const unsigned long long* __restrict__ ov, const unsigned long long* __restrict__ sup,
                                                             const unsigned long long* __restrict__ plt, uint8_t* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (!XUP) {
#pragma unroll
        for (uint32_t k = 0; k < kSupWordsPerWave; k++) {
            const uint32_t W = g * kSupWordsPerWave + k;  // (uniform over the wave)
            if (W < n_tasks) {
                const uint32_t w = W % f.nw, r = W / f.nw, v = r % f.nv, h = r / f.nv;
                const uint32_t u = w * 64u + lane, hh = f.neg ? f.nh - 1u - h : h;
                if (u < f.nu) mask[u + v * f.sv + hh * f.sh] = sup_class(ins[W], ov[W], sup[W], plt[W], lane);
            }
        }
    } else {
        if (g >= n_tasks) return;
        const uint32_t n_chunks = (f.nh + 63u) >> 6;
        const uint32_t c = g % n_chunks, r = g / n_chunks, w = r % f.nw, v = r / f.nw;
        const uint32_t x = c * 64u + lane;
        if (x >= f.nh) return;
        const uint32_t h = f.neg ? f.nh - 1u - x : x;
        const uint32_t at = (h * f.nv + v) * f.nw + w, bits = min(64u, f.nu - w * 64u);
        const unsigned long long i = ins[at], o = ov[at], s = sup[at], p = plt[at];
        uint8_t* m = mask + x + v * f.sv + w * 64u * f.su;
        for (uint32_t b = 0; b < bits; b++) m[b * f.su] = sup_class(i, o, s, p, b);
    }
}

}  // namespace rmk
