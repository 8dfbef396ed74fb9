// rm_class_mesh.h -- lattice meshing (rm_mesh_classes): the unit faces between the points of a class set A and their 6-neighbours
// of a class set B, on the padded lattice of rm_surface.h, as a welded, indexed triangle mesh in a fixed order.  Included by
// rm_abi.hip alone.  DESIGN.md section 29 is the contract; every output word is a function of the lattice alone, so no order of
// execution changes one.
//
// The CORNER lattice has (nx + 1)(ny + 1)(nz + 1) corners, corner (ci, cj, ck) at index position (ci - 1/2, cj - 1/2, ck - 1/2),
// L = ci + cx (cj + cy ck).  The 8 points around a corner are (ci - 1 + dx, cj - 1 + dy, ck - 1 + dz), point `dx + 2 dy + 4 dz` of
// the masks below; a corner OWNS the three faces whose lowest corner it is (the pairs of point 7 with the points 6, 5 and 3) and
// the three corner-lattice edges that leave it along +x, +y, +z (edge a: the four pairs inside the plane d_a = 1 of the 8 points).
// A point beyond the lattice has class 0, so a corner or an edge beyond the corner lattice has no face and needs no test.
//
// A WORD is 64 consecutive corners of an x row (a row has wpr = ceil(cx / 64) words, the last one partly beyond the row); the
// words in the order (ck, cj, word of the row) are the corners in the order of L.  A wave takes a word, a lane a corner.
//   mark   a workgroup takes kCmeshGroupWords consecutive words, four to a wave.  Per word: which corners are used (one ballot
//          word), and how many vertices and faces lie before the word in its workgroup (v | f << 16).  Per workgroup: its vertices
//          and faces packed lo | hi << 32 for rm_block_scan_kernel, and its counts as two rows (block_row).
//   emit   a wave takes a word again.  The rank of ANY corner is scanned[word / kCmeshGroupWords] + before[word] + popcount(used
//          bits below it): three loads, which is what lets a face name four corners that lie in other workgroups' words.
// The class bytes are read from memory as they lie (four byte loads a lane, the neighbour along x by a shuffle in mark; emit
// skips a word without a used corner): every byte serves four rows of corners, which neighbouring waves read out of the cache.
#pragma once
#include "rm_reduce.h"
#include "rm_surface.h"

namespace rmk {

constexpr uint32_t kCmeshWaveWords = 4u, kCmeshGroupWords = 4u * kCmeshWaveWords;  // words of a wave / of a workgroup in mark
constexpr uint32_t kCmeshNoId = 0xFFFFFFFFu;                                       // RM_NO_ID
// a workgroup has 1024 corners: before[] holds at most 1024 vertices and 3072 faces in its two halves, and a row's fields at most
// 1024 (11 bits) and 3072 (12 bits)
static_assert(kCmeshGroupWords * 64u == 1024u, "the widths of before[] and of the rows' fields");

struct CmeshGrid {
    uint32_t nx, ny, nz, cx, cy, wpr, n_words;
    float ox, oy, oz, sx, sy, sz;
    uint32_t mask_a, mask_b;
};

// Word w -> the corner of `lane`: c[0] may lie beyond the row (>= cx).
RM_DEV void cmesh_corner(const CmeshGrid& G, uint32_t w, uint32_t lane, uint32_t c[3]) {
    const uint32_t wx = w % G.wpr, r = w / G.wpr;
    c[0] = wx * 64u + lane;
    c[1] = r % G.cy;
    c[2] = r / G.cy;
}

// Point `bit` of a corner, of class k: bit `bit` of a8 when the class is in A, of b8 when in B.
RM_DEV void cmesh_member(const CmeshGrid& G, uint32_t k, uint32_t bit, uint32_t& a8, uint32_t& b8) {
    a8 |= ((G.mask_a >> k) & 1u) << bit;
    b8 |= ((G.mask_b >> k) & 1u) << bit;
}

// The pairs (point i, point i + 2^axis) that are faces, as bit i.
RM_DEV uint32_t cmesh_pairs(uint32_t a8, uint32_t b8, uint32_t axis) {
    const uint32_t sh = 1u << axis, low = axis == 0u ? 0x55u : axis == 1u ? 0x33u : 0x0Fu;
    return ((a8 & (b8 >> sh)) | (b8 & (a8 >> sh))) & low;
}

// An owned edge with n faces: EDGES | OPEN << 12 | BRANCH << 24 (the three 12-bit fields of the second row).
RM_DEV unsigned long long cmesh_edge(uint32_t n) {
    return (unsigned long long)(n != 0u) | (unsigned long long)(n & 1u) << 12 | (unsigned long long)(n >= 3u) << 24;
}

// ---- mark ---------------------------------------------------------------------------------------------------------------------
// rows: 2 gridDim.x rows; row g holds VERTICES and the x and y faces (entries 0-4), row gridDim.x + g the z faces and the edges
// (entries 5-9: five one-bit fields that stay 0 stand in front of them), so that one reduction sums both.
__global__ __launch_bounds__(256) void rm_cmesh_mark_kernel(CmeshGrid G, const uint8_t* __restrict__ cls, unsigned long long* __restrict__ bits,
                                                            uint32_t* __restrict__ before, unsigned long long* __restrict__ bsums,
                                                            unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long wred[8];
    __shared__ uint32_t s_cnt[kCmeshGroupWords];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    unsigned long long sum_a = 0ull, sum_b = 0ull;
    for (uint32_t r = 0; r < kCmeshWaveWords; r++) {
        const uint32_t slot = wave * kCmeshWaveWords + r, w = blockIdx.x * kCmeshGroupWords + slot;
        uint32_t used = 0u, nf = 0u;
        if (w < G.n_words) {  // (uniform over the wave)
            uint32_t c[3], a8 = 0u, b8 = 0u;
            cmesh_corner(G, w, lane, c);
            // the four rows (dy, dz) of the 8 points: a lane loads the point above it in x and takes the one below from its
            // neighbour; lane 0 loads that one as well
#pragma unroll
            for (uint32_t row = 0; row < 4u; row++) {
                const int gy = (int)c[1] - 1 + (int)(row & 1u), gz = (int)c[2] - 1 + (int)(row >> 1);
                const uint32_t hi = surf_class(cls, G.nx, G.ny, G.nz, (int)c[0], gy, gz);
                uint32_t lo = __shfl_up(hi, 1, 64);
                if (lane == 0u) lo = surf_class(cls, G.nx, G.ny, G.nz, (int)c[0] - 1, gy, gz);
                cmesh_member(G, lo, 2u * row, a8, b8);
                cmesh_member(G, hi, 2u * row + 1u, a8, b8);
            }
            const uint32_t fx = cmesh_pairs(a8, b8, 0u), fy = cmesh_pairs(a8, b8, 1u), fz = cmesh_pairs(a8, b8, 2u);
            used = (fx | fy | fz) != 0u;
            // the owned faces: point 7 (in B: the normal is positive) with the points 6, 5, 3
            const uint32_t pos = (b8 >> 7) & 1u, ox = (fx >> 6) & 1u, oy = (fy >> 5) & 1u, oz = (fz >> 3) & 1u;
            nf = ox + oy + oz;
            sum_a += (unsigned long long)used | (unsigned long long)(ox & pos) << 11 | (unsigned long long)(ox & ~pos) << 22 |
                     (unsigned long long)(oy & pos) << 33 | (unsigned long long)(oy & ~pos) << 44;
            sum_b += (unsigned long long)(oz & pos) << 5 | (unsigned long long)(oz & ~pos) << 16 |
                     (cmesh_edge(__popc(fy & 0x22u) + __popc(fz & 0x0Au)) + cmesh_edge(__popc(fx & 0x44u) + __popc(fz & 0x0Cu)) +
                      cmesh_edge(__popc(fx & 0x50u) + __popc(fy & 0x30u)))
                         << 27;
        }
        const unsigned long long ballot = __ballot(used != 0u);
        const uint32_t wf = wave_sum(nf);
        if (lane == 0u) {
            s_cnt[slot] = (uint32_t)__popcll(ballot) | wf << 16;
            if (w < G.n_words) bits[w] = ballot;
        }
    }
    __syncthreads();
    if (t < kCmeshGroupWords) {
        uint32_t v = 0u, f = 0u;
        for (uint32_t q = 0; q < t; q++) v += s_cnt[q] & 0xFFFFu, f += s_cnt[q] >> 16;
        const uint32_t w = blockIdx.x * kCmeshGroupWords + t;
        if (w < G.n_words) before[w] = v | f << 16;
        if (t == kCmeshGroupWords - 1u)
            bsums[blockIdx.x] = (unsigned long long)(v + (s_cnt[t] & 0xFFFFu)) | (unsigned long long)(f + (s_cnt[t] >> 16)) << 32;
    }
    block_row<11, 11, 11, 11, 11>(sum_a, wred, rows);
    block_row<1, 1, 1, 1, 1, 11, 11, 12, 12, 12>(sum_b, wred + 4, rows + (size_t)gridDim.x * kRowWords);
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------
// The vertex rank of the corner c (a used one).
RM_DEV uint32_t cmesh_rank(const CmeshGrid& G, const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ before,
                           const unsigned long long* __restrict__ bsums, const uint32_t c[3]) {
    const uint32_t w = (c[2] * G.cy + c[1]) * G.wpr + (c[0] >> 6);
    const unsigned long long below = bits[w] & ((1ull << (c[0] & 63u)) - 1ull);
    return (uint32_t)bsums[w / kCmeshGroupWords] + (before[w] & 0xFFFFu) + (uint32_t)__popcll(below);
}

// o + ((float)c - 0.5f) * s, the product and the sum rounded once each.
RM_DEV float cmesh_position(float o, uint32_t c, float s) { return __fadd_rn(o, __fmul_rn((float)c - 0.5f, s)); }

// The class and the linear index (kCmeshNoId: padding) of the point p.
RM_DEV uint2 cmesh_point(const CmeshGrid& G, const uint8_t* __restrict__ cls, const int p[3]) {
    if ((uint32_t)p[0] >= G.nx || (uint32_t)p[1] >= G.ny || (uint32_t)p[2] >= G.nz) return make_uint2(0u, kCmeshNoId);
    const uint32_t idx = ((uint32_t)p[2] * G.ny + (uint32_t)p[1]) * G.nx + (uint32_t)p[0];
    return make_uint2(min((uint32_t)cls[idx], kSurfClasses - 1u), idx);
}

// Wave w of the launch: word w.  vertices: 3 floats per vertex; triangles: 3 indices, ids: 2 words per triangle; any may be NULL
// only when the mesh is empty (the launch is skipped then).
__global__ __launch_bounds__(256) void rm_cmesh_emit_kernel(CmeshGrid G, const uint8_t* __restrict__ cls, const unsigned long long* __restrict__ bits,
                                                            const uint32_t* __restrict__ before, const unsigned long long* __restrict__ bsums,
                                                            float* __restrict__ vertices, uint32_t* __restrict__ triangles,
                                                            uint32_t* __restrict__ ids) {
    const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= G.n_words) return;  // (uniform over the wave; the kernel has no barrier)
    uint32_t c[3];
    cmesh_corner(G, w, lane, c);
    const unsigned long long word = bits[w];
    if (word == 0ull) return;  // (uniform: no corner of the word is used, so none owns a face)
    const unsigned long long base = bsums[w / kCmeshGroupWords];
    const uint32_t mine = before[w];
    if ((word >> lane) & 1ull) {
        const size_t v = (size_t)((uint32_t)base + (mine & 0xFFFFu) + (uint32_t)__popcll(word & ((1ull << lane) - 1ull)));
        vertices[3u * v] = cmesh_position(G.ox, c[0], G.sx);
        vertices[3u * v + 1u] = cmesh_position(G.oy, c[1], G.sy);
        vertices[3u * v + 2u] = cmesh_position(G.oz, c[2], G.sz);
    }
    // the owned faces again, from the four points they need
    const int hi[3] = {(int)c[0], (int)c[1], (int)c[2]};
    const uint2 q = cmesh_point(G, cls, hi);
    uint2 p[3];
    uint32_t exists = 0u, positive = 0u;
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        int lo[3] = {hi[0], hi[1], hi[2]};
        lo[a] -= 1;
        p[a] = cmesh_point(G, cls, lo);
        const uint32_t pa = (G.mask_a >> p[a].x) & 1u, pb = (G.mask_b >> p[a].x) & 1u, qa = (G.mask_a >> q.x) & 1u, qb = (G.mask_b >> q.x) & 1u;
        exists |= ((pa & qb) | (pb & qa)) << a;
        positive |= (pa & qb) << a;
    }
    const uint32_t nf = (uint32_t)__popc(exists);
    size_t f = (size_t)((uint32_t)(base >> 32) + (mine >> 16) + (wave_inclusive_sum(nf) - nf));
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        if (!((exists >> a) & 1u)) continue;
        const uint32_t u = (a + 1u) % 3u, v = (a + 2u) % 3u, pos = (positive >> a) & 1u;
        uint32_t c10[3] = {c[0], c[1], c[2]}, c11[3] = {c[0], c[1], c[2]}, c01[3] = {c[0], c[1], c[2]};
        c10[u] += 1u, c11[u] += 1u, c11[v] += 1u, c01[v] += 1u;
        const uint32_t q00 = cmesh_rank(G, bits, before, bsums, c), q10 = cmesh_rank(G, bits, before, bsums, c10),
                       q11 = cmesh_rank(G, bits, before, bsums, c11), q01 = cmesh_rank(G, bits, before, bsums, c01);
        uint32_t* tri = triangles + 6u * f;
        tri[0] = q00, tri[1] = pos ? q10 : q11, tri[2] = pos ? q11 : q10;
        tri[3] = q00, tri[4] = pos ? q11 : q01, tri[5] = pos ? q01 : q11;
        // the A side is the lower point when the normal is positive
        const uint2 sa = pos ? p[a] : q, sb = pos ? q : p[a];
        const uint32_t id0 = sa.x | sb.x << 8 | (2u * a + pos) << 16;
        uint32_t* id = ids + 4u * f;
        id[0] = id0, id[1] = sa.y, id[2] = id0, id[3] = sa.y;
        f++;
    }
}

}  // namespace rmk
