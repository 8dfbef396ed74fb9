// rm_lattice.h -- the lattice draw (rm_set_lattice, rm_draw_lattice, rm_cast_lattice): a lattice of class bytes as cubes, seen
// through the draws' camera or along a caller's rays.  Device code only (gfx950, wave64, plain C++, no scratch); included by
// rm_abi.hip alone.  DESIGN.md section 28 is the contract, to the last bit; tests/lattice_draw_ref.py restates it in numpy.
//
// The traversal (rm_lattice_walk.h, shared with a host program) reads bits only: one bit per point in u32 words along x (lat_row_words(nx) words a row), one bit per brick of
// 8 x 8 x 8 points (section 15's cut).  The class byte is fetched once, at the hit.  The plane between the points m - 1 and m of an
// axis is crossed at t(m) = (((float)m - 0.5f) - e) * r, a function of m alone: so the events of a ray are the merge of three
// monotone sequences, and a jump over an empty brick lands in the cell, with the record, that the walk cell by cell reaches --
// the brick's leaving event E is the smallest (t, axis) of its three leaving planes, and every other axis advances by the number
// of its planes inside the brick whose (t, axis) lies before E, a count that a binary search over at most 7 planes finds.
#pragma once
#include "rm_query.h"
#include "rm_reduce.h"
#include "rm_lattice_walk.h"

#ifndef RM_LAT_SKIP
#define RM_LAT_SKIP 1  // 0: rm_set_lattice sets every brick bit, so that the walk visits every cell (tools/ab_build.sh builds that
                       // library for the probe; the device code is the same)
#endif

namespace rmk {

constexpr uint32_t kLatFaceNone = 6u;  // RM_LAT_FACE_NONE
enum : uint32_t { LAT_N_POINTS = 0, LAT_N_BRICKS = 1, LAT_N_COUNTERS = 2 };

// ---- build: one lane per word of 32 points along x --------------------------------------------------------------------------
// bits[w] = the points' byte != 0; the bits of the (at most four) bricks the word touches are set by atomicOr, and the lane that
// sets one first counts the brick.  counters[LAT_N_POINTS], counters[LAT_N_BRICKS]: one atomic add per wave.
__global__ __launch_bounds__(256) void rm_lat_pack_kernel(uint32_t nx, uint32_t ny, uint32_t row_words, uint32_t n_words, uint32_t bx, uint32_t by,
                                                          const uint8_t* __restrict__ cls, uint32_t* __restrict__ bits,
                                                          uint32_t* __restrict__ bricks, unsigned long long* __restrict__ counters) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    uint32_t points = 0u, fresh = 0u;
    if (w < n_words) {
        const uint32_t row = w / row_words, x0 = (w - row * row_words) * 32u;
        const uint32_t count = nx - x0 < 32u ? nx - x0 : 32u;
        const uint8_t* p = cls + (size_t)row * nx + x0;
        uint32_t word = 0u;
        for (uint32_t x = 0; x < count; x++) word |= (p[x] != 0u ? 1u : 0u) << x;
        bits[w] = word;
        points = (uint32_t)__builtin_popcount(word);
        if (word != 0u) {
            const uint32_t j = row % ny, k = row / ny;
            const uint32_t base = ((k >> 3) * by + (j >> 3)) * bx + (x0 >> 3);
            for (uint32_t q = 0; q < 4u; q++) {
                if (((word >> (8u * q)) & 0xFFu) == 0u) continue;
                const uint32_t b = base + q, bit = 1u << (b & 31u);
                if ((atomicOr(&bricks[b >> 5], bit) & bit) == 0u) fresh++;
            }
        }
    }
    points = wave_sum(points);
    fresh = wave_sum(fresh);
    if ((threadIdx.x & 63u) == 0u) {
        if (points) atomicAdd(&counters[LAT_N_POINTS], (unsigned long long)points);
        if (fresh) atomicAdd(&counters[LAT_N_BRICKS], (unsigned long long)fresh);
    }
}

// What a ray sees: the record of rm_cast_rays (h0 = t, P; h1 = normal, diffuse), the ids and the colour.
struct LatSample {
    float4 h0, h1;
    uint4 ids;
    float r, g, b;
};
RM_DEV LatSample lat_shade(const LatGrid& G, float ox, float oy, float oz, float dx, float dy, float dz) {
    LatSample s;
    s.h0 = make_float4(__uint_as_float(0x7F800000u), 0.0f, 0.0f, 0.0f);
    s.h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s.ids = make_uint4(RM_HIT_NONE, RM_NO_ID, RM_NO_ID, RM_NO_ID);
    s.r = 0.0f; s.g = 0.0f; s.b = 0.0f;  // wgsl:130
    const LatRecord rec = lat_traverse<true>(G, ox, oy, oz, dx, dy, dz);
    if (rec.hit) {
        const float px = ox + dx * rec.t, py = oy + dy * rec.t, pz = oz + dz * rec.t;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, k = 0.02f;
        uint32_t face = kLatFaceNone;
        if (rec.axis != 3u) {
            const float sgn = rec.up ? -1.0f : 1.0f;  // against the direction of travel
            if (rec.axis == 0u) nx = sgn;
            else if (rec.axis == 1u) ny = sgn;
            else nz = sgn;
            face = 2u * rec.axis + (rec.up ? 0u : 1u);
            k = shade_hit(nx, ny, nz, px, py, pz);  // wgsl:98-103
        }
        const uint32_t cls = G.cls[rec.index];
        const float* al = G.materials + 4u * (cls < G.n_materials ? cls : G.n_materials - 1u);
        s.h0 = make_float4(rec.t, px, py, pz);
        s.h1 = make_float4(nx, ny, nz, k);
        s.ids = make_uint4(RM_HIT_SURFACE, rec.index, cls, face);
        s.r = al[0] * k; s.g = al[1] * k; s.b = al[2] * k;
    } else {
        const float t = (-1.5f - oy) / dy;  // wgsl:117-120 (shade_floor)
        if (t > 0.0f) {
            const float g = 0.2f * (float)shade_floor(oy, ox, oz, dx, dy, dz);  // wgsl:121-127
            s.r = 0.1f + g; s.g = 0.1f + g; s.b = 0.2f + g;
            s.h0 = make_float4(t, ox + dx * t, -1.5f, oz + dz * t);
            s.h1 = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
            s.ids.x = RM_HIT_FLOOR;
        }
    }
    return s;
}

// ---- rays: one lane per ray ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rm_cast_lattice_kernel(LatGrid G, uint32_t n, const float* __restrict__ rays, float* __restrict__ out_hit,
                                                              uint32_t* __restrict__ out_ids, float* __restrict__ out_rgb) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const LatSample s = lat_shade(G, rays[6u * i], rays[6u * i + 1u], rays[6u * i + 2u], rays[6u * i + 3u], rays[6u * i + 4u], rays[6u * i + 5u]);
    if (out_hit != nullptr) {  // 32 B per ray: two 16-B stores
        reinterpret_cast<float4*>(out_hit)[2u * i] = s.h0;
        reinterpret_cast<float4*>(out_hit)[2u * i + 1u] = s.h1;
    }
    if (out_ids != nullptr) reinterpret_cast<uint4*>(out_ids)[i] = s.ids;
    if (out_rgb != nullptr) { out_rgb[3u * i] = s.r; out_rgb[3u * i + 1u] = s.g; out_rgb[3u * i + 2u] = s.b; }
}

// ---- draw: rm_draw_lit's layout -- one wave per 2 x 2 block of pixels, a lane per AA sample -----------------------------------
struct LatFrame {
    rm_uniforms u;
    uint32_t W, H, row0, rows;
    int format;  // RM_OPT_OUTPUT_FORMAT
    void* out;   // rows x W pixels
};
__global__ __launch_bounds__(256) void rm_draw_lattice_kernel(LatGrid G, LatFrame F) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bw = (F.W + 1u) >> 1, bh = (F.rows + 1u) >> 1;  // 2 x 2 blocks of the band
    const uint32_t block = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (block >= bw * bh) return;  // whole waves only (no barrier in this kernel)
    const uint32_t px = (block % bw) * 2u + ((lane >> 4) & 1u), ry = (block / bw) * 2u + (lane >> 5);
    const bool live = px < F.W && ry < F.rows;  // odd sizes: the pixels of an edge block outside the band idle
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (live) {
        const V4 ro = matvec(F.u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);  // wgsl:39-40
        float sox, soy, dx, dy, dz;
        sample_offset(F.u, (lane >> 2) & 3u, lane & 3u, sox, soy);  // wgsl:44-53: (i, j) = (sample / 4, sample % 4)
        gen_ray_at(F.u.inv_proj, F.u.inv_view, ro, screen_x(px, F.W), screen_y(F.row0 + ry, F.H), sox, soy, dx, dy, dz);
        const LatSample s = lat_shade(G, ro.x, ro.y, ro.z, dx, dy, dz);
        cr = s.r; cg = s.g; cb = s.b;
    }
    // resolve (fs_main, wgsl:64-75): sqrt per sample, the 16 samples of a pixel summed in sample order
    cr = __builtin_sqrtf(cr); cg = __builtin_sqrtf(cg); cb = __builtin_sqrtf(cb);
    float tr = 0.0f, tg = 0.0f, tb = 0.0f;
#pragma unroll
    for (int s = 0; s < 16; s++) {  // every lane of a row reads its row's lanes in order: a tree would round differently
        tr += __shfl(cr, s, 16);
        tg += __shfl(cg, s, 16);
        tb += __shfl(cb, s, 16);
    }
    if (live && (lane & 15u) == 0u) {  // one store per pixel
        const size_t at = (size_t)ry * F.W + px;
        const float r = tr / 16.0f, g = tg / 16.0f, b = tb / 16.0f;
        if (F.format == RM_FORMAT_RGBA32F) {
            reinterpret_cast<float4*>(F.out)[at] = make_float4(r, g, b, 1.0f);  // wgsl:73-75
        } else {
            const uint32_t qr = unorm8(r), qg = unorm8(g), qb = unorm8(b);
            const bool bgra = F.format == RM_FORMAT_BGRA8_UNORM;
            reinterpret_cast<uint32_t*>(F.out)[at] = (bgra ? qb : qr) | (qg << 8) | ((bgra ? qr : qb) << 16) | 0xFF000000u;
        }
    }
}

}  // namespace rmk
