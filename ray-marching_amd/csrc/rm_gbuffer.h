// rm_gbuffer.h -- the G-buffer draw (rm_draw_gbuffer): per pixel, where the visible surface is, which way it faces, which
// primitive and material it shows, and how much of the pixel a selected range of commands covers.  Device code only (gfx950,
// wave64); included by rm_abi.hip alone, so neither the draw kernels nor the specialiser's embedded headers change.  The
// contract, to the last bit, is DESIGN.md section 14.
//
// Nothing new is defined per ray: the record of sample s of a pixel is what rm_cast_rays returns for the ray rm_camera_rays
// gives for it -- the same march through query_distance<LOOP>, the same taps and shade_hit, the same leaf walk, the same
// floor.  The feature is the fusion (rays generated in the kernel, nothing read but the program's records) and the per-pixel
// reduction: three masks by wave ballot, the step sum, and the record of the nearest sample (the minimum of (t, sample id)
// among the samples that hit something).
//
// ALL = true: a wave owns a 2 x 2 block of pixels; its 64 lanes are their 16 AA samples each (lane = pixel << 4 | sample, one
// pixel per 16-lane row), rm_draw_lit's layout.  ALL = false: one sample (or the centre ray) per pixel, one lane per pixel, a
// wave per 8 x 8 tile.  Both run in phases -- primary march; taps, walk and floor; reduction and stores -- and the wave
// reconverges between them.  Whether the taps and the walk run is decided by kernel arguments (wave-uniform branches).
#pragma once
#include "rm_query.h"

namespace rmk {

struct GBufferFrame {
    rm_uniforms u;
    uint32_t W, H, row0, rows;       // rows [row0, row0 + rows) of a W x H frame
    uint32_t sample;                 // ALL = false: 0..15, or RM_SAMPLE_CENTER
    uint32_t sel_first, sel_count;   // the selected range of command indices
    uint32_t taps, walk;             // 1: the hit record is wanted / the leaf is wanted (ids, or a non-empty selection's mask)
    float* geom;                     // rows x W x 8 floats, or nullptr
    uint32_t* ids;                   // rows x W x 4, or nullptr
    uint32_t* masks;                 // rows x W x 4, or nullptr
};

struct GBufferSample {  // what rm_cast_rays returns for one ray
    uint32_t kind, steps, leaf, mat;
    float4 h0, h1;      // (t, x, y, z), (nx, ny, nz, diffuse)
};

// One lane's ray: rm_camera_rays_kernel's ray for (px, row0 + ry, sample), then rm_cast_rays_kernel's body, operation for
// operation.  A lane that is not `live` marches nothing and returns the miss record with 0 steps.
template <int LOOP>
RM_DEV GBufferSample gbuffer_sample(const QueryLaunch& Q, const GBufferFrame& F, float* spill, bool live, uint32_t px, uint32_t ry,
                                    uint32_t sample) {
    // ---- phase 1: the primary ray and its march (ray_march, wgsl:87-115); a lane that is done waits for its wave ----
    const V4 ro = matvec(F.u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);  // wgsl:39-40
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    float dist = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;
    GBufferSample r;
    r.kind = RM_HIT_NONE;
    r.steps = 0u;
    r.leaf = RM_NO_ID;
    r.mat = RM_NO_ID;
    r.h0 = make_float4(__uint_as_float(0x7F800000u), 0.0f, 0.0f, 0.0f);
    r.h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) {
        float sox = 0.0f, soy = 0.0f;                                           // RM_SAMPLE_CENTER: the pixel centre
        if (sample < 16u) sample_offset(F.u, sample >> 2, sample & 3u, sox, soy);  // wgsl:44-53: (i, j) = (sample / 4, sample % 4)
        gen_ray_at(F.u.inv_proj, F.u.inv_view, ro, screen_x(px, F.W), screen_y(F.row0 + ry, F.H), sox, soy, dx, dy, dz);
        r.steps = Q.max_iter;
        for (uint32_t it = 0; it < Q.max_iter; it++) {  // wgsl:90
            const float qx = ro.x + dx * dist, qy = ro.y + dy * dist, qz = ro.z + dz * dist;  // wgsl:91
            const float sd = query_distance<LOOP>(Q, spill, qx, qy, qz);                      // wgsl:94
            if (sd < Q.min_dist) {  // wgsl:97
                r.kind = RM_HIT_SURFACE;
                hx = qx; hy = qy; hz = qz;
                r.steps = it + 1u;
                break;
            }
            if (sd > Q.max_dist) { r.steps = it + 1u; break; }  // wgsl:109-111
            dist += sd;                                          // wgsl:114
        }
    }

    // ---- phase 2: surface -- taps, shade_hit and the leaf walk; anything else that looks down: the floor ----
    if (r.kind == RM_HIT_SURFACE) {
        r.h0 = make_float4(dist, hx, hy, hz);
        if (F.taps) {
            float nx, ny, nz;
            query_taps<LOOP>(Q, spill, hx, hy, hz, nx, ny, nz);
            const float k = shade_hit(nx, ny, nz, hx, hy, hz);  // wgsl:98-103
            query_normalize(nx, ny, nz);
            r.h1 = make_float4(nx, ny, nz, k);
        }
        if (F.walk) {
            const uint32_t m = query_walk(Q, spill, hx, hy, hz);
            r.leaf = m >> 8; r.mat = m & 0xFFu;
        }
    } else if (live) {
        const float t = (-1.5f - ro.y) / dy;  // wgsl:117-120 (shade_floor)
        if (t > 0.0f) {                       // (rejects NaN)
            r.kind = RM_HIT_FLOOR;
            r.h0 = make_float4(t, ro.x + dx * t, -1.5f, ro.z + dz * t);
            r.h1 = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
        }
    }
    return r;
}

// The three records of one pixel, as 16-B stores.
RM_DEV void gbuffer_store(const GBufferFrame& F, size_t at, uint32_t surface, uint32_t floor, uint32_t selected, uint32_t steps,
                          uint32_t kind, uint32_t sample, uint32_t leaf, uint32_t mat, float4 h0, float4 h1) {
    if (F.masks != nullptr) reinterpret_cast<uint4*>(F.masks)[at] = make_uint4(surface, floor, selected, steps);
    if (F.ids != nullptr) reinterpret_cast<uint4*>(F.ids)[at] = make_uint4(kind, sample, leaf, mat);
    if (F.geom != nullptr) {
        reinterpret_cast<float4*>(F.geom)[2u * at] = h0;
        reinterpret_cast<float4*>(F.geom)[2u * at + 1u] = h1;
    }
}

template <int LOOP, bool ALL>
__global__ __launch_bounds__(256) void rm_draw_gbuffer_kernel(QueryLaunch Q, GBufferFrame F) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t unit = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // this wave's block or tile
    float* spill = query_spill(Q.slots);
    if constexpr (ALL) {
        const uint32_t bw = (F.W + 1u) >> 1, bh = (F.rows + 1u) >> 1;  // 2 x 2 blocks of the band
        if (unit >= bw * bh) return;  // whole waves only (no barrier in this kernel)
        const uint32_t px = (unit % bw) * 2u + ((lane >> 4) & 1u), ry = (unit / bw) * 2u + (lane >> 5);
        const bool live = px < F.W && ry < F.rows;  // odd sizes: the pixels of an edge block outside the band idle
        const uint32_t s = lane & 15u;
        const GBufferSample r = gbuffer_sample<LOOP>(Q, F, spill, live, px, ry, s);

        // ---- phase 3: the per-pixel reduction; every lane of the wave takes part, a row is one pixel ----
        const uint32_t shift = lane & 48u;  // this row's 16 bits of a ballot
        const bool selected = r.kind == RM_HIT_SURFACE && r.leaf - F.sel_first < F.sel_count;
        const uint32_t m_surface = (uint32_t)(__ballot(r.kind == RM_HIT_SURFACE) >> shift) & 0xFFFFu;
        const uint32_t m_floor = (uint32_t)(__ballot(r.kind == RM_HIT_FLOOR) >> shift) & 0xFFFFu;
        const uint32_t m_selected = (uint32_t)(__ballot(selected) >> shift) & 0xFFFFu;
        // the nearest sample: the minimum of (t, sample id) among the samples that hit; a sample that hit nothing carries
        // (+inf, 256 + id), which loses to every hit (a floor hit at t = +inf included).  No march is known to give a NaN t
        // (section 14); the key takes one as +inf all the same, so that the result cannot depend on the reduction's shape.
        float t = r.h0.x == r.h0.x ? r.h0.x : __uint_as_float(0x7F800000u);
        uint32_t id = r.kind != RM_HIT_NONE ? s : 256u + s;
        uint32_t steps = r.steps;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {  // xor butterfly inside the 16-lane row: every lane ends with the row's result
            const float ot = __shfl_xor(t, m, 16);
            const uint32_t oi = __shfl_xor(id, m, 16);
            steps += __shfl_xor(steps, m, 16);
            if (ot < t || (ot == t && oi < id)) { t = ot; id = oi; }
        }
        const bool any = id < 256u;
        const int w = (int)(id & 15u);  // no hit: every lane holds the miss record, lane 0's serves
        const uint32_t kind = __shfl(r.kind, w, 16), leaf = __shfl(r.leaf, w, 16), mat = __shfl(r.mat, w, 16);
        float4 h0, h1;
        h0.x = __shfl(r.h0.x, w, 16); h0.y = __shfl(r.h0.y, w, 16); h0.z = __shfl(r.h0.z, w, 16); h0.w = __shfl(r.h0.w, w, 16);
        h1.x = __shfl(r.h1.x, w, 16); h1.y = __shfl(r.h1.y, w, 16); h1.z = __shfl(r.h1.z, w, 16); h1.w = __shfl(r.h1.w, w, 16);
        if (live && s == 0u)  // one lane per pixel stores
            gbuffer_store(F, (size_t)ry * F.W + px, m_surface, m_floor, m_selected, steps, kind, any ? id : RM_NO_ID, leaf, mat, h0, h1);
    } else {
        const uint32_t tw = (F.W + 7u) >> 3, th = (F.rows + 7u) >> 3;  // 8 x 8 tiles of the band
        if (unit >= tw * th) return;
        const uint32_t px = (unit % tw) * 8u + (lane & 7u), ry = (unit / tw) * 8u + (lane >> 3);
        const bool live = px < F.W && ry < F.rows;
        const GBufferSample r = gbuffer_sample<LOOP>(Q, F, spill, live, px, ry, F.sample);
        // ---- phase 3: the sample set has one member; its bit index is its id ----
        if (live) {
            const uint32_t bit = 1u << F.sample;
            const bool selected = r.kind == RM_HIT_SURFACE && r.leaf - F.sel_first < F.sel_count;
            gbuffer_store(F, (size_t)ry * F.W + px, r.kind == RM_HIT_SURFACE ? bit : 0u, r.kind == RM_HIT_FLOOR ? bit : 0u,
                          selected ? bit : 0u, r.steps, r.kind, r.kind != RM_HIT_NONE ? F.sample : RM_NO_ID, r.leaf, r.mat, r.h0, r.h1);
        }
    }
}

}  // namespace rmk
