// rm_light.h -- lit rendering (rm_draw_lit): the draw's image with soft shadows and ambient occlusion marched through the
// same distance field.  Device code only (gfx950, wave64); included by rm_abi.hip alone, so neither the draw kernels nor the
// specialiser's embedded headers change.  The contract, to the last bit, is DESIGN.md section 13.
//
// Every distance goes through query_distance<LOOP> (rm_query.h), i.e. through the record loop the interpreter draw runs the
// program with; rays through sample_offset / gen_ray_at, normals through the draw's four taps, the floor through shade_floor,
// bytes through unorm8.  With both terms off the kernel performs shade_hit's operations in shade_hit's order, so the image
// is rm_draw's bit for bit.
//
// A wave owns a 2 x 2 block of pixels; its 64 lanes are their 16 AA samples each (lane = pixel << 4 | sample, one pixel per
// 16-lane row), the grouping that keeps a wave's rays together.  Rays are generated in the kernel:
// nothing is read from memory but the program's records (scalar cache) and, for tagged programs, the material table.  The
// kernel runs in phases -- primary march; taps, walk and floor; shadow march; occlusion taps; resolve -- and the wave
// reconverges between them; a phase no lane of the wave needs is jumped over (the phase bodies sit under one lane
// predicate each: an empty EXEC mask branches around them).  The template parameters SHADOW (S > 0) and AO (A > 0) remove
// a term's code altogether, so the identity configuration runs none of it.
#pragma once
#include "rm_query.h"

namespace rmk {

struct LightLaunch {       // enum rm_light, as the kernels take it
    float px, py, pz;      // P
    float shadow;          // S
    float softness;        // k
    float bias;            // b
    float shadow_max_t;
    uint32_t shadow_steps;
    float ao;              // A
    float ao_step, ao_falloff, ao_scale;
    uint32_t ao_taps;
};

struct LitFrame {
    rm_uniforms u;
    uint32_t W, H, row0, rows;  // rows [row0, row0 + rows) of a W x H frame
    uint32_t format;            // enum rm_format
    void* out;                  // rows x W pixels of 16 B (RGBA32F) or 4 B
};

// shadow(o, l) of the contract: the penumbra estimate min over the march of k h / t, 0 once the ray is inside a surface.
template <int LOOP>
RM_DEV float light_shadow(const QueryLaunch& Q, const LightLaunch& P, float* spill, float ox, float oy, float oz, float lx, float ly,
                          float lz) {
    float res = 1.0f, t = 0.0f;
    for (uint32_t i = 0; i < P.shadow_steps; i++) {
        const float h = query_distance<LOOP>(Q, spill, ox + lx * t, oy + ly * t, oz + lz * t);
        if (h < Q.min_dist) { res = 0.0f; break; }
        res = fmin_(res, (P.softness * h) / t);  // t = 0: +inf or NaN, both lose to res
        t = t + h;
        if (t > P.shadow_max_t) break;
    }
    return fmax_(res, 0.0f);
}

// ao(p, n) of the contract: how much closer than the tap distance the scene is along the normal, nearer taps weighing more.
template <int LOOP>
RM_DEV float light_ao(const QueryLaunch& Q, const LightLaunch& P, float* spill, float x, float y, float z, float nx, float ny, float nz) {
    float occ = 0.0f, w = 1.0f;
    for (uint32_t i = 1; i <= P.ao_taps; i++) {
        const float h = P.ao_step * (float)i;
        const float d = query_distance<LOOP>(Q, spill, x + nx * h, y + ny * h, z + nz * h);
        occ = occ + (h - d) * w;
        w = w * P.ao_falloff;
    }
    return fmin_(fmax_(1.0f - P.ao_scale * occ, 0.0f), 1.0f);
}

template <int LOOP, bool SHADOW, bool AO>
__global__ __launch_bounds__(256) void rm_draw_lit_kernel(QueryLaunch Q, LightLaunch P, LitFrame F) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bw = (F.W + 1u) >> 1, bh = (F.rows + 1u) >> 1;  // 2 x 2 blocks of the band
    const uint32_t block = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (block >= bw * bh) return;  // whole waves only (no barrier in this kernel)
    const uint32_t px = (block % bw) * 2u + ((lane >> 4) & 1u), ry = (block / bw) * 2u + (lane >> 5);
    const bool live = px < F.W && ry < F.rows;  // odd sizes: the pixels of an edge block outside the band idle
    float* spill = query_spill(Q.slots);

    // ---- phase 1: the primary ray and its march (ray_march, wgsl:87-115); a lane that is done waits for its wave ----
    const V4 ro = matvec(F.u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);  // wgsl:39-40
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;  // the point that is shaded: the hit step's position, or the floor point
    uint32_t kind = RM_HIT_NONE;
    if (live) {
        float sox, soy;
        sample_offset(F.u, (lane >> 2) & 3u, lane & 3u, sox, soy);  // wgsl:44-53: (i, j) = (sample / 4, sample % 4)
        gen_ray_at(F.u.inv_proj, F.u.inv_view, ro, screen_x(px, F.W), screen_y(F.row0 + ry, F.H), sox, soy, dx, dy, dz);
        float dist = 0.0f;
        for (uint32_t it = 0; it < Q.max_iter; it++) {  // wgsl:90
            const float qx = ro.x + dx * dist, qy = ro.y + dy * dist, qz = ro.z + dz * dist;  // wgsl:91
            const float sd = query_distance<LOOP>(Q, spill, qx, qy, qz);                      // wgsl:94
            if (sd < Q.min_dist) {  // wgsl:97
                kind = RM_HIT_SURFACE;
                hx = qx; hy = qy; hz = qz;
                break;
            }
            if (sd > Q.max_dist) break;  // wgsl:109-111
            dist += sd;                  // wgsl:114
        }
    }

    // ---- phase 2: what is shaded -- surface: normal, l, n.l, albedo; anything else that looks down: the floor ----
    float nx = 0.0f, ny = 1.0f, nz = 0.0f;  // the floor's normal
    float lx = 0.0f, ly = 0.0f, lz = 0.0f;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;  // albedo, or the floor's colour; the sky is (0, 0, 0) (wgsl:130)
    float ndl = 0.0f;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;  // origin of the shadow ray
    bool shadowed = false;                  // this lane marches a shadow ray
    if (kind == RM_HIT_SURFACE) {
        query_taps<LOOP>(Q, spill, hx, hy, hz, nx, ny, nz);
        query_normalize(nx, ny, nz);  // shade_hit, wgsl:98-103
        lx = hx - P.px; ly = hy - P.py; lz = hz - P.pz;  // pos - light_position
        const float ll = __builtin_sqrtf((lx * lx + ly * ly) + lz * lz);
        lx = lx / ll; ly = ly / ll; lz = lz / ll;
        ndl = (nx * lx + ny * ly) + nz * lz;
        ar = 0.4f; ag = 0.7f; ab = 0.1f;  // wgsl:105
        if (Q.materials != nullptr && Q.tagged) {  // extension: the albedo of the material the surface carries
            const float4 al = Q.materials[query_walk(Q, spill, hx, hy, hz) & 0xFFu];
            ar = al.x; ag = al.y; ab = al.z;
        }
        if constexpr (SHADOW) {
            shadowed = ndl > 0.0f;
            sx = hx + nx * P.bias; sy = hy + ny * P.bias; sz = hz + nz * P.bias;
        }
    } else if (live) {
        const float t = (-1.5f - ro.y) / dy;  // wgsl:117-120
        if (t > 0.0f) {
            kind = RM_HIT_FLOOR;
            const float g = 0.2f * (float)shade_floor(ro.y, ro.x, ro.z, dx, dy, dz);  // wgsl:121-127
            ar = 0.1f + g; ag = 0.1f + g; ab = 0.2f + g;
            hx = ro.x + dx * t; hy = -1.5f; hz = ro.z + dz * t;
            if constexpr (SHADOW) {
                lx = hx - P.px; ly = hy - P.py; lz = hz - P.pz;
                const float ll = __builtin_sqrtf((lx * lx + ly * ly) + lz * lz);
                lx = lx / ll; ly = ly / ll; lz = lz / ll;
                shadowed = ly > 0.0f;
                sx = hx; sy = -1.5f + P.bias; sz = hz;
            }
        }
    }

    // ---- phase 3: shadow rays along +l ----
    float shade = 1.0f;  // what multiplies the albedo (surface: kd) or the floor's colour (f)
    if constexpr (SHADOW) {
        float sh = 1.0f;
        if (shadowed) sh = light_shadow<LOOP>(Q, P, spill, sx, sy, sz, lx, ly, lz);
        shade = 1.0f - P.shadow * (1.0f - sh);
    }
    if (kind == RM_HIT_SURFACE) shade = fmax_(0.02f, SHADOW ? ndl * shade : ndl);

    // ---- phase 4: occlusion taps along the normal ----
    if constexpr (AO) {
        if (kind != RM_HIT_NONE) shade = shade * (1.0f - P.ao * (1.0f - light_ao<LOOP>(Q, P, spill, hx, hy, hz, nx, ny, nz)));
    }

    // ---- phase 5: resolve (fs_main, wgsl:64-75): sqrt per sample, the 16 samples of a pixel summed in sample order ----
    float cr = ar, cg = ag, cb = ab;
    if (kind == RM_HIT_SURFACE || ((SHADOW || AO) && kind == RM_HIT_FLOOR)) { cr = ar * shade; cg = ag * shade; cb = ab * shade; }
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
