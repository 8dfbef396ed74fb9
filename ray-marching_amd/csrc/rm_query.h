// rm_query.h -- scene queries (rm_query_points, rm_cast_rays, rm_camera_rays): what the scene the draws render says at
// a point or along a ray.  Device code only (gfx950, wave64); included by rm_abi.hip alone, so neither the draw kernels nor
// the specialiser's embedded headers change.
//
// Every value goes through the operations of the draw path (rm_interp.h, rm_kernels.h) in the same order: distances
// through the record loop the interpreter draw runs the program with (chain, tree or the general loop, fast square root
// behind its SqrtGuard), normals through the draw's four taps and shade_hit, rays through gen_ray_at.  So the results are
// bit-identical to the oracle under the arithmetic contract, and a frame resolved from cast sample
// rays is bit-identical to rm_draw's.
//
// One lane per point, ray or pixel; 256-thread workgroups; records are wave-uniform and come through the scalar data cache
// (ProgSmem: one s_load_dwordx8 per record), so program size is bounded by the command buffer, never by LDS.  The value
// stacks live in per-wave LDS columns [slot][lane], sized by the host from the program's actual depths.
#pragma once
#include "rm_interp.h"
#include "rm_kernel_v5.h"  // anchor_reach, anchor_thr_base for rm_selftest_anchor_kernel

namespace rmk {

enum : uint32_t { Q_LOOP_GENERAL = 0, Q_LOOP_CHAIN = 1, Q_LOOP_TREE = 3 };  // the RM_INFO_INTERPRETER_LOOP numbers

struct QueryLaunch {
    const RmRecord* prog;      // the draw's decoding (RmDecoded::rec): distances
    const RmRecord* qprog;     // the query program (RmDecoded::qrec): leaf and material walk
    uint32_t n_rec, n_qrec;
    uint32_t value_spill_depth;  // RmDecoded::spill_depth: the general loop's saved positions start at this slot
    uint32_t q_value_depth;      // RmDecoded::q_spill_depth: the walk's layout (below)
    uint32_t slots;              // LDS dwords per lane of a wave's column: the larger of the two needs
    uint32_t tagged;             // 1: the program carries Material tags (rgb takes the albedo of the walk's material)
    float min_dist, max_dist;
    uint32_t max_iter;
    const float4* materials;     // the context's material table (tagged programs with rgb requested), else nullptr
};

// map_scene (wgsl:187-203) at one point per lane, through the loop the interpreter draw uses for this program
// (rm_kernel_v5.h eval_scene with every unit needed): the fast square root first, the generic one for the whole wave
// when any lane's argument is outside its range.
template <int LOOP>
RM_DEV float query_distance(const QueryLaunch& Q, float* spill, float x, float y, float z) {
    ProgSmem prog{Q.prog};
    SqrtGuard tiny;
    if constexpr (LOOP == Q_LOOP_CHAIN) {
        float v = map_scene_chain<true>(prog, Q.n_rec, x, y, z, ~0ull, false, tiny);
        if (tiny.any_bad()) v = map_scene_chain<false>(prog, Q.n_rec, x, y, z, ~0ull, false, tiny);
        return v;
    } else if constexpr (LOOP == Q_LOOP_TREE) {
        float v = map_scene_tree<true>(prog, Q.n_rec, spill, x, y, z, tiny);
        if (tiny.any_bad()) v = map_scene_tree<false>(prog, Q.n_rec, spill, x, y, z, tiny);
        return v;
    } else {
        const float qx[1] = {x}, qy[1] = {y}, qz[1] = {z};
        float v[1];
        map_scene_multi<1, true, ProgSmem, true>(prog, Q.n_rec, spill, Q.max_dist, qx, qy, qz, v, tiny, Q.value_spill_depth);
        if (tiny.any_bad()) map_scene_multi<1, false, ProgSmem, true>(prog, Q.n_rec, spill, Q.max_dist, qx, qy, qz, v, tiny, Q.value_spill_depth);
        return v[0];
    }
}

// Which primitive and which material the value of map_scene at (x, y, z) carries: map_scene_material (rm_interp.h) with the
// primitive's command index (RmDecoded::qrec p[6]) carried next to the material index.  A primitive carries its own index and
// material 0; an operator keeps the entry of the operand that decides its result (Union / SmoothUnion b < a, Subtraction
// -b > a, Intersection b > a take b's, ties and NaN a's); a tag sets the material on top; transforms keep both.  The pair is
// packed leaf << 8 | material (command indices < 2^14, materials < 2^8).  Per lane column (`spill` points at this lane):
// [depth] distances, [depth] packed pairs, 3 floats per transform level.  Every distance takes the generic square root,
// which is bit for bit what the guarded fast one gives.
RM_DEV uint32_t query_walk(const QueryLaunch& Q, float* spill, float x, float y, float z) {
    const uint32_t depth = Q.q_value_depth;
    float acc = 0.0f;
    uint32_t accm = 0u, sp = 0u;
    uint32_t* mspill = reinterpret_cast<uint32_t*>(spill) + (size_t)depth * 64u;
    float* saved = spill + (size_t)2u * depth * 64u;
    SqrtGuard unused;
    for (uint32_t c = 0; c < Q.n_qrec; c++) {
        const RmRecord& r = Q.qprog[c];  // wave-uniform address: scalar loads
        const uint32_t op = __builtin_amdgcn_readfirstlane(r.op), kind = RM_OP_KIND(op), mode = RM_OP_MODE(op);
        float p[7];
#pragma unroll
        for (int k = 0; k < 7; k++) p[k] = r.p[k];
        if (kind == RM_KIND_MATERIAL) {
            accm = (accm & ~0xFFu) | __float_as_uint(p[0]);
            continue;
        }
        if (kind == RM_KIND_XFORM) {
            float* save = saved + (size_t)3u * __float_as_uint(p[6]) * 64u;
            if ((mode & 1u) == 0u) {
                save[0] = x; save[64] = y; save[128] = z;
                if (mode == RM_XF_T_PUSH) { x = x - p[0]; y = y - p[1]; z = z - p[2]; }
                else if (mode == RM_XF_R_PUSH) xf_rotate_conj(p[0], p[1], p[2], p[3], x, y, z);
                else { x = x / p[0]; y = y / p[0]; z = z / p[0]; }
            } else {
                x = save[0]; y = save[64]; z = save[128];
                if (mode == RM_XF_S_POP) acc = acc * p[0];
            }
            continue;
        }
        float a, b;
        uint32_t am, bm;
        if (kind == RM_KIND_POP) {
            --sp;
            b = acc; bm = accm;
            a = spill[sp * 64u]; am = mspill[sp * 64u];
        } else {
            if (kind == RM_KIND_SPHERE) b = sdf_sphere_t<false>(x, y, z, p, unused);
            else if (kind == RM_KIND_BOX) b = sdf_box_t<false>(x, y, z, p, unused);
            else if (kind == RM_KIND_CYLINDER) b = sdf_cylinder_t<false>(x, y, z, p, unused);
            else b = ((x * p[0] + y * p[1]) + z * p[2]) + p[3];
            bm = __float_as_uint(p[6]) << 8;  // this primitive, material 0
            if (op & RM_OP_SPILL) {
                spill[sp * 64u] = acc; mspill[sp * 64u] = accm;
                ++sp;
            }
            a = acc; am = accm;
        }
        if (mode == RM_MODE_PUSH) {
            acc = b; accm = bm;
        } else if (mode == RM_MODE_UNION) {
            acc = vmin(a, b); accm = b < a ? bm : am;
        } else if (mode == RM_MODE_SUB) {
            acc = vmax_negb(a, b); accm = -b > a ? bm : am;
        } else if (mode == RM_MODE_INTER) {
            acc = fmax_(a, b); accm = b > a ? bm : am;
        } else {  // RM_MODE_SMOOTH
            acc = material_smooth_union(p[0], a, b); accm = b < a ? bm : am;
        }
    }
    return accm;
}

// calculate_normal (wgsl:135-144) as the draw computes it: taps k.xyy, k.yyx, k.yxy, k.xxx (k = (1,-1), eps = 0.0001),
// summed as in rm_render_pixel; (nx, ny, nz) is the sum before normalisation (shade_hit normalises it).
template <int LOOP>
RM_DEV void query_taps(const QueryLaunch& Q, float* spill, float x, float y, float z, float& nx, float& ny, float& nz) {
    const float eps = 0.0001f;
    const float f0 = query_distance<LOOP>(Q, spill, x + eps, y + -eps, z + -eps);
    const float f1 = query_distance<LOOP>(Q, spill, x + -eps, y + -eps, z + eps);
    const float f2 = query_distance<LOOP>(Q, spill, x + -eps, y + eps, z + -eps);
    const float f3 = query_distance<LOOP>(Q, spill, x + eps, y + eps, z + eps);
    nx = ((f0 + -f1) + -f2) + f3;
    ny = ((-f0 + -f1) + f2) + f3;
    nz = ((-f0 + f1) + -f2) + f3;
}
// normalize3 of the oracle, the first three lines of shade_hit
RM_DEV void query_normalize(float& nx, float& ny, float& nz) {
    const float nl = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
    nx = nx / nl; ny = ny / nl; nz = nz / nl;
}

// This lane's column of the wave's LDS stack area (rml::QueryLds, from which the host sizes the launch).
RM_DEV float* query_spill(uint32_t slots) {
    extern __shared__ __attribute__((aligned(16))) float qsmem[];
    return qsmem + (size_t)(threadIdx.x / rml::kQueryLanes) * slots * rml::kQueryLanes + (threadIdx.x % rml::kQueryLanes);
}

// ---- points: distance, normal, (leaf, material) -----------------------------------------------------------------------
template <int LOOP, bool DIST, bool NORMAL, bool IDS>
__global__ __launch_bounds__(256) void rm_query_points_kernel(QueryLaunch Q, uint32_t n, const float* __restrict__ xyz,
                                                              float* __restrict__ out_dist, float* __restrict__ out_normal,
                                                              uint32_t* __restrict__ out_ids) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;  // (no barrier in this kernel; the record loops only need the lanes that are left)
    float* spill = query_spill(Q.slots);
    const float x = xyz[3u * i], y = xyz[3u * i + 1u], z = xyz[3u * i + 2u];
    if constexpr (DIST) out_dist[i] = query_distance<LOOP>(Q, spill, x, y, z);
    if constexpr (NORMAL) {
        float nx, ny, nz;
        query_taps<LOOP>(Q, spill, x, y, z, nx, ny, nz);
        query_normalize(nx, ny, nz);
        out_normal[3u * i] = nx; out_normal[3u * i + 1u] = ny; out_normal[3u * i + 2u] = nz;
    }
    if constexpr (IDS) {
        uint2 ids;
        if (Q.n_qrec == 0u) {  // wgsl:189-191: no primitive; the oracle's material is 0
            ids.x = RM_NO_ID; ids.y = 0u;
        } else {
            const uint32_t m = query_walk(Q, spill, x, y, z);
            ids.x = m >> 8; ids.y = m & 0xFFu;
        }
        reinterpret_cast<uint2*>(out_ids)[i] = ids;
    }
}

// ---- rays: ray_march (wgsl:87-131) per lane -----------------------------------------------------------------------------
// TAPS: the hit record or the colour is wanted (normal, diffuse); WALK: the ids are wanted, or the colour of a tagged program.
template <int LOOP, bool TAPS, bool WALK>
__global__ __launch_bounds__(256) void rm_cast_rays_kernel(QueryLaunch Q, uint32_t n, const float* __restrict__ rays,
                                                           float* __restrict__ out_hit, uint32_t* __restrict__ out_ids,
                                                           float* __restrict__ out_rgb) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float* spill = query_spill(Q.slots);
    const float ox = rays[6u * i], oy = rays[6u * i + 1u], oz = rays[6u * i + 2u];
    const float dx = rays[6u * i + 3u], dy = rays[6u * i + 4u], dz = rays[6u * i + 5u];
    // the march: a lane that is done waits for the last lane of its wave
    float dist = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;
    uint32_t steps = Q.max_iter, kind = RM_HIT_NONE;
    for (uint32_t it = 0; it < Q.max_iter; it++) {  // wgsl:90
        const float px = ox + dx * dist, py = oy + dy * dist, pz = oz + dz * dist;  // wgsl:91
        const float sd = query_distance<LOOP>(Q, spill, px, py, pz);               // wgsl:94
        if (sd < Q.min_dist) {  // wgsl:97
            kind = RM_HIT_SURFACE;
            hx = px; hy = py; hz = pz;
            steps = it + 1u;
            break;
        }
        if (sd > Q.max_dist) { steps = it + 1u; break; }  // wgsl:109-111
        dist += sd;                                         // wgsl:114
    }
    float4 h0 = make_float4(__uint_as_float(0x7F800000u), 0.0f, 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;  // wgsl:130
    uint32_t leaf = RM_NO_ID, mat = RM_NO_ID;
    if (kind == RM_HIT_SURFACE) {
        float k = 0.0f;
        if constexpr (TAPS) {
            float nx, ny, nz;
            query_taps<LOOP>(Q, spill, hx, hy, hz, nx, ny, nz);
            k = shade_hit(nx, ny, nz, hx, hy, hz);  // wgsl:98-103
            query_normalize(nx, ny, nz);
            h0 = make_float4(dist, hx, hy, hz);
            h1 = make_float4(nx, ny, nz, k);
        }
        cr = 0.4f * k; cg = 0.7f * k; cb = 0.1f * k;  // wgsl:105
        if constexpr (WALK) {
            const uint32_t m = query_walk(Q, spill, hx, hy, hz);
            leaf = m >> 8; mat = m & 0xFFu;
            if (Q.materials != nullptr && Q.tagged) {  // extension: the albedo of the material the surface carries
                const float4 al = Q.materials[mat];
                cr = al.x * k; cg = al.y * k; cb = al.z * k;
            }
        }
    } else {
        const float t = (-1.5f - oy) / dy;  // wgsl:117-120 (shade_floor)
        if (t > 0.0f) {
            kind = RM_HIT_FLOOR;
            const float g = 0.2f * (float)shade_floor(oy, ox, oz, dx, dy, dz);  // wgsl:121-127
            cr = 0.1f + g; cg = 0.1f + g; cb = 0.2f + g;
            h0 = make_float4(t, ox + dx * t, -1.5f, oz + dz * t);
            h1 = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
        }
    }
    if (out_hit != nullptr) {  // 32 B per ray: two 16-B stores
        reinterpret_cast<float4*>(out_hit)[2u * i] = h0;
        reinterpret_cast<float4*>(out_hit)[2u * i + 1u] = h1;
    }
    if (out_ids != nullptr) reinterpret_cast<uint4*>(out_ids)[i] = make_uint4(kind, steps, leaf, mat);
    if (out_rgb != nullptr) { out_rgb[3u * i] = cr; out_rgb[3u * i + 1u] = cg; out_rgb[3u * i + 2u] = cb; }
}

// ---- camera rays: the ray the draw marches for AA sample `sample` of each pixel of a w x h block (row-major) ------------
__global__ __launch_bounds__(256) void rm_camera_rays_kernel(rm_uniforms u, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0,
                                                             uint32_t w, uint64_t count, uint32_t sample, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t px = x0 + (uint32_t)(i % w), py = y0 + (uint32_t)(i / w);
    const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);  // wgsl:39-40
    float ox = 0.0f, oy = 0.0f;                                 // RM_SAMPLE_CENTER: the pixel centre
    if (sample < 16u) sample_offset(u, sample >> 2, sample & 3u, ox, oy);  // wgsl:44-53: (i, j) = (sample / 4, sample % 4)
    float dx, dy, dz;
    gen_ray_at(u.inv_proj, u.inv_view, ro, screen_x(px, W), screen_y(py, H), ox, oy, dx, dy, dz);
    out[6u * i] = ro.x; out[6u * i + 1u] = ro.y; out[6u * i + 2u] = ro.z;
    out[6u * i + 3u] = dx; out[6u * i + 4u] = dy; out[6u * i + 5u] = dz;
}

// ---- rm_selftest_anchor: the anchored threshold of a first own step (rm_kernel_v5.h "Pruning") on pairs (a, q) ----------------
// The march's own two functions around two evaluations of the program: out[4 i + ..] = aT, anchor_thr_base(+inf, ...) plus the
// step's position term, F(a), F(q).  prune_scale: the march kernel's (scene_scale + |ro|_1).
template <int LOOP>
__global__ __launch_bounds__(256) void rm_selftest_anchor_kernel(QueryLaunch Q, float prune_scale, uint32_t n, const float* __restrict__ pairs,
                                                                 float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float* spill = query_spill(Q.slots);
    const float ax = pairs[6u * i], ay = pairs[6u * i + 1u], az = pairs[6u * i + 2u];
    const float qx = pairs[6u * i + 3u], qy = pairs[6u * i + 4u], qz = pairs[6u * i + 5u];
    const float fa = query_distance<LOOP>(Q, spill, ax, ay, az);
    const float fq = query_distance<LOOP>(Q, spill, qx, qy, qz);
    const float aT = anchor_reach(ax, ay, az, fa, prune_scale);
    const float thr_base = anchor_thr_base(__uint_as_float(0x7F800000u), qx, qy, qz, ax, ay, az, aT);
    const float thr = thr_base + kPruneAbs * (prune_scale + ((__builtin_fabsf(qx) + __builtin_fabsf(qy)) + __builtin_fabsf(qz)));
    out[4u * i] = aT; out[4u * i + 1u] = thr; out[4u * i + 2u] = fa; out[4u * i + 3u] = fq;
}

}  // namespace rmk
