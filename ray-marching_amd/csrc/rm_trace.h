// rm_trace.h -- ray traversal (rm_trace_rays): every crossing of the level set along a ray, in order.
// Device code only (gfx950, wave64); included by rm_abi.hip alone, like rm_query.h, on whose distance loops, taps, walk and LDS
// columns it stands.  No draw kernel changes.
//
// Two phases.  rm_trace_march_kernel walks each ray through [T_MIN, T_MAX] with one query_distance per step and writes what it
// finds as it finds it: an event costs its lane a division and three stores, nothing the rest of the wave waits for.  The
// attributes of the events (normal: four more evaluations; ids: the walk) are a separate pass with one lane per STORED event:
// the march leaves each ray's stored count and each workgroup's sum, rm_mesh_scan_kernel turns the sums into offsets,
// rm_trace_list_kernel writes the compact (ray, slot) list and rm_trace_attr_kernel strides over it.  Every order is fixed by
// the ray order: no atomics, identical runs.
#pragma once
#include "rm_query.h"
#include "rm_mesh.h"

namespace rmk {

struct TraceLaunch {
    float t_min, t_max, min_step, scale, level;  // enum rm_trace
    uint32_t max_steps;
    uint32_t K;  // event slots per ray
};

// One lane per ray.  events / event_ids / counts / spans: the outputs (nullptr: not wanted; `events` is the scratch copy when
// only the ids are wanted with attributes, whose pass reads the positions there).  stored / sums: per ray min(events, K) and
// per workgroup their sum, for the attribute pass (both nullptr without one).
template <int LOOP>
__global__ __launch_bounds__(256) void rm_trace_march_kernel(QueryLaunch Q, TraceLaunch T, uint32_t n, const float* __restrict__ rays,
                                                             float* __restrict__ events, uint32_t* __restrict__ event_ids,
                                                             uint32_t* __restrict__ counts, float* __restrict__ spans,
                                                             uint32_t* __restrict__ stored, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long wsum[4];
    static_assert(sizeof wsum <= rml::kQueryOwnTrace, "the static LDS the host counts in front of the query columns");
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t kept = 0;
    if (i < n) {  // (the barrier below needs every lane of the workgroup; the record loops only the lanes that march)
        float* spill = query_spill(Q.slots);
        const float ox = rays[6u * i], oy = rays[6u * i + 1u], oz = rays[6u * i + 2u];
        const float dx = rays[6u * i + 3u], dy = rays[6u * i + 4u], dz = rays[6u * i + 5u];
        float4* ev = events != nullptr ? reinterpret_cast<float4*>(events) + 2u * (size_t)T.K * i : nullptr;
        uint4* id = event_ids != nullptr ? reinterpret_cast<uint4*>(event_ids) + (size_t)T.K * i : nullptr;
        float t = T.t_min;
        float da = query_distance<LOOP>(Q, spill, ox + dx * t, oy + dy * t, oz + dz * t);
        bool in = da < T.level;
        const bool start_inside = in;
        const float d_start = da;
        uint32_t steps = 1u, found = 0u;
        float length = 0.0f, t_enter = t;
        while (t < T.t_max && steps < T.max_steps) {
            const float h = fmax_(__builtin_fabsf(da - T.level) * T.scale, T.min_step);
            const float tn = fmin_(t + h, T.t_max);
            const float db = query_distance<LOOP>(Q, spill, ox + dx * tn, oy + dy * tn, oz + dz * tn);
            ++steps;
            const bool inb = db < T.level;
            if (inb != in) {
                const float w = tn - t;
                const float tc = fmin_(t + w * ((da - T.level) / (da - db)), tn);  // rm_extract_mesh's vertex rule on [t, tn]
                if (found < T.K) {
                    if (ev != nullptr) {
                        ev[2u * found] = make_float4(tc, ox + dx * tc, oy + dy * tc, oz + dz * tc);
                        ev[2u * found + 1u] = make_float4(0.0f, 0.0f, 0.0f, w);
                    }
                    if (id != nullptr) id[found] = make_uint4(inb ? RM_TRACE_ENTER : RM_TRACE_EXIT, steps, RM_NO_ID, RM_NO_ID);
                }
                ++found;
                if (inb) t_enter = tc;
                else length = length + (tc - t_enter);
            }
            t = tn; da = db; in = inb;
        }
        if (in) length = length + (t - t_enter);
        kept = found < T.K ? found : T.K;
        for (uint32_t k = kept; k < T.K; k++) {  // the unfilled slots
            if (ev != nullptr) {
                ev[2u * k] = make_float4(__uint_as_float(0x7F800000u), 0.0f, 0.0f, 0.0f);
                ev[2u * k + 1u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            if (id != nullptr) id[k] = make_uint4(0u, 0u, RM_NO_ID, RM_NO_ID);
        }
        if (counts != nullptr) {
            const uint32_t flags = (start_inside ? (uint32_t)RM_TRACE_START_INSIDE : 0u) | (in ? (uint32_t)RM_TRACE_END_INSIDE : 0u) |
                                   (t < T.t_max ? (uint32_t)RM_TRACE_OUT_OF_STEPS : 0u);
            reinterpret_cast<uint4*>(counts)[i] = make_uint4(found, steps, flags, kept);
        }
        if (spans != nullptr) reinterpret_cast<float4*>(spans)[i] = make_float4(t, length, d_start, da);
        if (stored != nullptr) stored[i] = kept;
    }
    if (sums != nullptr) {  // (the same for every lane of the launch)
        unsigned long long total;
        (void)block_exclusive_sum<4>((unsigned long long)kept, wsum, total);
        if (threadIdx.x == 0) sums[blockIdx.x] = total;
    }
}

// The stored events of each ray, in ray order, as (ray, slot) pairs from the ray's offset on: its workgroup's offset (the
// scanned sums) plus the stored counts of the rays before it in the workgroup.
__global__ __launch_bounds__(256) void rm_trace_list_kernel(uint32_t n, const uint32_t* __restrict__ stored,
                                                            const unsigned long long* __restrict__ block_offsets,
                                                            uint2* __restrict__ list) {
    __shared__ uint32_t wsum[4];
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t s = i < n ? stored[i] : 0u;
    uint32_t total;
    const unsigned long long base = block_offsets[blockIdx.x] + block_exclusive_sum<4>(s, wsum, total);
    for (uint32_t k = 0; k < s; k++) list[base + k] = make_uint2((uint32_t)i, k);
}

// One lane per stored event, striding over the list (its length is known on the device only: totals[0] | totals[1] << 32):
// the normal and the (leaf, material) rm_query_points returns at the event's position, read from `positions` (the event
// records the march wrote) and written into the records of `events` / `event_ids`.
template <int LOOP, bool NORMALS, bool IDS>
__global__ __launch_bounds__(256) void rm_trace_attr_kernel(QueryLaunch Q, uint32_t K, const uint32_t* __restrict__ totals,
                                                            const uint2* __restrict__ list, const float* positions, float* events,
                                                            uint32_t* __restrict__ event_ids) {
    const unsigned long long total = (unsigned long long)totals[0] | (unsigned long long)totals[1] << 32;
    float* spill = query_spill(Q.slots);
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256u) {
        const uint2 rs = list[e];
        const size_t slot = (size_t)rs.x * K + rs.y;
        const float4 p = reinterpret_cast<const float4*>(positions)[2u * slot];  // (t, x, y, z)
        if constexpr (NORMALS) {
            float nx, ny, nz;
            query_taps<LOOP>(Q, spill, p.y, p.z, p.w, nx, ny, nz);
            query_normalize(nx, ny, nz);
            events[8u * slot + 4u] = nx; events[8u * slot + 5u] = ny; events[8u * slot + 6u] = nz;
        }
        if constexpr (IDS) {
            uint2 ids;
            if (Q.n_qrec == 0u) {  // (an empty program has no crossing; as rm_query_points has it)
                ids.x = RM_NO_ID; ids.y = 0u;
            } else {
                const uint32_t m = query_walk(Q, spill, p.y, p.z, p.w);
                ids.x = m >> 8; ids.y = m & 0xFFu;
            }
            reinterpret_cast<uint2*>(event_ids)[2u * slot + 1u] = ids;
        }
    }
}

}  // namespace rmk
