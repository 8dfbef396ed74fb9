// rm_topo_union.h -- the lock-free union-find of the topology merge pass (rm_topology.h): topo_find,
// topo_unite and topo_for_preceding, and the two memory primitives they are written in.  Included by rm_topology.h for the
// kernels, and by tests/cpp/topo_union_model.cpp for a host model that runs the same three functions on CPU threads: the
// primitives below are the only lines that differ between the two.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
namespace rmk {
// A relaxed agent-scope load: a plain load may be served by a stale line of another XCD's L2.
RM_DEV uint32_t topo_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// *p = min(*p, v) in one step; the value before.
RM_DEV uint32_t topo_fetch_min(uint32_t* p, uint32_t v) { return atomicMin(p, v); }
}  // namespace rmk
#else
// The host: no HIP.  RM_TOPO_HOST_HOOK() runs before every primitive (a model yields there to widen the interleavings); a model
// that defines RM_TOPO_HOST_FETCH_MIN supplies rmk::topo_fetch_min itself, before this header.  SparseGrid: the three fields
// topo_for_preceding reads.
#define RM_DEV inline
#ifndef RM_TOPO_HOST_HOOK
#define RM_TOPO_HOST_HOOK() ((void)0)
#endif
namespace rmk {
struct SparseGrid {
    uint32_t nx, ny, nz;
};
inline uint32_t topo_load(const uint32_t* p) {
    RM_TOPO_HOST_HOOK();
    return __atomic_load_n(p, __ATOMIC_RELAXED);
}
#ifndef RM_TOPO_HOST_FETCH_MIN
inline uint32_t topo_fetch_min(uint32_t* p, uint32_t v) {
    RM_TOPO_HOST_HOOK();
    uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return cur;
}
#endif
}  // namespace rmk
#endif

namespace rmk {

// parent[x] < x or parent[x] == x (a root), always: an index falls at every step, so `bound` (the number of lattice points) is
// never reached.  Relaxed agent-scope loads: a stale parent is an older, still valid ancestor.
// HALVE (the merge pass): every visited point is hung below its grandparent on the way -- by atomicMin, so a parent only ever falls
// and stays a member of the component -- which keeps the chains of roots that unions across many bricks build short.
template <bool HALVE>
RM_DEV uint32_t topo_find(uint32_t* parent, uint32_t x, uint32_t bound) {
    for (uint32_t n = 0; n < bound; n++) {
        const uint32_t up = topo_load(parent + x);
        if (up == x) break;
        if (HALVE) {
            const uint32_t over = topo_load(parent + up);
            if (over == up) return up;
            topo_fetch_min(parent + x, over);
            x = over;
        } else {
            x = up;
        }
    }
    return x;
}
// Unites the components of a and b.  The larger root receives the smaller one by atomicMin.  When it was no root any more
// (`old` != a), its parent is now min(old, b): the link that lost is made good by uniting `old` with b.  Each retry continues
// with strictly smaller indices.
RM_DEV void topo_unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t bound) {
    for (uint32_t n = 0; n < bound; n++) {
        a = topo_find<true>(parent, a, bound);
        b = topo_find<true>(parent, b, bound);
        if (a == b) return;
        if (a < b) { const uint32_t s = a; a = b; b = s; }
        const uint32_t old = topo_fetch_min(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// The neighbours (dx, dy, dz) that PRECEDE a point in linear order: 13 of the 26, 3 of the 6.  f(qi, qj, qk, faces) for those
// inside the lattice.
template <class F>
RM_DEV void topo_for_preceding(const SparseGrid& g, uint32_t i, uint32_t j, uint32_t k, bool faces_only, F f) {
#pragma unroll
    for (int dz = -1; dz <= 0; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if (!(dz < 0 || dy < 0 || (dy == 0 && dx < 0))) continue;
                const int faces = (dx != 0) + (dy != 0) + (dz != 0);
                if (faces_only && faces != 1) continue;
                const uint32_t qi = i + (uint32_t)dx, qj = j + (uint32_t)dy, qk = k + (uint32_t)dz;  // (wraps past 0: >= n)
                if (qi >= g.nx || qj >= g.ny || qk >= g.nz) continue;
                f(qi, qj, qk);
            }
}

}  // namespace rmk
