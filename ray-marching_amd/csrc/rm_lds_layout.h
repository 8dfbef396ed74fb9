// rm_lds_layout.h -- where the arrays of a workgroup's DYNAMIC LDS lie: the one description the host sizes a launch from
// (`bytes`) and the kernels take their pointers from (the byte offsets, in declaration order).  Plain integer arithmetic, no HIP
// types: host and device code of rm_abi.hip, the translation units hipRTC compiles (rm_jit.h) and g++ all read it;
// tests/cpp/lds_layout_check.cpp checks every offset against the expressions written out by hand.  (Device allocations in
// GLOBAL memory: rm_abi_layout.h.)
#pragma once
#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#endif

// (rm_device.h's RM_HD is device-only under hipcc; these run on both sides of one translation unit)
#if defined(__HIPCC__)
#define RM_LDS_FN __host__ __device__ constexpr
#else
#define RM_LDS_FN constexpr
#endif

namespace rml {

// ---- Miss-test tables (rm_kernel_v5.h CullTables), as the pre-pass and the culling self-tests stage them -----------------
// {veto, 3 x pad}, cone[n_cone] float4, slab[3 n_slab] float4, and for the kernels that test whole pixels and tiles
// aux[n_cone + n_slab] float2.
constexpr uint32_t kConeBytes = 16u, kSlabBytes = 48u, kAuxBytes = 8u;
struct CullLds {
    uint32_t veto, cone, slab, aux, bytes;
    RM_LDS_FN CullLds(uint32_t n_cone, uint32_t n_slab, bool with_aux)
        : veto(0u), cone(veto + 16u), slab(cone + n_cone * kConeBytes), aux(slab + n_slab * kSlabBytes),
          bytes(aux + (with_aux ? (n_cone + n_slab) * kAuxBytes : 0u)) {}
};

// ---- March workgroup (rm_kernel_v5.h rm_render_v5_body) ---------------------------------------------------------------------
constexpr uint32_t V5_POOL = 1024u;  // rays of a tile: 64 pixels x 16 samples
constexpr uint32_t V5_RQ = 64u;      // ready buffer entries per wave (refilled only when empty)
constexpr uint32_t V5_SQ = 64u;      // miss buffer entries per wave
constexpr uint32_t V5_HQ = 128u;     // hit buffer entries per wave (64 are taken whenever 64 are waiting)
// per wave: the three buffers, the screen coordinates of the tile's 8 columns and 8 rows, and LAST the partial normals of a tap phase
// that takes its four taps one at a time or is followed by a material phase -- a generated kernel with the four-tap function and no
// materials leaves those 768 bytes away (RmLaunch::wave_dwords): 25.6 -> 22.5 KB per workgroup for the metric scene, 7 instead of 6
// workgroups per CU
constexpr uint32_t V5_TN_DWORDS = 3u * 64u;
constexpr uint32_t V5_WAVE_DWORDS = 4u * (V5_RQ + V5_SQ + V5_HQ) + 16u + V5_TN_DWORDS;
// byte offsets inside one wave's buffers (structure of arrays: ids, then three rows of coordinates)
struct MarchWaveLds {
    static constexpr uint32_t rq_rid = 0u;                  // ready rays: id ...
    static constexpr uint32_t rq_d = rq_rid + 4u * V5_RQ;   // ... direction [3][V5_RQ]
    static constexpr uint32_t sq_rid = rq_d + 12u * V5_RQ;  // rays that ended without a hit: id ...
    static constexpr uint32_t sq_v = sq_rid + 4u * V5_SQ;   // ... direction [3][V5_SQ]
    static constexpr uint32_t hq_rid = sq_v + 12u * V5_SQ;  // hits waiting for their normal: id ...
    static constexpr uint32_t hq_v = hq_rid + 4u * V5_HQ;   // ... position [3][V5_HQ]
    static constexpr uint32_t wxy = hq_v + 12u * V5_HQ;     // [16] pt_screen.x of the tile's 8 columns, .y of its 8 rows
    static constexpr uint32_t tn = wxy + 64u;               // [3][64] partial normals (absent when wave_dwords says so)
    static constexpr uint32_t bytes = tn + 4u * V5_TN_DWORDS;
};
static_assert(MarchWaveLds::bytes == 4u * V5_WAVE_DWORDS, "a wave's buffers");

// pool, per-wave buffers [wpt], spill columns [wpt][spill_depth][64], the miss-test tables, the staged program (records, unit
// table, tree table: prog_in_lds kernels only), {pool cursor, tile slot, veto, flag}, the 16 AA sample offsets, one
// material byte per ray of a tagged program, then `pad`: the current tile's primitive mask (one word) and 12 B unused.  Every
// region starts on a multiple of 16 bytes.
// (The march kernel takes the compile-time parts from here -- MarchWaveLds, the two sizes below -- and writes the sums that
// depend on the launch out on RmLaunch's fields, see the comment there; lds_layout_check.cpp compares the two.)
constexpr uint32_t kMarchCtlBytes = 16u, kMarchOffBytes = 16u * 2u * 4u;
struct MarchLds {
    uint32_t pool, waves, wave_bytes, spill, cone, slab, prog, units, tree, ctl, off, rmat, pad, bytes;
    RM_LDS_FN MarchLds(uint32_t wpt, uint32_t wave_dwords, uint32_t spill_depth, uint32_t n_cone, uint32_t n_slab, bool prog_in_lds,
                       uint32_t n_rec, uint32_t n_grp, uint32_t n_tree, bool tagged)
        : pool(0u), waves(pool + V5_POOL * 4u), wave_bytes(wave_dwords * 4u), spill(waves + wpt * wave_bytes),
          cone(spill + wpt * spill_depth * 256u), slab(cone + n_cone * kConeBytes), prog(slab + n_slab * kSlabBytes),
          units(prog + (prog_in_lds ? n_rec * 32u : 0u)), tree(units + (prog_in_lds ? n_grp * 32u : 0u)),
          ctl(tree + (prog_in_lds ? n_tree * 32u : 0u)), off(ctl + kMarchCtlBytes), rmat(off + kMarchOffBytes), pad(rmat + (tagged ? V5_POOL : 0u)),
          bytes(pad + 16u) {}
};

// ---- What a march launch may take ------------------------------------------------------------------------------------------
// A workgroup cannot be launched with more dynamic LDS than kLdsLaunchLimit.  The two budgets below it are choices, not limits:
// a CU has 160 KB of LDS, so workgroups of up to 48 KB still come three to a CU -- the launch halves its waves per tile until
// a workgroup is that small (or has one wave left) --, and a program is staged in LDS only when a ONE-wave workgroup with it
// stays 4 KB under the launch limit; a longer one is read through the scalar cache, which every size of program can be.
constexpr uint32_t kLdsLaunchLimit = 64u * 1024u, kLdsProgramBudget = 60u * 1024u, kLdsTileBudget = 48u * 1024u;

// What launch_v5 decides before it knows the kernel: program in LDS or through the scalar cache, waves per tile.  It sizes
// the workgroup for the most any kernel that may follow takes -- every wave buffer, the tables whenever the program is short
// enough to have them (256 records), the tree table whenever the decoder made one (n_tree_table, with the spill slot its loop
// adds), the material stack of a tagged program (mat_depth; 0 untagged) -- so `bytes` is never below the launch's own.
struct MarchChoice {
    bool prog_in_lds;
    uint32_t wpt, bytes;
};
RM_LDS_FN MarchLds march_worst_case(uint32_t wpt, bool prog_in_lds, uint32_t spill_depth, uint32_t mat_depth, bool tagged,
                                    uint32_t n_cone, uint32_t n_slab, uint32_t n_rec, uint32_t n_grp, uint32_t n_tree_table) {
    const uint32_t depth = spill_depth + (n_tree_table != 0u ? 1u : 0u);
    const bool tables = n_rec <= 256u;
    return MarchLds(wpt, V5_WAVE_DWORDS, depth > mat_depth ? depth : mat_depth, tables ? n_cone : 0u, tables ? n_slab : 0u,
                    prog_in_lds, n_rec, n_grp, n_tree_table, tagged);
}
RM_LDS_FN MarchChoice choose_march(bool want_lds, uint32_t wpt, uint32_t spill_depth, uint32_t mat_depth, bool tagged,
                                   uint32_t n_cone, uint32_t n_slab, uint32_t n_rec, uint32_t n_grp, uint32_t n_tree_table) {
    const bool lds = want_lds && march_worst_case(1u, true, spill_depth, mat_depth, tagged, n_cone, n_slab, n_rec, n_grp, n_tree_table).bytes <= kLdsProgramBudget;
    uint32_t bytes = 0u;
    for (;; wpt /= 2u) {
        bytes = march_worst_case(wpt, lds, spill_depth, mat_depth, tagged, n_cone, n_slab, n_rec, n_grp, n_tree_table).bytes;
        if (wpt <= 1u || bytes <= kLdsTileBudget) break;
    }
    return MarchChoice{lds, wpt, bytes};
}

// ---- Kernel v1 (rm_kernels.h rm_render_pixel): the program, then the value stack [spill_depth][256 threads] ----------------
struct PixelLds {
    uint32_t prog, spill, bytes;
    RM_LDS_FN PixelLds(uint32_t n_rec, uint32_t spill_depth) : prog(0u), spill(prog + n_rec * 32u), bytes(spill + spill_depth * 256u * 4u) {}
};

// ---- Query kernels (rm_query.h query_spill and every kernel that calls it) ---------------------------------------------------
// The whole dynamic LDS of a 256-thread workgroup: one column per wave of `slots` dwords per lane, slot k of lane l of wave w
// at dword (w * slots + k) * kQueryLanes + l.  It lies behind `own` bytes of the kernel's static __shared__ arrays, which count
// against what a workgroup may take: nothing for the point, ray and lattice kernels, kQueryOwnTrace for the traversal march,
// kQueryOwnBrick for the kernels that work a brick per workgroup -- each of those holds a static_assert next to its arrays.
constexpr uint32_t kQueryWaves = 4u, kQueryLanes = 64u;
constexpr uint32_t kQueryOwnTrace = 64u, kQueryOwnBrick = 4096u;
struct QueryLds {
    uint32_t slots, own, stride, dynamic, bytes;  // stride: bytes of one wave's column; dynamic: what the launch asks for
    RM_LDS_FN QueryLds(uint32_t slots_, uint32_t own_)
        : slots(slots_), own(own_), stride(slots_ * kQueryLanes * 4u), dynamic(kQueryWaves * stride), bytes(own + dynamic) {}
    RM_LDS_FN QueryLds behind(uint32_t other_own) const { return QueryLds(slots, other_own); }
    // `cap`: what the device gives one workgroup; a kernel has to ask for more than kLdsLaunchLimit before its launch
    RM_LDS_FN bool fits(uint64_t cap) const { return bytes <= cap; }
    RM_LDS_FN bool needs_opt_in() const { return bytes > kLdsLaunchLimit; }
};

// ---- Distance transform, column passes (rm_distance.h rm_dist_column_kernel) ------------------------------------------------
// A tile of `xt` adjacent columns of n points each, one word per point, point q of column lx at word q * xt + lx (the lanes of
// a wave read and write consecutive words).  xt: the power of two that keeps the tile within 32 KB, but at least 16 columns
// (64 contiguous bytes per row of the tile) and at most 64 (one row per wave): 64 KB, the launch limit, at the longest axis
// of 1024 points.
constexpr uint32_t kDistTileWords = 8192u, kDistMinColumns = 16u, kDistMaxColumns = 64u, kDistMaxAxis = 1024u;
RM_LDS_FN uint32_t dist_columns_log2(uint32_t n) {
    uint32_t l = 6u;  // kDistMaxColumns
    while (l > 4u && (n << l) > kDistTileWords) l--;
    return l;
}
struct DistColumnLds {
    uint32_t col, bytes;
    RM_LDS_FN DistColumnLds(uint32_t xt, uint32_t n) : col(0u), bytes(col + xt * n * 4u) {}
};

// ---- Overhang test (rm_support.h rm_sup_overhang_kernel) --------------------------------------------------------------------
// The bit rows of the layer below that a tile of `tv` rows of one layer can see: tv + 2 reach rows (reach = floor(sqrt(r2)) <= 15
// rows of halo on either side) of nw u64 words each (nw = ceil(points along the bit axis / 64) <= 16), row r at word r * nw.
// tv: as many rows as give every one of the workgroup's 256 threads at most one word, 64 at the most: 5888 bytes for the widest rows.
constexpr uint32_t kSupMaxReach = 15u, kSupMaxRows = 64u, kSupMaxWords = 16u, kSupMaxR2 = 255u;
RM_LDS_FN uint32_t sup_tile_rows(uint32_t nw) { return 256u / nw < kSupMaxRows ? 256u / nw : kSupMaxRows; }
struct SupCoverLds {
    uint32_t rows, bytes;
    RM_LDS_FN SupCoverLds(uint32_t tv, uint32_t reach, uint32_t nw) : rows(0u), bytes(rows + (tv + 2u * reach) * nw * 8u) {}
};

// ---- Layer regions, local labelling (rm_islands.h rm_isl_local_kernel) -------------------------------------------------------
// One tile is kIslTile rows x 64 bits (one word column) of one layer: the rows' words (8 B each), then one parent per bit, the
// bit b of row r at word r * 64 + b (only the entries of run starts are used).
constexpr uint32_t kIslTile = 64u;
struct IslTileLds {
    uint32_t words, parent, bytes;
    RM_LDS_FN IslTileLds() : words(0u), parent(words + kIslTile * 8u), bytes(parent + kIslTile * 64u * 4u) {}
};

// ---- Layer regions, links (rm_islands.h rm_isl_links_kernel) ------------------------------------------------------------------
// The labels of the layer below that a tile of kIslLinkRows rows x 64 points can see: kIslLinkRows + 2 reach rows of 64 + 2 reach
// u32 words, the point (v0 - reach + r, u0 - reach + c) at word r * pitch + c (reach = floor(sqrt(r2)) <= kSupMaxReach).
constexpr uint32_t kIslLinkRows = 16u;
struct IslLinkLds {
    uint32_t labels, pitch, rows, bytes;
    RM_LDS_FN explicit IslLinkLds(uint32_t reach)
        : labels(0u), pitch(64u + 2u * reach), rows(kIslLinkRows + 2u * reach), bytes(labels + rows * pitch * 4u) {}
};

// ---- Surface measures, pair counts (rm_surface.h rm_surf_count_kernel) --------------------------------------------------------
// One tile is kSurfTileX x kSurfTileY x kSurfTileZ points of the PADDED lattice (coordinates -1 .. n per axis), one class byte per
// point, with the halo its 13 forward pairs reach: one point more on +x, one on either side of y and of z.  The point
// (x0 + cx, y0 - 1 + cy, z0 - 1 + cz) of the tile at (x0, y0, z0) lies at byte (cz * rows_y + cy) * pitch + cx.  Then the
// workgroup's table of counts: kSurfCounts u32 words (8 point bins, 8 x 8 x 13 pair bins).
constexpr uint32_t kSurfTileX = 64u, kSurfTileY = 16u, kSurfTileZ = 8u, kSurfCounts = 8u + 8u * 8u * 13u;
constexpr uint32_t kSurfMaxGroups = 1024u;  // workgroups of a launch: each walks the tiles g, g + groups, ... and writes one row
RM_LDS_FN uint32_t surf_tiles(uint32_t n, uint32_t extent) { return (n + 2u + extent - 1u) / extent; }
struct SurfTileLds {
    uint32_t pitch, rows_y, rows_z, cls, counts, bytes;
    RM_LDS_FN SurfTileLds()
        : pitch(kSurfTileX + 1u), rows_y(kSurfTileY + 2u), rows_z(kSurfTileZ + 2u), cls(0u),
          counts((cls + pitch * rows_y * rows_z + 15u) & ~15u), bytes(counts + kSurfCounts * 4u) {}
};

// ---- Mesh voxelisation, fill (rm_voxel.h rm_vox_fill_kernel) ------------------------------------------------------------------
// A workgroup makes kVoxFillCells consecutive bytes of the occupancy.  A row of nx points has nx + 1 bits in vox_row_words(nx) u32
// words; the cells lie in at most vox_fill_rows(nx) rows (a partial one at either end), whose words are staged as they are
// (`raw`) and with their prefix parities (`prefix`): kVoxFillMaxWords words each, the most any nx of 2..1024 needs (nx = 2).
constexpr uint32_t kVoxFillCells = 4096u, kVoxFillMaxWords = 2049u;
RM_LDS_FN uint32_t vox_row_words(uint32_t nx) { return (nx >> 5) + 1u; }
RM_LDS_FN uint32_t vox_fill_rows(uint32_t nx) { return (kVoxFillCells - 1u) / nx + 2u; }
struct VoxFillLds {
    uint32_t raw, prefix, bytes;
    RM_LDS_FN VoxFillLds() : raw(0u), prefix((raw + kVoxFillMaxWords * 4u + 15u) & ~15u), bytes(prefix + kVoxFillMaxWords * 4u) {}
};

// ---- Device sort (rm_sort.h rm_sort_count_kernel, rm_sort_scatter_kernel) -----------------------------------------------------
// STATIC LDS of a workgroup of kSortWaves waves working one tile of kSortRounds * 64 pairs.  ROUND r = it * kSortWaves + wave holds
// the 64 pairs the wave loads in its pass `it` over the tile, and the rounds in this order are the tile in input order.  One row
// of kSortLdsDigits words per round, digit d of round r at word r * kSortLdsDigits + d: first the round's count of the digit,
// then (the scatter) the output position of the round's first pair with it.  Every word has one writer between two barriers.
// (The tile itself is rml::kSortTile in rm_abi_layout.h, which sizes the global tables from it.)
constexpr uint32_t kSortWaves = 4u, kSortRounds = 16u, kSortLdsDigits = 256u;
struct SortLds {
    uint32_t rows, bytes;
    RM_LDS_FN SortLds() : rows(0u), bytes(rows + kSortRounds * kSortLdsDigits * 4u) {}
};

}  // namespace rml
