// rm_abi_layout.h -- where the typed arrays of rm_abi.hip's device allocations lie.  Pure host arithmetic (no HIP), so that
// tests/cpp/abi_layout_check.cpp can check every layout on the CPU.  A layout is declared first (sizes only), gives the bytes to
// reserve, and its regions are resolved against the buffer's base pointer afterwards; the entry points that read a result
// (rm_read_mesh, rm_read_slices) use the declarations of the ones that wrote it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rml {

constexpr size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// `bytes` bytes at `offset` of an allocation, holding an array of T.
template <class T>
struct Region {
    size_t offset = 0, bytes = 0;
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }
    const T* at(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + offset); }
};

// Hands out the regions of one allocation in declaration order.  Every region starts on a 16-byte boundary (device arrays
// are read and written with vector accesses of up to 16 bytes), so the total is a multiple of 16 as well.
struct Carver {
    size_t total = 0;
    template <class T>
    Region<T> take(size_t count) {
        const Region<T> r{total, count * sizeof(T)};
        total += align16(r.bytes);
        return r;
    }
};

// The layouts below declare their regions as members, in the order in which they lie: each constructor takes them from the
// Carver declared first (members are initialised in declaration order), `bytes` is the total to reserve.

// rm_extract_mesh's scratch for a lattice of n points in nb blocks: distances, vertex bases (4 B per point each), flags (1 B),
// block sums (8 B per block), the two totals.
struct DenseMeshScratch {
    Carver a;
    Region<float> dist;
    Region<uint32_t> vbase;
    Region<uint8_t> flags;
    Region<unsigned long long> sums;
    Region<uint32_t> totals;
    size_t bytes;
    DenseMeshScratch(uint32_t n, uint32_t nb)
        : dist(a.take<float>(n)), vbase(a.take<uint32_t>(n)), flags(a.take<uint8_t>(n)), sums(a.take<unsigned long long>(nb)),
          totals(a.take<uint32_t>(4)), bytes(a.total) {}
};

// rm_extract_mesh_sparse, per brick: 4 B (keep flag, then the kept bricks before it); per 256 bricks a block sum; totals and
// the evaluation count.
struct SparseBrickTables {
    Carver a;
    Region<uint32_t> boff;
    Region<unsigned long long> psums, ptot, evals;
    size_t bytes;
    SparseBrickTables(uint32_t n_entries, uint32_t n_pblocks)
        : boff(a.take<uint32_t>(n_entries)), psums(a.take<unsigned long long>(n_pblocks)), ptot(a.take<unsigned long long>(2)),
          evals(a.take<unsigned long long>(2)), bytes(a.total) {}
};

// ... and per kept brick: its index, its segment map, its tile of distances, its segment words and their first (vertex,
// triangle).  SegMap and Pair are the kernels' types (rmk::SparseSegMap, uint2).
template <class SegMap, class Pair>
struct SparseKeptScratch {
    Carver a;
    Region<uint32_t> klist;
    Region<SegMap> maps;
    Region<float> tiles;
    Region<uint32_t> words;
    Region<Pair> first;
    Region<unsigned long long> ssums, stot;
    size_t bytes;
    SparseKeptScratch(uint64_t K, uint32_t tile_points, uint32_t n_segs, uint32_t n_sblocks)
        : klist(a.take<uint32_t>(K)), maps(a.take<SegMap>(K)), tiles(a.take<float>(K * tile_points)), words(a.take<uint32_t>(n_segs)),
          first(a.take<Pair>(n_segs)), ssums(a.take<unsigned long long>(n_sblocks)), stot(a.take<unsigned long long>(2)),
          bytes(a.total) {}
};

// rm_mass_moments, per brick: 4 B as above; per 256 bricks a block sum and one row of 16 moments (128 B); totals, the
// evaluation count and the result row.
struct MassBrickTables {
    Carver a;
    Region<uint32_t> boff;
    Region<unsigned long long> psums, ptot, evals, prows, result;
    size_t bytes;
    MassBrickTables(uint32_t n_entries, uint32_t n_pblocks)
        : boff(a.take<uint32_t>(n_entries)), psums(a.take<unsigned long long>(n_pblocks)), ptot(a.take<unsigned long long>(2)),
          evals(a.take<unsigned long long>(2)), prows(a.take<unsigned long long>((size_t)n_pblocks * 16u)),
          result(a.take<unsigned long long>(16)), bytes(a.total) {}
};

// ... and per kept brick: its index and its row of 16 moments.
struct MassKeptScratch {
    Carver a;
    Region<uint32_t> klist;
    Region<unsigned long long> krows;
    size_t bytes;
    explicit MassKeptScratch(uint64_t K) : klist(a.take<uint32_t>(K)), krows(a.take<unsigned long long>(K * 16u)), bytes(a.total) {}
};

// rm_label_solid / rm_label_occupancy, for a lattice of n points in nb bricks: per point its parent (4 B), its occupancy and its
// root's exterior mark (1 B each); per brick its class (1 B) and one row of 16 words (128 B: the verify and the count pass, one
// after the other); per 256 bricks those rows folded into one and the probe's block sum, per 2048 points the numbering's;
// totals, the evaluation count and the reduced row.
struct TopoScratch {
    Carver a;
    Region<uint32_t> parent;
    Region<uint8_t> occ, ext, cls;
    Region<unsigned long long> rows, folded, psums, rsums, ptot, rtot, evals, result;
    size_t bytes;
    TopoScratch(uint32_t n, uint32_t nb, uint32_t n_pblocks, uint32_t n_rblocks)
        : parent(a.take<uint32_t>(n)), occ(a.take<uint8_t>(n)), ext(a.take<uint8_t>(n)), cls(a.take<uint8_t>(nb)),
          rows(a.take<unsigned long long>((size_t)nb * 16u)), folded(a.take<unsigned long long>((size_t)n_pblocks * 16u)),
          psums(a.take<unsigned long long>(n_pblocks)), rsums(a.take<unsigned long long>(n_rblocks)),
          ptot(a.take<unsigned long long>(2)), rtot(a.take<unsigned long long>(2)), evals(a.take<unsigned long long>(2)),
          result(a.take<unsigned long long>(16)), bytes(a.total) {}
};

// ... and the result: the label volume (4 B per point) in a buffer of its own, and the bodies' rows, then the cavities' (16
// words each), in another, allocated once B and C are known.
struct TopoRows {
    Carver a;
    Region<unsigned long long> bodies, cavities;
    size_t bytes;
    TopoRows(uint64_t B, uint64_t C) : bodies(a.take<unsigned long long>(B * 16u)), cavities(a.take<unsigned long long>(C * 16u)), bytes(a.total) {}
};

// rm_voxelize_mesh, for n_triangles triangles in n_blocks blocks of 256, a bit volume of n_words u32 words (rows x words of a row
// of nx + 1 bits) filled by n_groups workgroups: per triangle its record (kVoxTriWords u32: the snapped vertices and its box of
// rows) and the work items before it in its block; per block the items' sum (scanned in place) and the total; the counters
// (TRIANGLES, REJECTED, EDGE_ON, CROSSINGS) directly before the bit volume, so that one memset clears both; per fill workgroup one
// row of 16 words (INSIDE, OPEN_ROWS), per 256 of them one folded row, the reduced row; and the copies of a caller's host arrays
// (xyz: 3 floats per vertex, idx: 3 indices per triangle; empty for device inputs and for a soup).  The occupancy itself (1 B per
// point) is the result and lies in a buffer of its own.
constexpr uint32_t kVoxTriWords = 12u, kVoxCounters = 8u;
struct VoxScratch {
    Carver a;
    Region<uint32_t> tris, starts;
    Region<unsigned long long> bsums, btot, counters;
    Region<uint32_t> bits;
    Region<unsigned long long> rows, folded, result;
    Region<float> xyz;
    Region<uint32_t> idx;
    size_t bytes;
    VoxScratch(uint32_t n_triangles, uint32_t n_blocks, uint32_t n_words, uint32_t n_groups, uint32_t n_fblocks, uint64_t host_vertices,
               uint64_t host_triangles)
        : tris(a.take<uint32_t>((size_t)n_triangles * kVoxTriWords)), starts(a.take<uint32_t>(n_triangles)),
          bsums(a.take<unsigned long long>(n_blocks)), btot(a.take<unsigned long long>(2)),
          counters(a.take<unsigned long long>(kVoxCounters)), bits(a.take<uint32_t>(n_words)),
          rows(a.take<unsigned long long>((size_t)n_groups * 16u)), folded(a.take<unsigned long long>((size_t)n_fblocks * 16u)),
          result(a.take<unsigned long long>(16)), xyz(a.take<float>(host_vertices * 3u)), idx(a.take<uint32_t>(host_triangles * 3u)),
          bytes(a.total) {}
    // counters and bits as one span
    size_t clear_offset() const { return counters.offset; }
    size_t clear_bytes() const { return bits.offset + bits.bytes - counters.offset; }
};

// rm_set_lattice, the retained slot of a lattice of nx x ny x nz points: per point its class (1 B); per row (j, k) the bits
// `byte != 0` of its points in lat_row_words(nx) u32 words, point i in bit i & 31 of word i >> 5; per brick of 8 x 8 x 8 points
// (lat_bricks(n) along an axis, x fastest) one bit, brick b in bit b & 31 of word b >> 5; the two counters (POINTS, BRICKS)
// directly behind the brick words, so that one memset clears both.  The call has no scratch: a caller's bytes are copied into
// `classes` directly.
constexpr uint32_t lat_row_words(uint32_t nx) { return (nx + 31u) >> 5; }
constexpr uint32_t lat_bricks(uint32_t n) { return (n + 7u) >> 3; }
struct LatticeSlot {
    Carver a;
    Region<uint8_t> classes;
    Region<uint32_t> bits, bricks;
    Region<unsigned long long> counters;
    size_t bytes;
    LatticeSlot(uint32_t nx, uint32_t ny, uint32_t nz)
        : classes(a.take<uint8_t>((size_t)nx * ny * nz)), bits(a.take<uint32_t>((size_t)ny * nz * lat_row_words(nx))),
          bricks(a.take<uint32_t>(((size_t)lat_bricks(nx) * lat_bricks(ny) * lat_bricks(nz) + 31u) >> 5)),
          counters(a.take<unsigned long long>(2)), bytes(a.total) {}
    // bricks and counters as one span
    size_t clear_offset() const { return bricks.offset; }
    size_t clear_bytes() const { return counters.offset + counters.bytes - bricks.offset; }
};

// rm_distance_solid / rm_distance_occupancy, for a lattice of n points in nb bricks: per point its occupancy (1 B); per brick its
// class (1 B); per 256 bricks the probe's block sum; per 2048 points one row of 16 words (the maxima and the count), per 256 of
// those rows one folded row; totals, the evaluation count and the reduced row.  The distance volume itself (4 B per point) and
// the feature mask (1 B per point) are the result and lie in buffers of their own.
struct DistScratch {
    Carver a;
    Region<uint8_t> occ, cls;
    Region<unsigned long long> psums, rows, folded, ptot, evals, result;
    size_t bytes;
    DistScratch(uint32_t n, uint32_t nb, uint32_t n_pblocks, uint32_t n_rblocks, uint32_t n_fblocks)
        : occ(a.take<uint8_t>(n)), cls(a.take<uint8_t>(nb)), psums(a.take<unsigned long long>(n_pblocks)),
          rows(a.take<unsigned long long>((size_t)n_rblocks * 16u)), folded(a.take<unsigned long long>((size_t)n_fblocks * 16u)),
          ptot(a.take<unsigned long long>(2)), evals(a.take<unsigned long long>(2)), result(a.take<unsigned long long>(16)), bytes(a.total) {}
};

// rm_distance_features: per point the transform towards the core (4 B: one half after the other); the rows, the folded rows and
// the reduced row as above.
struct DistFeatureScratch {
    Carver a;
    Region<uint32_t> feat;
    Region<unsigned long long> rows, folded, result;
    size_t bytes;
    DistFeatureScratch(uint32_t n, uint32_t n_rblocks, uint32_t n_fblocks)
        : feat(a.take<uint32_t>(n)), rows(a.take<unsigned long long>((size_t)n_rblocks * 16u)),
          folded(a.take<unsigned long long>((size_t)n_fblocks * 16u)), result(a.take<unsigned long long>(16)), bytes(a.total) {}
};

// rm_support_solid / rm_support_occupancy, for a lattice of n points in nb bricks whose bit planes hold n_words u64 words each
// (rm_support.h: layers x rows x ceil(bit-axis points / 64)): per point its occupancy (1 B); per brick its class (1 B); per 256
// bricks the probe's block sum; totals and the evaluation count; the four planes (inside, overhang, support, support on the
// plate: half a byte per point in all when the bit axis fills its words); the automatic plate's height.  The mask (1 B per
// point) and the profile are the result and lie in buffers of their own.
struct SupportScratch {
    Carver a;
    Region<uint8_t> occ, cls;
    Region<unsigned long long> psums, ptot, evals, ins, ov, sup, plt;
    Region<uint32_t> plate;
    size_t bytes;
    SupportScratch(uint32_t n, uint32_t nb, uint32_t n_pblocks, uint32_t n_words)
        : occ(a.take<uint8_t>(n)), cls(a.take<uint8_t>(nb)), psums(a.take<unsigned long long>(n_pblocks)),
          ptot(a.take<unsigned long long>(2)), evals(a.take<unsigned long long>(2)), ins(a.take<unsigned long long>(n_words)),
          ov(a.take<unsigned long long>(n_words)), sup(a.take<unsigned long long>(n_words)), plt(a.take<unsigned long long>(n_words)),
          plate(a.take<uint32_t>(4)), bytes(a.total) {}
};

// ... and its profile, for nh layers: 4 words per layer (what rm_read_support copies out), then 2 per layer for the runs and
// the landings.
struct SupportProfile {
    Carver a;
    Region<uint32_t> profile, extra;
    size_t bytes;
    explicit SupportProfile(uint32_t nh) : profile(a.take<uint32_t>((size_t)nh * 4u)), extra(a.take<uint32_t>((size_t)nh * 2u)), bytes(a.total) {}
};

// rm_islands_solid / rm_islands_occupancy, for a lattice of n points in nb bricks, nh layers, bit planes of n_words u64 words and
// n_rblocks blocks of 256 points for the numbering: the occupancy, the brick classes, the probe's sums, totals and evaluation
// count and the planes `ins` and `ov` as SupportScratch has them; per point its parent and its region number in the canonical
// frame (4 B each); the numbering's block sums and total; per layer the regions before it (nh + 1 words); the automatic plate's
// height and the merge count.  Labels, mask, profile and the region table are the result and lie in buffers of their own.
struct IslandsScratch {
    Carver a;
    Region<uint8_t> occ, cls;
    Region<unsigned long long> psums, ptot, evals, ins, ov;
    Region<uint32_t> parent, lab;
    Region<unsigned long long> rsums, rtot;
    Region<uint32_t> lbase, plate, totals;
    size_t bytes;
    IslandsScratch(uint32_t n, uint32_t nb, uint32_t n_pblocks, uint32_t n_words, uint32_t n_rblocks, uint32_t nh)
        : occ(a.take<uint8_t>(n)), cls(a.take<uint8_t>(nb)), psums(a.take<unsigned long long>(n_pblocks)),
          ptot(a.take<unsigned long long>(2)), evals(a.take<unsigned long long>(2)), ins(a.take<unsigned long long>(n_words)),
          ov(a.take<unsigned long long>(n_words)), parent(a.take<uint32_t>(n)), lab(a.take<uint32_t>(n)),
          rsums(a.take<unsigned long long>(n_rblocks)), rtot(a.take<unsigned long long>(2)), lbase(a.take<uint32_t>((size_t)nh + 1u)),
          plate(a.take<uint32_t>(4)), totals(a.take<uint32_t>(4)), bytes(a.total) {}
};

// ... and its region table: kIslRowWords u32 per region (RM_ISL_ROW_*), allocated once the regions are counted.
constexpr uint32_t kIslRowWords = 12u;
struct IslandsRows {
    Carver a;
    Region<uint32_t> rows;
    size_t bytes;
    explicit IslandsRows(uint64_t regions) : rows(a.take<uint32_t>(regions * kIslRowWords)), bytes(a.total) {}
};

// rm_surface_solid / rm_surface_classes, for a lattice of n points in nb bricks counted by n_groups workgroups: per point its
// class (1 B; `occ`, as the front end names the region it fills); per brick its class, per 256 bricks the probe's block sum,
// totals and the evaluation count as above; per workgroup one row of kSurfRowWords u32 counts; the reduced row (u64).  Nothing
// is retained.
constexpr uint32_t kSurfRowWords = 840u;  // RM_SURF_COUNTS (rm_lds_layout.h kSurfCounts)
struct SurfScratch {
    Carver a;
    Region<uint8_t> occ, cls;
    Region<unsigned long long> psums, ptot, evals;
    Region<uint32_t> rows;
    Region<unsigned long long> result;
    uint32_t n_groups;
    size_t bytes;
    SurfScratch(uint32_t n, uint32_t nb, uint32_t n_pblocks, uint32_t groups)
        : occ(a.take<uint8_t>(n)), cls(a.take<uint8_t>(nb)), psums(a.take<unsigned long long>(n_pblocks)),
          ptot(a.take<unsigned long long>(2)), evals(a.take<unsigned long long>(2)), rows(a.take<uint32_t>((size_t)groups * kSurfRowWords)),
          result(a.take<unsigned long long>(kSurfRowWords)), n_groups(groups), bytes(a.total) {}
};

// rm_mesh_classes, for a lattice of nx x ny x nz points: its corner lattice has (nx + 1)(ny + 1)(nz + 1) corners in WORDS of 64
// consecutive corners of an x row (cmesh_row_words(nx) to a row, the last one partly beyond it), kCmeshGroupWords words to a
// workgroup of the mark kernel.  Per point its class (1 B, the caller's bytes); per word the ballot of its used corners (8 B)
// and the vertices and faces before it in its workgroup (4 B: v | f << 16); per workgroup its (vertices | faces << 32), scanned
// in place, and the two totals; per workgroup two rows of 16 words, per 256 rows one folded row, the reduced row.
constexpr uint32_t kCmeshGroupWords = 16u;
constexpr uint32_t cmesh_row_words(uint32_t nx) { return (nx + 1u + 63u) >> 6; }
constexpr uint32_t cmesh_words(uint32_t nx, uint32_t ny, uint32_t nz) { return cmesh_row_words(nx) * (ny + 1u) * (nz + 1u); }  // (< 2^24)
constexpr uint32_t cmesh_groups(uint32_t n_words) { return (n_words + kCmeshGroupWords - 1u) / kCmeshGroupWords; }
struct ClassMeshScratch {
    Carver a;
    Region<uint8_t> cls;
    Region<unsigned long long> bits;
    Region<uint32_t> before;
    Region<unsigned long long> bsums, btot, rows, folded, result;
    uint32_t n_words, n_groups;
    size_t bytes;
    ClassMeshScratch(uint32_t nx, uint32_t ny, uint32_t nz)
        : cls(a.take<uint8_t>((size_t)nx * ny * nz)), bits(a.take<unsigned long long>(cmesh_words(nx, ny, nz))),
          before(a.take<uint32_t>(cmesh_words(nx, ny, nz))), bsums(a.take<unsigned long long>(cmesh_groups(cmesh_words(nx, ny, nz)))),
          btot(a.take<unsigned long long>(2)), rows(a.take<unsigned long long>((size_t)cmesh_groups(cmesh_words(nx, ny, nz)) * 2u * 16u)),
          folded(a.take<unsigned long long>((size_t)((cmesh_groups(cmesh_words(nx, ny, nz)) * 2u + 255u) / 256u) * 16u)),
          result(a.take<unsigned long long>(16)), n_words(cmesh_words(nx, ny, nz)), n_groups(cmesh_groups(cmesh_words(nx, ny, nz))),
          bytes(a.total) {}
};

// ... and the retained slot of a class mesh of V vertices and T triangles: positions (3 floats), indices (3 u32 per triangle), ids
// (2 u32 per triangle).
struct ClassMeshSlot {
    Carver a;
    Region<float> vertices;
    Region<uint32_t> triangles, ids;
    size_t bytes;
    ClassMeshSlot(uint64_t V, uint64_t T) : vertices(a.take<float>(V * 3u)), triangles(a.take<uint32_t>(T * 3u)), ids(a.take<uint32_t>(T * 2u)), bytes(a.total) {}
};

// rm_slice_contours' per-layer tables: heights, layer_first, the first vertex of each layer of a batch of `per`, totals.
// (heights and layer_first lie before anything `per` sizes: rm_read_slices finds layer_first without it.)
struct SliceLayerTables {
    Carver a;
    Region<float> heights;
    Region<uint32_t> layer_first, base, totals;
    size_t bytes;
    explicit SliceLayerTables(uint32_t n_layers, uint32_t per = 0)
        : heights(a.take<float>(n_layers)), layer_first(a.take<uint32_t>((size_t)n_layers + 1u)),
          base(a.take<uint32_t>((size_t)per + 1u)), totals(a.take<uint32_t>(4)), bytes(a.total) {}
};

// ... the per-point scratch of a batch of n_max points in nb_max blocks: distances, packed vertex bases, block sums.
struct SlicePointScratch {
    Carver a;
    Region<float> dist;
    Region<uint32_t> packed, sums;
    size_t bytes;
    SlicePointScratch(uint32_t n_max, uint32_t nb_max)
        : dist(a.take<float>(n_max)), packed(a.take<uint32_t>(n_max)), sums(a.take<uint32_t>(nb_max)), bytes(a.total) {}
};

// ... and the per-vertex scratch of a batch of V vertices: next, prev, two (8-byte) ranking states, start, their block sums
// (vsb blocks), and per contour (at most c_max) length and first point.  Pair is the kernels' uint2.
template <class Pair>
struct SliceVertexScratch {
    Carver a;
    Region<uint32_t> next, prev;
    Region<Pair> state0, state1;
    Region<uint32_t> start, vsums, length, first_point;
    size_t bytes;
    SliceVertexScratch(uint32_t V, uint32_t vsb, uint32_t c_max)
        : next(a.take<uint32_t>(V)), prev(a.take<uint32_t>(V)), state0(a.take<Pair>(V)), state1(a.take<Pair>(V)),
          start(a.take<uint32_t>(V)), vsums(a.take<uint32_t>(vsb)), length(a.take<uint32_t>(c_max)),
          first_point(a.take<uint32_t>(c_max)), bytes(a.total) {}
};

// rm_slice_contours' attributes of its P points, in a buffer of their own: normals (3 floats) and (leaf, material) pairs, each
// only if asked for.
struct SliceAttributes {
    Carver a;
    Region<float> normals;
    Region<uint32_t> ids;
    size_t bytes;
    SliceAttributes(uint64_t P, bool with_normals, bool with_ids)
        : normals(a.take<float>(with_normals ? P * 3u : 0u)), ids(a.take<uint32_t>(with_ids ? P * 2u : 0u)), bytes(a.total) {}
};

// rml::sort_pairs (rm_sort.h), for n pairs in sort_tiles(n) tiles of kSortTile: the second buffer of each ping-pong pair (keys 8 B,
// values 4 B), the table of digit counts [kSortDigits][tiles] (4 B each; scanned in place into output positions), per kSortTile
// table entries a block sum (scanned in place) and the two totals.
constexpr uint32_t kSortTile = 1024u, kSortDigits = 256u;
constexpr uint32_t sort_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kSortTile - 1u) / kSortTile); }
constexpr uint32_t sort_passes(uint32_t bits) { return (bits + 7u) / 8u; }
constexpr uint32_t sort_table_blocks(uint32_t n) { return (uint32_t)(((uint64_t)sort_tiles(n) * kSortDigits + kSortTile - 1u) / kSortTile); }
struct SortScratch {
    Carver a;
    Region<unsigned long long> keys;
    Region<uint32_t> values, table;
    Region<unsigned long long> bsums, btot;
    size_t bytes;
    explicit SortScratch(uint32_t n)
        : keys(a.take<unsigned long long>(n)), values(a.take<uint32_t>(n)), table(a.take<uint32_t>((size_t)sort_tiles(n) * kSortDigits)),
          bsums(a.take<unsigned long long>(sort_table_blocks(n))), btot(a.take<unsigned long long>(2)), bytes(a.total) {}
};

// rm_slice_mesh, for a mesh of n_vertices vertices and n_triangles triangles (H = 3 n_triangles half-edges) cut by n_layers planes:
// per vertex its snapped coordinates (3 i32; the first is kMsliceBad for a vertex that does not snap); per plane its doubled
// position P2 (i32); per half-edge its sort key (8 B) and number (4 B), its mate (4 B), the vertices before its own in edge-major
// order (H + 1 entries: the last is their number) and its first plane (4 B); per kSortTile half-edges a block sum, the totals;
// one row of 16 counts per 256 half-edges, per 256 rows a folded row, the reduced row; the edge sort's scratch; and the copies of a
// caller's host arrays (empty for device inputs).
constexpr int32_t kMsliceBad = 0x7FFFFFFF;
struct MeshSliceScratch {
    Carver a;
    Region<int32_t> vq, p2;
    Region<unsigned long long> hkeys;
    Region<uint32_t> hvals, mate, estart, k0;
    Region<unsigned long long> bsums, btot, rows, folded, result;
    Region<float> xyz;
    Region<uint32_t> idx;
    size_t sort, bytes;  // sort: where the SortScratch of the half-edges begins
    MeshSliceScratch(uint32_t n_vertices, uint32_t n_triangles, uint32_t n_layers, uint64_t host_vertices, uint64_t host_triangles)
        : vq(a.take<int32_t>((size_t)n_vertices * 3u)), p2(a.take<int32_t>(n_layers)), hkeys(a.take<unsigned long long>((size_t)n_triangles * 3u)),
          hvals(a.take<uint32_t>((size_t)n_triangles * 3u)), mate(a.take<uint32_t>((size_t)n_triangles * 3u)),
          estart(a.take<uint32_t>((size_t)n_triangles * 3u + 1u)), k0(a.take<uint32_t>((size_t)n_triangles * 3u)),
          bsums(a.take<unsigned long long>(sort_tiles(n_triangles * 3u))), btot(a.take<unsigned long long>(2)),
          rows(a.take<unsigned long long>((size_t)((n_triangles * 3u + 255u) / 256u) * 16u)),
          folded(a.take<unsigned long long>((size_t)(((n_triangles * 3u + 255u) / 256u + 255u) / 256u) * 16u)),
          result(a.take<unsigned long long>(16)), xyz(a.take<float>(host_vertices * 3u)), idx(a.take<uint32_t>(host_triangles * 3u)),
          sort(a.total), bytes(a.total + SortScratch(n_triangles * 3u).bytes) {}
};

// ... and per vertex of the slices (N of them; an ITEM is a vertex in edge-major order, its ID its place in layer-major order):
// the item's sort key (its plane, 8 B) and number (4 B), the id of each item and the canonical half-edge of each id (4 B each), the
// first id of each layer (n_layers + 1 entries), the ranking scans' totals, one row of 16 counts per 256 vertices with their
// folded rows and the reduced row, and the item sort's scratch.
struct MeshSliceItems {
    Carver a;
    Region<unsigned long long> ikeys;
    Region<uint32_t> ivals, inv, vh, layer_base, totals;
    Region<unsigned long long> rows, folded, result;
    size_t sort, bytes;
    MeshSliceItems(uint32_t N, uint32_t n_layers)
        : ikeys(a.take<unsigned long long>(N)), ivals(a.take<uint32_t>(N)), inv(a.take<uint32_t>(N)), vh(a.take<uint32_t>(N)),
          layer_base(a.take<uint32_t>((size_t)n_layers + 1u)), totals(a.take<uint32_t>(4)),
          rows(a.take<unsigned long long>(((size_t)N + 255u) / 256u * 16u)),
          folded(a.take<unsigned long long>((((size_t)N + 255u) / 256u + 255u) / 256u * 16u)), result(a.take<unsigned long long>(16)),
          sort(a.total), bytes(a.total + SortScratch(N).bytes) {}
};

// rm_hatch_slices, for slices of P points in n_layers layers: per layer its line set (4 floats: dx, dy, offset, spacing); per point
// (= per contour segment, numbered by its tail) the crossings before its own (P + 1 entries: the last is their number) and its first
// line (4 B each); per kSortTile points a block sum (scanned in place) and the totals; one row of 16 counts per kSortTile points,
// per 256 rows a folded row, the reduced row.
constexpr uint32_t kHatchMaxLines = 1u << 24;
struct HatchScratch {
    Carver a;
    Region<float> lines;
    Region<uint32_t> cstart, j0;
    Region<unsigned long long> bsums, btot, rows, folded, result;
    size_t bytes;
    HatchScratch(uint32_t P, uint32_t n_layers)
        : lines(a.take<float>((size_t)n_layers * 4u)), cstart(a.take<uint32_t>((size_t)P + 1u)), j0(a.take<uint32_t>(P)),
          bsums(a.take<unsigned long long>(sort_tiles(P))), btot(a.take<unsigned long long>(2)),
          rows(a.take<unsigned long long>((size_t)sort_tiles(P) * 16u)),
          folded(a.take<unsigned long long>((size_t)((sort_tiles(P) + 255u) / 256u) * 16u)), result(a.take<unsigned long long>(16)),
          bytes(a.total) {}
};

// ... and per crossing (N of them; an ITEM is a crossing in the order (segment, line)): the item's sort key (8 B) and number (4 B),
// its point (u, v: 8 B), the hatch segments before its own in sorted order (N + 1 entries: the last is H); the block sums, rows
// and totals as above; and the sort's scratch.
struct HatchItems {
    Carver a;
    Region<unsigned long long> ikeys;
    Region<uint32_t> ivals;
    Region<float> xs;
    Region<uint32_t> hstart;
    Region<unsigned long long> bsums, btot, rows, folded, result;
    size_t sort, bytes;
    explicit HatchItems(uint32_t N)
        : ikeys(a.take<unsigned long long>(N)), ivals(a.take<uint32_t>(N)), xs(a.take<float>((size_t)N * 2u)),
          hstart(a.take<uint32_t>((size_t)N + 1u)), bsums(a.take<unsigned long long>(sort_tiles(N))), btot(a.take<unsigned long long>(2)),
          rows(a.take<unsigned long long>((size_t)sort_tiles(N) * 16u)),
          folded(a.take<unsigned long long>((size_t)((sort_tiles(N) + 255u) / 256u) * 16u)), result(a.take<unsigned long long>(16)),
          sort(a.total), bytes(a.total + SortScratch(N).bytes) {}
};

// ... and the retained slot of H hatch segments in n_layers layers: the segments (4 floats: u, v of one end, u, v of the other),
// their lines (4 B) and layer_first (n_layers + 1 entries).
struct HatchSlot {
    Carver a;
    Region<float> segments;
    Region<uint32_t> line, layer_first;
    size_t bytes;
    HatchSlot(uint64_t H, uint32_t n_layers)
        : segments(a.take<float>(H * 4u)), line(a.take<uint32_t>(H)), layer_first(a.take<uint32_t>((size_t)n_layers + 1u)), bytes(a.total) {}
};

// The count pass's block sums are 64-bit numbers that rm_block_scan_kernel adds up half by half: lo = the sum of the low halves,
// hi = that of the high ones.  The crossings fit 32 bits iff no block sum has a high half and the low halves' sum is below 2^32.
constexpr bool hatch_crossings_fit(uint64_t lo, uint64_t hi) { return hi == 0u && lo < (1ull << 32); }
// The bits of the sort key L << 32 | key32 for all_lines = n_layers * n_lines lines (1..2^32): 32 + the bit length of all_lines - 1.
constexpr uint32_t hatch_key_bits(uint64_t all_lines) {
    uint32_t b = 0;
    while (b < 32u && ((all_lines - 1u) >> b) != 0u) b++;
    return 32u + b;
}

// rm_trace_rays' scratch of the attribute pass over n rays (nb workgroups of 256) with K event slots each: the stored count
// per ray, the workgroups' sums (scanned in place into offsets), the total (2 of 4 words), the compact (ray, slot) list -- K
// entries per ray at most -- and, only when the caller takes no event records, a copy of them for the positions.  Pair is the
// kernels' uint2.
template <class Pair>
struct TraceScratch {
    Carver a;
    Region<uint32_t> stored;
    Region<unsigned long long> sums;
    Region<uint32_t> totals;
    Region<Pair> list;
    Region<float> events;
    size_t bytes;
    TraceScratch(uint32_t n, uint32_t nb, uint32_t K, bool own_events)
        : stored(a.take<uint32_t>(n)), sums(a.take<unsigned long long>(nb)), totals(a.take<uint32_t>(4)),
          list(a.take<Pair>((size_t)n * K)), events(a.take<float>(own_events ? (size_t)n * K * 8u : 0u)), bytes(a.total) {}
};

// Where the arrays of a mesh of V vertices and T triangles lie in the mesh buffer; the attributes as above.
struct MeshLayout {
    Carver a;
    Region<float> vertices;
    Region<uint32_t> triangles;
    Region<float> normals;
    Region<uint32_t> ids;
    size_t bytes;
    MeshLayout(uint64_t V, uint64_t T, bool with_normals, bool with_ids)
        : vertices(a.take<float>(V * 3u)), triangles(a.take<uint32_t>(T * 3u)), normals(a.take<float>(with_normals ? V * 3u : 0u)),
          ids(a.take<uint32_t>(with_ids ? V * 2u : 0u)), bytes(a.total) {}
};

// Output rows of the strips first, first+stride, ... (strip_rows rows each) of an H-row image.
inline uint32_t strip_row_count(uint32_t H, uint32_t strip_rows, uint32_t first, uint32_t stride) {
    const uint32_t n_strips = (H + strip_rows - 1u) / strip_rows;
    uint32_t rows = 0;
    for (uint32_t sidx = first; sidx < n_strips; sidx += stride) {
        const uint32_t r0 = sidx * strip_rows;
        rows += H - r0 < strip_rows ? H - r0 : strip_rows;
    }
    return rows;
}

}  // namespace rml
