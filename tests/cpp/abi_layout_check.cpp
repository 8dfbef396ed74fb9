// abi_layout_check.cpp -- the scratch layouts of the host ABI (ray-marching_amd/csrc/rm_abi_layout.h) on the CPU, under
// ASan + UBSan (tests/test_decoder_fuzz_cpu.py).  For every layout: its regions lie in declaration order, start on 16-byte
// boundaries, do not overlap and end inside the total; and the total and every offset equal the formulas the entry points
// used to spell out by hand (chained align16 offsets), which are written out again here, not taken from the header.
// strip_row_count is checked against a direct loop over the strips.
#include "rm_abi_layout.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

namespace {

int g_checks = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

size_t a16(size_t b) { return (b + 15u) & ~(size_t)15u; }

struct Span { size_t offset, bytes; };
template <class T>
Span span(const rml::Region<T>& r) { return Span{r.offset, r.bytes}; }

// declaration order, alignment, no overlap, inside the total
void check_regions(std::initializer_list<Span> regions, size_t total) {
    size_t end = 0;
    for (const Span& r : regions) {
        CHECK(r.offset % 16u == 0u);
        CHECK(r.offset >= end);
        end = r.offset + r.bytes;
        CHECK(end >= r.offset && end <= total);
    }
}

struct Pair { uint32_t x, y; };       // the kernels' uint2
struct SegMap { uint32_t w[4]; };     // as large as rmk::SparseSegMap

void dense_mesh() {
    const uint32_t kMeshBlock = 2048u;
    for (uint64_t n64 : {8ull, 27ull, 2048ull, 2049ull, 1ull << 28}) {
        const uint32_t n = (uint32_t)n64, nb = (n + kMeshBlock - 1u) / kMeshBlock;
        const rml::DenseMeshScratch S(n, nb);
        const size_t dist_o = 0, vbase_o = a16((size_t)n * 4u), flags_o = vbase_o + a16((size_t)n * 4u), sums_o = flags_o + a16(n),
                     totals_o = sums_o + a16((size_t)nb * 8u);
        CHECK(S.dist.offset == dist_o && S.vbase.offset == vbase_o && S.flags.offset == flags_o && S.sums.offset == sums_o &&
              S.totals.offset == totals_o);
        CHECK(S.bytes == totals_o + 16u);
        check_regions({span(S.dist), span(S.vbase), span(S.flags), span(S.sums), span(S.totals)}, S.bytes);
    }
}

void sparse_mesh() {
    const uint32_t kBrickSegs = 64u, kSegBlock = 2048u, kTilePoints = 729u;
    static_assert(sizeof(SegMap) == 16 && sizeof(Pair) == 8, "stand-ins of the kernels' types");
    for (uint32_t nb : {1u, 255u, 256u, 257u}) {
        const uint32_t n_entries = nb + 1u, n_pblocks = (n_entries + 255u) / 256u;
        const rml::SparseBrickTables B(n_entries, n_pblocks);
        const size_t boff_o = 0, psums_o = a16((size_t)n_entries * 4u), ptot_o = psums_o + a16((size_t)n_pblocks * 8u), evals_o = ptot_o + 16u;
        CHECK(B.boff.offset == boff_o && B.psums.offset == psums_o && B.ptot.offset == ptot_o && B.evals.offset == evals_o);
        CHECK(B.bytes == evals_o + 16u);
        check_regions({span(B.boff), span(B.psums), span(B.ptot), span(B.evals)}, B.bytes);
        for (uint64_t K : {1ull, 3ull, 4097ull}) {
            const uint32_t n_segs = (uint32_t)(K * kBrickSegs), n_sblocks = (n_segs + kSegBlock - 1u) / kSegBlock;
            const rml::SparseKeptScratch<SegMap, Pair> S(K, kTilePoints, n_segs, n_sblocks);
            // (the segment maps and the first pairs were not rounded: K * 16 and 64 K * 8 bytes are multiples of 16 as they are)
            const size_t klist_o = 0, maps_o = a16((size_t)K * 4u), tiles_o = maps_o + (size_t)K * sizeof(SegMap),
                         words_o = tiles_o + a16((size_t)K * kTilePoints * 4u), first_o = words_o + a16((size_t)n_segs * 4u),
                         ssums_o = first_o + (size_t)n_segs * 8u, stot_o = ssums_o + a16((size_t)n_sblocks * 8u);
            CHECK(S.klist.offset == klist_o && S.maps.offset == maps_o && S.tiles.offset == tiles_o && S.words.offset == words_o &&
                  S.first.offset == first_o && S.ssums.offset == ssums_o && S.stot.offset == stot_o);
            CHECK(S.bytes == stot_o + 16u);
            check_regions({span(S.klist), span(S.maps), span(S.tiles), span(S.words), span(S.first), span(S.ssums), span(S.stot)}, S.bytes);
        }
    }
}

void slicing() {
    const uint32_t kSliceBlock = 1024u;
    for (uint32_t n_layers : {1u, 5u})
        for (uint32_t n_max : {4u, 1025u}) {  // per * n2
            for (uint32_t per : {1u, n_layers}) {
                const rml::SliceLayerTables T(n_layers, per);
                const size_t lf_o = a16((size_t)n_layers * 4u), base_o = lf_o + a16(((size_t)n_layers + 1u) * 4u),
                             totals_o = base_o + a16(((size_t)per + 1u) * 4u);
                CHECK(T.heights.offset == 0u && T.layer_first.offset == lf_o && T.base.offset == base_o && T.totals.offset == totals_o);
                CHECK(T.bytes == totals_o + 16u);
                check_regions({span(T.heights), span(T.layer_first), span(T.base), span(T.totals)}, T.bytes);
                // what rm_read_slices needs without knowing `per`
                const rml::SliceLayerTables R(n_layers);
                CHECK(R.layer_first.offset == lf_o && R.layer_first.bytes == ((size_t)n_layers + 1u) * 4u);
            }
            const uint32_t nb_max = (n_max + kSliceBlock - 1u) / kSliceBlock;
            const rml::SlicePointScratch S(n_max, nb_max);
            const size_t packed_o = a16((size_t)n_max * 4u), sums_o = packed_o + a16((size_t)n_max * 4u);
            CHECK(S.dist.offset == 0u && S.packed.offset == packed_o && S.sums.offset == sums_o);
            CHECK(S.bytes == sums_o + a16((size_t)nb_max * 4u));
            check_regions({span(S.dist), span(S.packed), span(S.sums)}, S.bytes);
        }
    for (uint32_t V : {2u, 3u, 1024u, 1025u}) {
        const uint32_t vsb = (V + kSliceBlock - 1u) / kSliceBlock, c_max = V / 2u + 1u;
        const rml::SliceVertexScratch<Pair> W(V, vsb, c_max);
        const size_t prev_o = a16((size_t)V * 4u), st0_o = prev_o + a16((size_t)V * 4u), st1_o = st0_o + a16((size_t)V * 8u),
                     start_o = st1_o + a16((size_t)V * 8u), vsums_o = start_o + a16((size_t)V * 4u),
                     len_o = vsums_o + a16((size_t)vsb * 4u), fp_o = len_o + a16((size_t)c_max * 4u),
                     work_bytes = fp_o + a16((size_t)c_max * 4u);
        CHECK(W.next.offset == 0u && W.prev.offset == prev_o && W.state0.offset == st0_o && W.state1.offset == st1_o &&
              W.start.offset == start_o && W.vsums.offset == vsums_o && W.length.offset == len_o && W.first_point.offset == fp_o);
        CHECK(W.bytes == work_bytes);
        check_regions({span(W.next), span(W.prev), span(W.state0), span(W.state1), span(W.start), span(W.vsums), span(W.length),
                       span(W.first_point)}, W.bytes);
        // the attributes of V points.  The total was ids_o + 8 V when ids are kept: the last region now rounds up like every
        // other, so the total may exceed the earlier one by less than 16 bytes.
        for (int f = 0; f < 4; f++) {
            const bool normals = (f & 1) != 0, ids = (f & 2) != 0;
            const rml::SliceAttributes A(V, normals, ids);
            const size_t ids_o = normals ? a16((size_t)V * 12u) : 0u, total = ids_o + (ids ? (size_t)V * 8u : 0u);
            CHECK(A.normals.offset == 0u && A.ids.offset == ids_o);
            CHECK(A.normals.bytes == (normals ? (size_t)V * 12u : 0u) && A.ids.bytes == (ids ? (size_t)V * 8u : 0u));
            CHECK(A.bytes >= total && A.bytes - total < 16u);
            check_regions({span(A.normals), span(A.ids)}, A.bytes);
        }
    }
}

void mesh_result() {
    const uint64_t shapes[4][2] = {{0, 0}, {1, 0}, {5, 3}, {(1ull << 20) + 1u, (1ull << 21) + 3u}};
    for (const auto& vt : shapes)
        for (int f = 0; f < 4; f++) {
            const uint64_t v = vt[0], t = vt[1];
            const bool normals = (f & 1) != 0, ids = (f & 2) != 0;
            const rml::MeshLayout L(v, t, normals, ids);
            const size_t triangles = a16(v * 12u), normals_o = triangles + a16(t * 12u), ids_o = normals_o + (normals ? a16(v * 12u) : 0u),
                         bytes = ids_o + (ids ? v * 8u : 0u);
            CHECK(L.vertices.offset == 0u && L.triangles.offset == triangles && L.normals.offset == normals_o && L.ids.offset == ids_o);
            CHECK(L.vertices.bytes == v * 12u && L.triangles.bytes == t * 12u);
            CHECK(L.normals.bytes == (normals ? v * 12u : 0u) && L.ids.bytes == (ids ? v * 8u : 0u));
            // the total was the unrounded end of the ids: the last region now rounds up like every other, so the total may
            // exceed the earlier one by less than 16 bytes
            CHECK(L.bytes >= bytes && L.bytes - bytes < 16u);
            check_regions({span(L.vertices), span(L.triangles), span(L.normals), span(L.ids)}, L.bytes);
        }
}

void strips() {
    for (uint32_t H : {1u, 8u, 9u, 1080u})
        for (uint32_t strip_rows : {8u, 144u})
            for (uint32_t stride : {1u, 3u, 8u})
                for (uint32_t first = 0; first < stride; first++) {
                    uint32_t rows = 0;
                    for (uint32_t r = 0; r < H; r++)
                        if ((r / strip_rows) % stride == first) rows++;
                    CHECK(rml::strip_row_count(H, strip_rows, first, stride) == rows);
                }
}

// a region resolves to base + offset, typed
void resolve() {
    alignas(16) static char buf[256];
    const rml::DenseMeshScratch S(8, 1);
    CHECK(S.bytes <= sizeof buf);
    CHECK(reinterpret_cast<char*>(S.vbase.at(buf)) == buf + S.vbase.offset);
    S.totals.at(buf)[3] = 7u;
    CHECK(static_cast<const rml::Region<uint32_t>&>(S.totals).at(static_cast<const void*>(buf))[3] == 7u);
}

}  // namespace

int main() {
    dense_mesh();
    sparse_mesh();
    slicing();
    mesh_result();
    strips();
    resolve();
    std::printf("abi layout ok (%d checks)\n", g_checks);
    return 0;
}
