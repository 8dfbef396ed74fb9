// rm_abi.hip -- host side of librm_hip.so: the C ABI declared in include/rm_abi.h.
// Mirrors RayMarchingResources / RayMarchingCallback::{prepare,paint}
// (src/ray_marching/renderer.rs:43-49, 51-175, 195-256 of the reference).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "rm_abi.h"
#include "rm_abi_layout.h"
#include "rm_lds_layout.h"
#include "rm_decode.h"
#include "rm_jit.h"
#include "rm_device.h"
#include "rm_kernels.h"
#include "rm_interp.h"
#include "rm_kernel_v5.h"
#include "rm_query.h"
#include "rm_reduce.h"
#include "rm_trace.h"
#include "rm_mesh.h"
#include "rm_mesh_bound.h"
#include "rm_mesh_sparse.h"
#include "rm_mass.h"
#include "rm_topology.h"
#include "rm_distance.h"
#include "rm_support.h"
#include "rm_islands.h"
#include "rm_surface.h"
#include "rm_voxel.h"
#include "rm_lattice.h"
#include "rm_class_mesh.h"
#include "rm_slice.h"
#include "rm_sort.h"
#include "rm_mesh_slice.h"
#include "rm_hatch.h"
#include "rm_light.h"
#include "rm_gbuffer.h"

#define RM_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

constexpr uint64_t kRefCmdBufferBytes = 1024;  // renderer.rs:142-147
constexpr uint64_t kMaxCmdBufferBytes = 65536;
constexpr uint32_t kMaxDim = 1u << 16;
constexpr uint32_t kMaxIter = 1u << 16;
constexpr uint32_t kPruneLeaves = 12;  // RM_OPT_PRUNE = 2: programs that EVALUATE this many spheres + boxes (RmDecoded::n_leaves: subtracted
                                        // ones included, they have no miss-test slot but cost the same) get the pruned kernel

constexpr uint32_t kBlendPruneLeaves = 8;  // ... and programs that blend, the rules of their chains (rm_units.h), from this many
thread_local std::string g_create_error;
// enum rm_light: P (wgsl:100), S, k, b, shadow max t, shadow steps, A, AO step, falloff, scale, taps
#define RM_LIGHT_DEFAULTS {2.0f, -5.0f, 3.0f, 1.0f, 8.0f, 0.02f, 20.0f, 64.0f, 1.0f, 0.1f, 0.75f, 1.5f, 5.0f}
const float kLightDefaults[RM_LIGHT_PARAMS] = RM_LIGHT_DEFAULTS;

int fail(rm_ctx* c, int status, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, RM_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                       \
    } while (0)

// An array of T in device memory, owned: freed when the context, or the call that made it, goes away.  It only ever grows
// (scratch is allocated outside of any timed or captured region the first time a size is seen; later calls of the same size
// allocate nothing).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // in elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class U>
    U* as() const { return reinterpret_cast<U*>(p); }  // (the byte buffers: what they hold depends on the call)
    // Room for `need` elements; contents are lost when the buffer moves (the old one goes first: never both at once).
    int reserve(rm_ctx* c, size_t need, const char* what = "scratch") {
        if (need <= cap) return RM_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T));
        if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "hipMalloc(%s) failed: %s", what, hipGetErrorString(e));
        cap = need;
        return RM_OK;
    }
    // reserve() for a result that is built batch by batch: the first `used` elements survive the move
    int grow_keep(rm_ctx* c, size_t need, size_t used, hipStream_t s) {
        if (need <= cap) return RM_OK;
        DevBuf fresh;
        if (hipMalloc(reinterpret_cast<void**>(&fresh.p), (need + need / 2u) * sizeof(T)) == hipSuccess) {
            fresh.cap = need + need / 2u;
        } else {
            (void)hipGetLastError();
            if (int rc = fresh.reserve(c, need)) return rc;
        }
        if (used) {
            HIP_TRY(c, hipMemcpyAsync(fresh.p, p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
            HIP_TRY(c, hipStreamSynchronize(s));
        }
        *this = std::move(fresh);  // (the old buffer goes with `fresh`)
        return RM_OK;
    }
};

}  // namespace

struct rm_ctx {
    int device = -1;
    int cu_count = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Draws of one context share its scratch (program copy, tile cost / order / counters / measurements).  They are
    // ordered by their stream; when a draw arrives on ANOTHER stream than the previous one (a host-destination draw
    // runs on the context's own stream, device-destination draws on the caller's), the new stream first waits for
    // everything queued on the previous one: order_with_previous().
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t ev_order = nullptr;
    // RM_OPT_TIMING: one event pair per timed launch of the dominant kernel, read back (and
    // reset) by rm_get_info(RM_INFO_KERNEL_MS): no synchronisation inside the launch path.
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
    size_t tev_used = 0;
    // host shadows of the three buffers of the reference's bind group
    rm_limits limits{0.01f, 100.0f, 100u};  // renderer.rs:133-137
    rm_uniforms uniforms{};                 // Uniforms::default(), renderer.rs:126
    std::vector<uint32_t> cmd;              // [0] = cmd_count, [1..] = words; zero-initialised like a wgpu buffer
    bool cmd_dirty = true;
    int cmd_status = RM_OK;
    // decoded program, device copy
    RmDecoded decoded;
    DevBuf<RmRecord> d_prog;
    DevBuf<float4> d_bounds;  // world-space bounding spheres of a program with transforms (RmDecoded::bounds)
    // materials (extension): the tagged decoding of the program and the albedo table
    DevBuf<RmRecord> d_mprog;
    std::vector<float4> materials{make_float4(0.4f, 0.7f, 0.1f, 0.0f)};  // wgsl:105
    DevBuf<float4> d_materials;  // RM_MAX_MATERIALS entries
    bool materials_dirty = true;
    // scene queries (rm_query.h): the query program (RmDecoded::qrec), uploaded by the first query after a program change
    // (prog_gen it belongs to in qprog_gen: draws never upload it), and the staging buffers of host-memory queries (never
    // the draws' scratch)
    DevBuf<RmRecord> d_qprog;
    uint64_t qprog_gen = ~0ull;
    DevBuf<char> d_qin, d_qout;
    DevBuf<char> d_tscratch;  // ray traversal (rm_trace.h): the attribute pass's scratch (rml::TraceScratch)
    size_t max_lds = 0;  // LDS a workgroup may allocate on this device
    // lit rendering (rm_light.h): enum rm_light, validated by rm_set_lighting; travels with each lit draw as kernel arguments
    float light[RM_LIGHT_PARAMS] = RM_LIGHT_DEFAULTS;
    // the scratch of the lattice calls (mesh, slices, mass and the analyses; none of it holds a result), and that of the sparse
    // extraction's and the mass moments' per-brick tables (rm_mesh_sparse.h; d_mscratch then holds the kept bricks' data)
    DevBuf<char> d_mscratch, d_mbricks;
    // Retained results (DESIGN.md "Retained results"): what a call leaves behind for rm_read_*, one slot per family -- its own
    // buffers, the dimensions a read needs, and `valid`, which only the slot's two operations write.  drop(): the previous result
    // is gone; a call says so after its last check that can refuse, when its scratch is reserved and the slot's buffers start to
    // change, not before.  commit(dims): the last statement of a successful call.
    struct Mesh {  // rm_extract_mesh, rm_extract_mesh_sparse: the arrays of mesh_layout(v, t, flags) in buf
        DevBuf<char> buf;
        bool valid = false;
        uint64_t v = 0, t = 0;
        uint32_t flags = 0;
        void drop() { valid = false; }
        void commit(uint64_t v_, uint64_t t_, uint32_t flags_) { v = v_, t = t_, flags = flags_, valid = true; }
    } mesh;
    struct Slices {  // rm_slice_contours: points, contours, attributes (rml::SliceAttributes) and layer_first in the per-layer tables
        DevBuf<char> points, contours, attr, layers;  // layers (rml::SliceLayerTables) also holds the call's small scratch
        bool valid = false;
        uint64_t p = 0, c = 0;
        uint32_t n_layers = 0, flags = 0, axis = 0;
        void drop() { valid = false; }
        void commit(uint64_t p_, uint64_t c_, uint32_t n_layers_, uint32_t flags_, uint32_t axis_) {
            p = p_, c = c_, n_layers = n_layers_, flags = flags_, axis = axis_, valid = true;
        }
    } slices;
    struct Hatch {  // rm_hatch_slices: the arrays of rml::HatchSlot(h, n_layers) in buf; of the slices as they were at the call
        DevBuf<char> buf;
        bool valid = false;
        uint64_t h = 0;
        uint32_t n_layers = 0;
        void drop() { valid = false; }
        void commit(uint64_t h_, uint32_t n_layers_) { h = h_, n_layers = n_layers_, valid = true; }
    } hatch;
    // A call that replaces the slices: their hatch is no longer of slices that exist.
    void drop_slices() { slices.drop(), hatch.drop(); }
    DevBuf<char> d_swork;  // slicing (rm_slice.h): the per-vertex scratch of a batch of layers
    struct Labels {  // rm_label_*: the label volume of n points and the rows (rml::TopoRows) of b bodies and c cavities
        DevBuf<char> labels, rows;
        bool valid = false;
        uint64_t n = 0, b = 0, c = 0;
        void drop() { valid = false; }
        void commit(uint64_t n_, uint64_t b_, uint64_t c_) { n = n_, b = b_, c = c_, valid = true; }
    } topo;
    struct Distance {  // rm_distance_*: the distance volume, and nested the feature mask rm_distance_features made of it
        DevBuf<char> vol;
        bool valid = false;
        uint32_t nx = 0, ny = 0, nz = 0;
        struct Mask {
            DevBuf<char> buf;
            bool valid = false;
            void drop() { valid = false; }
            void commit() { valid = true; }
        } mask;
        size_t points() const { return (size_t)nx * ny * nz; }
        void drop() { valid = false, mask.drop(); }
        void commit(uint32_t nx_, uint32_t ny_, uint32_t nz_) { nx = nx_, ny = ny_, nz = nz_, valid = true; }
    } dist;
    struct Support {  // rm_support_*: the mask of n points and the profile (rml::SupportProfile) of nh layers
        DevBuf<char> mask, profile;
        bool valid = false;
        uint32_t n = 0, nh = 0;
        void drop() { valid = false; }
        void commit(uint32_t n_, uint32_t nh_) { n = n_, nh = nh_, valid = true; }
    } sup;
    struct Islands {  // rm_islands_*: labels and mask of n points, the profile of nh layers, the table (rml::IslandsRows) of `regions`
        DevBuf<char> labels, mask, profile, rows;
        bool valid = false;
        uint32_t n = 0, nh = 0;
        uint64_t regions = 0;
        void drop() { valid = false; }
        void commit(uint32_t n_, uint32_t nh_, uint64_t regions_) { n = n_, nh = nh_, regions = regions_, valid = true; }
    } isl;
    struct Voxels {  // rm_voxelize_mesh: the occupancy of nx x ny x nz points, one byte each
        DevBuf<char> buf;
        bool valid = false;
        uint32_t nx = 0, ny = 0, nz = 0;
        size_t points() const { return (size_t)nx * ny * nz; }
        void drop() { valid = false; }
        void commit(uint32_t nx_, uint32_t ny_, uint32_t nz_) { nx = nx_, ny = ny_, nz = nz_, valid = true; }
    } vox;
    struct Lattice {  // rm_set_lattice: the classes of nx x ny x nz points and the traversal's bit words (rml::LatticeSlot)
        DevBuf<char> buf;
        bool valid = false;
        uint32_t nx = 0, ny = 0, nz = 0;
        float origin[3] = {0.0f, 0.0f, 0.0f}, step[3] = {1.0f, 1.0f, 1.0f};
        void drop() { valid = false; }
        void commit(uint32_t nx_, uint32_t ny_, uint32_t nz_, const float* o, const float* st) {
            nx = nx_, ny = ny_, nz = nz_, valid = true;
            for (int a = 0; a < 3; a++) origin[a] = o[a], step[a] = st[a];
        }
    } lat;
    struct ClassMesh {  // rm_mesh_classes: the arrays of rml::ClassMeshSlot(v, t) in buf
        DevBuf<char> buf;
        bool valid = false;
        uint64_t v = 0, t = 0;
        void drop() { valid = false; }
        void commit(uint64_t v_, uint64_t t_) { v = v_, t = t_, valid = true; }
    } cmesh;
    // scratch for host-destination draws and batch uniforms
    DevBuf<char> d_out;
    DevBuf<rm_uniforms> d_frames;
    // options / info
    int kernel = RM_KERNEL_DEFAULT;
    uint32_t refill_min_v5 = 0;  // 0: by what the kernel does with coherent rays (launch_v5_w)
    bool cull = true;
    int balance = 3;  // RM_OPT_BALANCE: 0 raster order, 1 most pending pixels first, 2 partially covered tiles first,
                      // 3 (default) longest tiles of the previous draw of the same shape first
    int waves_per_tile = 0;  // 0: by the size of the launch (launch_v5)
    bool wave_stats = false;
    DevBuf<unsigned long long> d_stats;
    size_t stats_valid_bytes = 0;
    DevBuf<uint32_t> d_cost, d_order;  // per-tile cost estimates / dispatch order of the balance pre-pass
    DevBuf<uint32_t> d_masks;          // per-tile primitive masks of the pre-pass, for the march kernel's ray tests
    DevBuf<uint32_t> d_counters;       // v5: {work-list length, cursor} per frame
    DevBuf<uint32_t> d_measured;       // v5, RM_OPT_BALANCE = 3: per-tile durations of the previous draw of the same shape
    uint64_t measured_shape = 0;       // hash of (W, rows, strips, frames) the measurements belong to; 0 = none yet
    bool timing = false;
    double last_kernel_ms = 0.0;
    // structure specialisation (rm_jit.h): 0 off, 1 compile in the background and switch over when
    // ready, 2 wait for the compiler at the first draw of a new structure
    int specialize = 1;
    int out_format = RM_FORMAT_RGBA32F;  // RM_OPT_OUTPUT_FORMAT
    int prune = 2;  // RM_OPT_PRUNE: far-primitive pruning in specialised kernels: 0 off, 1 on, 2 (default) on for programs
                    // with at least kPruneLeaves spheres + boxes (measured: 4 leaves -6 %, 16 leaves +6 %, 32 leaves +14 %)
    uint64_t prog_gen = 0;  // bumped whenever the decoded program changes
    std::shared_ptr<rmjit::Entry> spec;
    uint64_t spec_gen = ~0ull;
    int spec_wpt = 0;
    int spec_pruned = 0;            // rmjit::PRUNE_* of the requested kernel
    bool spec_stats = false;        // ... and whether it keeps the counters of RM_OPT_WAVE_STATS
    bool spec_range = false;        // ... and whether it is the variant without the range guards (rmjit::KERNEL_RANGE_PROVED)
    bool last_specialized = false;  // the last march launch ran a specialised kernel
    bool last_range_proof = false;  // ... the variant without the range guards (RM_INFO_RANGE_PROOF)
    int last_loop = 0;              // RM_INFO_INTERPRETER_LOOP of the last march launch
    // stream-ordered uploads (program records, bounds, batch uniforms): four pinned staging buffers, see upload()
    struct Staging { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
    Staging staging[4];
    unsigned staging_next = 0;
    std::string err;
};

namespace {

int fail(rm_ctx* c, int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return status;
}

// Host data -> device scratch of the context, ordered on the stream the next draw is issued on (what
// queue.write_buffer is to wgpu, renderer.rs:213-239): a draw of the previous program that is still queued or
// running on `s` keeps reading the previous contents, and the caller's memory is free again when this returns.
// The bytes wait in one of four pinned staging buffers; only a fifth upload with the first still pending blocks.
int upload(rm_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t s) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) (void)hipGetLastError();
    else if (capturing != hipStreamCaptureStatusNone)
        return fail(c, RM_ERR_ARG, "the program or batch changed during stream capture: draw once before capturing");
    rm_ctx::Staging& st = c->staging[c->staging_next++ & 3u];
    if (st.pending) {
        HIP_TRY(c, hipEventSynchronize(st.done));
        st.pending = false;
    }
    if (bytes > st.cap) {
        if (st.host) (void)hipHostFree(st.host);
        st.host = nullptr;
        st.cap = 0;
        const size_t cap = std::max<size_t>(4096, bytes + bytes / 2);
        HIP_TRY(c, hipHostMalloc(&st.host, cap, hipHostMallocDefault));
        st.cap = cap;
    }
    if (!st.done) HIP_TRY(c, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    std::memcpy(st.host, src, bytes);
    HIP_TRY(c, hipMemcpyAsync(dst, st.host, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(st.done, s));
    st.pending = true;
    return RM_OK;
}

int ensure_program(rm_ctx* c, hipStream_t s) {
    if (!c->cmd_dirty) return c->cmd_status;
    c->cmd_dirty = false;
    const uint32_t cap_words = (uint32_t)c->cmd.size() - 1u;
    RmDecoded d;
    int rc = rm_decode_program(c->cmd[0], c->cmd.data() + 1, cap_words, &d);
    if (rc != RM_OK) {
        c->cmd_status = rc;
        return fail(c, rc, "invalid CSG program in command buffer: %s", rm_status_string(rc));
    }
    // the unit records of wave-level culling (RmDecoded::units) follow the program's records in the same buffer
    std::vector<RmRecord> image = d.rec;
    image.insert(image.end(), d.units.begin(), d.units.end());
    image.insert(image.end(), d.tree.begin(), d.tree.end());  // ... and the operand masks of a tree program's records (RmDecoded::tree)
    // device copies: room for twice what is needed (an edited scene grows record by record), then the stream-ordered upload;
    // a program that did not arrive is decoded and sent again by the next draw
    auto put = [&](auto& buf, const char* what, size_t n, const void* src, size_t bytes) {
        int prc = n <= buf.cap ? RM_OK : buf.reserve(c, std::max<size_t>(64, 2 * n), what);
        if (prc == RM_OK && bytes) prc = upload(c, buf.p, src, bytes, s);
        if (prc != RM_OK) c->cmd_dirty = true;
        return prc;
    };
    if (int prc = put(c->d_prog, "program", image.size(), image.data(), image.size() * sizeof(RmRecord))) return prc;
    if (!d.bounds.empty())
        if (int prc = put(c->d_bounds, "bounds", d.bounds.size() / 4u, d.bounds.data(), d.bounds.size() * sizeof(float))) return prc;
    if (!d.mrec.empty())
        if (int prc = put(c->d_mprog, "material program", d.mrec.size(), d.mrec.data(), d.mrec.size() * sizeof(RmRecord))) return prc;
    c->decoded = std::move(d);
    c->prog_gen++;
    c->cmd_status = RM_OK;
    return RM_OK;
}

// The material table of a tagged program, on the stream of the draw that needs it.
int upload_materials(rm_ctx* c, hipStream_t s);
int ensure_materials(rm_ctx* c, hipStream_t s) {
    if (!c->decoded.has_materials) return RM_OK;
    if (c->decoded.max_material >= c->materials.size())
        return fail(c, RM_ERR_MATERIAL, "the program tags a surface with material %u, the material table has %zu entries "
                    "(rm_set_materials)", c->decoded.max_material, c->materials.size());
    return upload_materials(c, s);
}
// The device copy of the material table as it stands (the lattice draw reads it whatever the program tags).
int upload_materials(rm_ctx* c, hipStream_t s) {
    if (int rc = c->d_materials.reserve(c, RM_MAX_MATERIALS, "materials")) return rc;
    if (c->materials_dirty) {
        if (int rc = upload(c, c->d_materials.p, c->materials.data(), c->materials.size() * sizeof(float4), s)) return rc;
        c->materials_dirty = false;
    }
    return RM_OK;
}

// Which skipping rule the specialised kernel of a program gets (rmjit::PRUNE_*): RM_OPT_PRUNE 0 none, 1 whichever applies, 2
// (default) whichever applies if the program evaluates enough leaves for the tests to pay.
int prune_kind(const RmDecoded& d, int option) {
    if (option == 0) return rmjit::PRUNE_NONE;
    if (d.unit_mode == RM_UNITS_LATTICE && (option == 1 || d.n_leaves >= kPruneLeaves)) return rmjit::PRUNE_LATTICE;
    if (d.unit_mode == RM_UNITS_BLEND && (option == 1 || d.n_leaves >= kBlendPruneLeaves)) return rmjit::PRUNE_BLEND;
    return rmjit::PRUNE_NONE;
}

// Whether the march launches of the current program may run the kernel compiled without the range guards its facts make
// unnecessary (rm_interp.h "Range proofs"): every box half-extent at least 2^-23 in magnitude and finite (the lower side of the boxes'
// guard), no material table (the gamma roots), and a kernel that has the variant at all -- a pruned lattice program
// (rmjit::range_variant).  Nothing here depends on the camera, the limits or where the uniforms live: a batch of frames qualifies.
// RM_JIT_RANGE_PROOF=0 in the environment (read at every launch) keeps the guarded kernel, for comparisons and tests.
bool range_facts_hold(const rm_ctx* c) {
    if (rmjit::jit_knob("RM_JIT_RANGE_PROOF", 1) == 0) return false;
    const RmDecoded& d = c->decoded;
    return d.box_sizes_normal && rmjit::range_variant(prune_kind(d, c->prune) | rmjit::KERNEL_RANGE_PROVED, !d.mrec.empty());
}

// The specialised march kernel for the current program and WPT waves per tile on this device, or
// nullptr: specialisation off, not possible, still compiling (mode 1) or failed -- the caller then
// launches the interpreter kernel.  Never an error.
// range_proved: the variant without the range guards the program's facts make unnecessary (range_facts_hold above).
hipFunction_t specialised_kernel(rm_ctx* c, int wpt, bool range_proved) {
    if (!c->specialize || !rmjit::can_specialise(c->decoded.rec)) return nullptr;
    if (c->spec_gen != c->prog_gen || c->spec_wpt != wpt || c->spec_stats != c->wave_stats || c->spec_range != range_proved) {
        // same structure as before (parameters moved): the key lookup finds the same entry
        const int prune = prune_kind(c->decoded, c->prune);
        // (the per-wave counters of RM_OPT_WAVE_STATS are compiled into a kernel of their own: the default one does without)
        c->spec = rmjit::Cache::get().request(c->decoded.rec, c->decoded.mrec, wpt, prune | (c->wave_stats ? rmjit::KERNEL_WITH_STATS : 0) |
                                                                                      (range_proved ? rmjit::KERNEL_RANGE_PROVED : 0));
        c->spec_pruned = prune;
        c->spec_stats = c->wave_stats;
        c->spec_range = range_proved;
        c->spec_gen = c->prog_gen;
        c->spec_wpt = wpt;
    }
    rmjit::Entry* e = c->spec.get();
    if (!e) return nullptr;
    const rmjit::Entry::State st = c->specialize >= 2 ? e->wait() : e->peek();
    if (st != rmjit::Entry::READY) return nullptr;
    std::lock_guard<std::mutex> lk(e->m);
    rmjit::Entry::Loaded& l = e->loaded[c->device];
    if (!l.function && !l.module && !e->code.empty()) {
        auto load = [&]() -> bool {
            hipModule_t mod = nullptr;
            hipFunction_t fn = nullptr;
            if (hipModuleLoadData(&mod, e->code.data()) == hipSuccess &&
                hipModuleGetFunction(&fn, mod, rmjit::kernel_name()) == hipSuccess) {
                l.module = mod;
                l.function = fn;
                return true;
            }
            (void)hipGetLastError();
            if (mod) (void)hipModuleUnload(mod);
            return false;
        };
        bool ok = load();
        if (!ok && !e->cached_source.empty()) {
            // the code object came from the disk cache and the loader rejects it (written by another driver stack, or
            // damaged in a way the checksum cannot see): drop the file and compile the source afresh, once
            const std::string src = std::move(e->cached_source);
            e->cached_source.clear();
            const std::string file = rmjit::cache_path(src);
            if (!file.empty()) std::remove(file.c_str());
            std::string log;
            double ms = 0.0;
            e->code.clear();
            if (rmjit::compile(src, &e->code, &log, &ms)) {
                e->compile_ms = ms;
                e->log += "\ncached code object rejected by the loader; recompiled";
                ok = load();
            } else {
                e->log += "\n" + log;
            }
        }
        if (ok) {
            // an evicted entry (more than 256 structures in one process) may still have launches in flight on a
            // context that moved on to another program: wait for the device before the code object goes away
            e->unload = [](void* m, int device) {
                int current = -1;
                if (hipGetDevice(&current) != hipSuccess) current = -1;
                if (hipSetDevice(device) == hipSuccess) (void)hipDeviceSynchronize();
                (void)hipModuleUnload(static_cast<hipModule_t>(m));
                if (current >= 0) (void)hipSetDevice(current);
                (void)hipGetLastError();
            };
        } else {
            e->log += "\nloading the compiled module failed";
            e->code.clear();  // do not try again
        }
    }
    return static_cast<hipFunction_t>(l.function);
}

int ensure_stats(rm_ctx* c, RmLaunch& L, size_t n_waves);

int finish_launch(rm_ctx* c);
int time_begin(rm_ctx* c, hipStream_t s);
int time_end(rm_ctx* c, hipStream_t s);

// What a march launch decides before it launches: whether the miss tests run, which record loop an interpreter kernel takes and
// whether it culls per wave -- written into L (n_cull, n_tree, spill_depth, flags, n_cone, n_slab).  The culling self-tests
// (rm_selftest_cull_*) fill their launch through it too, so that they see the fields a frame would see.
struct V5Plan { bool units; int loop; };
V5Plan plan_v5(rm_ctx* c, RmLaunch& L, bool lds) {
    const RmDecoded& d = c->decoded;
    bool cull = c->cull && L.n_rec <= 256u && !d.cull_veto;
    if (L.n_rec == 0u && L.max_dist < L.min_dist) cull = false;  // see launch_multi_w
    L.n_cull = cull ? L.n_rec : 0u;
    // Interpreter kernels: the record loop that runs the program (RM_INFO_INTERPRETER_LOOP) and whether it runs only the units the
    // wave's culling mask names (RmLaunch::flags bit 3).  Measured (profiles/r03_interpreter_loops.txt): over a chain the mask names
    // the records to fetch at all -- 64-node scene at 4K 15.5 -> 5.3 ms, metric scene 1.23 -> 0.71 ms --, and over a tree the records
    // that are left once operands without a needed leaf are dropped with their operators (map_scene_tree_masked); but it has a fixed
    // price per evaluation (~250 cycles) that four leaves do not repay (8-node scene 0.44 -> 0.66 ms), and in the general loop, where
    // a skipped record is still fetched and decoded, it loses (the blended scene 4.0 -> 4.4): chains and trees of a dozen leaves or
    // more, and chains of blends (the wider interpreter: SmoothUnion is an extension) of kBlendPruneLeaves leaves or more.  The
    // scalar-cache variant (no LDS) has no unit records at hand.
    const bool lattice_units = d.unit_mode == RM_UNITS_LATTICE && d.n_leaves >= kPruneLeaves;
    const bool blend_units = d.unit_mode == RM_UNITS_BLEND && d.n_leaves >= kBlendPruneLeaves && lds;
    bool units;
    int loop;
    if (d.is_chain) {                             // 1 the chain loop, 2 over the records the mask names
        units = lattice_units;
        loop = units && lds ? 2 : 1;
    } else if (d.is_tree && !d.has_extensions) {  // 3 the tree loop, 4 over the tree records the mask leaves
        const bool tree_units = lds && !d.tree.empty();
        units = blend_units || (lattice_units && tree_units);
        loop = units && tree_units ? 4 : 3;
    } else {                                      // 0 the general record loop, 5 over the units of a blending chain
        units = blend_units;
        loop = units ? 5 : 0;
    }
    L.n_tree = loop == 4 ? (uint32_t)d.tree.size() : 0u;
    if (L.n_tree != 0u) L.spill_depth += 1u;  // (map_scene_tree_masked spills at every push)
    // bit 2: chain program, bit 4: tree program (every record one of the eight fast shapes)
    L.flags = (cull ? 1u : 0u) | (d.is_chain ? 4u : 0u) | (units ? 8u : 0u) | (d.is_tree ? 16u : 0u);
    // programs that blend: a ray the plain miss tests cannot clear (every bound is inflated by the blend radius) gets the
    // program run on lower bounds of its leaves along the ray
    if (cull && d.bound_walk) L.flags |= 32u;
    if (!cull) L.n_cone = L.n_slab = 0u;
    return V5Plan{units, loop};
}

template <int WPT>
int launch_v5_w(rm_ctx* c, const RmLaunch& L_in, bool lds, uint32_t n_frames, hipStream_t s) {
    RmLaunch L = L_in;
    const RmDecoded& d = c->decoded;
    const V5Plan plan = plan_v5(c, L, lds);
    const bool units = plan.units;
    const int loop = plan.loop;
    c->last_loop = loop;
    const uint32_t n_tiles = ((L.W + 7u) / 8u) * ((L.rows + 7u) / 8u);
    // structure-specialised kernel (values live in registers: no LDS spill stack)
    const bool range_proved = lds && range_facts_hold(c);
    hipFunction_t spec_fn = lds ? specialised_kernel(c, WPT, range_proved) : nullptr;
    if (spec_fn) { L.spill_depth = 0u; L.n_tree = 0u; }
    // the material evaluation of a tagged program borrows the spill area: (distance, index) pairs + saved positions
    // (a specialised kernel with the generated material walk keeps those pairs in registers too)
    if (L.n_mrec != 0u && !(spec_fn && c->spec && c->spec->material_walk))
        L.spill_depth = std::max(L.spill_depth, 2u * d.mat_spill_depth + 3u * d.mat_xform_depth);
    L.wave_dwords = rml::V5_WAVE_DWORDS - ((spec_fn && c->spec && c->spec->taps4 && L.n_mrec == 0u) ? rml::V5_TN_DWORDS : 0u);
    const size_t shmem = rml::MarchLds(WPT, L.wave_dwords, L.spill_depth, L.n_cone, L.n_slab, lds, L.n_rec, L.n_grp, L.n_tree, L.n_mrec != 0u).bytes;
    if (shmem > rml::kLdsLaunchLimit) return fail(c, RM_ERR_TOO_LARGE, "program needs %zu bytes of LDS per tile", shmem);
    // pre-pass buffers: cost + work list per tile, {count, cursor} per frame
    if (int rc = c->d_cost.reserve(c, (size_t)n_tiles * n_frames)) return rc;
    if (int rc = c->d_order.reserve(c, (size_t)n_tiles * n_frames)) return rc;
    if (int rc = c->d_masks.reserve(c, (size_t)n_tiles * n_frames)) return rc;
    if (int rc = c->d_counters.reserve(c, (size_t)n_frames * 4u)) return rc;
    hipLaunchKernelGGL(rmk::rm_tile_pre_v5, dim3((n_tiles + rmk::V5_PRE_BLOCK - 1u) / rmk::V5_PRE_BLOCK, 1, n_frames),
                       dim3(64u * rmk::V5_PRE_TILES), rml::CullLds(L.n_cone, L.n_slab, true).bytes, s, L, c->d_cost.p, c->d_masks.p, n_tiles);
    // RM_OPT_BALANCE = 3: the march kernel records how long every tile took; the next draw of the same shape
    // dispatches the longest first (consecutive frames of an interactive view or an orbit look alike)
    const uint32_t* prev = nullptr;
    uint32_t* measured = nullptr;
    if (c->balance == 3) {
        const size_t need = (size_t)n_tiles * n_frames;
        if (need > c->d_measured.cap) {
            if (int rc = c->d_measured.reserve(c, need)) return rc;
            c->measured_shape = 0;
        }
        const uint64_t shape = ((uint64_t)L.W << 40) ^ ((uint64_t)L.rows << 20) ^ ((uint64_t)L.strip_rows << 12) ^
                               ((uint64_t)L.strip_first << 6) ^ (uint64_t)L.strip_stride ^ ((uint64_t)n_frames << 52) ^ 1ull;
        if (c->measured_shape == shape) prev = c->d_measured.p;
        else HIP_TRY(c, hipMemsetAsync(c->d_measured.p, 0, need * sizeof(uint32_t), s));
        c->measured_shape = shape;
        measured = c->d_measured.p;
    }
    hipLaunchKernelGGL(rmk::rm_tile_sort_v5, dim3(n_frames), dim3(1024), 0, s, L, c->d_cost.p, c->d_order.p, c->d_counters.p,
                       n_tiles, (uint32_t)c->balance, prev);
    rmk::V5Work work{c->d_order.p, c->d_counters.p, measured, c->d_masks.p};
    // persistent grid: about as many workgroups as fit the chip (LDS, 32 waves per CU), never more than tiles
    uint32_t per_cu = (uint32_t)std::min<size_t>(32u / WPT, (160u * 1024u) / shmem);
    if (per_cu < 1u) per_cu = 1u;
    // ... but never more than 24 waves of ONE launch on a CU: where a seventh workgroup would fit (kernels of at most 72 vector
    // registers and 22.8 KB of LDS), a frame drawn alone is slower with it (a tile's four waves get a seventh of the CU instead of a
    // sixth, and the launch ends with its last tiles: -4 %), while the free slot lets the next frame's launch start on the same CU
    // (frames in flight +6 %).
    if (per_cu > 24u / WPT) per_cu = 24u / WPT;
    const uint32_t n_wg = std::min<uint32_t>(n_tiles, (uint32_t)std::max(1, c->cu_count) * per_cu);
    dim3 grid(n_wg, 1, n_frames);
    if (int rc = ensure_stats(c, L, (size_t)n_wg * n_frames * WPT)) return rc;
    if (int rc = time_begin(c, s)) return rc;
    // reference-only programs run the lean interpreter (chain and tree loops only); extension node types select the wider one,
    // which has the general record loop
    const bool ext = d.has_extensions || !d.is_tree;
    c->last_specialized = spec_fn != nullptr;
    c->last_range_proof = spec_fn != nullptr && range_proved;
    // When a wave takes new rays.  With far-primitive pruning every evaluation tests which primitives are near for ANY lane:
    // lanes at unrelated march depths (a lane refilled the moment it retires) keep most of them near, while 64 rays started
    // together stay in step -- far from everything at first, then close to one or two primitives each -- and the union shrinks
    // with them.  That is worth more than the lanes that idle until the last ray of the batch is done (metric frame 0.505 ->
    // 0.482 ms, 64-node scene +7 %; profiles/r02_refill_threshold_ab.txt); without pruning nothing is gained and the idle
    // lanes cost (8-node scene -17 %, the blended scene -2 %), so those kernels keep refilling lane by lane.
    const bool pruning = spec_fn ? (c->spec && c->spec_pruned != rmjit::PRUNE_NONE) : units && lds;
    const uint32_t refill_auto = c->refill_min_v5 != 0u ? c->refill_min_v5 : (pruning ? 64u : 1u);
    if (spec_fn) {
        uint32_t n_tiles_arg = n_tiles, refill = refill_auto;
        void* args[] = {&L, &work, &n_tiles_arg, &refill};
        hipError_t e = hipModuleLaunchKernel(spec_fn, grid.x, grid.y, grid.z, 64u * WPT, 1, 1, (unsigned)shmem, s, args, nullptr);
        if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "launch of the specialised kernel failed: %s", hipGetErrorString(e));
    } else if (lds && !ext) {  // one lean kernel per record loop (1 .. 4 here)
        switch (loop) {
        case 1: hipLaunchKernelGGL((rmk::rm_render_v5_lean<WPT, 1>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto); break;
        case 2: hipLaunchKernelGGL((rmk::rm_render_v5_lean<WPT, 2>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto); break;
        case 3: hipLaunchKernelGGL((rmk::rm_render_v5_lean<WPT, 3>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto); break;
        default: hipLaunchKernelGGL((rmk::rm_render_v5_lean<WPT, 4>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto); break;
        }
    }
    else if (lds)
        hipLaunchKernelGGL((rmk::rm_render_v5<rmk::ProgLds, true, WPT, true>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto);
    else if (!ext)
        hipLaunchKernelGGL((rmk::rm_render_v5<rmk::ProgSmem, false, WPT, false>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto);
    else
        hipLaunchKernelGGL((rmk::rm_render_v5<rmk::ProgSmem, false, WPT, true>), grid, dim3(64 * WPT), shmem, s, L, work, n_tiles, refill_auto);
    if (int rc = time_end(c, s)) return rc;
    return finish_launch(c);
}

int launch_v5(rm_ctx* c, const RmLaunch& L, bool lds, uint32_t n_frames, hipStream_t s) {
    // Waves per tile.  A march launch lasts at least as long as its heaviest tile (1024 rays through one workgroup); four waves
    // per tile give the best throughput when there are tiles to fill the chip with, eight halve that latency and win once a
    // launch has fewer tiles than the chip has room for -- one GPU's share of a frame tiled over eight (DESIGN.md section 7:
    // 144 rows of 1080p: 0.095 -> 0.084 ms per frame; the whole frame: 0.546 -> 0.613).
    const size_t launch_tiles = (size_t)((L.W + 7u) / 8u) * ((L.rows + 7u) / 8u) * n_frames;
    const int wpt = c->waves_per_tile != 0 ? c->waves_per_tile : (launch_tiles <= 6000u ? 8 : 4);
    // A long program (rm_resize_command_buffer admits 64 KB of commands, ~2 700 leaves = 85 KB of records) does not fit
    // a workgroup's LDS next to the ray buffers: it is then read through the scalar cache instead (ProgSmem).
    const RmDecoded& d = c->decoded;
    const rml::MarchChoice m = rml::choose_march(lds, (uint32_t)wpt, L.spill_depth, L.n_mrec != 0u ? 2u * d.mat_spill_depth + 3u * d.mat_xform_depth : 0u,
                                                 L.n_mrec != 0u, L.n_cone, L.n_slab, L.n_rec, L.n_grp, (uint32_t)d.tree.size());
    switch (m.wpt) {
    case 1: return launch_v5_w<1>(c, L, m.prog_in_lds, n_frames, s);
    case 2: return launch_v5_w<2>(c, L, m.prog_in_lds, n_frames, s);
    case 8: return launch_v5_w<8>(c, L, m.prog_in_lds, n_frames, s);
    default: return launch_v5_w<4>(c, L, m.prog_in_lds, n_frames, s);
    }
}

struct StripSpec { uint32_t rows = 0, first = 0, stride = 0; };

// The launch of the context's current program, limits, uniforms and output format for a W x H frame (rows [row0, row0 + rows),
// or strips): everything but what the kernel variant decides (plan_v5).
RmLaunch fill_launch(rm_ctx* c, const rm_uniforms* frames_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, float* d_out,
                     StripSpec strips) {
    RmLaunch L;
    L.strip_rows = strips.rows; L.strip_first = strips.first; L.strip_stride = strips.stride;
    L.prog = c->d_prog.p;
    L.n_rec = (uint32_t)c->decoded.rec.size();
    L.n_grp = (uint32_t)c->decoded.units.size();
    L.n_tree = 0u;  // (set by launch_v5_w when the interpreter runs the masked tree loop)
    L.unit_mode = c->decoded.unit_mode;
    L.unit_kmax = c->decoded.unit_kmax;
    L.value_spill_depth = c->decoded.spill_depth;
    L.spill_depth = c->decoded.spill_depth + 3u * c->decoded.xform_depth;  // saved positions follow the value stack
    L.bounds = c->decoded.has_xforms ? c->d_bounds.p : nullptr;
    L.mprog = c->d_mprog.p;
    L.n_mrec = (uint32_t)c->decoded.mrec.size();
    L.mat_value_depth = c->decoded.mat_spill_depth;
    L.materials = c->d_materials.p;
    L.n_cull = 0;
    L.flags = 0;
    L.n_cone = c->decoded.n_sphere;
    L.n_slab = c->decoded.n_box;
    L.smooth_slack = (float)c->decoded.smooth_slack;
    L.scene_scale = c->decoded.scene_scale;
    L.min_dist = c->limits.min_dist;
    L.max_dist = c->limits.max_dist;
    L.max_iter = c->limits.max_iter;
    L.W = W; L.H = H; L.row0 = row0; L.rows = rows;
    L.out = d_out;
    L.out_format = (uint32_t)c->out_format;
    L.frames = frames_dev;
    L.order = nullptr;
    L.stats = nullptr;
    L.u = c->uniforms;
    return L;
}

int launch(rm_ctx* c, const rm_uniforms* frames_dev, uint32_t n_frames, uint32_t W, uint32_t H, uint32_t row0,
           uint32_t rows, float* d_out, hipStream_t s, StripSpec strips = StripSpec()) {
    RmLaunch L = fill_launch(c, frames_dev, W, H, row0, rows, d_out, strips);
    if (c->out_format != RM_FORMAT_RGBA32F && !(c->kernel == RM_KERNEL_DEFAULT || c->kernel == RM_KERNEL_V5 || c->kernel == RM_KERNEL_V5_LDS))
        return fail(c, RM_ERR_ARG, "kernel variant %d writes RGBA32F only (8-bit output formats need the default kernels)", c->kernel);
    int kernel = c->kernel == RM_KERNEL_DEFAULT ? RM_KERNEL_V5_LDS : c->kernel;
    if (kernel == RM_KERNEL_V5 || kernel == RM_KERNEL_V5_LDS) return launch_v5(c, L, kernel == RM_KERNEL_V5_LDS, n_frames, s);
    if (kernel != RM_KERNEL_PIXEL) return fail(c, RM_ERR_ARG, "kernel variant %d is not available", kernel);
    // v1: north_star's literal design (one thread per pixel, program staged in LDS, lock-step loops); reference node types only
    if (c->decoded.has_extensions)
        return fail(c, RM_ERR_ARG, "kernel variant %d renders reference node types only (program uses extension nodes)", kernel);
    if (int rc = time_begin(c, s)) return rc;
    {
        dim3 grid((W + 15u) / 16u, (rows + 15u) / 16u, n_frames);
        const size_t shmem = rml::PixelLds(L.n_rec, L.spill_depth).bytes;
        if (shmem > rml::kLdsLaunchLimit) return fail(c, RM_ERR_TOO_LARGE, "program needs %zu bytes of LDS per workgroup", shmem);
        hipLaunchKernelGGL(rmk::rm_render_pixel, grid, dim3(256), shmem, s, L);
    }
    if (int rc = time_end(c, s)) return rc;
    return finish_launch(c);
}

int ensure_stats(rm_ctx* c, RmLaunch& L, size_t n_waves) {
    if (!c->wave_stats) return RM_OK;
    if (int rc = c->d_stats.reserve(c, n_waves * 4u)) return rc;
    c->stats_valid_bytes = n_waves * 4u * sizeof(unsigned long long);
    L.stats = c->d_stats.p;
    return RM_OK;
}

int time_begin(rm_ctx* c, hipStream_t s) {
    if (!c->timing) return RM_OK;
    if (c->tev_used == c->tev.size()) {
        if (c->tev.size() >= 4096) return RM_OK;  // stop recording, keep running
        hipEvent_t a, b;
        HIP_TRY(c, hipEventCreate(&a));
        HIP_TRY(c, hipEventCreate(&b));
        c->tev.emplace_back(a, b);
    }
    HIP_TRY(c, hipEventRecord(c->tev[c->tev_used].first, s));
    return RM_OK;
}
int time_end(rm_ctx* c, hipStream_t s) {
    if (!c->timing || c->tev_used >= c->tev.size()) return RM_OK;
    HIP_TRY(c, hipEventRecord(c->tev[c->tev_used].second, s));
    c->tev_used++;
    return RM_OK;
}

int finish_launch(rm_ctx* c) {
    HIP_TRY(c, hipGetLastError());
    return RM_OK;
}

int check_dims(rm_ctx* c, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows) {
    if (W == 0 || H == 0 || W > kMaxDim || H > kMaxDim) return fail(c, RM_ERR_RANGE, "image size %ux%u out of range", W, H);
    if (rows == 0 || row0 >= H || rows > H - row0)
        return fail(c, RM_ERR_RANGE, "row band [%u,+%u) outside image height %u", row0, rows, H);
    return RM_OK;
}

// A draw with an astronomically large max_iter would never finish (an empty scene marches all
// max_iter steps, wgsl:189-191 + :109); refuse it instead of hanging the GPU.
int check_limits(rm_ctx* c) {
    if (c->limits.max_iter > kMaxIter)
        return fail(c, RM_ERR_RANGE, "max_iter %u exceeds the supported maximum %u", c->limits.max_iter, kMaxIter);
    return RM_OK;
}

hipStream_t user_stream(const rm_ctx* c, void* stream) {
    return stream == RM_STREAM_OWN ? c->stream : static_cast<hipStream_t>(stream);
}

// See rm_ctx::last_stream.  Nothing is issued while consecutive draws stay on one stream (the steady state, and the
// only state during stream capture).  A previous stream that no longer exists, or that is still being captured (its
// draws have not run and cannot race), makes the record fail: there is nothing to wait for then.
void order_with_previous(rm_ctx* c, hipStream_t s) {
    if (c->last_stream_valid && c->last_stream != s) {
        // a stream that is being captured cannot wait for work outside its graph (the attempt would invalidate the capture):
        // capture a draw on the stream the context drew on last
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &capturing) != hipSuccess) (void)hipGetLastError();
        if (capturing != hipStreamCaptureStatusNone) {
            c->last_stream = s;
            return;
        }
        // The PREVIOUS stream may be the one that is capturing (capture begun on A, a draw captured there, and now -- before
        // the capture ends -- a draw on another stream B): an event recorded on A would become a node of A's graph, and B's
        // wait on it would pull B into that capture (or fail with a capture-isolation error, invalidating it).  Captured work
        // has not run and cannot race with this draw: nothing to wait for.
        hipStreamCaptureStatus prev_capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c->last_stream, &prev_capturing) != hipSuccess) {
            (void)hipGetLastError();  // the previous stream no longer exists
            prev_capturing = hipStreamCaptureStatusActive;
        }
        if (prev_capturing == hipStreamCaptureStatusNone) {
            if (hipEventRecord(c->ev_order, c->last_stream) == hipSuccess) {
                if (hipStreamWaitEvent(s, c->ev_order, 0) != hipSuccess) (void)hipGetLastError();
            } else {
                (void)hipGetLastError();
            }
        }
    }
    c->last_stream = s;
    c->last_stream_valid = true;
}

size_t pixel_bytes(const rm_ctx* c) { return c->out_format == RM_FORMAT_RGBA32F ? 16u : 4u; }

// The stream an entry point works on: results for host memory are staged and copied on the context's own stream.
hipStream_t dest_stream(const rm_ctx* c, int is_device, void* stream) { return is_device ? user_stream(c, stream) : c->stream; }

// The outputs of an entry point whose destination is device memory (the kernel writes the caller's arrays, asynchronously on
// the caller's stream) or host memory: then the kernel writes one of the context's staging buffers -- d_out for the draws,
// d_qout for the queries (never the draws' scratch) --, and finish() copies every output back and waits for the stream.  add()
// the outputs, reserve(), launch with dev(i), finish().  An output the caller passed as NULL stays NULL for the kernel.
struct Outputs {
    rm_ctx* c;
    bool to_host;
    DevBuf<char>& staging;
    struct Out { void* user; size_t offset, bytes; } out[4] = {};
    int n = 0;
    size_t total = 0;
    Outputs(rm_ctx* c, int is_device, DevBuf<char>& staging) : c(c), to_host(!is_device), staging(staging) {}
    void add(void* user, size_t bytes) {
        assert(n < 4);
        out[n++] = Out{user, total, bytes};
        if (user) total += rml::align16(bytes);
    }
    int reserve() { return to_host ? staging.reserve(c, total) : RM_OK; }
    template <class T>
    T* dev(int i) const { return static_cast<T*>(to_host && out[i].user ? staging.p + out[i].offset : out[i].user); }
    int finish(hipStream_t s) const {
        if (!to_host) return RM_OK;
        for (int i = 0; i < n; i++)
            if (out[i].user) HIP_TRY(c, hipMemcpyAsync(out[i].user, staging.p + out[i].offset, out[i].bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        return RM_OK;
    }
};

// What rm_draw, rm_draw_strips and rm_draw_batch do before they launch, on the stream *s they draw on.
int draw_begin(rm_ctx* c, int out_is_device, void* stream, hipStream_t* s) {
    HIP_TRY(c, hipSetDevice(c->device));
    *s = dest_stream(c, out_is_device, stream);
    order_with_previous(c, *s);
    int rc = ensure_program(c, *s);
    if (rc == RM_OK) rc = ensure_materials(c, *s);
    if (rc == RM_OK) rc = check_limits(c);
    return rc;
}

// ... and after: the launch into the caller's device memory, or into d_out and from there to the caller's host memory.
int draw_launch(rm_ctx* c, const rm_uniforms* frames_dev, uint32_t n_frames, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                float* out_rgba, int out_is_device, hipStream_t s, StripSpec strips = StripSpec()) {
    Outputs o(c, out_is_device, c->d_out);
    o.add(out_rgba, (size_t)n_frames * rows * W * pixel_bytes(c));
    int rc = o.reserve();
    if (rc == RM_OK) rc = launch(c, frames_dev, n_frames, W, H, row0, rows, o.dev<float>(0), s, strips);
    return rc == RM_OK ? o.finish(s) : rc;
}

int check_strips(rm_ctx* c, const char* fn, uint32_t strip_rows, uint32_t first, uint32_t stride) {
    if (strip_rows == 0u || (strip_rows % 8u) != 0u || stride == 0u || first >= stride)
        return fail(c, RM_ERR_ARG, "%s: strip_rows %u must be a positive multiple of 8, first %u < stride %u", fn, strip_rows, first, stride);
    return RM_OK;
}

}  // namespace

RM_EXPORT int rm_abi_version(void) { return RM_ABI_VERSION; }

RM_EXPORT int rm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

RM_EXPORT int rm_create(int device, rm_ctx** out) {
    if (!out) return fail(nullptr, RM_ERR_NULL, "rm_create: out is NULL");
    *out = nullptr;
    int n = rm_device_count();
    if (n <= 0) return fail(nullptr, RM_ERR_NO_DEVICE, "rm_create: no HIP device is visible");
    if (device < 0 || device >= n) return fail(nullptr, RM_ERR_ARG, "rm_create: device %d not in [0,%d)", device, n);
    rm_ctx* c = new (std::nothrow) rm_ctx();
    if (!c) return fail(nullptr, RM_ERR_DEVICE, "rm_create: out of host memory");
    c->device = device;
    c->cmd.assign(kRefCmdBufferBytes / 4, 0u);
    hipError_t e = hipSetDevice(device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) {
        c->cu_count = prop.multiProcessorCount;
        c->max_lds = prop.sharedMemPerBlock;
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    }
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming);
    if (e != hipSuccess) {
        int rc = fail(nullptr, RM_ERR_DEVICE, "rm_create: HIP initialisation failed: %s", hipGetErrorString(e));
        rm_destroy(c);
        return rc;
    }
    *out = c;
    return RM_OK;
}

RM_EXPORT void rm_destroy(rm_ctx* c) {
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& st : c->staging) {
        if (st.host) (void)hipHostFree(st.host);
        if (st.done) (void)hipEventDestroy(st.done);
    }
    for (auto& e : c->tev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    // the device buffers go with the context, after the stream on purpose: it was synchronised above, hipFree waits for the
    // device, and no buffer refers to the stream or to an event
    delete c;
}

RM_EXPORT int rm_write_buffer(rm_ctx* c, int buffer, uint64_t offset, const void* data, uint64_t size) {
    if (!c) return RM_ERR_NULL;
    if (!data && size) return fail(c, RM_ERR_NULL, "rm_write_buffer: data is NULL");
    if ((offset & 3u) || (size & 3u))
        return fail(c, RM_ERR_ARG, "rm_write_buffer: offset %llu / size %llu not multiples of 4",
                    (unsigned long long)offset, (unsigned long long)size);
    uint8_t* dst = nullptr;
    uint64_t cap = 0;
    switch (buffer) {
    case RM_BUF_LIMITS: dst = reinterpret_cast<uint8_t*>(&c->limits); cap = sizeof(rm_limits); break;
    case RM_BUF_COMMANDS: dst = reinterpret_cast<uint8_t*>(c->cmd.data()); cap = c->cmd.size() * 4; break;
    case RM_BUF_UNIFORMS: dst = reinterpret_cast<uint8_t*>(&c->uniforms); cap = sizeof(rm_uniforms); break;
    default: return fail(c, RM_ERR_ARG, "rm_write_buffer: unknown buffer %d", buffer);
    }
    if (offset > cap || size > cap - offset)
        return fail(c, RM_ERR_TOO_LARGE, "rm_write_buffer: [%llu,+%llu) exceeds the %llu-byte buffer %d",
                    (unsigned long long)offset, (unsigned long long)size, (unsigned long long)cap, buffer);
    if (buffer == RM_BUF_COMMANDS && size && std::memcmp(dst + offset, data, size) != 0) c->cmd_dirty = true;
    if (size) std::memcpy(dst + offset, data, size);
    return RM_OK;
}

RM_EXPORT int rm_set_uniforms(rm_ctx* c, const rm_uniforms* u) {
    if (!c) return RM_ERR_NULL;
    if (!u) return fail(c, RM_ERR_NULL, "rm_set_uniforms: u is NULL");
    return rm_write_buffer(c, RM_BUF_UNIFORMS, 0, u, sizeof *u);
}

RM_EXPORT int rm_set_limits(rm_ctx* c, const rm_limits* l) {
    if (!c) return RM_ERR_NULL;
    if (!l) return fail(c, RM_ERR_NULL, "rm_set_limits: l is NULL");
    return rm_write_buffer(c, RM_BUF_LIMITS, 0, l, sizeof *l);
}

RM_EXPORT int rm_set_program(rm_ctx* c, uint32_t cmd_count, const uint32_t* words, uint32_t n_words) {
    if (!c) return RM_ERR_NULL;
    if (n_words && !words) return fail(c, RM_ERR_NULL, "rm_set_program: words is NULL");
    const uint64_t cap_words = c->cmd.size() - 1;
    if (n_words > cap_words)
        return fail(c, RM_ERR_TOO_LARGE, "rm_set_program: %u words do not fit the %llu-byte command buffer "
                    "(rm_resize_command_buffer lifts the reference's 1024-byte limit)",
                    n_words, (unsigned long long)(c->cmd.size() * 4));
    // The reference rebuilds and rewrites the command buffer every frame (renderer.rs:224-239); a rewrite that leaves
    // the buffer as it is keeps the decoded program and its device copy.
    if (!c->cmd_dirty && c->cmd_status == RM_OK && c->cmd[0] == cmd_count &&
        (n_words == 0u || std::memcmp(c->cmd.data() + 1, words, (size_t)n_words * 4) == 0))
        return RM_OK;
    RmDecoded d;
    int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc != RM_OK) return fail(c, rc, "rm_set_program: %s", rm_status_string(rc));
    c->cmd[0] = cmd_count;                                               // renderer.rs:230-234
    if (n_words) std::memcpy(c->cmd.data() + 1, words, (size_t)n_words * 4);  // renderer.rs:235-239
    c->cmd_dirty = true;
    return RM_OK;
}

RM_EXPORT int rm_set_materials(rm_ctx* c, uint32_t count, const float* rgb) {
    if (!c) return RM_ERR_NULL;
    if (!rgb) return fail(c, RM_ERR_NULL, "rm_set_materials: rgb is NULL");
    if (count < 1u || count > RM_MAX_MATERIALS)
        return fail(c, RM_ERR_MATERIAL, "rm_set_materials: %u entries, the table holds 1 to %u", count, (unsigned)RM_MAX_MATERIALS);
    c->materials.resize(count);
    for (uint32_t i = 0; i < count; i++) c->materials[i] = make_float4(rgb[3u * i], rgb[3u * i + 1u], rgb[3u * i + 2u], 0.0f);
    c->materials_dirty = true;
    return RM_OK;
}

RM_EXPORT int rm_resize_command_buffer(rm_ctx* c, uint64_t bytes) {
    if (!c) return RM_ERR_NULL;
    if (bytes < kRefCmdBufferBytes || bytes > kMaxCmdBufferBytes || (bytes & 3u))
        return fail(c, RM_ERR_ARG, "rm_resize_command_buffer: %llu not a multiple of 4 in [1024, 65536]",
                    (unsigned long long)bytes);
    c->cmd.resize(bytes / 4, 0u);
    c->cmd_dirty = true;
    return RM_OK;
}

RM_EXPORT int rm_validate(rm_ctx* c) {
    if (!c) return RM_ERR_NULL;
    RmDecoded d;
    int rc = rm_decode_program(c->cmd[0], c->cmd.data() + 1, (uint32_t)c->cmd.size() - 1u, &d);
    if (rc != RM_OK) return fail(c, rc, "invalid CSG program in command buffer: %s", rm_status_string(rc));
    return RM_OK;
}

RM_EXPORT int rm_validate_program(uint32_t cmd_count, const uint32_t* words, uint32_t n_words,
                                  uint32_t* out_max_depth) {
    RmDecoded d;
    int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc == RM_OK && out_max_depth) *out_max_depth = d.max_depth;
    return rc;
}

RM_EXPORT int rm_program_info(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, uint32_t* out, uint32_t n_out) {
    RmDecoded d;
    int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc != RM_OK) return rc;
    uint32_t subtracted = 0u;
    for (const RmRecord& r : d.rec) subtracted += (r.op & RM_OP_NOCULL) != 0u;
    const uint32_t facts[RM_PROGRAM_FACTS] = {(uint32_t)d.rec.size(), d.n_sphere, d.n_box, subtracted, (uint32_t)d.units.size(), d.spill_depth,
                                              d.is_chain ? 1u : 0u, d.prunable ? 1u : 0u, d.bound_walk ? 1u : 0u, d.has_xforms ? 1u : 0u,
                                              d.n_leaves, (uint32_t)prune_kind(d, 2)};
    for (uint32_t i = 0; out && i < n_out && i < (uint32_t)RM_PROGRAM_FACTS; i++) out[i] = facts[i];
    return RM_OK;
}

RM_EXPORT int rm_draw(rm_ctx* c, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, float* out_rgba,
                      int out_is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_rgba) return fail(c, RM_ERR_NULL, "rm_draw: out_rgba is NULL");
    int rc = check_dims(c, W, H, row0, rows);
    if (rc != RM_OK) return rc;
    hipStream_t s;
    if ((rc = draw_begin(c, out_is_device, stream, &s)) != RM_OK) return rc;
    return draw_launch(c, nullptr, 1, W, H, row0, rows, out_rgba, out_is_device, s);
}

RM_EXPORT int rm_draw_strips(rm_ctx* c, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t first, uint32_t stride,
                             float* out_rgba, int out_is_device, void* stream, uint32_t* out_rows) {
    if (!c) return RM_ERR_NULL;
    if (!out_rows) return fail(c, RM_ERR_NULL, "rm_draw_strips: out_rows is NULL");
    int rc = check_dims(c, W, H, 0, H);
    if (rc != RM_OK) return rc;
    if ((rc = check_strips(c, "rm_draw_strips", strip_rows, first, stride)) != RM_OK) return rc;
    const uint32_t rows = rml::strip_row_count(H, strip_rows, first, stride);
    *out_rows = rows;
    if (rows == 0u) return RM_OK;  // more ranks than strips: nothing to do for this one
    if (!out_rgba) return fail(c, RM_ERR_NULL, "rm_draw_strips: out_rgba is NULL");
    hipStream_t s;
    if ((rc = draw_begin(c, out_is_device, stream, &s)) != RM_OK) return rc;
    StripSpec sp;
    sp.rows = strip_rows; sp.first = first; sp.stride = stride;
    return draw_launch(c, nullptr, 1, W, H, 0, rows, out_rgba, out_is_device, s, sp);
}

// The final host-side gather of a tiled frame (north-star): this GPU's strips go from the compact device
// buffer rm_draw_strips filled to their rows of the full H-row host image, one D2H copy per strip on `stream`.
RM_EXPORT int rm_gather_strips(rm_ctx* c, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t first, uint32_t stride,
                               const void* strips_device, void* host_image, void* stream) {
    if (!c) return RM_ERR_NULL;
    int rc = check_dims(c, W, H, 0, H);
    if (rc != RM_OK) return rc;
    if ((rc = check_strips(c, "rm_gather_strips", strip_rows, first, stride)) != RM_OK) return rc;
    const uint32_t n_strips = (H + strip_rows - 1u) / strip_rows;
    if (first >= n_strips) return RM_OK;  // this GPU has no strip
    if (!strips_device || !host_image) return fail(c, RM_ERR_NULL, "rm_gather_strips: NULL buffer");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = user_stream(c, stream);
    const size_t row_bytes = (size_t)W * pixel_bytes(c);
    const uint8_t* src = static_cast<const uint8_t*>(strips_device);
    uint8_t* dst = static_cast<uint8_t*>(host_image);
    if (stride == 1u) {  // one GPU: the compact buffer IS the frame
        HIP_TRY(c, hipMemcpyAsync(dst, src, row_bytes * H, hipMemcpyDeviceToHost, s));
        return RM_OK;
    }
    // This GPU's strips are equally spaced in the frame: all the full ones go in ONE pitched copy (a row of the copy = one
    // strip, destination pitch = `stride` strips), a ragged last strip in a second one.
    const size_t strip_bytes = row_bytes * strip_rows;
    uint32_t n_mine = 0, n_full = 0;
    for (uint32_t sidx = first; sidx < n_strips; sidx += stride) {
        n_mine++;
        if ((sidx + 1u) * strip_rows <= H) n_full++;
    }
    if (n_full >= 2u) {
        HIP_TRY(c, hipMemcpy2DAsync(dst + strip_bytes * first, strip_bytes * stride, src, strip_bytes, strip_bytes, n_full,
                                    hipMemcpyDeviceToHost, s));
        if (n_mine > n_full) {  // the frame's last strip is this GPU's and is shorter
            const uint32_t sidx = first + n_full * stride, r0 = sidx * strip_rows;
            HIP_TRY(c, hipMemcpyAsync(dst + row_bytes * r0, src + strip_bytes * n_full, row_bytes * (H - r0), hipMemcpyDeviceToHost, s));
        }
        return RM_OK;
    }
    for (uint32_t sidx = first; sidx < n_strips; sidx += stride) {
        const uint32_t r0 = sidx * strip_rows, rows = H - r0 < strip_rows ? H - r0 : strip_rows;
        HIP_TRY(c, hipMemcpyAsync(dst + row_bytes * r0, src, row_bytes * rows, hipMemcpyDeviceToHost, s));
        src += row_bytes * rows;
    }
    return RM_OK;
}

RM_EXPORT int rm_host_register(void* ptr, uint64_t bytes) {
    if (!ptr || !bytes) return RM_ERR_NULL;
    if (hipHostRegister(ptr, bytes, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        return RM_ERR_DEVICE;
    }
    return RM_OK;
}

RM_EXPORT int rm_host_unregister(void* ptr) {
    if (!ptr) return RM_ERR_NULL;
    if (hipHostUnregister(ptr) != hipSuccess) {
        (void)hipGetLastError();
        return RM_ERR_DEVICE;
    }
    return RM_OK;
}

RM_EXPORT int rm_draw_batch(rm_ctx* c, const rm_uniforms* frames, uint32_t n_frames, uint32_t W, uint32_t H,
                            float* out_rgba, int out_is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_rgba || !frames) return fail(c, RM_ERR_NULL, "rm_draw_batch: NULL argument");
    if (n_frames == 0 || n_frames > 65535u) return fail(c, RM_ERR_RANGE, "rm_draw_batch: n_frames %u not in [1,65535]", n_frames);
    int rc = check_dims(c, W, H, 0, H);
    if (rc != RM_OK) return rc;
    hipStream_t s;
    if ((rc = draw_begin(c, out_is_device, stream, &s)) != RM_OK) return rc;
    if ((rc = c->d_frames.reserve(c, n_frames)) != RM_OK) return rc;
    rc = upload(c, c->d_frames.p, frames, (size_t)n_frames * sizeof(rm_uniforms), s);
    if (rc != RM_OK) return rc;
    return draw_launch(c, c->d_frames.p, n_frames, W, H, 0, H, out_rgba, out_is_device, s);
}

// ---- scene queries (rm_query.h) -----------------------------------------------------------------------------------------
namespace {

// The record loop the interpreter draw runs the current program with (launch_v5_w without wave-level culling).
int query_loop(const RmDecoded& d) {
    if (d.is_chain) return rmk::Q_LOOP_CHAIN;
    if (d.is_tree && !d.has_extensions) return rmk::Q_LOOP_TREE;
    return rmk::Q_LOOP_GENERAL;
}

// A record loop as a compile-time constant: f(std::integral_constant<int, LOOP>) for the run-time `loop`, so that every kernel
// template with a LOOP parameter is chosen in one place.
template <class F>
auto with_loop(int loop, F&& f) {
    if (loop == rmk::Q_LOOP_CHAIN) return f(std::integral_constant<int, rmk::Q_LOOP_CHAIN>());
    if (loop == rmk::Q_LOOP_TREE) return f(std::integral_constant<int, rmk::Q_LOOP_TREE>());
    return f(std::integral_constant<int, rmk::Q_LOOP_GENERAL>());
}

// Device arrays of a query are read and written with vector accesses of their element size: floats 4 B, the (leaf, material)
// pairs of rm_query_points 8 B, the hit records and id quadruples of rm_cast_rays 16 B.  A pointer off that alignment is refused.
bool misaligned(const void* p, uintptr_t align) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (align - 1u)) != 0u; }

// The one read path of the retained results: what every rm_read_* ends in once its own refusals are past.  A device
// destination off an item's alignment is refused with the family's message; then the copies go out on the destination's
// stream, ordered after the context's earlier work (the family's next producing call waits for this stream in turn) -- one per
// item the caller wants (out) that holds anything (bytes) --, and a host destination waits for them.
struct ReadItem {
    void* out;
    const void* src;
    size_t bytes;
    uintptr_t align;
    ReadItem(void* out_, const void* src_, size_t bytes_, uintptr_t align_) : out(out_), src(src_), bytes(bytes_), align(align_) {}
    template <class T>  // a region of the buffer at `base`
    ReadItem(void* out_, const rml::Region<T>& r, const void* base, uintptr_t align_) : ReadItem(out_, r.at(base), r.bytes, align_) {}
};
int read_back(rm_ctx* c, int is_device, void* stream, const char* misaligned_message, std::initializer_list<ReadItem> items) {
    for (const ReadItem& it : items)
        if (is_device && misaligned(it.out, it.align)) return fail(c, RM_ERR_ARG, "%s", misaligned_message);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    order_with_previous(c, s);
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (const ReadItem& it : items)
        if (it.out && it.bytes) HIP_TRY(c, hipMemcpyAsync(it.out, it.src, it.bytes, kind, s));
    if (!is_device) HIP_TRY(c, hipStreamSynchronize(s));
    return RM_OK;
}

// LDS dwords per lane of a wave's column: what the distance loop needs (value stack, then 3 floats per transform level) and,
// with the leaf walk, the larger of that and the walk's ([depth] distances, [depth] pairs, 3 floats per transform level).
uint32_t query_slots(const RmDecoded& d, int loop, bool walk) {
    uint32_t slots = loop == rmk::Q_LOOP_CHAIN ? 0u : loop == rmk::Q_LOOP_TREE ? d.spill_depth : d.spill_depth + 3u * d.xform_depth;
    if (walk) slots = std::max(slots, 2u * d.q_spill_depth + 3u * d.q_xform_depth);
    return slots;
}

// A kernel template over the record loop alone, as QueryCall::launch chooses it.
#define RM_BY_LOOP(kernel) [](auto tag) { return rmk::kernel<decltype(tag)::value>; }

// As many 256-thread workgroups as give `items` one lane each.
uint32_t query_blocks(uint64_t items) { return (uint32_t)((items + 255u) / 256u); }

// The launch state of a call that runs query kernels of the program on one stream: what the kernels take (Q), the record loop
// they are instantiated for and their LDS columns (rml::QueryLds: four wave columns of Q.slots dwords per lane).
struct QueryCall {
    rm_ctx* c = nullptr;
    hipStream_t s = nullptr;
    rmk::QueryLaunch Q;
    int loop = 0;
    rml::QueryLds lds{0u, 0u};

    // What every query does first, on stream `s`, exactly as a draw would: ordering with the context's earlier work and the
    // program (decoded, validated and uploaded by ensure_program).  A call that has to see the program before it knows
    // whether the leaf walk runs takes this step by itself and begin_columns after it.
    int begin_program(rm_ctx* ctx, hipStream_t stream) {
        c = ctx;
        s = stream;
        order_with_previous(c, s);
        return ensure_program(c, s);
    }
    // Then the limits and -- for colours of a tagged program -- the material table, the query program, the launch and the
    // columns of one workgroup: the larger of what the distance loop and, with `walk`, the leaf walk need for THIS program
    // (query_slots).
    int begin_columns(bool walk, bool rgb) {
        int rc = rgb ? ensure_materials(c, s) : RM_OK;
        if (rc == RM_OK) rc = check_limits(c);
        if (rc != RM_OK) return rc;
        const RmDecoded& d = c->decoded;
        // the query program of this decoding, stream-ordered like the draws' images (a query still queued on an earlier stream
        // keeps the previous one: order_with_previous made this stream wait for it)
        if (c->qprog_gen != c->prog_gen) {
            if (d.qrec.size() > c->d_qprog.cap)
                if ((rc = c->d_qprog.reserve(c, std::max<size_t>(64, d.qrec.size() * 2), "query program")) != RM_OK) return rc;
            if (!d.qrec.empty())
                if (int urc = upload(c, c->d_qprog.p, d.qrec.data(), d.qrec.size() * sizeof(RmRecord), s)) return urc;
            c->qprog_gen = c->prog_gen;
        }
        loop = query_loop(d);
        lds = rml::QueryLds(query_slots(d, loop, walk), 0u);
        if (!fits(0u)) return fail(c, RM_ERR_TOO_LARGE, "the query needs %zu bytes of LDS per workgroup", (size_t)lds.bytes);
        Q.prog = c->d_prog.p;
        Q.qprog = c->d_qprog.p;
        Q.n_rec = (uint32_t)d.rec.size();
        Q.n_qrec = (uint32_t)d.qrec.size();
        Q.value_spill_depth = d.spill_depth;
        Q.q_value_depth = d.q_spill_depth;
        Q.slots = lds.slots;
        Q.tagged = d.has_materials ? 1u : 0u;
        Q.min_dist = c->limits.min_dist;
        Q.max_dist = c->limits.max_dist;
        Q.max_iter = c->limits.max_iter;
        Q.materials = rgb && d.has_materials ? c->d_materials.p : nullptr;
        return RM_OK;
    }
    int begin(rm_ctx* ctx, hipStream_t stream, bool walk, bool rgb) {
        const int rc = begin_program(ctx, stream);
        return rc == RM_OK ? begin_columns(walk, rgb) : rc;
    }

    // Whether a workgroup of a kernel with `own` bytes of static LDS fits what the device gives one (gfx950: up to 160 KB).
    bool fits(uint32_t own) const { return lds.behind(own).fits(std::max<size_t>(c->max_lds, rml::kLdsLaunchLimit)); }
    // The same call with columns of other `slots` (a second pass over the program with or without the leaf walk).
    QueryCall with_slots(uint32_t slots) const {
        QueryCall q = *this;
        q.lds = rml::QueryLds(slots, lds.own);
        q.Q.slots = slots;
        return q;
    }

    // `blocks` 256-thread workgroups of the kernel that choose(std::integral_constant<int, LOOP>) gives for this call's loop,
    // on (Q, args...), with the columns behind the kernel's `own` bytes of static LDS.
    template <class F, class... Args>
    int launch(F&& choose, uint32_t blocks, uint32_t own, Args... args) const {
        const auto kernel = with_loop(loop, choose);
        const rml::QueryLds L = lds.behind(own);
        if (L.needs_opt_in())  // (deep programs)
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.dynamic));
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), L.dynamic, s, Q, args...);
        HIP_TRY(c, hipGetLastError());
        return RM_OK;
    }
};

// The kernels that are chosen by more than the loop: each gives QueryCall::launch its chooser.
auto points_kernel(bool dist, bool normal, bool ids) {
    return [=](auto tag) {
        constexpr int LOOP = decltype(tag)::value;
        switch ((dist ? 1 : 0) | (normal ? 2 : 0) | (ids ? 4 : 0)) {
        case 1: return rmk::rm_query_points_kernel<LOOP, true, false, false>;
        case 2: return rmk::rm_query_points_kernel<LOOP, false, true, false>;
        case 3: return rmk::rm_query_points_kernel<LOOP, true, true, false>;
        case 4: return rmk::rm_query_points_kernel<LOOP, false, false, true>;
        case 5: return rmk::rm_query_points_kernel<LOOP, true, false, true>;
        case 6: return rmk::rm_query_points_kernel<LOOP, false, true, true>;
        default: return rmk::rm_query_points_kernel<LOOP, true, true, true>;
        }
    };
}
auto rays_kernel(bool taps, bool walk) {
    return [=](auto tag) {
        constexpr int LOOP = decltype(tag)::value;
        if (!walk) return rmk::rm_cast_rays_kernel<LOOP, true, false>;
        return taps ? rmk::rm_cast_rays_kernel<LOOP, true, true> : rmk::rm_cast_rays_kernel<LOOP, false, true>;
    };
}

// The input array of a query with outputs `o`: the caller's device array, or -- host memory: staged through the context's query
// buffers, synchronously on its own stream -- its copy in d_qin.  Reserves the outputs' staging on the way.
int query_input(rm_ctx* c, Outputs& o, const float* in, size_t bytes, hipStream_t s, const float** dev) {
    *dev = in;
    if (!o.to_host) return RM_OK;
    if (int rc = c->d_qin.reserve(c, bytes)) return rc;
    if (int rc = o.reserve()) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_qin.p, in, bytes, hipMemcpyHostToDevice, s));
    *dev = c->d_qin.as<const float>();
    return RM_OK;
}

}  // namespace

RM_EXPORT int rm_query_points(rm_ctx* c, uint32_t n, const float* xyz, float* out_dist, float* out_normal, uint32_t* out_ids,
                              int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_dist && !out_normal && !out_ids) return fail(c, RM_ERR_NULL, "rm_query_points: every output is NULL");
    if (n == 0u) return RM_OK;
    if (!xyz) return fail(c, RM_ERR_NULL, "rm_query_points: xyz is NULL");
    if (is_device && (misaligned(xyz, 4) || misaligned(out_dist, 4) || misaligned(out_normal, 4) || misaligned(out_ids, 8)))
        return fail(c, RM_ERR_ARG, "rm_query_points: device arrays need 4-byte alignment (out_ids: 8-byte)");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    QueryCall q;
    int rc = q.begin(c, s, out_ids != nullptr, false);
    if (rc != RM_OK) return rc;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_dist, (size_t)n * 4u);
    o.add(out_normal, (size_t)n * 12u);
    o.add(out_ids, (size_t)n * 8u);
    const float* d_xyz = nullptr;
    if ((rc = query_input(c, o, xyz, (size_t)n * 12u, s, &d_xyz)) != RM_OK) return rc;
    rc = q.launch(points_kernel(out_dist, out_normal, out_ids), query_blocks(n), 0u, n, d_xyz, o.dev<float>(0), o.dev<float>(1), o.dev<uint32_t>(2));
    return rc == RM_OK ? o.finish(s) : rc;
}

RM_EXPORT int rm_cast_rays(rm_ctx* c, uint32_t n, const float* rays, float* out_hit, uint32_t* out_ids, float* out_rgb,
                           int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_hit && !out_ids && !out_rgb) return fail(c, RM_ERR_NULL, "rm_cast_rays: every output is NULL");
    if (n == 0u) return RM_OK;
    if (!rays) return fail(c, RM_ERR_NULL, "rm_cast_rays: rays is NULL");
    if (is_device && (misaligned(rays, 4) || misaligned(out_hit, 16) || misaligned(out_ids, 16) || misaligned(out_rgb, 4)))
        return fail(c, RM_ERR_ARG, "rm_cast_rays: device arrays need 4-byte alignment (out_hit, out_ids: 16-byte)");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    QueryCall q;
    int rc = q.begin_program(c, s);
    if (rc != RM_OK) return rc;
    // the leaf walk runs for the ids, and for the colour of a tagged program (its albedo)
    const bool taps = out_hit || out_rgb;
    const bool walk = out_ids != nullptr || (out_rgb != nullptr && c->decoded.has_materials);
    if ((rc = q.begin_columns(walk, out_rgb != nullptr)) != RM_OK) return rc;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_hit, (size_t)n * 32u);
    o.add(out_ids, (size_t)n * 16u);
    o.add(out_rgb, (size_t)n * 12u);
    const float* d_rays = nullptr;
    if ((rc = query_input(c, o, rays, (size_t)n * 24u, s, &d_rays)) != RM_OK) return rc;
    rc = q.launch(rays_kernel(taps, walk), query_blocks(n), 0u, n, d_rays, o.dev<float>(0), o.dev<uint32_t>(1), o.dev<float>(2));
    return rc == RM_OK ? o.finish(s) : rc;
}

RM_EXPORT int rm_camera_rays(rm_ctx* c, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                             uint32_t sample, float* out_rays, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const uint64_t count = (uint64_t)w * h;
    if (count == 0u) return RM_OK;
    if (!out_rays) return fail(c, RM_ERR_NULL, "rm_camera_rays: out_rays is NULL");
    if (W == 0 || H == 0 || W > kMaxDim || H > kMaxDim) return fail(c, RM_ERR_RANGE, "image size %ux%u out of range", W, H);
    if ((uint64_t)x0 + w > W || (uint64_t)y0 + h > H)
        return fail(c, RM_ERR_RANGE, "pixel block [%u,+%u) x [%u,+%u) outside the %ux%u image", x0, w, y0, h, W, H);
    if (sample > RM_SAMPLE_CENTER) return fail(c, RM_ERR_RANGE, "sample %u: 0..15 or RM_SAMPLE_CENTER (16)", sample);
    if (is_device && misaligned(out_rays, 4)) return fail(c, RM_ERR_ARG, "rm_camera_rays: out_rays needs 4-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    order_with_previous(c, s);
    Outputs o(c, is_device, c->d_qout);
    o.add(out_rays, (size_t)count * 24u);
    int rc = o.reserve();
    if (rc != RM_OK) return rc;
    hipLaunchKernelGGL(rmk::rm_camera_rays_kernel, dim3(query_blocks(count)), dim3(256), 0, s, c->uniforms, W, H, x0, y0, w, count, sample, o.dev<float>(0));
    HIP_TRY(c, hipGetLastError());
    return o.finish(s);
}

// ---- ray traversal (rm_trace.h) ------------------------------------------------------------------------------------------
namespace {

// enum rm_trace: T_MIN, T_MAX, MIN_STEP, STEP_SCALE, LEVEL, MAX_STEPS
const float kTraceDefaults[RM_TRACE_PARAMS] = {0.0f, 100.0f, 0.001f, 1.0f, 0.0f, 1024.0f};

// The first parameter outside the table of enum rm_trace (NaN and infinities are outside everywhere), or -1.
int bad_trace_param(const float* p) {
    for (int i = 0; i < RM_TRACE_PARAMS; i++)
        if (!std::isfinite(p[i])) return i;
    if (!(p[RM_TRACE_T_MAX] >= p[RM_TRACE_T_MIN])) return RM_TRACE_T_MAX;
    if (!(p[RM_TRACE_MIN_STEP] > 0.0f)) return RM_TRACE_MIN_STEP;
    if (!(p[RM_TRACE_STEP_SCALE] > 0.0f && p[RM_TRACE_STEP_SCALE] <= 1.0f)) return RM_TRACE_STEP_SCALE;
    const float ms = p[RM_TRACE_MAX_STEPS];
    if (!(ms >= 1.0f && ms <= (float)kMaxIter && ms == std::floor(ms))) return RM_TRACE_MAX_STEPS;
    return -1;
}

auto trace_attr_kernel(bool normals, bool ids) {
    return [=](auto tag) {
        constexpr int LOOP = decltype(tag)::value;
        if (normals) return ids ? rmk::rm_trace_attr_kernel<LOOP, true, true> : rmk::rm_trace_attr_kernel<LOOP, true, false>;
        return rmk::rm_trace_attr_kernel<LOOP, false, true>;
    };
}

}  // namespace

RM_EXPORT int rm_trace_defaults(float* out, uint32_t n_out) {
    if (!out) return RM_ERR_NULL;
    if (n_out < (uint32_t)RM_TRACE_PARAMS) return RM_ERR_ARG;
    std::memcpy(out, kTraceDefaults, sizeof kTraceDefaults);
    return RM_OK;
}

RM_EXPORT int rm_trace_rays(rm_ctx* c, uint32_t n, const float* rays, const float* params, uint32_t n_params, uint32_t max_events,
                            uint32_t flags, float* out_events, uint32_t* out_event_ids, uint32_t* out_counts, float* out_spans,
                            int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_events && !out_event_ids && !out_counts && !out_spans) return fail(c, RM_ERR_NULL, "rm_trace_rays: every output is NULL");
    if (n_params != (uint32_t)RM_TRACE_PARAMS)
        return fail(c, RM_ERR_ARG, "rm_trace_rays: %u parameters, not %d", n_params, (int)RM_TRACE_PARAMS);
    if (flags & ~(uint32_t)(RM_MESH_NORMALS | RM_MESH_IDS)) return fail(c, RM_ERR_ARG, "rm_trace_rays: unknown flags 0x%x", flags);
    if (max_events == 0u || max_events > (uint32_t)RM_TRACE_MAX_EVENTS)
        return fail(c, RM_ERR_RANGE, "rm_trace_rays: max_events %u not in [1,%d]", max_events, (int)RM_TRACE_MAX_EVENTS);
    if (params) {
        const int bad = bad_trace_param(params);
        if (bad >= 0)
            return fail(c, RM_ERR_RANGE, "rm_trace_rays: parameter %d = %g is outside its range (enum rm_trace)", bad, (double)params[bad]);
    }
    if (n == 0u) return RM_OK;
    if (!rays || !params) return fail(c, RM_ERR_NULL, "rm_trace_rays: %s is NULL", rays ? "params" : "rays");
    if (is_device && (misaligned(rays, 4) || misaligned(out_events, 16) || misaligned(out_event_ids, 16) || misaligned(out_counts, 16) ||
                      misaligned(out_spans, 16)))
        return fail(c, RM_ERR_ARG, "rm_trace_rays: device arrays need 16-byte alignment (rays: 4-byte)");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    QueryCall q;
    int rc = q.begin(c, s, false, false);  // the march: the distance loop's columns
    if (rc != RM_OK) return rc;
    if (!q.fits(rml::kQueryOwnTrace))
        return fail(c, RM_ERR_TOO_LARGE, "the query needs %zu bytes of LDS per workgroup", (size_t)q.lds.behind(rml::kQueryOwnTrace).bytes);
    // the attribute pass runs for what the caller both asked for and takes; with the ids its columns hold the walk's layout
    const bool normals = (flags & RM_MESH_NORMALS) && out_events, ids = (flags & RM_MESH_IDS) && out_event_ids, attr = normals || ids;
    const QueryCall qa = q.with_slots(query_slots(c->decoded, q.loop, ids));
    if (attr && !qa.fits(0u)) return fail(c, RM_ERR_TOO_LARGE, "the query needs %zu bytes of LDS per workgroup", (size_t)qa.lds.bytes);
    const uint32_t K = max_events, nb = (uint32_t)(((uint64_t)n + 255u) / 256u);
    const rmk::TraceLaunch T{params[RM_TRACE_T_MIN], params[RM_TRACE_T_MAX], params[RM_TRACE_MIN_STEP], params[RM_TRACE_STEP_SCALE],
                             params[RM_TRACE_LEVEL], (uint32_t)params[RM_TRACE_MAX_STEPS], K};
    const rml::TraceScratch<uint2> L(n, nb, K, attr && !out_events);
    if (attr)
        if ((rc = c->d_tscratch.reserve(c, L.bytes, "traversal scratch")) != RM_OK) return rc;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_events, (size_t)n * K * 32u);
    o.add(out_event_ids, (size_t)n * K * 16u);
    o.add(out_counts, (size_t)n * 16u);
    o.add(out_spans, (size_t)n * 16u);
    const float* d_rays = nullptr;
    if ((rc = query_input(c, o, rays, (size_t)n * 24u, s, &d_rays)) != RM_OK) return rc;
    void* base = c->d_tscratch.p;
    // the event records the march writes and the attribute pass reads the positions from: the caller's, else the scratch copy
    float* d_events = out_events ? o.dev<float>(0) : attr ? L.events.at(base) : nullptr;
    rc = q.launch(RM_BY_LOOP(rm_trace_march_kernel), nb, rml::kQueryOwnTrace, T, n, d_rays, d_events, o.dev<uint32_t>(1), o.dev<uint32_t>(2),
                  o.dev<float>(3), attr ? L.stored.at(base) : nullptr, attr ? L.sums.at(base) : nullptr);
    if (rc == RM_OK && attr) {
        hipLaunchKernelGGL(rmk::rm_mesh_scan_kernel, dim3(1), dim3(1024), 0, s, L.sums.at(base), nb, L.totals.at(base));
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(rmk::rm_trace_list_kernel, dim3(nb), dim3(256), 0, s, n, L.stored.at(base), L.sums.at(base), L.list.at(base));
        HIP_TRY(c, hipGetLastError());
        // one lane per stored event; how many there are only the device knows, so a fixed number of workgroups strides over them
        const uint64_t most = ((uint64_t)n * K + 255u) / 256u;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(most, (uint64_t)std::max(c->cu_count, 1) * 8u);
        rc = qa.launch(trace_attr_kernel(normals, ids), blocks, 0u, K, L.totals.at(base), L.list.at(base), d_events,
                       normals ? o.dev<float>(0) : nullptr, ids ? o.dev<uint32_t>(1) : nullptr);
    }
    return rc == RM_OK ? o.finish(s) : rc;
}

// ---- lit rendering (rm_light.h) ------------------------------------------------------------------------------------------
namespace {

// The first parameter outside the table of enum rm_light (NaN and infinities are outside everywhere), or -1.
int bad_light_param(const float* p) {
    const auto integral = [](float v, float lo, float hi) { return v >= lo && v <= hi && v == std::floor(v); };
    for (int i = 0; i < RM_LIGHT_PARAMS; i++)
        if (!std::isfinite(p[i])) return i;
    if (!(p[RM_LIGHT_SHADOW] >= 0.0f && p[RM_LIGHT_SHADOW] <= 1.0f)) return RM_LIGHT_SHADOW;
    if (!(p[RM_LIGHT_SHADOW_SOFTNESS] > 0.0f)) return RM_LIGHT_SHADOW_SOFTNESS;
    if (!(p[RM_LIGHT_BIAS] >= 0.0f)) return RM_LIGHT_BIAS;
    if (!(p[RM_LIGHT_SHADOW_MAX_T] > 0.0f)) return RM_LIGHT_SHADOW_MAX_T;
    if (!integral(p[RM_LIGHT_SHADOW_STEPS], 1.0f, 1024.0f)) return RM_LIGHT_SHADOW_STEPS;
    if (!(p[RM_LIGHT_AO] >= 0.0f && p[RM_LIGHT_AO] <= 1.0f)) return RM_LIGHT_AO;
    if (!(p[RM_LIGHT_AO_STEP] > 0.0f)) return RM_LIGHT_AO_STEP;
    if (!(p[RM_LIGHT_AO_FALLOFF] > 0.0f && p[RM_LIGHT_AO_FALLOFF] <= 1.0f)) return RM_LIGHT_AO_FALLOFF;
    if (!(p[RM_LIGHT_AO_SCALE] >= 0.0f)) return RM_LIGHT_AO_SCALE;
    if (!integral(p[RM_LIGHT_AO_TAPS], 1.0f, 16.0f)) return RM_LIGHT_AO_TAPS;
    return -1;
}

auto lit_kernel(bool shadow, bool ao) {
    return [=](auto tag) {
        constexpr int LOOP = decltype(tag)::value;
        if (shadow) return ao ? rmk::rm_draw_lit_kernel<LOOP, true, true> : rmk::rm_draw_lit_kernel<LOOP, true, false>;
        return ao ? rmk::rm_draw_lit_kernel<LOOP, false, true> : rmk::rm_draw_lit_kernel<LOOP, false, false>;
    };
}

}  // namespace

RM_EXPORT int rm_lighting_defaults(float* out, uint32_t n_out) {
    if (!out) return RM_ERR_NULL;
    if (n_out < (uint32_t)RM_LIGHT_PARAMS) return RM_ERR_ARG;
    std::memcpy(out, kLightDefaults, sizeof kLightDefaults);
    return RM_OK;
}

RM_EXPORT int rm_set_lighting(rm_ctx* c, const float* params, uint32_t count) {
    if (!c) return RM_ERR_NULL;
    if (!params) return fail(c, RM_ERR_NULL, "rm_set_lighting: params is NULL");
    if (count != (uint32_t)RM_LIGHT_PARAMS) return fail(c, RM_ERR_ARG, "rm_set_lighting: %u parameters, not %d", count, (int)RM_LIGHT_PARAMS);
    const int bad = bad_light_param(params);
    if (bad >= 0) return fail(c, RM_ERR_RANGE, "rm_set_lighting: parameter %d = %g is outside its range (enum rm_light)", bad, (double)params[bad]);
    std::memcpy(c->light, params, sizeof c->light);
    return RM_OK;
}

RM_EXPORT int rm_draw_lit(rm_ctx* c, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, float* out_rgba, int out_is_device,
                          void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_rgba) return fail(c, RM_ERR_NULL, "rm_draw_lit: out_rgba is NULL");
    int rc = check_dims(c, W, H, row0, rows);
    if (rc != RM_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, out_is_device, stream);
    QueryCall q;
    if ((rc = q.begin_program(c, s)) != RM_OK) return rc;
    // the leaf walk runs for the albedo of a tagged program
    if ((rc = q.begin_columns(c->decoded.has_materials, true)) != RM_OK) return rc;
    const float* p = c->light;
    rmk::LightLaunch P{p[RM_LIGHT_POS_X], p[RM_LIGHT_POS_Y], p[RM_LIGHT_POS_Z], p[RM_LIGHT_SHADOW], p[RM_LIGHT_SHADOW_SOFTNESS],
                       p[RM_LIGHT_BIAS], p[RM_LIGHT_SHADOW_MAX_T], (uint32_t)p[RM_LIGHT_SHADOW_STEPS], p[RM_LIGHT_AO],
                       p[RM_LIGHT_AO_STEP], p[RM_LIGHT_AO_FALLOFF], p[RM_LIGHT_AO_SCALE], (uint32_t)p[RM_LIGHT_AO_TAPS]};
    const bool shadow = P.shadow > 0.0f, ao = P.ao > 0.0f;
    rmk::LitFrame F;
    F.u = c->uniforms;
    F.W = W; F.H = H; F.row0 = row0; F.rows = rows;
    F.format = (uint32_t)c->out_format;
    const size_t lanes = (size_t)((W + 1u) / 2u) * ((rows + 1u) / 2u) * 64u;  // one wave per 2 x 2 block of pixels
    // host memory: staged through the context's query buffer (never the draws' scratch), synchronously on its own stream
    Outputs o(c, out_is_device, c->d_qout);
    o.add(out_rgba, (size_t)rows * W * pixel_bytes(c));
    if ((rc = o.reserve()) != RM_OK) return rc;
    F.out = o.dev<void>(0);
    rc = q.launch(lit_kernel(shadow, ao), query_blocks(lanes), 0u, P, F);
    return rc == RM_OK ? o.finish(s) : rc;
}

// ---- G-buffer draw (rm_gbuffer.h) ----------------------------------------------------------------------------------------
RM_EXPORT int rm_program_subtree(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, uint32_t cmd_index,
                                 uint32_t* out_first, uint32_t* out_count) {
    RmDecoded d;
    const int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc != RM_OK) return rc;
    if (cmd_index >= cmd_count) return RM_ERR_RANGE;
    // the value stack of the (valid) program, holding for each value the first command of the sub-tree that produced it
    std::vector<uint32_t> first, scopes;  // scopes: the command index of each open transform Push
    uint32_t lo = 0u, hi = 0u, wanted_pop = cmd_index;  // cmd_index names a Push: answered at its Pop
    bool found = false, at_pop = false;
    for (uint32_t i = 0, q = 0; i < cmd_count && !found; i++) {
        const uint32_t op = words[q];
        q += 1u + (op == RM_CMD_SPHERE || op == RM_CMD_PLANE || op == RM_CMD_ROTATION_PUSH ? 4u : op == RM_CMD_BOX ? 6u
                   : op == RM_CMD_CYLINDER ? 5u : op == RM_CMD_TRANSLATION_PUSH ? 3u
                   : op == RM_CMD_SMOOTH_UNION || op == RM_CMD_SCALE_PUSH || op == RM_CMD_MATERIAL ? 1u : 0u);
        uint32_t start;
        if (op == RM_CMD_TRANSLATION_PUSH || op == RM_CMD_ROTATION_PUSH || op == RM_CMD_SCALE_PUSH) {
            scopes.push_back(i);
            if (i == cmd_index) at_pop = true;
            continue;
        } else if (op == RM_CMD_TRANSLATION_POP || op == RM_CMD_ROTATION_POP || op == RM_CMD_SCALE_POP) {
            start = first.back() = scopes.back();  // the scope's value now spans Push .. Pop
            scopes.pop_back();
            if (at_pop && start == wanted_pop) found = true;
        } else if (op == RM_CMD_MATERIAL) {
            start = first.back();
        } else if (op == RM_CMD_UNION || op == RM_CMD_SUBTRACTION || op == RM_CMD_INTERSECTION || op == RM_CMD_SMOOTH_UNION) {
            first.pop_back();  // the right operand's; the left operand's first command stays: the result spans both
            start = first.back();
        } else {
            first.push_back(i);
            start = i;
        }
        if (i == cmd_index) found = true;
        if (found) { lo = start; hi = i; }
    }
    if (!found) return RM_ERR_RANGE;  // (unreachable for a valid program: every Push has its Pop)
    if (out_first) *out_first = lo;
    if (out_count) *out_count = hi - lo + 1u;
    return RM_OK;
}

namespace {
auto gbuffer_kernel(bool all) {
    return [=](auto tag) {
        constexpr int LOOP = decltype(tag)::value;
        return all ? rmk::rm_draw_gbuffer_kernel<LOOP, true> : rmk::rm_draw_gbuffer_kernel<LOOP, false>;
    };
}
}  // namespace

RM_EXPORT int rm_draw_gbuffer(rm_ctx* c, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t sample, uint32_t sel_first,
                              uint32_t sel_count, float* out_geom, uint32_t* out_ids, uint32_t* out_masks, int is_device,
                              void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_geom && !out_ids && !out_masks) return fail(c, RM_ERR_NULL, "rm_draw_gbuffer: every output is NULL");
    if ((uint64_t)W * rows == 0u) return RM_OK;
    int rc = check_dims(c, W, H, row0, rows);
    if (rc != RM_OK) return rc;
    if (sample > (uint32_t)RM_SAMPLE_ALL)
        return fail(c, RM_ERR_ARG, "rm_draw_gbuffer: sample %u: 0..15, RM_SAMPLE_CENTER (16) or RM_SAMPLE_ALL (17)", sample);
    if (is_device && (misaligned(out_geom, 16) || misaligned(out_ids, 16) || misaligned(out_masks, 16)))
        return fail(c, RM_ERR_ARG, "rm_draw_gbuffer: device arrays need 16-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    QueryCall q;
    if ((rc = q.begin_program(c, s)) != RM_OK) return rc;
    if ((uint64_t)sel_first + sel_count > c->cmd[0])
        return fail(c, RM_ERR_ARG, "rm_draw_gbuffer: selection [%u,+%u) reaches past the program's %u commands", sel_first, sel_count, c->cmd[0]);
    // the leaf walk runs for the ids, and for the selected mask of a selection that is not empty
    const bool walk = out_ids != nullptr || (out_masks != nullptr && sel_count != 0u);
    if ((rc = q.begin_columns(walk, false)) != RM_OK) return rc;
    const bool all = sample == (uint32_t)RM_SAMPLE_ALL;
    rmk::GBufferFrame F;
    F.u = c->uniforms;
    F.W = W; F.H = H; F.row0 = row0; F.rows = rows;
    F.sample = sample;
    F.sel_first = sel_first; F.sel_count = sel_count;
    F.taps = out_geom != nullptr ? 1u : 0u;
    F.walk = walk ? 1u : 0u;
    // one wave per 2 x 2 block of pixels (all samples), or per 8 x 8 tile (one sample)
    const size_t lanes = all ? (size_t)((W + 1u) / 2u) * ((rows + 1u) / 2u) * 64u : (size_t)((W + 7u) / 8u) * ((rows + 7u) / 8u) * 64u;
    // host memory: staged through the context's query buffer (never the draws' scratch), synchronously on its own stream
    const size_t n = (size_t)rows * W;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_geom, n * 32u);
    o.add(out_ids, n * 16u);
    o.add(out_masks, n * 16u);
    if ((rc = o.reserve()) != RM_OK) return rc;
    F.geom = o.dev<float>(0); F.ids = o.dev<uint32_t>(1); F.masks = o.dev<uint32_t>(2);
    rc = q.launch(gbuffer_kernel(all), query_blocks(lanes), 0u, F);
    return rc == RM_OK ? o.finish(s) : rc;
}

// ---- mesh export (rm_mesh.h) ---------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t kMaxGridPoints = 1ull << 31;  // rm_sample_grid
constexpr uint64_t kMaxMeshPoints = 1ull << 28;  // rm_extract_mesh: u32 prefix sums (<= 3 * 2^28 vertices, 5 * 2^28 triangles)

// origin and step of a lattice (host arrays of 3 floats): finite, and step > 0 so that no axis is flipped (the winding)
int check_lattice(rm_ctx* c, const char* fn, const float* origin, const float* step) {
    if (!origin || !step) return fail(c, RM_ERR_NULL, "%s: origin or step is NULL", fn);
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(origin[a])) return fail(c, RM_ERR_ARG, "%s: origin[%d] = %g is not finite", fn, a, (double)origin[a]);
        if (!std::isfinite(step[a]) || !(step[a] > 0.0f))
            return fail(c, RM_ERR_ARG, "%s: step[%d] = %g: a step must be finite and > 0", fn, a, (double)step[a]);
    }
    return RM_OK;
}

int launch_grid(const QueryCall& q, const float* o, const float* st, uint32_t nx, uint32_t ny, uint64_t n, float* out) {
    return q.launch(RM_BY_LOOP(rm_grid_dist_kernel), query_blocks(n), 0u, o[0], o[1], o[2], st[0], st[1], st[2], nx, ny, n, out);
}

// level and flags of the iso-surface entry points (rm_extract_mesh, rm_extract_mesh_sparse, rm_slice_contours)
int check_iso(rm_ctx* c, const char* fn, float level, uint32_t flags) {
    if (!std::isfinite(level)) return fail(c, RM_ERR_ARG, "%s: level %g is not finite", fn, (double)level);
    if (flags & ~(uint32_t)(RM_MESH_NORMALS | RM_MESH_IDS)) return fail(c, RM_ERR_ARG, "%s: unknown flags 0x%x", fn, flags);
    return RM_OK;
}

// Where the arrays of a mesh of v vertices and t triangles lie in rm_ctx::mesh.buf.
rml::MeshLayout mesh_layout(uint64_t v, uint64_t t, uint32_t flags) {
    return rml::MeshLayout(v, t, (flags & RM_MESH_NORMALS) != 0, (flags & RM_MESH_IDS) != 0);
}

// The attributes (regions of the buffer at `base`) of n points: rm_query_points at their positions, device to device.
int point_attributes(const QueryCall& q, uint32_t flags, uint64_t n, const float* points, char* base, const rml::Region<float>& nrm,
                     const rml::Region<uint32_t>& idp) {
    const bool normals = (flags & RM_MESH_NORMALS) != 0, ids = (flags & RM_MESH_IDS) != 0;
    if (!(normals || ids) || n == 0u) return RM_OK;
    return q.launch(points_kernel(false, normals, ids), query_blocks(n), 0u, (uint32_t)n, points, static_cast<float*>(nullptr),
                    normals ? nrm.at(base) : nullptr, ids ? idp.at(base) : nullptr);
}

// ---- sparse extraction (rm_mesh_sparse.h) ----
// The regions of the kept bricks' scratch round up to 16 bytes like all others; the segment maps and the segments' first
// (vertex, triangle) pairs always were whole multiples of 16, so RM_MESH_STAT_SCRATCH_BYTES is what it was.
static_assert(sizeof(rmk::SparseSegMap) % 16u == 0u && (rmk::kBrickSegs * sizeof(uint2)) % 16u == 0u, "sparse scratch layout");
static_assert(rmk::kRowWords == (uint32_t)RM_MOMENTS, "a row holds the moments of enum rm_moment");
constexpr uint32_t kMaxMassDim = 4096u;  // rm_mass_moments: every sum below 2^60 (rm_abi.h)
constexpr uint32_t kMaxTopoDim = 1024u;        // rm_label_solid: labels are linear indices with the two top bits free ...
constexpr uint64_t kMaxTopoPoints = 1ull << 28;  // ... and every moment stays far below 2^60
constexpr uint32_t kMaxMergePasses = 8u;
static_assert(rmk::kRowsFold == 256u, "TopoScratch folds the bricks' rows by the probe's blocks of 256");
static_assert(rmk::kTopoExterior == RM_TOPO_EXTERIOR && rmk::kTopoCavityBit == RM_TOPO_CAVITY_BIT, "the label volume's marks");
static_assert(rmk::kDistInside == RM_DIST_INSIDE_BIT && rmk::kDistNone == RM_DIST_NONE, "the distance volume's marks");
static_assert(rml::kDistMaxAxis == kMaxTopoDim, "a column tile holds the longest axis");
constexpr uint32_t kMaxDistR2 = 1u << 22;  // rm_distance_features: every finite D2 is below it

// The lattice of a caller's occupancy: the unit lattice at the origin.
constexpr float kUnitOrigin[3] = {0.0f, 0.0f, 0.0f}, kUnitStep[3] = {1.0f, 1.0f, 1.0f};

// A lattice in bricks.  nb stays 0: how many bricks a call takes is its own check.
rmk::SparseGrid sparse_grid(const float* o, const float* st, uint32_t nx, uint32_t ny, uint32_t nz) {
    return rmk::SparseGrid{o[0], o[1], o[2], st[0], st[1], st[2], nx, ny, nz,
                           (nx + rmk::kBrick - 1u) / rmk::kBrick, (ny + rmk::kBrick - 1u) / rmk::kBrick, (nz + rmk::kBrick - 1u) / rmk::kBrick, 0u};
}

// What a call over the bricks of a lattice does after QueryCall::begin: the LDS check of its workgroups (the query's columns
// behind the brick kernels' own LDS), the bounds of the program for points up to the lattice's largest coordinate (as the
// kernels compute it), the lattice in bricks.
int brick_lattice(const QueryCall& q, const char* fn, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                  RmProgramBound* bound, rmk::SparseGrid* g) {
    rm_ctx* c = q.c;
    if (!q.fits(rml::kQueryOwnBrick))
        return fail(c, RM_ERR_TOO_LARGE, "%s: the program needs %zu bytes of LDS per workgroup", fn, (size_t)q.lds.behind(rml::kQueryOwnBrick).bytes);
    double P = 0.0;
    const uint32_t dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++) {
        const float last = origin[a] + (float)(dims[a] - 1u) * step[a];
        P = std::fmax(P, std::fmax(std::fabs((double)origin[a]), std::fabs((double)last)));
    }
    *g = sparse_grid(origin, step, nx, ny, nz);
    return rm_program_bound(c->cmd[0], c->cmd.data() + 1, (uint32_t)c->cmd.size() - 1u, P, bound);
}

// The bricks of rm_extract_mesh_sparse and rm_mass_moments, whose lattices can hold more than a brick table has entries.
int count_bricks(rm_ctx* c, const char* fn, rmk::SparseGrid* g) {
    const uint64_t nb64 = (uint64_t)g->bx * g->by * g->bz;
    if (nb64 >= 0xFFFFFFFFull - 256u)
        return fail(c, RM_ERR_DEVICE, "%s: %llu bricks: the brick table is limited to 2^32 entries", fn, (unsigned long long)nb64);
    g->nb = (uint32_t)nb64;
    return RM_OK;
}

// ---- the reductions' host side (rm_reduce.h) ----
// One more copy from device to host that rides on the single synchronise of the helpers below.
struct AlsoRead {
    void* host = nullptr;
    const void* dev = nullptr;
    size_t bytes = 0;
};

// The two totals rm_block_scan_kernel left in totals_dev -> out, with `also` beside them; synchronises.
int read_totals(rm_ctx* c, hipStream_t s, const unsigned long long* totals_dev, uint64_t out[2], AlsoRead also = AlsoRead()) {
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the totals are copied as they lie");
    HIP_TRY(c, hipMemcpyAsync(out, totals_dev, 2u * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (also.bytes) HIP_TRY(c, hipMemcpyAsync(also.host, also.dev, also.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return RM_OK;
}

// The n_blocks block sums (lo | hi << 32) -> exclusive offsets in place, the two totals into totals_dev; queued, not read.
int scan_launch(rm_ctx* c, hipStream_t s, unsigned long long* sums, uint32_t n_blocks, unsigned long long* totals_dev) {
    hipLaunchKernelGGL(rmk::rm_block_scan_kernel, dim3(1), dim3(1024), 0, s, sums, n_blocks, totals_dev);
    HIP_TRY(c, hipGetLastError());
    return RM_OK;
}

// Both: the scan, and its totals on the host.
int scan_totals(rm_ctx* c, hipStream_t s, unsigned long long* sums, uint32_t n_blocks, unsigned long long* totals_dev, uint64_t out[2],
                AlsoRead also = AlsoRead()) {
    if (int rc = scan_launch(c, s, sums, n_blocks, totals_dev)) return rc;
    return read_totals(c, s, totals_dev, out, also);
}

// The rows a[0, na) and b[0, nb) -> result (rm_rows_reduce_kernel, one workgroup) -> row on the host, with `also` beside it;
// synchronises.
int reduce_to_row(rm_ctx* c, hipStream_t s, const unsigned long long* a, uint32_t na, const unsigned long long* b, uint32_t nb,
                  unsigned long long* result, unsigned long long row[RM_MOMENTS], AlsoRead also = AlsoRead()) {
    hipLaunchKernelGGL(rmk::rm_rows_reduce_kernel, dim3(1), dim3(256), 0, s, a, na, b, nb, result);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(row, result, RM_MOMENTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (also.bytes) HIP_TRY(c, hipMemcpyAsync(also.host, also.dev, also.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return RM_OK;
}

// A launch's n_rows rows -> folded (rm_rows_fold_kernel, kRowsFold rows to a workgroup) -> result -> row, as above.
int reduce_rows(rm_ctx* c, hipStream_t s, const unsigned long long* rows, uint32_t n_rows, unsigned long long* folded,
                unsigned long long* result, unsigned long long row[RM_MOMENTS], AlsoRead also = AlsoRead()) {
    const uint32_t n_folded = rmk::rows_folded(n_rows);
    hipLaunchKernelGGL(rmk::rm_rows_fold_kernel, dim3(n_folded), dim3(256), 0, s, rows, n_rows, folded);
    return reduce_to_row(c, s, folded, n_folded, nullptr, 0u, result, row, also);
}

// The front of a pass over the bricks, in the tables B of the buffer at `base` (regions psums, ptot, evals): the evaluation
// counter zeroed, the probe `probe` of n_pblocks blocks of 256 bricks on (g, level, the program's bounds, its table, psums,
// extra...), the scan of its block sums (kept in the low half, inside in the high half -> ptot).
template <class F, class Tables, class T, class... Extra>
int brick_probe(const QueryCall& q, F&& probe, const rmk::SparseGrid& g, float level, const RmProgramBound& bound, uint32_t n_pblocks,
                const Tables& B, char* base, T* table, Extra... extra) {
    unsigned long long* psums = B.psums.at(base);
    HIP_TRY(q.c, hipMemsetAsync(B.evals.at(base), 0, 8, q.s));
    if (int rc = q.launch(probe, n_pblocks, rml::kQueryOwnBrick, g, level, bound.L, 2.0 * bound.E, table, psums, extra...)) return rc;
    return scan_launch(q.c, q.s, psums, n_pblocks, B.ptot.at(base));
}

// The whole pass of a call that goes on with the kept bricks alone: the front above with the keep flags in B.boff, its two
// totals read into tot (kept, inside), and -- any kept -- their indices compacted into the list that reserve_kept(kept, &klist)
// makes room for.
template <class F, class Tables, class R, class... Extra>
int brick_pass(const QueryCall& q, F&& probe, const rmk::SparseGrid& g, float level, const RmProgramBound& bound, uint32_t n_entries,
               uint32_t n_pblocks, const Tables& B, char* base, uint64_t tot[2], R&& reserve_kept, Extra... extra) {
    uint32_t* boff = B.boff.at(base);
    if (int rc = brick_probe(q, probe, g, level, bound, n_pblocks, B, base, boff, extra...)) return rc;
    if (int rc = read_totals(q.c, q.s, B.ptot.at(base), tot)) return rc;
    if (tot[0] == 0u) return RM_OK;
    uint32_t* klist = nullptr;
    if (int rc = reserve_kept(tot[0], &klist)) return rc;
    hipLaunchKernelGGL(rmk::rm_sparse_compact_kernel, dim3(n_pblocks), dim3(256), 0, q.s, n_entries, B.psums.at(base), boff, klist);
    return RM_OK;
}

}  // namespace

RM_EXPORT int rm_sample_grid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                             float* out_dist, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (int rc = check_lattice(c, "rm_sample_grid", origin, step)) return rc;
    const uint64_t n = (uint64_t)nx * ny * nz;
    if (nx == 0 || ny == 0 || nz == 0 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim || n > kMaxGridPoints)
        return fail(c, RM_ERR_RANGE, "rm_sample_grid: lattice %ux%ux%u: 1..65536 points per axis, at most 2^31 in all", nx, ny, nz);
    if (!out_dist) return fail(c, RM_ERR_NULL, "rm_sample_grid: out_dist is NULL");
    if (is_device && misaligned(out_dist, 4)) return fail(c, RM_ERR_ARG, "rm_sample_grid: out_dist needs 4-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    QueryCall q;
    int rc = q.begin(c, s, false, false);
    if (rc != RM_OK) return rc;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_dist, n * 4u);
    if ((rc = o.reserve()) != RM_OK) return rc;
    rc = launch_grid(q, origin, step, nx, ny, n, o.dev<float>(0));
    return rc == RM_OK ? o.finish(s) : rc;
}

RM_EXPORT int rm_extract_mesh(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                              float level, uint32_t flags, uint64_t* out_counts) {
    if (!c) return RM_ERR_NULL;
    if (!out_counts) return fail(c, RM_ERR_NULL, "rm_extract_mesh: out_counts is NULL");
    if (int rc = check_lattice(c, "rm_extract_mesh", origin, step)) return rc;
    if (int rc = check_iso(c, "rm_extract_mesh", level, flags)) return rc;
    const uint64_t n64 = (uint64_t)nx * ny * nz;
    if (nx < 2 || ny < 2 || nz < 2 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim || n64 > kMaxMeshPoints)
        return fail(c, RM_ERR_RANGE, "rm_extract_mesh: lattice %ux%ux%u: 2..65536 points per axis, at most 2^28 in all", nx, ny, nz);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    QueryCall q;
    int rc = q.begin(c, s, (flags & RM_MESH_IDS) != 0, false);  // after a device read of the previous mesh, too
    if (rc != RM_OK) return rc;
    c->mesh.drop();
    const uint32_t n = (uint32_t)n64, nb = (n + rmk::kMeshBlock - 1u) / rmk::kMeshBlock;
    const rml::DenseMeshScratch S(n, nb);
    if ((rc = c->d_mscratch.reserve(c, S.bytes)) != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    float* dist = S.dist.at(sc);
    uint32_t* vbase = S.vbase.at(sc);
    uint8_t* fl = S.flags.at(sc);
    unsigned long long* sums = S.sums.at(sc);
    uint32_t* totals = S.totals.at(sc);
    const rmk::MeshGrid g{origin[0], origin[1], origin[2], step[0], step[1], step[2], nx, ny, nz, n};
    if ((rc = launch_grid(q, origin, step, nx, ny, n, dist)) != RM_OK) return rc;
    hipLaunchKernelGGL(rmk::rm_mesh_count_kernel, dim3(nb), dim3(256), 0, s, g, level, dist, sums);
    hipLaunchKernelGGL(rmk::rm_mesh_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, totals);
    HIP_TRY(c, hipGetLastError());
    uint32_t tot[2] = {0u, 0u};
    HIP_TRY(c, hipMemcpyAsync(tot, totals, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t V = tot[0], T = tot[1];
    const rml::MeshLayout L = mesh_layout(V, T, flags);
    if ((rc = c->mesh.buf.reserve(c, L.bytes)) != RM_OK) return rc;
    char* m = c->mesh.buf.p;
    float* verts = L.vertices.at(m);
    if (V > 0u) {
        const unsigned long long* offs = sums;
        hipLaunchKernelGGL(rmk::rm_mesh_vertex_kernel, dim3(nb), dim3(256), 0, s, g, level, dist, offs, vbase, fl, verts);
        if (T > 0u)
            hipLaunchKernelGGL(rmk::rm_mesh_triangle_kernel, dim3(nb), dim3(256), 0, s, g, offs, vbase, fl, L.triangles.at(m));
        HIP_TRY(c, hipGetLastError());
        if ((rc = point_attributes(q, flags, V, verts, m, L.normals, L.ids)) != RM_OK) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    out_counts[0] = V;
    out_counts[1] = T;
    c->mesh.commit(V, T, flags);
    return RM_OK;
}

RM_EXPORT int rm_program_lipschitz(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, double* out_L) {
    if (!out_L) return RM_ERR_NULL;
    RmProgramBound b;
    const int rc = rm_program_bound(cmd_count, words, n_words, 1.0, &b);
    if (rc != RM_OK) return rc;
    *out_L = b.L;
    return RM_OK;
}

RM_EXPORT int rm_extract_mesh_sparse(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                                     float level, uint32_t flags, uint64_t* out_stats, uint32_t n_stats) {
    if (!c) return RM_ERR_NULL;
    if (!out_stats) return fail(c, RM_ERR_NULL, "rm_extract_mesh_sparse: out_stats is NULL");
    if (n_stats < (uint32_t)RM_MESH_STATS) return fail(c, RM_ERR_ARG, "rm_extract_mesh_sparse: n_stats %u < RM_MESH_STATS", n_stats);
    if (int rc = check_lattice(c, "rm_extract_mesh_sparse", origin, step)) return rc;
    if (int rc = check_iso(c, "rm_extract_mesh_sparse", level, flags)) return rc;
    if (nx < 2 || ny < 2 || nz < 2 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim)
        return fail(c, RM_ERR_RANGE, "rm_extract_mesh_sparse: lattice %ux%ux%u: 2..65536 points per axis", nx, ny, nz);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    QueryCall q;
    int rc = q.begin(c, s, (flags & RM_MESH_IDS) != 0, false);  // after a device read of the previous mesh, too
    if (rc != RM_OK) return rc;
    RmProgramBound bound;
    rmk::SparseGrid g;
    if ((rc = brick_lattice(q, "rm_extract_mesh_sparse", origin, step, nx, ny, nz, &bound, &g)) != RM_OK) return rc;
    c->mesh.drop();  // (brick_lattice refuses at its LDS check only: the program's bound decodes what QueryCall::begin has decoded)
    if ((rc = count_bricks(c, "rm_extract_mesh_sparse", &g)) != RM_OK) return rc;
    // per brick: 4 B (keep flag, then the kept bricks before it); per 256 bricks a block sum; totals and the evaluation count
    const uint32_t n_entries = g.nb + 1u, n_pblocks = (n_entries + 255u) / 256u;
    const rml::SparseBrickTables B(n_entries, n_pblocks);
    if ((rc = c->d_mbricks.reserve(c, B.bytes)) != RM_OK) return rc;
    char* bs = c->d_mbricks.p;
    uint32_t* boff = B.boff.at(bs);
    unsigned long long* evals = B.evals.at(bs);
    // per kept brick: its index, its segment map, its tile of distances, 64 segment words and their first (vertex, triangle)
    using Kept = rml::SparseKeptScratch<rmk::SparseSegMap, uint2>;
    Kept S(0u, rmk::kTilePoints, 0u, 0u);
    uint32_t n_segs = 0u, n_sblocks = 0u;
    uint64_t tot[2] = {0u, 0u};
    rc = brick_pass(q, RM_BY_LOOP(rm_sparse_probe_kernel), g, level, bound, n_entries, n_pblocks, B, bs, tot, [&](uint64_t kept, uint32_t** klist) {
        if (kept * rmk::kBrickSegs >= 0xFFFFFFFFull)
            return fail(c, RM_ERR_DEVICE, "rm_extract_mesh_sparse: %llu bricks to evaluate: more than the segment index holds", (unsigned long long)kept);
        n_segs = (uint32_t)(kept * rmk::kBrickSegs);
        n_sblocks = (n_segs + rmk::kSegBlock - 1u) / rmk::kSegBlock;
        S = Kept(kept, rmk::kTilePoints, n_segs, n_sblocks);
        if (int rrc = c->d_mscratch.reserve(c, S.bytes)) return rrc;
        *klist = S.klist.at(c->d_mscratch.p);
        return (int)RM_OK;
    });
    if (rc != RM_OK) return rc;
    const uint64_t K = tot[0];
    uint64_t V = 0, T = 0, n_evals = g.nb;
    size_t kept_bytes = 0;
    rml::MeshLayout L = mesh_layout(0, 0, flags);
    if (K > 0u) {
        kept_bytes = S.bytes;
        char* sc = c->d_mscratch.p;
        uint32_t* klist = S.klist.at(sc);
        rmk::SparseSegMap* maps = S.maps.at(sc);
        float* tiles = S.tiles.at(sc);
        uint32_t* words = S.words.at(sc);
        uint2* first = S.first.at(sc);
        unsigned long long* ssums = S.ssums.at(sc);
        unsigned long long* stot = S.stot.at(sc);
        if ((rc = q.launch(RM_BY_LOOP(rm_sparse_count_kernel), (uint32_t)K, rml::kQueryOwnBrick, g, level, boff, klist, tiles, maps, words,
                           evals)) != RM_OK)
            return rc;
        hipLaunchKernelGGL(rmk::rm_sparse_seg_sum_kernel, dim3(n_sblocks), dim3(256), 0, s, n_segs, words, ssums);
        unsigned long long ev = 0ull;
        if ((rc = scan_totals(c, s, ssums, n_sblocks, stot, tot, {&ev, evals, sizeof ev})) != RM_OK) return rc;
        V = tot[0];
        T = tot[1];
        n_evals += ev;
        if (V > 0xFFFFFFFFull || T > 0xFFFFFFFFull)
            return fail(c, RM_ERR_RANGE, "rm_extract_mesh_sparse: %llu vertices and %llu triangles do not fit 32-bit indices",
                        (unsigned long long)V, (unsigned long long)T);
        L = mesh_layout(V, T, flags);
        if ((rc = c->mesh.buf.reserve(c, L.bytes)) != RM_OK) return rc;
        char* m = c->mesh.buf.p;
        if (V > 0u) {
            hipLaunchKernelGGL(rmk::rm_sparse_seg_scan_kernel, dim3(n_sblocks), dim3(256), 0, s, n_segs, words, ssums, first);
            hipLaunchKernelGGL(rmk::rm_sparse_emit_kernel, dim3((uint32_t)K), dim3(256), 0, s, g, level, (uint32_t)K, boff, klist, tiles, maps, words,
                               first, L.vertices.at(m), L.triangles.at(m));
            HIP_TRY(c, hipGetLastError());
            if ((rc = point_attributes(q, flags, V, L.vertices.at(m), m, L.normals, L.ids)) != RM_OK) return rc;
        }
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    out_stats[RM_MESH_STAT_VERTICES] = V;
    out_stats[RM_MESH_STAT_TRIANGLES] = T;
    out_stats[RM_MESH_STAT_BRICKS] = g.nb;
    out_stats[RM_MESH_STAT_BRICKS_KEPT] = K;
    out_stats[RM_MESH_STAT_EVALUATIONS] = n_evals;
    out_stats[RM_MESH_STAT_SCRATCH_BYTES] = B.bytes + kept_bytes;
    c->mesh.commit(V, T, flags);
    return RM_OK;
}

// ---- mass properties (rm_mass.h) ----
RM_EXPORT int rm_mass_moments(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                              uint64_t* out_moments, uint32_t n_moments, uint64_t* out_stats, uint32_t n_stats) {
    if (!c) return RM_ERR_NULL;
    if (!out_moments || !out_stats) return fail(c, RM_ERR_NULL, "rm_mass_moments: out_moments or out_stats is NULL");
    if (n_moments < (uint32_t)RM_MOMENTS) return fail(c, RM_ERR_ARG, "rm_mass_moments: n_moments %u < RM_MOMENTS", n_moments);
    if (n_stats < (uint32_t)RM_MASS_STATS) return fail(c, RM_ERR_ARG, "rm_mass_moments: n_stats %u < RM_MASS_STATS", n_stats);
    if (int rc = check_lattice(c, "rm_mass_moments", origin, step)) return rc;
    if (int rc = check_iso(c, "rm_mass_moments", level, 0u)) return rc;
    if (nx < 2 || ny < 2 || nz < 2 || nx > kMaxMassDim || ny > kMaxMassDim || nz > kMaxMassDim)
        return fail(c, RM_ERR_RANGE, "rm_mass_moments: lattice %ux%ux%u: 2..4096 points per axis", nx, ny, nz);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    QueryCall q;
    int rc = q.begin(c, s, false, false);
    if (rc != RM_OK) return rc;
    RmProgramBound bound;
    rmk::SparseGrid g;
    if ((rc = brick_lattice(q, "rm_mass_moments", origin, step, nx, ny, nz, &bound, &g)) != RM_OK) return rc;
    if ((rc = count_bricks(c, "rm_mass_moments", &g)) != RM_OK) return rc;  // (<= 2^27 with 4096 points per axis)
    // the mesh's scratch buffers (neither holds a result): the brick tables, then the kept bricks' rows
    const uint32_t n_entries = g.nb + 1u, n_pblocks = (n_entries + 255u) / 256u;
    const rml::MassBrickTables B(n_entries, n_pblocks);
    if ((rc = c->d_mbricks.reserve(c, B.bytes)) != RM_OK) return rc;
    char* bs = c->d_mbricks.p;
    unsigned long long* evals = B.evals.at(bs);
    unsigned long long* prows = B.prows.at(bs);
    unsigned long long* result = B.result.at(bs);
    rml::MassKeptScratch S(0u);
    uint64_t tot[2] = {0u, 0u};
    rc = brick_pass(q, RM_BY_LOOP(rm_mass_probe_kernel), g, level, bound, n_entries, n_pblocks, B, bs, tot, [&](uint64_t kept, uint32_t** klist) {
        S = rml::MassKeptScratch(kept);
        if (int rrc = c->d_mscratch.reserve(c, S.bytes)) return rrc;
        *klist = S.klist.at(c->d_mscratch.p);
        return (int)RM_OK;
    }, prows);
    if (rc != RM_OK) return rc;
    const uint64_t K = tot[0], n_inside = tot[1];
    size_t kept_bytes = 0;
    const unsigned long long* krows = nullptr;
    if (K > 0u) {
        kept_bytes = S.bytes;
        char* sc = c->d_mscratch.p;
        if ((rc = q.launch(RM_BY_LOOP(rm_mass_count_kernel), (uint32_t)K, rml::kQueryOwnBrick, g, level, S.klist.at(sc), S.krows.at(sc),
                           evals)) != RM_OK)
            return rc;
        krows = S.krows.at(sc);
    }
    unsigned long long mom[RM_MOMENTS], ev = 0ull;
    if ((rc = reduce_to_row(c, s, prows, n_pblocks, krows, (uint32_t)K, result, mom, {&ev, evals, sizeof ev})) != RM_OK) return rc;
    for (int m = 0; m < RM_MOMENTS; m++) out_moments[m] = mom[m];
    out_stats[RM_MASS_STAT_BRICKS] = g.nb;
    out_stats[RM_MASS_STAT_BRICKS_KEPT] = K;
    out_stats[RM_MASS_STAT_BRICKS_INSIDE] = n_inside;
    out_stats[RM_MASS_STAT_EVALUATIONS] = g.nb + ev;
    out_stats[RM_MASS_STAT_SCRATCH_BYTES] = B.bytes + kept_bytes;
    return RM_OK;
}

RM_EXPORT int rm_mass_from_moments(const uint64_t* moments, uint32_t n_moments, const float* origin, const float* step, double density,
                                   double* out, uint32_t n_out) {
    if (!moments || !origin || !step || !out) return RM_ERR_NULL;
    if (n_moments < (uint32_t)RM_MOMENTS || n_out < (uint32_t)RM_MASS_PROPS) return RM_ERR_ARG;
    if (!std::isfinite(density)) return RM_ERR_ARG;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(origin[a]) || !std::isfinite(step[a]) || !(step[a] > 0.0f)) return RM_ERR_ARG;
    const double o[3] = {origin[0], origin[1], origin[2]}, st[3] = {step[0], step[1], step[2]};
    for (int p = 0; p < RM_MASS_PROPS; p++) out[p] = 0.0;
    const uint64_t N = moments[RM_MOMENT_COUNT];
    if (N == 0u) {
        for (int a = 0; a < 3; a++) {
            out[RM_MASS_LO_X + a] = HUGE_VAL;
            out[RM_MASS_HI_X + a] = -HUGE_VAL;
        }
        return RM_OK;
    }
    const double n = (double)N, dV = st[0] * st[1] * st[2], volume = n * dV, mass = density * volume;
    out[RM_MASS_VOLUME] = volume;
    out[RM_MASS_MASS] = mass;
    for (int a = 0; a < 3; a++) {
        out[RM_MASS_CX + a] = o[a] + st[a] * ((double)moments[RM_MOMENT_X + a] / n);
        out[RM_MASS_LO_X + a] = o[a] + (double)moments[RM_MOMENT_MIN_X + a] * st[a];
        out[RM_MASS_HI_X + a] = o[a] + (double)moments[RM_MOMENT_MAX_X + a] * st[a];
    }
#if !defined(__HIP_DEVICE_COMPILE__)
    // central second moments from exact integers: D_ab = N S_ab - S_a S_b, |D_ab| <= 2^96
    using i128 = __int128;
    const auto central = [&](int a, int b, int ab) {
        const i128 D = (i128)N * (i128)moments[ab] - (i128)moments[RM_MOMENT_X + a] * (i128)moments[RM_MOMENT_X + b];
        return st[a] * st[b] * ((double)D / (n * n));
    };
    const double mxx = central(0, 0, RM_MOMENT_XX) + st[0] * st[0] / 12.0, myy = central(1, 1, RM_MOMENT_YY) + st[1] * st[1] / 12.0,
                 mzz = central(2, 2, RM_MOMENT_ZZ) + st[2] * st[2] / 12.0;  // (+ the cell's own extent)
    out[RM_MASS_IXX] = mass * (myy + mzz);
    out[RM_MASS_IYY] = mass * (mxx + mzz);
    out[RM_MASS_IZZ] = mass * (mxx + myy);
    out[RM_MASS_IXY] = 0.0 - mass * central(0, 1, RM_MOMENT_XY);
    out[RM_MASS_IYZ] = 0.0 - mass * central(1, 2, RM_MOMENT_YZ);
    out[RM_MASS_IXZ] = 0.0 - mass * central(0, 2, RM_MOMENT_XZ);
#endif
    return RM_OK;
}

// ---- solid topology (rm_topology.h) ----
namespace {

struct TopoGrid {
    rmk::SparseGrid g;
    uint32_t n, n_pblocks, n_rblocks;
};
TopoGrid topo_grid(const rmk::SparseGrid& g) {
    TopoGrid t;
    t.g = g;
    t.g.nb = g.bx * g.by * g.bz;  // (<= 2^21 with 1024 points per axis)
    t.n = g.nx * g.ny * g.nz;     // (<= 2^28)
    t.n_pblocks = (t.g.nb + 255u) / 256u;
    t.n_rblocks = (t.n + rmk::kTopoRankBlock - 1u) / rmk::kTopoRankBlock;
    return t;
}
int check_topo_lattice(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx >= 2 && ny >= 2 && nz >= 2 && nx <= kMaxTopoDim && ny <= kMaxTopoDim && nz <= kMaxTopoDim && (uint64_t)nx * ny * nz <= kMaxTopoPoints)
        return RM_OK;
    return fail(c, RM_ERR_RANGE, "%s: lattice %ux%ux%u: 2..1024 points per axis, at most 2^28 in all", fn, nx, ny, nz);
}

// ---- the front end of the lattice analyses: labelling, distance, supports, islands, surface measures, each of a solid and of an occupancy ----
// The statistics every analysis reports first, and the size of its scratch last.
enum { kStatBricks = 0, kStatBricksKept = 1, kStatBricksInside = 2, kStatEvaluations = 3 };
#define RM_LATTICE_STATS_ASSERT(P)                                                                                             \
    static_assert(P##_STAT_BRICKS == kStatBricks && P##_STAT_BRICKS_KEPT == kStatBricksKept &&                                 \
                      P##_STAT_BRICKS_INSIDE == kStatBricksInside && P##_STAT_EVALUATIONS == kStatEvaluations &&               \
                      P##_STAT_SCRATCH_BYTES == P##_STATS - 1,                                                                 \
                  "lattice_call writes the brick statistics first and the scratch size last")
RM_LATTICE_STATS_ASSERT(RM_TOPO);
RM_LATTICE_STATS_ASSERT(RM_DIST);
RM_LATTICE_STATS_ASSERT(RM_SUP);
RM_LATTICE_STATS_ASSERT(RM_ISL);
RM_LATTICE_STATS_ASSERT(RM_SURF);
#undef RM_LATTICE_STATS_ASSERT

// Where the occupancy of a call comes from: the solid {d < level} of the program on the lattice (origin, step), or the caller's
// bytes on the unit lattice.  A scratch layout S of any analysis has the regions occ, cls, psums, ptot and evals.
struct OccupancySource {
    bool solid;
    const float *origin, *step;
    float level;
    const void* bytes;
    int is_device;
    void* stream;
    QueryCall q;  // begin's, for fill (a solid)
    RmProgramBound bound;

    static OccupancySource of_solid(const float* origin, const float* step, float level) {
        return OccupancySource{true, origin, step, level, nullptr, 0, nullptr};
    }
    static OccupancySource of_bytes(const void* occupancy, int is_device, void* stream) {
        return OccupancySource{false, kUnitOrigin, kUnitStep, 0.0f, occupancy, is_device, stream};
    }

    // Orders stream s after the context's earlier work -- a device read of the family's previous result, too -- and gives the
    // lattice in bricks; a solid: the query's launch state and the program's bounds, every check before the first launch.
    int begin(rm_ctx* c, const char* fn, hipStream_t s, uint32_t nx, uint32_t ny, uint32_t nz, rmk::SparseGrid* g) {
        if (!solid) {
            order_with_previous(c, s);
            *g = sparse_grid(origin, step, nx, ny, nz);
            return RM_OK;
        }
        int rc = q.begin(c, s, false, false);
        if (rc != RM_OK) return rc;
        return brick_lattice(q, fn, origin, step, nx, ny, nz, &bound, g);
    }

    // The occupancy into S.occ.  A solid (rm_topology.h): probe, scan of the block sums (kept low, inside high -> ptot),
    // occupancy, the evaluations of the kept bricks' points in evals[0].
    template <class S>
    int fill(rm_ctx* c, hipStream_t s, const TopoGrid& G, const S& L) const {
        char* sc = c->d_mscratch.p;
        if (!solid) {
            if (is_device) {
                // the caller's array is ready when the work queued on its stream is done; the call is synchronous anyway
                const hipStream_t su = user_stream(c, stream);
                if (su != s) HIP_TRY(c, hipStreamSynchronize(su));
            }
            HIP_TRY(c, hipMemcpyAsync(L.occ.at(sc), bytes, G.n, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
            return RM_OK;
        }
        uint8_t* cls = L.cls.at(sc);
        int rc = brick_probe(q, RM_BY_LOOP(rm_topo_probe_kernel), G.g, level, bound, G.n_pblocks, L, sc, cls);
        if (rc != RM_OK) return rc;
        return q.launch(RM_BY_LOOP(rm_topo_occupancy_kernel), G.g.nb, rml::kQueryOwnBrick, G.g, level, cls, L.occ.at(sc), L.evals.at(sc));
    }

    // The brick statistics of the fill; those of a caller's occupancy stay 0.
    template <class S>
    int brick_stats(rm_ctx* c, hipStream_t s, const TopoGrid& G, const S& L, uint64_t* stats) const {
        if (!solid) return RM_OK;
        char* sc = c->d_mscratch.p;
        uint64_t tot[2];
        unsigned long long ev = 0ull;
        if (int rc = read_totals(c, s, L.ptot.at(sc), tot, {&ev, L.evals.at(sc), sizeof ev})) return rc;
        stats[kStatBricks] = G.g.nb;
        stats[kStatBricksKept] = tot[0];
        stats[kStatBricksInside] = tot[1];
        stats[kStatEvaluations] = G.g.nb + ev;
        return RM_OK;
    }
};

// One call of an analysis A on the occupancy of `src`, on the context's own stream.  A names its outputs (kCounts, kStats and
// what rm_abi.h calls them) and gives check() of its own arguments, layout() of its scratch, reserve() of its buffers -- which
// drops the family's previous result once the scratch is reserved, not before -- and run() from the occupancy in the scratch's
// occ on, which writes the counts and what statistics are the analysis' own.
template <class A>
int lattice_call(rm_ctx* c, const char* fn, OccupancySource src, uint32_t nx, uint32_t ny, uint32_t nz, A a, uint64_t* out_counts,
                 uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    if (!c) return RM_ERR_NULL;
    if ((!src.solid && !src.bytes) || !out_counts || !out_stats)
        return fail(c, RM_ERR_NULL, "%s: %sout_counts or out_stats is NULL", fn, src.solid ? "" : "occupancy, ");
    if (n_counts < A::kCounts) return fail(c, RM_ERR_ARG, "%s: n_counts %u < %s", fn, n_counts, A::kCountsName);
    if (n_stats < A::kStats) return fail(c, RM_ERR_ARG, "%s: n_stats %u < %s", fn, n_stats, A::kStatsName);
    if (src.solid) {
        if (int rc = check_lattice(c, fn, src.origin, src.step)) return rc;
        if (int rc = check_iso(c, fn, src.level, 0u)) return rc;
    }
    if (int rc = a.check(c, fn, nx, ny, nz)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    rmk::SparseGrid g;
    int rc = src.begin(c, fn, s, nx, ny, nz, &g);
    if (rc != RM_OK) return rc;
    const TopoGrid G = topo_grid(g);
    const auto S = a.layout(G);
    if ((rc = a.reserve(c, G, S)) != RM_OK) return rc;
    if ((rc = src.fill(c, s, G, S)) != RM_OK) return rc;
    uint64_t counts[A::kCounts], stats[A::kStats] = {};
    if ((rc = a.run(c, fn, s, G, S, counts, stats)) != RM_OK) return rc;
    if ((rc = src.brick_stats(c, s, G, S, stats)) != RM_OK) return rc;
    stats[A::kStats - 1u] = S.bytes;
    for (uint32_t k = 0; k < A::kCounts; k++) out_counts[k] = counts[k];
    for (uint32_t k = 0; k < A::kStats; k++) out_stats[k] = stats[k];
    return RM_OK;
}

// From the occupancy in T.occ on: local labelling; merge, flatten and verify until no pair of neighbours has two roots; the
// exterior; the numbering; the rows, the counts and the label volume.  counts: RM_TOPO_COUNTS words.
int label_lattice(rm_ctx* c, const char* fn, hipStream_t s, const TopoGrid& G, const rml::TopoScratch& T, uint64_t* counts,
                  uint64_t* merge_passes) {
    const rmk::SparseGrid& g = G.g;
    char* sc = c->d_mscratch.p;
    uint32_t* parent = T.parent.at(sc);
    const uint8_t* occ = T.occ.at(sc);
    uint8_t* ext = T.ext.at(sc);
    unsigned long long* rows = T.rows.at(sc);
    unsigned long long* rsums = T.rsums.at(sc);
    unsigned long long* rtot = T.rtot.at(sc);
    unsigned long long* result = T.result.at(sc);
    int rc = RM_OK;
    uint32_t* labels = c->topo.labels.as<uint32_t>();
    const uint32_t point_blocks = (G.n + 255u) / 256u;
    unsigned long long row[RM_MOMENTS];
    unsigned long long* folded = T.folded.at(sc);
    hipLaunchKernelGGL(rmk::rm_topo_local_kernel, dim3(g.nb), dim3(256), 0, s, g, occ, parent);
    // A bounded host loop over a convergent process: one pass unites everything unless a union was lost, which the verification
    // after the kernel boundary (every write visible) would find.
    uint32_t passes = 0;
    for (;;) {
        passes++;
        hipLaunchKernelGGL(rmk::rm_topo_merge_kernel, dim3(g.nb), dim3(256), 0, s, g, occ, parent);
        hipLaunchKernelGGL(rmk::rm_topo_flatten_kernel, dim3(point_blocks), dim3(256), 0, s, G.n, parent);
        hipLaunchKernelGGL(rmk::rm_topo_verify_kernel, dim3(g.nb), dim3(256), 0, s, g, occ, parent, rows);
        if ((rc = reduce_rows(c, s, rows, g.nb, folded, result, row)) != RM_OK) return rc;
        if (row[4] == 0ull) break;
        if (passes == kMaxMergePasses)
            return fail(c, RM_ERR_DEVICE, "%s: %llu pairs of neighbours still have different roots after %u merge passes", fn, row[4], passes);
    }
    HIP_TRY(c, hipMemsetAsync(ext, 0, G.n, s));
    hipLaunchKernelGGL(rmk::rm_topo_exterior_kernel, dim3(g.nb), dim3(256), 0, s, g, occ, parent, ext);
    hipLaunchKernelGGL(rmk::rm_topo_root_sum_kernel, dim3(G.n_rblocks), dim3(256), 0, s, G.n, occ, parent, ext, rsums);
    uint64_t tot[2];
    if ((rc = scan_totals(c, s, rsums, G.n_rblocks, rtot, tot)) != RM_OK) return rc;
    const uint64_t B = tot[0], C = tot[1];
    const rml::TopoRows R(B, C);
    if (R.bytes > 0u) {
        if ((rc = c->topo.rows.reserve(c, R.bytes, "component rows")) != RM_OK) return rc;
        hipLaunchKernelGGL(rmk::rm_topo_rows_init_kernel, dim3((uint32_t)(((B + C) * rmk::kRowWords + 255u) / 256u)), dim3(256), 0, s,
                           (uint32_t)(B + C), R.bodies.at(c->topo.rows.p));
    }
    hipLaunchKernelGGL(rmk::rm_topo_rank_kernel, dim3(G.n_rblocks), dim3(256), 0, s, G.n, occ, parent, ext, rsums, labels);
    hipLaunchKernelGGL(rmk::rm_topo_rows_kernel, dim3(g.nb), dim3(256), 0, s, g, occ, parent, labels, (uint32_t)B, R.bodies.at(c->topo.rows.p), rows);
    if ((rc = reduce_rows(c, s, rows, g.nb, folded, result, row)) != RM_OK) return rc;
    const uint64_t V = row[0], E = row[1], F = row[2], K = row[3];
    const int64_t euler = (int64_t)V - (int64_t)E + (int64_t)F - (int64_t)K;
    counts[RM_TOPO_BODIES] = B;
    counts[RM_TOPO_CAVITIES] = C;
    counts[RM_TOPO_POINTS] = V;
    counts[RM_TOPO_EDGES] = E;
    counts[RM_TOPO_FACES] = F;
    counts[RM_TOPO_CELLS] = K;
    counts[RM_TOPO_EULER] = (uint64_t)euler;
    counts[RM_TOPO_TUNNELS] = (uint64_t)((int64_t)B + (int64_t)C - euler);
    counts[RM_TOPO_EXTERIOR_POINTS] = row[4];
    *merge_passes = passes;
    c->topo.commit(G.n, B, C);
    return RM_OK;
}

struct LabelAnalysis {
    static constexpr uint32_t kCounts = RM_TOPO_COUNTS, kStats = RM_TOPO_STATS;
    static constexpr const char *kCountsName = "RM_TOPO_COUNTS", *kStatsName = "RM_TOPO_STATS";
    int check(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz) const { return check_topo_lattice(c, fn, nx, ny, nz); }
    rml::TopoScratch layout(const TopoGrid& G) const { return rml::TopoScratch(G.n, G.g.nb, G.n_pblocks, G.n_rblocks); }
    int reserve(rm_ctx* c, const TopoGrid& G, const rml::TopoScratch& T) const {
        if (int rc = c->d_mscratch.reserve(c, T.bytes)) return rc;
        c->topo.drop();
        return c->topo.labels.reserve(c, (size_t)G.n * 4u, "label volume");
    }
    int run(rm_ctx* c, const char* fn, hipStream_t s, const TopoGrid& G, const rml::TopoScratch& T, uint64_t* counts, uint64_t* stats) const {
        return label_lattice(c, fn, s, G, T, counts, &stats[RM_TOPO_STAT_MERGE_PASSES]);
    }
};

}  // namespace

RM_EXPORT int rm_label_solid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                             uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_label_solid", OccupancySource::of_solid(origin, step, level), nx, ny, nz, LabelAnalysis(), out_counts, n_counts,
                        out_stats, n_stats);
}

RM_EXPORT int rm_label_occupancy(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                                 uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_label_occupancy", OccupancySource::of_bytes(occupancy, is_device, stream), nx, ny, nz, LabelAnalysis(), out_counts,
                        n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_read_topology(rm_ctx* c, uint64_t* out_body_moments, uint64_t* out_cavity_moments, uint32_t* out_labels, int is_device,
                               void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Labels& r = c->topo;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_topology: nothing has been labelled");
    const rml::TopoRows R(r.b, r.c);
    return read_back(c, is_device, stream, "rm_read_topology: device arrays need 8-byte alignment (out_labels: 4-byte)",
                     {{out_body_moments, R.bodies, r.rows.p, 8}, {out_cavity_moments, R.cavities, r.rows.p, 8},
                      {out_labels, r.labels.p, (size_t)r.n * 4u, 4}});
}

// ---- distance transform (rm_distance.h) ----
namespace {

struct DistBlocks {
    uint32_t n_rblocks, n_fblocks;  // rows of 2048 points, folded rows of 256 rows
    explicit DistBlocks(uint32_t n) : n_rblocks((n + rmk::kDistBlock - 1u) / rmk::kDistBlock), n_fblocks(rmk::rows_folded(n_rblocks)) {}
};

// The y and the z pass over `vol` (rm_dist_column_kernel): a launch each.
template <bool SINGLE>
int dist_columns(rm_ctx* c, hipStream_t s, const rmk::SparseGrid& g, uint32_t none, uint32_t* vol) {
    const auto kernel = rmk::rm_dist_column_kernel<SINGLE>;
    const uint32_t axes[2][3] = {{g.ny, g.nx, g.nx * g.ny}, {g.nz, g.nx * g.ny, g.nx}};  // points, stride, outer stride
    const uint32_t slabs[2] = {g.nz, g.ny};
    for (int a = 0; a < 2; a++) {
        const uint32_t n = axes[a][0], xl = rml::dist_columns_log2(n), xt = 1u << xl;
        const uint32_t shmem = rml::DistColumnLds(xt, n).bytes;
        if (shmem + 1024u > rml::kLdsLaunchLimit)
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(kernel, dim3((g.nx + xt - 1u) / xt, slabs[a]), dim3(256), shmem, s, g.nx, n, axes[a][1], axes[a][2], xl, none, vol);
    }
    HIP_TRY(c, hipGetLastError());
    return RM_OK;
}

// From the occupancy in S.occ on: rows, columns, maxima.  counts: RM_DIST_COUNTS words.
int distance_lattice(rm_ctx* c, hipStream_t s, const TopoGrid& G, const rml::DistScratch& S, uint64_t* counts) {
    const rmk::SparseGrid& g = G.g;
    char* sc = c->d_mscratch.p;
    uint32_t* vol = c->dist.vol.as<uint32_t>();
    const DistBlocks D(G.n);
    const uint32_t n_rows = g.ny * g.nz;
    hipLaunchKernelGGL(rmk::rm_dist_row_kernel<rmk::DIST_FROM_OCCUPANCY>, dim3((n_rows + 3u) / 4u), dim3(256), 0, s, g.nx, n_rows, S.occ.at(sc),
                       nullptr, 0u, vol);
    if (int rc = dist_columns<false>(c, s, g, rmk::kDistNone, vol)) return rc;
    hipLaunchKernelGGL(rmk::rm_dist_max_kernel, dim3(D.n_rblocks), dim3(256), 0, s, G.n, vol, S.rows.at(sc));
    unsigned long long row[RM_MOMENTS];
    if (int rc = reduce_rows(c, s, S.rows.at(sc), D.n_rblocks, S.folded.at(sc), S.result.at(sc), row)) return rc;
    counts[RM_DIST_POINTS] = row[0];
    counts[RM_DIST_MAX_INSIDE] = row[13] >> 32;
    counts[RM_DIST_ARGMAX_INSIDE] = ~row[13] & 0xFFFFFFFFull;
    counts[RM_DIST_MAX_OUTSIDE] = row[14] >> 32;
    counts[RM_DIST_ARGMAX_OUTSIDE] = ~row[14] & 0xFFFFFFFFull;
    c->dist.commit(g.nx, g.ny, g.nz);
    return RM_OK;
}

struct DistanceAnalysis {
    static constexpr uint32_t kCounts = RM_DIST_COUNTS, kStats = RM_DIST_STATS;
    static constexpr const char *kCountsName = "RM_DIST_COUNTS", *kStatsName = "RM_DIST_STATS";
    int check(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz) const { return check_topo_lattice(c, fn, nx, ny, nz); }
    rml::DistScratch layout(const TopoGrid& G) const {
        const DistBlocks D(G.n);
        return rml::DistScratch(G.n, G.g.nb, G.n_pblocks, D.n_rblocks, D.n_fblocks);
    }
    int reserve(rm_ctx* c, const TopoGrid& G, const rml::DistScratch& S) const {
        if (int rc = c->d_mscratch.reserve(c, S.bytes)) return rc;
        c->dist.drop();  // (the mask of the previous volume with it)
        return c->dist.vol.reserve(c, (size_t)G.n * 4u, "distance volume");
    }
    int run(rm_ctx* c, const char*, hipStream_t s, const TopoGrid& G, const rml::DistScratch& S, uint64_t* counts, uint64_t*) const {
        return distance_lattice(c, s, G, S, counts);
    }
};

}  // namespace

RM_EXPORT int rm_distance_solid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                                uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_distance_solid", OccupancySource::of_solid(origin, step, level), nx, ny, nz, DistanceAnalysis(), out_counts,
                        n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_distance_occupancy(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                                    uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_distance_occupancy", OccupancySource::of_bytes(occupancy, is_device, stream), nx, ny, nz, DistanceAnalysis(),
                        out_counts, n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_distance_features(rm_ctx* c, uint32_t r2_wall, uint32_t r2_gap, uint64_t* out_counts, uint32_t n_counts) {
    if (!c) return RM_ERR_NULL;
    if (!out_counts) return fail(c, RM_ERR_NULL, "rm_distance_features: out_counts is NULL");
    if (n_counts < (uint32_t)RM_DIST_FEATURE_COUNTS)
        return fail(c, RM_ERR_ARG, "rm_distance_features: n_counts %u < RM_DIST_FEATURE_COUNTS", n_counts);
    if (!c->dist.valid) return fail(c, RM_ERR_ARG, "rm_distance_features: no distance volume has been computed");
    if ((r2_wall != RM_DIST_SKIP && r2_wall >= kMaxDistR2) || (r2_gap != RM_DIST_SKIP && r2_gap >= kMaxDistR2))
        return fail(c, RM_ERR_RANGE, "rm_distance_features: r2_wall %u, r2_gap %u: below 2^22, or RM_DIST_SKIP", r2_wall, r2_gap);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a device read of the last mask, too
    const TopoGrid G = topo_grid(sparse_grid(kUnitOrigin, kUnitStep, c->dist.nx, c->dist.ny, c->dist.nz));
    const rmk::SparseGrid& g = G.g;
    const DistBlocks D(G.n);
    const rml::DistFeatureScratch S(G.n, D.n_rblocks, D.n_fblocks);
    int rc = c->d_mscratch.reserve(c, S.bytes);
    if (rc != RM_OK) return rc;
    c->dist.mask.drop();
    if ((rc = c->dist.mask.buf.reserve(c, G.n, "feature mask")) != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    const uint32_t* vol = c->dist.vol.as<uint32_t>();
    uint8_t* mask = c->dist.mask.buf.as<uint8_t>();
    uint32_t* feat = S.feat.at(sc);
    const uint32_t n_rows = g.ny * g.nz;
    hipLaunchKernelGGL(rmk::rm_dist_mask_init_kernel, dim3((G.n + 255u) / 256u), dim3(256), 0, s, G.n, vol, mask);
    uint64_t counts[RM_DIST_FEATURE_COUNTS] = {0u, 0u, 0u, 0u};
    unsigned long long row[RM_MOMENTS];
    if (r2_wall != RM_DIST_SKIP) {
        hipLaunchKernelGGL(rmk::rm_dist_row_kernel<rmk::DIST_FROM_WALL_CORE>, dim3((n_rows + 3u) / 4u), dim3(256), 0, s, g.nx, n_rows, nullptr, vol,
                           r2_wall, feat);
        if ((rc = dist_columns<true>(c, s, g, r2_wall + 1u, feat)) != RM_OK) return rc;
        hipLaunchKernelGGL((rmk::rm_dist_compose_kernel<1u, 2u>), dim3(D.n_rblocks), dim3(256), 0, s, G.n, vol, feat, r2_wall, mask, S.rows.at(sc));
        if ((rc = reduce_rows(c, s, S.rows.at(sc), D.n_rblocks, S.folded.at(sc), S.result.at(sc), row)) != RM_OK) return rc;
        counts[RM_DIST_CORE] = row[0];
        counts[RM_DIST_THIN] = row[1];
    }
    if (r2_gap != RM_DIST_SKIP) {
        hipLaunchKernelGGL(rmk::rm_dist_row_kernel<rmk::DIST_FROM_GAP_CORE>, dim3((n_rows + 3u) / 4u), dim3(256), 0, s, g.nx, n_rows, nullptr, vol,
                           r2_gap, feat);
        if ((rc = dist_columns<true>(c, s, g, r2_gap + 1u, feat)) != RM_OK) return rc;
        hipLaunchKernelGGL((rmk::rm_dist_compose_kernel<0u, 3u>), dim3(D.n_rblocks), dim3(256), 0, s, G.n, vol, feat, r2_gap, mask, S.rows.at(sc));
        if ((rc = reduce_rows(c, s, S.rows.at(sc), D.n_rblocks, S.folded.at(sc), S.result.at(sc), row)) != RM_OK) return rc;
        counts[RM_DIST_GAP_CORE] = row[0];
        counts[RM_DIST_NARROW] = row[1];
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    for (int k = 0; k < RM_DIST_FEATURE_COUNTS; k++) out_counts[k] = counts[k];
    c->dist.mask.commit();
    return RM_OK;
}

RM_EXPORT int rm_read_distance(rm_ctx* c, uint32_t* out_d2, void* out_mask, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Distance& r = c->dist;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_distance: no distance volume has been computed");
    if (out_mask && !r.mask.valid) return fail(c, RM_ERR_ARG, "rm_read_distance: rm_distance_features has made no mask of this volume");
    return read_back(c, is_device, stream, "rm_read_distance: a device out_d2 needs 4-byte alignment",
                     {{out_d2, r.vol.p, r.points() * 4u, 4}, {out_mask, r.mask.buf.p, r.points(), 1}});
}

// ---- overhangs and supports (rm_support.h) ----
namespace {

static_assert(rmk::kSupPlateAuto == RM_SUPPORT_PLATE_AUTO, "the automatic plate");
static_assert(rml::kSupMaxWords * 64u == kMaxTopoDim, "a bit row holds the longest axis");
static_assert(rml::kSupMaxReach * rml::kSupMaxReach <= rml::kSupMaxR2 && (rml::kSupMaxReach + 1u) * (rml::kSupMaxReach + 1u) > rml::kSupMaxR2,
              "the halo of the overhang tile is floor(sqrt(r2))");

// The canonical frame (rm_support.h) of a lattice for a build direction.
rmk::SupFrame sup_frame(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t up) {
    rmk::SupFrame f;
    switch (up >> 1) {
    case 0: f = rmk::SupFrame{ny, nz, nx, 0u, nx, nx * ny, 1u, 0u}; break;   // x up: the bits run along y
    case 1: f = rmk::SupFrame{nx, nz, ny, 0u, 1u, nx * ny, nx, 0u}; break;   // y up
    default: f = rmk::SupFrame{nx, ny, nz, 0u, 1u, nx, nx * ny, 0u}; break;  // z up
    }
    f.nw = (f.nu + 63u) / 64u;
    f.neg = up & 1u;
    return f;
}
uint32_t sup_plane_words(const rmk::SupFrame& f) { return f.nh * f.nv * f.nw; }  // (<= 2^28 / 64 * 2: a 65th point costs a whole word)

// The argument checks the two support calls share, after those of their outputs and their lattice's values.
int check_support(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t up, uint32_t r2, uint32_t plate) {
    if (up > (uint32_t)RM_UP_NEG_Z) return fail(c, RM_ERR_ARG, "%s: up %u is not one of RM_UP_*", fn, up);
    if (int rc = check_topo_lattice(c, fn, nx, ny, nz)) return rc;
    if (r2 > rml::kSupMaxR2) return fail(c, RM_ERR_RANGE, "%s: r2 %u: a squared reach is 0..255", fn, r2);
    const uint32_t nh = sup_frame(nx, ny, nz, up).nh;
    if (plate != RM_SUPPORT_PLATE_AUTO && plate >= nh)
        return fail(c, RM_ERR_RANGE, "%s: plate %u: a height of 0..%u, or RM_SUPPORT_PLATE_AUTO", fn, plate, nh - 1u);
    return RM_OK;
}

// A wave's tasks in pack and compose: four words each, or with x up (the kernels' template argument) one (row, word) and 64 layers.
struct SupTasks {
    bool xup;
    uint32_t n;
    dim3 grid;
    explicit SupTasks(const rmk::SupFrame& f) : xup(f.sh == 1u), n(xup ? f.nv * f.nw * ((f.nh + 63u) / 64u) : sup_plane_words(f)) {
        const uint32_t n_waves = xup ? n : (n + rmk::kSupWordsPerWave - 1u) / rmk::kSupWordsPerWave;
        grid = dim3((n_waves + 3u) / 4u);
    }
};
// floor(sqrt(r2)): the halo, in points, of a squared reach.
uint32_t sup_reach(uint32_t r2) {
    uint32_t reach = 0u;
    while ((reach + 1u) * (reach + 1u) <= r2) reach++;
    return reach;
}
// The plate's height: the caller's, or what the pack kernel found for RM_SUPPORT_PLATE_AUTO (h0: its word; no inside point: 0).
uint32_t sup_plate_height(uint32_t plate, uint32_t h0) { return plate != RM_SUPPORT_PLATE_AUTO ? plate : h0 == RM_SUPPORT_PLATE_AUTO ? 0u : h0; }

// The planes `ins` and `ov` of an occupancy (rm_support.h pack and overhang); h0w: the automatic plate's word, 0xFF.. before.
void support_planes(hipStream_t s, const rmk::SupFrame& f, uint32_t r2, uint32_t plate, const uint8_t* occ, unsigned long long* ins,
                    unsigned long long* ov, uint32_t* h0w) {
    const SupTasks tasks(f);
    if (tasks.xup)
        hipLaunchKernelGGL(rmk::rm_sup_pack_kernel<true>, tasks.grid, dim3(256), 0, s, f, tasks.n, plate, occ, ins, h0w);
    else
        hipLaunchKernelGGL(rmk::rm_sup_pack_kernel<false>, tasks.grid, dim3(256), 0, s, f, tasks.n, plate, occ, ins, h0w);
    const uint32_t reach = sup_reach(r2), tv = rml::sup_tile_rows(f.nw);
    hipLaunchKernelGGL(rmk::rm_sup_overhang_kernel, dim3((f.nv + tv - 1u) / tv, f.nh), dim3(256), rml::SupCoverLds(tv, reach, f.nw).bytes, s, f.nv,
                       f.nw, tv, r2, reach, plate, h0w, ins, ov);
}

// From the occupancy in S.occ on: pack, overhang, columns, count, compose; the profile summed on the host (at most 1024 layers of
// six words).  counts: RM_SUP_COUNTS words.
int support_lattice(rm_ctx* c, hipStream_t s, const TopoGrid& G, const rmk::SupFrame& f, const rml::SupportScratch& S, uint32_t r2,
                    uint32_t plate, uint64_t* counts) {
    char* sc = c->d_mscratch.p;
    const rml::SupportProfile R(f.nh);
    char* pr = c->sup.profile.p;
    uint8_t* mask = c->sup.mask.as<uint8_t>();
    unsigned long long *ins = S.ins.at(sc), *ov = S.ov.at(sc), *sup = S.sup.at(sc), *plt = S.plt.at(sc);
    uint32_t* h0w = S.plate.at(sc);
    const uint32_t ncw = f.nv * f.nw;
    const SupTasks tasks(f);
    HIP_TRY(c, hipMemsetAsync(h0w, 0xFF, 16, s));
    HIP_TRY(c, hipMemsetAsync(pr, 0, R.bytes, s));
    const uint8_t* occ = S.occ.at(sc);
    support_planes(s, f, r2, plate, occ, ins, ov, h0w);
    hipLaunchKernelGGL(rmk::rm_sup_columns_kernel, dim3((ncw + rmk::kSupColumnThreads - 1u) / rmk::kSupColumnThreads), dim3(rmk::kSupColumnThreads),
                       0, s, ncw, f.nh, plate, h0w, ins, ov, sup, plt);
    hipLaunchKernelGGL(rmk::rm_sup_count_kernel, dim3((ncw + 255u) / 256u, f.nh), dim3(256), 0, s, ncw, f.nh, plate, h0w, ins, ov, sup, plt,
                       R.profile.at(pr), R.extra.at(pr));
    if (tasks.xup)
        hipLaunchKernelGGL(rmk::rm_sup_compose_kernel<true>, tasks.grid, dim3(256), 0, s, f, tasks.n, ins, ov, sup, plt, mask);
    else
        hipLaunchKernelGGL(rmk::rm_sup_compose_kernel<false>, tasks.grid, dim3(256), 0, s, f, tasks.n, ins, ov, sup, plt, mask);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> rows((size_t)f.nh * 6u);
    uint32_t h0 = 0u;
    HIP_TRY(c, hipMemcpyAsync(rows.data(), R.profile.at(pr), (size_t)f.nh * 16u, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(rows.data() + (size_t)f.nh * 4u, R.extra.at(pr), (size_t)f.nh * 8u, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&h0, h0w, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    h0 = sup_plate_height(plate, h0);
    for (int k = 0; k < RM_SUP_COUNTS; k++) counts[k] = 0u;
    for (uint32_t h = 0; h < f.nh; h++) {
        counts[RM_SUP_POINTS] += rows[4u * h];
        counts[RM_SUP_OVERHANG] += rows[4u * h + 1u];
        counts[RM_SUP_SUPPORT_ON_PLATE] += rows[4u * h + 2u];
        counts[RM_SUP_SUPPORT_ON_PART] += rows[4u * h + 3u];
        counts[RM_SUP_RUNS] += rows[4u * f.nh + 2u * h];
        counts[RM_SUP_LANDINGS] += rows[4u * f.nh + 2u * h + 1u];
    }
    counts[RM_SUP_PLATE] = h0;
    counts[RM_SUP_BASE] = rows[4u * h0];
    c->sup.commit(G.n, f.nh);
    return RM_OK;
}

// The arguments of the analyses with a build direction, and their frame (layout() sets it).
struct DirectedAnalysis {
    uint32_t up, r2, plate;
    rmk::SupFrame f;
    DirectedAnalysis(uint32_t up_, uint32_t r2_, uint32_t plate_) : up(up_), r2(r2_), plate(plate_), f() {}
    int check(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz) const { return check_support(c, fn, nx, ny, nz, up, r2, plate); }
};

struct SupportAnalysis : DirectedAnalysis {
    using DirectedAnalysis::DirectedAnalysis;
    static constexpr uint32_t kCounts = RM_SUP_COUNTS, kStats = RM_SUP_STATS;
    static constexpr const char *kCountsName = "RM_SUP_COUNTS", *kStatsName = "RM_SUP_STATS";
    rml::SupportScratch layout(const TopoGrid& G) {
        f = sup_frame(G.g.nx, G.g.ny, G.g.nz, up);
        return rml::SupportScratch(G.n, G.g.nb, G.n_pblocks, sup_plane_words(f));
    }
    int reserve(rm_ctx* c, const TopoGrid& G, const rml::SupportScratch& S) const {
        if (int rc = c->d_mscratch.reserve(c, S.bytes)) return rc;
        c->sup.drop();
        if (int rc = c->sup.mask.reserve(c, G.n, "support mask")) return rc;
        return c->sup.profile.reserve(c, rml::SupportProfile(f.nh).bytes, "support profile");
    }
    int run(rm_ctx* c, const char*, hipStream_t s, const TopoGrid& G, const rml::SupportScratch& S, uint64_t* counts, uint64_t*) const {
        return support_lattice(c, s, G, f, S, r2, plate, counts);
    }
};

}  // namespace

RM_EXPORT int rm_support_solid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                               uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                               uint32_t n_stats) {
    return lattice_call(c, "rm_support_solid", OccupancySource::of_solid(origin, step, level), nx, ny, nz, SupportAnalysis(up, r2, plate),
                        out_counts, n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_support_occupancy(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                                   uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                                   uint32_t n_stats) {
    return lattice_call(c, "rm_support_occupancy", OccupancySource::of_bytes(occupancy, is_device, stream), nx, ny, nz,
                        SupportAnalysis(up, r2, plate), out_counts, n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_read_support(rm_ctx* c, void* out_mask, uint32_t* out_profile, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Support& r = c->sup;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_support: no support call has been made");
    return read_back(c, is_device, stream, "rm_read_support: a device out_profile needs 4-byte alignment",
                     {{out_mask, r.mask.p, r.n, 1}, {out_profile, rml::SupportProfile(r.nh).profile.at(r.profile.p), (size_t)r.nh * 16u, 4}});
}

// ---- layer regions and islands (rm_islands.h) ----
namespace {

static_assert(rmk::kIslRowWords == RM_ISL_ROW_WORDS && rml::kIslRowWords == RM_ISL_ROW_WORDS, "a row of the region table");
static_assert(rmk::kIslLayer == RM_ISL_ROW_LAYER && rmk::kIslFirst == RM_ISL_ROW_FIRST && rmk::kIslPoints == RM_ISL_ROW_POINTS &&
                  rmk::kIslSupported == RM_ISL_ROW_SUPPORTED && rmk::kIslSumA == RM_ISL_ROW_SUM_A && rmk::kIslSumB == RM_ISL_ROW_SUM_B &&
                  rmk::kIslMinA == RM_ISL_ROW_MIN_A && rmk::kIslMaxA == RM_ISL_ROW_MAX_A && rmk::kIslMinB == RM_ISL_ROW_MIN_B &&
                  rmk::kIslMaxB == RM_ISL_ROW_MAX_B && rmk::kIslBelowMin == RM_ISL_ROW_BELOW_MIN && rmk::kIslBelowMax == RM_ISL_ROW_BELOW_MAX,
              "the words of a row");
static_assert(rml::IslLinkLds(rml::kSupMaxReach).bytes + 256u <= rml::kLdsLaunchLimit, "the links tile fits a workgroup");

// The plane words and the blocks of 256 points of an islands call.
struct IslandsPlan {
    uint32_t n_words, n_rblocks;
    IslandsPlan(const TopoGrid& G, const rmk::SupFrame& f) : n_words(sup_plane_words(f)), n_rblocks((G.n + 255u) / 256u) {}
};

// From the occupancy in S.occ on (rm_islands.h): pack, overhang, local, border, roots, scan; the table; rank, spread, rows, links,
// finish, compose; the profile summed on the host (at most 1024 layers of four words).  counts: RM_ISL_COUNTS words.
int islands_lattice(rm_ctx* c, hipStream_t s, const TopoGrid& G, const rmk::SupFrame& f, const rml::IslandsScratch& S, uint32_t up, uint32_t r2,
                    uint32_t plate, uint64_t* counts) {
    const IslandsPlan P(G, f);
    char* sc = c->d_mscratch.p;
    unsigned long long *ins = S.ins.at(sc), *ov = S.ov.at(sc), *rsums = S.rsums.at(sc), *rtot = S.rtot.at(sc);
    uint32_t *h0w = S.plate.at(sc), *parent = S.parent.at(sc), *lab = S.lab.at(sc), *lbase = S.lbase.at(sc), *totals = S.totals.at(sc);
    uint32_t* prof = c->isl.profile.as<uint32_t>();
    HIP_TRY(c, hipMemsetAsync(h0w, 0xFF, 16, s));
    HIP_TRY(c, hipMemsetAsync(totals, 0, 16, s));
    HIP_TRY(c, hipMemsetAsync(prof, 0, (size_t)f.nh * 16u, s));
    support_planes(s, f, r2, plate, S.occ.at(sc), ins, ov, h0w);
    const uint32_t reach = sup_reach(r2), ncw = f.nv * f.nw;
    hipLaunchKernelGGL(rmk::rm_isl_local_kernel, dim3(f.nw, (f.nv + rml::kIslTile - 1u) / rml::kIslTile, f.nh), dim3(64), rml::IslTileLds().bytes, s,
                       f, plate, h0w, ins, parent);
    hipLaunchKernelGGL(rmk::rm_isl_border_kernel, dim3((P.n_words + 255u) / 256u), dim3(256), 0, s, f, P.n_words, G.n, plate, h0w, ins, parent);
    hipLaunchKernelGGL(rmk::rm_isl_roots_kernel, dim3(P.n_rblocks), dim3(256), 0, s, f, G.n, plate, h0w, ins, parent, rsums);
    uint64_t tot[2];
    if (int rc = scan_totals(c, s, rsums, P.n_rblocks, rtot, tot)) return rc;
    const uint64_t R = tot[0];  // (<= 2^27: no two neighbours are both roots)
    const rml::IslandsRows T(R);
    uint32_t* rows = nullptr;
    if (R != 0u) {
        if (int rc = c->isl.rows.reserve(c, T.bytes, "region table")) return rc;
        rows = T.rows.at(c->isl.rows.p);
        hipLaunchKernelGGL(rmk::rm_isl_rows_init_kernel, dim3((uint32_t)((R * rmk::kIslRowWords + 255u) / 256u)), dim3(256), 0, s,
                           (uint32_t)(R * rmk::kIslRowWords), rows);
    }
    hipLaunchKernelGGL(rmk::rm_isl_rank_kernel, dim3(P.n_rblocks), dim3(256), 0, s, f, G.n, plate, h0w, ins, parent, rsums, lab, rows, lbase);
    hipLaunchKernelGGL(rmk::rm_isl_spread_kernel, dim3(P.n_rblocks), dim3(256), 0, s, f, G.n, plate, h0w, ins, parent, lab);
    hipLaunchKernelGGL(rmk::rm_isl_rows_kernel, dim3((ncw + 255u) / 256u, f.nh), dim3(256), 0, s, f, plate, h0w, ins, ov, lab, rows, prof);
    if (R != 0u)
        hipLaunchKernelGGL(rmk::rm_isl_links_kernel, dim3(f.nw, (f.nv + rml::kIslLinkRows - 1u) / rml::kIslLinkRows, f.nh), dim3(256),
                           rml::IslLinkLds(reach).bytes, s, f, r2, reach, plate, h0w, ins, ov, lab, rows);
    hipLaunchKernelGGL(rmk::rm_isl_finish_kernel, dim3((uint32_t)((std::max<uint64_t>(R, f.nh) + 255u) / 256u)), dim3(256), 0, s, (uint32_t)R, f.nh,
                       plate, h0w, lbase, rows, prof, totals);
    hipLaunchKernelGGL(rmk::rm_isl_compose_kernel, dim3(P.n_rblocks), dim3(256), 0, s, f, up >> 1, G.g.nx, G.g.ny, G.n, plate, h0w, ins, lab, rows,
                       c->isl.labels.as<uint32_t>(), c->isl.mask.as<uint8_t>());
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> layers((size_t)f.nh * 4u);
    uint32_t h0 = 0u, merges = 0u;
    HIP_TRY(c, hipMemcpyAsync(layers.data(), prof, (size_t)f.nh * 16u, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&h0, h0w, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&merges, totals, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    h0 = sup_plate_height(plate, h0);
    for (int k = 0; k < RM_ISL_COUNTS; k++) counts[k] = 0u;
    for (uint32_t h = 0; h < f.nh; h++) {
        counts[RM_ISL_POINTS] += layers[4u * h];
        counts[RM_ISL_ISLANDS] += layers[4u * h + 2u];
        counts[RM_ISL_ISLAND_POINTS] += layers[4u * h + 3u];
        counts[RM_ISL_MAX_LAYER_REGIONS] = std::max<uint64_t>(counts[RM_ISL_MAX_LAYER_REGIONS], layers[4u * h + 1u]);
    }
    counts[RM_ISL_PLATE] = h0;
    counts[RM_ISL_REGIONS] = R;
    counts[RM_ISL_BASE_REGIONS] = layers[4u * h0 + 1u];
    counts[RM_ISL_MERGES] = merges;
    c->isl.commit(G.n, f.nh, R);
    return RM_OK;
}

struct IslandsAnalysis : DirectedAnalysis {
    using DirectedAnalysis::DirectedAnalysis;
    static constexpr uint32_t kCounts = RM_ISL_COUNTS, kStats = RM_ISL_STATS;
    static constexpr const char *kCountsName = "RM_ISL_COUNTS", *kStatsName = "RM_ISL_STATS";
    rml::IslandsScratch layout(const TopoGrid& G) {
        f = sup_frame(G.g.nx, G.g.ny, G.g.nz, up);
        const IslandsPlan P(G, f);
        return rml::IslandsScratch(G.n, G.g.nb, G.n_pblocks, P.n_words, P.n_rblocks, f.nh);
    }
    int reserve(rm_ctx* c, const TopoGrid& G, const rml::IslandsScratch& S) const {  // (the region table follows the count)
        if (int rc = c->d_mscratch.reserve(c, S.bytes)) return rc;
        c->isl.drop();
        if (int rc = c->isl.labels.reserve(c, (size_t)G.n * 4u, "region labels")) return rc;
        if (int rc = c->isl.mask.reserve(c, G.n, "island mask")) return rc;
        return c->isl.profile.reserve(c, (size_t)f.nh * 16u, "region profile");
    }
    int run(rm_ctx* c, const char*, hipStream_t s, const TopoGrid& G, const rml::IslandsScratch& S, uint64_t* counts, uint64_t*) const {
        return islands_lattice(c, s, G, f, S, up, r2, plate, counts);
    }
};

}  // namespace

RM_EXPORT int rm_islands_solid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                               uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                               uint32_t n_stats) {
    return lattice_call(c, "rm_islands_solid", OccupancySource::of_solid(origin, step, level), nx, ny, nz, IslandsAnalysis(up, r2, plate),
                        out_counts, n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_islands_occupancy(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                                   uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                                   uint32_t n_stats) {
    return lattice_call(c, "rm_islands_occupancy", OccupancySource::of_bytes(occupancy, is_device, stream), nx, ny, nz,
                        IslandsAnalysis(up, r2, plate), out_counts, n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_read_islands(rm_ctx* c, uint32_t* out_rows, uint64_t row_capacity, uint32_t* out_labels, void* out_mask,
                              uint32_t* out_profile, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Islands& r = c->isl;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_islands: no islands call has been made");
    if (out_rows && row_capacity < r.regions)
        return fail(c, RM_ERR_RANGE, "rm_read_islands: row_capacity %llu < %llu regions", (unsigned long long)row_capacity,
                    (unsigned long long)r.regions);
    return read_back(c, is_device, stream, "rm_read_islands: device out_rows, out_labels and out_profile need 4-byte alignment",
                     {{out_rows, rml::IslandsRows(r.regions).rows, r.rows.p, 4}, {out_labels, r.labels.p, (size_t)r.n * 4u, 4},
                      {out_mask, r.mask.p, r.n, 1}, {out_profile, r.profile.p, (size_t)r.nh * 16u, 4}});
}

// ---- surface measures (rm_surface.h) ----
namespace {

static_assert(RM_SURF_COUNTS == (int)rml::kSurfCounts && RM_SURF_COUNTS == (int)rml::kSurfRowWords && RM_SURF_CLASSES == (int)rmk::kSurfClasses &&
                  RM_SURF_DIRS == (int)rmk::kSurfDirs && RM_SURF_PAIR(0, 0, 0) == (int)rmk::kSurfPairs && RM_SURF_PAIR(7, 7, 12) == RM_SURF_COUNTS - 1,
              "rm_abi.h's layout of out_counts is the kernel's table");

// The tiles of the padded lattice and the workgroups that walk them.
struct SurfTiles {
    uint32_t tx, ty, tz, n_tiles, groups;
    explicit SurfTiles(const rmk::SparseGrid& g)
        : tx(rml::surf_tiles(g.nx, rml::kSurfTileX)), ty(rml::surf_tiles(g.ny, rml::kSurfTileY)), tz(rml::surf_tiles(g.nz, rml::kSurfTileZ)),
          n_tiles(tx * ty * tz), groups(std::min(n_tiles, rml::kSurfMaxGroups)) {}  // (<= 17 * 65 * 129 tiles)
};

struct SurfaceAnalysis {
    static constexpr uint32_t kCounts = RM_SURF_COUNTS, kStats = RM_SURF_STATS;
    static constexpr const char *kCountsName = "RM_SURF_COUNTS", *kStatsName = "RM_SURF_STATS";
    int check(rm_ctx* c, const char* fn, uint32_t nx, uint32_t ny, uint32_t nz) const { return check_topo_lattice(c, fn, nx, ny, nz); }
    rml::SurfScratch layout(const TopoGrid& G) const { return rml::SurfScratch(G.n, G.g.nb, G.n_pblocks, SurfTiles(G.g).groups); }
    int reserve(rm_ctx* c, const TopoGrid&, const rml::SurfScratch& S) const { return c->d_mscratch.reserve(c, S.bytes); }  // (nothing retained)
    // From the classes in S.occ on: one row per workgroup, the rows' sums.  A workgroup counts at most its tiles' owners per bin:
    // ceil(n_tiles / groups) * 8192 < 2^32.
    int run(rm_ctx* c, const char*, hipStream_t s, const TopoGrid& G, const rml::SurfScratch& S, uint64_t* counts, uint64_t*) const {
        const rmk::SparseGrid& g = G.g;
        char* sc = c->d_mscratch.p;
        const SurfTiles T(g);
        constexpr rml::SurfTileLds L;
        static_assert(L.bytes + 1024u <= rml::kLdsLaunchLimit, "a tile and its table fit a workgroup's LDS");
        hipLaunchKernelGGL(rmk::rm_surf_count_kernel, dim3(T.groups), dim3(256), L.bytes, s, g.nx, g.ny, g.nz, T.tx, T.ty, T.n_tiles, S.occ.at(sc),
                           S.rows.at(sc));
        hipLaunchKernelGGL(rmk::rm_surf_reduce_kernel, dim3(rml::kSurfCounts / 8u), dim3(256), 0, s, S.rows.at(sc), T.groups, S.result.at(sc));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(counts, S.result.at(sc), sizeof(uint64_t) * RM_SURF_COUNTS, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        uint64_t others = 0u;
        for (int a = 1; a < RM_SURF_CLASSES; a++) others += counts[RM_SURF_POINTS + a];
        counts[RM_SURF_POINTS] = (uint64_t)G.n - others;
        return RM_OK;
    }
};

// The direction weights of AREA: the fraction of the sphere nearer to +-nu than to any other of the 26 directions, for an axis, a
// face diagonal and a space diagonal (tools/surface_weights.py derives them in closed form; 3 w1 + 6 w2 + 4 w3 = 1).
constexpr double kSurfWeight[3] = {0.091555782409523431, 0.073961255752150262, 0.070391279564633452};

}  // namespace

RM_EXPORT int rm_surface_solid(rm_ctx* c, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                               uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_surface_solid", OccupancySource::of_solid(origin, step, level), nx, ny, nz, SurfaceAnalysis(), out_counts,
                        n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_surface_classes(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                                 uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    return lattice_call(c, "rm_surface_classes", OccupancySource::of_bytes(classes, is_device, stream), nx, ny, nz, SurfaceAnalysis(), out_counts,
                        n_counts, out_stats, n_stats);
}

RM_EXPORT int rm_surface_directions(int* out, uint32_t n_out) {
    if (!out) return RM_ERR_NULL;
    if (n_out < 3u * (uint32_t)RM_SURF_DIRS) return RM_ERR_ARG;
    for (uint32_t d = 0; d < (uint32_t)RM_SURF_DIRS; d++) {
        const rmk::SurfDir nu = rmk::surf_dir(d);
        out[3u * d] = nu.x;
        out[3u * d + 1u] = nu.y;
        out[3u * d + 2u] = nu.z;
    }
    return RM_OK;
}

RM_EXPORT int rm_surface_measures(const uint64_t* counts, uint32_t n_counts, const float* step, uint32_t mask_a, uint32_t mask_b, double* out,
                                  uint32_t n_out) {
    if (!counts || !step || !out) return RM_ERR_NULL;
    if (n_counts < (uint32_t)RM_SURF_COUNTS || n_out < (uint32_t)RM_SURF_MEASURES) return RM_ERR_ARG;
    const uint32_t all = (1u << RM_SURF_CLASSES) - 1u;
    if (mask_a == 0u || mask_b == 0u || (mask_a & mask_b) != 0u || ((mask_a | mask_b) & ~all) != 0u) return RM_ERR_ARG;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(step[a]) || !(step[a] > 0.0f)) return RM_ERR_ARG;
    const double st[3] = {step[0], step[1], step[2]};
    // from[nu]: the pairs that lead from A into B along +nu; back[nu]: from B into A
    uint64_t from[RM_SURF_DIRS] = {}, back[RM_SURF_DIRS] = {};
    for (uint32_t a = 0; a < (uint32_t)RM_SURF_CLASSES; a++)
        for (uint32_t b = 0; b < (uint32_t)RM_SURF_CLASSES; b++)
            if (((mask_a >> a) & 1u) != 0u && ((mask_b >> b) & 1u) != 0u)
                for (uint32_t d = 0; d < (uint32_t)RM_SURF_DIRS; d++) {
                    from[d] += counts[RM_SURF_PAIR(a, b, d)];
                    back[d] += counts[RM_SURF_PAIR(b, a, d)];
                }
    double facets = 0.0;
    for (int a = 0; a < 3; a++) {
        const double cell = st[(a + 1) % 3] * st[(a + 2) % 3];
        out[RM_SURF_FACET_POS_X + 2 * a] = cell * (double)from[a];
        out[RM_SURF_FACET_NEG_X + 2 * a] = cell * (double)back[a];
        facets += out[RM_SURF_FACET_POS_X + 2 * a] + out[RM_SURF_FACET_NEG_X + 2 * a];
    }
    out[RM_SURF_FACET_AREA] = facets;
    if (step[0] != step[1] || step[1] != step[2]) {
        out[RM_SURF_AREA] = std::nan("");
        return RM_OK;
    }
    const double dV = st[0] * st[1] * st[2];
    double sum = 0.0;
    for (uint32_t d = 0; d < (uint32_t)RM_SURF_DIRS; d++) {
        const rmk::SurfDir nu = rmk::surf_dir(d);
        const double vx = nu.x * st[0], vy = nu.y * st[1], vz = nu.z * st[2];
        const int kind = nu.x * nu.x + nu.y * nu.y + nu.z * nu.z;  // 1, 2, 3
        sum += kSurfWeight[kind - 1] * (double)(from[d] + back[d]) / std::sqrt(vx * vx + vy * vy + vz * vz);
    }
    out[RM_SURF_AREA] = 2.0 * dV * sum;
    return RM_OK;
}

// ---- mesh voxelisation (rm_voxel.h) ----
namespace {

static_assert(rmk::kVoxTriWords == rml::kVoxTriWords && (uint32_t)rmk::VOX_N_COUNTERS == rml::kVoxCounters, "VoxScratch holds the kernels' records");
static_assert(RM_VOX_STAT_BRICKS == kStatBricks && RM_VOX_STAT_BRICKS_KEPT == kStatBricksKept && RM_VOX_STAT_BRICKS_INSIDE == kStatBricksInside &&
                  RM_VOX_STAT_EVALUATIONS == kStatEvaluations && RM_VOX_STAT_SCRATCH_BYTES == RM_VOX_STATS - 1,
              "the brick statistics first (zeros, as for a caller's occupancy) and the scratch size last");
constexpr uint64_t kMaxVoxItems = 1ull << 31;

// The launches of a voxelisation: how many blocks of triangles, words of the bit volume, fill workgroups and folded rows.
struct VoxPlan {
    uint32_t n, n_blocks, row_words, n_words, n_groups, n_fblocks;
    VoxPlan(uint32_t n_triangles, uint32_t nx, uint32_t ny, uint32_t nz)
        : n(nx * ny * nz), n_blocks((uint32_t)(((uint64_t)n_triangles + rmk::kVoxBlock - 1u) / rmk::kVoxBlock)), row_words(rml::vox_row_words(nx)),
          n_words(ny * nz * row_words), n_groups((n + rml::kVoxFillCells - 1u) / rml::kVoxFillCells),
          n_fblocks(rmk::rows_folded(n_groups)) {}  // (rows <= 2^20, 33 words each at most)
};

}  // namespace

RM_EXPORT int rm_voxelize_mesh(rm_ctx* c, uint32_t n_vertices, const float* xyz, uint32_t n_triangles, const uint32_t* indices, int is_device,
                               void* stream, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, uint64_t* out_counts,
                               uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    const char* fn = "rm_voxelize_mesh";
    if (!c) return RM_ERR_NULL;
    if (!xyz || !out_counts || !out_stats) return fail(c, RM_ERR_NULL, "%s: xyz, out_counts or out_stats is NULL", fn);
    if (n_counts < (uint32_t)RM_VOX_COUNTS) return fail(c, RM_ERR_ARG, "%s: n_counts %u < RM_VOX_COUNTS", fn, n_counts);
    if (n_stats < (uint32_t)RM_VOX_STATS) return fail(c, RM_ERR_ARG, "%s: n_stats %u < RM_VOX_STATS", fn, n_stats);
    if (int rc = check_lattice(c, fn, origin, step)) return rc;
    if (int rc = check_topo_lattice(c, fn, nx, ny, nz)) return rc;
    if (n_triangles == 0u || n_vertices == 0u) return fail(c, RM_ERR_ARG, "%s: %u vertices, %u triangles: at least one of each", fn, n_vertices, n_triangles);
    if (!indices && (uint64_t)n_vertices != 3ull * n_triangles)
        return fail(c, RM_ERR_ARG, "%s: a soup (indices NULL) of %u triangles has %llu vertices, not %u", fn, n_triangles, 3ull * n_triangles, n_vertices);
    if (is_device && (misaligned(xyz, 4) || misaligned(indices, 4))) return fail(c, RM_ERR_ARG, "%s: device xyz and indices need 4-byte alignment", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a device read of the last occupancy, too
    const VoxPlan P(n_triangles, nx, ny, nz);
    const rml::VoxScratch S(n_triangles, P.n_blocks, P.n_words, P.n_groups, P.n_fblocks, is_device ? 0u : n_vertices,
                            is_device || !indices ? 0u : n_triangles);
    int rc = c->d_mscratch.reserve(c, S.bytes);
    if (rc != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    const float* d_xyz = xyz;
    const uint32_t* d_idx = indices;
    if (is_device) {
        // the caller's arrays are ready when the work queued on its stream is done; the call is synchronous anyway
        const hipStream_t su = user_stream(c, stream);
        if (su != s) HIP_TRY(c, hipStreamSynchronize(su));
    } else {
        HIP_TRY(c, hipMemcpyAsync(S.xyz.at(sc), xyz, S.xyz.bytes, hipMemcpyHostToDevice, s));
        d_xyz = S.xyz.at(sc);
        if (indices) {
            HIP_TRY(c, hipMemcpyAsync(S.idx.at(sc), indices, S.idx.bytes, hipMemcpyHostToDevice, s));
            d_idx = S.idx.at(sc);
        }
    }
    const rmk::VoxLattice g{origin[0], origin[1], origin[2], step[0], step[1], step[2], nx, ny, nz, P.row_words};
    uint32_t* bits = S.bits.at(sc);
    unsigned long long* counters = S.counters.at(sc);
    HIP_TRY(c, hipMemsetAsync(sc + S.clear_offset(), 0, S.clear_bytes(), s));
    hipLaunchKernelGGL(rmk::rm_vox_setup_kernel, dim3(P.n_blocks), dim3(256), 0, s, g, n_vertices, d_xyz, n_triangles, d_idx, S.tris.at(sc),
                       S.starts.at(sc), S.bsums.at(sc), bits, counters);
    uint64_t tot[2];
    if ((rc = scan_totals(c, s, S.bsums.at(sc), P.n_blocks, S.btot.at(sc), tot)) != RM_OK) return rc;
    if (tot[0] >= kMaxVoxItems)
        return fail(c, RM_ERR_TOO_LARGE, "%s: %llu work items of 64 rows: fewer than 2^31", fn, (unsigned long long)tot[0]);
    // the last check that can refuse is past: the previous occupancy goes
    c->vox.drop();
    if ((rc = c->vox.buf.reserve(c, P.n, "occupancy")) != RM_OK) return rc;
    const uint32_t n_items = (uint32_t)tot[0];
    if (n_items)
        hipLaunchKernelGGL(rmk::rm_vox_raster_kernel, dim3((n_items + 3u) / 4u), dim3(256), 0, s, g, n_triangles, n_items, S.tris.at(sc),
                           S.starts.at(sc), S.bsums.at(sc), bits, counters);
    constexpr rml::VoxFillLds L;
    static_assert(L.bytes + 1024u <= rml::kLdsLaunchLimit, "the staged words fit a workgroup's LDS");
    hipLaunchKernelGGL(rmk::rm_vox_fill_kernel, dim3(P.n_groups), dim3(256), L.bytes, s, nx, P.n, bits, c->vox.buf.as<uint8_t>(), S.rows.at(sc));
    unsigned long long row[RM_MOMENTS], cnt[rmk::VOX_N_COUNTERS];
    if ((rc = reduce_rows(c, s, S.rows.at(sc), P.n_groups, S.folded.at(sc), S.result.at(sc), row, {cnt, counters, sizeof cnt})) != RM_OK) return rc;
    out_counts[RM_VOX_TRIANGLES] = cnt[rmk::VOX_N_TRIANGLES];
    out_counts[RM_VOX_REJECTED] = cnt[rmk::VOX_N_REJECTED];
    out_counts[RM_VOX_EDGE_ON] = cnt[rmk::VOX_N_EDGE_ON];
    out_counts[RM_VOX_CROSSINGS] = cnt[rmk::VOX_N_CROSSINGS];
    out_counts[RM_VOX_INSIDE] = row[0];
    out_counts[RM_VOX_OPEN_ROWS] = row[1];
    for (uint32_t k = 0; k < (uint32_t)RM_VOX_STATS; k++) out_stats[k] = 0u;
    out_stats[RM_VOX_STAT_ITEMS] = n_items;
    out_stats[RM_VOX_STAT_SCRATCH_BYTES] = S.bytes;
    c->vox.commit(nx, ny, nz);
    return RM_OK;
}

RM_EXPORT int rm_read_voxels(rm_ctx* c, void* out_occupancy, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Voxels& r = c->vox;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_voxels: no mesh has been voxelised");
    return read_back(c, is_device, stream, "rm_read_voxels: out_occupancy needs no alignment", {{out_occupancy, r.buf.p, r.points(), 1}});
}

// ---- lattice meshing (rm_class_mesh.h) ----
namespace {

static_assert(rmk::kCmeshGroupWords == rml::kCmeshGroupWords && rmk::kCmeshNoId == RM_NO_ID, "ClassMeshScratch sizes the mark kernel's arrays");
static_assert(RM_CMESH_STAT_BRICKS == kStatBricks && RM_CMESH_STAT_BRICKS_KEPT == kStatBricksKept && RM_CMESH_STAT_BRICKS_INSIDE == kStatBricksInside &&
                  RM_CMESH_STAT_EVALUATIONS == kStatEvaluations && RM_CMESH_STAT_SCRATCH_BYTES == RM_CMESH_STATS - 1,
              "the brick statistics first (zeros, as for a caller's occupancy) and the scratch size last");
static_assert(RM_CMESH_FACES_POS_X == 3 && RM_CMESH_BRANCH_EDGES == RM_CMESH_FACES_POS_X + 8 && RM_CMESH_COUNTS == 12,
              "the mark kernel's rows hold VERTICES in entry 0 and FACES_POS_X .. BRANCH_EDGES in the entries 1 .. 9");

}  // namespace

RM_EXPORT int rm_mesh_classes(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                              const float* origin, const float* step, uint32_t mask_a, uint32_t mask_b, uint64_t* out_counts,
                              uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    const char* fn = "rm_mesh_classes";
    if (!c) return RM_ERR_NULL;
    if (!classes || !out_counts || !out_stats) return fail(c, RM_ERR_NULL, "%s: classes, out_counts or out_stats is NULL", fn);
    if (n_counts < (uint32_t)RM_CMESH_COUNTS) return fail(c, RM_ERR_ARG, "%s: n_counts %u < RM_CMESH_COUNTS", fn, n_counts);
    if (n_stats < (uint32_t)RM_CMESH_STATS) return fail(c, RM_ERR_ARG, "%s: n_stats %u < RM_CMESH_STATS", fn, n_stats);
    if (int rc = check_lattice(c, fn, origin, step)) return rc;
    if (int rc = check_topo_lattice(c, fn, nx, ny, nz)) return rc;
    const uint32_t all = (1u << RM_SURF_CLASSES) - 1u;
    if (mask_a == 0u || mask_b == 0u || (mask_a & mask_b) != 0u || ((mask_a | mask_b) & ~all) != 0u)
        return fail(c, RM_ERR_ARG, "%s: masks 0x%x, 0x%x: non-empty, disjoint, no bit above 7", fn, mask_a, mask_b);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a device read of the last class mesh, too
    const rml::ClassMeshScratch S(nx, ny, nz);
    int rc = c->d_mscratch.reserve(c, S.bytes);
    if (rc != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    if (is_device) {
        // the caller's array is ready when the work queued on its stream is done; the call is synchronous anyway
        const hipStream_t su = user_stream(c, stream);
        if (su != s) HIP_TRY(c, hipStreamSynchronize(su));
    }
    HIP_TRY(c, hipMemcpyAsync(S.cls.at(sc), classes, S.cls.bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    const rmk::CmeshGrid G{nx, ny, nz, nx + 1u, ny + 1u, rml::cmesh_row_words(nx), S.n_words, origin[0], origin[1], origin[2],
                           step[0], step[1], step[2], mask_a, mask_b};
    hipLaunchKernelGGL(rmk::rm_cmesh_mark_kernel, dim3(S.n_groups), dim3(256), 0, s, G, S.cls.at(sc), S.bits.at(sc), S.before.at(sc), S.bsums.at(sc),
                       S.rows.at(sc));
    if ((rc = scan_launch(c, s, S.bsums.at(sc), S.n_groups, S.btot.at(sc))) != RM_OK) return rc;
    unsigned long long row[RM_MOMENTS];
    uint64_t tot[2];
    if ((rc = reduce_rows(c, s, S.rows.at(sc), 2u * S.n_groups, S.folded.at(sc), S.result.at(sc), row, {tot, S.btot.at(sc), sizeof tot})) != RM_OK)
        return rc;
    // V < 2^32 and T < 2^32: a lattice of n <= 2^28 points with at least 2 along every axis has 3 n + ny nz + nx nz + nx ny <= 4.5 n
    // pairs with a point inside it, and four corners to a face
    const uint64_t V = tot[0], F = tot[1], T = 2u * F;
    const rml::ClassMeshSlot M(V, T);
    // the last check that can refuse is past: the previous mesh goes
    c->cmesh.drop();
    if ((rc = c->cmesh.buf.reserve(c, M.bytes, "class mesh")) != RM_OK) return rc;
    if (F) {
        char* base = c->cmesh.buf.p;
        hipLaunchKernelGGL(rmk::rm_cmesh_emit_kernel, dim3((S.n_words + 3u) / 4u), dim3(256), 0, s, G, S.cls.at(sc), S.bits.at(sc), S.before.at(sc),
                           S.bsums.at(sc), M.vertices.at(base), M.triangles.at(base), M.ids.at(base));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    out_counts[RM_CMESH_VERTICES] = V;
    out_counts[RM_CMESH_TRIANGLES] = T;
    out_counts[RM_CMESH_FACES] = F;
    for (uint32_t k = 0; k < 9u; k++) out_counts[RM_CMESH_FACES_POS_X + k] = row[1u + k];
    for (uint32_t k = 0; k < (uint32_t)RM_CMESH_STATS; k++) out_stats[k] = 0u;
    out_stats[RM_CMESH_STAT_RETAINED_BYTES] = M.bytes;
    out_stats[RM_CMESH_STAT_SCRATCH_BYTES] = S.bytes;
    c->cmesh.commit(V, T);
    return RM_OK;
}

RM_EXPORT int rm_read_class_mesh(rm_ctx* c, float* out_vertices, uint32_t* out_triangles, uint32_t* out_ids, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::ClassMesh& r = c->cmesh;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_class_mesh: no lattice has been meshed");
    const rml::ClassMeshSlot M(r.v, r.t);
    const char* base = r.buf.p;
    return read_back(c, is_device, stream, "rm_read_class_mesh: device arrays need 4-byte alignment",
                     {{out_vertices, M.vertices, base, 4}, {out_triangles, M.triangles, base, 4}, {out_ids, M.ids, base, 4}});
}

// ---- lattice draw (rm_lattice.h) ----
namespace {

static_assert((uint32_t)rmk::LAT_N_COUNTERS == 2u && RM_LAT_FACE_NONE == rmk::kLatFaceNone, "LatticeSlot holds the kernel's two counters");
static_assert(RM_LAT_STAT_BRICKS == kStatBricks && RM_LAT_STAT_BRICKS_KEPT == kStatBricksKept && RM_LAT_STAT_BRICKS_INSIDE == kStatBricksInside &&
                  RM_LAT_STAT_EVALUATIONS == kStatEvaluations && RM_LAT_STAT_SCRATCH_BYTES == RM_LAT_STATS - 1,
              "the brick statistics first (zeros, as for a caller's occupancy) and the scratch size last");

// The retained lattice and a call's window (six u32 in host memory, or NULL: the whole lattice) as the kernels take them, with
// the material table uploaded on stream s.  RM_ERR_ARG before any rm_set_lattice and for a bad window.
int lattice_grid(rm_ctx* c, const char* fn, const uint32_t* window, hipStream_t s, rmk::LatGrid* G) {
    const rm_ctx::Lattice& r = c->lat;
    if (!r.valid) return fail(c, RM_ERR_ARG, "%s: no lattice has been set (rm_set_lattice)", fn);
    const uint32_t n[3] = {r.nx, r.ny, r.nz};
    uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {r.nx, r.ny, r.nz};
    for (int a = 0; window && a < 3; a++) {
        lo[a] = window[a], hi[a] = window[3 + a];
        if (!(lo[a] < hi[a] && hi[a] <= n[a]))
            return fail(c, RM_ERR_ARG, "%s: window [%u, %u) on axis %d of %u points: lo < hi <= n", fn, lo[a], hi[a], a, n[a]);
    }
    if (int rc = upload_materials(c, s)) return rc;
    const rml::LatticeSlot S(r.nx, r.ny, r.nz);
    const char* base = r.buf.p;
    *G = rmk::LatGrid{r.origin[0], r.origin[1], r.origin[2], r.step[0], r.step[1], r.step[2], r.nx, r.ny, r.nz, rml::lat_row_words(r.nx),
                      rml::lat_bricks(r.nx), rml::lat_bricks(r.ny), lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], S.classes.at(base), S.bits.at(base),
                      S.bricks.at(base), reinterpret_cast<const float*>(c->d_materials.p), (uint32_t)c->materials.size()};
    return RM_OK;
}

}  // namespace

RM_EXPORT int rm_set_lattice(rm_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                             const float* origin, const float* step, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                             uint32_t n_stats) {
    const char* fn = "rm_set_lattice";
    if (!c) return RM_ERR_NULL;
    if (!classes || !out_counts || !out_stats) return fail(c, RM_ERR_NULL, "%s: classes, out_counts or out_stats is NULL", fn);
    if (n_counts < (uint32_t)RM_LAT_COUNTS) return fail(c, RM_ERR_ARG, "%s: n_counts %u < RM_LAT_COUNTS", fn, n_counts);
    if (n_stats < (uint32_t)RM_LAT_STATS) return fail(c, RM_ERR_ARG, "%s: n_stats %u < RM_LAT_STATS", fn, n_stats);
    if (int rc = check_lattice(c, fn, origin, step)) return rc;
    if (int rc = check_topo_lattice(c, fn, nx, ny, nz)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a draw or a cast of the last lattice on another stream, too
    const rml::LatticeSlot S(nx, ny, nz);
    // the last check that can refuse is past: the previous lattice goes
    c->lat.drop();
    if (int rc = c->lat.buf.reserve(c, S.bytes, "lattice")) return rc;
    char* base = c->lat.buf.p;
    if (is_device) {
        // the caller's array is ready when the work queued on its stream is done; the call is synchronous anyway
        const hipStream_t su = user_stream(c, stream);
        if (su != s) HIP_TRY(c, hipStreamSynchronize(su));
    }
    HIP_TRY(c, hipMemcpyAsync(S.classes.at(base), classes, S.classes.bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(base + S.clear_offset(), 0, S.clear_bytes(), s));
    const uint32_t row_words = rml::lat_row_words(nx), n_words = ny * nz * row_words;  // (<= 2^27: rows of two points)
    hipLaunchKernelGGL(rmk::rm_lat_pack_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, s, nx, ny, row_words, n_words, rml::lat_bricks(nx),
                       rml::lat_bricks(ny), S.classes.at(base), S.bits.at(base), S.bricks.at(base), S.counters.at(base));
#if !RM_LAT_SKIP
    HIP_TRY(c, hipMemsetAsync(S.bricks.at(base), 0xFF, S.bricks.bytes, s));  // the probe's A/B library: no brick is ever jumped
#endif
    HIP_TRY(c, hipGetLastError());
    unsigned long long cnt[rmk::LAT_N_COUNTERS];
    HIP_TRY(c, hipMemcpyAsync(cnt, S.counters.at(base), sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    out_counts[RM_LAT_POINTS] = cnt[rmk::LAT_N_POINTS];
    out_counts[RM_LAT_BRICKS] = cnt[rmk::LAT_N_BRICKS];
    for (uint32_t k = 0; k < (uint32_t)RM_LAT_STATS; k++) out_stats[k] = 0u;
    out_stats[RM_LAT_STAT_RETAINED_BYTES] = S.bytes;
    c->lat.commit(nx, ny, nz, origin, step);
    return RM_OK;
}

RM_EXPORT int rm_draw_lattice(rm_ctx* c, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* window, void* out_rgba,
                              int out_is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_rgba) return fail(c, RM_ERR_NULL, "rm_draw_lattice: out_rgba is NULL");
    int rc = check_dims(c, W, H, row0, rows);
    if (rc != RM_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, out_is_device, stream);
    rmk::LatGrid G;
    if (!c->lat.valid) return lattice_grid(c, "rm_draw_lattice", window, s, &G);  // (refused before the stream is touched)
    order_with_previous(c, s);
    if ((rc = lattice_grid(c, "rm_draw_lattice", window, s, &G)) != RM_OK) return rc;
    // host memory: staged through the context's query buffer (never the draws' scratch), synchronously on its own stream
    Outputs o(c, out_is_device, c->d_qout);
    o.add(out_rgba, (size_t)rows * W * pixel_bytes(c));
    if ((rc = o.reserve()) != RM_OK) return rc;
    rmk::LatFrame F;
    F.u = c->uniforms;
    F.W = W; F.H = H; F.row0 = row0; F.rows = rows;
    F.format = c->out_format;
    F.out = o.dev<char>(0);
    // one wave per 2 x 2 block of pixels
    const size_t lanes = (size_t)((W + 1u) / 2u) * ((rows + 1u) / 2u) * 64u;
    hipLaunchKernelGGL(rmk::rm_draw_lattice_kernel, dim3(query_blocks(lanes)), dim3(256), 0, s, G, F);
    HIP_TRY(c, hipGetLastError());
    return o.finish(s);
}

RM_EXPORT int rm_cast_lattice(rm_ctx* c, uint32_t n, const float* rays, const uint32_t* window, float* out_hit, uint32_t* out_ids,
                              float* out_rgb, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    if (!out_hit && !out_ids && !out_rgb) return fail(c, RM_ERR_NULL, "rm_cast_lattice: every output is NULL");
    if (n == 0u) return RM_OK;
    if (!rays) return fail(c, RM_ERR_NULL, "rm_cast_lattice: rays is NULL");
    if (is_device && (misaligned(rays, 4) || misaligned(out_hit, 16) || misaligned(out_ids, 16) || misaligned(out_rgb, 4)))
        return fail(c, RM_ERR_ARG, "rm_cast_lattice: device arrays need 4-byte alignment (out_hit, out_ids: 16-byte)");
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = dest_stream(c, is_device, stream);
    rmk::LatGrid G;
    if (!c->lat.valid) return lattice_grid(c, "rm_cast_lattice", window, s, &G);
    order_with_previous(c, s);
    int rc = lattice_grid(c, "rm_cast_lattice", window, s, &G);
    if (rc != RM_OK) return rc;
    Outputs o(c, is_device, c->d_qout);
    o.add(out_hit, (size_t)n * 32u);
    o.add(out_ids, (size_t)n * 16u);
    o.add(out_rgb, (size_t)n * 12u);
    const float* d_rays = nullptr;
    if ((rc = query_input(c, o, rays, (size_t)n * 24u, s, &d_rays)) != RM_OK) return rc;
    hipLaunchKernelGGL(rmk::rm_cast_lattice_kernel, dim3(query_blocks(n)), dim3(256), 0, s, G, n, d_rays, o.dev<float>(0), o.dev<uint32_t>(1),
                       o.dev<float>(2));
    HIP_TRY(c, hipGetLastError());
    return o.finish(s);
}

RM_EXPORT int rm_read_mesh(rm_ctx* c, float* out_vertices, uint32_t* out_triangles, float* out_normals, uint32_t* out_ids,
                           int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Mesh& r = c->mesh;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_mesh: no mesh has been extracted");
    if (out_normals && !(r.flags & RM_MESH_NORMALS)) return fail(c, RM_ERR_ARG, "rm_read_mesh: the mesh was extracted without RM_MESH_NORMALS");
    if (out_ids && !(r.flags & RM_MESH_IDS)) return fail(c, RM_ERR_ARG, "rm_read_mesh: the mesh was extracted without RM_MESH_IDS");
    const rml::MeshLayout L = mesh_layout(r.v, r.t, r.flags);
    const char* m = r.buf.p;
    return read_back(c, is_device, stream, "rm_read_mesh: device arrays need 4-byte alignment (out_ids: 8-byte)",
                     {{out_vertices, L.vertices, m, 4}, {out_triangles, L.triangles, m, 4}, {out_normals, L.normals, m, 4}, {out_ids, L.ids, m, 8}});
}

RM_EXPORT int rm_mesh_case_table(uint32_t* out, uint32_t n_out) {
    if (!out) return RM_ERR_NULL;
    if (n_out < 256u * rmk::kMeshCaseWords) return RM_ERR_ARG;
    std::memcpy(out, rmk::kMeshCaseTable.w, sizeof rmk::kMeshCaseTable.w);
    return RM_OK;
}

// ---- slicing (rm_slice.h) ------------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t kMaxSlicePoints = 1ull << 26;  // lattice points of one layer

uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1u) / per); }

}  // namespace

RM_EXPORT int rm_slice_contours(rm_ctx* c, uint32_t axis, const float* origin_uv, const float* step_uv, uint32_t nu, uint32_t nv,
                                const float* heights, uint32_t n_layers, float level, uint32_t flags, uint64_t* out_counts,
                                uint32_t n_counts) {
    if (!c) return RM_ERR_NULL;
    if (!out_counts) return fail(c, RM_ERR_NULL, "rm_slice_contours: out_counts is NULL");
    if (!origin_uv || !step_uv || !heights) return fail(c, RM_ERR_NULL, "rm_slice_contours: origin_uv, step_uv or heights is NULL");
    if (n_counts < (uint32_t)RM_SLICE_COUNTS) return fail(c, RM_ERR_ARG, "rm_slice_contours: n_counts %u < RM_SLICE_COUNTS", n_counts);
    if (axis > 2u) return fail(c, RM_ERR_ARG, "rm_slice_contours: axis %u is not 0, 1 or 2", axis);
    for (int a = 0; a < 2; a++) {
        if (!std::isfinite(origin_uv[a])) return fail(c, RM_ERR_ARG, "rm_slice_contours: origin_uv[%d] = %g is not finite", a, (double)origin_uv[a]);
        if (!std::isfinite(step_uv[a]) || !(step_uv[a] > 0.0f))
            return fail(c, RM_ERR_ARG, "rm_slice_contours: step_uv[%d] = %g: a step must be finite and > 0", a, (double)step_uv[a]);
    }
    if (int rc = check_iso(c, "rm_slice_contours", level, flags)) return rc;
    const uint64_t n2_64 = (uint64_t)nu * nv;
    if (nu < 2 || nv < 2 || nu > kMaxDim || nv > kMaxDim || n2_64 > kMaxSlicePoints || n_layers < 1 || n_layers > kMaxDim)
        return fail(c, RM_ERR_RANGE, "rm_slice_contours: lattice %ux%u, %u layers: 2..65536 points per axis, at most 2^26 per layer, 1..65536 layers",
                    nu, nv, n_layers);
    for (uint32_t k = 0; k < n_layers; k++)
        if (!std::isfinite(heights[k])) return fail(c, RM_ERR_ARG, "rm_slice_contours: heights[%u] = %g is not finite", k, (double)heights[k]);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    QueryCall q;
    int rc = q.begin(c, s, (flags & RM_MESH_IDS) != 0, false);  // after a device read of the previous slices, too
    if (rc != RM_OK) return rc;
    c->drop_slices();
    const uint32_t n2 = (uint32_t)n2_64, per = std::min(n_layers, std::max(1u, rmk::kSliceBatchPoints / n2));
    const uint32_t n_max = per * n2, nb_max = blocks_of(n_max, rmk::kSliceBlock);
    const rml::SliceLayerTables T(n_layers, per);
    if ((rc = c->slices.layers.reserve(c, T.bytes)) != RM_OK) return rc;
    char* lt = c->slices.layers.p;
    float* d_heights = T.heights.at(lt);
    uint32_t* d_lf = T.layer_first.at(lt);
    uint32_t* d_base = T.base.at(lt);
    uint32_t* d_totals = T.totals.at(lt);
    HIP_TRY(c, hipMemcpyAsync(d_heights, heights, (size_t)n_layers * 4u, hipMemcpyHostToDevice, s));
    const rml::SlicePointScratch S(n_max, nb_max);
    if ((rc = c->d_mscratch.reserve(c, S.bytes)) != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    float* dist = S.dist.at(sc);
    uint32_t* packed = S.packed.at(sc);
    uint32_t* sums = S.sums.at(sc);
    std::vector<uint32_t> base(per + 1u);
    uint64_t P = 0, Cn = 0;
    for (uint32_t k0 = 0; k0 < n_layers; k0 += per) {
        const uint32_t nl = std::min(per, n_layers - k0), n = nl * n2, nb = blocks_of(n, rmk::kSliceBlock), pb = blocks_of(n, 256u);
        const rmk::SliceGrid g{origin_uv[0], origin_uv[1], step_uv[0], step_uv[1], nu, nv, n2, axis, k0, n};
        if ((rc = q.launch(RM_BY_LOOP(rm_slice_dist_kernel), query_blocks(n), 0u, g, d_heights, dist)) != RM_OK) return rc;
        hipLaunchKernelGGL(rmk::rm_slice_count_kernel, dim3(nb), dim3(256), 0, s, g, level, dist, sums);
        hipLaunchKernelGGL(rmk::rm_slice_scan_kernel, dim3(1), dim3(1024), 0, s, sums, nb, d_totals);
        hipLaunchKernelGGL(rmk::rm_slice_pack_kernel, dim3(nb), dim3(256), 0, s, g, level, dist, sums, packed);
        hipLaunchKernelGGL(rmk::rm_slice_layer_base_kernel, dim3(blocks_of(nl + 1u, 256u)), dim3(256), 0, s, packed, n2, nl, d_totals, d_base);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(base.data(), d_base, ((size_t)nl + 1u) * 4u, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const uint32_t V = base[nl];
        if (P + V > 0xFFFFFFFFull) return fail(c, RM_ERR_RANGE, "rm_slice_contours: more than 2^32 - 1 points");
        if (V == 0u) {
            hipLaunchKernelGGL(rmk::rm_slice_layer_first_kernel, dim3(blocks_of(nl + 1u, 256u)), dim3(256), 0, s, d_base, nl, 0u, nullptr, 0u,
                               (uint32_t)Cn, d_lf + k0);
            HIP_TRY(c, hipGetLastError());
            continue;
        }
        // ranking rounds: 2^rounds >= the vertices of the fullest layer >= the longest chain
        uint32_t v_layer = 0, rounds = 0;
        for (uint32_t l = 0; l < nl; l++) v_layer = std::max(v_layer, base[l + 1u] - base[l]);
        while ((1ull << rounds) < v_layer) rounds++;
        // per contour: at most V / 2 (a chain has two vertices or more)
        const uint32_t vb = blocks_of(V, 256u), vsb = blocks_of(V, rmk::kSliceBlock), c_max = V / 2u + 1u;
        const rml::SliceVertexScratch<uint2> Wk(V, vsb, c_max);
        if ((rc = c->d_swork.reserve(c, Wk.bytes)) != RM_OK) return rc;
        char* wk = c->d_swork.p;
        uint32_t* next = Wk.next.at(wk);
        uint32_t* prev = Wk.prev.at(wk);
        uint2* st_a = Wk.state0.at(wk);
        uint2* st_b = Wk.state1.at(wk);
        uint32_t* start = Wk.start.at(wk);
        uint32_t* vsums = Wk.vsums.at(wk);
        uint32_t* length = Wk.length.at(wk);
        uint32_t* first_point = Wk.first_point.at(wk);
        if ((rc = c->slices.points.grow_keep(c, (size_t)(P + V) * 12u, (size_t)P * 12u, s)) != RM_OK) return rc;
        HIP_TRY(c, hipMemsetAsync(wk, 0xFF, Wk.state0.offset, s));  // next and prev: kSliceNil
        hipLaunchKernelGGL(rmk::rm_slice_link_kernel, dim3(pb), dim3(256), 0, s, g, packed, next, prev);
        hipLaunchKernelGGL(rmk::rm_slice_low_init_kernel, dim3(vb), dim3(256), 0, s, next, V, st_a);
        for (uint32_t r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(rmk::rm_slice_low_round_kernel, dim3(vb), dim3(256), 0, s, st_a, V, st_b);
            std::swap(st_a, st_b);
        }
        hipLaunchKernelGGL(rmk::rm_slice_cut_kernel, dim3(vb), dim3(256), 0, s, st_a, prev, V, start, st_b);
        std::swap(st_a, st_b);
        for (uint32_t r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(rmk::rm_slice_rank_round_kernel, dim3(vb), dim3(256), 0, s, st_a, V, st_b);
            std::swap(st_a, st_b);
        }
        hipLaunchKernelGGL(rmk::rm_slice_start_count_kernel, dim3(vsb), dim3(256), 0, s, start, V, vsums);
        hipLaunchKernelGGL(rmk::rm_slice_scan_kernel, dim3(1), dim3(1024), 0, s, vsums, vsb, d_totals + 1);
        hipLaunchKernelGGL(rmk::rm_slice_start_scan_kernel, dim3(vsb), dim3(256), 0, s, start, V, vsums);
        HIP_TRY(c, hipGetLastError());
        uint32_t Cb = 0;
        HIP_TRY(c, hipMemcpyAsync(&Cb, d_totals + 1, 4u, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (Cb > c_max) return fail(c, RM_ERR_DEVICE, "rm_slice_contours: %u contours from %u vertices", Cb, V);
        if (Cn + Cb > 0xFFFFFFFFull) return fail(c, RM_ERR_RANGE, "rm_slice_contours: more than 2^32 - 1 contours");
        if ((rc = c->slices.contours.grow_keep(c, (size_t)(Cn + Cb) * 16u, (size_t)Cn * 16u, s)) != RM_OK) return rc;
        const uint32_t cb = blocks_of(Cb, rmk::kSliceBlock);
        hipLaunchKernelGGL(rmk::rm_slice_length_kernel, dim3(vb), dim3(256), 0, s, st_a, next, start, V, length);
        hipLaunchKernelGGL(rmk::rm_slice_length_count_kernel, dim3(cb), dim3(256), 0, s, length, Cb, vsums);
        hipLaunchKernelGGL(rmk::rm_slice_scan_kernel, dim3(1), dim3(1024), 0, s, vsums, cb, d_totals + 2);
        hipLaunchKernelGGL(rmk::rm_slice_length_scan_kernel, dim3(cb), dim3(256), 0, s, length, Cb, vsums, first_point);
        hipLaunchKernelGGL(rmk::rm_slice_layer_first_kernel, dim3(blocks_of(nl + 1u, 256u)), dim3(256), 0, s, d_base, nl, V, start, Cb, (uint32_t)Cn,
                           d_lf + k0);
        hipLaunchKernelGGL(rmk::rm_slice_emit_kernel, dim3(pb), dim3(256), 0, s, g, level, dist, d_heights, packed, st_a, start, length, first_point,
                           (uint32_t)P, (uint32_t)Cn, c->slices.points.as<float>(), c->slices.contours.as<uint4>());
        HIP_TRY(c, hipGetLastError());
        P += V;
        Cn += Cb;
    }
    // the attributes of the points: rm_query_points at their positions, device to device
    const rml::SliceAttributes A(P, (flags & RM_MESH_NORMALS) != 0, (flags & RM_MESH_IDS) != 0);
    if (P > 0u) {
        if ((rc = c->slices.attr.reserve(c, A.bytes)) != RM_OK) return rc;
        if ((rc = point_attributes(q, flags, P, c->slices.points.as<const float>(), c->slices.attr.p, A.normals, A.ids)) != RM_OK) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    out_counts[RM_SLICE_POINTS] = P;
    out_counts[RM_SLICE_CONTOURS] = Cn;
    c->slices.commit(P, Cn, n_layers, flags, axis);
    return RM_OK;
}

RM_EXPORT int rm_read_slices(rm_ctx* c, float* out_points, uint32_t* out_contours, uint32_t* out_layer_first, float* out_normals,
                             uint32_t* out_ids, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Slices& r = c->slices;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_slices: nothing has been sliced");
    if (out_normals && !(r.flags & RM_MESH_NORMALS)) return fail(c, RM_ERR_ARG, "rm_read_slices: the slices were computed without RM_MESH_NORMALS");
    if (out_ids && !(r.flags & RM_MESH_IDS)) return fail(c, RM_ERR_ARG, "rm_read_slices: the slices were computed without RM_MESH_IDS");
    const rml::SliceLayerTables T(r.n_layers);
    const rml::SliceAttributes A(r.p, (r.flags & RM_MESH_NORMALS) != 0, (r.flags & RM_MESH_IDS) != 0);
    return read_back(c, is_device, stream, "rm_read_slices: device arrays need 4-byte alignment (out_contours: 16-byte, out_ids: 8-byte)",
                     {{out_points, r.points.p, (size_t)r.p * 12u, 4}, {out_contours, r.contours.p, (size_t)r.c * 16u, 16},
                      {out_layer_first, T.layer_first, r.layers.p, 4}, {out_normals, A.normals, r.attr.p, 4}, {out_ids, A.ids, r.attr.p, 8}});
}

RM_EXPORT int rm_slice_case_table(uint32_t* out, uint32_t n_out) {
    if (!out) return RM_ERR_NULL;
    if (n_out < 16u * rmk::kSliceCaseWords) return RM_ERR_ARG;
    std::memcpy(out, rmk::kSliceCaseTable.w, sizeof rmk::kSliceCaseTable.w);
    return RM_OK;
}

// ---- mesh slicing (rm_mesh_slice.h) ----
namespace {

static_assert(RM_MSLICE_STAT_SCRATCH_BYTES == RM_MSLICE_STATS - 1, "the scratch size last");
constexpr double kMsliceMaxR = 262144.0;  // |r_k| <= 2^18

// Room for `need` bytes of a retained result WITHOUT touching the buffer that holds the previous one: nothing when it is large
// enough, else a fresh allocation for the caller to move in once the previous result is dropped.
int reserve_beside(rm_ctx* c, const DevBuf<char>& current, size_t need, DevBuf<char>& fresh) {
    return need <= current.cap ? RM_OK : fresh.reserve(c, need, "slices");
}
void move_in(DevBuf<char>& current, DevBuf<char>& fresh) {
    if (fresh.p) current = std::move(fresh);  // (the old buffer goes with `fresh`)
}

}  // namespace

RM_EXPORT int rm_slice_mesh(rm_ctx* c, const float* xyz, uint32_t n_vertices, const uint32_t* triangles, uint32_t n_triangles, int is_device,
                            void* stream, const float* origin, const float* step, uint32_t axis, const float* heights, uint32_t n_layers,
                            uint32_t flags, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    const char* fn = "rm_slice_mesh";
    if (!c) return RM_ERR_NULL;
    if (!xyz || !triangles || !heights || !out_counts || !out_stats || !origin || !step)
        return fail(c, RM_ERR_NULL, "%s: xyz, triangles, origin, step, heights, out_counts or out_stats is NULL", fn);
    if (n_counts < (uint32_t)RM_MSLICE_COUNTS) return fail(c, RM_ERR_ARG, "%s: n_counts %u < RM_MSLICE_COUNTS", fn, n_counts);
    if (n_stats < (uint32_t)RM_MSLICE_STATS) return fail(c, RM_ERR_ARG, "%s: n_stats %u < RM_MSLICE_STATS", fn, n_stats);
    if (flags != 0u) return fail(c, RM_ERR_ARG, "%s: flags 0x%x: must be 0", fn, flags);
    if (axis > 2u) return fail(c, RM_ERR_ARG, "%s: axis %u is not 0, 1 or 2", fn, axis);
    if (int rc = check_lattice(c, fn, origin, step)) return rc;
    if (n_vertices == 0u) return fail(c, RM_ERR_ARG, "%s: no vertices", fn);
    if (n_layers < 1u || n_layers > kMaxDim || n_triangles < 1u || n_triangles > (1u << 28))
        return fail(c, RM_ERR_RANGE, "%s: %u layers, %u triangles: 1..65536 layers, 1..2^28 triangles", fn, n_layers, n_triangles);
    // the planes, before the first launch
    std::vector<int32_t> p2(n_layers);
    for (uint32_t k = 0; k < n_layers; k++) {
        if (!std::isfinite(heights[k])) return fail(c, RM_ERR_ARG, "%s: heights[%u] = %g is not finite", fn, k, (double)heights[k]);
        const double r = ((double)heights[k] - (double)origin[axis]) / (double)step[axis] * 64.0;
        if (!(std::fabs(r) <= kMsliceMaxR)) return fail(c, RM_ERR_RANGE, "%s: heights[%u] = %g lies more than 4096 steps from the origin", fn, k, (double)heights[k]);
        p2[k] = 2 * (int32_t)std::floor(r) + 1;
    }
    for (uint32_t k = 1; k < n_layers; k++)
        if (!(p2[k] > p2[k - 1u]))
            return fail(c, RM_ERR_ARG, "%s: heights[%u] = %g does not lie in a plane above heights[%u] = %g: planes must be strictly increasing", fn, k,
                        (double)heights[k], k - 1u, (double)heights[k - 1u]);
    if (is_device && (misaligned(xyz, 4) || misaligned(triangles, 4))) return fail(c, RM_ERR_ARG, "%s: device xyz and triangles need 4-byte alignment", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a device read of the previous slices, too
    const uint32_t H = 3u * n_triangles;
    const rml::MeshSliceScratch S(n_vertices, n_triangles, n_layers, is_device ? 0u : n_vertices, is_device ? 0u : n_triangles);
    int rc = c->d_mscratch.reserve(c, S.bytes);
    if (rc != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    const float* d_xyz = xyz;
    const uint32_t* d_tri = triangles;
    if (is_device) {
        // the caller's arrays are ready when the work queued on its stream is done; the call is synchronous anyway
        const hipStream_t su = user_stream(c, stream);
        if (su != s) HIP_TRY(c, hipStreamSynchronize(su));
    } else {
        HIP_TRY(c, hipMemcpyAsync(S.xyz.at(sc), xyz, S.xyz.bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(S.idx.at(sc), triangles, S.idx.bytes, hipMemcpyHostToDevice, s));
        d_xyz = S.xyz.at(sc);
        d_tri = S.idx.at(sc);
    }
    HIP_TRY(c, hipMemcpyAsync(S.p2.at(sc), p2.data(), (size_t)n_layers * 4u, hipMemcpyHostToDevice, s));
    rmk::MsliceFrame f{};
    for (int a = 0; a < 3; a++) f.o[a] = (double)origin[a], f.s[a] = (double)step[a];
    f.axis = axis, f.n_layers = n_layers;
    int32_t* vq = S.vq.at(sc);
    const int32_t* d_p2 = S.p2.at(sc);
    uint32_t* mate = S.mate.at(sc);
    uint32_t* estart = S.estart.at(sc);
    uint32_t* k0 = S.k0.at(sc);
    // edges: b = the bit length of n_vertices - 1, keys of 2 b bits
    uint32_t b = 0;
    while (b < 32u && ((uint64_t)(n_vertices - 1u) >> b) != 0u) b++;
    const uint32_t edge_bits = std::max(1u, 2u * b), hb = blocks_of(H, 256u), hsb = blocks_of(H, rmk::kSliceBlock);
    hipLaunchKernelGGL(rmk::rm_mslice_snap_kernel, dim3(blocks_of(n_vertices, 256u)), dim3(256), 0, s, f, n_vertices, d_xyz, vq);
    hipLaunchKernelGGL(rmk::rm_mslice_keys_kernel, dim3(hb), dim3(256), 0, s, n_vertices, H, b, d_tri, vq, S.hkeys.at(sc), S.hvals.at(sc));
    const rml::SortedPairs E = rml::sort_pairs(s, S.hkeys.at(sc), S.hvals.at(sc), H, edge_bits, sc + S.sort);
    hipLaunchKernelGGL(rmk::rm_mslice_groups_kernel, dim3(hb), dim3(256), 0, s, H, d_tri, E.keys, E.values, mate, S.rows.at(sc));
    hipLaunchKernelGGL(rmk::rm_mslice_count_kernel, dim3(hsb), dim3(256), 0, s, f, n_vertices, H, d_tri, vq, d_p2, mate, estart, k0, S.bsums.at(sc));
    HIP_TRY(c, hipGetLastError());
    if ((rc = scan_launch(c, s, S.bsums.at(sc), hsb, S.btot.at(sc))) != RM_OK) return rc;
    unsigned long long erow[RM_MOMENTS];
    uint64_t tot[2];
    if ((rc = reduce_rows(c, s, S.rows.at(sc), hb, S.folded.at(sc), S.result.at(sc), erow, {tot, S.btot.at(sc), sizeof tot})) != RM_OK) return rc;
    if (tot[0] > 0xFFFFFFFFull) return fail(c, RM_ERR_RANGE, "%s: %llu points: more than 2^32 - 1", fn, (unsigned long long)tot[0]);
    const uint32_t N = (uint32_t)tot[0];
    const rml::SliceLayerTables T(n_layers);
    uint32_t Cb = 0, rounds = 0, item_passes = 0;
    uint64_t open = 0;
    size_t scratch_bytes = S.bytes;
    DevBuf<char> f_points, f_contours, f_layers;
    if (N == 0u) {
        if ((rc = reserve_beside(c, c->slices.layers, T.bytes, f_layers)) != RM_OK) return rc;
        // the last check that can refuse is past: the previous slices go
        c->drop_slices();
        move_in(c->slices.layers, f_layers);
        HIP_TRY(c, hipMemsetAsync(T.layer_first.at(c->slices.layers.p), 0, T.layer_first.bytes, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    } else {
        const rml::MeshSliceItems I(N, n_layers);
        if ((rc = c->d_mbricks.reserve(c, I.bytes)) != RM_OK) return rc;
        char* ic = c->d_mbricks.p;
        uint32_t layer_bits = 1;
        while (layer_bits < 32u && ((n_layers - 1u) >> layer_bits) != 0u) layer_bits++;
        const uint32_t vb = blocks_of(N, 256u), vsb = blocks_of(N, rmk::kSliceBlock), c_max = N / 2u + 1u;
        hipLaunchKernelGGL(rmk::rm_mslice_scan_kernel, dim3(hsb), dim3(256), 0, s, H, S.bsums.at(sc), estart);
        hipLaunchKernelGGL(rmk::rm_mslice_items_kernel, dim3(vb), dim3(256), 0, s, N, H, estart, k0, I.ikeys.at(ic), I.ivals.at(ic));
        const rml::SortedPairs V = rml::sort_pairs(s, I.ikeys.at(ic), I.ivals.at(ic), N, layer_bits, ic + I.sort);
        item_passes = V.passes;
        uint32_t* inv = I.inv.at(ic);
        uint32_t* vh = I.vh.at(ic);
        uint32_t* d_base = I.layer_base.at(ic);
        uint32_t* d_totals = I.totals.at(ic);
        hipLaunchKernelGGL(rmk::rm_mslice_ids_kernel, dim3(vb), dim3(256), 0, s, N, H, n_layers, estart, V.keys, V.values, inv, vh, d_base);
        HIP_TRY(c, hipGetLastError());
        std::vector<uint32_t> base((size_t)n_layers + 1u);
        HIP_TRY(c, hipMemcpyAsync(base.data(), d_base, base.size() * 4u, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        // ranking rounds: 2^rounds >= the vertices of the fullest layer >= the longest chain
        uint32_t v_layer = 0;
        for (uint32_t l = 0; l < n_layers; l++) v_layer = std::max(v_layer, base[l + 1u] - base[l]);
        while ((1ull << rounds) < v_layer) rounds++;
        const rml::SliceVertexScratch<uint2> Wk(N, vsb, c_max);
        if ((rc = c->d_swork.reserve(c, Wk.bytes)) != RM_OK) return rc;
        scratch_bytes += I.bytes + Wk.bytes;
        char* wk = c->d_swork.p;
        uint32_t* next = Wk.next.at(wk);
        uint32_t* prev = Wk.prev.at(wk);
        uint2* st_a = Wk.state0.at(wk);
        uint2* st_b = Wk.state1.at(wk);
        uint32_t* start = Wk.start.at(wk);
        uint32_t* vsums = Wk.vsums.at(wk);
        uint32_t* length = Wk.length.at(wk);
        uint32_t* first_point = Wk.first_point.at(wk);
        HIP_TRY(c, hipMemsetAsync(wk, 0xFF, Wk.state0.offset, s));  // next and prev: kSliceNil
        hipLaunchKernelGGL(rmk::rm_mslice_link_kernel, dim3(vb), dim3(256), 0, s, f, N, d_tri, vq, d_p2, mate, estart, k0, V.keys, vh, inv, next, prev);
        hipLaunchKernelGGL(rmk::rm_slice_low_init_kernel, dim3(vb), dim3(256), 0, s, next, N, st_a);
        for (uint32_t r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(rmk::rm_slice_low_round_kernel, dim3(vb), dim3(256), 0, s, st_a, N, st_b);
            std::swap(st_a, st_b);
        }
        hipLaunchKernelGGL(rmk::rm_slice_cut_kernel, dim3(vb), dim3(256), 0, s, st_a, prev, N, start, st_b);
        std::swap(st_a, st_b);
        for (uint32_t r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(rmk::rm_slice_rank_round_kernel, dim3(vb), dim3(256), 0, s, st_a, N, st_b);
            std::swap(st_a, st_b);
        }
        hipLaunchKernelGGL(rmk::rm_slice_start_count_kernel, dim3(vsb), dim3(256), 0, s, start, N, vsums);
        hipLaunchKernelGGL(rmk::rm_slice_scan_kernel, dim3(1), dim3(1024), 0, s, vsums, vsb, d_totals + 1);
        hipLaunchKernelGGL(rmk::rm_slice_start_scan_kernel, dim3(vsb), dim3(256), 0, s, start, N, vsums);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&Cb, d_totals + 1, 4u, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (Cb > c_max) return fail(c, RM_ERR_DEVICE, "%s: %u contours from %u vertices", fn, Cb, N);
        // every size is known: room for the result beside the previous one, which goes only when nothing can refuse any more
        if ((rc = reserve_beside(c, c->slices.points, (size_t)N * 12u, f_points)) != RM_OK) return rc;
        if ((rc = reserve_beside(c, c->slices.contours, (size_t)Cb * 16u, f_contours)) != RM_OK) return rc;
        if ((rc = reserve_beside(c, c->slices.layers, T.bytes, f_layers)) != RM_OK) return rc;
        c->drop_slices();
        move_in(c->slices.points, f_points);
        move_in(c->slices.contours, f_contours);
        move_in(c->slices.layers, f_layers);
        const uint32_t cb = blocks_of(Cb, rmk::kSliceBlock);
        hipLaunchKernelGGL(rmk::rm_slice_length_kernel, dim3(vb), dim3(256), 0, s, st_a, next, start, N, length);
        hipLaunchKernelGGL(rmk::rm_slice_length_count_kernel, dim3(cb), dim3(256), 0, s, length, Cb, vsums);
        hipLaunchKernelGGL(rmk::rm_slice_scan_kernel, dim3(1), dim3(1024), 0, s, vsums, cb, d_totals + 2);
        hipLaunchKernelGGL(rmk::rm_slice_length_scan_kernel, dim3(cb), dim3(256), 0, s, length, Cb, vsums, first_point);
        hipLaunchKernelGGL(rmk::rm_slice_layer_first_kernel, dim3(blocks_of(n_layers + 1u, 256u)), dim3(256), 0, s, d_base, n_layers, N, start, Cb, 0u,
                           T.layer_first.at(c->slices.layers.p));
        hipLaunchKernelGGL(rmk::rm_mslice_emit_kernel, dim3(vb), dim3(256), 0, s, f, N, d_tri, vq, d_p2, V.keys, vh, prev, st_a, start, length, first_point,
                           c->slices.points.as<float>(), c->slices.contours.as<uint4>(), I.rows.at(ic));
        HIP_TRY(c, hipGetLastError());
        unsigned long long vrow[RM_MOMENTS];
        if ((rc = reduce_rows(c, s, I.rows.at(ic), vb, I.folded.at(ic), I.result.at(ic), vrow)) != RM_OK) return rc;
        open = vrow[0];
    }
    out_counts[RM_MSLICE_TRIANGLES] = n_triangles;
    out_counts[RM_MSLICE_REJECTED] = erow[3];
    out_counts[RM_MSLICE_PAIRED_EDGES] = erow[0];
    out_counts[RM_MSLICE_BORDER_EDGES] = erow[1];
    out_counts[RM_MSLICE_BRANCH_EDGES] = erow[2];
    out_counts[RM_MSLICE_SEGMENTS] = (uint64_t)N - open;  // a closed contour has a segment per point, an open one one fewer
    out_counts[RM_MSLICE_POINTS] = N;
    out_counts[RM_MSLICE_CONTOURS] = Cb;
    out_counts[RM_MSLICE_OPEN_CONTOURS] = open;
    out_stats[RM_MSLICE_STAT_SORT_PASSES] = E.passes + item_passes;
    out_stats[RM_MSLICE_STAT_RANK_ROUNDS] = rounds;
    out_stats[RM_MSLICE_STAT_SCRATCH_BYTES] = scratch_bytes;
    c->slices.commit(N, Cb, n_layers, 0u, axis);
    return RM_OK;
}

// ---- hatching (rm_hatch.h) ----
static_assert(RM_HATCH_STAT_SCRATCH_BYTES == RM_HATCH_STATS - 1, "the scratch size last");

RM_EXPORT int rm_hatch_slices(rm_ctx* c, const float* lines, uint32_t n_layers, uint32_t n_lines, uint32_t flags, uint64_t* out_counts,
                              uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats) {
    const char* fn = "rm_hatch_slices";
    if (!c) return RM_ERR_NULL;
    if (!lines || !out_counts || !out_stats) return fail(c, RM_ERR_NULL, "%s: lines, out_counts or out_stats is NULL", fn);
    if (n_counts < (uint32_t)RM_HATCH_COUNTS) return fail(c, RM_ERR_ARG, "%s: n_counts %u < RM_HATCH_COUNTS", fn, n_counts);
    if (n_stats < (uint32_t)RM_HATCH_STATS) return fail(c, RM_ERR_ARG, "%s: n_stats %u < RM_HATCH_STATS", fn, n_stats);
    if ((flags & ~(uint32_t)RM_HATCH_ZIGZAG) != 0u) return fail(c, RM_ERR_ARG, "%s: flags 0x%x: RM_HATCH_ZIGZAG or 0", fn, flags);
    const rm_ctx::Slices& sl = c->slices;
    if (!sl.valid) return fail(c, RM_ERR_ARG, "%s: nothing has been sliced", fn);
    if (n_layers != sl.n_layers) return fail(c, RM_ERR_ARG, "%s: %u line sets for slices of %u layers", fn, n_layers, sl.n_layers);
    for (uint32_t k = 0; k < n_layers; k++) {
        const float* l = lines + (size_t)k * 4u;
        if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !std::isfinite(l[3]))
            return fail(c, RM_ERR_ARG, "%s: lines[%u] = (%g, %g, %g, %g) is not finite", fn, k, (double)l[0], (double)l[1], (double)l[2], (double)l[3]);
        if (!(l[3] > 0.0f)) return fail(c, RM_ERR_ARG, "%s: lines[%u]: spacing %g must be > 0", fn, k, (double)l[3]);
        if (l[0] == 0.0f && l[1] == 0.0f) return fail(c, RM_ERR_ARG, "%s: lines[%u]: the direction is (0, 0)", fn, k);
    }
    if (n_lines < 1u || n_lines > rml::kHatchMaxLines) return fail(c, RM_ERR_RANGE, "%s: %u lines per layer: 1..2^24", fn, n_lines);
    const uint64_t all_lines = (uint64_t)n_layers * n_lines;
    if (all_lines > (1ull << 32)) return fail(c, RM_ERR_RANGE, "%s: %u layers of %u lines: more than 2^32 lines", fn, n_layers, n_lines);
    HIP_TRY(c, hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    order_with_previous(c, s);  // after a device read of the slices or of the previous hatch, too
    const uint32_t P = (uint32_t)sl.p, pb = blocks_of(P, rmk::kSliceBlock);
    const rml::HatchScratch S(P, n_layers);
    int rc = c->d_mscratch.reserve(c, S.bytes);
    if (rc != RM_OK) return rc;
    char* sc = c->d_mscratch.p;
    size_t scratch_bytes = S.bytes;
    uint32_t N = 0, passes = 0;
    uint64_t H = 0;
    unsigned long long crow[RM_MOMENTS] = {}, prow[RM_MOMENTS] = {};
    rmk::HatchFrame f{};
    f.u = sl.axis == 2u ? 0u : sl.axis + 1u, f.v = f.u == 2u ? 0u : f.u + 1u;
    f.n_points = P, f.n_contours = (uint32_t)sl.c, f.n_lines = n_lines;
    const float* points = sl.points.as<const float>();
    const uint4* contours = sl.contours.as<const uint4>();
    const float4* d_lines = reinterpret_cast<const float4*>(S.lines.at(sc));
    uint32_t* cstart = S.cstart.at(sc);
    uint32_t* j0 = S.j0.at(sc);
    if (P > 0u) {
        HIP_TRY(c, hipMemcpyAsync(S.lines.at(sc), lines, (size_t)n_layers * 16u, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(rmk::rm_hatch_count_kernel, dim3(pb), dim3(256), 0, s, f, points, contours, d_lines, cstart, j0, S.bsums.at(sc), S.rows.at(sc));
        HIP_TRY(c, hipGetLastError());
        if ((rc = scan_launch(c, s, S.bsums.at(sc), pb, S.btot.at(sc))) != RM_OK) return rc;
        uint64_t tot[2];
        if ((rc = reduce_rows(c, s, S.rows.at(sc), pb, S.folded.at(sc), S.result.at(sc), crow, {tot, S.btot.at(sc), sizeof tot})) != RM_OK) return rc;
        if (!rml::hatch_crossings_fit(tot[0], tot[1])) return fail(c, RM_ERR_RANGE, "%s: 2^32 crossings or more", fn);
        N = (uint32_t)tot[0];
    }
    DevBuf<char> fresh;
    if (N == 0u) {
        const rml::HatchSlot T(0u, n_layers);
        if ((rc = reserve_beside(c, c->hatch.buf, T.bytes, fresh)) != RM_OK) return rc;
        // the last check that can refuse is past: the previous hatch goes
        c->hatch.drop();
        move_in(c->hatch.buf, fresh);
        HIP_TRY(c, hipMemsetAsync(T.layer_first.at(c->hatch.buf.p), 0, T.layer_first.bytes, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    } else {
        const rml::HatchItems I(N);
        if ((rc = c->d_mbricks.reserve(c, I.bytes)) != RM_OK) return rc;
        scratch_bytes += I.bytes;
        char* ic = c->d_mbricks.p;
        const uint32_t nb = blocks_of(N, rmk::kSliceBlock);
        float2* xs = reinterpret_cast<float2*>(I.xs.at(ic));
        uint32_t* hstart = I.hstart.at(ic);
        hipLaunchKernelGGL(rmk::rm_mslice_scan_kernel, dim3(pb), dim3(256), 0, s, P, S.bsums.at(sc), cstart);
        hipLaunchKernelGGL(rmk::rm_hatch_items_kernel, dim3(blocks_of(N, 256u)), dim3(256), 0, s, f, N, points, contours, d_lines, cstart, j0,
                           I.ikeys.at(ic), I.ivals.at(ic), xs);
        const rml::SortedPairs V = rml::sort_pairs(s, I.ikeys.at(ic), I.ivals.at(ic), N, rml::hatch_key_bits(all_lines), ic + I.sort);
        passes = V.passes;
        hipLaunchKernelGGL(rmk::rm_hatch_pair_kernel, dim3(nb), dim3(256), 0, s, N, V.keys, hstart, I.bsums.at(ic), I.rows.at(ic));
        HIP_TRY(c, hipGetLastError());
        if ((rc = scan_launch(c, s, I.bsums.at(ic), nb, I.btot.at(ic))) != RM_OK) return rc;
        uint64_t htot[2];
        if ((rc = reduce_rows(c, s, I.rows.at(ic), nb, I.folded.at(ic), I.result.at(ic), prow, {htot, I.btot.at(ic), sizeof htot})) != RM_OK) return rc;
        H = htot[0];  // (at most N / 2)
        // every size is known: room for the result beside the previous one, which goes only when nothing can refuse any more
        const rml::HatchSlot T(H, n_layers);
        if ((rc = reserve_beside(c, c->hatch.buf, T.bytes, fresh)) != RM_OK) return rc;
        c->hatch.drop();
        move_in(c->hatch.buf, fresh);
        char* hb = c->hatch.buf.p;
        hipLaunchKernelGGL(rmk::rm_mslice_scan_kernel, dim3(nb), dim3(256), 0, s, N, I.bsums.at(ic), hstart);
        hipLaunchKernelGGL(rmk::rm_hatch_emit_kernel, dim3(blocks_of(std::max(N, n_layers + 1u), 256u)), dim3(256), 0, s, N, n_layers, n_lines,
                           flags & (uint32_t)RM_HATCH_ZIGZAG, V.keys, V.values, xs, hstart, reinterpret_cast<float4*>(T.segments.at(hb)),
                           T.line.at(hb), T.layer_first.at(hb));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    out_counts[RM_HATCH_SEGMENTS_IN] = crow[0];
    out_counts[RM_HATCH_CROSSINGS] = N;
    out_counts[RM_HATCH_SEGMENTS] = H;
    out_counts[RM_HATCH_LINES_HIT] = prow[0];
    out_counts[RM_HATCH_ODD_LINES] = prow[1];
    out_stats[RM_HATCH_STAT_SORT_PASSES] = passes;
    out_stats[RM_HATCH_STAT_SCRATCH_BYTES] = scratch_bytes;
    c->hatch.commit(H, n_layers);
    return RM_OK;
}

RM_EXPORT int rm_read_hatch(rm_ctx* c, float* out_segments, uint32_t* out_line, uint32_t* out_layer_first, int is_device, void* stream) {
    if (!c) return RM_ERR_NULL;
    const rm_ctx::Hatch& r = c->hatch;
    if (!r.valid) return fail(c, RM_ERR_ARG, "rm_read_hatch: no hatch of the current slices");
    const rml::HatchSlot T(r.h, r.n_layers);
    return read_back(c, is_device, stream, "rm_read_hatch: device arrays need 4-byte alignment (out_segments: 16-byte)",
                     {{out_segments, T.segments, r.buf.p, 16}, {out_line, T.line, r.buf.p, 4}, {out_layer_first, T.layer_first, r.buf.p, 4}});
}

RM_EXPORT int rm_sync_context(rm_ctx* c) {
    if (!c) return RM_ERR_NULL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RM_OK;
}

RM_EXPORT int rm_sync(rm_ctx* c) {
    if (!c) return RM_ERR_NULL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    return RM_OK;
}

RM_EXPORT int rm_set_option(rm_ctx* c, int key, int64_t value) {
    if (!c) return RM_ERR_NULL;
    switch (key) {
    case RM_OPT_KERNEL:
        if (value != RM_KERNEL_DEFAULT && value != RM_KERNEL_PIXEL && value != RM_KERNEL_V5 && value != RM_KERNEL_V5_LDS)
            return fail(c, RM_ERR_ARG, "unknown kernel %lld (the v2-v4 variants 2..11 of ABI version 1 are retired)", (long long)value);
        c->kernel = (int)value;
        return RM_OK;
    case RM_OPT_TIMING: c->timing = value != 0; c->tev_used = 0; return RM_OK;
    case RM_OPT_STRICT_CAP: return RM_OK;
    case RM_OPT_CULL: c->cull = value != 0; return RM_OK;
    case RM_OPT_BALANCE: c->balance = value < 0 ? 0 : value > 3 ? 3 : (int)value; c->measured_shape = 0; return RM_OK;
    case RM_OPT_WAVE_STATS: c->wave_stats = value != 0; return RM_OK;
    case RM_OPT_PRUNE:
        if (value < 0 || value > 2) return fail(c, RM_ERR_ARG, "RM_OPT_PRUNE: %lld is not 0, 1 or 2", (long long)value);
        c->prune = (int)value;
        c->spec_gen = ~0ull;
        return RM_OK;
    case RM_OPT_OUTPUT_FORMAT:
        if (value < RM_FORMAT_RGBA32F || value > RM_FORMAT_BGRA8_UNORM) return fail(c, RM_ERR_ARG, "unknown output format %lld", (long long)value);
        c->out_format = (int)value;
        return RM_OK;
    case RM_OPT_SPECIALIZE:
        if (value < 0 || value > 2) return fail(c, RM_ERR_ARG, "RM_OPT_SPECIALIZE: %lld is not 0, 1 or 2", (long long)value);
        c->specialize = (int)value;
        return RM_OK;
    case RM_OPT_WAVES_PER_TILE:
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return fail(c, RM_ERR_ARG, "waves_per_tile must be 0 (automatic), 1, 2, 4 or 8");
        c->waves_per_tile = (int)value;
        return RM_OK;
    case RM_OPT_REFILL_MIN:
        if (value < 0 || value > 64) return fail(c, RM_ERR_ARG, "refill_min %lld not in [0,64]", (long long)value);
        c->refill_min_v5 = (uint32_t)value;
        return RM_OK;
    default: return fail(c, RM_ERR_ARG, "unknown option %d", key);
    }
}

RM_EXPORT int rm_get_info(rm_ctx* c, int key, double* out) {
    if (!c) return RM_ERR_NULL;
    if (!out) return fail(c, RM_ERR_NULL, "rm_get_info: out is NULL");
    switch (key) {
    case RM_INFO_KERNEL_MS: {  // mean duration of the dominant kernel over the launches timed since the last query
        double sum = 0.0;
        for (size_t i = 0; i < c->tev_used; i++) {
            HIP_TRY(c, hipEventSynchronize(c->tev[i].second));
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->tev[i].first, c->tev[i].second));
            sum += ms;
        }
        if (c->tev_used) c->last_kernel_ms = sum / (double)c->tev_used;
        c->tev_used = 0;
        *out = c->last_kernel_ms;
        return RM_OK;
    }
    case RM_INFO_DEVICE: *out = c->device; return RM_OK;
    case RM_INFO_CU_COUNT: *out = c->cu_count; return RM_OK;
    case RM_INFO_SPECIALIZED: *out = c->last_specialized ? 1.0 : 0.0; return RM_OK;
    case RM_INFO_RANGE_PROOF: *out = c->last_range_proof ? 1.0 : 0.0; return RM_OK;
    case RM_INFO_INTERPRETER_LOOP: *out = c->last_specialized ? 0.0 : (double)c->last_loop; return RM_OK;
    case RM_INFO_PRUNED: *out = c->spec && c->spec_gen == c->prog_gen && !c->cmd_dirty ? (double)c->spec_pruned : 0.0; return RM_OK;
    case RM_INFO_JIT_STATE:
    case RM_INFO_JIT_FROM_CACHE:
    case RM_INFO_JIT_COMPILE_MS: {
        *out = 0.0;
        if (c->spec && c->spec_gen == c->prog_gen && !c->cmd_dirty) {
            std::lock_guard<std::mutex> lk(c->spec->m);
            if (key == RM_INFO_JIT_STATE) *out = 1.0 + (double)c->spec->state;
            else if (key == RM_INFO_JIT_FROM_CACHE) *out = c->spec->from_cache ? 1.0 : 0.0;
            else *out = c->spec->compile_ms;
        }
        return RM_OK;
    }
    case RM_INFO_PROGRAM_COMMANDS:
    case RM_INFO_PROGRAM_WORDS:
    case RM_INFO_PROGRAM_DEPTH: {
        RmDecoded d;
        int rc = rm_decode_program(c->cmd[0], c->cmd.data() + 1, (uint32_t)c->cmd.size() - 1u, &d);
        if (rc != RM_OK) return fail(c, rc, "invalid CSG program in command buffer: %s", rm_status_string(rc));
        *out = key == RM_INFO_PROGRAM_COMMANDS ? c->cmd[0] : key == RM_INFO_PROGRAM_WORDS ? d.n_words : d.max_depth;
        return RM_OK;
    }
    default: return fail(c, RM_ERR_ARG, "unknown info key %d", key);
    }
}

RM_EXPORT int rm_read_wave_stats(rm_ctx* c, void* dst, uint64_t cap_bytes, uint64_t* out_bytes) {
    if (!c) return RM_ERR_NULL;
    if (!dst || !out_bytes) return fail(c, RM_ERR_NULL, "rm_read_wave_stats: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    const uint64_t n = c->stats_valid_bytes < cap_bytes ? c->stats_valid_bytes : cap_bytes;
    if (n) HIP_TRY(c, hipMemcpy(dst, c->d_stats.p, n, hipMemcpyDeviceToHost));
    *out_bytes = n;
    return RM_OK;
}

RM_EXPORT int rm_selftest_sqrt(rm_ctx* c, uint64_t* out_mismatches, uint32_t* out_first_bad_bits) {
    if (!c) return RM_ERR_NULL;
    if (!out_mismatches || !out_first_bad_bits) return fail(c, RM_ERR_NULL, "rm_selftest_sqrt: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d_bad;
    DevBuf<uint32_t> d_first;
    if (int rc = d_bad.reserve(c, 1)) return rc;
    if (int rc = d_first.reserve(c, 1)) return rc;
    HIP_TRY(c, hipMemset(d_bad.p, 0, 8));
    HIP_TRY(c, hipMemset(d_first.p, 0xFF, 4));
    hipLaunchKernelGGL(rmk::rm_selftest_sqrt_kernel, dim3(std::max(1, c->cu_count) * 16), dim3(256), 0, c->stream, 0u,
                       (uint64_t)1 << 32, d_bad.p, d_first.p);
    hipError_t e = hipStreamSynchronize(c->stream);
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad.p, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_first_bad_bits, d_first.p, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_sqrt: %s", hipGetErrorString(e));
    *out_mismatches = bad;
    return RM_OK;
}

RM_EXPORT int rm_selftest_div(rm_ctx* c, const float* a, const float* b, uint32_t n, uint32_t seed, uint32_t n_seeded, uint64_t* out) {
    if (!c) return RM_ERR_NULL;
    if (!out || (n != 0u && (!a || !b))) return fail(c, RM_ERR_NULL, "rm_selftest_div: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> da, db;
    DevBuf<unsigned long long> d_out;
    if (int rc = da.reserve(c, n ? n : 1u)) return rc;
    if (int rc = db.reserve(c, n ? n : 1u)) return rc;
    if (int rc = d_out.reserve(c, 8)) return rc;
    unsigned long long init[8] = {0, ~0ull, 0, 0, 0, ~0ull, 0, 0};
    hipError_t e = hipMemcpy(d_out.p, init, sizeof init, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(da.p, a, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(db.p, b, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rmk::rm_selftest_div_kernel, dim3(std::max(1, c->cu_count) * 16), dim3(256), 0, c->stream, da.p, db.p, n, seed,
                           n_seeded, d_out.p);
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out.p, 64, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_div: %s", hipGetErrorString(e));
    return RM_OK;
}

RM_EXPORT int rm_selftest_normalise(rm_ctx* c, const float* in, uint32_t n, int mode, uint32_t* out) {
    if (!c) return RM_ERR_NULL;
    if (!in || !out) return fail(c, RM_ERR_NULL, "rm_selftest_normalise: NULL argument");
    if (n == 0u || (n & 63u) != 0u || n > (1u << 24) || mode < 0 || mode > 2)
        return fail(c, RM_ERR_ARG, "rm_selftest_normalise: n must be a multiple of 64 in [64, 2^24] and mode 0, 1 or 2");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> din;
    DevBuf<uint32_t> dout;
    if (int rc = din.reserve(c, (size_t)n * 8)) return rc;
    if (int rc = dout.reserve(c, (size_t)n * 8)) return rc;
    hipError_t e = hipMemcpy(din.p, in, (size_t)n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rmk::rm_selftest_normalise_kernel, dim3(n / 256u + (n % 256u ? 1u : 0u)), dim3(256), 0, c->stream, din.p, n,
                           (uint32_t)mode, dout.p);
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_normalise: %s", hipGetErrorString(e));
    return RM_OK;
}

RM_EXPORT int rm_selftest_ops(rm_ctx* c, const float* a, const float* b, float* out, uint32_t n) {
    if (!c) return RM_ERR_NULL;
    if (!a || !b || !out || n == 0u) return fail(c, RM_ERR_NULL, "rm_selftest_ops: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> da, db, dout;
    if (int rc = da.reserve(c, n)) return rc;
    if (int rc = db.reserve(c, n)) return rc;
    if (int rc = dout.reserve(c, (size_t)n * 8)) return rc;
    hipError_t e = hipMemcpy(da.p, a, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db.p, b, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rmk::rm_selftest_ops_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, da.p, db.p, dout.p, n);
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)n * 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_ops: %s", hipGetErrorString(e));
    return RM_OK;
}

RM_EXPORT int rm_selftest_wave(rm_ctx* c, const float* in, uint32_t n_waves, float* out) {
    if (!c) return RM_ERR_NULL;
    if (!in || !out || n_waves == 0u || n_waves > 65535u) return fail(c, RM_ERR_NULL, "rm_selftest_wave: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_waves * 64u;
    DevBuf<float> din, dout;
    if (int rc = din.reserve(c, n)) return rc;
    if (int rc = dout.reserve(c, n * 2)) return rc;
    hipError_t e = hipMemcpy(din.p, in, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rmk::rm_selftest_wave_kernel, dim3(n_waves), dim3(64), 0, c->stream, din.p, dout.p, n_waves);
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_wave: %s", hipGetErrorString(e));
    return RM_OK;
}

RM_EXPORT int rm_selftest_sort(rm_ctx* c, const uint64_t* keys, const uint32_t* values, uint32_t n, uint32_t bits, uint64_t* out_keys,
                               uint32_t* out_values) {
    if (!c) return RM_ERR_NULL;
    if (!keys || !values || !out_keys || !out_values) return fail(c, RM_ERR_NULL, "rm_selftest_sort: NULL argument");
    if (n == 0u || bits < 1u || bits > 64u) return fail(c, RM_ERR_ARG, "rm_selftest_sort: n = %u, bits = %u: n >= 1, bits in 1..64", n, bits);
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> dk;
    DevBuf<uint32_t> dv;
    DevBuf<char> scratch;
    if (int rc = dk.reserve(c, n)) return rc;
    if (int rc = dv.reserve(c, n)) return rc;
    if (int rc = scratch.reserve(c, rml::SortScratch(n).bytes)) return rc;
    hipError_t e = hipMemcpy(dk.p, keys, (size_t)n * 8u, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dv.p, values, (size_t)n * 4u, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const rml::SortedPairs r = rml::sort_pairs(c->stream, dk.p, dv.p, n, bits, scratch.p);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(out_keys, r.keys, (size_t)n * 8u, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out_values, r.values, (size_t)n * 4u, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "rm_selftest_sort: %s", hipGetErrorString(e));
    return RM_OK;
}

// ---- self-tests of the culling decisions (rm_kernel_v5.h rm_selftest_cull_*_kernel) -----------------------------------------
namespace {
// What a draw does before it launches, and the launch it would fill for a W x H frame of the context's program with the default
// march kernel: rm_selftest_cull_* hand their kernels the same flags, table sizes, bounds, slack, scale and unit table.
int cull_probe_begin(rm_ctx* c, const char* fn, uint32_t W, uint32_t H, RmLaunch* L) {
    HIP_TRY(c, hipSetDevice(c->device));
    order_with_previous(c, c->stream);
    int rc = ensure_program(c, c->stream);
    if (rc == RM_OK) rc = check_limits(c);
    if (rc != RM_OK) return rc;
    if (W == 0u || H == 0u || W > kMaxDim || H > kMaxDim) return fail(c, RM_ERR_RANGE, "%s: image size %ux%u out of range", fn, W, H);
    *L = fill_launch(c, nullptr, W, H, 0u, H, nullptr, StripSpec());
    (void)plan_v5(c, *L, true);
    return RM_OK;
}
// host array -> a device buffer of this call
template <class T>
int probe_put(rm_ctx* c, DevBuf<T>& buf, const void* src, size_t n) {
    if (int rc = buf.reserve(c, n)) return rc;
    HIP_TRY(c, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return RM_OK;
}
int probe_finish(rm_ctx* c, const char* fn) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    return RM_OK;
}
}  // namespace

RM_EXPORT int rm_selftest_cull_rays(rm_ctx* c, const float* origin, const float* dirs, uint32_t n, uint32_t* out_flags, float* out_bound) {
    if (!c) return RM_ERR_NULL;
    if (!origin || !dirs || !out_flags || !out_bound) return fail(c, RM_ERR_NULL, "rm_selftest_cull_rays: NULL argument");
    if (n == 0u || n > (1u << 20)) return fail(c, RM_ERR_ARG, "rm_selftest_cull_rays: n = %u, must be 1 .. 2^20", n);
    RmLaunch L;
    if (int rc = cull_probe_begin(c, "rm_selftest_cull_rays", 8u, 8u, &L)) return rc;
    DevBuf<float> d_dirs, d_bound;
    DevBuf<uint32_t> d_flags;
    if (int rc = probe_put(c, d_dirs, dirs, (size_t)n * 3u)) return rc;
    if (int rc = d_flags.reserve(c, n)) return rc;
    if (int rc = d_bound.reserve(c, n)) return rc;
    const size_t shmem = rml::CullLds(L.n_cone, L.n_slab, false).bytes;
    const rmk::V4 ro{origin[0], origin[1], origin[2], 1.0f};
    hipLaunchKernelGGL(rmk::rm_selftest_cull_rays_kernel, dim3((n + 63u) / 64u), dim3(64), shmem, c->stream, L, ro, d_dirs.p, n, d_flags.p, d_bound.p);
    if (int rc = probe_finish(c, "rm_selftest_cull_rays")) return rc;
    HIP_TRY(c, hipMemcpy(out_flags, d_flags.p, (size_t)n * 4u, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_bound, d_bound.p, (size_t)n * 4u, hipMemcpyDeviceToHost));
    return RM_OK;
}

RM_EXPORT int rm_selftest_cull_pixels(rm_ctx* c, uint32_t W, uint32_t H, const uint32_t* xy, uint32_t n, float* out) {
    if (!c) return RM_ERR_NULL;
    if (!xy || !out) return fail(c, RM_ERR_NULL, "rm_selftest_cull_pixels: NULL argument");
    if (n == 0u || n > (1u << 20)) return fail(c, RM_ERR_ARG, "rm_selftest_cull_pixels: n = %u, must be 1 .. 2^20", n);
    RmLaunch L;
    if (int rc = cull_probe_begin(c, "rm_selftest_cull_pixels", W, H, &L)) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (xy[2u * i] >= W || xy[2u * i + 1u] >= H)
            return fail(c, RM_ERR_RANGE, "rm_selftest_cull_pixels: pixel %u = (%u, %u) outside the %ux%u image", i, xy[2u * i], xy[2u * i + 1u], W, H);
    DevBuf<uint32_t> d_xy;
    DevBuf<float> d_out;
    if (int rc = probe_put(c, d_xy, xy, (size_t)n * 2u)) return rc;
    if (int rc = d_out.reserve(c, (size_t)n * 8u)) return rc;
    const size_t shmem = rml::CullLds(L.n_cone, L.n_slab, true).bytes;
    hipLaunchKernelGGL(rmk::rm_selftest_cull_pixels_kernel, dim3((n + 63u) / 64u), dim3(64), shmem, c->stream, L, d_xy.p, n, d_out.p);
    if (int rc = probe_finish(c, "rm_selftest_cull_pixels")) return rc;
    HIP_TRY(c, hipMemcpy(out, d_out.p, (size_t)n * 32u, hipMemcpyDeviceToHost));
    return RM_OK;
}

RM_EXPORT int rm_selftest_cull_tiles(rm_ctx* c, uint32_t W, uint32_t H, const uint32_t* xy, uint32_t n, float* out) {
    if (!c) return RM_ERR_NULL;
    if (!xy || !out) return fail(c, RM_ERR_NULL, "rm_selftest_cull_tiles: NULL argument");
    if (n == 0u || n > (1u << 20)) return fail(c, RM_ERR_ARG, "rm_selftest_cull_tiles: n = %u, must be 1 .. 2^20", n);
    RmLaunch L;
    if (int rc = cull_probe_begin(c, "rm_selftest_cull_tiles", W, H, &L)) return rc;
    const uint32_t tiles_x = (W + 7u) / 8u, tiles_y = (H + 7u) / 8u;
    for (uint32_t i = 0; i < n; i++)
        if (xy[2u * i] >= tiles_x || xy[2u * i + 1u] >= tiles_y)
            return fail(c, RM_ERR_RANGE, "rm_selftest_cull_tiles: tile %u = (%u, %u) outside the %ux%u tiles of the image", i, xy[2u * i], xy[2u * i + 1u],
                        tiles_x, tiles_y);
    DevBuf<uint32_t> d_xy;
    DevBuf<float> d_out;
    if (int rc = probe_put(c, d_xy, xy, (size_t)n * 2u)) return rc;
    if (int rc = d_out.reserve(c, (size_t)n * 8u)) return rc;
    const size_t shmem = rml::CullLds(L.n_cone, L.n_slab, true).bytes;
    hipLaunchKernelGGL(rmk::rm_selftest_cull_tiles_kernel, dim3((n + 63u) / 64u), dim3(64), shmem, c->stream, L, d_xy.p, n, d_out.p);
    if (int rc = probe_finish(c, "rm_selftest_cull_tiles")) return rc;
    HIP_TRY(c, hipMemcpy(out, d_out.p, (size_t)n * 32u, hipMemcpyDeviceToHost));
    return RM_OK;
}

RM_EXPORT int rm_selftest_cull_waves(rm_ctx* c, const float* origin, const float* pos, const float* thr, const uint64_t* live, uint32_t n_waves,
                                     float extra_margin, uint64_t* out_masks) {
    if (!c) return RM_ERR_NULL;
    if (!origin || !pos || !thr || !live || !out_masks) return fail(c, RM_ERR_NULL, "rm_selftest_cull_waves: NULL argument");
    if (n_waves == 0u || n_waves > 65535u) return fail(c, RM_ERR_ARG, "rm_selftest_cull_waves: n_waves = %u, must be 1 .. 65535", n_waves);
    for (uint32_t w = 0; w < n_waves; w++)
        if (live[w] == 0u) return fail(c, RM_ERR_ARG, "rm_selftest_cull_waves: wave %u has no live lane", w);
    RmLaunch L;
    if (int rc = cull_probe_begin(c, "rm_selftest_cull_waves", 8u, 8u, &L)) return rc;
    if (L.unit_mode == RM_UNITS_NONE || L.n_grp == 0u || L.n_grp > 64u)
        return fail(c, RM_ERR_ARG, "rm_selftest_cull_waves: the program has no units of wave-level culling");
    DevBuf<float> d_pos, d_thr;
    DevBuf<unsigned long long> d_live, d_out;
    if (int rc = probe_put(c, d_pos, pos, (size_t)n_waves * 192u)) return rc;
    if (int rc = probe_put(c, d_thr, thr, (size_t)n_waves * 64u)) return rc;
    if (int rc = probe_put(c, d_live, live, (size_t)n_waves)) return rc;
    if (int rc = d_out.reserve(c, n_waves)) return rc;
    const rmk::V4 ro{origin[0], origin[1], origin[2], 1.0f};
    hipLaunchKernelGGL(rmk::rm_selftest_cull_waves_kernel, dim3(n_waves), dim3(64), (size_t)L.n_grp * 32u, c->stream, L, ro, d_pos.p, d_thr.p,
                       d_live.p, extra_margin, d_out.p);
    if (int rc = probe_finish(c, "rm_selftest_cull_waves")) return rc;
    HIP_TRY(c, hipMemcpy(out_masks, d_out.p, (size_t)n_waves * 8u, hipMemcpyDeviceToHost));
    return RM_OK;
}

RM_EXPORT int rm_selftest_anchor(rm_ctx* c, const float* origin, const float* pairs, uint32_t n, float* out) {
    if (!c) return RM_ERR_NULL;
    if (!origin || !pairs || !out) return fail(c, RM_ERR_NULL, "rm_selftest_anchor: NULL argument");
    if (n == 0u || n > (1u << 20)) return fail(c, RM_ERR_ARG, "rm_selftest_anchor: n = %u, must be 1 .. 2^20", n);
    RmLaunch L;
    if (int rc = cull_probe_begin(c, "rm_selftest_anchor", 8u, 8u, &L)) return rc;  // the march's scene_scale
    QueryCall q;
    if (int rc = q.begin(c, c->stream, false, false)) return rc;
    DevBuf<float> d_pairs, d_out;
    if (int rc = probe_put(c, d_pairs, pairs, (size_t)n * 6u)) return rc;
    if (int rc = d_out.reserve(c, (size_t)n * 4u)) return rc;
    const float prune_scale = L.scene_scale + ((std::fabs(origin[0]) + std::fabs(origin[1])) + std::fabs(origin[2]));  // prune_scale_v5
    if (int rc = q.launch(RM_BY_LOOP(rm_selftest_anchor_kernel), query_blocks(n), 0u, prune_scale, n, (const float*)d_pairs.p, d_out.p)) return rc;
    if (int rc = probe_finish(c, "rm_selftest_anchor")) return rc;
    HIP_TRY(c, hipMemcpy(out, d_out.p, (size_t)n * 16u, hipMemcpyDeviceToHost));
    return RM_OK;
}

RM_EXPORT int rm_measure_write_bandwidth(rm_ctx* c, uint64_t bytes, int iters, double* out_gbps) {
    if (!c) return RM_ERR_NULL;
    if (!out_gbps) return fail(c, RM_ERR_NULL, "rm_measure_write_bandwidth: out is NULL");
    if (bytes < 4096 || (bytes & 15u) || iters < 1 || iters > 1000) return fail(c, RM_ERR_ARG, "bad bytes/iters");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float4> buf;
    if (int rc = buf.reserve(c, bytes / 16u)) return rc;
    const size_t n_vec = bytes / 16u;
    const int grid = std::max(1, c->cu_count) * 8;
    hipLaunchKernelGGL(rmk::rm_fill, dim3(grid), dim3(256), 0, c->stream, buf.p, n_vec, 0.0f);  // warm-up
    hipError_t e = hipEventRecord(c->ev0, c->stream);
    for (int i = 0; i < iters && e == hipSuccess; i++)
        hipLaunchKernelGGL(rmk::rm_fill, dim3(grid), dim3(256), 0, c->stream, buf.p, n_vec, (float)i);
    if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
    if (e != hipSuccess) return fail(c, RM_ERR_DEVICE, "write-bandwidth calibration failed: %s", hipGetErrorString(e));
    *out_gbps = (double)bytes * iters / (ms * 1e-3) / 1e9;
    return RM_OK;
}

namespace {
int jit_decode(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, int waves_per_tile, std::string* src, std::string* capped = nullptr) {
    const int wpt = waves_per_tile & 0xFF;
    const bool prune = (waves_per_tile & RM_JIT_PRUNE) != 0;
    if (wpt != 1 && wpt != 2 && wpt != 4 && wpt != 8) return RM_ERR_ARG;
    RmDecoded d;
    int rc = rm_decode_program(cmd_count, words, n_words, &d);
    if (rc != RM_OK) return rc;
    int kind = !prune ? rmjit::PRUNE_NONE : d.unit_mode == RM_UNITS_LATTICE ? rmjit::PRUNE_LATTICE : d.unit_mode == RM_UNITS_BLEND ? rmjit::PRUNE_BLEND : rmjit::PRUNE_NONE;
    if ((waves_per_tile & RM_JIT_RANGE_PROVED) != 0) kind |= rmjit::KERNEL_RANGE_PROVED;  // (taken by the programs that have the variant)
    if (!rmjit::can_specialise(d.rec) || !rmjit::generate_source(d.rec, d.mrec, wpt, kind, src, nullptr, nullptr, capped)) return RM_ERR_ARG;
    return RM_OK;
}
void copy_out(const std::string& s, char* buf, size_t cap) {
    if (!buf || !cap) return;
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
}
}  // namespace

RM_EXPORT int rm_jit_source(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, int waves_per_tile, char* buf,
                            size_t cap, size_t* needed) {
    std::string src;
    int rc = jit_decode(cmd_count, words, n_words, waves_per_tile, &src);
    if (rc != RM_OK) return rc;
    if (needed) *needed = src.size() + 1;
    copy_out(src, buf, cap);
    return RM_OK;
}

RM_EXPORT int rm_jit_compile(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, int waves_per_tile,
                             double* compile_ms, size_t* code_bytes, char* log, size_t log_cap) {
    std::string src, capped, msg;
    int rc = jit_decode(cmd_count, words, n_words, waves_per_tile, &src, &capped);
    if (rc != RM_OK) return rc;
    std::vector<char> code;
    double ms = 0.0;
    const bool ok = rmjit::compile_best(src, capped, &code, &msg, &ms);  // (what a draw would get: the disk cache is warmed through here)
    if (compile_ms) *compile_ms = ms;
    if (code_bytes) *code_bytes = code.size();
    copy_out(msg, log, log_cap);
    return ok ? RM_OK : RM_ERR_DEVICE;
}

RM_EXPORT int rm_jit_log(rm_ctx* c, char* buf, size_t cap) {
    if (!c) return RM_ERR_NULL;
    std::string msg;
    if (c->spec) {
        std::lock_guard<std::mutex> lk(c->spec->m);
        msg = c->spec->log;
    }
    copy_out(msg, buf, cap);
    return RM_OK;
}

RM_EXPORT const char* rm_last_error(rm_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

RM_EXPORT const char* rm_status_string(int status) {
    switch (status) {
    case RM_OK: return "ok";
    case RM_ERR_NULL: return "null pointer";
    case RM_ERR_TRUNCATED: return "command reads past the end of the command buffer";
    case RM_ERR_STACK_UNDERFLOW: return "binary operator with fewer than two operands on the value stack";
    case RM_ERR_STACK_OVERFLOW: return "value stack deeper than 32";
    case RM_ERR_EMPTY_RESULT: return "program leaves no value on the stack";
    case RM_ERR_OPCODE: return "unknown opcode";
    case RM_ERR_TOO_LARGE: return "write exceeds buffer size";
    case RM_ERR_RANGE: return "image size or row band out of range";
    case RM_ERR_DEVICE: return "HIP runtime error";
    case RM_ERR_NO_DEVICE: return "no GPU available";
    case RM_ERR_ARG: return "invalid argument";
    case RM_ERR_TRANSFORM: return "transform push/pop commands are not properly nested around one value";
    case RM_ERR_MATERIAL: return "material index outside the material table";
    default: return "unknown status";
    }
}
