/*
 * rm_abi.h -- C ABI of the MI355X-native SDF ray-marching render path (librm_hip.so).
 *
 * This is the drop-in boundary for the `src/ray_marching` wgpu pipeline of
 * Mesoptier/ray-marching.  Everything the reference's `RayMarchingCallback::prepare`
 * hands to the GPU is three flat byte blobs (limits, CSG command buffer, uniforms) and
 * one draw; this header exposes exactly that.  All citations are file:line relative to
 * the reference root.
 *
 *   reference (Rust/wgpu)                                   this ABI
 *   ------------------------------------------------------  ---------------------------
 *   RayMarchingResources::new          renderer.rs:51-175   rm_create
 *   (drop of RayMarchingResources)                          rm_destroy
 *   queue.write_buffer(uniforms, 0,..) renderer.rs:213-222  rm_write_buffer(RM_BUF_UNIFORMS) / rm_set_uniforms
 *   queue.write_buffer(cmd_buffer,0,..) renderer.rs:230-234 rm_write_buffer(RM_BUF_COMMANDS, 0, &cmd_count, 4)
 *   queue.write_buffer(cmd_buffer,4,..) renderer.rs:235-239 rm_write_buffer(RM_BUF_COMMANDS, 4, words, 4*n) / rm_set_program
 *   create_buffer_init(limits)         renderer.rs:130-140  rm_write_buffer(RM_BUF_LIMITS) / rm_set_limits
 *   render_pass.draw(0..4, 0..2)       renderer.rs:252-254  rm_draw   (the image is shaded once, not twice)
 *   TODO "Recreate the buffers if too small" renderer.rs:229 rm_resize_command_buffer
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returning
 * `int` returns RM_OK (0) or a negative rm_status; nothing throws or unwinds across the
 * ABI.  The caller owns every pointer it passes in; the library copies before returning.
 * An rm_ctx is bound to one GPU and is externally synchronised (one thread at a time);
 * different contexts may be used concurrently from different threads/processes.  All draws of ONE
 * context share its scratch buffers and therefore execute in the order they were issued: a draw issued
 * on another stream than the context's previous draw (a host-destination draw runs on the context's own
 * stream) first waits for everything queued on that previous stream.  Frames that should overlap use
 * one context each (RM_STREAM_OWN below).  Buffer writes are ordered with the
 * draws like queue.write_buffer is in wgpu (renderer.rs:213-239): limits and uniforms travel with each
 * draw as kernel arguments; a changed program (and the cameras of rm_draw_batch) is copied to the GPU on
 * the stream of the next draw, behind the draws already queued there, so a frame that is still in flight
 * keeps the program it was issued with.  Rewriting the command buffer with the bytes it already holds
 * (the reference does so every frame, renderer.rs:224-239) costs a memcmp and no decode or copy.
 *
 * Output image: RGBA32F, 16 bytes per pixel, row-major, top row first (framebuffer
 * orientation); pixel (px,py) has pt_screen = (-1 + 2(px+.5)/W, 1 - 2(py+.5)/H), the
 * mapping vs_main + the rasteriser imply (ray_marching.wgsl:7-20).
 */
#ifndef RM_ABI_H
#define RM_ABI_H

#if !defined(__HIPCC_RTC__) /* hipRTC provides the fixed-width types itself */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RM_ABI_VERSION 2 /* 2: kernel variants 2..11 (v2-v4) retired; rm_gather_strips, rm_host_register added */

typedef struct rm_ctx rm_ctx;

/* binding 2: `Uniforms` (ray_marching.wgsl:22-31 <-> renderer.rs:29-34), 144 bytes,
 * matrices column-major, as produced by encase's UniformBuffer::write. */
typedef struct rm_uniforms {
    float viewport_extent[2]; /* byte 0  */
    float _pad[2];            /* byte 8  */
    float inv_proj[16];       /* byte 16 */
    float inv_view[16];       /* byte 80 */
} rm_uniforms;

/* binding 0: `RayMarchLimits` (ray_marching.wgsl:78-85 <-> renderer.rs:36-41), 12 bytes. */
typedef struct rm_limits {
    float min_dist;
    float max_dist;
    uint32_t max_iter;
} rm_limits;

/* Command stream (csg/builder.rs:1-62): u32 opcode followed by f32::to_bits parameters, post-order.
 *   reference:  Sphere 0 (c.xyz, r)   Box 1 (c.xyz, half-extents.xyz)   Union 100   Subtraction 101
 *   extensions (NOT implemented by the reference, semantics in DESIGN.md section 8; only the v5 kernels):
 *               Plane 2 (n.xyz, h)   Cylinder 10 (c.xyz, r, half_h)   Intersection 102   SmoothUnion 110 (k)
 *               space transformations, the slots the reference reserves by comment (builder.rs:16-23), written
 *               Push(params), <one child>, Pop:  TranslationPush 200 (t.xyz) / Pop 201   RotationPush 202 (unit
 *               quaternion w,i,j,k) / Pop 203   ScalePush 204 (uniform s) / Pop 205
 * Any other opcode is rejected with RM_ERR_OPCODE. */

/* binding numbers of the reference's bind group (renderer.rs:60-94, 149-166) */
enum rm_buffer {
    RM_BUF_LIMITS = 0,   /* 12 B,  initial {0.01, 100.0, 100}      renderer.rs:130-140 */
    RM_BUF_COMMANDS = 1, /* 1024 B, u32 cmd_count @0, u32 words @4 renderer.rs:142-147, wgsl:146-151 */
    RM_BUF_UNIFORMS = 2  /* 144 B, initial all-zero                 renderer.rs:124-128 */
};

enum rm_status {
    RM_OK = 0,
    RM_ERR_NULL = -1,            /* required pointer is NULL */
    RM_ERR_TRUNCATED = -2,       /* a command reads past the end of the command buffer */
    RM_ERR_STACK_UNDERFLOW = -3, /* binary operator with fewer than two operands (UB in wgsl:177-180) */
    RM_ERR_STACK_OVERFLOW = -4,  /* value stack deeper than 32 (wgsl:173) */
    RM_ERR_EMPTY_RESULT = -5,    /* program leaves nothing on the stack */
    RM_ERR_OPCODE = -6,          /* opcode the reference does not define (wgsl:223-225 would yield 0.0) */
    RM_ERR_TOO_LARGE = -7,       /* write past the end of a buffer / program larger than the buffer */
    RM_ERR_RANGE = -8,           /* row band / image size out of range, or max_iter > 65536 */
    RM_ERR_DEVICE = -9,          /* a HIP call failed; see rm_last_error */
    RM_ERR_NO_DEVICE = -10,      /* no usable GPU */
    RM_ERR_ARG = -11,            /* invalid enum / option value, or a misaligned device array of a scene query */
    RM_ERR_TRANSFORM = -12,      /* transform push / pop (extension opcodes 200-205) not nested properly, deeper than 8,
                                    or not around exactly one value */
    RM_ERR_MATERIAL = -13        /* a Material tag (extension opcode 300) names an index >= 256, or (at draw time) one
                                    the material table does not have */
};

/* rm_set_option / rm_get_info keys */
enum rm_option {
    RM_OPT_KERNEL = 0,     /* which kernel rm_draw launches; see enum rm_kernel */
    RM_OPT_TIMING = 1,     /* 1: bracket every launch of the dominant (march) kernel with HIP events on its stream,
                              without synchronising; read with rm_get_info(RM_INFO_KERNEL_MS) */
    RM_OPT_STRICT_CAP = 2, /* reserved */
    RM_OPT_REFILL_MIN = 3, /* idle lanes of a wave that trigger a refill from the tile's ray pool, 1..64; 0 (default): 64 -- a wave
                              marches its 64 rays in step -- when the kernel prunes far primitives, else 1 */
    RM_OPT_CULL = 4,       /* 1 (default) = shade rays that provably miss the scene without marching (exact) */
    RM_OPT_BALANCE = 5,    /* dispatch order of the tiles that need marching (it never changes a pixel): 0 raster order;
                              1 most pending pixels first; 2 partially covered tiles first; 3 (default) the tiles that
                              took longest in the context's previous draw of the same shape first -- consecutive frames
                              of a view look alike, and a kernel that ends on its shortest tiles has no tail
                              (one frame at a time: +6-9 %); the first draw of a shape falls back to 1 */
    RM_OPT_WAVES_PER_TILE = 7, /* waves (1, 2, 4, 8) sharing one tile's ray pool; 0 (default): 4, or 8 for a launch of at most
                                  6000 tiles, whose duration is the latency of its heaviest tile */
    RM_OPT_WAVE_STATS = 6, /* diagnostics: the v5 kernels record per-wave timing/loop statistics (rm_read_wave_stats) */
    RM_OPT_OUTPUT_FORMAT = 10, /* enum rm_format: what rm_draw / rm_draw_strips / rm_draw_batch write (default RM_FORMAT_RGBA32F).
                                  The 8-bit formats are the output stage of SURVEY 8(f)-3: the reference's own colour target is
                                  the 8-bit egui surface (renderer.rs:113).  Only the default (v5) kernels implement them. */
    RM_OPT_PRUNE = 9,      /* specialised kernels: skip, per wave and per march step, primitives that provably cannot
                              influence the scene value there (exact; DESIGN.md "Pruning"): 0 never, 1 always, 2 (default)
                              for programs with at least 12 spheres + boxes -- on MI355X the wave-uniform tests cost more
                              than they save at 4 primitives (-6 %) and pay from there on (+6 % at 16, +14 % at 32) */
    RM_OPT_SPECIALIZE = 8  /* structure specialisation of the default (v5) march kernel: the command sequence is compiled
                              into straight-line code with hipRTC, once per program STRUCTURE (parameters stay data);
                              results are bit-identical to the interpreter kernel.
                              0 = never; 1 (default) = compile on a background thread, draw with the interpreter kernel
                              until the compiled one is ready; 2 = the first draw of a new structure waits for the compiler.
                              Without libhiprtc, or if compilation fails, the interpreter kernel keeps drawing. */
};
/* Pixel formats of the output image (row-major, top row first).  The 8-bit formats quantise the RGBA32F value the
 * shader returns (wgsl:73-75) the way a UNORM colour target does: clamp to [0,1] (NaN -> 0), times 255, round to nearest
 * even; alpha is 255.  "out_rgba" pointers then address 4 bytes per pixel instead of 16. */
enum rm_format {
    RM_FORMAT_RGBA32F = 0,      /* 16 B/pixel: r, g, b, a as binary32 */
    RM_FORMAT_RGBA8_UNORM = 1,  /* 4 B/pixel: bytes r, g, b, a */
    RM_FORMAT_BGRA8_UNORM = 2   /* 4 B/pixel: bytes b, g, r, a (wgpu's usual surface format) */
};
enum rm_kernel {
    RM_KERNEL_DEFAULT = 0,   /* the tuned kernel: v5 with the program staged in LDS, its march kernel compiled per program
                                structure (RM_OPT_SPECIALIZE) */
    RM_KERNEL_PIXEL = 1,     /* v1: north_star's literal design -- one thread per pixel, program staged in LDS, lock-step AA
                                and march loops (reference node types only); kept as the A/B reference point */
    /* 2..11 were the v2-v4 ray-pool / queue experiments of ABI version 1; retired (DESIGN.md 5 keeps their measurements) */
    /* v5: ray pool shared by the waves of a tile, full-width ray production / shading through per-wave LDS buffers, exact
       miss tests, persistent workgroups over a sorted work list; the interpreter form (RM_OPT_SPECIALIZE = 0) of the default */
    RM_KERNEL_V5 = 12,       /* program read through the scalar cache (what programs too long for LDS fall back to) */
    RM_KERNEL_V5_LDS = 13    /* program staged in LDS once per workgroup */
};
enum rm_info {
    RM_INFO_KERNEL_MS = 0,       /* mean duration (ms) of the march kernel over the launches timed since the last query
                                    (synchronises on them and resets the set) */
    RM_INFO_PROGRAM_COMMANDS = 1,
    RM_INFO_PROGRAM_WORDS = 2,
    RM_INFO_PROGRAM_DEPTH = 3,   /* maximum value-stack depth of the current program */
    RM_INFO_DEVICE = 4,
    RM_INFO_CU_COUNT = 5,
    RM_INFO_SPECIALIZED = 6,     /* 1 if the last march launch ran a structure-specialised kernel, else 0 */
    RM_INFO_JIT_STATE = 7,       /* specialisation of the current program: 0 none requested, 1 compiling, 2 ready, 3 failed
                                    (rm_jit_log has the reason) */
    RM_INFO_JIT_COMPILE_MS = 8,  /* wall time hipRTC took for the current program's kernel -- or the read from the disk cache
                                  * (RM_INFO_JIT_FROM_CACHE) --; 0 until it is ready */
    RM_INFO_PRUNED = 9,          /* which skipping rule the kernel requested for the current program carries (RM_OPT_PRUNE): 0 none,
                                  * 1 far-primitive pruning on a threshold (min / max programs), 2 the rules of programs that blend
                                  * with SmoothUnion along a top-level chain; both through wave-level culling */
    RM_INFO_INTERPRETER_LOOP = 10, /* record loop the interpreter kernels ran the program of the last march launch with: 0 the
                                    general one (value stack, every node type; also reported when a specialised kernel ran), 1 the chain loop ("a op b op c ...": no
                                    stack), 2 the chain loop over the records wave-level culling names (exact; the default for chains of a dozen leaves or more staged in
                                    LDS), 3 the tree loop (reference node types in any arrangement: one dispatch per record), 4 the tree loop over the
                                    records wave-level culling leaves (exact; trees of a dozen leaves or more and at most 128 records, staged in LDS), 5 the
                                    general record machine over the units of a blending chain that wave-level culling names (exact; eight leaves or more) */
    RM_INFO_JIT_FROM_CACHE = 11, /* 1 when the current program's kernel was read from the disk cache of compiled structures
                                  * (RM_JIT_CACHE_DIR; default: jit_cache next to the library) instead of being compiled */
    RM_INFO_RANGE_PROOF = 12     /* 1 when the last march launch ran the specialised kernel compiled WITHOUT the range guards that facts of
                                  * the program make unnecessary (every box half-extent at least 2^-23 in magnitude and finite, no material
                                  * table, a pruned min / max program; DESIGN.md section 5 "Range proofs"); 0 when it ran the guarded
                                  * kernel -- a program without those facts, RM_JIT_RANGE_PROOF=0 in the environment -- or an interpreter
                                  * kernel.  The frames are the same bit for bit.  (Additive: RM_ABI_VERSION stays 2.) */
};

int rm_abi_version(void);
int rm_device_count(void);

/* RayMarchingResources::new (renderer.rs:51-175).  device = HIP ordinal. */
int rm_create(int device, rm_ctx** out);
void rm_destroy(rm_ctx* ctx);

/* Queue::write_buffer(buffer, offset, data) (renderer.rs:213,230,235).  offset and size
 * must be multiples of 4 (wgpu COPY_BUFFER_ALIGNMENT) and stay inside the buffer. */
int rm_write_buffer(rm_ctx* ctx, int buffer, uint64_t offset, const void* data, uint64_t size);

/* Typed forms of the same writes. */
int rm_set_uniforms(rm_ctx* ctx, const rm_uniforms* u);
int rm_set_limits(rm_ctx* ctx, const rm_limits* l);
/* = write_buffer(cmd,0,&cmd_count) + write_buffer(cmd,4,words) after validating the program;
 * on error the command buffer is left unchanged.  cmd_count = 0 is the `csg_node == None`
 * case (renderer.rs:224-227). */
int rm_set_program(rm_ctx* ctx, uint32_t cmd_count, const uint32_t* words, uint32_t n_words);

/* Material table (extension; the reference has no materials -- README.md:11 lists them as future work -- and shades
 * every hit with (0.4, 0.7, 0.1) * diffuse, wgsl:105).  `rgb` = count x 3 floats, count in [1, 256]; entry i is the
 * albedo of the surfaces tagged by the command [300, i] (a unary postfix tag on the value on top of the stack; a
 * binary operator keeps the tag of the operand that decides its result, primitives start with tag 0).  The default
 * table is the single entry (0.4, 0.7, 0.1): programs without tags render exactly as the reference does whatever the
 * table holds in its other entries.  A draw of a program that names an index >= count fails with RM_ERR_MATERIAL.
 * Like every buffer write the table is ordered with the draws of the stream. */
int rm_set_materials(rm_ctx* ctx, uint32_t count, const float* rgb);

/* The reference's TODO (renderer.rs:229): grow the command buffer beyond 1024 bytes.
 * Contents are preserved.  bytes in [1024, 65536], multiple of 4. */
int rm_resize_command_buffer(rm_ctx* ctx, uint64_t bytes);

/* Validate the current command-buffer contents without drawing. */
int rm_validate(rm_ctx* ctx);

/* Context-free validation of a program in the reference wire format (pure host code, usable
 * without a GPU): the checks the reference leaves as UB (wgsl:177-185) or as a wgpu panic.
 * out_max_depth (nullable) receives the deepest value-stack use of the reference machine. */
int rm_validate_program(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, uint32_t* out_max_depth);

/* Diagnostics (pure host code): what the upload-time decoder makes of a command stream.  out[0..n_out) receives, in this order
 * (indices RM_PROGRAM_*): records, cone entries and slab entries of the miss-test tables, leaves left out of those tables
 * because they sit in the right operand of a Subtraction, units of wave-level culling (RM_PROGRAM_GROUPS: the name is round 2's, when
 * they were pairs of leaves; 0 when the program has none), value-stack slots the accumulator machine spills, then four 0/1 facts -- chain program (stack-free interpreter loop), prunable (far-primitive pruning applies),
 * miss test on lower bounds applies, program has space transformations --, the sphere + box leaves the program evaluates
 * (subtracted ones included), and what the automatic pruning decision (RM_OPT_PRUNE = 2) gives this program: 0 the plain kernel,
 * 1 / 2 as RM_INFO_PRUNED.
 * Same status codes as rm_validate_program. */
enum rm_program_fact {
    RM_PROGRAM_RECORDS = 0, RM_PROGRAM_CONES = 1, RM_PROGRAM_SLABS = 2, RM_PROGRAM_SUBTRACTED_LEAVES = 3, RM_PROGRAM_GROUPS = 4,
    RM_PROGRAM_SPILL_DEPTH = 5, RM_PROGRAM_IS_CHAIN = 6, RM_PROGRAM_PRUNABLE = 7, RM_PROGRAM_BOUND_WALK = 8, RM_PROGRAM_HAS_XFORMS = 9,
    RM_PROGRAM_LEAVES = 10, RM_PROGRAM_AUTO_PRUNED = 11, RM_PROGRAM_FACTS = 12
};
int rm_program_info(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, uint32_t* out, uint32_t n_out);

/* paint (renderer.rs:244-255) restricted to rows [row0,row0+rows) of a W x H target.
 * out_rgba receives rows*W*4 floats.  out_is_device = 0: host memory, filled on return.
 * out_is_device = 1: device memory on ctx's GPU; the launch is asynchronous on `stream`, a
 * hipStream_t of the caller (NULL = HIP's null stream, as everywhere in HIP); the caller
 * synchronises that stream, or calls rm_sync.  `stream` is ignored for host output. */
int rm_draw(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, float* out_rgba,
            int out_is_device, void* stream);

/* One GPU's share of an image tiled over `stride` GPUs (north-star: "the image tiles across the
 * GPUs of one node with a final host-side gather"): renders the strips first, first+stride,
 * first+2*stride, ... of strip_rows rows each (strip_rows a multiple of 8: the kernels work on 8x8-pixel tiles) in ONE launch.
 * out_rgba receives them back to back; *out_rows = number of rows written (0 if this GPU has no
 * strip).  Interleaving balances the load: the costly part of a frame is usually its centre. */
int rm_draw_strips(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t first, uint32_t stride,
                   float* out_rgba, int out_is_device, void* stream, uint32_t* out_rows);

/* The final host-side gather of a tiled frame (north-star: "a final host-side gather (no RCCL collectives)"):
 * copies the strips rm_draw_strips(first, stride) wrote back to back into `strips_device` to their rows of the full
 * W x H host image `host_image` (pixel size per RM_OPT_OUTPUT_FORMAT), asynchronously on `stream` (as rm_draw's stream).
 * Every GPU of the node targets the same image -- e.g. one POSIX shared-memory segment mapped by all rank processes and
 * registered with rm_host_register -- and writes only its own rows: no rank relays another rank's pixels and the only
 * inter-process traffic is a "frame complete" flag.  With unregistered (pageable) memory the copies are synchronous. */
int rm_gather_strips(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t first, uint32_t stride,
                     const void* strips_device, void* host_image, void* stream);
/* Page-locks / unlocks caller-owned host memory (hipHostRegister) so that copies into it run asynchronously at PCIe rate. */
int rm_host_register(void* ptr, uint64_t bytes);
int rm_host_unregister(void* ptr);

/* n_frames draws that differ only in their uniforms (camera-orbit batch); frame f is
 * written at out_rgba + f*W*H*4. */
int rm_draw_batch(rm_ctx* ctx, const rm_uniforms* frames, uint32_t n_frames, uint32_t W, uint32_t H,
                  float* out_rgba, int out_is_device, void* stream);

/* Scene queries (extension): what the scene the next rm_draw would render says at a point or along a ray -- the command
 * buffer (validated like a draw's program), the limits, the uniforms and the material table as they are now.  Every float
 * is bit-identical to the oracle; queries never touch the draw state (RM_OPT_TIMING, RM_INFO_*, the
 * specialised kernel, the tile buffers).
 *   is_device = 0: every array is host memory; the call is synchronous on the context's own stream.
 *   is_device = 1: every array is device memory on the context's GPU; the call is asynchronous on `stream` (as rm_draw's,
 *                  RM_STREAM_OWN included) and ordered with the context's earlier draws and uploads.  Device arrays are
 *                  accessed a record at a time: float arrays need 4-byte alignment, out_ids of rm_query_points 8-byte,
 *                  out_hit and out_ids of rm_cast_rays 16-byte (what any allocator returns); RM_ERR_ARG otherwise.
 * Any output may be NULL (that work is skipped); RM_ERR_NULL when all are, or when an input is NULL with n > 0.  n = 0 (or
 * w*h = 0) writes nothing.  Errors: the draw's status for an invalid program, RM_ERR_RANGE for max_iter > 65536, and
 * RM_ERR_MATERIAL for a tag beyond the material table when colours are requested.
 * leaf = command index of the primitive whose value a result carries: its 0-based position in the command stream, counting
 * every command (operators, transform pushes / pops, Material tags).  Union / SmoothUnion take the right operand's leaf iff
 * b < a, Subtraction iff -b > a, Intersection iff b > a; ties and NaN keep the left operand's; transforms and tags keep it. */
#define RM_NO_ID 0xFFFFFFFFu /* no primitive (empty program, or a ray that hit no surface) */
enum rm_hit { RM_HIT_NONE = 0, RM_HIT_SURFACE = 1, RM_HIT_FLOOR = 2 };
enum rm_sample { RM_SAMPLE_CENTER = 16 }; /* rm_camera_rays: the ray through the pixel centre; 0..15 are fs_main's AA samples */
/* A set of samples where rm_sample names one (rm_draw_gbuffer's `sample` takes either): all sixteen AA samples.  An enum of
 * its own: rm_sample stays the list of values rm_camera_rays accepts. */
enum rm_sampleset { RM_SAMPLE_ALL = 17 };
/* Points.  xyz: n x 3.  out_dist: n, map_scene(p) (an empty program: limits.max_dist).  out_normal: n x 3, calculate_normal(p)
 * (wgsl:135-144) normalised as the shading does (NaN where the tap sum is zero).  out_ids: n x 2 (leaf, material); an empty
 * program gives (RM_NO_ID, 0). */
int rm_query_points(rm_ctx* ctx, uint32_t n, const float* xyz, float* out_dist, float* out_normal, uint32_t* out_ids,
                    int is_device, void* stream);
/* Rays (ray_march, wgsl:87-131; the direction is used as given).  rays: n x 6 (ox, oy, oz, dx, dy, dz).
 * out_hit: n x 8 (t, x, y, z, nx, ny, nz, diffuse): surface -- the march distance and position of the hit step, the shading
 * normal, max(0.02, n.l); floor -- floor_dist, (x, -1.5, z), (0, 1, 0), 0; none -- +inf and zeros.
 * out_ids: n x 4 (kind RM_HIT_*, steps = map_scene evaluations of the march loop, leaf, material; RM_NO_ID unless a surface).
 * out_rgb: n x 3, the colour ray_march returns (with the context's material table). */
int rm_cast_rays(rm_ctx* ctx, uint32_t n, const float* rays, float* out_hit, uint32_t* out_ids, float* out_rgb,
                 int is_device, void* stream);
/* The rays rm_draw marches for AA sample `sample` (0..15: (i, j) = (sample / 4, sample % 4), wgsl:44-53; or
 * RM_SAMPLE_CENTER) of the pixels of the w x h block at (x0, y0) of a W x H frame, row-major.  out_rays: w*h x 6, as
 * rm_cast_rays reads them. */
int rm_camera_rays(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                   uint32_t sample, float* out_rays, int is_device, void* stream);

/* Ray traversal (extension): every crossing of the level set along a ray over [T_MIN, T_MAX], in
 * order -- where rm_cast_rays stops at the first surface.  A ray is (o, d), d used as given.  D(t) is what rm_query_points
 * returns at (ox + dx t, oy + dy t, oz + dz t) (one rounded product and one rounded sum per coordinate); inside(t) is
 * D(t) < LEVEL (NaN is outside, as in rm_extract_mesh).  Every operation is one binary32 operation in the order written;
 * fmin / fmax: NaN loses.
 *   t = T_MIN; da = D(t); in = da < LEVEL; steps = 1; events = 0; length = 0; t_enter = t
 *   while t < T_MAX and steps < MAX_STEPS:
 *       h  = fmax(|da - LEVEL| * STEP_SCALE, MIN_STEP);  tn = fmin(t + h, T_MAX)
 *       db = D(tn); steps += 1; inb = db < LEVEL
 *       if inb != in:
 *           tc = fmin(t + (tn - t) * ((da - LEVEL) / (da - db)), tn)      (rm_extract_mesh's vertex rule on [t, tn])
 *           event number `events` (stored while events < max_events): t = tc, position o + d tc, width tn - t,
 *                                                                     kind ENTER if inb else EXIT, step = steps
 *           events += 1;  if inb: t_enter = tc  else: length = length + (tc - t_enter)
 *       t = tn; da = db; in = inb
 *   if in: length = length + (t - t_enter)
 * With STEP_SCALE <= 1 / max(1, L), L from rm_program_lipschitz, no step can pass the level set in real arithmetic: what can
 * be missed is a pair of crossings closer than MIN_STEP, and each event lies within its width of a true crossing.  The call
 * accepts any scale in (0, 1]. */
enum rm_trace {
    RM_TRACE_T_MIN = 0,      /* default 0; finite */
    RM_TRACE_T_MAX = 1,      /* default 100; finite, >= T_MIN */
    RM_TRACE_MIN_STEP = 2,   /* default 0.001; finite, > 0 */
    RM_TRACE_STEP_SCALE = 3, /* default 1; (0, 1] */
    RM_TRACE_LEVEL = 4,      /* default 0; finite */
    RM_TRACE_MAX_STEPS = 5,  /* map_scene evaluations a ray may take: default 1024; integral, 1..65536 */
    RM_TRACE_PARAMS = 6
};
enum rm_tracekind { RM_TRACE_ENTER = 1, RM_TRACE_EXIT = 2 };
enum rm_traceflag { RM_TRACE_START_INSIDE = 1, RM_TRACE_END_INSIDE = 2, RM_TRACE_OUT_OF_STEPS = 4 }; /* OUT_OF_STEPS: ended with t < T_MAX */
enum rm_tracelimit { RM_TRACE_MAX_EVENTS = 64 };
/* The table above (host code; no context).  RM_ERR_NULL for a NULL out, RM_ERR_ARG when n_out < RM_TRACE_PARAMS. */
int rm_trace_defaults(float* out, uint32_t n_out);
/* rays: n x 6 as rm_cast_rays reads them.  params: RM_TRACE_PARAMS floats in host memory (n_params must be RM_TRACE_PARAMS:
 * RM_ERR_ARG; a value outside its range: RM_ERR_RANGE).  max_events K: 1..RM_TRACE_MAX_EVENTS (RM_ERR_RANGE).  flags:
 * RM_MESH_NORMALS / RM_MESH_IDS, the attributes to compute per stored event (others: RM_ERR_ARG).
 *   out_counts:    n x 4 u32 (events found -- counting past K --, steps, flags RM_TRACE_*, events stored = min(events, K))
 *   out_spans:     n x 4 f32 (the final t, length inside the solid over the interval marched, D(T_MIN), the final D)
 *   out_events:    n x K x 8 f32 (t, x, y, z, nx, ny, nz, width); an unfilled slot is (+inf, 0, ..., 0)
 *   out_event_ids: n x K x 4 u32 (kind RM_TRACE_ENTER / RM_TRACE_EXIT, step, leaf, material); unfilled (0, 0, RM_NO_ID, RM_NO_ID)
 * The normal and (leaf, material) of an event are what rm_query_points returns at its (x, y, z) when asked for in flags,
 * zeros / RM_NO_ID otherwise.  Any output may be NULL (that work is skipped; with both event arrays NULL no attribute work
 * runs); what one array receives does not depend on the others.  is_device, stream, ordering, statuses and the draw state as
 * for rm_cast_rays; every device output needs 16-byte alignment, rays 4-byte.  n = 0 writes nothing; a failed call launches
 * nothing. */
int rm_trace_rays(rm_ctx* ctx, uint32_t n, const float* rays, const float* params, uint32_t n_params, uint32_t max_events,
                  uint32_t flags, float* out_events, uint32_t* out_event_ids, uint32_t* out_counts, float* out_spans,
                  int is_device, void* stream);

/* Mesh export (extension): the scene's distance on a lattice, and its level surface as an indexed triangle mesh, from the
 * program, limits and material table as they are at the call.  Every float is bit-identical to the
 * oracle's map_scene at the lattice points; vertices and triangles follow from them by the rule below, so two runs give
 * identical arrays.
 * Lattice: origin and step are host arrays of 3 floats (finite; step > 0); point (i, j, k) is (ox + (float)i * sx,
 * oy + (float)j * sy, oz + (float)k * sz), its linear index i + nx * (j + ny * k).
 * Inside: d < level (NaN is outside).  One vertex on each lattice edge (p, p + e_a) whose ends differ, at
 * t = (da - level) / (da - db) along axis a; vertices ordered by (linear index of p, axis).  Triangles: per cell (anchored
 * at its lowest corner, ordered by linear cell index) the entries of the case table (rm_mesh_case_table), wound
 * counter-clockwise seen from outside (the geometric normal points toward larger d).  The mesh is open where the surface
 * meets the lattice's border. */
enum rm_mesh { RM_MESH_NORMALS = 1, RM_MESH_IDS = 2 }; /* flags of rm_extract_mesh: per-vertex attributes to compute */
/* map_scene at the nx x ny x nz points (1..65536 per axis, at most 2^31 in all; RM_ERR_RANGE otherwise) into out_dist,
 * x fastest.  is_device and stream as for rm_query_points; a device out_dist needs 4-byte alignment. */
int rm_sample_grid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                   float* out_dist, int is_device, void* stream);
/* Extracts the surface d = level (finite) on the lattice (2..65536 points per axis, at most 2^28 in all; RM_ERR_RANGE
 * otherwise) into buffers the context owns until its next rm_extract_mesh or rm_destroy; out_counts[0] = vertices,
 * [1] = triangles.  Synchronous on the context's own stream, ordered after its earlier work.  flags: RM_MESH_NORMALS and
 * RM_MESH_IDS add per-vertex normal and (leaf, material), exactly what rm_query_points returns at the vertex positions.
 * Errors: those of a query for the program and limits; RM_ERR_DEVICE when device memory runs out (about 10 bytes per
 * lattice point of scratch, plus the mesh). */
int rm_extract_mesh(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                    float level, uint32_t flags, uint64_t* out_counts);
/* Copies the last extracted mesh out: out_vertices V x 3, out_triangles T x 3 (vertex indices), out_normals V x 3, out_ids
 * V x 2 (leaf, material); any may be NULL.  RM_ERR_ARG before any extraction, or for normals / ids that extraction did not
 * compute.  is_device and stream as for rm_query_points (device arrays: out_ids 8-byte aligned, the others 4-byte); the
 * next rm_extract_mesh waits for a device read that is still running. */
int rm_read_mesh(rm_ctx* ctx, float* out_vertices, uint32_t* out_triangles, float* out_normals, uint32_t* out_ids,
                 int is_device, void* stream);
/* The case table of rm_extract_mesh (host code; no context): 256 cases x 16 words.  out[16 * case] = triangle count (0..5),
 * out[16 * case + 1 + 3 * t + m] = the cube edge of vertex m of triangle t, 0xFFFFFFFF after the last.  Case = sum over
 * corners c of inside(c) << c, corner c at (c & 1, c >> 1 & 1, c >> 2 & 1); edge e runs along axis e >> 2 from the corner
 * with 0 on it to the one with 1, bit 0 / bit 1 of e & 3 its offset on the lower / higher other axis.  RM_ERR_ARG when
 * n_out < 4096. */
int rm_mesh_case_table(uint32_t* out, uint32_t n_out);
/* Sparse extraction: the mesh of rm_extract_mesh -- the same vertices bit for bit, the same
 * triangles, the same order, the same attributes -- computed only where the surface can be.  The lattice is cut into bricks
 * of 8 x 8 x 8 points; one map_scene probe per brick and a Lipschitz bound of the program (rm_program_lipschitz) prove for
 * most bricks that none of their edges crosses `level`, and only the others are evaluated.  Skipping never changes an
 * output bit, only the statistics.  Lattice: 2..65536 points per axis and no limit on the product (beyond 2^28 points the
 * rule of rm_extract_mesh defines the mesh with 64-bit linear indices).  out_stats[RM_MESH_STAT_*]:
 *   VERTICES, TRIANGLES   of the mesh (what rm_extract_mesh returns in out_counts)
 *   BRICKS, BRICKS_KEPT   bricks of the lattice, and those that were evaluated
 *   EVALUATIONS           map_scene evaluations at brick probes and lattice points (not the attribute queries)
 *   SCRATCH_BYTES         device memory the call used besides the arrays rm_read_mesh returns
 * The result replaces the context's mesh like rm_extract_mesh's (rm_read_mesh reads the last extraction of either kind);
 * synchronous on the context's own stream, ordered after its earlier work; never touches the draw state.
 * Errors: those of rm_extract_mesh; RM_ERR_NULL for a NULL out_stats, RM_ERR_ARG for n_stats < RM_MESH_STATS, RM_ERR_RANGE
 * when vertices or triangles would not fit a 32-bit index, RM_ERR_DEVICE when device memory runs out. */
enum rm_meshstat { RM_MESH_STAT_VERTICES = 0, RM_MESH_STAT_TRIANGLES = 1, RM_MESH_STAT_BRICKS = 2,
                    RM_MESH_STAT_BRICKS_KEPT = 3, RM_MESH_STAT_EVALUATIONS = 4, RM_MESH_STAT_SCRATCH_BYTES = 5,
                    RM_MESH_STATS = 6 };
int rm_extract_mesh_sparse(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                           float level, uint32_t flags, uint64_t* out_stats, uint32_t n_stats);
/* A Lipschitz bound of the program's map_scene in real arithmetic (host code; no context):
 * |map_scene(p) - map_scene(q)| <= L |p - q| for all p, q.  Sphere, Box, Cylinder 1; Plane |n|; the operators the maximum
 * of their operands; Translation and Scale unchanged; Rotation (w, a) times max(1, sqrt((1 - 2|a|^2)^2 + 4 w^2 |a|^2)), which
 * is 1 for a unit quaternion.  The empty program: 0.  +infinity when there is no bound: a parameter that is not finite, or
 * a Scale of 0.  Errors: rm_validate_program's status for an invalid program, RM_ERR_NULL for a NULL out_L. */
int rm_program_lipschitz(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, double* out_L);

/* Mass properties (extension; DESIGN.md section 17 is the contract, to the last bit): integer moments of the solid d < level
 * on a lattice, and volume, centre of mass, inertia tensor and bounding box from them.
 * Lattice, values and "inside" are rm_extract_mesh's: point (i, j, k) lies at o + (float)i * s per axis, its value is what
 * rm_query_points returns there for the program and limits at the call (the empty program: max_dist), and it is inside iff
 * d < level (NaN is outside).  out_moments[RM_MOMENT_*], over the inside points (i, j, k):
 *   COUNT                 their number N
 *   X, Y, Z               sum i, sum j, sum k
 *   XX, YY, ZZ            sum i^2, sum j^2, sum k^2
 *   XY, YZ, XZ            sum i j, sum j k, sum i k
 *   MIN_*, MAX_*          the smallest and the largest inside index per axis; for an empty solid 0xFFFFFFFF and 0
 * All are integers and integer addition is associative, so the words do not depend on any order: two runs, and any correct
 * implementation, give identical words.  Lattice: 2..4096 points per axis (RM_ERR_RANGE otherwise) and no limit on the
 * product.  With that limit no sum overflows: N <= 4096^3 = 2^36 and every term (an index below 2^12, or a product of two)
 * is below 2^24, so every sum is below 2^60.
 * Bricks: section 15's rule, unchanged and on the same tile, decides which bricks of 8 x 8 x 8 points are evaluated
 * (BRICKS_KEPT is rm_extract_mesh_sparse's for the same lattice and level).  A brick's own points are a subset of its tile, so
 * a brick proven clear lies wholly on the side of its probe: inside (probe < level) it contributes the closed-form moments of
 * its index box and no evaluation, outside nothing.  out_stats[RM_MASS_STAT_*]:
 *   BRICKS, BRICKS_KEPT   bricks of the lattice, and those that were evaluated point by point
 *   BRICKS_INSIDE         bricks proven wholly inside
 *   EVALUATIONS           map_scene evaluations: one probe per brick and the kept bricks' own points
 *   SCRATCH_BYTES         device memory the call used
 * Synchronous on the context's own stream, ordered after its earlier work; never touches the draw state and replaces neither
 * the context's mesh nor its slices.  Errors: RM_ERR_NULL for a NULL output, RM_ERR_ARG for n_moments < RM_MOMENTS,
 * n_stats < RM_MASS_STATS, a level, origin or step that is not finite or a step <= 0; RM_ERR_TOO_LARGE and RM_ERR_DEVICE as
 * for rm_extract_mesh_sparse; otherwise those of a query for the program and limits. */
enum rm_moment { RM_MOMENT_COUNT = 0, RM_MOMENT_X = 1, RM_MOMENT_Y = 2, RM_MOMENT_Z = 3, RM_MOMENT_XX = 4, RM_MOMENT_YY = 5,
                 RM_MOMENT_ZZ = 6, RM_MOMENT_XY = 7, RM_MOMENT_YZ = 8, RM_MOMENT_XZ = 9, RM_MOMENT_MIN_X = 10,
                 RM_MOMENT_MIN_Y = 11, RM_MOMENT_MIN_Z = 12, RM_MOMENT_MAX_X = 13, RM_MOMENT_MAX_Y = 14, RM_MOMENT_MAX_Z = 15,
                 RM_MOMENTS = 16 };
enum rm_massstat { RM_MASS_STAT_BRICKS = 0, RM_MASS_STAT_BRICKS_KEPT = 1, RM_MASS_STAT_BRICKS_INSIDE = 2,
                   RM_MASS_STAT_EVALUATIONS = 3, RM_MASS_STAT_SCRATCH_BYTES = 4, RM_MASS_STATS = 5 };
int rm_mass_moments(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                    uint64_t* out_moments, uint32_t n_moments, uint64_t* out_stats, uint32_t n_stats);
/* Volume, mass, centre of mass, inertia tensor about the centre of mass and bounding box from the moments of rm_mass_moments
 * on the lattice (origin, step) (host code; no context), by the midpoint rule: each inside point stands for a cell of volume
 * dV = sx sy sz centred on it.  All arithmetic is binary64.  out[RM_MASS_*]:
 *   VOLUME = N dV, MASS = density VOLUME, C_a = o_a + s_a S_a / N
 *   central second moments from exact integers: D_ab = N S_ab - S_a S_b (128-bit), mu_ab = s_a s_b D_ab / N^2, plus
 *   s_a^2 / 12 on the diagonal for the cell's own extent; IXX = MASS (mu_yy + mu_zz), ..., IXY = -MASS mu_xy, ...
 *   LO_a = o_a + min_a s_a, HI_a = o_a + max_a s_a (the outermost inside points, not their cells' faces)
 * N = 0: volume, mass, centre and inertia 0, LO = +infinity, HI = -infinity.  This is a first-order quadrature of the solid
 * (volume error at most surface area x sqrt(3) max(step)) and exact as a statement about the lattice.
 * Errors: RM_ERR_NULL for a NULL pointer, RM_ERR_ARG for n_moments < RM_MOMENTS, n_out < RM_MASS_PROPS, a density, origin or
 * step that is not finite, or a step <= 0. */
enum rm_massprop { RM_MASS_VOLUME = 0, RM_MASS_MASS = 1, RM_MASS_CX = 2, RM_MASS_CY = 3, RM_MASS_CZ = 4, RM_MASS_IXX = 5,
                   RM_MASS_IYY = 6, RM_MASS_IZZ = 7, RM_MASS_IXY = 8, RM_MASS_IYZ = 9, RM_MASS_IXZ = 10, RM_MASS_LO_X = 11,
                   RM_MASS_LO_Y = 12, RM_MASS_LO_Z = 13, RM_MASS_HI_X = 14, RM_MASS_HI_Y = 15, RM_MASS_HI_Z = 16,
                   RM_MASS_PROPS = 17 };
int rm_mass_from_moments(const uint64_t* moments, uint32_t n_moments, const float* origin, const float* step, double density,
                         double* out, uint32_t n_out);

/* Solid topology (extension; DESIGN.md section 19 is the contract, to the last bit): is the part one piece, does it enclose
 * voids, does it have through-holes -- and the moments of every piece.
 * Lattice, values and "inside" are rm_mass_moments': point (i, j, k) lies at o + (float)i * s per axis, its value is what
 * rm_query_points returns there (the empty program: max_dist), inside iff d < level (NaN is outside), linear index
 * i + nx * (j + ny * k).  2..1024 points per axis and at most 2^28 in all (RM_ERR_RANGE otherwise).
 * Adjacency (the complementary pair): BODIES are the connected components of the inside points under 6-adjacency (face
 * neighbours), VOIDS those of the outside points under 26-adjacency (face, edge and corner neighbours).  The lattice counts as
 * surrounded by one layer of outside points: every void with a point on the lattice's border belongs to THE EXTERIOR, every
 * other void is a CAVITY.  Two cubes that touch along an edge or at a corner are two bodies, and the gap joins the voids.
 * Canonical numbers: a component's label is the smallest linear index among its points; bodies are numbered 0..B-1 and
 * cavities 0..C-1 in ascending order of it.  out_counts[RM_TOPO_*]:
 *   BODIES, CAVITIES      B and C
 *   POINTS                V, the inside points (RM_MOMENT_COUNT of rm_mass_moments on the same lattice and level)
 *   EDGES, FACES, CELLS   E, F, K: the pairs of face-adjacent inside points, the unit squares whose four corners are inside,
 *                         the unit cubes whose eight corners are
 *   EULER                 V - E + F - K, a two's-complement int64
 *   TUNNELS               B + C - EULER, a two's-complement int64: the first Betti number of the cubical complex (through-holes
 *                         and handles, summed over the bodies)
 *   EXTERIOR_POINTS       the outside points of the exterior
 * Per body, and per cavity over its (outside) points, a row of the sixteen RM_MOMENT_* words; rm_mass_from_moments turns a row
 * into that component's volume, centre, inertia and box, and the body rows combine entry by entry (sum 0-9, minimum 10-12,
 * maximum 13-15) into rm_mass_moments' words.  The label volume: one u32 per point, x fastest -- an inside point holds its
 * body's number, a cavity point RM_TOPO_CAVITY_BIT | its cavity's number, an exterior point RM_TOPO_EXTERIOR.
 * Every output is an integer that no order of execution changes: two runs, and any correct implementation, give identical
 * words.  out_stats[RM_TOPO_STAT_*]: BRICKS, BRICKS_KEPT, BRICKS_INSIDE, EVALUATIONS as rm_mass_moments reports them for the
 * same lattice and level (0 for rm_label_occupancy); MERGE_PASSES, the merge passes over the union-find that ran (1 unless a
 * verification found a pair of neighbours with different roots; after 8 the call fails with RM_ERR_DEVICE); SCRATCH_BYTES,
 * the device memory the call used besides the label volume and the rows.
 * rm_label_occupancy labels the caller's occupancy instead: one byte per point, x fastest, nonzero = inside; in host memory, or
 * (is_device) in device memory, read after the work queued on `stream` (RM_STREAM_OWN: the context's).
 * Both are synchronous on the context's own stream, ordered after its earlier work; they never touch the draw state, and the
 * result lives in buffers of its own until the next labelling call or rm_destroy: it replaces neither the context's mesh nor
 * its slices.  Errors (every check precedes the first launch, and a failed call leaves the outputs untouched): RM_ERR_NULL for
 * a NULL output or occupancy; RM_ERR_ARG for n_counts < RM_TOPO_COUNTS, n_stats < RM_TOPO_STATS, a level, origin or step that
 * is not finite or a step <= 0; RM_ERR_RANGE for the lattice; RM_ERR_DEVICE when device memory runs out (about 10 bytes per
 * point, and 128 per component once B and C are known); otherwise those of a query for the program and limits. */
#define RM_TOPO_CAVITY_BIT 0x80000000u /* label volume: this bit | the cavity's number */
#define RM_TOPO_EXTERIOR 0xFFFFFFFFu   /* label volume: a point of the exterior */
enum rm_topocount { RM_TOPO_BODIES = 0, RM_TOPO_CAVITIES = 1, RM_TOPO_POINTS = 2, RM_TOPO_EDGES = 3, RM_TOPO_FACES = 4,
                    RM_TOPO_CELLS = 5, RM_TOPO_EULER = 6, RM_TOPO_TUNNELS = 7, RM_TOPO_EXTERIOR_POINTS = 8, RM_TOPO_COUNTS = 9 };
enum rm_topostat { RM_TOPO_STAT_BRICKS = 0, RM_TOPO_STAT_BRICKS_KEPT = 1, RM_TOPO_STAT_BRICKS_INSIDE = 2,
                   RM_TOPO_STAT_EVALUATIONS = 3, RM_TOPO_STAT_MERGE_PASSES = 4, RM_TOPO_STAT_SCRATCH_BYTES = 5, RM_TOPO_STATS = 6 };
int rm_label_solid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                   uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_label_occupancy(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                       uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
/* Copies the last labelling out: out_body_moments B x 16 u64, out_cavity_moments C x 16 u64, out_labels nx * ny * nz u32; any
 * may be NULL.  RM_ERR_ARG before any labelling.  is_device and stream as for rm_query_points (device arrays: the moments
 * 8-byte aligned, the labels 4-byte); the next labelling call waits for a device read that is still running. */
int rm_read_topology(rm_ctx* ctx, uint64_t* out_body_moments, uint64_t* out_cavity_moments, uint32_t* out_labels,
                     int is_device, void* stream);

/* Distance transform (extension; DESIGN.md section 20 is the contract, to the last bit): how thick is the part, how wide are
 * its gaps -- the exact squared Euclidean distance transform of the occupancy lattice, the largest inscribed ball, and the
 * material (the clearance) that no ball of a given radius fits into.
 * Lattice, values, "inside" and limits are rm_label_solid's: point (i, j, k) at o + (float)i * s per axis, inside iff
 * rm_query_points' distance < level (NaN is outside; the empty program: max_dist), linear index i + nx * (j + ny * k), 2..1024
 * points per axis and at most 2^28 in all (RM_ERR_RANGE otherwise), and the lattice counts as surrounded by ONE LAYER OF
 * OUTSIDE POINTS: every point with a coordinate of -1, or of n on that axis.
 * Distance is measured in index space, exactly.  For an inside point p, D2(p) is the minimum of |p - q|^2 over all outside
 * points q, the surrounding layer included (so never more than min(i+1, nx-i, j+1, ny-j, k+1, nz-k)^2).  For an outside point
 * p, D2(p) is the minimum of |p - q|^2 over all inside points q of the lattice; the layer plays no part, and when the solid is
 * empty D2 = RM_DIST_NONE.  Every finite value is below 3 * 1023^2 < 2^22.  World distance is step * sqrt(D2) when the three
 * steps are equal; this interface stays in index units.
 * The distance volume: one u32 per point, x fastest -- D2, with RM_DIST_INSIDE_BIT ORed in for an inside point.
 * out_counts[RM_DIST_*]:
 *   POINTS                      the inside points (RM_TOPO_POINTS on the same lattice)
 *   MAX_INSIDE, ARGMAX_INSIDE   the largest inside D2 and the smallest linear index that attains it: squared radius and centre
 *                               of the largest inscribed ball.  An empty solid: 0 and 0xFFFFFFFF
 *   MAX_OUTSIDE, ARGMAX_OUTSIDE the same over the outside points.  A full lattice: 0 and 0xFFFFFFFF; an empty solid:
 *                               RM_DIST_NONE and 0
 * out_stats[RM_DIST_STAT_*]: BRICKS, BRICKS_KEPT, BRICKS_INSIDE, EVALUATIONS as rm_mass_moments reports them for the same
 * lattice and level (0 for rm_distance_occupancy); SCRATCH_BYTES, the device memory the call used besides the distance volume.
 * rm_distance_occupancy transforms the caller's occupancy instead: one byte per point, x fastest, nonzero = inside; in host
 * memory, or (is_device) in device memory, read after the work queued on `stream` (RM_STREAM_OWN: the context's).
 * rm_distance_features works on the last distance volume, with squared radii in index units (RM_DIST_SKIP skips that half):
 *   core   = { inside p : D2(p) > r2_wall }: the centres of closed balls of radius sqrt(r2_wall) that hold no outside point
 *   opened = { p : some c in core has |p - c|^2 <= r2_wall }, a subset of the inside (the morphological opening)
 *   THIN   = inside \ opened: the material that no ball of that radius fits into
 *   NARROW   the same with the classes exchanged and r2_gap: the outside points that no ball of radius sqrt(r2_gap) centred on
 *            an outside point of the lattice with D2 > r2_gap covers.  Centres lie on the lattice only: a solid nearer than
 *            2 sqrt(r2_gap) to the lattice's border can report gap points against the border.
 * The feature mask: one byte per point -- 0 outside and not narrow, 1 inside and not thin, 2 thin, 3 narrow; a skipped half
 * leaves its class at 0 or 1.  out_counts[RM_DIST_CORE, THIN, GAP_CORE, NARROW]: the points of core, thin, the gap's core and
 * narrow (0 for a skipped half).  (mask == 2) as bytes is an occupancy for rm_label_occupancy: the thin regions as bodies.
 * rm_read_distance copies the last distance volume (out_d2, nx * ny * nz u32) and the last feature mask (out_mask, one byte per
 * point) out; either may be NULL; is_device and stream as for rm_query_points (a device out_d2: 4-byte aligned); the next
 * distance call waits for a device read that is still running.
 * Every output is an integer defined by a minimum or a count: two runs, and any correct implementation, give identical words.
 * The calls are synchronous on the context's own stream, ordered after its earlier work; they never touch the draw state, and
 * the result lives in buffers of its own until the next distance call or rm_destroy: it replaces neither the context's mesh,
 * its slices nor its labelling.  Errors (every check precedes the first launch, and a failed call leaves the outputs
 * untouched): RM_ERR_NULL for a NULL output or occupancy; RM_ERR_ARG for n_counts < RM_DIST_COUNTS (features:
 * RM_DIST_FEATURE_COUNTS), n_stats < RM_DIST_STATS, a level, origin or step that is not finite or a step <= 0, for
 * rm_distance_features or rm_read_distance before any distance call, and for rm_read_distance asked for a mask that no
 * features call has made of the last volume; RM_ERR_RANGE for the lattice, and for an r2 >= 2^22 that is not RM_DIST_SKIP;
 * RM_ERR_DEVICE when device memory runs out (about 5 bytes per point, 4 more during the features); otherwise those of a query
 * for the program and limits. */
#define RM_DIST_INSIDE_BIT 0x80000000u /* distance volume: ORed into the D2 of an inside point */
#define RM_DIST_NONE 0x7FFFFFFFu       /* distance volume: the D2 of an outside point when the solid is empty */
#define RM_DIST_SKIP 0xFFFFFFFFu       /* rm_distance_features: leave this half out */
enum rm_distcount { RM_DIST_POINTS = 0, RM_DIST_MAX_INSIDE = 1, RM_DIST_ARGMAX_INSIDE = 2, RM_DIST_MAX_OUTSIDE = 3,
                    RM_DIST_ARGMAX_OUTSIDE = 4, RM_DIST_COUNTS = 5 };
enum rm_distfeature { RM_DIST_CORE = 0, RM_DIST_THIN = 1, RM_DIST_GAP_CORE = 2, RM_DIST_NARROW = 3, RM_DIST_FEATURE_COUNTS = 4 };
enum rm_diststat { RM_DIST_STAT_BRICKS = 0, RM_DIST_STAT_BRICKS_KEPT = 1, RM_DIST_STAT_BRICKS_INSIDE = 2,
                   RM_DIST_STAT_EVALUATIONS = 3, RM_DIST_STAT_SCRATCH_BYTES = 4, RM_DIST_STATS = 5 };
int rm_distance_solid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                      uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_distance_occupancy(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                          uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_distance_features(rm_ctx* ctx, uint32_t r2_wall, uint32_t r2_gap, uint64_t* out_counts, uint32_t n_counts);
int rm_read_distance(rm_ctx* ctx, uint32_t* out_d2, void* out_mask, int is_device, void* stream);

/* Overhangs and supports (extension; DESIGN.md section 21 is the contract, to the last bit): for one of the six axis directions
 * as the build direction, which points of the solid overhang, which points of the clearance a support column would fill, and
 * whether that column stands on the plate or on the part.
 * Lattice, values, "inside" and limits are rm_label_solid's and rm_distance_solid's (2..1024 points per axis, at most 2^28 in
 * all, RM_ERR_RANGE otherwise; linear index i + nx * (j + ny * k)); points beyond the lattice are outside.
 * `up` is one of RM_UP_* (RM_ERR_ARG otherwise), a its axis and n_a that axis' points.  The HEIGHT of a point is h = p_a for a
 * positive direction and n_a - 1 - p_a for a negative one; BELOW p is the point of height h - 1 with the same other two
 * coordinates; a LAYER is all points of one height, a COLUMN all points that share the other two coordinates.
 * `plate` is a height h0 in 0..n_a - 1 (RM_ERR_RANGE for more), or RM_SUPPORT_PLATE_AUTO: the lowest height that holds an
 * inside point, 0 for an empty solid.  Layers below h0 are under the plate: their points keep class 0 or 1 in the mask, count
 * in POINTS and in column 0 of the profile, and take part in nothing else.
 * `r2` is a squared reach in index units, 0..255 (RM_ERR_RANGE otherwise).  An inside point p with h > h0 is an OVERHANG iff no
 * inside point q of layer h - 1 has du^2 + dv^2 <= r2, du and dv the differences of p and q in the two in-layer coordinates
 * (the digital disc).  Inside points of layer h0 rest on the plate and never overhang.  r2 = 0: only the point directly below
 * supports; 1: 45 degrees at equal steps, with the four neighbours; 2: with eight.  The test is local, as in a slicer: material
 * in the layer below counts as built.
 * An outside point p with h >= h0 is a SUPPORT point iff the first inside point above it in its column exists and is an
 * overhang.  Its RUN is the maximal stretch of support points of its column around it; the run ends ON THE PLATE if no inside
 * point of the column has a height in [h0, h), ON THE PART otherwise.
 * The mask: one byte per point, x fastest -- 0 outside, 1 inside, 2 overhang (inside), 3 support on the plate, 4 support on the
 * part.  (mask == 2) or (mask >= 3) as bytes is an occupancy for rm_label_occupancy: overhang regions, support bodies.
 * out_counts[RM_SUP_*]:
 *   POINTS            the inside points (RM_TOPO_POINTS on the same lattice)
 *   PLATE             the h0 used
 *   BASE              the inside points of layer h0
 *   OVERHANG          the overhang points
 *   SUPPORT_ON_PLATE, SUPPORT_ON_PART   the support points whose run ends on the plate / on the part
 *   RUNS              the support points directly below an overhang point
 *   LANDINGS          the support points with h > h0 whose point below is inside
 * The profile: n_a x 4 u32 in height order (height 0 first) -- per layer its inside points, overhang points, support points on
 * the plate and support points on the part; the last three are 0 below h0.
 * out_stats[RM_SUP_STAT_*]: BRICKS, BRICKS_KEPT, BRICKS_INSIDE, EVALUATIONS as rm_mass_moments reports them for the same lattice
 * and level (0 for rm_support_occupancy); SCRATCH_BYTES, the device memory the call used besides mask and profile.
 * rm_support_occupancy analyses the caller's occupancy instead: one byte per point, x fastest, nonzero = inside; in host memory,
 * or (is_device) in device memory, read after the work queued on `stream` (RM_STREAM_OWN: the context's).
 * rm_read_support copies the last mask (out_mask, one byte per point) and the last profile (out_profile, n_a * 4 u32) out; either
 * may be NULL; is_device and stream as for rm_query_points (a device out_profile: 4-byte aligned); the next support call waits
 * for a device read that is still running.
 * Every output is a bit, a count or a minimum: two runs, and any correct implementation, give identical words.
 * The calls are synchronous on the context's own stream, ordered after its earlier work; they never touch the draw state, and
 * the result lives in buffers of its own until the next support call or rm_destroy: it replaces neither the context's mesh, its
 * slices, its labelling nor its distance volume.  Errors (every check precedes the first launch, and a failed call leaves the
 * outputs untouched): RM_ERR_NULL for a NULL output or occupancy; RM_ERR_ARG for n_counts < RM_SUP_COUNTS, n_stats <
 * RM_SUP_STATS, an `up` above 5, a level, origin or step that is not finite or a step <= 0, and for rm_read_support before any
 * support call; RM_ERR_RANGE for the lattice, r2 and plate; RM_ERR_DEVICE when device memory runs out (about 2.6 bytes per
 * point); otherwise those of a query for the program and limits. */
#define RM_SUPPORT_PLATE_AUTO 0xFFFFFFFFu /* plate: the lowest height that holds an inside point */
enum rm_up { RM_UP_POS_X = 0, RM_UP_NEG_X = 1, RM_UP_POS_Y = 2, RM_UP_NEG_Y = 3, RM_UP_POS_Z = 4, RM_UP_NEG_Z = 5 };
enum rm_supcount { RM_SUP_POINTS = 0, RM_SUP_PLATE = 1, RM_SUP_BASE = 2, RM_SUP_OVERHANG = 3, RM_SUP_SUPPORT_ON_PLATE = 4,
                   RM_SUP_SUPPORT_ON_PART = 5, RM_SUP_RUNS = 6, RM_SUP_LANDINGS = 7, RM_SUP_COUNTS = 8 };
enum rm_supstat { RM_SUP_STAT_BRICKS = 0, RM_SUP_STAT_BRICKS_KEPT = 1, RM_SUP_STAT_BRICKS_INSIDE = 2,
                  RM_SUP_STAT_EVALUATIONS = 3, RM_SUP_STAT_SCRATCH_BYTES = 4, RM_SUP_STATS = 5 };
int rm_support_solid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                     uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                     uint32_t n_stats);
int rm_support_occupancy(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                         uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                         uint32_t n_stats);
int rm_read_support(rm_ctx* ctx, void* out_mask, uint32_t* out_profile, int is_device, void* stream);

/* Layer regions and islands (extension; DESIGN.md section 22 is the contract, to the last bit): for a build direction, the
 * 4-connected REGIONS of the inside points of every layer at or above the plate, which regions of the layer below each one rests
 * on, and which are ISLANDS -- regions that start printing in mid air.
 * Lattice, "inside", `up`, height, layer, `plate` / RM_SUPPORT_PLATE_AUTO -> h0, `r2`, the digital disc, OVERHANG and the limits
 * are rm_support_solid's.  Neighbours differ by one in exactly one in-layer coordinate; layers below h0 have no regions.  A point
 * of a region is SUPPORTED iff h == h0 or it is no overhang.  A region R of layer h > h0 LINKS to Q of layer h - 1 iff some p in R
 * and q in Q have du^2 + dv^2 <= r2.  R is an ISLAND iff h > h0 and it has no supported point (iff it links to nothing), a MERGE
 * iff it links to at least two regions, a BASE region iff h == h0.  Regions are numbered 1..REGIONS by ascending (h, FIRST), FIRST
 * the smallest linear index i + nx * (j + ny * k) among the region's points.
 * out_counts[RM_ISL_*]: POINTS (all inside points, RM_SUP_POINTS), PLATE (the h0 used), REGIONS, BASE_REGIONS, ISLANDS,
 * ISLAND_POINTS, MERGES, MAX_LAYER_REGIONS (the most regions in one layer).
 * out_stats[RM_ISL_STAT_*]: as RM_SUP_STAT_* (the first four are 0 for rm_islands_occupancy).
 * rm_read_islands copies the last result out; any output may be NULL; is_device and stream as for rm_read_support (device arrays
 * of u32: 4-byte aligned):
 *   out_rows     REGIONS rows of RM_ISL_ROW_WORDS u32, row r - 1 for region r (row_capacity: the rows out_rows holds;
 *                RM_ERR_RANGE when it is below REGIONS).  A and B are the two in-layer axes in ascending axis order (up z: x, y).
 *                LAYER, FIRST, POINTS, SUPPORTED, SUM_A, SUM_B (coordinate sums), MIN_A, MAX_A, MIN_B, MAX_B (bounding box),
 *                BELOW_MIN, BELOW_MAX (the smallest and largest number of a linked region; 0, 0 without one).
 *                Island: LAYER > PLATE && BELOW_MIN == 0.  Merge: BELOW_MIN != BELOW_MAX.
 *   out_labels   one u32 per point, x fastest: the region's number for inside points with h >= h0, else 0
 *   out_mask     one byte per point: 0 outside, 1 inside, 2 inside and in an island ((mask == 2) is an occupancy for
 *                rm_label_occupancy)
 *   out_profile  n_a x 4 u32, height 0 first: per layer its inside points, regions, islands, island points (the last three 0
 *                below h0)
 * Every word is a bit, a count, a sum of small integers, a minimum or a maximum: two runs, and any correct implementation, give
 * identical words.  The calls are synchronous on the context's own stream; the result lives in buffers of its own until the next
 * islands call or rm_destroy and replaces neither the draw state, the mesh, the slices, the labelling, the distance volume nor the
 * support result.  Errors (every check precedes the first launch; a failed call leaves the outputs untouched): those of
 * rm_support_solid / rm_support_occupancy, word for word; RM_ERR_ARG for rm_read_islands before any islands call; RM_ERR_DEVICE
 * when device memory runs out (about 14.3 bytes per point, and 48 per region: a checkerboard has half its points as regions). */
enum rm_islcount { RM_ISL_POINTS = 0, RM_ISL_PLATE = 1, RM_ISL_REGIONS = 2, RM_ISL_BASE_REGIONS = 3, RM_ISL_ISLANDS = 4,
                   RM_ISL_ISLAND_POINTS = 5, RM_ISL_MERGES = 6, RM_ISL_MAX_LAYER_REGIONS = 7, RM_ISL_COUNTS = 8 };
enum rm_islstat { RM_ISL_STAT_BRICKS = 0, RM_ISL_STAT_BRICKS_KEPT = 1, RM_ISL_STAT_BRICKS_INSIDE = 2,
                  RM_ISL_STAT_EVALUATIONS = 3, RM_ISL_STAT_SCRATCH_BYTES = 4, RM_ISL_STATS = 5 };
enum rm_islrow { RM_ISL_ROW_LAYER = 0, RM_ISL_ROW_FIRST = 1, RM_ISL_ROW_POINTS = 2, RM_ISL_ROW_SUPPORTED = 3, RM_ISL_ROW_SUM_A = 4,
                 RM_ISL_ROW_SUM_B = 5, RM_ISL_ROW_MIN_A = 6, RM_ISL_ROW_MAX_A = 7, RM_ISL_ROW_MIN_B = 8, RM_ISL_ROW_MAX_B = 9,
                 RM_ISL_ROW_BELOW_MIN = 10, RM_ISL_ROW_BELOW_MAX = 11, RM_ISL_ROW_WORDS = 12 };
int rm_islands_solid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                     uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                     uint32_t n_stats);
int rm_islands_occupancy(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* occupancy, int is_device, void* stream,
                         uint32_t up, uint32_t r2, uint32_t plate, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                         uint32_t n_stats);
int rm_read_islands(rm_ctx* ctx, uint32_t* out_rows, uint64_t row_capacity, uint32_t* out_labels, void* out_mask,
                    uint32_t* out_profile, int is_device, void* stream);

/* Surface measures (extension; DESIGN.md section 25 is the contract, to the last bit): what is the surface area, how large is
 * the interface between two materials, how much area do the supports touch the part with -- from the counts of the pairs of
 * neighbouring lattice points by the classes of their two ends.
 * Lattice, "inside", limits and linear index are rm_label_solid's (2..1024 points per axis, at most 2^28 in all, RM_ERR_RANGE
 * otherwise; i + nx * (j + ny * k)).  Every point has a CLASS 0..7 (RM_SURF_CLASSES).  rm_surface_solid: 1 inside, 0 outside.
 * rm_surface_classes: min(byte, 7) of the caller's bytes (one per point, x fastest; host memory, or (is_device) device memory
 * read after the work queued on `stream`) -- a total function, so no call fails after a launch for its input; the 0/1
 * occupancies and the masks of rm_read_support (0..4), rm_read_distance (0..3) and rm_read_islands (0..2) are valid as they are.
 * The lattice counts as surrounded by ONE LAYER OF CLASS-0 POINTS (every point with a coordinate of -1, or of n on that axis):
 * the PADDED lattice; a solid that touches the border still has a closed surface.
 * Thirteen DIRECTIONS nu, in this order (RM_SURF_DIRS; rm_surface_directions writes the 39 words): the axes (1,0,0) (0,1,0)
 * (0,0,1); the face diagonals (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1); the space diagonals (1,1,1) (1,1,-1) (1,-1,1)
 * (1,-1,-1).
 * out_counts, RM_SURF_COUNTS = 840 words:
 *   POINTS[a]        at RM_SURF_POINTS + a: the lattice points of class a (padding is not counted)
 *   PAIR[a][b][nu]   at RM_SURF_PAIR(a, b, nu) = 8 + (8 a + b) * 13 + nu: the pairs (p, p + nu), both in the padded lattice, with
 *                    class(p) = a and class(p + nu) = b.  PAIR[0][0][.] is written as 0 (it would only count padding).  The
 *                    ordered pair carries the orientation: PAIR[1][0][z] are up-facing faces, PAIR[0][1][z] down-facing ones.
 * out_stats[RM_SURF_STAT_*]: BRICKS, BRICKS_KEPT, BRICKS_INSIDE, EVALUATIONS as rm_mass_moments reports them for the same lattice
 * and level (0 for rm_surface_classes); SCRATCH_BYTES, the device memory the call used.
 * Every word is a count: two runs, and any correct implementation, give identical words.  The calls are synchronous on the
 * context's own stream, ordered after its earlier work; nothing is retained (there is no rm_read_*), and no earlier retained
 * result -- mesh, slices, labelling, distance volume, support or islands result -- is dropped or replaced.  Errors (every check
 * precedes the first launch, and a failed call leaves the outputs untouched) are those of rm_label_solid / rm_label_occupancy,
 * word for word, with RM_SURF_COUNTS and RM_SURF_STATS; RM_ERR_DEVICE when device memory runs out (about 1 byte per point).
 * rm_surface_measures (host code, binary64, no context) measures the interface between the class sets A and B, bit masks over
 * the classes (bit a = class a), from the counts and the lattice's step.  out[RM_SURF_*], RM_SURF_MEASURES doubles:
 *   FACET_POS_X .. FACET_NEG_Z   the exact staircase areas by orientation from A into B: POS_X = s_y s_z * sum over a in A, b in B
 *                                of PAIR[a][b][x], NEG_X the same of PAIR[b][a][x]; for any steps
 *   FACET_AREA                   the sum of the six
 *   AREA                         the Cauchy-Crofton estimate 2 dV sum over nu of w_nu N_nu / r_nu: N_nu = sum over a in A, b in B
 *                                of PAIR[a][b][nu] + PAIR[b][a][nu] (the crossings), dV = s_x s_y s_z, r_nu = |nu o step|, w_nu the
 *                                fraction of the sphere nearer to +-nu than to any other of the 26 directions (0.0915557824...,
 *                                0.0739612557..., 0.0703912795... for an axis, a face and a space diagonal).  Defined for three
 *                                equal steps only: NaN otherwise.  Balls converge (over six centres within 3.5 % of 4 pi R^2
 *                                at a radius of 6 points, 1.1 % at 10.3, 0.65 % at 14.7, 0.11 % at 20.2); an axis-aligned box
 *                                is the worst case (-12.6 % for a 10-point cube), for which FACET_AREA is exact.
 * RM_ERR_NULL for a NULL array; RM_ERR_ARG for n_counts < RM_SURF_COUNTS, n_out < RM_SURF_MEASURES, a mask that is empty or has
 * a bit above class 7, masks that overlap, and a step that is not finite or <= 0.  rm_surface_directions: RM_ERR_NULL,
 * RM_ERR_ARG for n_out < 3 * RM_SURF_DIRS. */
#define RM_SURF_PAIR(a, b, nu) (8 + (8 * (int)(a) + (int)(b)) * 13 + (int)(nu)) /* the index of PAIR[a][b][nu] in out_counts */
enum rm_surfcount { RM_SURF_CLASSES = 8, RM_SURF_DIRS = 13, RM_SURF_POINTS = 0, RM_SURF_PAIRS = 8, RM_SURF_COUNTS = 840 };
enum rm_surfstat { RM_SURF_STAT_BRICKS = 0, RM_SURF_STAT_BRICKS_KEPT = 1, RM_SURF_STAT_BRICKS_INSIDE = 2,
                   RM_SURF_STAT_EVALUATIONS = 3, RM_SURF_STAT_SCRATCH_BYTES = 4, RM_SURF_STATS = 5 };
enum rm_surfmeasure { RM_SURF_AREA = 0, RM_SURF_FACET_AREA = 1, RM_SURF_FACET_POS_X = 2, RM_SURF_FACET_NEG_X = 3,
                      RM_SURF_FACET_POS_Y = 4, RM_SURF_FACET_NEG_Y = 5, RM_SURF_FACET_POS_Z = 6, RM_SURF_FACET_NEG_Z = 7,
                      RM_SURF_MEASURES = 8 };
int rm_surface_solid(rm_ctx* ctx, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                     uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_surface_classes(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                       uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_surface_directions(int* out, uint32_t n_out);
int rm_surface_measures(const uint64_t* counts, uint32_t n_counts, const float* step, uint32_t mask_a, uint32_t mask_b,
                        double* out, uint32_t n_out);

/* Mesh voxelisation (extension; DESIGN.md section 27 is the contract, to the last bit): a triangle mesh into the occupancy of a
 * lattice -- the source of the rm_*_occupancy calls and of rm_surface_classes for parts that arrive as STL, OBJ or PLY files.
 * Needs no program: a context with an empty or invalid command buffer voxelises.
 * Mesh: xyz holds n_vertices x 3 floats, indices n_triangles x 3 vertex indices, or NULL for a SOUP (triangle t has the vertices
 * 3 t, 3 t + 1, 3 t + 2; n_vertices == 3 n_triangles).  Both in host memory, or (is_device) both in device memory, 4-byte aligned,
 * read after the work queued on `stream`.  No host pass looks at the data: device inputs are judged on the device.
 * Lattice: rm_label_solid's (2..1024 points per axis, at most 2^28 in all, RM_ERR_RANGE otherwise; linear index
 * i + nx * (j + ny * k)); origin and step as rm_sample_grid takes them, but the snapping below is an exact affine map in binary64,
 * not the o + (float)i * s of the lattice calls.
 * A coordinate v on axis a becomes q = rint(((double)v - (double)o_a) / (double)s_a * 64): index space with 6 fractional bits,
 * every operation rounded once, half to even; lattice point i sits at 64 i.  A triangle is REJECTED (counted, contributes
 * nothing) when an index is >= n_vertices, a coordinate is not finite, or some |q| > 2^17.  An accepted triangle whose projection
 * onto y-z has no area is EDGE_ON (counted, skipped).  Any other crosses the row (j, k) -- the ray along +x through (64 j, 64 k) --
 * iff its three edge functions admit the row: E > 0, or E == 0 and (dy > 0 or (dy == 0 and dz > 0)) for the directed edge (dy, dz)
 * of the triangle oriented counter-clockwise in y-z, so that a row through a shared edge or vertex counts as a generic row would.
 * The crossing at x (exact, a quotient of int64) toggles bit t = ceil(x / 64), clamped to [0, nx], of the row's nx + 1 bits;
 * occupancy(i, j, k) is the XOR of the bits 0..i: the even-odd rule, a point exactly on the surface inside where the row enters.
 * A row whose bit nx has an odd prefix -- an odd number of crossings in all -- is an OPEN ROW: the mesh is not closed along it.
 * out_counts[RM_VOX_*]: TRIANGLES (n_triangles), REJECTED, EDGE_ON, CROSSINGS (every admitted pair of a row and a triangle, the
 * clamped ones included), INSIDE (points of occupancy 1), OPEN_ROWS.  out_stats[RM_VOX_STAT_*]: BRICKS, BRICKS_KEPT,
 * BRICKS_INSIDE, EVALUATIONS are 0, as for a caller's occupancy; ITEMS, the work items of 64 rows the raster launch took;
 * SCRATCH_BYTES, the device memory the call used beside the occupancy.
 * Every word is an integer that no order of execution changes: two runs, any order of the triangles, any rotation or reversal
 * of a triangle's vertices, and any correct implementation give identical words.
 * The call is synchronous on the context's own stream, ordered after its earlier work.  The occupancy (one byte per point, 0 or
 * 1, x fastest -- what rm_label_occupancy, rm_distance_occupancy, rm_support_occupancy, rm_islands_occupancy and
 * rm_surface_classes take) stays in the context until the next rm_voxelize_mesh; rm_read_voxels copies it out (is_device and
 * stream as for rm_read_distance).  No other retained result is dropped or replaced, and no other call replaces this one.
 * Errors, every check before the first launch, outputs untouched and the previous voxel result still readable: RM_ERR_NULL for
 * a NULL ctx, xyz, out_counts or out_stats (and origin or step); RM_ERR_ARG for n_counts < RM_VOX_COUNTS, then n_stats <
 * RM_VOX_STATS, then an origin or a step that is not finite or a step <= 0; RM_ERR_RANGE for the lattice; RM_ERR_ARG for
 * n_triangles == 0, n_vertices == 0, a soup with n_vertices != 3 n_triangles and device arrays off 4-byte alignment.  After the
 * first launches: RM_ERR_TOO_LARGE for 2^31 work items or more (the previous result is still readable); RM_ERR_DEVICE when
 * device memory runs out.  rm_read_voxels: RM_ERR_ARG before any voxelisation. */
enum rm_voxcount { RM_VOX_TRIANGLES = 0, RM_VOX_REJECTED = 1, RM_VOX_EDGE_ON = 2, RM_VOX_CROSSINGS = 3, RM_VOX_INSIDE = 4,
                   RM_VOX_OPEN_ROWS = 5, RM_VOX_COUNTS = 6 };
enum rm_voxstat { RM_VOX_STAT_BRICKS = 0, RM_VOX_STAT_BRICKS_KEPT = 1, RM_VOX_STAT_BRICKS_INSIDE = 2,
                  RM_VOX_STAT_EVALUATIONS = 3, RM_VOX_STAT_ITEMS = 4, RM_VOX_STAT_SCRATCH_BYTES = 5, RM_VOX_STATS = 6 };
int rm_voxelize_mesh(rm_ctx* ctx, uint32_t n_vertices, const float* xyz, uint32_t n_triangles, const uint32_t* indices,
                     int is_device, void* stream, const float* origin, const float* step, uint32_t nx, uint32_t ny, uint32_t nz,
                     uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
int rm_read_voxels(rm_ctx* ctx, void* out_occupancy, int is_device, void* stream);

/* Lattice draw (extension; DESIGN.md section 28 is the contract, to the last bit): a lattice of class bytes -- an occupancy, a
 * mask, their sum -- as an image through the draws' camera, or along a caller's rays.  Needs no program.
 * rm_set_lattice copies the bytes (nx x ny x nz, x fastest, one byte per point; host memory, or (is_device) device memory read
 * after the work queued on `stream`) into a retained slot of the context and builds the traversal's bit words there.  Lattice:
 * rm_label_solid's (2..1024 points per axis, at most 2^28 in all, RM_ERR_RANGE otherwise); origin and step as rm_sample_grid
 * takes them.  Byte 0 is empty; a byte c > 0 is the cube [i - 1/2, i + 1/2]^3 of its point in index space, of albedo
 * table[min(c, count - 1)] of the material table (rm_set_materials) as it stands at the draw or cast.
 * out_counts[RM_LAT_*]: POINTS (bytes != 0), BRICKS (the bricks of 8 x 8 x 8 points that hold one).  out_stats[RM_LAT_STAT_*]:
 * the four brick statistics are 0, as for a caller's occupancy; RETAINED_BYTES, the device memory the slot keeps; SCRATCH_BYTES,
 * the scratch memory the call used (0: the bytes are copied into the slot).  The call is synchronous on the context's own
 * stream, ordered after its earlier work.  The lattice stays until the next rm_set_lattice; no other retained result is dropped
 * or replaced, and no other call replaces this one.
 * Errors, every check before the first launch, outputs untouched and the previous lattice still drawable: RM_ERR_NULL for a NULL
 * ctx, classes, out_counts or out_stats (and origin or step); RM_ERR_ARG for n_counts < RM_LAT_COUNTS, then n_stats <
 * RM_LAT_STATS, then an origin or a step that is not finite or a step <= 0; RM_ERR_RANGE for the lattice.  RM_ERR_DEVICE when
 * device memory runs out (no lattice is retained then).
 *
 * rm_cast_lattice: n rays (n x 6 floats: origin, direction, used as given) through the retained lattice.  window: six u32
 * (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), host memory, lo_a < hi_a <= n_a, points outside it are empty and the ray is clipped to
 * its box; NULL: the whole lattice.  out_hit (n x 8 floats: t, position, normal, diffuse) and out_rgb (n x 3) as rm_cast_rays
 * gives them -- a miss is exactly rm_cast_rays' miss: the floor, or nothing --; out_ids (n x 4 u32): kind (RM_HIT_*), linear
 * point index i + nx (j + ny k), class byte, face (2 axis + (normal positive ? 1 : 0), or RM_LAT_FACE_NONE for an origin inside a
 * cube), RM_NO_ID unless a surface was hit.  There is no step limit and the march limits are not used: a ray takes at most
 * nx + ny + nz events.  NULL outputs, alignment, n == 0, is_device and stream as for rm_cast_rays.
 * rm_draw_lattice: the image of the retained lattice through the uniforms' camera -- per pixel the sixteen AA sample rays
 * of rm_draw, each cast as above, resolved as rm_draw resolves them, written in RM_OPT_OUTPUT_FORMAT.  Rows, destination,
 * stream (RM_STREAM_OWN included) and ordering as for rm_draw; like a query it leaves the draw state alone.
 * Errors of both: RM_ERR_NULL for NULL outputs; RM_ERR_ARG before any rm_set_lattice, for a bad window and for device arrays off
 * their alignment; rm_draw_lattice: RM_ERR_RANGE for an image or a row band outside rm_draw's ranges. */
enum rm_latcount { RM_LAT_POINTS = 0, RM_LAT_BRICKS = 1, RM_LAT_COUNTS = 2 };
enum rm_latstat { RM_LAT_STAT_BRICKS = 0, RM_LAT_STAT_BRICKS_KEPT = 1, RM_LAT_STAT_BRICKS_INSIDE = 2, RM_LAT_STAT_EVALUATIONS = 3,
                  RM_LAT_STAT_RETAINED_BYTES = 4, RM_LAT_STAT_SCRATCH_BYTES = 5, RM_LAT_STATS = 6 };
#define RM_LAT_FACE_NONE 6u
int rm_set_lattice(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                   const float* origin, const float* step, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats,
                   uint32_t n_stats);
int rm_draw_lattice(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* window, void* out_rgba,
                    int out_is_device, void* stream);
int rm_cast_lattice(rm_ctx* ctx, uint32_t n, const float* rays, const uint32_t* window, float* out_hit, uint32_t* out_ids,
                    float* out_rgb, int is_device, void* stream);

/* Lattice meshing (extension; DESIGN.md section 29 is the contract, to the last bit): the interface between two class sets of a
 * lattice of class bytes as a welded, indexed, consistently wound triangle mesh -- the unit faces that rm_surface_classes counts
 * as PAIR[a][b][x|y|z] and rm_surface_measures measures as FACET_AREA, in a fixed order.  Needs no program.
 * Lattice, bytes, is_device and stream as rm_surface_classes takes them (class = min(byte, 7), one layer of class-0 points
 * around the lattice); origin and step as rm_set_lattice takes them; mask_a and mask_b as rm_surface_measures takes them
 * (non-empty, disjoint, no bit above 7).
 * Faces: a pair (p, p + e_a) of points of the padded lattice, a = x, y, z, is a face with normal +a when class(p) is in A and
 * class(p + e_a) in B, with normal -a when the other way round.  Corners: (nx + 1)(ny + 1)(nz + 1), corner (ci, cj, ck) at index
 * position (ci - 1/2, cj - 1/2, ck - 1/2), L = ci + (nx + 1)(cj + (ny + 1) ck); the face's lowest corner is p + e_a, its key
 * 3 L + a.  Faces are ordered by key; vertices are the corners that a face touches, each once, ordered by L, at
 * o + ((float)c - 0.5f) * s per axis (product and sum rounded once each, no fma).  Face f gives the triangles 2 f and 2 f + 1:
 * with (u, v) the other two axes in cyclic order and q00, q10, q11, q01 the corners by their offsets in (u, v), (q00, q10, q11)
 * and (q00, q11, q01) for a normal +a, (q00, q11, q10) and (q00, q01, q11) for -a: counter-clockwise seen from the B side.
 * rm_read_class_mesh: out_vertices V x 3 floats, out_triangles T x 3 u32, out_ids T x 2 u32 -- word 0 is class_A | class_B << 8 |
 * face << 16 (face = 2 axis + (normal positive ? 1 : 0), as rm_cast_lattice numbers faces), word 1 the linear index
 * i + nx (j + ny k) of the face's A-side point, RM_NO_ID when that point is padding (only when class 0 is in A).  Any output may
 * be NULL; device arrays need 4-byte alignment; an empty mesh is valid; the next producing call waits for a device read that is
 * still running.
 * out_counts[RM_CMESH_*]: VERTICES, TRIANGLES, FACES; FACES_POS_X .. FACES_NEG_Z; EDGES (corner-lattice edges with at least one
 * face), OPEN_EDGES (with 1 or 3 faces: 0 whenever A and B together hold every class present), BRANCH_EDGES (with 3 or 4 faces:
 * two voxels meet diagonally; the mesh is closed there but not 2-manifold).  V, T < 2^32: the lattice has at most 4.5 x 2^28
 * faces.  out_stats[RM_CMESH_STAT_*]: the four brick statistics are 0, as for a caller's occupancy; RETAINED_BYTES, the device
 * memory the mesh takes; SCRATCH_BYTES.  The call is synchronous on the context's own stream.  The mesh stays until the next
 * rm_mesh_classes; no other retained result is dropped or replaced, and no other call replaces this one.
 * Errors, every check before the first launch, outputs untouched and the previous class mesh still readable: rm_set_lattice's,
 * in its order, with RM_CMESH_COUNTS and RM_CMESH_STATS; then RM_ERR_ARG for a bad mask.  RM_ERR_DEVICE when device memory runs
 * out (no mesh is retained then).  rm_read_class_mesh: RM_ERR_ARG before any rm_mesh_classes. */
enum rm_cmeshcount { RM_CMESH_VERTICES = 0, RM_CMESH_TRIANGLES = 1, RM_CMESH_FACES = 2, RM_CMESH_FACES_POS_X = 3, RM_CMESH_FACES_NEG_X = 4,
                     RM_CMESH_FACES_POS_Y = 5, RM_CMESH_FACES_NEG_Y = 6, RM_CMESH_FACES_POS_Z = 7, RM_CMESH_FACES_NEG_Z = 8,
                     RM_CMESH_EDGES = 9, RM_CMESH_OPEN_EDGES = 10, RM_CMESH_BRANCH_EDGES = 11, RM_CMESH_COUNTS = 12 };
enum rm_cmeshstat { RM_CMESH_STAT_BRICKS = 0, RM_CMESH_STAT_BRICKS_KEPT = 1, RM_CMESH_STAT_BRICKS_INSIDE = 2, RM_CMESH_STAT_EVALUATIONS = 3,
                    RM_CMESH_STAT_RETAINED_BYTES = 4, RM_CMESH_STAT_SCRATCH_BYTES = 5, RM_CMESH_STATS = 6 };
int rm_mesh_classes(rm_ctx* ctx, uint32_t nx, uint32_t ny, uint32_t nz, const void* classes, int is_device, void* stream,
                    const float* origin, const float* step, uint32_t mask_a, uint32_t mask_b, uint64_t* out_counts, uint32_t n_counts,
                    uint64_t* out_stats, uint32_t n_stats);
int rm_read_class_mesh(rm_ctx* ctx, float* out_vertices, uint32_t* out_triangles, uint32_t* out_ids, int is_device, void* stream);

/* Slicing (extension; DESIGN.md section 16 is the contract, to the last bit): the closed outlines of the solid d < level in a
 * stack of planes, as ordered polylines -- what a slicer or a section drawing needs, evaluated directly on a 2-D lattice
 * per layer instead of through a triangle mesh.  From the program, limits and material table as they are at the call.
 * Lattice: the slicing axis w = axis (0, 1 or 2), the in-plane axes u = (w + 1) % 3 and v = (w + 2) % 3 ((u, v, w) is
 * right-handed; for y up pass axis = 1: u = z, v = x).  origin_uv and step_uv are host arrays of 2 floats (finite; step
 * > 0), heights a host array of n_layers finite floats in any order, duplicates allowed.  Point (i, j) of layer k is
 * (ou + (float)i * su, ov + (float)j * sv) on (u, v) and heights[k] on w; its value is rm_query_points' distance there.
 * Inside: d < level (NaN is outside).  One vertex on each in-plane lattice edge whose ends differ, by rm_extract_mesh's rule,
 * ordered by (layer, i + nu * j, axis).  Per cell the directed segments of the case table (rm_slice_case_table), the inside
 * on their left seen from +w; they chain into contours: an open one (it starts and ends on the lattice's border) begins at
 * the vertex no segment ends at, a closed one at its lowest vertex and does not repeat it.  Contours are ordered by layer
 * (in the order of `heights`) and then by their first vertex.  So outer boundaries are counter-clockwise seen from +w and
 * holes clockwise.  Results (rm_read_slices): points P x 3 floats (world x, y, z, in contour order), contours C x 4 u32
 * (first point, point count, layer, closed 0/1), layer_first n_layers + 1 u32 (the contour each layer starts at; the last
 * entry is C), and with RM_MESH_NORMALS / RM_MESH_IDS in flags normals P x 3 and ids P x 2 (leaf, material), exactly what
 * rm_query_points returns at the points.  Two runs give identical arrays; one call over all layers gives the concatenation
 * of one call per layer (indices shifted).
 * nu and nv: 2..65536 with nu * nv <= 2^26; n_layers: 1..65536; RM_ERR_RANGE otherwise, or when P or C would not fit 32
 * bits.  RM_ERR_ARG for an axis above 2, a value that is not finite, a step <= 0, unknown flags, n_counts < RM_SLICE_COUNTS.
 * Otherwise the errors of rm_extract_mesh.  out_counts[RM_SLICE_POINTS] = P, [RM_SLICE_CONTOURS] = C.
 * Synchronous on the context's own stream, ordered after its earlier work.  The result lives in buffers of its own until the
 * next rm_slice_contours or rm_destroy: it does not replace the context's mesh, and like a query the call never touches
 * the draw state (RM_OPT_TIMING, RM_INFO_*, the specialised kernel, the tile buffers). */
enum rm_slicecount { RM_SLICE_POINTS = 0, RM_SLICE_CONTOURS = 1, RM_SLICE_COUNTS = 2 };
int rm_slice_contours(rm_ctx* ctx, uint32_t axis, const float* origin_uv, const float* step_uv, uint32_t nu, uint32_t nv,
                      const float* heights, uint32_t n_layers, float level, uint32_t flags, uint64_t* out_counts,
                      uint32_t n_counts);
/* Copies the last slices out; any output may be NULL.  RM_ERR_ARG before any rm_slice_contours, or for normals / ids that
 * call did not compute.  is_device and stream as for rm_query_points (device arrays: out_contours 16-byte aligned, out_ids
 * 8-byte, the others 4-byte); the next rm_slice_contours waits for a device read that is still running. */
int rm_read_slices(rm_ctx* ctx, float* out_points, uint32_t* out_contours, uint32_t* out_layer_first, float* out_normals,
                   uint32_t* out_ids, int is_device, void* stream);
/* The case table of rm_slice_contours (host code; no context): 16 cases x 5 words.  out[5 * case] = segment count (0..2),
 * then (tail edge, head edge) pairs ordered by tail edge, 0xFFFFFFFF after the last.  Case = sum over corners c of
 * inside(c) << c, corner c at (c & 1, c >> 1) in (u, v); edge e runs along in-plane axis e >> 1 from the corner with 0 on
 * it, e & 1 its offset on the other axis: 0 bottom, 1 top, 2 left, 3 right.  The diagonal cases 6 and 9 give one segment
 * around each inside corner.  RM_ERR_ARG when n_out < 80. */
int rm_slice_case_table(uint32_t* out, uint32_t n_out);

/* Mesh slicing (extension; DESIGN.md section 30 is the contract): the outlines of an INDEXED triangle mesh in a stack of planes,
 * as the ordered polylines of rm_slice_contours, retained in the same slot and read with rm_read_slices (points, contours,
 * layer_first; asking for normals or ids is RM_ERR_ARG).  Needs no scene.  xyz: n_vertices x 3 floats, triangles: n_triangles x
 * 3 u32 (required); host arrays, or with is_device != 0 device arrays (4-byte aligned), read after the work queued on `stream`
 * (RM_STREAM_OWN: the context's own).  origin and step (host, 3 floats, finite, step > 0) are a resolution frame, not a lattice:
 * a vertex is snapped exactly as rm_voxelize_mesh snaps it, q = rint(((double)v - o) / s * 64) per axis, valid iff finite and
 * |q| <= 2^17.  axis = w (0, 1, 2), u = (w + 1) % 3, v = (w + 2) % 3.  heights: a HOST array of n_layers finite floats;
 * r_k = ((double)h_k - o_w) / s_w * 64 and the plane sits at P2_k = 2 floor(r_k) + 1 in units of 1 / 128 of a step: at most
 * 1 / 128 of a step from the height asked for, and never through a vertex.  P2 must be strictly increasing.
 * A triangle with an index >= n_vertices, two equal indices or an invalid corner is REJECTED: counted, and contributes nothing.
 * Half-edge h = 3 t + s runs from triangles[3 t + s] to triangles[3 t + (s + 1) % 3].  The half-edges of accepted triangles are
 * grouped by their unordered index pair: two of opposite direction are a PAIRED edge (canonical half-edge: the lower h), one is
 * a BORDER edge, anything else a BRANCH edge; every half-edge of a border or branch group is its own canonical half-edge.  A
 * canonical half-edge carries one vertex for each plane strictly between its ends; vertices are ordered by (plane, canonical
 * half-edge).  A plane that meets an accepted triangle crosses two of its half-edges; the segment runs from the vertex of the one
 * going down the axis to the vertex of the one going up, so that for triangles wound counter-clockwise seen from outside the
 * inside is on the left seen from +w: outer boundaries counter-clockwise, holes clockwise.  Segments chain into contours exactly
 * as rm_slice_contours': a closed one starts at its lowest vertex, an open one at the vertex no segment ends at; ordered by
 * layer, then first vertex.  The point of the edge A -> B (A_w < B_w, snapped) in plane P2: on a = u, v
 * g_a = (double)A_a + (double)((B_a - A_a) (P2 - 2 A_w)) / (double)(2 (B_w - A_w)), on w g_w = (double)P2 / 2; the world
 * coordinate is (float)((double)o_a + g_a / 64 * (double)s_a); no fma.  All outputs are identical from run to run; permuting the
 * triangles or rotating a triangle's corners changes only where loops start and their order within a layer.
 * out_counts (enum rm_mslicecount, n_counts >= RM_MSLICE_COUNTS), out_stats (enum rm_mslicestat, n_stats >= RM_MSLICE_STATS).
 * Refusals, in this order: RM_ERR_NULL for a NULL array; RM_ERR_ARG for n_counts or n_stats too small, flags != 0, axis > 2, an
 * origin or step that is not finite or a step <= 0, n_vertices = 0; RM_ERR_RANGE for n_layers outside 1..65536 or n_triangles
 * outside 1..2^28; RM_ERR_ARG for a height that is not finite; RM_ERR_RANGE for |r_k| > 2^18; RM_ERR_ARG when P2 is not strictly
 * increasing or a device array is misaligned; RM_ERR_RANGE when POINTS does not fit 32 bits; RM_ERR_DEVICE when device memory runs
 * out.  Every one of them leaves the previous slices readable.  Synchronous; touches no other family's result and no draw state. */
enum rm_mslicecount { RM_MSLICE_TRIANGLES = 0, RM_MSLICE_REJECTED = 1, RM_MSLICE_PAIRED_EDGES = 2, RM_MSLICE_BORDER_EDGES = 3,
                      RM_MSLICE_BRANCH_EDGES = 4, RM_MSLICE_SEGMENTS = 5, RM_MSLICE_POINTS = 6, RM_MSLICE_CONTOURS = 7,
                      RM_MSLICE_OPEN_CONTOURS = 8, RM_MSLICE_COUNTS = 9 };
enum rm_mslicestat { RM_MSLICE_STAT_SORT_PASSES = 0, RM_MSLICE_STAT_RANK_ROUNDS = 1, RM_MSLICE_STAT_SCRATCH_BYTES = 2, RM_MSLICE_STATS = 3 };
int rm_slice_mesh(rm_ctx* ctx, const float* xyz, uint32_t n_vertices, const uint32_t* triangles, uint32_t n_triangles, int is_device,
                  void* stream, const float* origin, const float* step, uint32_t axis, const float* heights, uint32_t n_layers,
                  uint32_t flags, uint64_t* out_counts, uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);

/* Hatching (extension; DESIGN.md section 31 is the contract, to the last bit): the retained slices -- of rm_slice_contours or of
 * rm_slice_mesh -- filled layer by layer with parallel lines under the even-odd rule: infill, scan vectors, section hatching.  The
 * slices are read on the device and never changed.  lines: a HOST array of n_layers x 4 floats (dx, dy, offset, spacing) per
 * layer, n_layers the slices' own layer count; n_lines lines per layer (1..2^24, n_layers * n_lines <= 2^32).
 * Frame: w the slices' axis, u = (w + 1) % 3, v = (w + 2) % 3.  The normal coordinate of a point is
 * s(P) = (double)P_v (double)dx - (double)P_u (double)dy (exact products, one rounded difference; the direction need not be a unit
 * vector: offset and spacing are in units of s).  Line j of a layer lies at c_j = (double)offset + (double)j (double)spacing.
 * Point i of a contour with first point f and n points is the tail of the segment to f + (i - f + 1) % n -- the last point of an
 * open contour of none --, and the segment's id is i.  With A its end of the smaller s and B the other, the segment CROSSES line
 * j iff sA <= c_j < sB; sA == sB or a value that is not finite crosses nothing.  The crossing's point, in binary64 without fma:
 * t = (c_j - sA) / (sB - sA), X_a = (float)((double)A_a + t ((double)B_a - (double)A_a)) on a = u, v; its place along the line
 * r = (float)((double)X_u (double)dx + (double)X_v (double)dy), as key32 = bits(r) ^ (sign ? 0xFFFFFFFF : 0x80000000).  Crossings
 * are enumerated by (segment id, j) and sorted stably by L * 2^32 + key32, L = layer * n_lines + j: equal keys keep the enumeration's
 * order.  On each line the crossings of ranks 2 i and 2 i + 1 are one hatch segment; a line with an odd number -- open contours
 * alone cause one -- drops its last and counts in ODD_LINES; zero-length segments are kept.  Segments are ordered by L, then rank;
 * with RM_HATCH_ZIGZAG the segments of a line with odd j come in reverse order with their ends swapped.
 * Results (rm_read_hatch): segments H x 4 floats (u, v of the first end, u, v of the second), line H u32 (L), layer_first
 * n_layers + 1 u32 (the segment each layer starts at; the last entry is H).  Identical from run to run.
 * out_counts (enum rm_hatchcount, n_counts >= RM_HATCH_COUNTS): SEGMENTS_IN the contour segments looked at, CROSSINGS, SEGMENTS = H,
 * LINES_HIT the lines with a crossing, ODD_LINES.  out_stats (enum rm_hatchstat, n_stats >= RM_HATCH_STATS).
 * Refusals, in this order: RM_ERR_NULL for lines, out_counts or out_stats NULL; RM_ERR_ARG for n_counts or n_stats too small,
 * unknown flags, no valid slices, n_layers other than the slices', a value of lines that is not finite, spacing <= 0,
 * dx = dy = 0; RM_ERR_RANGE for n_lines outside 1..2^24, n_layers * n_lines > 2^32, 2^32 crossings or more; RM_ERR_DEVICE when
 * device memory runs out.  Every one of them leaves the previous hatch and the slices readable.  The hatch lives in buffers of its
 * own until the next rm_hatch_slices, rm_destroy, or any call that replaces the slices (rm_slice_contours, rm_slice_mesh): from
 * there on rm_read_hatch is RM_ERR_ARG until the next hatch.  Synchronous; touches no other family's result and no draw state. */
enum rm_hatchflag { RM_HATCH_ZIGZAG = 1 };
enum rm_hatchcount { RM_HATCH_SEGMENTS_IN = 0, RM_HATCH_CROSSINGS = 1, RM_HATCH_SEGMENTS = 2, RM_HATCH_LINES_HIT = 3, RM_HATCH_ODD_LINES = 4,
                     RM_HATCH_COUNTS = 5 };
enum rm_hatchstat { RM_HATCH_STAT_SORT_PASSES = 0, RM_HATCH_STAT_SCRATCH_BYTES = 1, RM_HATCH_STATS = 2 };
int rm_hatch_slices(rm_ctx* ctx, const float* lines, uint32_t n_layers, uint32_t n_lines, uint32_t flags, uint64_t* out_counts,
                    uint32_t n_counts, uint64_t* out_stats, uint32_t n_stats);
/* Copies the last hatch out; any output may be NULL.  RM_ERR_ARG without a valid hatch.  is_device and stream as for
 * rm_read_slices (device arrays: out_segments 16-byte aligned, the others 4-byte). */
int rm_read_hatch(rm_ctx* ctx, float* out_segments, uint32_t* out_line, uint32_t* out_layer_first, int is_device, void* stream);

/* Lit rendering (extension): rm_draw with soft shadows and ambient occlusion marched through the same distance field
 * (DESIGN.md section 13 is the contract, to the last bit).  The reference has one fixed light and max(0.02, n.l)
 * (wgsl:98-105); with RM_LIGHT_SHADOW = 0 and RM_LIGHT_AO = 0 rm_draw_lit writes rm_draw's image bit for bit.
 * The light keeps the reference's convention: l = normalize(pos - P) is the vector whose dot product with the normal lights
 * a surface, and shadow rays travel along +l.  The floor (wgsl:117-127) receives shadow and occlusion but is not part of
 * map_scene, so it casts neither. */
enum rm_light {
    RM_LIGHT_POS_X = 0, RM_LIGHT_POS_Y = 1, RM_LIGHT_POS_Z = 2, /* P: default (2, -5, 3), wgsl:100; finite */
    RM_LIGHT_SHADOW = 3,          /* S, strength of the shadow term: default 1; [0, 1] */
    RM_LIGHT_SHADOW_SOFTNESS = 4, /* k, penumbra = min over the march of k h / t: default 8; > 0 */
    RM_LIGHT_BIAS = 5,            /* b, shadow rays start at pos + n b: default 0.02; >= 0 */
    RM_LIGHT_SHADOW_MAX_T = 6,    /* a shadow ray that travelled further is lit: default 20; > 0 */
    RM_LIGHT_SHADOW_STEPS = 7,    /* map_scene evaluations a shadow ray may take: default 64; integral, 1..1024 */
    RM_LIGHT_AO = 8,              /* A, strength of the occlusion term: default 1; [0, 1] */
    RM_LIGHT_AO_STEP = 9,         /* tap i = 1.. lies at pos + n (step i): default 0.1; > 0 */
    RM_LIGHT_AO_FALLOFF = 10,     /* weight of tap i + 1 over tap i: default 0.75; (0, 1] */
    RM_LIGHT_AO_SCALE = 11,       /* ao = clamp(1 - scale * sum, 0, 1): default 1.5; >= 0 */
    RM_LIGHT_AO_TAPS = 12,        /* default 5; integral, 1..16 */
    RM_LIGHT_PARAMS = 13
};
/* The table above (host code; no context).  RM_ERR_NULL for a NULL out, RM_ERR_ARG when n_out < RM_LIGHT_PARAMS. */
int rm_lighting_defaults(float* out, uint32_t n_out);
/* All RM_LIGHT_PARAMS values at once (a new context holds the defaults); count must be RM_LIGHT_PARAMS (RM_ERR_ARG).
 * RM_ERR_RANGE for a value outside the table (every value must be finite); a failed call changes nothing.  The
 * parameters travel with each lit draw as kernel arguments, like limits and uniforms. */
int rm_set_lighting(rm_ctx* ctx, const float* params, uint32_t count);
/* rm_draw in every respect but the shading: rows, output (RM_OPT_OUTPUT_FORMAT), host / device destination, stream
 * (RM_STREAM_OWN included) and ordering with the context's other work.  Errors are those of a scene query (program
 * status, RM_ERR_RANGE for max_iter > 65536, RM_ERR_MATERIAL); like a query it never touches the draw state
 * (RM_OPT_TIMING, RM_INFO_*, the specialised kernel, the tile buffers). */
int rm_draw_lit(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, float* out_rgba, int out_is_device,
                void* stream);

/* G-buffer draw (extension; DESIGN.md section 14 is the contract, to the last bit): the per-pixel geometry behind a frame.
 * The record of sample s of a pixel is exactly what rm_cast_rays returns for the ray rm_camera_rays(sample = s) gives for
 * that pixel; rm_draw_gbuffer generates the rays, marches them and reduces them per pixel in one kernel.
 * sample: 0..15 (that AA sample), RM_SAMPLE_CENTER, or RM_SAMPLE_ALL (the sixteen AA samples); a sample's bit in the masks is
 * its id (16 for the centre).  Each pixel of rows [row0, row0 + rows), row-major, receives
 *   out_masks: 4 x u32 -- [0] samples with kind RM_HIT_SURFACE, [1] samples with kind RM_HIT_FLOOR, [2] surface samples whose
 *              leaf lies in [sel_first, sel_first + sel_count), [3] the sum of the samples' steps (<= 2^20);
 *   out_ids:   4 x u32 -- (kind, sample id, leaf, material) of the nearest sample: the one that minimises (t, sample id)
 *              among the samples that hit a surface or the floor; (RM_HIT_NONE, RM_NO_ID, RM_NO_ID, RM_NO_ID) when none did;
 *              on the floor leaf and material are RM_NO_ID;
 *   out_geom:  8 x f32 -- that sample's hit record (t, x, y, z, nx, ny, nz, diffuse) as rm_cast_rays defines it; the miss
 *              record (+inf and zeros) when no sample hit.
 * Any output may be NULL (that work is skipped; what the others receive does not change); RM_ERR_NULL when all are.
 * W * rows = 0 writes nothing.  is_device and stream as for rm_query_points (RM_STREAM_OWN included); device arrays need
 * 16-byte alignment (RM_ERR_ARG).  Errors: the program's status, RM_ERR_RANGE for max_iter > 65536 or a row band outside the
 * frame, RM_ERR_ARG for another `sample` or a selection that reaches past cmd_count.  sel_count = 0 selects nothing.
 * RM_OPT_OUTPUT_FORMAT does not apply; like a query the call never touches the draw state (RM_OPT_TIMING, RM_INFO_*, the
 * specialised kernel, the tile buffers). */
int rm_draw_gbuffer(rm_ctx* ctx, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t sample,
                    uint32_t sel_first, uint32_t sel_count, float* out_geom, uint32_t* out_ids,
                    uint32_t* out_masks, int is_device, void* stream);
/* The selection of a graph node (pure host code, usable without a GPU): the contiguous range of command indices that
 * produce the value command `cmd_index` leaves on the stack -- a primitive: itself; a binary operator: from the first
 * command of its left operand through itself; a Material tag: from the first command of its child through itself; a
 * transform Pop: its Push through itself; a transform Push: the range of its Pop.  The root gives [0, cmd_count).
 * Errors: rm_validate_program's status for an invalid program, RM_ERR_RANGE for cmd_index >= cmd_count. */
int rm_program_subtree(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, uint32_t cmd_index,
                       uint32_t* out_first, uint32_t* out_count);

/* Waits for all work on the context's GPU (hipDeviceSynchronize). */
int rm_sync(rm_ctx* ctx);
/* HIP graphs: after its first draw of a given size and program (which allocates scratch buffers and compiles /
 * loads the scene's kernel), a device-destination rm_draw issues nothing but kernel launches on `stream` -- no
 * allocation, copy, event or synchronisation (RM_OPT_TIMING off) -- and can be stream-captured and replayed
 * (tests: test_draw_is_stream_capturable).  The uniforms travel as kernel arguments, i.e. are baked into the graph. */
/* Frames in flight without creating HIP streams in the host language: pass RM_STREAM_OWN as `stream` of a
 * device-destination draw and the launches go to the context's own stream; rm_sync_context waits for that stream
 * only.  A host that alternates two or three contexts this way (frame f -> context f % F, each with its own output
 * buffer) overlaps the tail of one frame with the start of the next: +15-20 % frames per second. */
#define RM_STREAM_OWN ((void*)(intptr_t)-1)
int rm_sync_context(rm_ctx* ctx);

int rm_set_option(rm_ctx* ctx, int key, int64_t value);
int rm_get_info(rm_ctx* ctx, int key, double* out);

/* Stream-write calibration: a fill kernel writes `bytes` of device memory `iters` times
 * with 16 B/lane stores; reports the achieved GB/s (the measured HBM-write ceiling). */
int rm_measure_write_bandwidth(rm_ctx* ctx, uint64_t bytes, int iters, double* out_gbps);

/* Self-tests of the arithmetic building blocks (used by tests/test_gpu_arithmetic.py).
 * rm_selftest_sqrt: runs the kernels' short correctly-rounded sqrt (v_rsq_f32 + one FMA-form Newton step, with its range
 * guard) against the generic one on EVERY non-negative binary32 bit pattern: wherever the guard lets the short form
 * through, the result must be the correctly rounded root, and the guard must not reject anything in [2^-96, FLT_MAX];
 * *out_mismatches must come back 0.
 * rm_selftest_ops: out[k*n + i], k = 0..7: min(a,b), max(a,b), v_min_f32(a,b), v_max_f32(a,-b), short sqrt(a),
 * generic sqrt(a), a / b, (float) i32(round(a)) -- compared on the host with the oracle's definitions. */
int rm_selftest_sqrt(rm_ctx* ctx, uint64_t* out_mismatches, uint32_t* out_first_bad_bits);
int rm_selftest_ops(rm_ctx* ctx, const float* a, const float* b, float* out, uint32_t n);
/* rm_selftest_div: the kernels' short division by one denominator (v_rcp_f32 refined by two FMA; per numerator a multiply, two
 * FMA and a sign transfer; a range guard in front) against the generic one.  (a) On EVERY b with the sign bit clear: where the
 * guard accepts b, the refined reciprocal equals 1.0f / b bit for bit.  (b) On the caller's pairs (a[i], b[i]), i < n (host
 * arrays; may be NULL with n = 0), and on n_seeded pairs generated on the device from `seed`: where the guard accepts the pair
 * the short quotient equals a / b bit for bit, signed zeros included.  out[8]: 0 reciprocal mismatches, 1 the lowest
 * mismatching b (bit pattern; all ones: none), 2 the b in [2^-48, 2^44] the guard rejects, 3 those of them whose significand
 * is not one of the top four, 4 quotient mismatches, 5 the lowest mismatching pair (bits of a << 32 | bits of b; all ones:
 * none), 6 the caller's pairs the guard sent to the generic form, 7 the seeded ones.  0, 3 and 4 must come back 0. */
int rm_selftest_div(rm_ctx* ctx, const float* a, const float* b, uint32_t n, uint32_t seed, uint32_t n_seeded, uint64_t* out);
/* rm_selftest_normalise: the normalisations of the march kernels as those kernels call them -- the device functions themselves,
 * not restatements -- on records the caller chooses.  in[8 n] (host array): one record of 8 floats per lane, 64 consecutive
 * records per wave, so the caller decides which lanes share a wave's fall-back to the generic form; n a multiple of 64, at most
 * 2^24 (RM_ERR_ARG otherwise).  mode 0: (x, y, z) = in[8 i + 0..2], divided by the root of (x x + y y) + z z (normalize3);
 * mode 1: (dx, dy, dz, ew) = in[8 i + 0..3], the ray form: (dx, dy, dz) divided by the root of ((dx dx + dy dy) + dz dz) + ew ew;
 * mode 2: the tap sum n = in[8 i + 0..2] and the hit position pos = in[8 i + 4..6] through shade_hit:
 * max(0.02, normalize(n) . normalize(pos - (2, -5, 3))).  Unused fields are ignored.
 * out[8 n] (host array, 32-bit words; floats as their bit patterns): out[8 i + 0..2] the result of the short form as the
 * kernels run it (whole-wave fall-back included; mode 2: word 0 alone, 1..2 zero), 3..5 the same call in its generic form
 * (mode 2: word 3 alone), 6 the range guard's verdict for lane i alone (1: outside the short form's range; mode 2: bit 0 the
 * normal, bit 1 the light vector), 7 zero.  tests/test_gpu_normalise_direct.py compares all of it with numpy. */
int rm_selftest_normalise(rm_ctx* ctx, const float* in, uint32_t n, int mode, uint32_t* out);
/* The two cross-lane primitives of wave-level culling (DPP row operations), one wave per 64 inputs (non-negative floats, +inf,
 * NaN): out[i] = the largest value of input i's wave (by bit pattern: a NaN wins), out[64 n_waves + i] = the minimum over the
 * inputs of the LOWER lanes of its wave (+inf for lane 0; a NaN is skipped).  tests/test_gpu_arithmetic.py compares with numpy. */
int rm_selftest_wave(rm_ctx* ctx, const float* in, uint32_t n_waves, float* out);
/* The device sort (csrc/rm_sort.h) on the caller's pairs: host arrays keys[n] (u64) and values[n] (u32), n >= 1, bits in 1..64.
 * out_keys / out_values: the pairs ordered by the low `bits` bits of their keys, equal ones in input order (stable); key bits above
 * `bits` travel with their pair and are not compared.  RM_ERR_ARG for n = 0 or bits outside 1..64.  tests/test_gpu_sort.py compares
 * with numpy's stable argsort. */
int rm_selftest_sort(rm_ctx* ctx, const uint64_t* keys, const uint32_t* values, uint32_t n, uint32_t bits, uint64_t* out_keys,
                     uint32_t* out_values);
/* The culling decisions of the march on inputs the caller chooses (tests/test_gpu_cull_bounds.py compares them with binary64
 * geometry): the device functions of a draw, on the context's current program, limits and options, with the launch a draw would
 * fill and the tables staged as the kernels stage them.  Host arrays only; they wait for the result.
 * rm_selftest_cull_rays: half-lines from origin[3] along dirs[3 n] (any length).  out_flags[i]: bit 0 the miss-test tables clear
 *   the ray, bit 1 the tables were usable (culling on, nothing vetoed), bit 2 the miss test on lower bounds applies to the
 *   program, bit 3 it clears the ray, bits 8.. the veto word of the tables; out_bound[i]: the lower bound that test computes
 *   (NaN when it does not apply).
 * rm_selftest_cull_pixels: pixels xy[2 n] of a W x H frame under the context's uniforms, as the pre-pass sees them.  out[8 i + ..]:
 *   0..2 the centre direction and 3 the radius rho of the cone of the pixel's sixteen sample directions (NaN: no usable cone),
 *   4 the lower bound over the cone (NaN when that test does not apply), 5 flags as the bits of an integer (bit 0 the tables
 *   clear the pixel, bit 1 the tables were usable, bit 2 the test on lower bounds applies, bit 3 it clears the pixel), 6..7 zero.
 * rm_selftest_cull_tiles: 8 x 8 tiles xy[2 n] = (tile_x, tile_y) of a W x H frame under the context's uniforms, as the pre-pass
 *   classifies a whole tile from the rectangle of its 32 x 32 sample positions.  out[8 i + ..]: 0..2 the centre direction and 3 the
 *   radius rho of the cone of those directions (NaN: no usable cone), 4 the checker bit of a one-cell tile (else 0), 5 flags as
 *   the bits of an integer (bit 0 the tables clear the tile, bit 1 every sample is sky, bit 2 every sample falls in one checker
 *   cell, bit 3 the tables were usable), 6 the tile's primitive mask as the bits of an integer (bit k: the tile's cone does not
 *   clear miss-test entry k, spheres first, then boxes; all ones when the mask is not in use), 7 the number of those entries,
 *   likewise.  The pre-pass settles a tile with bit 0 and bit 1 or 2 without looking at its pixels.
 * rm_selftest_cull_waves: n_waves waves of 64 positions, pos[(3 w + k) * 64 + lane] (k = x, y, z), thresholds thr[64 w + lane]
 *   and live-lane masks live[w] (not 0); camera position origin[3].  out_masks[w]: the units wave-level culling keeps -- the
 *   threshold rule (lattice programs; extra_margin unused) or the rules of a blending chain (thr unused), by the program;
 *   RM_ERR_ARG when the program has no units. */
int rm_selftest_cull_rays(rm_ctx* ctx, const float* origin, const float* dirs, uint32_t n, uint32_t* out_flags, float* out_bound);
int rm_selftest_cull_pixels(rm_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* xy, uint32_t n, float* out);
int rm_selftest_cull_tiles(rm_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* xy, uint32_t n, float* out);
int rm_selftest_cull_waves(rm_ctx* ctx, const float* origin, const float* pos, const float* thr, const uint64_t* live, uint32_t n_waves,
                           float extra_margin, uint64_t* out_masks);
/* rm_selftest_anchor: the anchored pruning threshold of a ray's first own step (rm_kernel_v5.h "Pruning"; the device functions
 * the march calls, anchor_reach and anchor_thr_base) on n <= 2^20 pairs of points the caller chooses, pairs[6 i + 0..2] the
 * anchor a and 3..5 the evaluation point q; camera position origin[3] (the |ro|_1 of the margins).  The context's program is
 * evaluated at both points by the interpreter loop a query of it runs.  out[4 i + ..]: 0 the anchor's reach aT, 1 the
 * threshold the step would hand to the culling at q when the camera's own bound is +inf -- anchor_thr_base(+inf, q, a, aT)
 * plus the step's position term --, 2 the value computed at a, 3 the value computed at q.  (Additive: RM_ABI_VERSION stays 2.)
 * tests/test_gpu_anchor.py holds 1 against |3| and against binary64 geometry. */
int rm_selftest_anchor(rm_ctx* ctx, const float* origin, const float* pairs, uint32_t n, float* out);

/* Diagnostics: per-wave records of the last draw made with RM_OPT_WAVE_STATS = 1, four u64 per
 * wave in dispatch order (frame, workgroup, wave of the workgroup): [0] start, [1] end (100 MHz s_memrealtime ticks),
 * [2] tiles the wave's workgroup took from the work list << 32 | map_scene iterations, [3] refills << 32 | sum over
 * iterations of live lanes. */
int rm_read_wave_stats(rm_ctx* ctx, void* dst, uint64_t cap_bytes, uint64_t* out_bytes);

/* Message for the last error on this context (ctx may be NULL: last rm_create error). */
/* Structure specialisation (RM_OPT_SPECIALIZE), inspection entry points.  None of them needs a GPU.
 * rm_jit_source: the HIP source generated for a command stream (NUL-terminated, truncated to cap; *needed = full length + 1).
 * rm_jit_compile: generate and compile it for gfx950 with hipRTC; RM_ERR_DEVICE if libhiprtc is missing or the
 *                 compilation fails (log receives the reason).  Nothing is cached or loaded.
 * rm_jit_log: compiler / loader messages for the context's current program (empty string if none). */
#define RM_JIT_PRUNE 0x100 /* OR into waves_per_tile: generate the RM_OPT_PRUNE = 1 form of the kernel */
#define RM_JIT_RANGE_PROVED 0x200 /* OR into waves_per_tile, with RM_JIT_PRUNE: the variant without the range guards
                                     (RM_INFO_RANGE_PROOF); ignored for programs that get no such variant */
int rm_jit_source(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, int waves_per_tile, char* buf, size_t cap,
                  size_t* needed);
int rm_jit_compile(uint32_t cmd_count, const uint32_t* words, uint32_t n_words, int waves_per_tile, double* compile_ms,
                   size_t* code_bytes, char* log, size_t log_cap);
int rm_jit_log(rm_ctx* ctx, char* buf, size_t cap);

const char* rm_last_error(rm_ctx* ctx);
const char* rm_status_string(int status);

#ifdef __cplusplus
}
#endif
#endif /* RM_ABI_H */
