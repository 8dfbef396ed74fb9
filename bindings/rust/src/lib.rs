//! rm_hip -- Rust binding of include/rm_abi.h (librm_hip.so, C ABI version 2).
//!
//! NOT COMPILED IN THE BUILD IMAGE: it has no rustc/cargo.  What is checked there instead
//! (tests/test_rust_binding.py): every function include/rm_abi.h declares appears in the `extern "C"`
//! block below with the same name, the same number of parameters and matching parameter / return
//! types, every constant has the header's value, and attributes sit on items that accept them; the
//! same test runs `cargo check --offline` when a toolchain is on PATH.  The verified consumers of
//! the ABI are the ctypes bindings (ray-marching_amd/_ffi.py) and the C++ mirror
//! (ray-marching_amd/csrc/host/renderer.hpp).
//!
//! The crate shows what a maintainer of Mesoptier/ray-marching would add to swap the wgpu objects
//! of `src/ray_marching/renderer.rs` for the HIP path while keeping `CSGNode`, `BuildCommands`,
//! `CSGCommandBufferBuilder`, `Camera` and `RayMarchingCallback::new(time, csg_node, viewport,
//! camera)` untouched.
#![allow(non_camel_case_types)]
use std::cell::Cell;
use std::ffi::{c_char, c_int, c_void, CStr};
use std::fmt;

/// Version of the C ABI these declarations were written against (`RM_ABI_VERSION`).
pub const RM_ABI_VERSION: c_int = 2;

#[repr(C)]
pub struct rm_ctx {
    _private: [u8; 0],
}

/// `Uniforms` (renderer.rs:29-34), 144 bytes: exactly `Uniforms::as_shader_bytes()`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct rm_uniforms {
    pub viewport_extent: [f32; 2],
    pub _pad: [f32; 2],
    pub inv_proj: [f32; 16],
    pub inv_view: [f32; 16],
}

/// `RayMarchLimits` (renderer.rs:36-41), 12 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct rm_limits {
    pub min_dist: f32,
    pub max_dist: f32,
    pub max_iter: u32,
}

// enum rm_buffer: binding numbers of the reference's bind group (renderer.rs:60-94)
pub const RM_BUF_LIMITS: c_int = 0;
pub const RM_BUF_COMMANDS: c_int = 1;
pub const RM_BUF_UNIFORMS: c_int = 2;

// enum rm_status
pub const RM_OK: c_int = 0;
pub const RM_ERR_NULL: c_int = -1;
pub const RM_ERR_TRUNCATED: c_int = -2;
pub const RM_ERR_STACK_UNDERFLOW: c_int = -3;
pub const RM_ERR_STACK_OVERFLOW: c_int = -4;
pub const RM_ERR_EMPTY_RESULT: c_int = -5;
pub const RM_ERR_OPCODE: c_int = -6;
pub const RM_ERR_TOO_LARGE: c_int = -7;
pub const RM_ERR_RANGE: c_int = -8;
pub const RM_ERR_DEVICE: c_int = -9;
pub const RM_ERR_NO_DEVICE: c_int = -10;
pub const RM_ERR_ARG: c_int = -11;
pub const RM_ERR_TRANSFORM: c_int = -12;
pub const RM_ERR_MATERIAL: c_int = -13;

// enum rm_option (rm_set_option keys)
pub const RM_OPT_KERNEL: c_int = 0;
pub const RM_OPT_TIMING: c_int = 1;
pub const RM_OPT_STRICT_CAP: c_int = 2;
pub const RM_OPT_REFILL_MIN: c_int = 3;
pub const RM_OPT_CULL: c_int = 4;
pub const RM_OPT_BALANCE: c_int = 5;
pub const RM_OPT_WAVE_STATS: c_int = 6;
pub const RM_OPT_WAVES_PER_TILE: c_int = 7;
pub const RM_OPT_SPECIALIZE: c_int = 8; // 0 interpreter kernel only, 1 (default) compile per scene structure in the background, 2 blocking
pub const RM_OPT_PRUNE: c_int = 9;
pub const RM_OPT_OUTPUT_FORMAT: c_int = 10; // RM_FORMAT_*

// enum rm_format
pub const RM_FORMAT_RGBA32F: c_int = 0;
pub const RM_FORMAT_RGBA8_UNORM: c_int = 1;
pub const RM_FORMAT_BGRA8_UNORM: c_int = 2; // what an egui/wgpu surface usually is (renderer.rs:113 `target_format`)

// enum rm_kernel
pub const RM_KERNEL_DEFAULT: c_int = 0;
pub const RM_KERNEL_PIXEL: c_int = 1;
pub const RM_KERNEL_V5: c_int = 12;
pub const RM_KERNEL_V5_LDS: c_int = 13;

// enum rm_info (rm_get_info keys)
pub const RM_INFO_KERNEL_MS: c_int = 0;
pub const RM_INFO_PROGRAM_COMMANDS: c_int = 1;
pub const RM_INFO_PROGRAM_WORDS: c_int = 2;
pub const RM_INFO_PROGRAM_DEPTH: c_int = 3;
pub const RM_INFO_DEVICE: c_int = 4;
pub const RM_INFO_CU_COUNT: c_int = 5;
pub const RM_INFO_SPECIALIZED: c_int = 6;
pub const RM_INFO_JIT_STATE: c_int = 7;
pub const RM_INFO_JIT_COMPILE_MS: c_int = 8;
pub const RM_INFO_PRUNED: c_int = 9;
pub const RM_INFO_INTERPRETER_LOOP: c_int = 10;
pub const RM_INFO_JIT_FROM_CACHE: c_int = 11;
/// 1 when the last march launch ran the kernel compiled without the per-lane range guards (the host proved the ranges).
pub const RM_INFO_RANGE_PROOF: c_int = 12;

// enum rm_program_fact: indices into the array rm_program_info fills
pub const RM_PROGRAM_RECORDS: usize = 0;
pub const RM_PROGRAM_CONES: usize = 1;
pub const RM_PROGRAM_SLABS: usize = 2;
pub const RM_PROGRAM_SUBTRACTED_LEAVES: usize = 3;
pub const RM_PROGRAM_GROUPS: usize = 4;
pub const RM_PROGRAM_SPILL_DEPTH: usize = 5;
pub const RM_PROGRAM_IS_CHAIN: usize = 6;
pub const RM_PROGRAM_PRUNABLE: usize = 7;
pub const RM_PROGRAM_BOUND_WALK: usize = 8;
pub const RM_PROGRAM_HAS_XFORMS: usize = 9;
pub const RM_PROGRAM_LEAVES: usize = 10;
pub const RM_PROGRAM_AUTO_PRUNED: usize = 11;
pub const RM_PROGRAM_FACTS: usize = 12;

/// `RM_JIT_PRUNE`: OR into `waves_per_tile` of rm_jit_source / rm_jit_compile.
pub const RM_JIT_PRUNE: c_int = 0x100;

/// `RM_STREAM_OWN`: pass as `stream` of a device-destination draw to use the context's own stream.
pub const RM_STREAM_OWN: *mut c_void = usize::MAX as *mut c_void;

// Scene queries (rm_query_points / rm_cast_rays / rm_camera_rays).
/// `RM_NO_ID`: no primitive (an empty program, or a ray that hit no surface).
pub const RM_NO_ID: u32 = 0xFFFF_FFFF;
// enum rm_hit
pub const RM_HIT_NONE: c_int = 0;
pub const RM_HIT_SURFACE: c_int = 1;
pub const RM_HIT_FLOOR: c_int = 2;
// enum rm_sample
pub const RM_SAMPLE_CENTER: c_int = 16;
// enum rm_sampleset
/// `rm_draw_gbuffer` only: all sixteen AA samples.
pub const RM_SAMPLE_ALL: c_int = 17;

// Mesh export (rm_sample_grid / rm_extract_mesh / rm_read_mesh / rm_mesh_case_table).
// enum rm_mesh: flags of rm_extract_mesh
pub const RM_MESH_NORMALS: c_int = 1;
pub const RM_MESH_IDS: c_int = 2;
// enum rm_meshstat: indices into the statistics of rm_extract_mesh_sparse; RM_MESH_STATS is their number
pub const RM_MESH_STAT_VERTICES: c_int = 0;
pub const RM_MESH_STAT_TRIANGLES: c_int = 1;
pub const RM_MESH_STAT_BRICKS: c_int = 2;
pub const RM_MESH_STAT_BRICKS_KEPT: c_int = 3;
pub const RM_MESH_STAT_EVALUATIONS: c_int = 4;
pub const RM_MESH_STAT_SCRATCH_BYTES: c_int = 5;
pub const RM_MESH_STATS: c_int = 6;
// enum rm_moment: indices into the moments of rm_mass_moments; RM_MOMENTS is their number
pub const RM_MOMENT_COUNT: c_int = 0;
pub const RM_MOMENT_X: c_int = 1;
pub const RM_MOMENT_Y: c_int = 2;
pub const RM_MOMENT_Z: c_int = 3;
pub const RM_MOMENT_XX: c_int = 4;
pub const RM_MOMENT_YY: c_int = 5;
pub const RM_MOMENT_ZZ: c_int = 6;
pub const RM_MOMENT_XY: c_int = 7;
pub const RM_MOMENT_YZ: c_int = 8;
pub const RM_MOMENT_XZ: c_int = 9;
pub const RM_MOMENT_MIN_X: c_int = 10;
pub const RM_MOMENT_MIN_Y: c_int = 11;
pub const RM_MOMENT_MIN_Z: c_int = 12;
pub const RM_MOMENT_MAX_X: c_int = 13;
pub const RM_MOMENT_MAX_Y: c_int = 14;
pub const RM_MOMENT_MAX_Z: c_int = 15;
pub const RM_MOMENTS: c_int = 16;
// enum rm_massstat: indices into the statistics of rm_mass_moments; RM_MASS_STATS is their number
pub const RM_MASS_STAT_BRICKS: c_int = 0;
pub const RM_MASS_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_MASS_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_MASS_STAT_EVALUATIONS: c_int = 3;
pub const RM_MASS_STAT_SCRATCH_BYTES: c_int = 4;
pub const RM_MASS_STATS: c_int = 5;
// enum rm_massprop: indices into the output of rm_mass_from_moments; RM_MASS_PROPS is their number
pub const RM_MASS_VOLUME: c_int = 0;
pub const RM_MASS_MASS: c_int = 1;
pub const RM_MASS_CX: c_int = 2;
pub const RM_MASS_CY: c_int = 3;
pub const RM_MASS_CZ: c_int = 4;
pub const RM_MASS_IXX: c_int = 5;
pub const RM_MASS_IYY: c_int = 6;
pub const RM_MASS_IZZ: c_int = 7;
pub const RM_MASS_IXY: c_int = 8;
pub const RM_MASS_IYZ: c_int = 9;
pub const RM_MASS_IXZ: c_int = 10;
pub const RM_MASS_LO_X: c_int = 11;
pub const RM_MASS_LO_Y: c_int = 12;
pub const RM_MASS_LO_Z: c_int = 13;
pub const RM_MASS_HI_X: c_int = 14;
pub const RM_MASS_HI_Y: c_int = 15;
pub const RM_MASS_HI_Z: c_int = 16;
pub const RM_MASS_PROPS: c_int = 17;

// Solid topology (rm_label_solid / rm_label_occupancy / rm_read_topology).
/// `RM_TOPO_CAVITY_BIT`: a cavity point of the label volume holds this bit | its cavity's number.
pub const RM_TOPO_CAVITY_BIT: u32 = 0x8000_0000;
/// `RM_TOPO_EXTERIOR`: a point of the exterior in the label volume.
pub const RM_TOPO_EXTERIOR: u32 = 0xFFFF_FFFF;
// enum rm_topocount: indices into the counts of a labelling call; RM_TOPO_COUNTS is their number
pub const RM_TOPO_BODIES: c_int = 0;
pub const RM_TOPO_CAVITIES: c_int = 1;
pub const RM_TOPO_POINTS: c_int = 2;
pub const RM_TOPO_EDGES: c_int = 3;
pub const RM_TOPO_FACES: c_int = 4;
pub const RM_TOPO_CELLS: c_int = 5;
pub const RM_TOPO_EULER: c_int = 6;
pub const RM_TOPO_TUNNELS: c_int = 7;
pub const RM_TOPO_EXTERIOR_POINTS: c_int = 8;
pub const RM_TOPO_COUNTS: c_int = 9;
// enum rm_topostat: indices into the statistics of a labelling call; RM_TOPO_STATS is their number
pub const RM_TOPO_STAT_BRICKS: c_int = 0;
pub const RM_TOPO_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_TOPO_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_TOPO_STAT_EVALUATIONS: c_int = 3;
pub const RM_TOPO_STAT_MERGE_PASSES: c_int = 4;
pub const RM_TOPO_STAT_SCRATCH_BYTES: c_int = 5;
pub const RM_TOPO_STATS: c_int = 6;

// Distance transform (rm_distance_solid / rm_distance_occupancy / rm_distance_features / rm_read_distance).
/// `RM_DIST_INSIDE_BIT`: ORed into the squared distance of an inside point of the distance volume.
pub const RM_DIST_INSIDE_BIT: u32 = 0x8000_0000;
/// `RM_DIST_NONE`: the squared distance of an outside point when the solid is empty.
pub const RM_DIST_NONE: u32 = 0x7FFF_FFFF;
/// `RM_DIST_SKIP`: as a squared radius of `distance_features`, leaves that half out.
pub const RM_DIST_SKIP: u32 = 0xFFFF_FFFF;
// enum rm_distcount: indices into the counts of a distance call; RM_DIST_COUNTS is their number
pub const RM_DIST_POINTS: c_int = 0;
pub const RM_DIST_MAX_INSIDE: c_int = 1;
pub const RM_DIST_ARGMAX_INSIDE: c_int = 2;
pub const RM_DIST_MAX_OUTSIDE: c_int = 3;
pub const RM_DIST_ARGMAX_OUTSIDE: c_int = 4;
pub const RM_DIST_COUNTS: c_int = 5;
// enum rm_distfeature: indices into the counts of rm_distance_features; RM_DIST_FEATURE_COUNTS is their number
pub const RM_DIST_CORE: c_int = 0;
pub const RM_DIST_THIN: c_int = 1;
pub const RM_DIST_GAP_CORE: c_int = 2;
pub const RM_DIST_NARROW: c_int = 3;
pub const RM_DIST_FEATURE_COUNTS: c_int = 4;
// enum rm_diststat: indices into the statistics of a distance call; RM_DIST_STATS is their number
pub const RM_DIST_STAT_BRICKS: c_int = 0;
pub const RM_DIST_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_DIST_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_DIST_STAT_EVALUATIONS: c_int = 3;
pub const RM_DIST_STAT_SCRATCH_BYTES: c_int = 4;
pub const RM_DIST_STATS: c_int = 5;

// Overhangs and supports (rm_support_solid / rm_support_occupancy / rm_read_support).
/// `RM_SUPPORT_PLATE_AUTO`: as a plate, the lowest height that holds an inside point.
pub const RM_SUPPORT_PLATE_AUTO: u32 = 0xFFFF_FFFF;
// enum rm_up: the build directions
pub const RM_UP_POS_X: c_int = 0;
pub const RM_UP_NEG_X: c_int = 1;
pub const RM_UP_POS_Y: c_int = 2;
pub const RM_UP_NEG_Y: c_int = 3;
pub const RM_UP_POS_Z: c_int = 4;
pub const RM_UP_NEG_Z: c_int = 5;
// enum rm_supcount: indices into the counts of a support call; RM_SUP_COUNTS is their number
pub const RM_SUP_POINTS: c_int = 0;
pub const RM_SUP_PLATE: c_int = 1;
pub const RM_SUP_BASE: c_int = 2;
pub const RM_SUP_OVERHANG: c_int = 3;
pub const RM_SUP_SUPPORT_ON_PLATE: c_int = 4;
pub const RM_SUP_SUPPORT_ON_PART: c_int = 5;
pub const RM_SUP_RUNS: c_int = 6;
pub const RM_SUP_LANDINGS: c_int = 7;
pub const RM_SUP_COUNTS: c_int = 8;
// enum rm_supstat: indices into the statistics of a support call; RM_SUP_STATS is their number
pub const RM_SUP_STAT_BRICKS: c_int = 0;
pub const RM_SUP_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_SUP_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_SUP_STAT_EVALUATIONS: c_int = 3;
pub const RM_SUP_STAT_SCRATCH_BYTES: c_int = 4;
pub const RM_SUP_STATS: c_int = 5;

// Layer regions and islands (rm_islands_solid / rm_islands_occupancy / rm_read_islands).
// enum rm_islcount: indices into the counts of an islands call; RM_ISL_COUNTS is their number
pub const RM_ISL_POINTS: c_int = 0;
pub const RM_ISL_PLATE: c_int = 1;
pub const RM_ISL_REGIONS: c_int = 2;
pub const RM_ISL_BASE_REGIONS: c_int = 3;
pub const RM_ISL_ISLANDS: c_int = 4;
pub const RM_ISL_ISLAND_POINTS: c_int = 5;
pub const RM_ISL_MERGES: c_int = 6;
pub const RM_ISL_MAX_LAYER_REGIONS: c_int = 7;
pub const RM_ISL_COUNTS: c_int = 8;
// enum rm_islstat: indices into the statistics of an islands call; RM_ISL_STATS is their number
pub const RM_ISL_STAT_BRICKS: c_int = 0;
pub const RM_ISL_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_ISL_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_ISL_STAT_EVALUATIONS: c_int = 3;
pub const RM_ISL_STAT_SCRATCH_BYTES: c_int = 4;
pub const RM_ISL_STATS: c_int = 5;
// enum rm_islrow: the words of a row of the region table; RM_ISL_ROW_WORDS is their number
pub const RM_ISL_ROW_LAYER: c_int = 0;
pub const RM_ISL_ROW_FIRST: c_int = 1;
pub const RM_ISL_ROW_POINTS: c_int = 2;
pub const RM_ISL_ROW_SUPPORTED: c_int = 3;
pub const RM_ISL_ROW_SUM_A: c_int = 4;
pub const RM_ISL_ROW_SUM_B: c_int = 5;
pub const RM_ISL_ROW_MIN_A: c_int = 6;
pub const RM_ISL_ROW_MAX_A: c_int = 7;
pub const RM_ISL_ROW_MIN_B: c_int = 8;
pub const RM_ISL_ROW_MAX_B: c_int = 9;
pub const RM_ISL_ROW_BELOW_MIN: c_int = 10;
pub const RM_ISL_ROW_BELOW_MAX: c_int = 11;
pub const RM_ISL_ROW_WORDS: c_int = 12;

// Surface measures (rm_surface_solid / rm_surface_classes / rm_surface_directions / rm_surface_measures).
// enum rm_surfcount: classes, directions, where POINTS and PAIR start in the counts of a surface call; RM_SURF_COUNTS is their number
pub const RM_SURF_CLASSES: c_int = 8;
pub const RM_SURF_DIRS: c_int = 13;
pub const RM_SURF_POINTS: c_int = 0;
pub const RM_SURF_PAIRS: c_int = 8;
pub const RM_SURF_COUNTS: c_int = 840;
// enum rm_surfstat: indices into the statistics of a surface call; RM_SURF_STATS is their number
pub const RM_SURF_STAT_BRICKS: c_int = 0;
pub const RM_SURF_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_SURF_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_SURF_STAT_EVALUATIONS: c_int = 3;
pub const RM_SURF_STAT_SCRATCH_BYTES: c_int = 4;
pub const RM_SURF_STATS: c_int = 5;
// enum rm_surfmeasure: indices into the output of rm_surface_measures; RM_SURF_MEASURES is their number
pub const RM_SURF_AREA: c_int = 0;
pub const RM_SURF_FACET_AREA: c_int = 1;
pub const RM_SURF_FACET_POS_X: c_int = 2;
pub const RM_SURF_FACET_NEG_X: c_int = 3;
pub const RM_SURF_FACET_POS_Y: c_int = 4;
pub const RM_SURF_FACET_NEG_Y: c_int = 5;
pub const RM_SURF_FACET_POS_Z: c_int = 6;
pub const RM_SURF_FACET_NEG_Z: c_int = 7;
pub const RM_SURF_MEASURES: c_int = 8;

// Mesh voxelisation (rm_voxelize_mesh / rm_read_voxels).
// enum rm_voxcount: indices into the counts of a voxelisation; RM_VOX_COUNTS is their number
pub const RM_VOX_TRIANGLES: c_int = 0;
pub const RM_VOX_REJECTED: c_int = 1;
pub const RM_VOX_EDGE_ON: c_int = 2;
pub const RM_VOX_CROSSINGS: c_int = 3;
pub const RM_VOX_INSIDE: c_int = 4;
pub const RM_VOX_OPEN_ROWS: c_int = 5;
pub const RM_VOX_COUNTS: c_int = 6;
// enum rm_voxstat: indices into the statistics of a voxelisation; RM_VOX_STATS is their number
pub const RM_VOX_STAT_BRICKS: c_int = 0;
pub const RM_VOX_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_VOX_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_VOX_STAT_EVALUATIONS: c_int = 3;
pub const RM_VOX_STAT_ITEMS: c_int = 4;
pub const RM_VOX_STAT_SCRATCH_BYTES: c_int = 5;
pub const RM_VOX_STATS: c_int = 6;

// Lattice draw (rm_set_lattice / rm_draw_lattice / rm_cast_lattice).
// enum rm_latcount: indices into the counts of a lattice; RM_LAT_COUNTS is their number
pub const RM_LAT_POINTS: c_int = 0;
pub const RM_LAT_BRICKS: c_int = 1;
pub const RM_LAT_COUNTS: c_int = 2;
// enum rm_latstat: indices into the statistics of a lattice; RM_LAT_STATS is their number
pub const RM_LAT_STAT_BRICKS: c_int = 0;
pub const RM_LAT_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_LAT_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_LAT_STAT_EVALUATIONS: c_int = 3;
pub const RM_LAT_STAT_RETAINED_BYTES: c_int = 4;
pub const RM_LAT_STAT_SCRATCH_BYTES: c_int = 5;
pub const RM_LAT_STATS: c_int = 6;
/// The face word of a cast whose origin lies inside a full cube.
pub const RM_LAT_FACE_NONE: u32 = 6;

// Lattice meshing (rm_mesh_classes / rm_read_class_mesh).
// enum rm_cmeshcount: indices into the counts of a class mesh; RM_CMESH_COUNTS is their number
pub const RM_CMESH_VERTICES: c_int = 0;
pub const RM_CMESH_TRIANGLES: c_int = 1;
pub const RM_CMESH_FACES: c_int = 2;
pub const RM_CMESH_FACES_POS_X: c_int = 3;
pub const RM_CMESH_FACES_NEG_X: c_int = 4;
pub const RM_CMESH_FACES_POS_Y: c_int = 5;
pub const RM_CMESH_FACES_NEG_Y: c_int = 6;
pub const RM_CMESH_FACES_POS_Z: c_int = 7;
pub const RM_CMESH_FACES_NEG_Z: c_int = 8;
pub const RM_CMESH_EDGES: c_int = 9;
pub const RM_CMESH_OPEN_EDGES: c_int = 10;
pub const RM_CMESH_BRANCH_EDGES: c_int = 11;
pub const RM_CMESH_COUNTS: c_int = 12;
// enum rm_cmeshstat: indices into the statistics of a class mesh; RM_CMESH_STATS is their number
pub const RM_CMESH_STAT_BRICKS: c_int = 0;
pub const RM_CMESH_STAT_BRICKS_KEPT: c_int = 1;
pub const RM_CMESH_STAT_BRICKS_INSIDE: c_int = 2;
pub const RM_CMESH_STAT_EVALUATIONS: c_int = 3;
pub const RM_CMESH_STAT_RETAINED_BYTES: c_int = 4;
pub const RM_CMESH_STAT_SCRATCH_BYTES: c_int = 5;
pub const RM_CMESH_STATS: c_int = 6;

/// The index of `PAIR[a][b][nu]` in the counts of a surface call (the header's `RM_SURF_PAIR`).
pub const fn surf_pair(a: usize, b: usize, nu: usize) -> usize {
    8 + (8 * a + b) * 13 + nu
}

// Slicing (rm_slice_contours / rm_read_slices / rm_slice_case_table).
// enum rm_slicecount: indices into the counts of rm_slice_contours; RM_SLICE_COUNTS is their number
pub const RM_SLICE_POINTS: c_int = 0;
pub const RM_SLICE_CONTOURS: c_int = 1;
pub const RM_SLICE_COUNTS: c_int = 2;

// Mesh slicing (rm_slice_mesh; read with rm_read_slices).
// enum rm_mslicecount: indices into the counts of rm_slice_mesh; RM_MSLICE_COUNTS is their number
pub const RM_MSLICE_TRIANGLES: c_int = 0;
pub const RM_MSLICE_REJECTED: c_int = 1;
pub const RM_MSLICE_PAIRED_EDGES: c_int = 2;
pub const RM_MSLICE_BORDER_EDGES: c_int = 3;
pub const RM_MSLICE_BRANCH_EDGES: c_int = 4;
pub const RM_MSLICE_SEGMENTS: c_int = 5;
pub const RM_MSLICE_POINTS: c_int = 6;
pub const RM_MSLICE_CONTOURS: c_int = 7;
pub const RM_MSLICE_OPEN_CONTOURS: c_int = 8;
pub const RM_MSLICE_COUNTS: c_int = 9;
// enum rm_mslicestat: indices into the statistics of rm_slice_mesh; RM_MSLICE_STATS is their number
pub const RM_MSLICE_STAT_SORT_PASSES: c_int = 0;
pub const RM_MSLICE_STAT_RANK_ROUNDS: c_int = 1;
pub const RM_MSLICE_STAT_SCRATCH_BYTES: c_int = 2;
pub const RM_MSLICE_STATS: c_int = 3;
// Hatching (rm_hatch_slices / rm_read_hatch).
// enum rm_hatchflag
pub const RM_HATCH_ZIGZAG: c_int = 1;
// enum rm_hatchcount: indices into the counts of rm_hatch_slices; RM_HATCH_COUNTS is their number
pub const RM_HATCH_SEGMENTS_IN: c_int = 0;
pub const RM_HATCH_CROSSINGS: c_int = 1;
pub const RM_HATCH_SEGMENTS: c_int = 2;
pub const RM_HATCH_LINES_HIT: c_int = 3;
pub const RM_HATCH_ODD_LINES: c_int = 4;
pub const RM_HATCH_COUNTS: c_int = 5;
// enum rm_hatchstat: indices into the statistics of rm_hatch_slices; RM_HATCH_STATS is their number
pub const RM_HATCH_STAT_SORT_PASSES: c_int = 0;
pub const RM_HATCH_STAT_SCRATCH_BYTES: c_int = 1;
pub const RM_HATCH_STATS: c_int = 2;

// Lit rendering (rm_lighting_defaults / rm_set_lighting / rm_draw_lit).
// enum rm_light: indices into the parameter array; RM_LIGHT_PARAMS is its length
pub const RM_LIGHT_POS_X: c_int = 0;
pub const RM_LIGHT_POS_Y: c_int = 1;
pub const RM_LIGHT_POS_Z: c_int = 2;
pub const RM_LIGHT_SHADOW: c_int = 3;
pub const RM_LIGHT_SHADOW_SOFTNESS: c_int = 4;
pub const RM_LIGHT_BIAS: c_int = 5;
pub const RM_LIGHT_SHADOW_MAX_T: c_int = 6;
pub const RM_LIGHT_SHADOW_STEPS: c_int = 7;
pub const RM_LIGHT_AO: c_int = 8;
pub const RM_LIGHT_AO_STEP: c_int = 9;
pub const RM_LIGHT_AO_FALLOFF: c_int = 10;
pub const RM_LIGHT_AO_SCALE: c_int = 11;
pub const RM_LIGHT_AO_TAPS: c_int = 12;
pub const RM_LIGHT_PARAMS: c_int = 13;

// Ray traversal (rm_trace_defaults / rm_trace_rays).
// enum rm_trace: indices into the parameter array; RM_TRACE_PARAMS is its length
pub const RM_TRACE_T_MIN: c_int = 0;
pub const RM_TRACE_T_MAX: c_int = 1;
pub const RM_TRACE_MIN_STEP: c_int = 2;
pub const RM_TRACE_STEP_SCALE: c_int = 3;
pub const RM_TRACE_LEVEL: c_int = 4;
pub const RM_TRACE_MAX_STEPS: c_int = 5;
pub const RM_TRACE_PARAMS: c_int = 6;
// enum rm_tracekind: the kind of an event
pub const RM_TRACE_ENTER: c_int = 1;
pub const RM_TRACE_EXIT: c_int = 2;
// enum rm_traceflag: bits of a ray's flags word
pub const RM_TRACE_START_INSIDE: c_int = 1;
pub const RM_TRACE_END_INSIDE: c_int = 2;
pub const RM_TRACE_OUT_OF_STEPS: c_int = 4;
// enum rm_tracelimit
pub const RM_TRACE_MAX_EVENTS: c_int = 64;

// Opcodes of the node types the reference only names in comments (builder.rs:8,14,16-23) and that the device
// path implements as extensions: a CSGCommandType that gains these variants serialises them unchanged.
//   Plane = 2, Intersection = 102, TranslationPush = 200, TranslationPop, RotationPush, RotationPop, ScalePush, ScalePop
//   (Cylinder = 10, SmoothUnion = 110 and Material = 300 are this repo's own numbers)

#[link(name = "rm_hip")]
extern "C" {
    pub fn rm_abi_version() -> c_int;
    pub fn rm_device_count() -> c_int;
    pub fn rm_create(device: c_int, out: *mut *mut rm_ctx) -> c_int;
    pub fn rm_destroy(ctx: *mut rm_ctx);
    pub fn rm_write_buffer(ctx: *mut rm_ctx, buffer: c_int, offset: u64, data: *const c_void, size: u64) -> c_int;
    pub fn rm_set_uniforms(ctx: *mut rm_ctx, u: *const rm_uniforms) -> c_int;
    pub fn rm_set_limits(ctx: *mut rm_ctx, l: *const rm_limits) -> c_int;
    pub fn rm_set_program(ctx: *mut rm_ctx, cmd_count: u32, words: *const u32, n_words: u32) -> c_int;
    pub fn rm_set_materials(ctx: *mut rm_ctx, count: u32, rgb: *const f32) -> c_int;
    pub fn rm_resize_command_buffer(ctx: *mut rm_ctx, bytes: u64) -> c_int;
    pub fn rm_validate(ctx: *mut rm_ctx) -> c_int;
    pub fn rm_validate_program(cmd_count: u32, words: *const u32, n_words: u32, out_max_depth: *mut u32) -> c_int;
    pub fn rm_program_info(cmd_count: u32, words: *const u32, n_words: u32, out: *mut u32, n_out: u32) -> c_int;
    pub fn rm_draw(ctx: *mut rm_ctx, w: u32, h: u32, row0: u32, rows: u32, out_rgba: *mut f32, out_is_device: c_int,
                   stream: *mut c_void) -> c_int;
    pub fn rm_draw_strips(ctx: *mut rm_ctx, w: u32, h: u32, strip_rows: u32, first: u32, stride: u32, out_rgba: *mut f32,
                          out_is_device: c_int, stream: *mut c_void, out_rows: *mut u32) -> c_int;
    pub fn rm_gather_strips(ctx: *mut rm_ctx, w: u32, h: u32, strip_rows: u32, first: u32, stride: u32,
                            strips_device: *const c_void, host_image: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn rm_host_register(ptr: *mut c_void, bytes: u64) -> c_int;
    pub fn rm_host_unregister(ptr: *mut c_void) -> c_int;
    pub fn rm_draw_batch(ctx: *mut rm_ctx, frames: *const rm_uniforms, n_frames: u32, w: u32, h: u32, out_rgba: *mut f32,
                         out_is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_query_points(ctx: *mut rm_ctx, n: u32, xyz: *const f32, out_dist: *mut f32, out_normal: *mut f32, out_ids: *mut u32,
                           is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_cast_rays(ctx: *mut rm_ctx, n: u32, rays: *const f32, out_hit: *mut f32, out_ids: *mut u32, out_rgb: *mut f32,
                        is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_camera_rays(ctx: *mut rm_ctx, w_frame: u32, h_frame: u32, x0: u32, y0: u32, w: u32, h: u32, sample: u32,
                          out_rays: *mut f32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_trace_defaults(out: *mut f32, n_out: u32) -> c_int;
    pub fn rm_trace_rays(ctx: *mut rm_ctx, n: u32, rays: *const f32, params: *const f32, n_params: u32, max_events: u32, flags: u32,
                         out_events: *mut f32, out_event_ids: *mut u32, out_counts: *mut u32, out_spans: *mut f32,
                         is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_sample_grid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, out_dist: *mut f32,
                          is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_extract_mesh(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                           flags: u32, out_counts: *mut u64) -> c_int;
    pub fn rm_read_mesh(ctx: *mut rm_ctx, out_vertices: *mut f32, out_triangles: *mut u32, out_normals: *mut f32,
                        out_ids: *mut u32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_mesh_case_table(out: *mut u32, n_out: u32) -> c_int;
    pub fn rm_extract_mesh_sparse(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                                  flags: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_mass_moments(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                           out_moments: *mut u64, n_moments: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_mass_from_moments(moments: *const u64, n_moments: u32, origin: *const f32, step: *const f32, density: f64,
                                out: *mut f64, n_out: u32) -> c_int;
    pub fn rm_label_solid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                          out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_label_occupancy(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, occupancy: *const c_void, is_device: c_int,
                              stream: *mut c_void, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_topology(ctx: *mut rm_ctx, out_body_moments: *mut u64, out_cavity_moments: *mut u64, out_labels: *mut u32,
                            is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_distance_solid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                             out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_distance_occupancy(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, occupancy: *const c_void, is_device: c_int,
                                 stream: *mut c_void, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_distance_features(ctx: *mut rm_ctx, r2_wall: u32, r2_gap: u32, out_counts: *mut u64, n_counts: u32) -> c_int;
    pub fn rm_read_distance(ctx: *mut rm_ctx, out_d2: *mut u32, out_mask: *mut c_void, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_support_solid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32, up: u32,
                            r2: u32, plate: u32, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_support_occupancy(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, occupancy: *const c_void, is_device: c_int,
                                stream: *mut c_void, up: u32, r2: u32, plate: u32, out_counts: *mut u64, n_counts: u32,
                                out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_support(ctx: *mut rm_ctx, out_mask: *mut c_void, out_profile: *mut u32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_islands_solid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32, up: u32,
                            r2: u32, plate: u32, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_islands_occupancy(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, occupancy: *const c_void, is_device: c_int,
                                stream: *mut c_void, up: u32, r2: u32, plate: u32, out_counts: *mut u64, n_counts: u32,
                                out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_islands(ctx: *mut rm_ctx, out_rows: *mut u32, row_capacity: u64, out_labels: *mut u32, out_mask: *mut c_void,
                           out_profile: *mut u32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_surface_solid(ctx: *mut rm_ctx, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32, level: f32,
                            out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_surface_classes(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, classes: *const c_void, is_device: c_int,
                              stream: *mut c_void, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_surface_directions(out: *mut c_int, n_out: u32) -> c_int;
    pub fn rm_surface_measures(counts: *const u64, n_counts: u32, step: *const f32, mask_a: u32, mask_b: u32, out: *mut f64,
                               n_out: u32) -> c_int;
    pub fn rm_voxelize_mesh(ctx: *mut rm_ctx, n_vertices: u32, xyz: *const f32, n_triangles: u32, indices: *const u32,
                            is_device: c_int, stream: *mut c_void, origin: *const f32, step: *const f32, nx: u32, ny: u32, nz: u32,
                            out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_voxels(ctx: *mut rm_ctx, out_occupancy: *mut c_void, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_set_lattice(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, classes: *const c_void, is_device: c_int, stream: *mut c_void,
                          origin: *const f32, step: *const f32, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64,
                          n_stats: u32) -> c_int;
    pub fn rm_draw_lattice(ctx: *mut rm_ctx, w: u32, h: u32, row0: u32, rows: u32, window: *const u32, out_rgba: *mut c_void,
                           out_is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_cast_lattice(ctx: *mut rm_ctx, n: u32, rays: *const f32, window: *const u32, out_hit: *mut f32, out_ids: *mut u32,
                           out_rgb: *mut f32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_mesh_classes(ctx: *mut rm_ctx, nx: u32, ny: u32, nz: u32, classes: *const c_void, is_device: c_int, stream: *mut c_void,
                           origin: *const f32, step: *const f32, mask_a: u32, mask_b: u32, out_counts: *mut u64, n_counts: u32,
                           out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_class_mesh(ctx: *mut rm_ctx, out_vertices: *mut f32, out_triangles: *mut u32, out_ids: *mut u32, is_device: c_int,
                              stream: *mut c_void) -> c_int;
    pub fn rm_slice_mesh(ctx: *mut rm_ctx, xyz: *const f32, n_vertices: u32, triangles: *const u32, n_triangles: u32, is_device: c_int,
                         stream: *mut c_void, origin: *const f32, step: *const f32, axis: u32, heights: *const f32, n_layers: u32,
                         flags: u32, out_counts: *mut u64, n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_hatch_slices(ctx: *mut rm_ctx, lines: *const f32, n_layers: u32, n_lines: u32, flags: u32, out_counts: *mut u64,
                           n_counts: u32, out_stats: *mut u64, n_stats: u32) -> c_int;
    pub fn rm_read_hatch(ctx: *mut rm_ctx, out_segments: *mut f32, out_line: *mut u32, out_layer_first: *mut u32, is_device: c_int,
                         stream: *mut c_void) -> c_int;
    pub fn rm_slice_contours(ctx: *mut rm_ctx, axis: u32, origin_uv: *const f32, step_uv: *const f32, nu: u32, nv: u32,
                             heights: *const f32, n_layers: u32, level: f32, flags: u32, out_counts: *mut u64,
                             n_counts: u32) -> c_int;
    pub fn rm_read_slices(ctx: *mut rm_ctx, out_points: *mut f32, out_contours: *mut u32, out_layer_first: *mut u32,
                          out_normals: *mut f32, out_ids: *mut u32, is_device: c_int, stream: *mut c_void) -> c_int;
    pub fn rm_slice_case_table(out: *mut u32, n_out: u32) -> c_int;
    pub fn rm_program_lipschitz(cmd_count: u32, words: *const u32, n_words: u32, out_l: *mut f64) -> c_int;
    pub fn rm_lighting_defaults(out: *mut f32, n_out: u32) -> c_int;
    pub fn rm_set_lighting(ctx: *mut rm_ctx, params: *const f32, count: u32) -> c_int;
    pub fn rm_draw_lit(ctx: *mut rm_ctx, w: u32, h: u32, row0: u32, rows: u32, out_rgba: *mut f32, out_is_device: c_int,
                       stream: *mut c_void) -> c_int;
    pub fn rm_draw_gbuffer(ctx: *mut rm_ctx, w: u32, h: u32, row0: u32, rows: u32, sample: u32, sel_first: u32, sel_count: u32,
                           out_geom: *mut f32, out_ids: *mut u32, out_masks: *mut u32, is_device: c_int,
                           stream: *mut c_void) -> c_int;
    pub fn rm_program_subtree(cmd_count: u32, words: *const u32, n_words: u32, cmd_index: u32, out_first: *mut u32,
                              out_count: *mut u32) -> c_int;
    pub fn rm_sync(ctx: *mut rm_ctx) -> c_int;
    pub fn rm_sync_context(ctx: *mut rm_ctx) -> c_int;
    pub fn rm_set_option(ctx: *mut rm_ctx, key: c_int, value: i64) -> c_int;
    pub fn rm_get_info(ctx: *mut rm_ctx, key: c_int, out: *mut f64) -> c_int;
    pub fn rm_measure_write_bandwidth(ctx: *mut rm_ctx, bytes: u64, iters: c_int, out_gbps: *mut f64) -> c_int;
    pub fn rm_selftest_sqrt(ctx: *mut rm_ctx, out_mismatches: *mut u64, out_first_bad_bits: *mut u32) -> c_int;
    pub fn rm_selftest_ops(ctx: *mut rm_ctx, a: *const f32, b: *const f32, out: *mut f32, n: u32) -> c_int;
    pub fn rm_selftest_div(ctx: *mut rm_ctx, a: *const f32, b: *const f32, n: u32, seed: u32, n_seeded: u32, out: *mut u64) -> c_int;
    pub fn rm_selftest_normalise(ctx: *mut rm_ctx, input: *const f32, n: u32, mode: c_int, out: *mut u32) -> c_int;
    pub fn rm_selftest_wave(ctx: *mut rm_ctx, input: *const f32, n_waves: u32, out: *mut f32) -> c_int;
    pub fn rm_selftest_sort(ctx: *mut rm_ctx, keys: *const u64, values: *const u32, n: u32, bits: u32, out_keys: *mut u64,
                            out_values: *mut u32) -> c_int;
    pub fn rm_selftest_cull_rays(ctx: *mut rm_ctx, origin: *const f32, dirs: *const f32, n: u32, out_flags: *mut u32, out_bound: *mut f32) -> c_int;
    pub fn rm_selftest_cull_pixels(ctx: *mut rm_ctx, w: u32, h: u32, xy: *const u32, n: u32, out: *mut f32) -> c_int;
    pub fn rm_selftest_cull_tiles(ctx: *mut rm_ctx, w: u32, h: u32, xy: *const u32, n: u32, out: *mut f32) -> c_int;
    pub fn rm_selftest_cull_waves(ctx: *mut rm_ctx, origin: *const f32, pos: *const f32, thr: *const f32, live: *const u64, n_waves: u32,
                                  extra_margin: f32, out_masks: *mut u64) -> c_int;
    pub fn rm_selftest_anchor(ctx: *mut rm_ctx, origin: *const f32, pairs: *const f32, n: u32, out: *mut f32) -> c_int;
    pub fn rm_read_wave_stats(ctx: *mut rm_ctx, dst: *mut c_void, cap_bytes: u64, out_bytes: *mut u64) -> c_int;
    pub fn rm_jit_source(cmd_count: u32, words: *const u32, n_words: u32, waves_per_tile: c_int, buf: *mut c_char,
                         cap: usize, needed: *mut usize) -> c_int;
    pub fn rm_jit_compile(cmd_count: u32, words: *const u32, n_words: u32, waves_per_tile: c_int, compile_ms: *mut f64,
                          code_bytes: *mut usize, log: *mut c_char, log_cap: usize) -> c_int;
    pub fn rm_jit_log(ctx: *mut rm_ctx, buf: *mut c_char, cap: usize) -> c_int;
    pub fn rm_last_error(ctx: *mut rm_ctx) -> *const c_char;
    pub fn rm_status_string(status: c_int) -> *const c_char;
}

/// The default lighting parameters (`rm_lighting_defaults`; host code, no GPU needed).
pub fn lighting_defaults() -> [f32; RM_LIGHT_PARAMS as usize] {
    let mut out = [0.0f32; RM_LIGHT_PARAMS as usize];
    let rc = unsafe { rm_lighting_defaults(out.as_mut_ptr(), RM_LIGHT_PARAMS as u32) };
    assert_eq!(rc, RM_OK);
    out
}

/// The default traversal parameters (`rm_trace_defaults`; host code, no GPU needed), indexed by `RM_TRACE_*`.
pub fn trace_defaults() -> [f32; RM_TRACE_PARAMS as usize] {
    let mut out = [0.0f32; RM_TRACE_PARAMS as usize];
    let rc = unsafe { rm_trace_defaults(out.as_mut_ptr(), RM_TRACE_PARAMS as u32) };
    assert_eq!(rc, RM_OK);
    out
}

/// The selection of a graph node (`rm_program_subtree`; host code, no GPU needed): the range (first, count) of command
/// indices that produce the value command `cmd_index` leaves on the stack, as `draw_gbuffer` takes it.  `Err(status)` for an
/// invalid program (the validator's status) or an index past the end (`RM_ERR_RANGE`).
pub fn program_subtree(cmd_count: u32, words: &[u32], cmd_index: u32) -> Result<(u32, u32), c_int> {
    assert!(words.len() <= u32::MAX as usize);
    let (mut first, mut count) = (0u32, 0u32);
    let rc = unsafe { rm_program_subtree(cmd_count, words.as_ptr(), words.len() as u32, cmd_index, &mut first, &mut count) };
    if rc == RM_OK { Ok((first, count)) } else { Err(rc) }
}

/// A Lipschitz bound of a program's `map_scene` in real arithmetic (`rm_program_lipschitz`; host code, no GPU needed):
/// `f64::INFINITY` when the program has none (a parameter that is not finite, a Scale of 0).  `Err(status)` for an invalid
/// program.
pub fn program_lipschitz(cmd_count: u32, words: &[u32]) -> Result<f64, c_int> {
    assert!(words.len() <= u32::MAX as usize);
    let mut l = 0.0f64;
    let rc = unsafe { rm_program_lipschitz(cmd_count, words.as_ptr(), words.len() as u32, &mut l) };
    if rc == RM_OK { Ok(l) } else { Err(rc) }
}

/// Volume, mass, centre of mass, inertia about it and bounding box (`out`, at least `RM_MASS_PROPS` entries indexed by
/// `RM_MASS_*`) from the moments of `mass_moments` on the lattice (`origin`, `step`), by the midpoint rule
/// (`rm_mass_from_moments`; host code, no GPU needed).  `Err(status)` for a density or step that is not finite or a step <= 0.
pub fn mass_from_moments(moments: &[u64], origin: [f32; 3], step: [f32; 3], density: f64, out: &mut [f64]) -> Result<(), c_int> {
    assert!(moments.len() >= RM_MOMENTS as usize, "mass_from_moments: moments is shorter than RM_MOMENTS entries");
    assert!(out.len() >= RM_MASS_PROPS as usize, "mass_from_moments: out is shorter than RM_MASS_PROPS entries");
    let rc = unsafe {
        rm_mass_from_moments(moments.as_ptr(), RM_MOMENTS as u32, origin.as_ptr(), step.as_ptr(), density, out.as_mut_ptr(),
                             RM_MASS_PROPS as u32)
    };
    if rc == RM_OK { Ok(()) } else { Err(rc) }
}

/// The 13 directions of the pair counts of a surface call, (x, y, z) each (`rm_surface_directions`; host code, no GPU needed).
pub fn surface_directions() -> [[c_int; 3]; RM_SURF_DIRS as usize] {
    let mut out = [[0 as c_int; 3]; RM_SURF_DIRS as usize];
    let rc = unsafe { rm_surface_directions(out.as_mut_ptr() as *mut c_int, 3 * RM_SURF_DIRS as u32) };
    assert_eq!(rc, RM_OK);
    out
}

/// The interface between the class sets `mask_a` and `mask_b` (bit a = class a; disjoint, not empty) from the counts of
/// `surface_solid` / `surface_classes` and the lattice's `step`: fills `out` (at least `RM_SURF_MEASURES` entries indexed by
/// `RM_SURF_AREA`, `RM_SURF_FACET_*`; AREA is NaN unless the three steps are equal) (`rm_surface_measures`; host code, no GPU
/// needed).  `Err(status)` for masks that are empty, overlap or name a ninth class, and a step that is not finite or <= 0.
pub fn surface_measures(counts: &[u64], step: [f32; 3], mask_a: u32, mask_b: u32, out: &mut [f64]) -> Result<(), c_int> {
    assert!(counts.len() >= RM_SURF_COUNTS as usize, "surface_measures: counts is shorter than RM_SURF_COUNTS entries");
    assert!(out.len() >= RM_SURF_MEASURES as usize, "surface_measures: out is shorter than RM_SURF_MEASURES entries");
    let rc = unsafe {
        rm_surface_measures(counts.as_ptr(), RM_SURF_COUNTS as u32, step.as_ptr(), mask_a, mask_b, out.as_mut_ptr(), RM_SURF_MEASURES as u32)
    };
    if rc == RM_OK { Ok(()) } else { Err(rc) }
}

/// What the reference `unwrap()`s away (renderer.rs:24, 203, 250): a status code of `enum rm_status`
/// plus the library's message for it.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct RmError {
    pub status: i32,
    pub message: String,
}

impl fmt::Display for RmError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "rm_hip error {}: {}", self.status, self.message)
    }
}

impl std::error::Error for RmError {}

/// Replaces `RayMarchingResources` (renderer.rs:43-49): owns the GPU state of one device.
pub struct RayMarchingResources {
    ctx: *mut rm_ctx,
    /// (vertices, triangles) of the mesh the context holds since the last successful `extract_mesh`: what `read_mesh`
    /// writes, so what its slices must hold
    mesh: Cell<Option<(u64, u64)>>,
    /// (points, contours, layers) of the slices the context holds since the last successful `slice_contours`: what
    /// `read_slices` writes, so what its slices must hold
    slices: Cell<Option<(u64, u64, u32)>>,
    hatch: Cell<Option<(u64, u32)>>,  // (segments, layers) of the last hatch of the current slices
    /// (bodies, cavities, lattice points) of the last successful labelling call: what `read_topology` writes
    topology: Cell<Option<(u64, u64, u64)>>,
    /// (lattice points, whether a features call has made a mask) of the last successful distance call: what `read_distance` writes
    distance: Cell<Option<(u64, bool)>>,
    /// (lattice points, layers along the build direction) of the last successful support call: what `read_support` writes
    support: Cell<Option<(u64, u32)>>,
    /// (lattice points, layers along the build direction, regions) of the last successful islands call: what `read_islands` writes
    islands: Cell<Option<(u64, u32, u64)>>,
    /// lattice points of the last successful `voxelize_mesh`: what `read_voxels` writes
    voxels: Cell<Option<u64>>,
    /// (vertices, triangles) of the last successful `mesh_classes`: what `read_class_mesh` writes
    class_mesh: Cell<Option<(u64, u64)>>,
}

unsafe impl Send for RayMarchingResources {} // a context may move between threads; it is not Sync

impl RayMarchingResources {
    /// `RayMarchingResources::new` (renderer.rs:51-175) without a wgpu `RenderState`.
    pub fn new(device: i32) -> Result<Self, RmError> {
        let mut ctx: *mut rm_ctx = std::ptr::null_mut();
        let rc = unsafe { rm_create(device, &mut ctx) };
        if rc != RM_OK {
            let msg = unsafe { CStr::from_ptr(rm_last_error(std::ptr::null_mut())) };
            return Err(RmError { status: rc, message: msg.to_string_lossy().into_owned() });
        }
        Ok(Self { ctx, mesh: Cell::new(None), slices: Cell::new(None), hatch: Cell::new(None), topology: Cell::new(None), distance: Cell::new(None),
                  support: Cell::new(None), islands: Cell::new(None), voxels: Cell::new(None),
                  class_mesh: Cell::new(None) })
    }

    fn check(&self, rc: c_int) -> Result<(), RmError> {
        if rc == RM_OK {
            return Ok(());
        }
        let msg = unsafe { CStr::from_ptr(rm_last_error(self.ctx)) };
        Err(RmError { status: rc, message: msg.to_string_lossy().into_owned() })
    }

    /// `queue.write_buffer(buffer, offset, data)` (renderer.rs:213, 230, 235).
    pub fn write_buffer(&self, buffer: c_int, offset: u64, data: &[u8]) -> Result<(), RmError> {
        self.check(unsafe { rm_write_buffer(self.ctx, buffer, offset, data.as_ptr() as *const c_void, data.len() as u64) })
    }

    /// The reference's TODO (renderer.rs:229): a command buffer larger than 1024 bytes.
    pub fn resize_command_buffer(&self, bytes: u64) -> Result<(), RmError> {
        self.check(unsafe { rm_resize_command_buffer(self.ctx, bytes) })
    }

    /// `RayMarchLimits` (renderer.rs:130-140): the reference writes them once at start-up.
    pub fn set_limits(&self, limits: &rm_limits) -> Result<(), RmError> {
        self.check(unsafe { rm_set_limits(self.ctx, limits) })
    }

    pub fn set_option(&self, key: c_int, value: i64) -> Result<(), RmError> {
        self.check(unsafe { rm_set_option(self.ctx, key, value) })
    }

    /// `render_pass.draw(0..4, 0..2)` (renderer.rs:254) into a host RGBA32F image (top row first).
    pub fn draw(&self, width: u32, height: u32, out_rgba: &mut [f32]) -> Result<(), RmError> {
        assert!(out_rgba.len() >= (width as usize) * (height as usize) * 4);
        self.check(unsafe { rm_draw(self.ctx, width, height, 0, height, out_rgba.as_mut_ptr(), 0, std::ptr::null_mut()) })
    }

    /// All lighting parameters at once (indices `RM_LIGHT_*`; `lighting_defaults()` is the starting point).  A value
    /// outside its range is `RM_ERR_RANGE` and changes nothing.
    pub fn set_lighting(&self, params: &[f32; RM_LIGHT_PARAMS as usize]) -> Result<(), RmError> {
        self.check(unsafe { rm_set_lighting(self.ctx, params.as_ptr(), RM_LIGHT_PARAMS as u32) })
    }

    /// `draw` with soft shadows and ambient occlusion into a host RGBA32F image; with
    /// `RM_LIGHT_SHADOW` and `RM_LIGHT_AO` at 0 the image is `draw`'s bit for bit.
    pub fn draw_lit(&self, width: u32, height: u32, out_rgba: &mut [f32]) -> Result<(), RmError> {
        assert!(out_rgba.len() >= (width as usize) * (height as usize) * 4);
        self.check(unsafe { rm_draw_lit(self.ctx, width, height, 0, height, out_rgba.as_mut_ptr(), 0, std::ptr::null_mut()) })
    }

    /// The geometry behind rows `row0 .. row0 + rows` of a frame (host memory), per pixel: the hit
    /// record of the nearest sample (`out_geom`, eight floats: t, position, normal, diffuse), its (kind, sample id, leaf,
    /// material) (`out_ids`, four words) and (surface mask, floor mask, selected mask, summed steps) (`out_masks`, four
    /// words).  `sample`: 0..15, `RM_SAMPLE_CENTER` or `RM_SAMPLE_ALL`; `select`: a (first, count) range of command indices
    /// (`program_subtree`), (0, 0) for none.  `None` skips that output.
    pub fn draw_gbuffer(&self, width: u32, height: u32, row0: u32, rows: u32, sample: u32, select: (u32, u32),
                        out_geom: Option<&mut [f32]>, out_ids: Option<&mut [u32]>,
                        out_masks: Option<&mut [u32]>) -> Result<(), RmError> {
        let n = (width as usize) * (rows as usize);
        assert!(out_geom.as_ref().map_or(true, |s| s.len() >= 8 * n), "draw_gbuffer: out_geom is shorter than {} pixels", n);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 4 * n), "draw_gbuffer: out_ids is shorter than {} pixels", n);
        assert!(out_masks.as_ref().map_or(true, |s| s.len() >= 4 * n), "draw_gbuffer: out_masks is shorter than {} pixels", n);
        let geom = out_geom.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let ids = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let masks = out_masks.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe {
            rm_draw_gbuffer(self.ctx, width, height, row0, rows, sample, select.0, select.1, geom, ids, masks, 0, std::ptr::null_mut())
        })
    }

    /// This GPU's interleaved strips of a frame tiled over `stride` GPUs (north-star layout), host destination.
    /// Returns the number of rows written.
    pub fn draw_strips(&self, width: u32, height: u32, strip_rows: u32, first: u32, stride: u32,
                       out_rgba: &mut [f32]) -> Result<u32, RmError> {
        // The library writes every row of this GPU's strips: the slice must hold them, or a safe caller could make it
        // write past the end.  (Arguments the library rejects -- strip_rows 0, first >= stride -- write nothing.)
        let need = strip_row_count(height, strip_rows, first, stride) as usize * width as usize * 4;
        assert!(out_rgba.len() >= need, "draw_strips: out_rgba holds {} floats, this GPU's strips need {}", out_rgba.len(), need);
        let mut rows: u32 = 0;
        self.check(unsafe {
            rm_draw_strips(self.ctx, width, height, strip_rows, first, stride, out_rgba.as_mut_ptr(), 0, std::ptr::null_mut(),
                           &mut rows)
        })?;
        Ok(rows)
    }

    /// Scene query at `xyz.len() / 3` points (host memory): signed distance (`out_dist`, one per point), shading normal
    /// (`out_normal`, three per point) and (leaf, material) (`out_ids`, two per point).  `None` skips that output.
    pub fn query_points(&self, xyz: &[f32], out_dist: Option<&mut [f32]>, out_normal: Option<&mut [f32]>,
                        out_ids: Option<&mut [u32]>) -> Result<(), RmError> {
        assert!(xyz.len() % 3 == 0, "query_points: xyz holds {} floats, not a multiple of 3", xyz.len());
        let n = xyz.len() / 3;
        assert!(n <= u32::MAX as usize);
        assert!(out_dist.as_ref().map_or(true, |s| s.len() >= n), "query_points: out_dist is shorter than {} points", n);
        assert!(out_normal.as_ref().map_or(true, |s| s.len() >= 3 * n), "query_points: out_normal is shorter than {} points", n);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 2 * n), "query_points: out_ids is shorter than {} points", n);
        let dist = out_dist.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let normal = out_normal.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let ids = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_query_points(self.ctx, n as u32, xyz.as_ptr(), dist, normal, ids, 0, std::ptr::null_mut()) })
    }

    /// Casts `rays.len() / 6` rays (ox, oy, oz, dx, dy, dz; host memory) as the draw marches them: hit records (`out_hit`,
    /// eight per ray: t, position, normal, diffuse), (kind, steps, leaf, material) (`out_ids`, four per ray) and the colour
    /// (`out_rgb`, three per ray).  `None` skips that output.
    pub fn cast_rays(&self, rays: &[f32], out_hit: Option<&mut [f32]>, out_ids: Option<&mut [u32]>,
                     out_rgb: Option<&mut [f32]>) -> Result<(), RmError> {
        assert!(rays.len() % 6 == 0, "cast_rays: rays holds {} floats, not a multiple of 6", rays.len());
        let n = rays.len() / 6;
        assert!(n <= u32::MAX as usize);
        assert!(out_hit.as_ref().map_or(true, |s| s.len() >= 8 * n), "cast_rays: out_hit is shorter than {} rays", n);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 4 * n), "cast_rays: out_ids is shorter than {} rays", n);
        assert!(out_rgb.as_ref().map_or(true, |s| s.len() >= 3 * n), "cast_rays: out_rgb is shorter than {} rays", n);
        let hit = out_hit.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let ids = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let rgb = out_rgb.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_cast_rays(self.ctx, n as u32, rays.as_ptr(), hit, ids, rgb, 0, std::ptr::null_mut()) })
    }

    /// Every crossing of the level set along `rays.len() / 6` rays (host memory) over [T_MIN, T_MAX], in order (DESIGN.md
    /// section 18): `params` indexed by `RM_TRACE_*` (`trace_defaults()` is the starting point), `max_events` slots per ray
    /// (1..`RM_TRACE_MAX_EVENTS`), `flags` `RM_MESH_NORMALS` / `RM_MESH_IDS`.  Per slot: `out_events` (eight floats: t,
    /// position, normal, width) and `out_event_ids` (four words: kind, step, leaf, material); per ray: `out_counts` (four
    /// words: events found, steps, flags, events stored) and `out_spans` (four floats: final t, length inside, first and
    /// final distance).  `None` skips that output.
    pub fn trace_rays(&self, rays: &[f32], params: &[f32; RM_TRACE_PARAMS as usize], max_events: u32, flags: u32,
                      out_events: Option<&mut [f32]>, out_event_ids: Option<&mut [u32]>, out_counts: Option<&mut [u32]>,
                      out_spans: Option<&mut [f32]>) -> Result<(), RmError> {
        assert!(rays.len() % 6 == 0, "trace_rays: rays holds {} floats, not a multiple of 6", rays.len());
        let n = rays.len() / 6;
        assert!(n <= u32::MAX as usize);
        // (the library rejects a max_events outside 1..RM_TRACE_MAX_EVENTS before it writes; the slices are sized for the
        // value as given)
        let slots = n * max_events as usize;
        assert!(out_events.as_ref().map_or(true, |s| s.len() >= 8 * slots), "trace_rays: out_events is shorter than {} slots", slots);
        assert!(out_event_ids.as_ref().map_or(true, |s| s.len() >= 4 * slots), "trace_rays: out_event_ids is shorter than {} slots", slots);
        assert!(out_counts.as_ref().map_or(true, |s| s.len() >= 4 * n), "trace_rays: out_counts is shorter than {} rays", n);
        assert!(out_spans.as_ref().map_or(true, |s| s.len() >= 4 * n), "trace_rays: out_spans is shorter than {} rays", n);
        let events = out_events.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let event_ids = out_event_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let counts = out_counts.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let spans = out_spans.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe {
            rm_trace_rays(self.ctx, n as u32, rays.as_ptr(), params.as_ptr(), RM_TRACE_PARAMS as u32, max_events, flags, events,
                          event_ids, counts, spans, 0, std::ptr::null_mut())
        })
    }

    /// The rays the draw marches for AA sample `sample` (0..15, or `RM_SAMPLE_CENTER`) of the `w` x `h` pixels at (`x0`,
    /// `y0`) of a `width` x `height` frame, row-major, six floats each.
    pub fn camera_rays(&self, width: u32, height: u32, x0: u32, y0: u32, w: u32, h: u32, sample: u32,
                       out_rays: &mut [f32]) -> Result<(), RmError> {
        assert!(out_rays.len() >= (w as usize) * (h as usize) * 6, "camera_rays: out_rays is shorter than {} rays", w as usize * h as usize);
        self.check(unsafe { rm_camera_rays(self.ctx, width, height, x0, y0, w, h, sample, out_rays.as_mut_ptr(), 0, std::ptr::null_mut()) })
    }

    /// What lies under pixel (`x`, `y`) of a `width` x `height` frame: the ray through its centre, cast -- e.g. the node to
    /// select when the viewport is clicked (`hit.leaf` is the `cmd_count` the builder had before it pushed that primitive).
    pub fn pick(&self, width: u32, height: u32, x: u32, y: u32) -> Result<Hit, RmError> {
        let mut ray = [0.0f32; 6];
        self.camera_rays(width, height, x, y, 1, 1, RM_SAMPLE_CENTER as u32, &mut ray)?;
        let (mut rec, mut ids, mut rgb) = ([0.0f32; 8], [0u32; 4], [0.0f32; 3]);
        self.cast_rays(&ray, Some(&mut rec), Some(&mut ids), Some(&mut rgb))?;
        Ok(Hit { kind: ids[0] as c_int, steps: ids[1], leaf: ids[2], material: ids[3], t: rec[0], position: [rec[1], rec[2], rec[3]],
                 normal: [rec[4], rec[5], rec[6]], diffuse: rec[7], rgb })
    }

    /// `map_scene` at the `nx` x `ny` x `nz` lattice points `origin + (i, j, k) * step` (host memory, x fastest).
    pub fn sample_grid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32,
                       out_dist: &mut [f32]) -> Result<(), RmError> {
        let n = nx as usize * ny as usize * nz as usize;
        assert!(out_dist.len() >= n, "sample_grid: out_dist is shorter than {} points", n);
        self.check(unsafe {
            rm_sample_grid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, out_dist.as_mut_ptr(), 0, std::ptr::null_mut())
        })
    }

    /// Extracts the surface `map_scene = level` on the lattice into the context; `flags`: `RM_MESH_NORMALS`,
    /// `RM_MESH_IDS`.  Returns (vertices, triangles); `read_mesh` copies them out.
    pub fn extract_mesh(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32,
                        flags: u32) -> Result<(u64, u64), RmError> {
        let mut counts = [0u64; 2];
        self.mesh.set(None);  // a failed extraction may have released the previous mesh
        self.check(unsafe {
            rm_extract_mesh(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, flags, counts.as_mut_ptr())
        })?;
        self.mesh.set(Some((counts[0], counts[1])));
        Ok((counts[0], counts[1]))
    }

    /// `extract_mesh` brick by brick (`rm_extract_mesh_sparse`): the same mesh bit for bit, evaluated only where the
    /// surface can be, with no limit on the number of lattice points.  Fills `out_stats` (at least `RM_MESH_STATS`
    /// entries, indexed by `RM_MESH_STAT_*`) and returns (vertices, triangles); `read_mesh` copies the mesh out.
    pub fn extract_mesh_sparse(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, flags: u32,
                               out_stats: &mut [u64]) -> Result<(u64, u64), RmError> {
        assert!(out_stats.len() >= RM_MESH_STATS as usize, "extract_mesh_sparse: out_stats is shorter than RM_MESH_STATS entries");
        self.mesh.set(None);  // a failed extraction may have released the previous mesh
        self.check(unsafe {
            rm_extract_mesh_sparse(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, flags, out_stats.as_mut_ptr(),
                                   RM_MESH_STATS as u32)
        })?;
        let counts = (out_stats[RM_MESH_STAT_VERTICES as usize], out_stats[RM_MESH_STAT_TRIANGLES as usize]);
        self.mesh.set(Some(counts));
        Ok(counts)
    }

    /// The integer moments of the solid `map_scene < level` on the lattice (`rm_mass_moments`; 2..4096 points per axis): fills
    /// `out_moments` (at least `RM_MOMENTS` entries, indexed by `RM_MOMENT_*`) and `out_stats` (at least `RM_MASS_STATS`,
    /// indexed by `RM_MASS_STAT_*`).  Exact integers: every run gives the same words.  Leaves the context's mesh and slices alone.
    pub fn mass_moments(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, out_moments: &mut [u64],
                        out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_moments.len() >= RM_MOMENTS as usize, "mass_moments: out_moments is shorter than RM_MOMENTS entries");
        assert!(out_stats.len() >= RM_MASS_STATS as usize, "mass_moments: out_stats is shorter than RM_MASS_STATS entries");
        self.check(unsafe {
            rm_mass_moments(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, out_moments.as_mut_ptr(), RM_MOMENTS as u32,
                            out_stats.as_mut_ptr(), RM_MASS_STATS as u32)
        })
    }

    /// Bodies (6-adjacency), cavities (voids under 26-adjacency that do not reach the lattice's border) and tunnels of the solid
    /// `map_scene < level` on the lattice (`rm_label_solid`; 2..1024 points per axis, at most 2^28 in all): fills `out_counts`
    /// (at least `RM_TOPO_COUNTS` entries, indexed by `RM_TOPO_*`; EULER and TUNNELS are two's-complement `i64`) and `out_stats`
    /// (at least `RM_TOPO_STATS`, indexed by `RM_TOPO_STAT_*`).  Exact integers: every run gives the same words.  `read_topology`
    /// copies the rows and the label volume out.  Leaves the context's mesh and slices alone.
    pub fn label_solid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, out_counts: &mut [u64],
                       out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_TOPO_COUNTS as usize, "label_solid: out_counts is shorter than RM_TOPO_COUNTS entries");
        assert!(out_stats.len() >= RM_TOPO_STATS as usize, "label_solid: out_stats is shorter than RM_TOPO_STATS entries");
        self.topology.set(None);  // a failed call may have released the previous labelling
        self.check(unsafe {
            rm_label_solid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, out_counts.as_mut_ptr(), RM_TOPO_COUNTS as u32,
                           out_stats.as_mut_ptr(), RM_TOPO_STATS as u32)
        })?;
        self.topology.set(Some((out_counts[RM_TOPO_BODIES as usize], out_counts[RM_TOPO_CAVITIES as usize],
                                nx as u64 * ny as u64 * nz as u64)));
        Ok(())
    }

    /// `label_solid` of a caller's occupancy in host memory (`rm_label_occupancy`): one byte per point, x fastest, nonzero =
    /// inside.  The brick statistics are 0.
    pub fn label_occupancy(&self, nx: u32, ny: u32, nz: u32, occupancy: &[u8], out_counts: &mut [u64],
                           out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(occupancy.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "label_occupancy: occupancy is shorter than nx * ny * nz bytes");
        assert!(out_counts.len() >= RM_TOPO_COUNTS as usize, "label_occupancy: out_counts is shorter than RM_TOPO_COUNTS entries");
        assert!(out_stats.len() >= RM_TOPO_STATS as usize, "label_occupancy: out_stats is shorter than RM_TOPO_STATS entries");
        self.topology.set(None);  // a failed call may have released the previous labelling
        self.check(unsafe {
            rm_label_occupancy(self.ctx, nx, ny, nz, occupancy.as_ptr() as *const c_void, 0, std::ptr::null_mut(),
                               out_counts.as_mut_ptr(), RM_TOPO_COUNTS as u32, out_stats.as_mut_ptr(), RM_TOPO_STATS as u32)
        })?;
        self.topology.set(Some((out_counts[RM_TOPO_BODIES as usize], out_counts[RM_TOPO_CAVITIES as usize],
                                nx as u64 * ny as u64 * nz as u64)));
        Ok(())
    }

    /// The pair counts of the solid `map_scene < level` (class 1 inside, 0 outside) on the lattice (`rm_surface_solid`; 2..1024
    /// points per axis, at most 2^28 in all): fills `out_counts` (at least `RM_SURF_COUNTS` entries: the points per class at
    /// `RM_SURF_POINTS`, `PAIR[a][b][nu]` at `surf_pair(a, b, nu)`) and `out_stats` (at least `RM_SURF_STATS`, indexed by
    /// `RM_SURF_STAT_*`).  Exact integers: every run gives the same words.  `surface_measures` turns them into areas.  Nothing
    /// is retained, and no retained result of the context is touched.
    pub fn surface_solid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, out_counts: &mut [u64],
                         out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_SURF_COUNTS as usize, "surface_solid: out_counts is shorter than RM_SURF_COUNTS entries");
        assert!(out_stats.len() >= RM_SURF_STATS as usize, "surface_solid: out_stats is shorter than RM_SURF_STATS entries");
        self.check(unsafe {
            rm_surface_solid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, out_counts.as_mut_ptr(), RM_SURF_COUNTS as u32,
                             out_stats.as_mut_ptr(), RM_SURF_STATS as u32)
        })
    }

    /// `surface_solid` of a caller's classes in host memory (`rm_surface_classes`): one byte per point, x fastest, the class
    /// min(byte, 7) -- an occupancy, or the mask of `read_support`, `read_distance` or `read_islands` as it is.  The brick
    /// statistics are 0.
    pub fn surface_classes(&self, nx: u32, ny: u32, nz: u32, classes: &[u8], out_counts: &mut [u64],
                           out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(classes.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "surface_classes: classes is shorter than nx * ny * nz bytes");
        assert!(out_counts.len() >= RM_SURF_COUNTS as usize, "surface_classes: out_counts is shorter than RM_SURF_COUNTS entries");
        assert!(out_stats.len() >= RM_SURF_STATS as usize, "surface_classes: out_stats is shorter than RM_SURF_STATS entries");
        self.check(unsafe {
            rm_surface_classes(self.ctx, nx, ny, nz, classes.as_ptr() as *const c_void, 0, std::ptr::null_mut(),
                               out_counts.as_mut_ptr(), RM_SURF_COUNTS as u32, out_stats.as_mut_ptr(), RM_SURF_STATS as u32)
        })
    }

    /// The occupancy of a triangle mesh in host memory on the lattice (`rm_voxelize_mesh`; 2..1024 points per axis, at most 2^28
    /// in all), by the even-odd rule along +x: `xyz` holds three floats per vertex, `indices` three vertex indices per triangle,
    /// or `None` for a soup (every three vertices a triangle).  Fills `out_counts` (at least `RM_VOX_COUNTS` entries indexed by
    /// `RM_VOX_*`: triangles, rejected, edge-on, crossings, inside points, open rows) and `out_stats` (at least `RM_VOX_STATS`,
    /// indexed by `RM_VOX_STAT_*`).  Exact integers: every run and every order of the triangles gives the same words.  The
    /// occupancy stays in the context for `read_voxels`; no other retained result is touched.  Needs no program.
    pub fn voxelize_mesh(&self, xyz: &[f32], indices: Option<&[u32]>, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32,
                         out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(xyz.len() % 3 == 0 && xyz.len() / 3 <= u32::MAX as usize, "voxelize_mesh: xyz holds three floats per vertex");
        let n_vertices = (xyz.len() / 3) as u32;
        let n_triangles = match indices {
            Some(t) => {
                assert!(t.len() % 3 == 0 && t.len() / 3 <= u32::MAX as usize, "voxelize_mesh: indices holds three words per triangle");
                (t.len() / 3) as u32
            }
            None => {
                assert!(n_vertices % 3 == 0, "voxelize_mesh: a soup holds three vertices per triangle");
                n_vertices / 3
            }
        };
        assert!(out_counts.len() >= RM_VOX_COUNTS as usize, "voxelize_mesh: out_counts is shorter than RM_VOX_COUNTS entries");
        assert!(out_stats.len() >= RM_VOX_STATS as usize, "voxelize_mesh: out_stats is shorter than RM_VOX_STATS entries");
        self.voxels.set(None);  // a call that failed late may have released the previous occupancy
        self.check(unsafe {
            rm_voxelize_mesh(self.ctx, n_vertices, xyz.as_ptr(), n_triangles, indices.map_or(std::ptr::null(), |t| t.as_ptr()), 0,
                             std::ptr::null_mut(), origin.as_ptr(), step.as_ptr(), nx, ny, nz, out_counts.as_mut_ptr(),
                             RM_VOX_COUNTS as u32, out_stats.as_mut_ptr(), RM_VOX_STATS as u32)
        })?;
        self.voxels.set(Some(nx as u64 * ny as u64 * nz as u64));
        Ok(())
    }

    /// The lattice of class bytes that `draw_lattice` and `cast_lattice` show (`rm_set_lattice`): `classes`
    /// holds nx x ny x nz bytes in host memory, x fastest; 2..1024 points per axis, at most 2^28 in all.  Byte 0 is empty, a byte
    /// c > 0 the cube of its point with the albedo min(c, count - 1) of the material table as it stands at the draw.  Fills
    /// `out_counts` (at least `RM_LAT_COUNTS` entries indexed by `RM_LAT_*`: points, bricks) and `out_stats` (at least
    /// `RM_LAT_STATS`, indexed by `RM_LAT_STAT_*`).  The lattice stays in the context until the next `set_lattice`; no other
    /// retained result is touched.  Needs no program.
    pub fn set_lattice(&self, classes: &[u8], origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, out_counts: &mut [u64],
                       out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(classes.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "set_lattice: classes is shorter than the lattice");
        assert!(out_counts.len() >= RM_LAT_COUNTS as usize, "set_lattice: out_counts is shorter than RM_LAT_COUNTS entries");
        assert!(out_stats.len() >= RM_LAT_STATS as usize, "set_lattice: out_stats is shorter than RM_LAT_STATS entries");
        self.check(unsafe {
            rm_set_lattice(self.ctx, nx, ny, nz, classes.as_ptr() as *const c_void, 0, std::ptr::null_mut(), origin.as_ptr(),
                           step.as_ptr(), out_counts.as_mut_ptr(), RM_LAT_COUNTS as u32, out_stats.as_mut_ptr(), RM_LAT_STATS as u32)
        })
    }

    /// The image of the retained lattice through the uniforms' camera into a host RGBA32F image (top row first; with
    /// `RM_OPT_OUTPUT_FORMAT` at its default).  `window`: (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), the points lo <= i < hi are shown;
    /// `None`: the whole lattice.  `RM_ERR_ARG` before any `set_lattice` and for a bad window.
    pub fn draw_lattice(&self, width: u32, height: u32, window: Option<&[u32; 6]>, out_rgba: &mut [f32]) -> Result<(), RmError> {
        assert!(out_rgba.len() >= (width as usize) * (height as usize) * 4);
        let w = window.map_or(std::ptr::null(), |w| w.as_ptr());
        self.check(unsafe {
            rm_draw_lattice(self.ctx, width, height, 0, height, w, out_rgba.as_mut_ptr() as *mut c_void, 0, std::ptr::null_mut())
        })
    }

    /// Casts `rays.len() / 6` rays (host memory) through the retained lattice: hit records (`out_hit`, eight per ray, as
    /// `cast_rays`), (kind, linear point index, class byte, face) (`out_ids`, four per ray; `RM_NO_ID` unless a surface; face
    /// `RM_LAT_FACE_NONE` for an origin inside a cube) and the colour (`out_rgb`, three per ray).  `None` skips that output.
    pub fn cast_lattice(&self, rays: &[f32], window: Option<&[u32; 6]>, out_hit: Option<&mut [f32]>, out_ids: Option<&mut [u32]>,
                        out_rgb: Option<&mut [f32]>) -> Result<(), RmError> {
        assert!(rays.len() % 6 == 0, "cast_lattice: rays holds {} floats, not a multiple of 6", rays.len());
        let n = rays.len() / 6;
        assert!(n <= u32::MAX as usize);
        assert!(out_hit.as_ref().map_or(true, |s| s.len() >= 8 * n), "cast_lattice: out_hit is shorter than {} rays", n);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 4 * n), "cast_lattice: out_ids is shorter than {} rays", n);
        assert!(out_rgb.as_ref().map_or(true, |s| s.len() >= 3 * n), "cast_lattice: out_rgb is shorter than {} rays", n);
        let w = window.map_or(std::ptr::null(), |w| w.as_ptr());
        let hit = out_hit.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let ids = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let rgb = out_rgb.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_cast_lattice(self.ctx, n as u32, rays.as_ptr(), w, hit, ids, rgb, 0, std::ptr::null_mut()) })
    }

    /// The interface between two class sets of a lattice of class bytes as a welded, indexed triangle mesh (`rm_mesh_classes`;
    /// DESIGN.md section 29): `classes` holds nx x ny x nz bytes in host memory, x fastest, class = min(byte, 7); `mask_a` and
    /// `mask_b` are bit masks over the classes (non-empty, disjoint, no bit above 7).  The faces are the unit faces between a point
    /// of A and a 6-neighbour of B on the lattice padded with one layer of class 0, wound counter-clockwise seen from the B side.
    /// Fills `out_counts` (at least `RM_CMESH_COUNTS` entries indexed by `RM_CMESH_*`) and `out_stats` (at least `RM_CMESH_STATS`,
    /// indexed by `RM_CMESH_STAT_*`).  The mesh stays in the context for `read_class_mesh`; no other retained result is touched.
    /// Needs no program.
    pub fn mesh_classes(&self, classes: &[u8], origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, mask_a: u32, mask_b: u32,
                        out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(classes.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "mesh_classes: classes is shorter than the lattice");
        assert!(out_counts.len() >= RM_CMESH_COUNTS as usize, "mesh_classes: out_counts is shorter than RM_CMESH_COUNTS entries");
        assert!(out_stats.len() >= RM_CMESH_STATS as usize, "mesh_classes: out_stats is shorter than RM_CMESH_STATS entries");
        let rc = unsafe {
            rm_mesh_classes(self.ctx, nx, ny, nz, classes.as_ptr() as *const c_void, 0, std::ptr::null_mut(), origin.as_ptr(),
                            step.as_ptr(), mask_a, mask_b, out_counts.as_mut_ptr(), RM_CMESH_COUNTS as u32, out_stats.as_mut_ptr(),
                            RM_CMESH_STATS as u32)
        };
        if rc == RM_ERR_DEVICE {
            self.class_mesh.set(None);  // a call that failed late has released the previous mesh
        }
        self.check(rc)?;
        self.class_mesh.set(Some((out_counts[RM_CMESH_VERTICES as usize], out_counts[RM_CMESH_TRIANGLES as usize])));
        Ok(())
    }

    /// The mesh of the last successful `mesh_classes`, as a `ClassMesh`.  `RM_ERR_ARG` before any.
    pub fn read_class_mesh(&self) -> Result<ClassMesh, RmError> {
        let (v, t) = match self.class_mesh.get() {
            Some(vt) => (vt.0 as usize, vt.1 as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_class_mesh: no lattice has been meshed".to_string() }),
        };
        let mut m = ClassMesh { vertices: vec![0.0; 3 * v], triangles: vec![0; 3 * t], ids: vec![0; 2 * t] };
        self.check(unsafe {
            rm_read_class_mesh(self.ctx, m.vertices.as_mut_ptr(), m.triangles.as_mut_ptr(), m.ids.as_mut_ptr(), 0, std::ptr::null_mut())
        })?;
        Ok(m)
    }

    /// The occupancy of the last successful `voxelize_mesh`: one byte per lattice point, 0 or 1, x fastest -- what
    /// `label_occupancy`, `distance_occupancy`, `support_occupancy`, `islands_occupancy` and `surface_classes` take.
    /// `RM_ERR_ARG` before any voxelisation.
    pub fn read_voxels(&self, out_occupancy: &mut [u8]) -> Result<(), RmError> {
        let n = match self.voxels.get() {
            Some(n) => n as usize,
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_voxels: no mesh has been voxelised".to_string() }),
        };
        assert!(out_occupancy.len() >= n, "read_voxels: out_occupancy is shorter than {} points", n);
        self.check(unsafe { rm_read_voxels(self.ctx, out_occupancy.as_mut_ptr() as *mut c_void, 0, std::ptr::null_mut()) })
    }

    /// The result of the last successful labelling call: the bodies' rows and the cavities' rows (`RM_MOMENTS` words each, in
    /// body and cavity order) and the label volume (one word per lattice point: a body's number, `RM_TOPO_CAVITY_BIT` | a
    /// cavity's number, or `RM_TOPO_EXTERIOR`).  `None` skips that output.  `RM_ERR_ARG` before any labelling.
    pub fn read_topology(&self, out_body_moments: Option<&mut [u64]>, out_cavity_moments: Option<&mut [u64]>,
                         out_labels: Option<&mut [u32]>) -> Result<(), RmError> {
        let (b, c, n) = match self.topology.get() {
            Some((b, c, n)) => (b as usize, c as usize, n as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_topology: nothing has been labelled".to_string() }),
        };
        let m = RM_MOMENTS as usize;
        assert!(out_body_moments.as_ref().map_or(true, |s| s.len() >= m * b), "read_topology: out_body_moments is shorter than {} rows", b);
        assert!(out_cavity_moments.as_ref().map_or(true, |s| s.len() >= m * c), "read_topology: out_cavity_moments is shorter than {} rows", c);
        assert!(out_labels.as_ref().map_or(true, |s| s.len() >= n), "read_topology: out_labels is shorter than {} points", n);
        let pb = out_body_moments.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pc = out_cavity_moments.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pl = out_labels.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_topology(self.ctx, pb, pc, pl, 0, std::ptr::null_mut()) })
    }

    /// The exact squared Euclidean distance transform of the solid `map_scene < level` on the lattice (`rm_distance_solid`;
    /// 2..1024 points per axis, at most 2^28 in all), in index units: fills `out_counts` (at least `RM_DIST_COUNTS` entries,
    /// indexed by `RM_DIST_*`: the inside points, the largest inside and outside squared distance and where) and `out_stats`
    /// (at least `RM_DIST_STATS`, indexed by `RM_DIST_STAT_*`).  Exact integers: every run gives the same words.
    /// `read_distance` copies the distance volume out.  Leaves the context's mesh, slices and labelling alone.
    pub fn distance_solid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, out_counts: &mut [u64],
                          out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_DIST_COUNTS as usize, "distance_solid: out_counts is shorter than RM_DIST_COUNTS entries");
        assert!(out_stats.len() >= RM_DIST_STATS as usize, "distance_solid: out_stats is shorter than RM_DIST_STATS entries");
        self.distance.set(None);  // a failed call may have released the previous volume
        self.check(unsafe {
            rm_distance_solid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, out_counts.as_mut_ptr(), RM_DIST_COUNTS as u32,
                              out_stats.as_mut_ptr(), RM_DIST_STATS as u32)
        })?;
        self.distance.set(Some((nx as u64 * ny as u64 * nz as u64, false)));
        Ok(())
    }

    /// `distance_solid` of a caller's occupancy in host memory (`rm_distance_occupancy`): one byte per point, x fastest,
    /// nonzero = inside.  The brick statistics are 0.
    pub fn distance_occupancy(&self, nx: u32, ny: u32, nz: u32, occupancy: &[u8], out_counts: &mut [u64],
                              out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(occupancy.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "distance_occupancy: occupancy is shorter than nx * ny * nz bytes");
        assert!(out_counts.len() >= RM_DIST_COUNTS as usize, "distance_occupancy: out_counts is shorter than RM_DIST_COUNTS entries");
        assert!(out_stats.len() >= RM_DIST_STATS as usize, "distance_occupancy: out_stats is shorter than RM_DIST_STATS entries");
        self.distance.set(None);  // a failed call may have released the previous volume
        self.check(unsafe {
            rm_distance_occupancy(self.ctx, nx, ny, nz, occupancy.as_ptr() as *const c_void, 0, std::ptr::null_mut(),
                                  out_counts.as_mut_ptr(), RM_DIST_COUNTS as u32, out_stats.as_mut_ptr(), RM_DIST_STATS as u32)
        })?;
        self.distance.set(Some((nx as u64 * ny as u64 * nz as u64, false)));
        Ok(())
    }

    /// Thin walls and narrow gaps of the last distance volume (`rm_distance_features`): the inside points that no ball of
    /// squared radius `r2_wall` (index units) inside the solid covers, and the outside points that none of squared radius
    /// `r2_gap` centred on an outside lattice point covers; `None` skips that half.  Fills `out_counts` (at least
    /// `RM_DIST_FEATURE_COUNTS` entries, indexed by `RM_DIST_CORE`, `THIN`, `GAP_CORE`, `NARROW`); `read_distance` copies the
    /// mask out.  `RM_ERR_ARG` before any distance call, `RM_ERR_RANGE` for a squared radius of 2^22 or more.
    pub fn distance_features(&self, r2_wall: Option<u32>, r2_gap: Option<u32>, out_counts: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_DIST_FEATURE_COUNTS as usize, "distance_features: out_counts is shorter than RM_DIST_FEATURE_COUNTS entries");
        assert!(r2_wall != Some(RM_DIST_SKIP) && r2_gap != Some(RM_DIST_SKIP), "distance_features: None skips a half");
        if let Some((n, _)) = self.distance.get() {
            self.distance.set(Some((n, false)));  // a failed call may have released the previous mask
        }
        self.check(unsafe {
            rm_distance_features(self.ctx, r2_wall.unwrap_or(RM_DIST_SKIP), r2_gap.unwrap_or(RM_DIST_SKIP), out_counts.as_mut_ptr(),
                                 RM_DIST_FEATURE_COUNTS as u32)
        })?;
        if let Some((n, _)) = self.distance.get() {
            self.distance.set(Some((n, true)));
        }
        Ok(())
    }

    /// The last distance volume (one word per lattice point: the squared distance, `RM_DIST_INSIDE_BIT` ORed in for an inside
    /// point) and the last feature mask (one byte per point: 0 outside, 1 inside, 2 thin, 3 narrow).  `None` skips that output.
    /// `RM_ERR_ARG` before any distance call, and for a mask before any features call on the last volume.
    pub fn read_distance(&self, out_d2: Option<&mut [u32]>, out_mask: Option<&mut [u8]>) -> Result<(), RmError> {
        let (n, has_mask) = match self.distance.get() {
            Some((n, m)) => (n as usize, m),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_distance: no distance volume has been computed".to_string() }),
        };
        if out_mask.is_some() && !has_mask {
            return Err(RmError { status: RM_ERR_ARG, message: "read_distance: no features call has made a mask of this volume".to_string() });
        }
        assert!(out_d2.as_ref().map_or(true, |s| s.len() >= n), "read_distance: out_d2 is shorter than {} points", n);
        assert!(out_mask.as_ref().map_or(true, |s| s.len() >= n), "read_distance: out_mask is shorter than {} points", n);
        let pd = out_d2.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pm = out_mask.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr() as *mut c_void);
        self.check(unsafe { rm_read_distance(self.ctx, pd, pm, 0, std::ptr::null_mut()) })
    }

    /// Overhangs and supports of the solid `map_scene < level` on the lattice (`rm_support_solid`; 2..1024 points per axis, at
    /// most 2^28 in all) for the build direction `up` (`RM_UP_*`), the squared reach `r2` (index units, 0..255) and the plate's
    /// height (`None`: the lowest layer that holds an inside point): fills `out_counts` (at least `RM_SUP_COUNTS` entries,
    /// indexed by `RM_SUP_*`) and `out_stats` (at least `RM_SUP_STATS`, indexed by `RM_SUP_STAT_*`).  Exact integers: every run
    /// gives the same words.  `read_support` copies mask and profile out.  Leaves the context's mesh, slices, labelling and
    /// distance volume alone.
    pub fn support_solid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, up: c_int, r2: u32,
                         plate: Option<u32>, out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_SUP_COUNTS as usize, "support_solid: out_counts is shorter than RM_SUP_COUNTS entries");
        assert!(out_stats.len() >= RM_SUP_STATS as usize, "support_solid: out_stats is shorter than RM_SUP_STATS entries");
        assert!(plate != Some(RM_SUPPORT_PLATE_AUTO), "support_solid: None is the automatic plate");
        self.support.set(None);  // a failed call may have released the previous result
        self.check(unsafe {
            rm_support_solid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, up as u32, r2, plate.unwrap_or(RM_SUPPORT_PLATE_AUTO),
                             out_counts.as_mut_ptr(), RM_SUP_COUNTS as u32, out_stats.as_mut_ptr(), RM_SUP_STATS as u32)
        })?;
        self.support.set(Some((nx as u64 * ny as u64 * nz as u64, [nx, ny, nz][(up >> 1) as usize])));
        Ok(())
    }

    /// `support_solid` of a caller's occupancy in host memory (`rm_support_occupancy`): one byte per point, x fastest, nonzero =
    /// inside.  The brick statistics are 0.
    pub fn support_occupancy(&self, nx: u32, ny: u32, nz: u32, occupancy: &[u8], up: c_int, r2: u32, plate: Option<u32>,
                             out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(occupancy.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "support_occupancy: occupancy is shorter than nx * ny * nz bytes");
        assert!(out_counts.len() >= RM_SUP_COUNTS as usize, "support_occupancy: out_counts is shorter than RM_SUP_COUNTS entries");
        assert!(out_stats.len() >= RM_SUP_STATS as usize, "support_occupancy: out_stats is shorter than RM_SUP_STATS entries");
        assert!(plate != Some(RM_SUPPORT_PLATE_AUTO), "support_occupancy: None is the automatic plate");
        self.support.set(None);  // a failed call may have released the previous result
        self.check(unsafe {
            rm_support_occupancy(self.ctx, nx, ny, nz, occupancy.as_ptr() as *const c_void, 0, std::ptr::null_mut(), up as u32, r2,
                                 plate.unwrap_or(RM_SUPPORT_PLATE_AUTO), out_counts.as_mut_ptr(), RM_SUP_COUNTS as u32,
                                 out_stats.as_mut_ptr(), RM_SUP_STATS as u32)
        })?;
        self.support.set(Some((nx as u64 * ny as u64 * nz as u64, [nx, ny, nz][(up >> 1) as usize])));
        Ok(())
    }

    /// The mask of the last support call (one byte per lattice point: 0 outside, 1 inside, 2 overhang, 3 support on the plate,
    /// 4 support on the part) and its profile (four words per layer along the build direction, height 0 first: inside, overhang,
    /// support on the plate, support on the part).  `None` skips that output.  `RM_ERR_ARG` before any support call.
    pub fn read_support(&self, out_mask: Option<&mut [u8]>, out_profile: Option<&mut [u32]>) -> Result<(), RmError> {
        let (n, layers) = match self.support.get() {
            Some((n, l)) => (n as usize, l as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_support: no support call has been made".to_string() }),
        };
        assert!(out_mask.as_ref().map_or(true, |s| s.len() >= n), "read_support: out_mask is shorter than {} points", n);
        assert!(out_profile.as_ref().map_or(true, |s| s.len() >= 4 * layers), "read_support: out_profile is shorter than {} words", 4 * layers);
        let pm = out_mask.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr() as *mut c_void);
        let pp = out_profile.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_support(self.ctx, pm, pp, 0, std::ptr::null_mut()) })
    }

    /// Layer regions and islands of the solid `map_scene < level` on the lattice (`rm_islands_solid`; lattice, `up`, `r2` and
    /// `plate` as `support_solid` takes them): fills `out_counts` (at least `RM_ISL_COUNTS` entries, indexed by `RM_ISL_*`) and
    /// `out_stats` (at least `RM_ISL_STATS`, indexed by `RM_ISL_STAT_*`).  Exact integers: every run gives the same words.
    /// `read_islands` copies the region table, the labels, the mask and the profile out.  Leaves the context's mesh, slices,
    /// labelling, distance volume and support result alone.
    pub fn islands_solid(&self, origin: [f32; 3], step: [f32; 3], nx: u32, ny: u32, nz: u32, level: f32, up: c_int, r2: u32,
                         plate: Option<u32>, out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(out_counts.len() >= RM_ISL_COUNTS as usize, "islands_solid: out_counts is shorter than RM_ISL_COUNTS entries");
        assert!(out_stats.len() >= RM_ISL_STATS as usize, "islands_solid: out_stats is shorter than RM_ISL_STATS entries");
        assert!(plate != Some(RM_SUPPORT_PLATE_AUTO), "islands_solid: None is the automatic plate");
        self.islands.set(None);  // a failed call may have released the previous result
        self.check(unsafe {
            rm_islands_solid(self.ctx, origin.as_ptr(), step.as_ptr(), nx, ny, nz, level, up as u32, r2, plate.unwrap_or(RM_SUPPORT_PLATE_AUTO),
                             out_counts.as_mut_ptr(), RM_ISL_COUNTS as u32, out_stats.as_mut_ptr(), RM_ISL_STATS as u32)
        })?;
        self.islands.set(Some((nx as u64 * ny as u64 * nz as u64, [nx, ny, nz][(up >> 1) as usize], out_counts[RM_ISL_REGIONS as usize])));
        Ok(())
    }

    /// `islands_solid` of a caller's occupancy in host memory (`rm_islands_occupancy`): one byte per point, x fastest, nonzero =
    /// inside.
    pub fn islands_occupancy(&self, nx: u32, ny: u32, nz: u32, occupancy: &[u8], up: c_int, r2: u32, plate: Option<u32>,
                             out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(), RmError> {
        assert!(occupancy.len() as u64 >= nx as u64 * ny as u64 * nz as u64, "islands_occupancy: occupancy is shorter than nx * ny * nz bytes");
        assert!(out_counts.len() >= RM_ISL_COUNTS as usize, "islands_occupancy: out_counts is shorter than RM_ISL_COUNTS entries");
        assert!(out_stats.len() >= RM_ISL_STATS as usize, "islands_occupancy: out_stats is shorter than RM_ISL_STATS entries");
        assert!(plate != Some(RM_SUPPORT_PLATE_AUTO), "islands_occupancy: None is the automatic plate");
        self.islands.set(None);  // a failed call may have released the previous result
        self.check(unsafe {
            rm_islands_occupancy(self.ctx, nx, ny, nz, occupancy.as_ptr() as *const c_void, 0, std::ptr::null_mut(), up as u32, r2,
                                 plate.unwrap_or(RM_SUPPORT_PLATE_AUTO), out_counts.as_mut_ptr(), RM_ISL_COUNTS as u32,
                                 out_stats.as_mut_ptr(), RM_ISL_STATS as u32)
        })?;
        self.islands.set(Some((nx as u64 * ny as u64 * nz as u64, [nx, ny, nz][(up >> 1) as usize], out_counts[RM_ISL_REGIONS as usize])));
        Ok(())
    }

    /// The result of the last islands call: the region table (`RM_ISL_ROW_WORDS` words per region, row r - 1 for region r), the
    /// label volume (one word per lattice point), the mask (one byte per point: 0 outside, 1 inside, 2 inside and in an island)
    /// and the profile (four words per layer along the build direction, height 0 first: inside points, regions, islands, island
    /// points).  `None` skips that output.  `RM_ERR_ARG` before any islands call.
    pub fn read_islands(&self, out_rows: Option<&mut [u32]>, out_labels: Option<&mut [u32]>, out_mask: Option<&mut [u8]>,
                        out_profile: Option<&mut [u32]>) -> Result<(), RmError> {
        let (n, layers, regions) = match self.islands.get() {
            Some((n, l, r)) => (n as usize, l as usize, r as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_islands: no islands call has been made".to_string() }),
        };
        let words = RM_ISL_ROW_WORDS as usize;
        assert!(out_rows.as_ref().map_or(true, |s| s.len() >= words * regions), "read_islands: out_rows is shorter than {} rows", regions);
        assert!(out_labels.as_ref().map_or(true, |s| s.len() >= n), "read_islands: out_labels is shorter than {} points", n);
        assert!(out_mask.as_ref().map_or(true, |s| s.len() >= n), "read_islands: out_mask is shorter than {} points", n);
        assert!(out_profile.as_ref().map_or(true, |s| s.len() >= 4 * layers), "read_islands: out_profile is shorter than {} words", 4 * layers);
        let capacity = out_rows.as_ref().map_or(0, |s| (s.len() / words) as u64);
        let pr = out_rows.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pl = out_labels.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pm = out_mask.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr() as *mut c_void);
        let pp = out_profile.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_islands(self.ctx, pr, capacity, pl, pm, pp, 0, std::ptr::null_mut()) })
    }

    /// For every region of a region table the number of the island or base region it grows from, following `BELOW_MIN`
    /// downwards: one pass, because the rows are sorted by layer.
    pub fn island_roots(rows: &[u32]) -> Vec<u32> {
        let words = RM_ISL_ROW_WORDS as usize;
        let mut root = vec![0u32; rows.len() / words + 1];
        for r in 1..root.len() {
            let below = rows[(r - 1) * words + RM_ISL_ROW_BELOW_MIN as usize] as usize;
            root[r] = if below != 0 { root[below] } else { r as u32 };
        }
        root.remove(0);
        root
    }

    /// The mesh of the last successful `extract_mesh` (of the (vertices, triangles) it returned): positions (three per
    /// vertex), vertex indices (three per triangle), normals (three per vertex) and (leaf, material) (two per vertex).
    /// `None` skips that output.  `RM_ERR_ARG` before any extraction, or for normals / ids it did not compute.
    pub fn read_mesh(&self, out_vertices: Option<&mut [f32]>, out_triangles: Option<&mut [u32]>,
                     out_normals: Option<&mut [f32]>, out_ids: Option<&mut [u32]>) -> Result<(), RmError> {
        let (v, t) = match self.mesh.get() {
            Some((v, t)) => (v as usize, t as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_mesh: no mesh has been extracted".to_string() }),
        };
        assert!(out_vertices.as_ref().map_or(true, |s| s.len() >= 3 * v), "read_mesh: out_vertices is shorter than {} vertices", v);
        assert!(out_triangles.as_ref().map_or(true, |s| s.len() >= 3 * t), "read_mesh: out_triangles is shorter than {} triangles", t);
        assert!(out_normals.as_ref().map_or(true, |s| s.len() >= 3 * v), "read_mesh: out_normals is shorter than {} vertices", v);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 2 * v), "read_mesh: out_ids is shorter than {} vertices", v);
        let pv = out_vertices.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pt = out_triangles.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pn = out_normals.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pi = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_mesh(self.ctx, pv, pt, pn, pi, 0, std::ptr::null_mut()) })
    }

    /// The outlines of the solid `map_scene < level` in the planes `heights` across `axis` (0, 1, 2), as ordered contours
    /// (`rm_slice_contours`): point (i, j) of a layer lies at `origin_uv + (i, j) * step_uv` on the in-plane axes
    /// `(axis + 1) % 3` and `(axis + 2) % 3`.  `flags`: `RM_MESH_NORMALS`, `RM_MESH_IDS`.  Returns (points, contours);
    /// `read_slices` copies them out.
    pub fn slice_contours(&self, axis: u32, origin_uv: [f32; 2], step_uv: [f32; 2], nu: u32, nv: u32, heights: &[f32], level: f32,
                          flags: u32) -> Result<(u64, u64), RmError> {
        assert!(heights.len() <= u32::MAX as usize, "slice_contours: too many heights");
        let mut counts = [0u64; RM_SLICE_COUNTS as usize];
        self.slices.set(None);  // a failed call may have released the previous slices
        self.hatch.set(None);  // ... and a hatch is of the slices it was made of
        self.check(unsafe {
            rm_slice_contours(self.ctx, axis, origin_uv.as_ptr(), step_uv.as_ptr(), nu, nv, heights.as_ptr(), heights.len() as u32,
                              level, flags, counts.as_mut_ptr(), RM_SLICE_COUNTS as u32)
        })?;
        let (p, c) = (counts[RM_SLICE_POINTS as usize], counts[RM_SLICE_CONTOURS as usize]);
        self.slices.set(Some((p, c, heights.len() as u32)));
        Ok((p, c))
    }

    /// The outlines of an indexed triangle mesh in host memory in the planes `heights` (strictly increasing) across `axis`
    /// (`rm_slice_mesh`): `xyz` three floats per vertex, `triangles` three vertex indices per triangle; `origin` and `step` are the
    /// resolution frame the vertices are snapped in (1 / 64 of a step, as `voxelize_mesh` snaps them).  Fills `out_counts` (at least
    /// `RM_MSLICE_COUNTS` entries indexed by `RM_MSLICE_*`) and `out_stats` (at least `RM_MSLICE_STATS`, indexed by
    /// `RM_MSLICE_STAT_*`).  Returns (points, contours); `read_slices` copies points, contours and layer_first out (normals and ids
    /// are `RM_ERR_ARG`).  A call that fails leaves the previous slices readable.
    pub fn slice_mesh(&self, xyz: &[f32], triangles: &[u32], origin: [f32; 3], step: [f32; 3], axis: u32, heights: &[f32],
                      out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<(u64, u64), RmError> {
        assert!(xyz.len() % 3 == 0 && xyz.len() / 3 <= u32::MAX as usize, "slice_mesh: xyz holds three floats per vertex");
        assert!(triangles.len() % 3 == 0 && triangles.len() / 3 <= u32::MAX as usize, "slice_mesh: triangles holds three indices per triangle");
        assert!(heights.len() <= u32::MAX as usize, "slice_mesh: too many heights");
        assert!(out_counts.len() >= RM_MSLICE_COUNTS as usize, "slice_mesh: out_counts is shorter than RM_MSLICE_COUNTS entries");
        assert!(out_stats.len() >= RM_MSLICE_STATS as usize, "slice_mesh: out_stats is shorter than RM_MSLICE_STATS entries");
        self.check(unsafe {
            rm_slice_mesh(self.ctx, xyz.as_ptr(), (xyz.len() / 3) as u32, triangles.as_ptr(), (triangles.len() / 3) as u32, 0,
                          std::ptr::null_mut(), origin.as_ptr(), step.as_ptr(), axis, heights.as_ptr(), heights.len() as u32, 0,
                          out_counts.as_mut_ptr(), RM_MSLICE_COUNTS as u32, out_stats.as_mut_ptr(), RM_MSLICE_STATS as u32)
        })?;
        let (p, c) = (out_counts[RM_MSLICE_POINTS as usize], out_counts[RM_MSLICE_CONTOURS as usize]);
        self.slices.set(Some((p, c, heights.len() as u32)));
        self.hatch.set(None);
        Ok((p, c))
    }

    /// The slices of the last successful `slice_contours`: points (world x, y, z, three per point, in contour order),
    /// contours (first point, point count, layer, closed; four per contour), layer_first (layers + 1 entries), normals
    /// (three per point) and (leaf, material) (two per point).  `None` skips that output.  `RM_ERR_ARG` before any
    /// `slice_contours`, or for normals / ids it did not compute.
    pub fn read_slices(&self, out_points: Option<&mut [f32]>, out_contours: Option<&mut [u32]>,
                       out_layer_first: Option<&mut [u32]>, out_normals: Option<&mut [f32]>,
                       out_ids: Option<&mut [u32]>) -> Result<(), RmError> {
        let (p, c, l) = match self.slices.get() {
            Some((p, c, l)) => (p as usize, c as usize, l as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_slices: nothing has been sliced".to_string() }),
        };
        assert!(out_points.as_ref().map_or(true, |s| s.len() >= 3 * p), "read_slices: out_points is shorter than {} points", p);
        assert!(out_contours.as_ref().map_or(true, |s| s.len() >= 4 * c), "read_slices: out_contours is shorter than {} contours", c);
        assert!(out_layer_first.as_ref().map_or(true, |s| s.len() >= l + 1), "read_slices: out_layer_first is shorter than {} entries", l + 1);
        assert!(out_normals.as_ref().map_or(true, |s| s.len() >= 3 * p), "read_slices: out_normals is shorter than {} points", p);
        assert!(out_ids.as_ref().map_or(true, |s| s.len() >= 2 * p), "read_slices: out_ids is shorter than {} points", p);
        let pp = out_points.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pc = out_contours.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pl = out_layer_first.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pn = out_normals.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pi = out_ids.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_slices(self.ctx, pp, pc, pl, pn, pi, 0, std::ptr::null_mut()) })
    }

    /// The retained slices filled with parallel lines under the even-odd rule (`rm_hatch_slices`): `lines` holds
    /// (dx, dy, offset, spacing) per layer of the slices, `n_lines` lines per layer; `flags`: `RM_HATCH_ZIGZAG` or 0.  Fills
    /// `out_counts` (at least `RM_HATCH_COUNTS` entries indexed by `RM_HATCH_*`) and `out_stats` (at least `RM_HATCH_STATS`).
    /// Returns the number of hatch segments; `read_hatch` copies them out.  A call that fails leaves the previous hatch readable.
    pub fn hatch_slices(&self, lines: &[f32], n_lines: u32, flags: u32, out_counts: &mut [u64], out_stats: &mut [u64]) -> Result<u64, RmError> {
        assert!(lines.len() % 4 == 0 && lines.len() / 4 <= u32::MAX as usize, "hatch_slices: lines holds four floats per layer");
        assert!(out_counts.len() >= RM_HATCH_COUNTS as usize, "hatch_slices: out_counts is shorter than RM_HATCH_COUNTS entries");
        assert!(out_stats.len() >= RM_HATCH_STATS as usize, "hatch_slices: out_stats is shorter than RM_HATCH_STATS entries");
        self.check(unsafe {
            rm_hatch_slices(self.ctx, lines.as_ptr(), (lines.len() / 4) as u32, n_lines, flags, out_counts.as_mut_ptr(),
                            RM_HATCH_COUNTS as u32, out_stats.as_mut_ptr(), RM_HATCH_STATS as u32)
        })?;
        let h = out_counts[RM_HATCH_SEGMENTS as usize];
        self.hatch.set(Some((h, (lines.len() / 4) as u32)));
        Ok(h)
    }

    /// The hatch of the last successful `hatch_slices`: segments (u, v of the first end, u, v of the second; four per segment),
    /// line (layer * n_lines + j; one per segment), layer_first (layers + 1 entries).  `None` skips that output.  `RM_ERR_ARG`
    /// without a hatch of the current slices.
    pub fn read_hatch(&self, out_segments: Option<&mut [f32]>, out_line: Option<&mut [u32]>,
                      out_layer_first: Option<&mut [u32]>) -> Result<(), RmError> {
        let (h, l) = match self.hatch.get() {
            Some((h, l)) => (h as usize, l as usize),
            None => return Err(RmError { status: RM_ERR_ARG, message: "read_hatch: no hatch of the current slices".to_string() }),
        };
        assert!(out_segments.as_ref().map_or(true, |s| s.len() >= 4 * h), "read_hatch: out_segments is shorter than {} segments", h);
        assert!(out_line.as_ref().map_or(true, |s| s.len() >= h), "read_hatch: out_line is shorter than {} segments", h);
        assert!(out_layer_first.as_ref().map_or(true, |s| s.len() >= l + 1), "read_hatch: out_layer_first is shorter than {} entries", l + 1);
        let ps = out_segments.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pl = out_line.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        let pf = out_layer_first.map_or(std::ptr::null_mut(), |s| s.as_mut_ptr());
        self.check(unsafe { rm_read_hatch(self.ctx, ps, pl, pf, 0, std::ptr::null_mut()) })
    }
}

/// One cast ray (`RayMarchingResources::pick`): `kind` is `RM_HIT_NONE`, `RM_HIT_SURFACE` or `RM_HIT_FLOOR`; `leaf` and
/// `material` are `RM_NO_ID` unless a surface was hit.
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct Hit {
    pub kind: c_int,
    pub steps: u32,
    pub leaf: u32,
    pub material: u32,
    pub t: f32,
    pub position: [f32; 3],
    pub normal: [f32; 3],
    pub diffuse: f32,
    pub rgb: [f32; 3],
}

/// A class mesh (`RayMarchingResources::read_class_mesh`): `vertices` three floats per vertex, `triangles` three vertex indices
/// per triangle, `ids` two words per triangle -- class_A | class_B << 8 | face << 16 (face = 2 axis + (normal positive)), and
/// the linear index of the face's A-side point (`RM_NO_ID` for padding).
#[derive(Debug, Clone, PartialEq)]
pub struct ClassMesh {
    pub vertices: Vec<f32>,
    pub triangles: Vec<u32>,
    pub ids: Vec<u32>,
}

/// Output rows of strips `first`, `first + stride`, ... (`strip_rows` rows each; the frame's last strip may be ragged) of an
/// image `height` rows high: what `rm_draw_strips` renders for one GPU.  0 for arguments the library rejects.
pub fn strip_row_count(height: u32, strip_rows: u32, first: u32, stride: u32) -> u32 {
    if strip_rows == 0 || stride == 0 || first >= stride {
        return 0;
    }
    let n_strips = (height + strip_rows - 1) / strip_rows;
    let mut rows = 0u32;
    let mut s = first;
    while s < n_strips {
        let r0 = s * strip_rows;
        rows += (height - r0).min(strip_rows);
        s += stride;
    }
    rows
}

impl Drop for RayMarchingResources {
    fn drop(&mut self) {
        unsafe { rm_destroy(self.ctx) }
    }
}

// ---------------------------------------------------------------------------------------------
// What `impl CallbackTrait for RayMarchingCallback` (renderer.rs:195-256) becomes.  `Uniforms`,
// `AsShaderBytes`, `CSGCommandBufferBuilder`, `BuildCommands`, `CSGNode` and `Camera` are the
// reference's own items, unchanged:
//
//     fn prepare(&self, resources: &RayMarchingResources) -> Result<(), RmError> {
//         let projection = Perspective3::new(self.viewport[0] / self.viewport[1], FRAC_PI_4, 1.0, 10000.0);
//         let uniforms = Uniforms {
//             viewport_extent: Vector2::new(self.viewport[0], self.viewport[1]),
//             inv_proj: projection.inverse(),
//             inv_view: self.camera.view().inverse().to_homogeneous(),
//         };
//         resources.write_buffer(RM_BUF_UNIFORMS, 0, &uniforms.as_shader_bytes())?;       // renderer.rs:213-222
//         let mut builder = CSGCommandBufferBuilder::new();
//         if let Some(csg_node) = &self.csg_node { csg_node.build_commands(&mut builder); }
//         resources.write_buffer(RM_BUF_COMMANDS, 0, bytemuck::cast_slice(&[builder.cmd_count]))?;  // :230-234
//         resources.write_buffer(RM_BUF_COMMANDS, 4, bytemuck::cast_slice(&builder.buffer))         // :235-239
//     }
//     fn paint(&self, resources: &RayMarchingResources, out: &mut [f32]) -> Result<(), RmError> {
//         resources.draw(self.viewport[0] as u32, self.viewport[1] as u32, out)           // renderer.rs:252-254
//     }
// ---------------------------------------------------------------------------------------------

#[cfg(test)]
mod tests {
    use super::*;

    #[test]
    fn blob_layouts_match_the_reference() {
        assert_eq!(std::mem::size_of::<rm_uniforms>(), 144); // renderer.rs:29-34 through encase
        assert_eq!(std::mem::size_of::<rm_limits>(), 12); // renderer.rs:36-41
    }

    #[test]
    fn error_is_a_std_error() {
        let e: Box<dyn std::error::Error> = Box::new(RmError { status: RM_ERR_ARG, message: "x".into() });
        assert!(e.to_string().contains("-11"));
    }
}
