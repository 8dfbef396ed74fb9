"""ctypes bindings of the two native libraries.  There is NO fallback: if librm_hip.so is
missing or no GPU is visible, the render path raises (the product never runs on the CPU)."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.environ.get("RM_HIP_SO") or os.path.join(PKG, "librm_hip.so")   # RM_HIP_SO: A/B builds
HOST_SO = os.path.join(PKG, "librm_host.so")


class RmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("rm status %d: %s" % (status, message))
        self.status = status


class Uniforms(C.Structure):
    """rm_uniforms, 144 bytes (include/rm_abi.h)."""
    _fields_ = [("viewport_extent", C.c_float * 2), ("_pad", C.c_float * 2),
                ("inv_proj", C.c_float * 16), ("inv_view", C.c_float * 16)]


class Limits(C.Structure):
    """rm_limits, 12 bytes."""
    _fields_ = [("min_dist", C.c_float), ("max_dist", C.c_float), ("max_iter", C.c_uint32)]


# status codes (include/rm_abi.h enum rm_status)
RM_OK, RM_ERR_NULL, RM_ERR_TRUNCATED, RM_ERR_STACK_UNDERFLOW, RM_ERR_STACK_OVERFLOW = 0, -1, -2, -3, -4
RM_ERR_EMPTY_RESULT, RM_ERR_OPCODE, RM_ERR_TOO_LARGE, RM_ERR_RANGE, RM_ERR_DEVICE = -5, -6, -7, -8, -9
RM_ERR_NO_DEVICE, RM_ERR_ARG, RM_ERR_TRANSFORM, RM_ERR_MATERIAL = -10, -11, -12, -13
RM_BUF_LIMITS, RM_BUF_COMMANDS, RM_BUF_UNIFORMS = 0, 1, 2
RM_OPT_KERNEL, RM_OPT_TIMING, RM_OPT_STRICT_CAP, RM_OPT_REFILL_MIN, RM_OPT_CULL = 0, 1, 2, 3, 4
RM_OPT_BALANCE, RM_OPT_WAVE_STATS, RM_OPT_WAVES_PER_TILE, RM_OPT_SPECIALIZE, RM_OPT_PRUNE = 5, 6, 7, 8, 9
RM_KERNEL_DEFAULT, RM_KERNEL_PIXEL = 0, 1      # 2..11: the retired v2-v4 variants of ABI version 1
RM_KERNEL_V5, RM_KERNEL_V5_LDS = 12, 13
RM_JIT_PRUNE = 0x100
RM_JIT_RANGE_PROVED = 0x200
RM_STREAM_OWN = (1 << 64) - 1   # (void*)-1: the context's own stream
RM_OPT_OUTPUT_FORMAT = 10
RM_FORMAT_RGBA32F, RM_FORMAT_RGBA8_UNORM, RM_FORMAT_BGRA8_UNORM = 0, 1, 2
RM_INFO_KERNEL_MS, RM_INFO_PROGRAM_COMMANDS, RM_INFO_PROGRAM_WORDS, RM_INFO_PROGRAM_DEPTH = 0, 1, 2, 3
RM_INFO_DEVICE, RM_INFO_CU_COUNT, RM_INFO_SPECIALIZED, RM_INFO_JIT_STATE, RM_INFO_JIT_COMPILE_MS = 4, 5, 6, 7, 8
RM_INFO_PRUNED, RM_INFO_INTERPRETER_LOOP, RM_INFO_JIT_FROM_CACHE, RM_INFO_RANGE_PROOF = 9, 10, 11, 12
# scene queries (rm_query_points / rm_cast_rays / rm_camera_rays)
RM_NO_ID = 0xFFFFFFFF
RM_HIT_NONE, RM_HIT_SURFACE, RM_HIT_FLOOR = 0, 1, 2
RM_SAMPLE_CENTER = 16
RM_SAMPLE_ALL = 17      # rm_draw_gbuffer only: all sixteen AA samples
# mesh export (rm_sample_grid / rm_extract_mesh / rm_read_mesh / rm_mesh_case_table)
RM_MESH_NORMALS, RM_MESH_IDS = 1, 2
# enum rm_meshstat: out_stats of rm_extract_mesh_sparse
(RM_MESH_STAT_VERTICES, RM_MESH_STAT_TRIANGLES, RM_MESH_STAT_BRICKS, RM_MESH_STAT_BRICKS_KEPT, RM_MESH_STAT_EVALUATIONS,
 RM_MESH_STAT_SCRATCH_BYTES, RM_MESH_STATS) = range(7)
MESH_STAT_NAMES = ("vertices", "triangles", "bricks", "bricks_kept", "evaluations", "scratch_bytes")
# mass properties (rm_mass_moments / rm_mass_from_moments): enum rm_moment, enum rm_massstat, enum rm_massprop
(RM_MOMENT_COUNT, RM_MOMENT_X, RM_MOMENT_Y, RM_MOMENT_Z, RM_MOMENT_XX, RM_MOMENT_YY, RM_MOMENT_ZZ, RM_MOMENT_XY, RM_MOMENT_YZ,
 RM_MOMENT_XZ, RM_MOMENT_MIN_X, RM_MOMENT_MIN_Y, RM_MOMENT_MIN_Z, RM_MOMENT_MAX_X, RM_MOMENT_MAX_Y, RM_MOMENT_MAX_Z,
 RM_MOMENTS) = range(17)
(RM_MASS_STAT_BRICKS, RM_MASS_STAT_BRICKS_KEPT, RM_MASS_STAT_BRICKS_INSIDE, RM_MASS_STAT_EVALUATIONS, RM_MASS_STAT_SCRATCH_BYTES,
 RM_MASS_STATS) = range(6)
MASS_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "scratch_bytes")
(RM_MASS_VOLUME, RM_MASS_MASS, RM_MASS_CX, RM_MASS_CY, RM_MASS_CZ, RM_MASS_IXX, RM_MASS_IYY, RM_MASS_IZZ, RM_MASS_IXY, RM_MASS_IYZ,
 RM_MASS_IXZ, RM_MASS_LO_X, RM_MASS_LO_Y, RM_MASS_LO_Z, RM_MASS_HI_X, RM_MASS_HI_Y, RM_MASS_HI_Z, RM_MASS_PROPS) = range(18)
# solid topology (rm_label_solid / rm_label_occupancy / rm_read_topology): enum rm_topocount, enum rm_topostat, the label marks
(RM_TOPO_BODIES, RM_TOPO_CAVITIES, RM_TOPO_POINTS, RM_TOPO_EDGES, RM_TOPO_FACES, RM_TOPO_CELLS, RM_TOPO_EULER, RM_TOPO_TUNNELS,
 RM_TOPO_EXTERIOR_POINTS, RM_TOPO_COUNTS) = range(10)
TOPO_COUNT_NAMES = ("bodies", "cavities", "points", "edges", "faces", "cells", "euler", "tunnels", "exterior_points")
(RM_TOPO_STAT_BRICKS, RM_TOPO_STAT_BRICKS_KEPT, RM_TOPO_STAT_BRICKS_INSIDE, RM_TOPO_STAT_EVALUATIONS, RM_TOPO_STAT_MERGE_PASSES,
 RM_TOPO_STAT_SCRATCH_BYTES, RM_TOPO_STATS) = range(7)
TOPO_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "merge_passes", "scratch_bytes")
RM_TOPO_CAVITY_BIT, RM_TOPO_EXTERIOR = 0x80000000, 0xFFFFFFFF
# distance transform (rm_distance_solid / rm_distance_occupancy / rm_distance_features / rm_read_distance): enum rm_distcount,
# enum rm_distfeature, enum rm_diststat, the marks of the distance volume and the values of the feature mask
RM_DIST_POINTS, RM_DIST_MAX_INSIDE, RM_DIST_ARGMAX_INSIDE, RM_DIST_MAX_OUTSIDE, RM_DIST_ARGMAX_OUTSIDE, RM_DIST_COUNTS = range(6)
DIST_COUNT_NAMES = ("points", "max_inside", "argmax_inside", "max_outside", "argmax_outside")
RM_DIST_CORE, RM_DIST_THIN, RM_DIST_GAP_CORE, RM_DIST_NARROW, RM_DIST_FEATURE_COUNTS = range(5)
DIST_FEATURE_NAMES = ("core", "thin", "gap_core", "narrow")
(RM_DIST_STAT_BRICKS, RM_DIST_STAT_BRICKS_KEPT, RM_DIST_STAT_BRICKS_INSIDE, RM_DIST_STAT_EVALUATIONS, RM_DIST_STAT_SCRATCH_BYTES,
 RM_DIST_STATS) = range(6)
DIST_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "scratch_bytes")
RM_DIST_INSIDE_BIT, RM_DIST_NONE, RM_DIST_SKIP = 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF
DIST_MASK_OUTSIDE, DIST_MASK_INSIDE, DIST_MASK_THIN, DIST_MASK_NARROW = range(4)
# overhangs and supports (rm_support_solid / rm_support_occupancy / rm_read_support): enum rm_up, enum rm_supcount, enum rm_supstat,
# the automatic plate and the values of the mask
RM_UP_POS_X, RM_UP_NEG_X, RM_UP_POS_Y, RM_UP_NEG_Y, RM_UP_POS_Z, RM_UP_NEG_Z = range(6)
UP_NAMES = ("+x", "-x", "+y", "-y", "+z", "-z")
(RM_SUP_POINTS, RM_SUP_PLATE, RM_SUP_BASE, RM_SUP_OVERHANG, RM_SUP_SUPPORT_ON_PLATE, RM_SUP_SUPPORT_ON_PART, RM_SUP_RUNS,
 RM_SUP_LANDINGS, RM_SUP_COUNTS) = range(9)
SUP_COUNT_NAMES = ("points", "plate", "base", "overhang", "support_on_plate", "support_on_part", "runs", "landings")
(RM_SUP_STAT_BRICKS, RM_SUP_STAT_BRICKS_KEPT, RM_SUP_STAT_BRICKS_INSIDE, RM_SUP_STAT_EVALUATIONS, RM_SUP_STAT_SCRATCH_BYTES,
 RM_SUP_STATS) = range(6)
SUP_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "scratch_bytes")
RM_SUPPORT_PLATE_AUTO = 0xFFFFFFFF
SUP_MASK_OUTSIDE, SUP_MASK_INSIDE, SUP_MASK_OVERHANG, SUP_MASK_ON_PLATE, SUP_MASK_ON_PART = range(5)
# layer regions and islands (rm_islands_solid / rm_islands_occupancy / rm_read_islands): enum rm_islcount, enum rm_islstat, enum
# rm_islrow; the region table as a structured array
(RM_ISL_POINTS, RM_ISL_PLATE, RM_ISL_REGIONS, RM_ISL_BASE_REGIONS, RM_ISL_ISLANDS, RM_ISL_ISLAND_POINTS, RM_ISL_MERGES,
 RM_ISL_MAX_LAYER_REGIONS, RM_ISL_COUNTS) = range(9)
ISL_COUNT_NAMES = ("points", "plate", "regions", "base_regions", "islands", "island_points", "merges", "max_layer_regions")
(RM_ISL_STAT_BRICKS, RM_ISL_STAT_BRICKS_KEPT, RM_ISL_STAT_BRICKS_INSIDE, RM_ISL_STAT_EVALUATIONS, RM_ISL_STAT_SCRATCH_BYTES,
 RM_ISL_STATS) = range(6)
ISL_STAT_NAMES = SUP_STAT_NAMES
ISL_ROW_NAMES = ("layer", "first", "points", "supported", "sum_a", "sum_b", "min_a", "max_a", "min_b", "max_b", "below_min", "below_max")
RM_ISL_ROW_WORDS = len(ISL_ROW_NAMES)
ISL_MASK_OUTSIDE, ISL_MASK_INSIDE, ISL_MASK_ISLAND = range(3)
# surface measures (rm_surface_solid / rm_surface_classes / rm_surface_directions / rm_surface_measures): enum rm_surfcount, enum
# rm_surfstat, enum rm_surfmeasure
RM_SURF_CLASSES, RM_SURF_DIRS, RM_SURF_POINTS, RM_SURF_PAIRS, RM_SURF_COUNTS = 8, 13, 0, 8, 840
(RM_SURF_STAT_BRICKS, RM_SURF_STAT_BRICKS_KEPT, RM_SURF_STAT_BRICKS_INSIDE, RM_SURF_STAT_EVALUATIONS, RM_SURF_STAT_SCRATCH_BYTES,
 RM_SURF_STATS) = range(6)
SURF_STAT_NAMES = SUP_STAT_NAMES
(RM_SURF_AREA, RM_SURF_FACET_AREA, RM_SURF_FACET_POS_X, RM_SURF_FACET_NEG_X, RM_SURF_FACET_POS_Y, RM_SURF_FACET_NEG_Y,
 RM_SURF_FACET_POS_Z, RM_SURF_FACET_NEG_Z, RM_SURF_MEASURES) = range(9)
SURF_MEASURE_NAMES = ("area", "facet_area", "facet_pos_x", "facet_neg_x", "facet_pos_y", "facet_neg_y", "facet_pos_z", "facet_neg_z")
# mesh voxelisation (rm_voxelize_mesh / rm_read_voxels): enum rm_voxcount, enum rm_voxstat
(RM_VOX_TRIANGLES, RM_VOX_REJECTED, RM_VOX_EDGE_ON, RM_VOX_CROSSINGS, RM_VOX_INSIDE, RM_VOX_OPEN_ROWS, RM_VOX_COUNTS) = range(7)
VOX_COUNT_NAMES = ("triangles", "rejected", "edge_on", "crossings", "inside", "open_rows")
(RM_VOX_STAT_BRICKS, RM_VOX_STAT_BRICKS_KEPT, RM_VOX_STAT_BRICKS_INSIDE, RM_VOX_STAT_EVALUATIONS, RM_VOX_STAT_ITEMS,
 RM_VOX_STAT_SCRATCH_BYTES, RM_VOX_STATS) = range(7)
VOX_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "items", "scratch_bytes")
# lattice draw (rm_set_lattice / rm_draw_lattice / rm_cast_lattice): enum rm_latcount, enum rm_latstat, RM_LAT_FACE_NONE
(RM_LAT_POINTS, RM_LAT_BRICKS, RM_LAT_COUNTS) = range(3)
LAT_COUNT_NAMES = ("points", "bricks")
(RM_LAT_STAT_BRICKS, RM_LAT_STAT_BRICKS_KEPT, RM_LAT_STAT_BRICKS_INSIDE, RM_LAT_STAT_EVALUATIONS, RM_LAT_STAT_RETAINED_BYTES,
 RM_LAT_STAT_SCRATCH_BYTES, RM_LAT_STATS) = range(7)
LAT_STAT_NAMES = ("bricks", "bricks_kept", "bricks_inside", "evaluations", "retained_bytes", "scratch_bytes")
RM_LAT_FACE_NONE = 6
# lattice meshing (rm_mesh_classes / rm_read_class_mesh): enum rm_cmeshcount, enum rm_cmeshstat
(RM_CMESH_VERTICES, RM_CMESH_TRIANGLES, RM_CMESH_FACES, RM_CMESH_FACES_POS_X, RM_CMESH_FACES_NEG_X, RM_CMESH_FACES_POS_Y,
 RM_CMESH_FACES_NEG_Y, RM_CMESH_FACES_POS_Z, RM_CMESH_FACES_NEG_Z, RM_CMESH_EDGES, RM_CMESH_OPEN_EDGES, RM_CMESH_BRANCH_EDGES,
 RM_CMESH_COUNTS) = range(13)
CMESH_COUNT_NAMES = ("vertices", "triangles", "faces", "faces_pos_x", "faces_neg_x", "faces_pos_y", "faces_neg_y", "faces_pos_z",
                     "faces_neg_z", "edges", "open_edges", "branch_edges")
(RM_CMESH_STAT_BRICKS, RM_CMESH_STAT_BRICKS_KEPT, RM_CMESH_STAT_BRICKS_INSIDE, RM_CMESH_STAT_EVALUATIONS, RM_CMESH_STAT_RETAINED_BYTES,
 RM_CMESH_STAT_SCRATCH_BYTES, RM_CMESH_STATS) = range(7)
CMESH_STAT_NAMES = LAT_STAT_NAMES


def RM_SURF_PAIR(a, b, nu):
    """The index of PAIR[a][b][nu] in the counts of a surface call."""
    return 8 + (8 * a + b) * 13 + nu


# slicing (rm_slice_contours / rm_read_slices / rm_slice_case_table): enum rm_slicecount, the indices of out_counts
RM_SLICE_POINTS, RM_SLICE_CONTOURS, RM_SLICE_COUNTS = 0, 1, 2
# mesh slicing (rm_slice_mesh; read with rm_read_slices): enum rm_mslicecount, enum rm_mslicestat
(RM_MSLICE_TRIANGLES, RM_MSLICE_REJECTED, RM_MSLICE_PAIRED_EDGES, RM_MSLICE_BORDER_EDGES, RM_MSLICE_BRANCH_EDGES, RM_MSLICE_SEGMENTS,
 RM_MSLICE_POINTS, RM_MSLICE_CONTOURS, RM_MSLICE_OPEN_CONTOURS, RM_MSLICE_COUNTS) = range(10)
MSLICE_COUNT_NAMES = ("triangles", "rejected", "paired_edges", "border_edges", "branch_edges", "segments", "points", "contours",
                      "open_contours")
(RM_MSLICE_STAT_SORT_PASSES, RM_MSLICE_STAT_RANK_ROUNDS, RM_MSLICE_STAT_SCRATCH_BYTES, RM_MSLICE_STATS) = range(4)
MSLICE_STAT_NAMES = ("sort_passes", "rank_rounds", "scratch_bytes")
# hatching (rm_hatch_slices / rm_read_hatch): enum rm_hatchflag, enum rm_hatchcount, enum rm_hatchstat
RM_HATCH_ZIGZAG = 1
(RM_HATCH_SEGMENTS_IN, RM_HATCH_CROSSINGS, RM_HATCH_SEGMENTS, RM_HATCH_LINES_HIT, RM_HATCH_ODD_LINES, RM_HATCH_COUNTS) = range(6)
HATCH_COUNT_NAMES = ("segments_in", "crossings", "segments", "lines_hit", "odd_lines")
(RM_HATCH_STAT_SORT_PASSES, RM_HATCH_STAT_SCRATCH_BYTES, RM_HATCH_STATS) = range(3)
HATCH_STAT_NAMES = ("sort_passes", "scratch_bytes")
# the device sort (csrc/rm_sort.h, rm_selftest_sort): rml::kSortTile, the pairs one workgroup ranks
SORT_TILE = 1024
# lit rendering (rm_lighting_defaults / rm_set_lighting / rm_draw_lit): enum rm_light, the parameter names in index order
RM_LIGHT_PARAMS = 13
LIGHT_NAMES = ("pos_x", "pos_y", "pos_z", "shadow", "shadow_softness", "bias", "shadow_max_t", "shadow_steps", "ao", "ao_step",
               "ao_falloff", "ao_scale", "ao_taps")
# ray traversal (rm_trace_defaults / rm_trace_rays): enum rm_trace, the parameter names in index order; event kinds; ray flags
(RM_TRACE_T_MIN, RM_TRACE_T_MAX, RM_TRACE_MIN_STEP, RM_TRACE_STEP_SCALE, RM_TRACE_LEVEL, RM_TRACE_MAX_STEPS,
 RM_TRACE_PARAMS) = range(7)
TRACE_PARAM_NAMES = ("t_min", "t_max", "min_step", "step_scale", "level", "max_steps")
RM_TRACE_ENTER, RM_TRACE_EXIT = 1, 2
RM_TRACE_START_INSIDE, RM_TRACE_END_INSIDE, RM_TRACE_OUT_OF_STEPS = 1, 2, 4
RM_TRACE_MAX_EVENTS = 64

_hip = None
_host = None


def _preload_hip_runtime():
    """One HIP runtime per process.  The torch wheel bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7, requested by libtorch_hip.so as plain "libamdhip64.so"); if librm_hip.so
    pulled in /opt/rocm's copy first, a later `import torch` would load a SECOND runtime, which
    then sees no GPU, and torch stream handles would be meaningless to us.  So when torch is
    installed its copy is loaded first and librm_hip.so binds to it by SONAME.  Hosts without
    torch (C++, Rust) simply use the system ROCm runtime.  RM_HIP_RUNTIME=system skips this."""
    if os.environ.get("RM_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        cand = os.path.join(libdir, "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            # ... and the run-time compiler of the same ROCm release (csrc/rm_jit.h asks for it by SONAME)
            rtc = os.path.join(libdir, "libhiprtc.so")
            if os.path.exists(rtc) and not os.environ.get("RM_HIPRTC_SO"):
                C.CDLL(rtc, mode=C.RTLD_GLOBAL)


def hip_lib():
    """librm_hip.so, loaded once.  Raises if it has not been built."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise ImportError("%s is missing: run `python -m ray_marching_amd.build` (there is no CPU fallback)"
                              % HIP_SO)
        _preload_hip_runtime()
        L = C.CDLL(HIP_SO)
        vp, u32, u64, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64
        L.rm_abi_version.restype = C.c_int
        L.rm_device_count.restype = C.c_int
        L.rm_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rm_destroy.argtypes = [vp]
        L.rm_destroy.restype = None
        L.rm_write_buffer.argtypes = [vp, C.c_int, u64, vp, u64]
        L.rm_set_uniforms.argtypes = [vp, C.POINTER(Uniforms)]
        L.rm_set_limits.argtypes = [vp, C.POINTER(Limits)]
        L.rm_set_program.argtypes = [vp, u32, C.POINTER(u32), u32]
        L.rm_set_materials.argtypes = [vp, u32, C.POINTER(C.c_float)]
        L.rm_resize_command_buffer.argtypes = [vp, u64]
        L.rm_validate.argtypes = [vp]
        L.rm_validate_program.argtypes = [u32, C.POINTER(u32), u32, C.POINTER(u32)]
        L.rm_validate_program.restype = C.c_int
        L.rm_program_info.argtypes = [u32, C.POINTER(u32), u32, C.POINTER(u32), u32]
        L.rm_program_info.restype = C.c_int
        L.rm_draw.argtypes = [vp, u32, u32, u32, u32, vp, C.c_int, vp]
        L.rm_draw_strips.argtypes = [vp, u32, u32, u32, u32, u32, vp, C.c_int, vp, C.POINTER(u32)]
        L.rm_draw_strips.restype = C.c_int
        L.rm_draw_batch.argtypes = [vp, C.POINTER(Uniforms), u32, u32, u32, vp, C.c_int, vp]
        L.rm_gather_strips.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp, vp]
        L.rm_gather_strips.restype = C.c_int
        L.rm_host_register.argtypes = [vp, u64]
        L.rm_host_register.restype = C.c_int
        L.rm_host_unregister.argtypes = [vp]
        L.rm_host_unregister.restype = C.c_int
        L.rm_sync.argtypes = [vp]
        L.rm_sync_context.argtypes = [vp]
        L.rm_sync_context.restype = C.c_int
        L.rm_set_option.argtypes = [vp, C.c_int, i64]
        L.rm_get_info.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
        L.rm_measure_write_bandwidth.argtypes = [vp, u64, C.c_int, C.POINTER(C.c_double)]
        L.rm_selftest_sqrt.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
        L.rm_selftest_sqrt.restype = C.c_int
        L.rm_selftest_ops.argtypes = [vp, vp, vp, vp, u32]
        L.rm_selftest_ops.restype = C.c_int
        L.rm_selftest_div.argtypes = [vp, vp, vp, u32, u32, u32, C.POINTER(u64)]
        L.rm_selftest_div.restype = C.c_int
        L.rm_selftest_normalise.argtypes = [vp, vp, u32, C.c_int, vp]
        L.rm_selftest_normalise.restype = C.c_int
        L.rm_selftest_wave.argtypes = [vp, vp, u32, vp]
        L.rm_selftest_wave.restype = C.c_int
        L.rm_selftest_sort.argtypes = [vp, vp, vp, u32, u32, vp, vp]
        L.rm_selftest_sort.restype = C.c_int
        L.rm_selftest_cull_rays.argtypes = [vp, vp, vp, u32, vp, vp]
        L.rm_selftest_cull_rays.restype = C.c_int
        L.rm_selftest_cull_pixels.argtypes = [vp, u32, u32, vp, u32, vp]
        L.rm_selftest_cull_pixels.restype = C.c_int
        L.rm_selftest_cull_tiles.argtypes = [vp, u32, u32, vp, u32, vp]
        L.rm_selftest_cull_tiles.restype = C.c_int
        L.rm_selftest_cull_waves.argtypes = [vp, vp, vp, vp, vp, u32, C.c_float, vp]
        L.rm_selftest_cull_waves.restype = C.c_int
        L.rm_selftest_anchor.argtypes = [vp, vp, vp, u32, vp]
        L.rm_selftest_anchor.restype = C.c_int
        L.rm_read_wave_stats.argtypes = [vp, vp, u64, C.POINTER(u64)]
        L.rm_read_wave_stats.restype = C.c_int
        L.rm_query_points.argtypes = [vp, u32, vp, vp, vp, vp, C.c_int, vp]
        L.rm_query_points.restype = C.c_int
        L.rm_cast_rays.argtypes = [vp, u32, vp, vp, vp, vp, C.c_int, vp]
        L.rm_cast_rays.restype = C.c_int
        L.rm_camera_rays.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, vp, C.c_int, vp]
        L.rm_camera_rays.restype = C.c_int
        f3 = C.POINTER(C.c_float)
        L.rm_trace_defaults.argtypes = [f3, u32]
        L.rm_trace_defaults.restype = C.c_int
        L.rm_trace_rays.argtypes = [vp, u32, vp, f3, u32, u32, u32, vp, vp, vp, vp, C.c_int, vp]
        L.rm_trace_rays.restype = C.c_int
        L.rm_sample_grid.argtypes = [vp, f3, f3, u32, u32, u32, vp, C.c_int, vp]
        L.rm_sample_grid.restype = C.c_int
        L.rm_extract_mesh.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, u32, C.POINTER(u64)]
        L.rm_extract_mesh.restype = C.c_int
        L.rm_read_mesh.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp]
        L.rm_read_mesh.restype = C.c_int
        L.rm_mesh_case_table.argtypes = [vp, u32]
        L.rm_mesh_case_table.restype = C.c_int
        L.rm_extract_mesh_sparse.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, u32, C.POINTER(u64), u32]
        L.rm_extract_mesh_sparse.restype = C.c_int
        L.rm_mass_moments.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_mass_moments.restype = C.c_int
        L.rm_mass_from_moments.argtypes = [C.POINTER(u64), u32, f3, f3, C.c_double, C.POINTER(C.c_double), u32]
        L.rm_mass_from_moments.restype = C.c_int
        L.rm_label_solid.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_label_solid.restype = C.c_int
        L.rm_label_occupancy.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_label_occupancy.restype = C.c_int
        L.rm_read_topology.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        L.rm_read_topology.restype = C.c_int
        L.rm_distance_solid.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_distance_solid.restype = C.c_int
        L.rm_distance_occupancy.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_distance_occupancy.restype = C.c_int
        L.rm_distance_features.argtypes = [vp, u32, u32, C.POINTER(u64), u32]
        L.rm_distance_features.restype = C.c_int
        L.rm_read_distance.argtypes = [vp, vp, vp, C.c_int, vp]
        L.rm_read_distance.restype = C.c_int
        L.rm_support_solid.argtypes = [vp, f3, f3, u32, u32, u32, C.c_float, u32, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_support_solid.restype = C.c_int
        L.rm_support_occupancy.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, u32, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_support_occupancy.restype = C.c_int
        L.rm_read_support.argtypes = [vp, vp, vp, C.c_int, vp]
        L.rm_read_support.restype = C.c_int
        L.rm_islands_solid.argtypes = L.rm_support_solid.argtypes
        L.rm_islands_solid.restype = C.c_int
        L.rm_islands_occupancy.argtypes = L.rm_support_occupancy.argtypes
        L.rm_islands_occupancy.restype = C.c_int
        L.rm_read_islands.argtypes = [vp, vp, u64, vp, vp, vp, C.c_int, vp]
        L.rm_read_islands.restype = C.c_int
        L.rm_surface_solid.argtypes = L.rm_label_solid.argtypes
        L.rm_surface_solid.restype = C.c_int
        L.rm_surface_classes.argtypes = L.rm_label_occupancy.argtypes
        L.rm_surface_classes.restype = C.c_int
        L.rm_surface_directions.argtypes = [C.POINTER(C.c_int), u32]
        L.rm_surface_directions.restype = C.c_int
        L.rm_surface_measures.argtypes = [C.POINTER(u64), u32, f3, u32, u32, C.POINTER(C.c_double), u32]
        L.rm_surface_measures.restype = C.c_int
        L.rm_voxelize_mesh.argtypes = [vp, u32, vp, u32, vp, C.c_int, vp, f3, f3, u32, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_voxelize_mesh.restype = C.c_int
        L.rm_read_voxels.argtypes = [vp, vp, C.c_int, vp]
        L.rm_read_voxels.restype = C.c_int
        L.rm_set_lattice.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, f3, f3, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_set_lattice.restype = C.c_int
        L.rm_draw_lattice.argtypes = [vp, u32, u32, u32, u32, vp, vp, C.c_int, vp]
        L.rm_draw_lattice.restype = C.c_int
        L.rm_cast_lattice.argtypes = [vp, u32, vp, vp, vp, vp, vp, C.c_int, vp]
        L.rm_cast_lattice.restype = C.c_int
        L.rm_mesh_classes.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, f3, f3, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_mesh_classes.restype = C.c_int
        L.rm_read_class_mesh.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        L.rm_read_class_mesh.restype = C.c_int
        L.rm_slice_contours.argtypes = [vp, u32, f3, f3, u32, u32, f3, u32, C.c_float, u32, C.POINTER(u64), u32]
        L.rm_slice_contours.restype = C.c_int
        L.rm_read_slices.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.rm_read_slices.restype = C.c_int
        L.rm_slice_case_table.argtypes = [vp, u32]
        L.rm_slice_case_table.restype = C.c_int
        L.rm_slice_mesh.argtypes = [vp, vp, u32, vp, u32, C.c_int, vp, f3, f3, u32, f3, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_slice_mesh.restype = C.c_int
        L.rm_hatch_slices.argtypes = [vp, f3, u32, u32, u32, C.POINTER(u64), u32, C.POINTER(u64), u32]
        L.rm_hatch_slices.restype = C.c_int
        L.rm_read_hatch.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        L.rm_read_hatch.restype = C.c_int
        L.rm_program_lipschitz.argtypes = [u32, C.POINTER(u32), u32, C.POINTER(C.c_double)]
        L.rm_program_lipschitz.restype = C.c_int
        L.rm_lighting_defaults.argtypes = [f3, u32]
        L.rm_lighting_defaults.restype = C.c_int
        L.rm_set_lighting.argtypes = [vp, f3, u32]
        L.rm_set_lighting.restype = C.c_int
        L.rm_draw_lit.argtypes = [vp, u32, u32, u32, u32, vp, C.c_int, vp]
        L.rm_draw_lit.restype = C.c_int
        L.rm_draw_gbuffer.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, vp, vp, vp, C.c_int, vp]
        L.rm_draw_gbuffer.restype = C.c_int
        L.rm_program_subtree.argtypes = [u32, C.POINTER(u32), u32, u32, C.POINTER(u32), C.POINTER(u32)]
        L.rm_program_subtree.restype = C.c_int
        sz = C.c_size_t
        L.rm_jit_source.argtypes = [u32, C.POINTER(u32), u32, C.c_int, C.c_char_p, sz, C.POINTER(sz)]
        L.rm_jit_source.restype = C.c_int
        L.rm_jit_compile.argtypes = [u32, C.POINTER(u32), u32, C.c_int, C.POINTER(C.c_double), C.POINTER(sz),
                                     C.c_char_p, sz]
        L.rm_jit_compile.restype = C.c_int
        L.rm_jit_log.argtypes = [vp, C.c_char_p, sz]
        L.rm_jit_log.restype = C.c_int
        L.rm_last_error.argtypes = [vp]
        L.rm_last_error.restype = C.c_char_p
        L.rm_status_string.argtypes = [C.c_int]
        L.rm_status_string.restype = C.c_char_p
        for name in ("rm_create", "rm_write_buffer", "rm_set_uniforms", "rm_set_limits", "rm_set_program",
                     "rm_resize_command_buffer", "rm_validate", "rm_draw", "rm_draw_batch", "rm_sync",
                     "rm_set_option", "rm_get_info", "rm_measure_write_bandwidth", "rm_set_materials"):
            getattr(L, name).restype = C.c_int
        _hip = L
    return _hip


def check(ctx, status):
    if status != RM_OK:
        L = hip_lib()
        msg = L.rm_last_error(ctx) or b""
        raise RmError(status, msg.decode() or L.rm_status_string(status).decode())
    return status


class OrbitState(C.Structure):
    """rmh_orbit (include/rm_host.h)."""
    _fields_ = [("target", C.c_float * 3), ("pitch", C.c_float), ("yaw", C.c_float), ("radius", C.c_float),
                ("pan_speed", C.c_float), ("yaw_speed", C.c_float), ("pitch_speed", C.c_float),
                ("dolly_speed", C.c_float)]


class CameraState(C.Structure):
    """rmh_camera: position + unit quaternion (w,i,j,k)."""
    _fields_ = [("position", C.c_float * 3), ("rotation", C.c_float * 4)]


def host_lib():
    """librm_host.so (pure host code: scene model, serializer, camera)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_SO):
            raise ImportError("%s is missing: run `python -m ray_marching_amd.build`" % HOST_SO)
        L = C.CDLL(HOST_SO)
        vp, u32, f32p = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
        L.rmh_sphere.argtypes = [f32p, C.c_float]
        L.rmh_box.argtypes = [f32p, f32p]
        L.rmh_union.argtypes = [vp, vp]
        L.rmh_subtraction.argtypes = [vp, vp]
        L.rmh_plane.argtypes = [f32p, C.c_float]
        L.rmh_cylinder.argtypes = [f32p, C.c_float, C.c_float]
        L.rmh_intersection.argtypes = [vp, vp]
        L.rmh_smooth_union.argtypes = [vp, vp, C.c_float]
        L.rmh_translation.argtypes = [vp, f32p]
        L.rmh_rotation.argtypes = [vp, f32p]
        L.rmh_scale.argtypes = [vp, C.c_float]
        L.rmh_material.argtypes = [vp, u32]
        L.rmh_node_clone.argtypes = [vp]
        L.rmh_scene.argtypes = [C.c_char_p]
        for n in ("rmh_sphere", "rmh_box", "rmh_union", "rmh_subtraction", "rmh_node_clone", "rmh_scene",
                  "rmh_builder_new", "rmh_plane", "rmh_cylinder", "rmh_intersection", "rmh_smooth_union",
                  "rmh_translation", "rmh_rotation", "rmh_scale", "rmh_material"):
            getattr(L, n).restype = vp
        L.rmh_node_free.argtypes = [vp]
        L.rmh_node_free.restype = None
        L.rmh_builder_free.argtypes = [vp]
        L.rmh_builder_free.restype = None
        L.rmh_builder_push_command.argtypes = [vp, u32]
        L.rmh_builder_push_command.restype = None
        L.rmh_builder_push_param_vec3.argtypes = [vp, f32p]
        L.rmh_builder_push_param_vec3.restype = None
        L.rmh_builder_push_param_float.argtypes = [vp, C.c_float]
        L.rmh_builder_push_param_float.restype = None
        L.rmh_builder_cmd_count.argtypes = [vp]
        L.rmh_builder_cmd_count.restype = u32
        L.rmh_builder_len.argtypes = [vp]
        L.rmh_builder_len.restype = u32
        L.rmh_builder_buffer.argtypes = [vp]
        L.rmh_builder_buffer.restype = C.POINTER(u32)
        L.rmh_build_commands.argtypes = [vp, vp]
        L.rmh_build_commands.restype = None
        L.rmh_orbit_new.argtypes = [C.POINTER(OrbitState), f32p, C.c_float]
        L.rmh_orbit_new.restype = None
        L.rmh_orbit_update.argtypes = [C.POINTER(OrbitState), C.c_int, C.c_float, C.c_float]
        L.rmh_orbit_update.restype = None
        L.rmh_orbit_camera.argtypes = [C.POINTER(OrbitState), C.POINTER(CameraState)]
        L.rmh_orbit_camera.restype = None
        L.rmh_camera_view.argtypes = [C.POINTER(CameraState), f32p]
        L.rmh_camera_view.restype = None
        L.rmh_prepare_uniforms.argtypes = [f32p, C.POINTER(CameraState), vp]
        L.rmh_prepare_uniforms.restype = None
        _host = L
    return _host
