"""Python face of csrc/host/renderer.hpp: RayMarchingResources / RayMarchingCallback of
src/ray_marching/renderer.rs on top of the C ABI (include/rm_abi.h).  Device memory and
streams may come from torch; the render itself is always the HIP kernel (no CPU fallback)."""
import ctypes as C

import numpy as np

from . import _ffi
from . import csg as _csg
from . import mesh as _mesh
from ._ffi import Limits, Uniforms


def prepare_uniforms(viewport, camera):
    """The host half of prepare() (renderer.rs:205-222): the 144-byte Uniforms blob."""
    u = Uniforms()
    vp = (C.c_float * 2)(float(viewport[0]), float(viewport[1]))
    _ffi.host_lib().rmh_prepare_uniforms(vp, C.byref(camera._s), C.byref(u))
    return u


class RayMarchLimits:  # renderer.rs:36-41, defaults :133-137
    def __init__(self, min_dist=0.01, max_dist=100.0, max_iter=100):
        self.min_dist, self.max_dist, self.max_iter = float(min_dist), float(max_dist), int(max_iter)

    def as_struct(self):
        return Limits(self.min_dist, self.max_dist, self.max_iter)


class RayMarchingResources:
    """Long-lived GPU state (renderer.rs:43-49) = one rm_ctx on one GPU."""

    def __init__(self, device=0):
        self._L = _ffi.hip_lib()
        h = C.c_void_p()
        rc = self._L.rm_create(int(device), C.byref(h))
        if rc != _ffi.RM_OK:
            raise _ffi.RmError(rc, (self._L.rm_last_error(None) or b"").decode())
        self._h = h
        self.device = int(device)
        self._dtype = np.float32
        self._serials = {family: [0, None] for family in _FAMILIES}    # see _advance

    def close(self):
        if getattr(self, "_h", None):
            self._L.rm_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        return _ffi.check(self._h, rc)

    # -- the three buffers of the bind group ------------------------------------------------
    def write_buffer(self, buffer, offset, data):
        """Queue::write_buffer (renderer.rs:213,230,235); data: bytes-like."""
        b = bytes(data)
        if buffer == _ffi.RM_BUF_COMMANDS:
            self._program = None      # (no longer what set_program gave: trace_rays cannot bound its step from it)
        self._check(self._L.rm_write_buffer(self._h, buffer, offset, b, len(b)))

    def set_limits(self, limits):
        s = limits.as_struct() if isinstance(limits, RayMarchLimits) else Limits(*limits)
        self._check(self._L.rm_set_limits(self._h, C.byref(s)))

    def set_uniforms(self, u):
        self._check(self._L.rm_set_uniforms(self._h, C.byref(u)))

    def set_program(self, cmd_count, words):
        w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
        n = int(w.size)
        ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if n else None
        self._program = None
        self._check(self._L.rm_set_program(self._h, int(cmd_count), ptr, n))
        self._program = (int(cmd_count), w.copy())

    def set_materials(self, rgb):
        """Material table (extension): (n, 3) albedo values, n in [1, 256]; entry i colours the surfaces tagged Material(i)."""
        m = np.ascontiguousarray(np.asarray(rgb, dtype=np.float32).reshape(-1, 3))
        self._check(self._L.rm_set_materials(self._h, len(m), m.ctypes.data_as(C.POINTER(C.c_float))))

    def set_scene(self, node):
        self.set_program(*_csg.serialize(node))

    def resize_command_buffer(self, nbytes):
        self._check(self._L.rm_resize_command_buffer(self._h, int(nbytes)))

    def validate(self):
        self._check(self._L.rm_validate(self._h))

    # -- draws -------------------------------------------------------------------------------
    def set_output_format(self, fmt):
        """RM_OPT_OUTPUT_FORMAT: _ffi.RM_FORMAT_RGBA32F (default) / RGBA8_UNORM / BGRA8_UNORM.  The host-array draw
        methods then return uint8 (..., 4) arrays; the *_device methods write 4 bytes per pixel."""
        self.set_option(_ffi.RM_OPT_OUTPUT_FORMAT, fmt)
        self._dtype = np.float32 if fmt == _ffi.RM_FORMAT_RGBA32F else np.uint8

    def draw(self, W, H, row0=0, rows=None):
        """Render rows [row0,row0+rows) into a new host array (rows, W, 4): float32, or uint8 for the 8-bit formats."""
        rows = H - row0 if rows is None else rows
        out = np.empty((max(rows, 0), W, 4), dtype=self._dtype)
        self._check(self._L.rm_draw(self._h, W, H, row0, rows, out.ctypes.data_as(C.c_void_p), 0, None))
        return out

    def draw_device(self, W, H, out_ptr, row0=0, rows=None, stream=None):
        """Asynchronous render into device memory (out_ptr: integer device address)."""
        rows = H - row0 if rows is None else rows
        self._check(self._L.rm_draw(self._h, W, H, row0, rows, C.c_void_p(out_ptr), 1,
                                    C.c_void_p(stream) if stream else None))

    def draw_strips(self, W, H, strip_rows, first, stride):
        """This GPU's interleaved strips of a W x H image (rm_draw_strips) -> (rows, W, 4) host array."""
        from . import shard
        rows = shard.strip_row_count(H, strip_rows, first, stride)
        out = np.empty((rows, W, 4), dtype=self._dtype)
        n = C.c_uint32(0)
        self._check(self._L.rm_draw_strips(self._h, W, H, strip_rows, first, stride,
                                           out.ctypes.data_as(C.c_void_p) if rows else None, 0, None, C.byref(n)))
        assert n.value == rows
        return out

    def draw_strips_device(self, W, H, strip_rows, first, stride, out_ptr, stream=None):
        n = C.c_uint32(0)
        self._check(self._L.rm_draw_strips(self._h, W, H, strip_rows, first, stride, C.c_void_p(out_ptr), 1,
                                           C.c_void_p(stream) if stream else None, C.byref(n)))
        return n.value

    def gather_strips(self, W, H, strip_rows, first, stride, strips_ptr, host_ptr, stream=None):
        """rm_gather_strips: this GPU's strips (device buffer rm_draw_strips filled) -> their rows of the full host image
        at address host_ptr (pinned / registered memory: asynchronous on `stream`)."""
        self._check(self._L.rm_gather_strips(self._h, W, H, strip_rows, first, stride, C.c_void_p(strips_ptr),
                                             C.c_void_p(host_ptr), C.c_void_p(stream) if stream else None))

    def draw_batch(self, frames, W, H):
        arr = (Uniforms * len(frames))(*frames)
        out = np.empty((len(frames), H, W, 4), dtype=self._dtype)
        self._check(self._L.rm_draw_batch(self._h, arr, len(frames), W, H, out.ctypes.data_as(C.c_void_p), 0, None))
        return out

    def draw_batch_device(self, frames, W, H, out_ptr, stream=None):
        arr = (Uniforms * len(frames))(*frames)
        self._check(self._L.rm_draw_batch(self._h, arr, len(frames), W, H, C.c_void_p(out_ptr), 1,
                                          C.c_void_p(stream) if stream else None))

    # -- lit rendering (rm_set_lighting / rm_draw_lit): soft shadows and ambient occlusion, DESIGN.md section 13 -------------
    def set_lighting(self, **named):
        """Sets the named lighting parameters (_ffi.LIGHT_NAMES; pos=(x, y, z) names the first three); the others keep
        their current values.  A value outside its range raises RmError(RM_ERR_RANGE) and changes nothing."""
        p = list(getattr(self, "_light", None) or lighting_defaults())
        if "pos" in named:
            p[0:3] = [float(v) for v in named.pop("pos")]
        for k, v in named.items():
            if k not in _ffi.LIGHT_NAMES:
                raise ValueError("unknown lighting parameter %r (one of %s, or pos)" % (k, ", ".join(_ffi.LIGHT_NAMES)))
            p[_ffi.LIGHT_NAMES.index(k)] = float(v)
        arr = (C.c_float * _ffi.RM_LIGHT_PARAMS)(*p)
        self._check(self._L.rm_set_lighting(self._h, arr, _ffi.RM_LIGHT_PARAMS))
        self._light = [float(v) for v in arr]

    def lighting(self):
        """The context's lighting parameters as a dict (float32 values)."""
        return dict(zip(_ffi.LIGHT_NAMES, getattr(self, "_light", None) or lighting_defaults()))

    def draw_lit(self, W, H, row0=0, rows=None):
        """draw() with shadows and ambient occlusion (rm_draw_lit): rows [row0,row0+rows) into a new host array."""
        rows = H - row0 if rows is None else rows
        out = np.empty((max(rows, 0), W, 4), dtype=self._dtype)
        self._check(self._L.rm_draw_lit(self._h, W, H, row0, rows, out.ctypes.data_as(C.c_void_p), 0, None))
        return out

    def draw_lit_device(self, W, H, out_ptr, row0=0, rows=None, stream=None):
        """draw_device() with shadows and ambient occlusion: asynchronous render into device memory."""
        rows = H - row0 if rows is None else rows
        self._check(self._L.rm_draw_lit(self._h, W, H, row0, rows, C.c_void_p(out_ptr), 1,
                                        C.c_void_p(stream) if stream else None))

    # -- G-buffer draw (rm_draw_gbuffer): per-pixel depth, normals, ids and selection masks, DESIGN.md section 14 -----------
    GBUFFER_KEYS = ("t", "position", "normal", "diffuse", "kind", "sample", "leaf", "material", "surface_mask", "floor_mask",
                    "selected_mask", "steps")

    def draw_gbuffer(self, W, H, row0=0, rows=None, sample=_ffi.RM_SAMPLE_ALL, select=None):
        """The geometry behind rows [row0,row0+rows) of a W x H frame, per pixel (rm_draw_gbuffer).  sample: 0..15,
        RM_SAMPLE_CENTER, or RM_SAMPLE_ALL (the sixteen AA samples).  select: (first, count), a range of command indices
        (program_subtree gives a node's).  Returns a dict of host arrays of shape (rows, W[, 3]): t, position, normal,
        diffuse (the hit record of the nearest sample), kind (RM_HIT_*), sample, leaf, material (of that sample; RM_NO_ID
        where there is none), surface_mask, floor_mask, selected_mask (one bit per sample) and steps (summed over the
        samples)."""
        rows = H - row0 if rows is None else rows
        first, count = (0, 0) if select is None else (int(select[0]), int(select[1]))
        shape = (max(rows, 0), W)
        geom = np.empty(shape + (8,), dtype=np.float32)
        ids = np.empty(shape + (4,), dtype=np.uint32)
        masks = np.empty(shape + (4,), dtype=np.uint32)
        self._check(self._L.rm_draw_gbuffer(self._h, W, H, row0, rows, sample, first, count, geom.ctypes.data_as(C.c_void_p),
                                            ids.ctypes.data_as(C.c_void_p), masks.ctypes.data_as(C.c_void_p), 0, None))
        return {"t": geom[..., 0], "position": geom[..., 1:4], "normal": geom[..., 4:7], "diffuse": geom[..., 7],
                "kind": ids[..., 0], "sample": ids[..., 1], "leaf": ids[..., 2], "material": ids[..., 3],
                "surface_mask": masks[..., 0], "floor_mask": masks[..., 1], "selected_mask": masks[..., 2], "steps": masks[..., 3]}

    def draw_gbuffer_device(self, W, H, geom_ptr=0, ids_ptr=0, masks_ptr=0, row0=0, rows=None, sample=_ffi.RM_SAMPLE_ALL,
                            select=None, stream=None):
        """rm_draw_gbuffer on device memory (integer addresses, 16-byte aligned; 0 = not wanted), asynchronous on `stream`:
        per pixel 8 floats at geom_ptr, 4 u32 at ids_ptr, 4 u32 at masks_ptr."""
        rows = H - row0 if rows is None else rows
        first, count = (0, 0) if select is None else (int(select[0]), int(select[1]))
        self._check(self._L.rm_draw_gbuffer(self._h, W, H, row0, rows, sample, first, count, C.c_void_p(geom_ptr or None),
                                            C.c_void_p(ids_ptr or None), C.c_void_p(masks_ptr or None), 1,
                                            C.c_void_p(stream) if stream else None))

    def sync(self):
        self._check(self._L.rm_sync(self._h))

    def sync_context(self):
        """Wait for this context's own stream (draws issued with stream=_ffi.RM_STREAM_OWN)."""
        self._check(self._L.rm_sync_context(self._h))

    # -- options / info ------------------------------------------------------------------------
    def set_option(self, key, value):
        self._check(self._L.rm_set_option(self._h, key, int(value)))

    def info(self, key):
        v = C.c_double()
        self._check(self._L.rm_get_info(self._h, key, C.byref(v)))
        return v.value

    def jit_log(self):
        """Compiler / loader messages of the structure specialiser for the current program ('' if none)."""
        buf = C.create_string_buffer(1 << 16)
        self._check(self._L.rm_jit_log(self._h, buf, len(buf)))
        return buf.value.decode(errors="replace")

    def wave_stats(self, max_waves=1 << 20):
        """Diagnostics: (n_waves, 4) uint64 array recorded by the last draw with RM_OPT_WAVE_STATS."""
        buf = np.zeros((max_waves, 4), dtype=np.uint64)
        n = C.c_uint64(0)
        self._check(self._L.rm_read_wave_stats(self._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n)))
        return buf[: n.value // 32]

    def measure_write_bandwidth(self, nbytes=1 << 30, iters=10):
        v = C.c_double()
        self._check(self._L.rm_measure_write_bandwidth(self._h, nbytes, iters, C.byref(v)))
        return v.value

    # -- scene queries (rm_query_points / rm_cast_rays / rm_camera_rays) ---------------------------------------------------
    # numpy in, numpy out (host path, synchronous); a float32 torch tensor on this context's GPU in, torch tensors out on that
    # GPU, computed on torch.cuda.current_stream() without a host round trip.
    def _query_input(self, a, width, name):
        """(kind, array, n): kind "torch" or "numpy"; array contiguous float32 of shape (n, width)."""
        if type(a).__module__.split(".")[0] == "torch":
            import torch
            if a.device.type != "cuda" or a.device.index != self.device:
                raise ValueError("%s is on %s; this context is on cuda:%d" % (name, a.device, self.device))
            if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != width:
                raise ValueError("%s must be a float32 tensor of shape (n, %d)" % (name, width))
            return "torch", a.contiguous(), int(a.shape[0])
        arr = np.asarray(a, dtype=np.float32)
        if arr.shape == (width,):     # one row
            arr = arr.reshape(1, width)
        if arr.ndim != 2 or arr.shape[1] != width:
            raise ValueError("%s must be an array of shape (n, %d), not %s" % (name, width, arr.shape))
        arr = np.ascontiguousarray(arr)
        return "numpy", arr, int(arr.shape[0])

    @staticmethod
    def _torch_stream(t):
        import torch
        return torch.cuda.current_stream(t.device).cuda_stream

    def query_points(self, points, normals=False):
        """Signed distance, leaf (command index of the primitive the value comes from, RM_NO_ID for an empty program) and
        material at each point of an (n, 3) array; with normals=True also the shading normal.  Returns a dict of arrays:
        distance (n,), leaf (n,), material (n,)[, normal (n, 3)]."""
        kind, p, n = self._query_input(points, 3, "points")
        if kind == "torch":
            import torch
            dist = torch.empty(n, dtype=torch.float32, device=p.device)
            ids = torch.empty((n, 2), dtype=torch.int32, device=p.device)
            nrm = torch.empty((n, 3), dtype=torch.float32, device=p.device) if normals else None
            self.query_points_device(n, p.data_ptr(), dist.data_ptr(), nrm.data_ptr() if normals else 0, ids.data_ptr(),
                                     stream=self._torch_stream(p))
            out = {"distance": dist, "leaf": ids[:, 0], "material": ids[:, 1]}   # int32 views of the u32 ids (RM_NO_ID = -1)
        else:
            dist = np.empty(n, dtype=np.float32)
            ids = np.empty((n, 2), dtype=np.uint32)
            nrm = np.empty((n, 3), dtype=np.float32) if normals else None
            self._check(self._L.rm_query_points(self._h, n, p.ctypes.data, dist.ctypes.data, nrm.ctypes.data if normals else None,
                                                ids.ctypes.data, 0, None))
            out = {"distance": dist, "leaf": ids[:, 0], "material": ids[:, 1]}
        if normals:
            out["normal"] = nrm
        return out

    def query_points_device(self, n, xyz_ptr, dist_ptr=0, normal_ptr=0, ids_ptr=0, stream=None):
        """rm_query_points on device memory (integer addresses; 0 = not wanted), asynchronous on `stream`."""
        self._check(self._L.rm_query_points(self._h, int(n), C.c_void_p(xyz_ptr), C.c_void_p(dist_ptr or None),
                                            C.c_void_p(normal_ptr or None), C.c_void_p(ids_ptr or None), 1,
                                            C.c_void_p(stream) if stream else None))

    def _rays_input(self, origins, directions):
        """_query_input for rays: origins (n, 3) + directions (n, 3), or one (n, 6) array as camera_rays returns."""
        if directions is None:
            return self._query_input(origins, 6, "rays")
        ko, o, n = self._query_input(origins, 3, "origins")
        kd, d, nd = self._query_input(directions, 3, "directions")
        if ko != kd or n != nd:
            raise ValueError("origins and directions must be arrays of the same kind and length")
        if ko == "torch":
            import torch
            return ko, torch.cat([o, d], dim=1).contiguous(), n
        return ko, np.ascontiguousarray(np.concatenate([o, d], axis=1)), n

    def cast_rays(self, origins, directions=None):
        """March rays (origins (n, 3) + directions (n, 3), or one (n, 6) array as camera_rays returns) exactly as the draw
        does.  Returns a dict: kind (RM_HIT_*), steps, leaf, material (RM_NO_ID unless a surface), t, position (n, 3),
        normal (n, 3), diffuse, rgb (n, 3)."""
        kind, r, n = self._rays_input(origins, directions)
        if kind == "torch":
            import torch
            hit = torch.empty((n, 8), dtype=torch.float32, device=r.device)
            ids = torch.empty((n, 4), dtype=torch.int32, device=r.device)
            rgb = torch.empty((n, 3), dtype=torch.float32, device=r.device)
            self.cast_rays_device(n, r.data_ptr(), hit.data_ptr(), ids.data_ptr(), rgb.data_ptr(), stream=self._torch_stream(r))
        else:
            hit = np.empty((n, 8), dtype=np.float32)
            ids = np.empty((n, 4), dtype=np.uint32)
            rgb = np.empty((n, 3), dtype=np.float32)
            self._check(self._L.rm_cast_rays(self._h, n, r.ctypes.data, hit.ctypes.data, ids.ctypes.data, rgb.ctypes.data, 0, None))
        return {"kind": ids[:, 0], "steps": ids[:, 1], "leaf": ids[:, 2], "material": ids[:, 3], "t": hit[:, 0],
                "position": hit[:, 1:4], "normal": hit[:, 4:7], "diffuse": hit[:, 7], "rgb": rgb}

    def cast_rays_device(self, n, rays_ptr, hit_ptr=0, ids_ptr=0, rgb_ptr=0, stream=None):
        """rm_cast_rays on device memory (integer addresses; 0 = not wanted), asynchronous on `stream`."""
        self._check(self._L.rm_cast_rays(self._h, int(n), C.c_void_p(rays_ptr), C.c_void_p(hit_ptr or None),
                                         C.c_void_p(ids_ptr or None), C.c_void_p(rgb_ptr or None), 1,
                                         C.c_void_p(stream) if stream else None))

    # -- ray traversal (rm_trace_rays): every entry and exit of the solid along a ray, DESIGN.md section 18 -------------------
    @staticmethod
    def trace_defaults():
        """The default traversal parameters as a dict (_ffi.TRACE_PARAM_NAMES; pure host code)."""
        return dict(zip(_ffi.TRACE_PARAM_NAMES, trace_defaults()))

    def _trace_params(self, named):
        p = trace_defaults()
        for i, k in enumerate(_ffi.TRACE_PARAM_NAMES):
            if named.get(k) is not None:
                p[i] = float(named[k])
        if named.get("step_scale") is None:
            # a step of |d - level| / max(1, L) cannot pass the level set (L: the program's Lipschitz bound)
            prog = getattr(self, "_program", None)
            if prog is None:
                raise ValueError("step_scale=None needs the program as set_program / set_scene gave it; pass a step_scale")
            L = program_lipschitz(*prog)
            if not np.isfinite(L):
                raise ValueError("the program has no finite Lipschitz bound (rm_program_lipschitz): pass a step_scale, "
                                 "which then carries no guarantee")
            p[_ffi.RM_TRACE_STEP_SCALE] = float(np.float32(1.0 / max(1.0, L)))
        return (C.c_float * _ffi.RM_TRACE_PARAMS)(*p)

    def trace_rays(self, origins, directions=None, *, t_min=None, t_max=None, min_step=None, step_scale=None, level=None,
                   max_steps=None, max_events=8, normals=False, ids=True):
        """Every crossing of the level set along each ray over [t_min, t_max], in order (rays as for cast_rays; parameters
        left at None take trace_defaults(); step_scale=None: 1 / max(1, program_lipschitz), ValueError when that bound is
        infinite).  Returns a dict.  Per ray: events (found, counting past max_events), steps, flags (RM_TRACE_START_INSIDE /
        END_INSIDE / OUT_OF_STEPS), stored, t_end, length (inside the solid), d_start, d_end.  Per event slot (n, max_events):
        t (+inf when unfilled), position, normal (zeros unless normals=True), width, kind (RM_TRACE_ENTER / EXIT; 0 when
        unfilled), step, leaf, material (RM_NO_ID unless ids=True)."""
        params = self._trace_params(dict(t_min=t_min, t_max=t_max, min_step=min_step, step_scale=step_scale, level=level,
                                         max_steps=max_steps))
        kind, r, n = self._rays_input(origins, directions)
        K = int(max_events)
        flags = (_ffi.RM_MESH_NORMALS if normals else 0) | (_ffi.RM_MESH_IDS if ids else 0)
        if kind == "torch":
            import torch
            ev = torch.empty((n, K, 8), dtype=torch.float32, device=r.device)
            eid = torch.empty((n, K, 4), dtype=torch.int32, device=r.device)
            cnt = torch.empty((n, 4), dtype=torch.int32, device=r.device)
            sp = torch.empty((n, 4), dtype=torch.float32, device=r.device)
            self.trace_rays_device(n, r.data_ptr(), params, K, flags, ev.data_ptr(), eid.data_ptr(), cnt.data_ptr(), sp.data_ptr(),
                                   stream=self._torch_stream(r))
        else:
            ev = np.empty((n, K, 8), dtype=np.float32)
            eid = np.empty((n, K, 4), dtype=np.uint32)
            cnt = np.empty((n, 4), dtype=np.uint32)
            sp = np.empty((n, 4), dtype=np.float32)
            self._check(self._L.rm_trace_rays(self._h, n, r.ctypes.data, params, _ffi.RM_TRACE_PARAMS, K, flags, ev.ctypes.data,
                                              eid.ctypes.data, cnt.ctypes.data, sp.ctypes.data, 0, None))
        return {"events": cnt[:, 0], "steps": cnt[:, 1], "flags": cnt[:, 2], "stored": cnt[:, 3], "t_end": sp[:, 0],
                "length": sp[:, 1], "d_start": sp[:, 2], "d_end": sp[:, 3], "t": ev[:, :, 0], "position": ev[:, :, 1:4],
                "normal": ev[:, :, 4:7], "width": ev[:, :, 7], "kind": eid[:, :, 0], "step": eid[:, :, 1], "leaf": eid[:, :, 2],
                "material": eid[:, :, 3]}

    def trace_rays_device(self, n, rays_ptr, params, max_events, flags=0, events_ptr=0, event_ids_ptr=0, counts_ptr=0, spans_ptr=0,
                          stream=None):
        """rm_trace_rays on device memory (integer addresses; 0 = not wanted), asynchronous on `stream`.  params: the six
        values in _ffi.TRACE_PARAM_NAMES order."""
        p = params if isinstance(params, C.Array) else (C.c_float * _ffi.RM_TRACE_PARAMS)(*[float(v) for v in params])
        self._check(self._L.rm_trace_rays(self._h, int(n), C.c_void_p(rays_ptr), p, len(p), int(max_events), int(flags),
                                          C.c_void_p(events_ptr or None), C.c_void_p(event_ids_ptr or None),
                                          C.c_void_p(counts_ptr or None), C.c_void_p(spans_ptr or None), 1,
                                          C.c_void_p(stream) if stream else None))

    def camera_rays(self, W, H, x0=0, y0=0, w=None, h=None, sample=_ffi.RM_SAMPLE_CENTER, out=None):
        """The rays the draw marches for AA sample `sample` (0..15, or RM_SAMPLE_CENTER) of the pixels of the w x h block at
        (x0, y0) of a W x H frame: (w*h, 6) float32, row-major.  out: a contiguous float32 torch tensor of exactly w*h*6
        elements on this context's GPU, filled on torch.cuda.current_stream() (and returned) instead of a new host array --
        the rays rm_cast_rays then reads without a host round trip."""
        w = W - x0 if w is None else w
        h = H - y0 if h is None else h
        if out is not None:
            # the library writes w*h*6 floats from out's first element on: nothing but a dense tensor of that size may receive them
            if type(out).__module__.split(".")[0] != "torch":
                raise ValueError("out must be a torch tensor")
            import torch
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError("out is on %s; this context is on cuda:%d" % (out.device, self.device))
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != max(w, 0) * max(h, 0) * 6:
                raise ValueError("out must be a contiguous float32 tensor of %d elements (w*h x 6)" % (max(w, 0) * max(h, 0) * 6))
            self.camera_rays_device(W, H, x0, y0, w, h, out.data_ptr(), sample, stream=self._torch_stream(out))
            return out
        rays = np.empty((max(w, 0) * max(h, 0), 6), dtype=np.float32)
        self._check(self._L.rm_camera_rays(self._h, W, H, x0, y0, w, h, sample, rays.ctypes.data if rays.size else None, 0, None))
        return rays

    def camera_rays_device(self, W, H, x0, y0, w, h, out_ptr, sample=_ffi.RM_SAMPLE_CENTER, stream=None):
        self._check(self._L.rm_camera_rays(self._h, W, H, x0, y0, w, h, sample, C.c_void_p(out_ptr), 1,
                                           C.c_void_p(stream) if stream else None))

    def pick(self, W, H, x, y):
        """What is under pixel (x, y) of a W x H frame: the ray through its centre, cast.  Returns a dict of scalars (the
        keys of cast_rays): kind, steps, leaf (the command index of the primitive hit, RM_NO_ID if none), material, t,
        position, normal, diffuse, rgb."""
        hit = self.cast_rays(self.camera_rays(W, H, x, y, 1, 1))
        return {k: (v[0] if v.ndim == 1 else v[0].copy()) for k, v in hit.items()}

    # -- mesh export (rm_sample_grid / rm_extract_mesh / rm_read_mesh) ------------------------------------------------------
    # A lattice is (origin, step, shape), each in (x, y, z) order: point (i, j, k) lies at origin + (i, j, k) * step (float32,
    # one rounded product and one rounded sum per coordinate); arrays of lattice values are indexed [k, j, i].
    @staticmethod
    def _lattice(origin, step, shape, least):
        # copies: the library reads 3 floats from each address, and a broadcast or strided view (extract_mesh's scalar lo)
        # does not hold them there
        o = np.array(origin, dtype=np.float32, copy=True).reshape(-1)
        s = np.array(step, dtype=np.float32, copy=True).reshape(-1)
        n = tuple(int(x) for x in np.asarray(shape).reshape(-1))
        if o.shape != (3,) or s.shape != (3,) or len(n) != 3:
            raise ValueError("origin, step and shape must have 3 entries each (x, y, z)")
        if not np.all(np.isfinite(o)) or not np.all(np.isfinite(s)) or not np.all(s > 0):
            raise ValueError("origin must be finite and step finite and > 0")
        if min(n) < least:
            raise ValueError("a lattice needs at least %d points per axis, not %s" % (least, n))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        return o, s, n, fp

    def sample_grid(self, origin, step, shape, out=None):
        """map_scene at the lattice points: float32 (nz, ny, nx), bit-identical to the oracle.  out: a contiguous float32
        torch tensor of nx*ny*nz elements on this context's GPU, filled on torch.cuda.current_stream() (and returned)."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 1)
        if out is not None:
            if type(out).__module__.split(".")[0] != "torch":
                raise ValueError("out must be a torch tensor")
            import torch
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError("out is on %s; this context is on cuda:%d" % (out.device, self.device))
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != nx * ny * nz:
                raise ValueError("out must be a contiguous float32 tensor of %d elements (nx*ny*nz)" % (nx * ny * nz))
            self.sample_grid_device(o, s, (nx, ny, nz), out.data_ptr(), stream=self._torch_stream(out))
            return out
        d = np.empty((nz, ny, nx), dtype=np.float32)
        self._check(self._L.rm_sample_grid(self._h, fp(o), fp(s), nx, ny, nz, d.ctypes.data, 0, None))
        return d

    def sample_grid_device(self, origin, step, shape, out_ptr, stream=None):
        """rm_sample_grid into device memory (an integer address), asynchronous on `stream`."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 1)
        self._check(self._L.rm_sample_grid(self._h, fp(o), fp(s), nx, ny, nz, C.c_void_p(out_ptr), 1,
                                           C.c_void_p(stream) if stream else None))

    @staticmethod
    def _box_lattice(lo, hi, resolution):
        lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (3,))
        hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (3,))
        n = np.broadcast_to(np.asarray(resolution), (3,))
        if not np.all(np.isfinite(lo)) or not np.all(np.isfinite(hi)) or not np.all(lo < hi):
            raise ValueError("lo and hi must be finite with lo < hi on every axis")
        if n.dtype.kind not in "iu" or np.any(n < 2):
            raise ValueError("resolution must be an integer of at least 2 points per axis, not %s" % (resolution,))
        return lo, (hi - lo) / (n.astype(np.float32) - np.float32(1.0)), n

    def extract_mesh(self, lo, hi, resolution, level=0.0, normals=True, ids=True, device=False):
        """The surface map_scene = level inside the box [lo, hi], on a lattice of `resolution` points per axis (an int, or
        (nx, ny, nz)): origin lo, step (hi - lo) / (n - 1) in float32.  Returns a mesh.Mesh (numpy arrays, or torch tensors
        on this context's GPU with device=True).  The mesh is open where the surface leaves the box."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.extract_mesh_grid(lo, step, n, level, normals, ids, device)

    def extract_mesh_grid(self, origin, step, shape, level=0.0, normals=True, ids=True, device=False):
        """extract_mesh on an exact lattice (origin, step, shape as sample_grid takes them)."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 2)
        flags = (_ffi.RM_MESH_NORMALS if normals else 0) | (_ffi.RM_MESH_IDS if ids else 0)
        counts = (C.c_uint64 * 2)()
        self._check(self._L.rm_extract_mesh(self._h, fp(o), fp(s), nx, ny, nz, float(level), flags, counts))
        return self._read_mesh(int(counts[0]), int(counts[1]), normals, ids, device)

    def extract_mesh_sparse(self, lo, hi, resolution, level=0.0, normals=True, ids=True, device=False):
        """extract_mesh through rm_extract_mesh_sparse: the same mesh, bit for bit, evaluated only in the bricks of 8 x 8 x 8
        lattice points the surface can reach -- and with no limit on the number of lattice points.  The returned Mesh
        carries the call's statistics in mesh.stats (a dict: _ffi.MESH_STAT_NAMES)."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.extract_mesh_grid_sparse(lo, step, n, level, normals, ids, device)

    def extract_mesh_grid_sparse(self, origin, step, shape, level=0.0, normals=True, ids=True, device=False):
        """extract_mesh_sparse on an exact lattice (origin, step, shape as sample_grid takes them)."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 2)
        flags = (_ffi.RM_MESH_NORMALS if normals else 0) | (_ffi.RM_MESH_IDS if ids else 0)
        stats = (C.c_uint64 * _ffi.RM_MESH_STATS)()
        self._check(self._L.rm_extract_mesh_sparse(self._h, fp(o), fp(s), nx, ny, nz, float(level), flags, stats, _ffi.RM_MESH_STATS))
        m = self._read_mesh(int(stats[_ffi.RM_MESH_STAT_VERTICES]), int(stats[_ffi.RM_MESH_STAT_TRIANGLES]), normals, ids, device)
        m.stats = {name: int(stats[k]) for k, name in enumerate(_ffi.MESH_STAT_NAMES)}
        return m

    # -- mass properties (rm_mass_moments / rm_mass_from_moments) -------------------------------------------------------------
    def mass_moments(self, origin, step, shape, level=0.0):
        """The integer moments of the solid map_scene < level on an exact lattice (origin, step, shape as sample_grid takes them;
        2..4096 points per axis): a MassMoments with .moments (uint64[16], _ffi.RM_MOMENT_*: count, sums of i, j, k, of their
        squares and products, smallest and largest inside index per axis) and .stats (a dict: _ffi.MASS_STAT_NAMES).  Exact:
        every implementation and every run gives the same words."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 2)
        mom = np.zeros(_ffi.RM_MOMENTS, dtype=np.uint64)
        stats = (C.c_uint64 * _ffi.RM_MASS_STATS)()
        self._check(self._L.rm_mass_moments(self._h, fp(o), fp(s), nx, ny, nz, float(level), mom.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            _ffi.RM_MOMENTS, stats, _ffi.RM_MASS_STATS))
        return MassMoments(mom, {name: int(stats[k]) for k, name in enumerate(_ffi.MASS_STAT_NAMES)}, o, s, (nx, ny, nz))

    def mass_properties(self, lo, hi, resolution, level=0.0, density=1.0):
        """Volume, mass, centre of mass, inertia tensor (about the centre of mass) and bounding box of the solid map_scene < level
        inside the box [lo, hi], on the lattice extract_mesh_sparse builds from (lo, hi, resolution): a dict (mass_from_moments)
        that also carries "moments" and "stats".  A first-order quadrature: each inside lattice point stands for its cell."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        m = self.mass_moments(lo, step, n, level)
        props = mass_from_moments(m.moments, m.origin, m.step, density)
        props["moments"], props["stats"] = m.moments, m.stats
        return props

    # -- solid topology (rm_label_solid / rm_label_occupancy / rm_read_topology) -----------------------------------------------
    def label_solid(self, lo, hi, resolution, level=0.0):
        """Bodies, cavities and tunnels of the solid map_scene < level inside the box [lo, hi], on the lattice extract_mesh
        builds from (lo, hi, resolution) (2..1024 points per axis, at most 2^28 in all): a Topology."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.label_solid_grid(lo, step, n, level)

    def label_solid_grid(self, origin, step, shape, level=0.0):
        """label_solid on an exact lattice (origin, step, shape as sample_grid takes them)."""
        return self._solid_grid_call(self._L.rm_label_solid, *_TOPO_OUTPUTS, origin, step, shape, level, None, self._read_topology)

    def label_occupancy(self, occupancy):
        """rm_label_occupancy: the topology of a caller's occupancy, indexed [k, j, i] (shape (nz, ny, nx); nonzero = inside): a
        numpy array of a one-byte type (bool, uint8, int8), or such a contiguous torch tensor on this context's GPU, read after
        the work queued on torch.cuda.current_stream().  The Topology's lattice is the unit lattice at the origin."""
        return self._occupancy_call(self._L.rm_label_occupancy, *_TOPO_OUTPUTS, occupancy, None, self._read_topology)

    # What the eight analyses of a lattice share (rm_label_*, rm_distance_*, rm_support_*, rm_islands_*): fn, the families of retained
    # results it replaces, the sizes and the names of its counts and statistics (a row of the _*_OUTPUTS below), `direction` -- None,
    # or (up, r2, plate) as the caller gave them --, and result(counts, stats, origin, step, shape[, up, r2]): both outputs as dicts.
    def _solid_grid_call(self, fn, families, n_counts, n_stats, count_names, stat_names, origin, step, shape, level, direction, result):
        """A *_solid_grid call: fn = rm_*_solid on an exact lattice."""
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 2)
        extra = _support_args(*direction) if direction else ()
        counts, stats = (C.c_uint64 * n_counts)(), (C.c_uint64 * n_stats)()
        self._check(fn(self._h, fp(o), fp(s), nx, ny, nz, float(level), *extra, counts, n_counts, stats, n_stats))
        self._advance(fn, *families)
        return result(_named(counts, count_names), _named(stats, stat_names), o, s, (nx, ny, nz), *extra[:2])

    def _occupancy_call(self, fn, families, n_counts, n_stats, count_names, stat_names, occupancy, direction, result):
        """A *_occupancy call: fn = rm_*_occupancy on a caller's occupancy; the result's lattice is the unit lattice."""
        nx, ny, nz, ptr, is_device, stream, keep = self._occupancy_arg(occupancy)
        extra = _support_args(*direction) if direction else ()
        counts, stats = (C.c_uint64 * n_counts)(), (C.c_uint64 * n_stats)()
        self._check(fn(self._h, nx, ny, nz, ptr, is_device, stream, *extra, counts, n_counts, stats, n_stats))
        self._advance(fn, *families)
        del keep
        return result(_named(counts, count_names), _named(stats, stat_names), np.zeros(3, dtype=np.float32), np.ones(3, dtype=np.float32),
                      (nx, ny, nz), *extra[:2])

    def _occupancy_arg(self, occupancy):
        """A caller's occupancy as the library takes it: nx, ny, nz, its address, is_device, the stream, and the object to keep
        alive during the call."""
        if type(occupancy).__module__.split(".")[0] == "torch":
            t = occupancy
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("occupancy is on %s; this context is on cuda:%d" % (t.device, self.device))
            if t.element_size() != 1 or t.dim() != 3 or not t.is_contiguous():
                raise ValueError("occupancy must be a contiguous 3-D tensor of a one-byte type")
            nz, ny, nx = (int(x) for x in t.shape)
            ptr, is_device, stream, keep = C.c_void_p(t.data_ptr()), 1, C.c_void_p(self._torch_stream(t)), t
        else:
            a = np.asarray(occupancy)
            if a.ndim != 3 or a.dtype.itemsize != 1:
                raise ValueError("occupancy must be a 3-D array of a one-byte type, indexed [k, j, i]")
            keep = np.ascontiguousarray(a)
            nz, ny, nx = keep.shape
            ptr, is_device, stream = C.c_void_p(keep.ctypes.data), 0, None
        if min(nx, ny, nz) < 2:
            raise ValueError("a lattice needs at least 2 points per axis, not %s" % ((nx, ny, nz),))
        return nx, ny, nz, ptr, is_device, stream, keep

    def _read_topology(self, cd, sd, origin, step, shape):
        """The Topology of the labelling call that just returned: its counts and statistics, and both row tables read back."""
        for name in ("euler", "tunnels"):                                    # two's-complement int64
            cd[name] -= (cd[name] >> 63) << 64
        body, cav, _ = self._read_new(self._L.rm_read_topology, [((cd["bodies"], _ffi.RM_MOMENTS), *_U64, True),
                                                                 ((cd["cavities"], _ffi.RM_MOMENTS), *_U64, True), _SKIP])
        return Topology(self, cd, sd, body, cav, origin, step, shape)

    def read_topology_device(self, body_moments_ptr=0, cavity_moments_ptr=0, labels_ptr=0, stream=None):
        """rm_read_topology of the last labelling call into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_topology, (body_moments_ptr, cavity_moments_ptr, labels_ptr), True, stream)

    # -- distance transform (rm_distance_solid / rm_distance_occupancy / rm_distance_features / rm_read_distance) ----------------
    def distance_solid(self, lo, hi, resolution, level=0.0):
        """The exact squared distance transform of the solid map_scene < level inside the box [lo, hi], on the lattice
        extract_mesh builds from (lo, hi, resolution) (2..1024 points per axis, at most 2^28 in all): a Distance."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.distance_solid_grid(lo, step, n, level)

    def distance_solid_grid(self, origin, step, shape, level=0.0):
        """distance_solid on an exact lattice (origin, step, shape as sample_grid takes them)."""
        return self._solid_grid_call(self._L.rm_distance_solid, *_DIST_OUTPUTS, origin, step, shape, level, None,
                                     lambda *a: Distance(self, *a))

    def distance_occupancy(self, occupancy):
        """rm_distance_occupancy: the distance transform of a caller's occupancy, as label_occupancy takes it (indexed [k, j, i],
        nonzero = inside; numpy, or a torch tensor on this context's GPU).  The Distance's lattice is the unit lattice at the
        origin."""
        return self._occupancy_call(self._L.rm_distance_occupancy, *_DIST_OUTPUTS, occupancy, None, lambda *a: Distance(self, *a))

    def read_distance_device(self, d2_ptr=0, mask_ptr=0, stream=None):
        """rm_read_distance of the last distance volume and feature mask into device memory (integer addresses; 0 = not wanted),
        asynchronous."""
        self._read_into(self._L.rm_read_distance, (d2_ptr, mask_ptr), True, stream)

    # -- overhangs and supports (rm_support_solid / rm_support_occupancy / rm_read_support) ---------------------------------------
    def support_solid(self, lo, hi, resolution, level=0.0, up="+z", r2=1, plate=None):
        """Overhangs and supports of the solid map_scene < level inside the box [lo, hi], on the lattice extract_mesh builds from
        (lo, hi, resolution) (2..1024 points per axis, at most 2^28 in all), for the build direction `up` ("+x" .. "-z", or
        _ffi.RM_UP_*), the squared reach r2 (index units, 0..255; reach_r2 converts an angle) and the plate's height (None: the
        lowest layer that holds an inside point): a Support."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.support_solid_grid(lo, step, n, level, up, r2, plate)

    def support_solid_grid(self, origin, step, shape, level=0.0, up="+z", r2=1, plate=None):
        """support_solid on an exact lattice (origin, step, shape as sample_grid takes them)."""
        return self._solid_grid_call(self._L.rm_support_solid, *_SUP_OUTPUTS, origin, step, shape, level, (up, r2, plate),
                                     lambda *a: Support(self, *a))

    def support_occupancy(self, occupancy, up="+z", r2=1, plate=None):
        """rm_support_occupancy: overhangs and supports of a caller's occupancy, as label_occupancy takes it (indexed [k, j, i],
        nonzero = inside; numpy, or a torch tensor on this context's GPU).  The Support's lattice is the unit lattice at the
        origin."""
        return self._occupancy_call(self._L.rm_support_occupancy, *_SUP_OUTPUTS, occupancy, (up, r2, plate), lambda *a: Support(self, *a))

    def read_support_device(self, mask_ptr=0, profile_ptr=0, stream=None):
        """rm_read_support of the last mask and profile into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_support, (mask_ptr, profile_ptr), True, stream)

    # -- layer regions and islands (rm_islands_solid / rm_islands_occupancy / rm_read_islands) -----------------------------------
    def islands_solid(self, lo, hi, resolution, level=0.0, up="+z", r2=1, plate=None):
        """Layer regions and islands of the solid map_scene < level inside the box [lo, hi], on the lattice extract_mesh builds
        from (lo, hi, resolution) (2..1024 points per axis, at most 2^28 in all), for the build direction `up`, the squared reach
        r2 and the plate's height as support_solid takes them: an Islands."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.islands_solid_grid(lo, step, n, level, up, r2, plate)

    def islands_solid_grid(self, origin, step, shape, level=0.0, up="+z", r2=1, plate=None):
        """islands_solid on an exact lattice (origin, step, shape as sample_grid takes them)."""
        return self._solid_grid_call(self._L.rm_islands_solid, *_ISL_OUTPUTS, origin, step, shape, level, (up, r2, plate),
                                     lambda *a: Islands(self, *a))

    def islands_occupancy(self, occupancy, up="+z", r2=1, plate=None):
        """rm_islands_occupancy: layer regions and islands of a caller's occupancy, as label_occupancy takes it (indexed [k, j, i],
        nonzero = inside; numpy, or a torch tensor on this context's GPU).  The Islands' lattice is the unit lattice at the
        origin."""
        return self._occupancy_call(self._L.rm_islands_occupancy, *_ISL_OUTPUTS, occupancy, (up, r2, plate), lambda *a: Islands(self, *a))

    def read_islands_device(self, rows_ptr=0, row_capacity=0, labels_ptr=0, mask_ptr=0, profile_ptr=0, stream=None):
        """rm_read_islands of the last region table (row_capacity rows of room), label volume, mask and profile into device memory
        (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._islands_reader(row_capacity), (rows_ptr, labels_ptr, mask_ptr, profile_ptr), True, stream)

    # -- surface measures (rm_surface_solid / rm_surface_classes / rm_surface_measures) -----------------------------------------------
    def surface_solid(self, lo, hi, resolution, level=0.0):
        """The pair counts of the solid map_scene < level (class 1 inside, 0 outside) inside the box [lo, hi], on the lattice
        extract_mesh builds from (lo, hi, resolution) (2..1024 points per axis, at most 2^28 in all): a Surface, whose
        measures(1, 0) are the solid's surface area."""
        lo, step, n = self._box_lattice(lo, hi, resolution)
        return self.surface_solid_grid(lo, step, n, level)

    def surface_solid_grid(self, origin, step, shape, level=0.0):
        """surface_solid on an exact lattice (origin, step, shape as sample_grid takes them)."""
        return self._solid_grid_call(self._L.rm_surface_solid, *_SURF_OUTPUTS, origin, step, shape, level, None, Surface)

    def surface_classes(self, classes):
        """rm_surface_classes: the pair counts of a caller's classes, as label_occupancy takes an occupancy (indexed [k, j, i];
        numpy, or a torch tensor on this context's GPU): one byte per point, the class min(byte, 7) -- an occupancy, or the mask
        of a Support, a DistanceFeatures or an Islands as it is.  The Surface's lattice is the unit lattice at the origin; give
        measures() the step of the lattice the classes came from."""
        return self._occupancy_call(self._L.rm_surface_classes, *_SURF_OUTPUTS, classes, None, Surface)

    # -- mesh voxelisation (rm_voxelize_mesh / rm_read_voxels) ------------------------------------------------------------------------
    def _mesh_arg(self, vertices, triangles):
        """A mesh as the library takes it: n_vertices, the address of xyz, n_triangles, the address of the indices (None: a soup),
        is_device, the stream, and the objects to keep alive during the call."""
        if hasattr(vertices, "vertices") and hasattr(vertices, "triangles"):      # a mesh.Mesh
            if triangles is not None:
                raise ValueError("a Mesh brings its own triangles")
            vertices, triangles = vertices.vertices, vertices.triangles
        if type(vertices).__module__.split(".")[0] == "torch":
            import torch
            v = vertices
            if v.device.type != "cuda" or v.device.index != self.device:
                raise ValueError("vertices are on %s; this context is on cuda:%d" % (v.device, self.device))
            if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3 or not v.is_contiguous():
                raise ValueError("vertices must be a contiguous float32 tensor of shape (n, 3)")
            t = triangles
            if t is not None:
                if type(t).__module__.split(".")[0] != "torch" or t.device != v.device:
                    raise ValueError("triangles must be a tensor on the vertices' device")
                if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
                    raise ValueError("triangles must be a contiguous int32 tensor of shape (n, 3) (the u32 indices' words)")
            nv, nt = int(v.shape[0]), int(t.shape[0]) if t is not None else int(v.shape[0]) // 3
            return (nv, C.c_void_p(v.data_ptr() if nv else None), nt, C.c_void_p(t.data_ptr()) if t is not None and nt else None, 1,
                    C.c_void_p(self._torch_stream(v)), (v, t))
        v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError("vertices must be an array of shape (n, 3), not %s" % (v.shape,))
        t = None
        if triangles is not None:
            t = np.asarray(triangles)
            if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[1] != 3:
                raise ValueError("triangles must be an integer array of shape (n, 3)")
            if t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
                raise ValueError("a vertex index must fit 32 unsigned bits")
            t = np.ascontiguousarray(t.astype(np.uint32))
        nv, nt = len(v), len(t) if t is not None else len(v) // 3
        return (nv, C.c_void_p(v.ctypes.data if nv else None), nt, C.c_void_p(t.ctypes.data) if t is not None and nt else None, 0, None,
                (v, t))

    def voxelize_mesh(self, vertices, triangles=None, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), shape=(64, 64, 64)):
        """rm_voxelize_mesh: the occupancy of a triangle mesh on an exact lattice (origin, step, shape as sample_grid takes them;
        2..1024 points per axis, at most 2^28 in all), by the even-odd rule along +x: a Voxels.  vertices (n, 3) float32 and
        triangles (m, 3) vertex indices -- None: a soup, every three vertices a triangle -- as numpy arrays, or as contiguous torch
        tensors on this context's GPU (indices int32, as extract_mesh(device=True) gives them), read after the work queued on
        torch.cuda.current_stream(); or a mesh.Mesh of either kind in place of both.  Needs no scene."""
        nv, xyz, nt, idx, is_device, stream, keep = self._mesh_arg(vertices, triangles)
        o, s, (nx, ny, nz), fp = self._lattice(origin, step, shape, 2)
        counts, stats = (C.c_uint64 * _ffi.RM_VOX_COUNTS)(), (C.c_uint64 * _ffi.RM_VOX_STATS)()
        fn = self._L.rm_voxelize_mesh
        self._check(fn(self._h, nv, xyz, nt, idx, is_device, stream, fp(o), fp(s), nx, ny, nz, counts, _ffi.RM_VOX_COUNTS, stats,
                       _ffi.RM_VOX_STATS))
        self._advance(fn, "voxels")
        del keep
        return Voxels(self, _named(counts, _ffi.VOX_COUNT_NAMES), _named(stats, _ffi.VOX_STAT_NAMES), o, s, (nx, ny, nz))

    def voxelize_mesh_box(self, vertices, triangles=None, resolution=128, margin=2):
        """voxelize_mesh on a lattice chosen from the mesh's bounding box (over its finite coordinates): one step for all three
        axes, `resolution` points along the longest one, on the others as many as the box needs, with `margin` empty points all
        round -- the analyses treat what lies beyond the lattice as outside, and the distance transform measures to the border
        only where there is one."""
        resolution, margin = int(resolution), int(margin)
        if margin < 0 or resolution - 2 * margin < 2:
            raise ValueError("resolution %d leaves no two points between margins of %d" % (resolution, margin))
        v = vertices.vertices if hasattr(vertices, "vertices") else vertices
        if type(v).__module__.split(".")[0] == "torch":
            import torch
            finite = torch.where(torch.isfinite(v), v, torch.full_like(v, float("nan")))
            lo = torch.nan_to_num(finite, nan=float("inf")).amin(dim=0).cpu().numpy().astype(np.float64)
            hi = torch.nan_to_num(finite, nan=float("-inf")).amax(dim=0).cpu().numpy().astype(np.float64)
        else:
            a = np.asarray(v, dtype=np.float32).reshape(-1, 3).astype(np.float64)
            a = np.where(np.isfinite(a), a, np.nan)
            with np.errstate(all="ignore"):
                lo, hi = np.nanmin(a, axis=0), np.nanmax(a, axis=0)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.max(hi - lo) > 0):
            raise ValueError("the mesh has no finite extent")
        step = float(np.max(hi - lo)) / (resolution - 1 - 2 * margin)
        shape = [min(resolution, max(2, int(np.ceil((hi[a] - lo[a]) / step)) + 1 + 2 * margin)) for a in range(3)]
        return self.voxelize_mesh(vertices, triangles, lo - margin * step, (step, step, step), shape)

    def read_voxels_device(self, occupancy_ptr, stream=None):
        """rm_read_voxels of the last voxelisation into device memory (an integer address), asynchronous."""
        self._read_into(self._L.rm_read_voxels, (occupancy_ptr,), True, stream)

    # -- lattice draw (rm_set_lattice / rm_draw_lattice / rm_cast_lattice) -------------------------------------------------------------
    def set_lattice(self, classes, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
        """rm_set_lattice: the lattice of class bytes that draw_lattice and cast_lattice show -- an occupancy, a mask, their sum --
        as a 3-D array of a one-byte type indexed [k, j, i], or a contiguous torch tensor on this context's GPU (read after the
        work queued on torch.cuda.current_stream(), copied without a host round trip).  Point (i, j, k) is the cube of one step
        around origin + (i, j, k) * step; byte 0 is empty, a byte c > 0 takes the albedo min(c, count - 1) of the material table
        (set_materials) as it stands when it is drawn.  Needs no scene.  Returns a Lattice (counts, stats)."""
        nx, ny, nz, ptr, is_device, stream, keep = self._occupancy_arg(classes)
        o, s, _, fp = self._lattice(origin, step, (nx, ny, nz), 2)
        counts, stats = (C.c_uint64 * _ffi.RM_LAT_COUNTS)(), (C.c_uint64 * _ffi.RM_LAT_STATS)()
        fn = self._L.rm_set_lattice
        self._check(fn(self._h, nx, ny, nz, ptr, is_device, stream, fp(o), fp(s), counts, _ffi.RM_LAT_COUNTS, stats, _ffi.RM_LAT_STATS))
        self._advance(fn, "lattice")
        del keep
        return Lattice(self, _named(counts, _ffi.LAT_COUNT_NAMES), _named(stats, _ffi.LAT_STAT_NAMES), o, s, (nx, ny, nz))

    @staticmethod
    def _window(window):
        """A cut-away window (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z) -- points lo <= i < hi are shown -- as the library takes it; None:
        the whole lattice."""
        if window is None:
            return None, None
        w = np.array(window, dtype=np.int64).reshape(-1)
        if w.shape != (6,) or w.min() < 0 or w.max() > 0xFFFFFFFF:
            raise ValueError("a window is (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), six unsigned integers")
        w = w.astype(np.uint32)
        return w.ctypes.data_as(C.c_void_p), w

    def draw_lattice(self, W, H, row0=0, rows=None, window=None):
        """rm_draw_lattice: rows [row0, row0 + rows) of the image of the retained lattice (set_lattice) through the uniforms'
        camera, a new host array (rows, W, 4): float32, or uint8 for the 8-bit formats.  window: see _window."""
        rows = H - row0 if rows is None else rows
        out = np.empty((max(rows, 0), W, 4), dtype=self._dtype)
        wp, keep = self._window(window)
        self._check(self._L.rm_draw_lattice(self._h, W, H, row0, rows, wp, out.ctypes.data_as(C.c_void_p), 0, None))
        del keep
        return out

    def draw_lattice_device(self, W, H, out_ptr, row0=0, rows=None, window=None, stream=None):
        """rm_draw_lattice into device memory (out_ptr: integer device address), asynchronous on `stream`."""
        rows = H - row0 if rows is None else rows
        wp, keep = self._window(window)
        self._check(self._L.rm_draw_lattice(self._h, W, H, row0, rows, wp, C.c_void_p(out_ptr), 1, C.c_void_p(stream) if stream else None))
        del keep

    def cast_lattice(self, origins, directions=None, window=None):
        """rm_cast_lattice: rays (as cast_rays takes them) through the retained lattice.  Returns a dict: kind (RM_HIT_*), index
        (the linear point index i + nx (j + ny k)), cls (the class byte), face (2 axis + (normal positive), RM_LAT_FACE_NONE for
        an origin inside a cube) -- RM_NO_ID unless a surface --, t, position (n, 3), normal (n, 3), diffuse, rgb (n, 3)."""
        kind, r, n = self._rays_input(origins, directions)
        if kind == "torch":
            import torch
            hit = torch.empty((n, 8), dtype=torch.float32, device=r.device)
            ids = torch.empty((n, 4), dtype=torch.int32, device=r.device)
            rgb = torch.empty((n, 3), dtype=torch.float32, device=r.device)
            self.cast_lattice_device(n, r.data_ptr(), hit.data_ptr(), ids.data_ptr(), rgb.data_ptr(), window=window,
                                     stream=self._torch_stream(r))
        else:
            hit = np.empty((n, 8), dtype=np.float32)
            ids = np.empty((n, 4), dtype=np.uint32)
            rgb = np.empty((n, 3), dtype=np.float32)
            wp, keep = self._window(window)
            self._check(self._L.rm_cast_lattice(self._h, n, r.ctypes.data, wp, hit.ctypes.data, ids.ctypes.data, rgb.ctypes.data, 0, None))
            del keep
        return {"kind": ids[:, 0], "index": ids[:, 1], "cls": ids[:, 2], "face": ids[:, 3], "t": hit[:, 0],
                "position": hit[:, 1:4], "normal": hit[:, 4:7], "diffuse": hit[:, 7], "rgb": rgb}

    def cast_lattice_device(self, n, rays_ptr, hit_ptr=0, ids_ptr=0, rgb_ptr=0, window=None, stream=None):
        """rm_cast_lattice on device memory (integer addresses; 0 = not wanted), asynchronous on `stream`."""
        wp, keep = self._window(window)
        self._check(self._L.rm_cast_lattice(self._h, int(n), C.c_void_p(rays_ptr), wp, C.c_void_p(hit_ptr or None),
                                            C.c_void_p(ids_ptr or None), C.c_void_p(rgb_ptr or None), 1,
                                            C.c_void_p(stream) if stream else None))
        del keep

    # -- lattice meshing (rm_mesh_classes / rm_read_class_mesh) ----------------------------------------------------------------------
    def mesh_classes(self, classes, a, b=None, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), device=False):
        """rm_mesh_classes: the interface between the class sets a and b (a class, or an iterable of classes; b=None: every class
        not in a) of a lattice of class bytes, as set_lattice and surface_classes take one (indexed [k, j, i]; numpy, or a
        contiguous torch tensor on this context's GPU, taken without a host copy), as a welded, indexed triangle mesh: the unit
        faces between a point of a and a 6-neighbour of b, wound counter-clockwise seen from the b side.  Point (i, j, k) lies at
        origin + (i, j, k) * step, the faces half a step from it.  Returns a ClassMesh -- a mesh.Mesh without normals, with counts,
        stats and the per-triangle face_classes, face and face_point -- as numpy arrays, or (device=True) torch tensors on the
        context's GPU.  Needs no scene."""
        mask_a = _class_mask(a)
        mask_b = ((1 << _ffi.RM_SURF_CLASSES) - 1) & ~mask_a if b is None else _class_mask(b)
        if mask_a == 0 or mask_b == 0 or mask_a & mask_b:
            raise ValueError("the class sets %r and %r must be disjoint and not empty" % (a, b))
        nx, ny, nz, ptr, is_device, stream, keep = self._occupancy_arg(classes)
        o, s, _, fp = self._lattice(origin, step, (nx, ny, nz), 2)
        counts, stats = (C.c_uint64 * _ffi.RM_CMESH_COUNTS)(), (C.c_uint64 * _ffi.RM_CMESH_STATS)()
        fn = self._L.rm_mesh_classes
        self._check(fn(self._h, nx, ny, nz, ptr, is_device, stream, fp(o), fp(s), mask_a, mask_b, counts, _ffi.RM_CMESH_COUNTS, stats,
                       _ffi.RM_CMESH_STATS))
        self._advance(fn, "class_mesh")
        del keep
        return ClassMesh(self, _named(counts, _ffi.CMESH_COUNT_NAMES), _named(stats, _ffi.CMESH_STAT_NAMES), o, s, (nx, ny, nz), device)

    def read_class_mesh_device(self, vertices_ptr=0, triangles_ptr=0, ids_ptr=0, stream=None):
        """rm_read_class_mesh of the last mesh_classes into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_class_mesh, (vertices_ptr, triangles_ptr, ids_ptr), True, stream)

    # -- retained results (rm_read_*) ------------------------------------------------------------------------------------------
    # rm_read_* copies the size of the CONTEXT's last result, whatever the caller allocated.  So every read goes through _read_into,
    # and the result objects that read on demand (_Retained) are held to a serial per family: _advance moves it on when a producing
    # call has returned RM_OK (after a call that failed late the library itself refuses reads), and an object made under an earlier
    # serial refuses to read.  Mesh and slices are read inside their calls and need no serial.
    def _advance(self, fn, *families):
        for family in families:
            self._serials[family] = [self._serials[family][0] + 1, fn.__name__]

    def _islands_reader(self, row_capacity):
        return lambda h, rows, *rest: self._L.rm_read_islands(h, rows, int(row_capacity), *rest)    # (as _read_into calls a reader)

    def _read_into(self, fn, addresses, device=False, stream=None):
        """The one read path: fn(handle, a pointer per address, is_device, stream), status checked.  An output that is not wanted,
        or is empty, has the address 0 or None and goes as NULL."""
        self._check(fn(self._h, *[C.c_void_p(int(a) if a else None) for a in addresses], 1 if device else 0,
                       C.c_void_p(stream) if stream else None))

    def _read_new(self, fn, specs, device=False):
        """_read_into new arrays: per output (shape, numpy dtype, name of the torch dtype, wanted) of specs a numpy array, or with
        device=True a torch tensor on this context's GPU, filled on torch.cuda.current_stream(); None where not wanted."""
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            outs = [torch.empty(shape, dtype=getattr(torch, tdt), device=dev) if want else None for shape, _, tdt, want in specs]
            addresses, stream = [t.data_ptr() if t is not None and t.numel() else 0 for t in outs], torch.cuda.current_stream(dev).cuda_stream
        else:
            outs = [np.empty(shape, dtype=ndt) if want else None for shape, ndt, _, want in specs]
            addresses, stream = [a.ctypes.data if a is not None and a.size else 0 for a in outs], None
        self._read_into(fn, addresses, device, stream)
        return outs

    def _read_mesh(self, V, T, normals, ids, device):
        """rm_read_mesh of the extraction that just returned V vertices and T triangles, as a mesh.Mesh."""
        from . import mesh as _mesh
        verts, tris, nrm, idv = self._read_new(self._L.rm_read_mesh, [((V, 3), *_F32, True), ((T, 3), *_U32, True),
                                                                      ((V, 3), *_F32, normals), ((V, 2), *_U32, ids)], device)
        return _mesh.Mesh(verts, tris, nrm, idv[:, 0] if ids else None, idv[:, 1] if ids else None)

    def read_mesh_device(self, vertices_ptr=0, triangles_ptr=0, normals_ptr=0, ids_ptr=0, stream=None):
        """rm_read_mesh of the last extraction into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_mesh, (vertices_ptr, triangles_ptr, normals_ptr, ids_ptr), True, stream)

    # -- slicing (rm_slice_contours / rm_read_slices) ------------------------------------------------------------------------
    # The slicing axis w is 0, 1 or 2 (x, y, z); the in-plane axes are u = (w + 1) % 3 and v = (w + 2) % 3.
    @staticmethod
    def _slice_axis(axis):
        if isinstance(axis, str) and axis in ("x", "y", "z"):
            return "xyz".index(axis)
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= int(axis) <= 2:
            raise ValueError("axis must be 0, 1, 2 or 'x', 'y', 'z', not %r" % (axis,))
        return int(axis)

    @staticmethod
    def _slice_lattice(axis, origin_uv, step_uv, shape_uv, heights, level):
        axis = RayMarchingResources._slice_axis(axis)
        # copies: the library reads 2 floats from each address, and a broadcast or strided view does not hold them there
        o = np.array(origin_uv, dtype=np.float32, copy=True).reshape(-1)
        s = np.array(step_uv, dtype=np.float32, copy=True).reshape(-1)
        n = tuple(int(x) for x in np.asarray(shape_uv).reshape(-1))
        if o.shape != (2,) or s.shape != (2,) or len(n) != 2:
            raise ValueError("origin_uv, step_uv and shape_uv must have 2 entries each (u, v)")
        if not np.all(np.isfinite(o)) or not np.all(np.isfinite(s)) or not np.all(s > 0):
            raise ValueError("origin_uv must be finite and step_uv finite and > 0")
        if min(n) < 2:
            raise ValueError("a layer's lattice needs at least 2 points per axis, not %s" % (n,))
        h = np.array(heights, dtype=np.float32, copy=True).reshape(-1)
        if h.size < 1 or not np.all(np.isfinite(h)):
            raise ValueError("heights must be at least one finite value")
        if not np.isfinite(np.float32(level)):
            raise ValueError("level must be finite, not %r" % (level,))
        return axis, o, s, n, h

    @staticmethod
    def _layer_heights(lo_w, hi_w, layer_height):
        """Mid-layer heights lo_w + ((float)k + 0.5f) * h in float32, k = 0, 1, ... while below hi_w."""
        h = np.float32(layer_height)
        if not np.isfinite(h) or not h > 0:
            raise ValueError("layer_height must be finite and > 0, not %r" % (layer_height,))
        lo_w, hi_w = np.float32(lo_w), np.float32(hi_w)
        count = int(np.ceil((np.float64(hi_w) - np.float64(lo_w)) / np.float64(h))) + 2
        if count > (1 << 16) + 2:
            raise ValueError("layer_height %g gives more than 65536 layers between %g and %g" % (h, lo_w, hi_w))
        z = lo_w + (np.arange(count, dtype=np.float64).astype(np.float32) + np.float32(0.5)) * h
        below = z < hi_w
        z = z if below.all() else z[:int(np.argmin(below))]
        if z.size < 1:
            raise ValueError("no layer of height %g fits between %g and %g" % (h, lo_w, hi_w))
        return z

    def slice_contours(self, lo, hi, resolution, heights=None, layer_height=None, axis=1, level=0.0, normals=False, ids=False,
                       device=False):
        """The outlines of the solid map_scene < level in planes across `axis` (0, 1, 2 or "x", "y", "z"; default y, the up
        axis of the floor) inside the box [lo, hi]: a slicer.Slices.  resolution: lattice points per in-plane axis (an int,
        or (nu, nv)), over the box's extents on u = (axis + 1) % 3 and v = (axis + 2) % 3 as in extract_mesh.  Give either
        `heights` (any order, duplicates allowed) or `layer_height`: mid-layer heights lo_w + (k + 0.5) * layer_height in
        float32 while below hi_w.  Outer boundaries come counter-clockwise seen from +axis, holes clockwise; a contour is
        open where the outline leaves the box."""
        if (heights is None) == (layer_height is None):
            raise ValueError("give either heights or layer_height")
        lo3, extent, _ = self._box_lattice(lo, hi, 2)       # validates the box; with 2 points per axis the step is hi - lo
        hi3 = np.broadcast_to(np.asarray(hi, dtype=np.float32), (3,))
        axis = self._slice_axis(axis)
        u, v = (axis + 1) % 3, (axis + 2) % 3
        n = np.broadcast_to(np.asarray(resolution), (2,))
        if n.dtype.kind not in "iu" or np.any(n < 2):
            raise ValueError("resolution must be an integer of at least 2 points per in-plane axis, not %s" % (resolution,))
        lo_uv = lo3[[u, v]]
        step = extent[[u, v]] / (n.astype(np.float32) - np.float32(1.0))
        if heights is None:
            heights = self._layer_heights(lo3[axis], hi3[axis], layer_height)
        return self.slice_contours_grid(axis, lo_uv, step, n, heights, level, normals, ids, device)

    def slice_contours_grid(self, axis, origin_uv, step_uv, shape_uv, heights, level=0.0, normals=False, ids=False, device=False):
        """slice_contours on an exact lattice: point (i, j) of layer k lies at origin_uv + (i, j) * step_uv on the in-plane
        axes (float32, one rounded product and one rounded sum per coordinate) and at heights[k] on `axis`."""
        axis, o, s, (nu, nv), h = self._slice_lattice(axis, origin_uv, step_uv, shape_uv, heights, level)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        flags = (_ffi.RM_MESH_NORMALS if normals else 0) | (_ffi.RM_MESH_IDS if ids else 0)
        counts = (C.c_uint64 * _ffi.RM_SLICE_COUNTS)()
        self._check(self._L.rm_slice_contours(self._h, axis, fp(o), fp(s), nu, nv, fp(h), len(h), float(level), flags, counts,
                                              _ffi.RM_SLICE_COUNTS))
        self._advance(self._L.rm_slice_contours, "slices")
        return self._read_slices(int(counts[_ffi.RM_SLICE_POINTS]), int(counts[_ffi.RM_SLICE_CONTOURS]), axis, h, (o, s, (nu, nv)),
                                 normals, ids, device)

    def _read_slices(self, P, Cn, axis, heights, lattice, normals, ids, device):
        """rm_read_slices of the call that just returned P points and Cn contours, as a slicer.Slices."""
        from . import slicer as _slicer
        pts, con, lf, nrm, idv = self._read_new(self._L.rm_read_slices, [((P, 3), *_F32, True), ((Cn, 4), *_U32, True),
                                                                         ((len(heights) + 1,), *_U32, True), ((P, 3), *_F32, normals),
                                                                         ((P, 2), *_U32, ids)], device)
        return _slicer.Slices(pts, con, lf, heights, axis, nrm, idv[:, 0] if ids else None, idv[:, 1] if ids else None, lattice)

    # -- mesh slicing (rm_slice_mesh; the slices are read with rm_read_slices) -------------------------------------------------------
    @staticmethod
    def _mesh_extent(vertices):
        """(lo, hi) float64 (3,) over the finite coordinates of (n, 3) vertices (numpy, or a torch tensor)."""
        v = vertices.vertices if hasattr(vertices, "vertices") else vertices
        if type(v).__module__.split(".")[0] == "torch":
            import torch
            finite = torch.where(torch.isfinite(v), v, torch.full_like(v, float("nan")))
            lo = torch.nan_to_num(finite, nan=float("inf")).amin(dim=0).cpu().numpy().astype(np.float64)
            hi = torch.nan_to_num(finite, nan=float("-inf")).amax(dim=0).cpu().numpy().astype(np.float64)
        else:
            a = np.asarray(v, dtype=np.float32).reshape(-1, 3).astype(np.float64)
            a = np.where(np.isfinite(a), a, np.nan)
            with np.errstate(all="ignore"):
                lo, hi = np.nanmin(a, axis=0), np.nanmax(a, axis=0)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.max(hi - lo) > 0):
            raise ValueError("the mesh has no finite extent")
        return lo, hi

    def slice_mesh(self, vertices, triangles=None, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), axis=2, heights=None, layer_height=None,
                   device=False):
        """rm_slice_mesh: the outlines of an indexed triangle mesh in planes across `axis` (0, 1, 2 or "x", "y", "z"): a
        slicer.Slices with lattice None, and with `counts` and `stats` (dicts: _ffi.MSLICE_COUNT_NAMES, MSLICE_STAT_NAMES).
        vertices (n, 3) float32 and triangles (m, 3) indices as numpy arrays, or contiguous torch tensors on this context's GPU
        (indices int32), or a mesh.Mesh in place of both; a soup (mesh.read of an STL) goes through mesh.weld first.  origin and
        step are the resolution frame: vertices are snapped to 1 / 64 of a step from origin, as voxelize_mesh snaps them, and a
        plane lies within 1 / 128 of a step of its height.  Give either `heights` (strictly increasing planes) or `layer_height`:
        mid-layer heights over the mesh's extent on the axis.  Needs no scene.  device=True: torch tensors on the GPU."""
        if (heights is None) == (layer_height is None):
            raise ValueError("give either heights or layer_height")
        axis = self._slice_axis(axis)
        nv, xyz, nt, idx, is_device, stream, keep = self._mesh_arg(vertices, triangles)
        if keep[1] is None:
            raise ValueError("slice_mesh takes an indexed mesh: triangles are required (mesh.weld makes a soup one)")
        o = np.array(origin, dtype=np.float32, copy=True).reshape(-1)
        st = np.array(step, dtype=np.float32, copy=True).reshape(-1)
        if o.shape != (3,) or st.shape != (3,):
            raise ValueError("origin and step must have 3 entries each")
        if heights is None:
            lo, hi = self._mesh_extent(vertices)
            heights = self._layer_heights(lo[axis], hi[axis], layer_height)
        h = np.array(heights, dtype=np.float32, copy=True).reshape(-1)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        counts, stats = (C.c_uint64 * _ffi.RM_MSLICE_COUNTS)(), (C.c_uint64 * _ffi.RM_MSLICE_STATS)()
        fn = self._L.rm_slice_mesh
        self._check(fn(self._h, xyz, nv, idx, nt, is_device, stream, fp(o), fp(st), axis, fp(h), len(h), 0, counts, _ffi.RM_MSLICE_COUNTS,
                       stats, _ffi.RM_MSLICE_STATS))
        self._advance(fn, "slices")
        del keep
        s = self._read_slices(int(counts[_ffi.RM_MSLICE_POINTS]), int(counts[_ffi.RM_MSLICE_CONTOURS]), axis, h, None, False, False, device)
        s.counts, s.stats = _named(counts, _ffi.MSLICE_COUNT_NAMES), _named(stats, _ffi.MSLICE_STAT_NAMES)
        return s

    def slice_mesh_box(self, vertices, triangles=None, axis=2, layer_height=None, resolution=1024, device=False):
        """slice_mesh in a resolution frame chosen from the mesh's bounding box (over its finite coordinates), as voxelize_mesh_box
        chooses its lattice: origin at the box's lower corner, one step for all three axes, `resolution` points along the longest
        one.  Layers at the mid-layer heights lo_w + (k + 0.5) * layer_height while below hi_w."""
        resolution = int(resolution)
        if resolution < 2 or resolution > 2048:
            raise ValueError("resolution %d: 2..2048 points along the longest axis" % resolution)
        if layer_height is None:
            raise ValueError("slice_mesh_box needs a layer_height")
        lo, hi = self._mesh_extent(vertices)
        step = float(np.max(hi - lo)) / (resolution - 1)
        return self.slice_mesh(vertices, triangles, lo, (step, step, step), axis, layer_height=layer_height, device=device)

    def read_slices_device(self, points_ptr=0, contours_ptr=0, layer_first_ptr=0, normals_ptr=0, ids_ptr=0, stream=None):
        """rm_read_slices of the last slice call into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_slices, (points_ptr, contours_ptr, layer_first_ptr, normals_ptr, ids_ptr), True, stream)

    # -- hatching (rm_hatch_slices / rm_read_hatch) -------------------------------------------------------------------------------
    def hatch_slices(self, lines, n_lines, zigzag=False, device=False):
        """rm_hatch_slices: the slices this context retains -- of the last slice_contours or slice_mesh -- filled with parallel
        lines under the even-odd rule: a slicer.Hatch.  lines: (n_layers, 4) float32, (dx, dy, offset, spacing) per layer, in the
        slices' in-plane frame (u, v); n_lines lines per layer, line j at offset + j * spacing of the normal coordinate
        s = v dx - u dy (slicer.hatch_lines chooses both from an angle and a spacing).  zigzag: the segments of every other line
        reversed.  device=True: torch tensors on the GPU."""
        from . import slicer as _slicer
        l = np.array(lines, dtype=np.float32, copy=True)
        if l.ndim != 2 or l.shape[1] != 4:
            raise ValueError("lines must be (n_layers, 4): dx, dy, offset, spacing per layer")
        l = np.ascontiguousarray(l)
        counts, stats = (C.c_uint64 * _ffi.RM_HATCH_COUNTS)(), (C.c_uint64 * _ffi.RM_HATCH_STATS)()
        self._check(self._L.rm_hatch_slices(self._h, l.ctypes.data_as(C.POINTER(C.c_float)), len(l), int(n_lines),
                                            _ffi.RM_HATCH_ZIGZAG if zigzag else 0, counts, _ffi.RM_HATCH_COUNTS, stats, _ffi.RM_HATCH_STATS))
        H = int(counts[_ffi.RM_HATCH_SEGMENTS])
        seg, line, lf = self._read_new(self._L.rm_read_hatch, [((H, 4), *_F32, True), ((H,), *_U32, True), ((len(l) + 1,), *_U32, True)], device)
        return _slicer.Hatch(seg, line, lf, l, int(n_lines), _named(counts, _ffi.HATCH_COUNT_NAMES), _named(stats, _ffi.HATCH_STAT_NAMES))

    def read_hatch_device(self, segments_ptr=0, line_ptr=0, layer_first_ptr=0, stream=None):
        """rm_read_hatch of the last hatch into device memory (integer addresses; 0 = not wanted), asynchronous."""
        self._read_into(self._L.rm_read_hatch, (segments_ptr, line_ptr, layer_first_ptr), True, stream)


class RayMarchingCallback:
    """Per-frame value object (renderer.rs:177-193) with the reference's prepare/paint split."""

    def __init__(self, time, csg_node, viewport, camera):
        self.time = time            # carried, unused (renderer.rs:178; main.rs:74 always passes 0.0)
        self.csg_node = csg_node    # Option<CSGNode>
        self.viewport = viewport
        self.camera = camera

    @classmethod
    def new(cls, time, csg_node, viewport, camera):
        return cls(time, csg_node, viewport, camera)

    def prepare(self, resources):
        """renderer.rs:196-242: uniforms write, then cmd_count and words writes."""
        u = prepare_uniforms(self.viewport, self.camera)
        resources.write_buffer(_ffi.RM_BUF_UNIFORMS, 0, bytes(u))
        cmd_count, words = _csg.serialize(self.csg_node)
        resources.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.uint32(cmd_count).tobytes())
        resources.write_buffer(_ffi.RM_BUF_COMMANDS, 4, words.tobytes())

    def paint(self, resources, width=None, height=None):
        """renderer.rs:244-255: one draw over the viewport; returns (H, W, 4) float32."""
        W = int(self.viewport[0]) if width is None else width
        H = int(self.viewport[1]) if height is None else height
        return resources.draw(W, H)


# The outputs of the lattice analyses (RayMarchingResources._solid_grid_call): the families of retained results a call replaces
# (a new distance volume has no mask), how many counts and statistics, and their names.
_FAMILIES = ("topology", "distance", "distance_mask", "support", "islands", "voxels", "lattice", "class_mesh", "slices")
_TOPO_OUTPUTS = (("topology",), _ffi.RM_TOPO_COUNTS, _ffi.RM_TOPO_STATS, _ffi.TOPO_COUNT_NAMES, _ffi.TOPO_STAT_NAMES)
_DIST_OUTPUTS = (("distance", "distance_mask"), _ffi.RM_DIST_COUNTS, _ffi.RM_DIST_STATS, _ffi.DIST_COUNT_NAMES, _ffi.DIST_STAT_NAMES)
_SUP_OUTPUTS = (("support",), _ffi.RM_SUP_COUNTS, _ffi.RM_SUP_STATS, _ffi.SUP_COUNT_NAMES, _ffi.SUP_STAT_NAMES)
_ISL_OUTPUTS = (("islands",), _ffi.RM_ISL_COUNTS, _ffi.RM_ISL_STATS, _ffi.ISL_COUNT_NAMES, _ffi.ISL_STAT_NAMES)
# (no family: a surface call retains nothing; its 840 counts are named by their index)
_SURF_OUTPUTS = ((), _ffi.RM_SURF_COUNTS, _ffi.RM_SURF_STATS, tuple(range(_ffi.RM_SURF_COUNTS)), _ffi.SURF_STAT_NAMES)

# RayMarchingResources._read_new's specs: (numpy dtype, name of the torch dtype: u32 and u64 words as int32 and int64 views); _SKIP.
_F32, _U32, _U64, _U8 = (np.float32, "float32"), (np.uint32, "int32"), (np.uint64, "int64"), (np.uint8, "uint8")
_SKIP = ((0,), *_U8, False)


def _named(words, names):
    return {name: int(words[k]) for k, name in enumerate(names)}


class _Retained:
    """What the result objects that read on demand share.  They stand for the retained result of their family in their context and
    record the family's serial they were made under (RayMarchingResources._advance).  Once a newer call has replaced that result, a
    read would copy the newer one's size into arrays of this one's shape: _check_current raises ValueError before that."""

    def _retain(self, resources, family):
        self._res, self._family, self._serial = resources, family, resources._serials[family][0]

    def _check_current(self):
        serial, call = self._res._serials[self._family]
        if serial != self._serial:
            raise ValueError("%r is stale: %s has replaced the %s result of its context (now number %d, this was number %d)"
                             % (self, call, self._family.replace("_", " "), serial, self._serial))

    def _read(self, fn, position, n_outputs, dtype, shape=None):
        """Output `position` of fn's n_outputs as a new host array of `shape`; None: a volume (nz, ny, nx) of the lattice."""
        self._check_current()
        specs = [_SKIP] * n_outputs
        specs[position] = (shape or tuple(self.shape)[::-1], *dtype, True)
        return self._res._read_new(fn, specs)[position]


class MassMoments:
    """moments: uint64[16] (_ffi.RM_MOMENT_*); stats: a dict (bricks, bricks_kept, bricks_inside, evaluations, scratch_bytes);
    origin, step (float32[3]) and shape of the lattice they belong to."""

    def __init__(self, moments, stats, origin, step, shape):
        self.moments, self.stats, self.origin, self.step, self.shape = moments, stats, origin, step, shape

    def __repr__(self):
        return "MassMoments(%d inside points of %s)" % (int(self.moments[0]), "x".join(map(str, self.shape)))

    def properties(self, density=1.0):
        return mass_from_moments(self.moments, self.origin, self.step, density)


class Topology(_Retained):
    """The result of label_solid / label_occupancy.  bodies, cavities, euler, tunnels: ints; counts and stats: dicts
    (_ffi.TOPO_COUNT_NAMES, _ffi.TOPO_STAT_NAMES); body_moments (B, 16) and cavity_moments (C, 16): uint64 rows of the
    _ffi.RM_MOMENT_* words, in body and cavity order; origin, step (float32[3]) and shape of the lattice.  labels() reads the
    context's buffers: after a later labelling call of the context it raises ValueError."""

    def __init__(self, resources, counts, stats, body_moments, cavity_moments, origin, step, shape):
        self._retain(resources, "topology")
        self.counts, self.stats = counts, stats
        self.bodies, self.cavities, self.euler, self.tunnels = counts["bodies"], counts["cavities"], counts["euler"], counts["tunnels"]
        self.body_moments, self.cavity_moments = body_moments, cavity_moments
        self.origin, self.step, self.shape = origin, step, shape

    def __repr__(self):
        return "Topology(%d bodies, %d cavities, %d tunnels, euler %d on %s)" % (self.bodies, self.cavities, self.tunnels, self.euler,
                                                                               "x".join(map(str, self.shape)))

    def body_properties(self, density=1.0):
        """mass_from_moments of every body's row: a list of dicts."""
        return [mass_from_moments(row, self.origin, self.step, density) for row in self.body_moments]

    def cavity_properties(self):
        """mass_from_moments (density 1) of every cavity's row, over the cavity's outside points."""
        return [mass_from_moments(row, self.origin, self.step, 1.0) for row in self.cavity_moments]

    def labels(self):
        """The label volume, uint32 (nz, ny, nx): a body's number, _ffi.RM_TOPO_CAVITY_BIT | a cavity's number, or
        _ffi.RM_TOPO_EXTERIOR.  Read on demand."""
        return self._read(self._res._L.rm_read_topology, 2, 3, _U32)


def squared_radius(width, step):
    """The squared radius, in index units, of the ball that a wall (or gap) of `width` world units must hold: floor((width / 2 /
    step)^2).  step: one number, or three equal ones; ValueError otherwise (index distance is world distance / step only then)."""
    st = np.asarray(step, dtype=np.float64).reshape(-1)
    if st.size not in (1, 3) or not np.all(st == st[0]) or not st[0] > 0:
        raise ValueError("thickness in world units needs one step for all three axes, not %s" % (step,))
    w = float(width)
    if not w >= 0.0 or not np.isfinite(w):
        raise ValueError("a width must be finite and >= 0, not %r" % (width,))
    return int(np.floor((w / 2.0 / float(st[0])) ** 2))


class Distance(_Retained):
    """The result of distance_solid / distance_occupancy.  counts and stats: dicts (_ffi.DIST_COUNT_NAMES, _ffi.DIST_STAT_NAMES);
    origin, step (float32[3]) and shape of the lattice.  d2() and features() work on the context's buffers: after a later distance
    call of the context they raise ValueError."""

    def __init__(self, resources, counts, stats, origin, step, shape):
        self._retain(resources, "distance")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape

    def __repr__(self):
        return "Distance(%d inside points, largest inside D2 %d, on %s)" % (self.counts["points"], self.counts["max_inside"],
                                                                           "x".join(map(str, self.shape)))

    def d2(self):
        """The distance volume, uint32 (nz, ny, nx): D2 in index units, | _ffi.RM_DIST_INSIDE_BIT for an inside point."""
        return self._read(self._res._L.rm_read_distance, 0, 2, _U32)

    def inscribed_radius(self, step=None):
        """Radius (world units) and centre (i, j, k) of the largest inscribed ball: step * sqrt(max_inside) and the point of
        argmax_inside; (0.0, None) for an empty solid.  step defaults to the lattice's; ValueError when its three differ."""
        st = np.asarray(self.step if step is None else step, dtype=np.float64).reshape(-1)
        if not np.all(st == st[0]):
            raise ValueError("a radius in world units needs one step for all three axes, not %s" % (st,))
        if self.counts["points"] == 0:
            return 0.0, None
        nx, ny, _ = self.shape
        p = self.counts["argmax_inside"]
        return float(st[0]) * float(np.sqrt(self.counts["max_inside"])), (p % nx, (p // nx) % ny, p // (nx * ny))

    def features(self, r2_wall=None, r2_gap=None, wall=None, gap=None):
        """rm_distance_features: thin walls and narrow gaps.  r2_wall, r2_gap: squared radii in index units; or wall, gap: widths in
        world units (squared_radius with this lattice's step); None skips that half.  A DistanceFeatures."""
        if wall is not None:
            if r2_wall is not None:
                raise ValueError("give r2_wall or wall, not both")
            r2_wall = squared_radius(wall, self.step)
        if gap is not None:
            if r2_gap is not None:
                raise ValueError("give r2_gap or gap, not both")
            r2_gap = squared_radius(gap, self.step)
        skip = _ffi.RM_DIST_SKIP
        for r2 in (r2_wall, r2_gap):
            if r2 is not None and not 0 <= int(r2) < skip:
                raise ValueError("a squared radius must be >= 0, not %r" % (r2,))
        self._check_current()
        counts = (C.c_uint64 * _ffi.RM_DIST_FEATURE_COUNTS)()
        fn = self._res._L.rm_distance_features
        self._res._check(fn(self._res._h, *(skip if r2 is None else int(r2) for r2 in (r2_wall, r2_gap)), counts, _ffi.RM_DIST_FEATURE_COUNTS))
        self._res._advance(fn, "distance_mask")
        return DistanceFeatures(self._res, {name: int(counts[k]) for k, name in enumerate(_ffi.DIST_FEATURE_NAMES)}, r2_wall, r2_gap,
                                self.shape)


class DistanceFeatures(_Retained):
    """The result of Distance.features: counts (a dict: _ffi.DIST_FEATURE_NAMES), r2_wall and r2_gap as used (None: skipped).
    mask() reads the context's buffer: after a later features or distance call of the context it raises ValueError."""

    def __init__(self, resources, counts, r2_wall, r2_gap, shape):
        self._retain(resources, "distance_mask")
        self.counts, self.r2_wall, self.r2_gap, self.shape = counts, r2_wall, r2_gap, shape

    def mask(self):
        """The feature mask, uint8 (nz, ny, nx): 0 outside, 1 inside, 2 thin, 3 narrow (_ffi.DIST_MASK_*)."""
        return self._read(self._res._L.rm_read_distance, 1, 2, _U8)


def reach_r2(angle_deg, step_up, step_in):
    """The squared reach r2 (index units) of support_solid for a largest self-supporting overhang angle, measured from the build
    direction: a layer may step out by t = tan(angle) * step_up / step_in points per layer, and r2 = floor(t^2 + 1e-9) (tan(45
    degrees) is 0.9999999999999999 in binary64, and 45 degrees at equal steps must give 1).  step_in: the in-layer step, one
    number or two equal ones.  ValueError for unequal in-layer steps, an angle outside [0, 90) and an r2 above 255."""
    si = np.asarray(step_in, dtype=np.float64).reshape(-1)
    if si.size not in (1, 2) or not np.all(si == si[0]) or not si[0] > 0 or not float(step_up) > 0:
        raise ValueError("a reach needs one positive step for both in-layer axes and a positive step upwards, not %s and %s" % (step_in, step_up))
    a = float(angle_deg)
    if not 0.0 <= a < 90.0:
        raise ValueError("an overhang angle lies in [0, 90) degrees, not %r" % (angle_deg,))
    t = float(np.tan(np.radians(a))) * float(step_up) / float(si[0])
    r2 = int(np.floor(t * t + 1e-9))
    if r2 > 255:
        raise ValueError("%g degrees at these steps reach %d squared points; the most is 255" % (a, r2))
    return r2


def _support_args(up, r2, plate):
    """up, r2 and plate as the library takes them."""
    if isinstance(up, str):
        if up not in _ffi.UP_NAMES:
            raise ValueError("up is one of %s, not %r" % (", ".join(_ffi.UP_NAMES), up))
        up = _ffi.UP_NAMES.index(up)
    if not 0 <= int(up) < 6:
        raise ValueError("up is one of _ffi.RM_UP_* (0..5), not %r" % (up,))
    if not 0 <= int(r2) < _ffi.RM_SUPPORT_PLATE_AUTO:
        raise ValueError("a squared reach must be >= 0, not %r" % (r2,))
    if plate is not None and not 0 <= int(plate) < _ffi.RM_SUPPORT_PLATE_AUTO:
        raise ValueError("a plate is a height >= 0 or None, not %r" % (plate,))
    return int(up), int(r2), _ffi.RM_SUPPORT_PLATE_AUTO if plate is None else int(plate)


class Support(_Retained):
    """The result of support_solid / support_occupancy.  counts and stats: dicts (_ffi.SUP_COUNT_NAMES, _ffi.SUP_STAT_NAMES); up
    (_ffi.RM_UP_*), r2, and origin, step (float32[3]) and shape of the lattice.  mask() and profile() read the context's buffers:
    after a later support call of the context they raise ValueError."""

    def __init__(self, resources, counts, stats, origin, step, shape, up, r2):
        self._retain(resources, "support")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape
        self.up, self.r2 = up, r2

    def __repr__(self):
        return "Support(up %s, %d overhang points, %d support points, on %s)" % (
            _ffi.UP_NAMES[self.up], self.counts["overhang"], self.support_points, "x".join(map(str, self.shape)))

    @property
    def support_points(self):
        return self.counts["support_on_plate"] + self.counts["support_on_part"]

    @property
    def layers(self):
        """The points along the up axis."""
        return self.shape[self.up >> 1]

    def mask(self):
        """The mask, uint8 (nz, ny, nx): 0 outside, 1 inside, 2 overhang, 3 support on the plate, 4 support on the part
        (_ffi.SUP_MASK_*)."""
        return self._read(self._res._L.rm_read_support, 0, 2, _U8)

    def profile(self):
        """The profile, uint32 (layers, 4), height 0 first: per layer its inside points, overhang points, support points on the
        plate and support points on the part."""
        return self._read(self._res._L.rm_read_support, 1, 2, _U32, (self.layers, 4))

    def volume(self):
        """The support material in world units: the support points times the volume of a cell."""
        return self.support_points * float(np.prod(np.asarray(self.step, dtype=np.float64)))

    def contact_area(self):
        """The area (world units) over which supports touch the part: the runs (a support's top under an overhang point) and the
        landings (its foot on the part), times the area of a cell of a layer."""
        st = np.asarray(self.step, dtype=np.float64)
        return (self.counts["runs"] + self.counts["landings"]) * float(np.prod(np.delete(st, self.up >> 1)))


ISL_ROW_DTYPE = np.dtype([(name, np.uint32) for name in _ffi.ISL_ROW_NAMES])


def island_roots(rows):
    """For every region (row r - 1 for region r) the number of the island or base region it grows from, following BELOW_MIN
    downwards: one pass, because the rows are sorted by layer.  int64 (REGIONS,)."""
    below = np.asarray(rows["below_min"] if getattr(rows, "dtype", None) is not None and rows.dtype.names else
                       np.asarray(rows)[:, _ffi.ISL_ROW_NAMES.index("below_min")], dtype=np.int64)
    root = np.zeros(len(below) + 1, dtype=np.int64)
    for r in range(1, len(below) + 1):
        root[r] = root[below[r - 1]] if below[r - 1] else r
    return root[1:]


class Islands(_Retained):
    """The result of islands_solid / islands_occupancy.  counts and stats: dicts (_ffi.ISL_COUNT_NAMES, _ffi.ISL_STAT_NAMES); up
    (_ffi.RM_UP_*), r2, and origin, step (float32[3]) and shape of the lattice.  rows(), labels(), mask() and profile() read the
    context's buffers: after a later islands call of the context they raise ValueError."""

    def __init__(self, resources, counts, stats, origin, step, shape, up, r2):
        self._retain(resources, "islands")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape
        self.up, self.r2 = up, r2

    def __repr__(self):
        return "Islands(up %s, %d regions, %d islands of %d points, on %s)" % (
            _ffi.UP_NAMES[self.up], self.counts["regions"], self.counts["islands"], self.counts["island_points"],
            "x".join(map(str, self.shape)))

    @property
    def layers(self):
        """The points along the up axis."""
        return self.shape[self.up >> 1]

    def _read_islands(self, position, dtype, shape=None):
        return self._read(self._res._islands_reader(self.counts["regions"]), position, 4, dtype, shape)

    def rows(self):
        """The region table, a structured array (REGIONS,) of uint32 fields _ffi.ISL_ROW_NAMES; row r - 1 is region r.  a and b
        are the two in-layer axes in ascending axis order (up z: x and y)."""
        return self._read_islands(0, (ISL_ROW_DTYPE, None), (self.counts["regions"],))

    def labels(self):
        """The label volume, uint32 (nz, ny, nx): the region's number for inside points at or above the plate, 0 elsewhere."""
        return self._read_islands(1, _U32)

    def mask(self):
        """The mask, uint8 (nz, ny, nx): 0 outside, 1 inside, 2 inside and in an island (_ffi.ISL_MASK_*)."""
        return self._read_islands(2, _U8)

    def profile(self):
        """The profile, uint32 (layers, 4), height 0 first: per layer its inside points, regions, islands and island points."""
        return self._read_islands(3, _U32, (self.layers, 4))

    def roots(self, rows=None):
        """island_roots of the region table."""
        return island_roots(self.rows() if rows is None else rows)

    def islands(self, rows=None):
        """Per island a dict: its region number, layer, points, centroid (world x, y, z) and area (world units: points times the
        area of a cell of a layer)."""
        rows = self.rows() if rows is None else rows
        a = self.up >> 1
        b, c = [ax for ax in range(3) if ax != a]
        o, st = np.asarray(self.origin, dtype=np.float64), np.asarray(self.step, dtype=np.float64)
        out = []
        for r in np.flatnonzero((rows["layer"] > self.counts["plate"]) & (rows["below_min"] == 0)):
            row = rows[r]
            idx = np.zeros(3)
            idx[a] = self.layers - 1 - int(row["layer"]) if self.up & 1 else int(row["layer"])
            idx[b], idx[c] = row["sum_a"] / row["points"], row["sum_b"] / row["points"]
            out.append({"region": int(r) + 1, "layer": int(row["layer"]), "points": int(row["points"]),
                        "centroid": [float(x) for x in o + idx * st], "area": float(row["points"] * st[b] * st[c])})
        return out


class Voxels(_Retained):
    """The result of voxelize_mesh / voxelize_mesh_box.  counts and stats: dicts (_ffi.VOX_COUNT_NAMES: triangles, rejected,
    edge_on, crossings, inside, open_rows; _ffi.VOX_STAT_NAMES); origin, step (float32[3]) and shape of the lattice.  open_rows > 0:
    the mesh is not closed along that many rows.  occupancy() and occupancy_device() read the context's buffer: after a later
    voxelisation of the context they raise ValueError."""

    def __init__(self, resources, counts, stats, origin, step, shape):
        self._retain(resources, "voxels")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape

    def __repr__(self):
        return "Voxels(%d inside points, %d open rows, on %s)" % (self.counts["inside"], self.counts["open_rows"],
                                                                  "x".join(map(str, self.shape)))

    def occupancy(self):
        """The occupancy, uint8 (nz, ny, nx) of 0 and 1: what the *_occupancy calls and surface_classes take."""
        return self._read(self._res._L.rm_read_voxels, 0, 1, _U8)

    def occupancy_device(self):
        """occupancy() as a torch tensor on the context's GPU, filled on torch.cuda.current_stream() without a host round trip."""
        self._check_current()
        return self._res._read_new(self._res._L.rm_read_voxels, [(tuple(self.shape)[::-1], *_U8, True)], device=True)[0]


class Lattice(_Retained):
    """The result of set_lattice: the lattice draw_lattice and cast_lattice of its context show until the next set_lattice.
    counts and stats: dicts (_ffi.LAT_COUNT_NAMES: points, bricks; _ffi.LAT_STAT_NAMES); origin, step (float32[3]) and shape."""

    def __init__(self, resources, counts, stats, origin, step, shape):
        self._retain(resources, "lattice")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape

    def __repr__(self):
        return "Lattice(%d points in %d bricks, on %s)" % (self.counts["points"], self.counts["bricks"], "x".join(map(str, self.shape)))

    def current(self):
        """Whether this is still the lattice its context draws."""
        try:
            self._check_current()
        except ValueError:
            return False
        return True

    def box(self):
        """The lattice's box in world space, (lo, hi) float64[3]: the cubes' outer faces."""
        o, s = self.origin.astype(np.float64), self.step.astype(np.float64)
        return o - 0.5 * s, o + (np.asarray(self.shape, dtype=np.float64) - 0.5) * s


def surface_directions():
    """rm_surface_directions: the 13 directions of the pair counts, int32 (13, 3) of (x, y, z) (host code, no GPU)."""
    out = np.zeros((_ffi.RM_SURF_DIRS, 3), dtype=np.int32)
    rc = _ffi.hip_lib().rm_surface_directions(out.ctypes.data_as(C.POINTER(C.c_int)), out.size)
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, "rm_surface_directions: " + _ffi.hip_lib().rm_status_string(rc).decode())
    return out


def _class_mask(classes):
    """A set of classes as rm_surface_measures takes it: one class, or an iterable of classes -> the bit mask."""
    members = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
    if any(not 0 <= int(a) < _ffi.RM_SURF_CLASSES for a in members):
        raise ValueError("a class is 0..%d, not %r" % (_ffi.RM_SURF_CLASSES - 1, classes))
    mask = 0
    for a in members:
        mask |= 1 << int(a)
    return mask


def surface_measures(counts, step, a, b, raw=False):
    """rm_surface_measures (host code, no GPU): the interface between the class sets a and b (a class, or an iterable of
    classes; disjoint, not empty) from the 840 counts of a surface call and the lattice's step -> a dict
    (_ffi.SURF_MEASURE_NAMES): area (the Cauchy-Crofton estimate; NaN unless the three steps are equal), facet_area and the six
    facet areas by orientation from a into b (exact staircase areas).  raw=True: the float64[8] array in _ffi.RM_SURF_* order."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    s = np.array(step, dtype=np.float32, copy=True).reshape(-1)
    if s.shape != (3,):
        raise ValueError("step must have 3 entries (x, y, z)")
    out = np.zeros(_ffi.RM_SURF_MEASURES, dtype=np.float64)
    rc = _ffi.hip_lib().rm_surface_measures(c.ctypes.data_as(C.POINTER(C.c_uint64)), len(c), s.ctypes.data_as(C.POINTER(C.c_float)),
                                            _class_mask(a), _class_mask(b), out.ctypes.data_as(C.POINTER(C.c_double)), len(out))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, "rm_surface_measures: " + _ffi.hip_lib().rm_status_string(rc).decode())
    return out if raw else {name: float(out[k]) for k, name in enumerate(_ffi.SURF_MEASURE_NAMES)}


class ClassMesh(_mesh.Mesh, _Retained):
    """The result of mesh_classes: a mesh.Mesh (vertices (V, 3) float32, triangles (T, 3), normals None) with counts and stats
    (dicts: _ffi.CMESH_COUNT_NAMES, _ffi.CMESH_STAT_NAMES), origin, step (float32[3]) and shape of the lattice, and per triangle
    face_classes (T, 2: the class on the a side and on the b side), face (2 axis + (normal positive)) and face_point (the linear
    index i + nx (j + ny k) of the a-side point, _ffi.RM_NO_ID for padding).  read() reads the context's buffers again: after a
    later mesh_classes of the context it raises ValueError."""

    def __init__(self, resources, counts, stats, origin, step, shape, device=False):
        self._retain(resources, "class_mesh")
        self.counts, self.stats = counts, stats
        self.origin, self.step, self.shape = origin, step, shape
        _mesh.Mesh.__init__(self, None, None)
        self.read(device)

    def __repr__(self):
        return "ClassMesh(%d vertices, %d triangles, on %s)" % (self.counts["vertices"], self.counts["triangles"],
                                                                "x".join(map(str, self.shape)))

    def read(self, device=False):
        """rm_read_class_mesh into new arrays of this mesh (numpy, or torch tensors on the context's GPU); returns self."""
        self._check_current()
        V, T = self.counts["vertices"], self.counts["triangles"]
        self.vertices, self.triangles, ids = self._res._read_new(self._res._L.rm_read_class_mesh,
                                                                 [((V, 3), *_F32, True), ((T, 3), *_U32, True), ((T, 2), *_U32, True)], device)
        word = ids[:, 0]
        self.face_classes = ids.new_empty((T, 2)) if device else np.empty((T, 2), dtype=np.uint32)
        self.face_classes[:, 0], self.face_classes[:, 1] = word & 0xFF, (word >> 8) & 0xFF
        self.face, self.face_point, self.ids = word >> 16, ids[:, 1], ids
        return self


class Surface:
    """The result of surface_solid / surface_classes.  points: uint64[8], the lattice points per class; pairs: uint64 (8, 8, 13),
    pairs[a, b, nu] the pairs (p, p + nu) with class(p) = a and class(p + nu) = b (surface_directions() gives nu); counts: the
    840 words as the library wrote them; stats: a dict (_ffi.SURF_STAT_NAMES); origin, step (float32[3]) and shape of the
    lattice.  Nothing of it lives in the context."""

    def __init__(self, counts, stats, origin, step, shape):
        self.counts = np.array([counts[k] for k in range(_ffi.RM_SURF_COUNTS)], dtype=np.uint64)
        self.points = self.counts[_ffi.RM_SURF_POINTS:_ffi.RM_SURF_POINTS + _ffi.RM_SURF_CLASSES]
        self.pairs = self.counts[_ffi.RM_SURF_PAIRS:].reshape(_ffi.RM_SURF_CLASSES, _ffi.RM_SURF_CLASSES, _ffi.RM_SURF_DIRS)
        self.stats, self.origin, self.step, self.shape = stats, origin, step, shape

    def __repr__(self):
        return "Surface(%s points per class on %s)" % (" ".join(str(int(x)) for x in self.points), "x".join(map(str, self.shape)))

    def measures(self, a, b, step=None):
        """surface_measures of the interface between the class sets a and b, on this lattice's step (or `step`: that of the
        lattice a caller's classes came from)."""
        return surface_measures(self.counts, self.step if step is None else step, a, b)


MASS_PROP_NAMES = ("volume", "mass", "cx", "cy", "cz", "ixx", "iyy", "izz", "ixy", "iyz", "ixz", "lo_x", "lo_y", "lo_z", "hi_x", "hi_y",
                   "hi_z")


def mass_from_moments(moments, origin, step, density=1.0, raw=False):
    """rm_mass_from_moments (host code, no GPU): the moments of mass_moments on the lattice (origin, step) -> a dict with volume,
    mass, centroid (3), inertia (3 x 3, about the centroid), bbox_lo and bbox_hi (3 each: the outermost inside points), all float64
    by the midpoint rule.  raw=True: the float64[17] array in _ffi.RM_MASS_* order instead."""
    m = np.ascontiguousarray(moments, dtype=np.uint64).reshape(-1)
    o = np.array(origin, dtype=np.float32, copy=True).reshape(-1)
    s = np.array(step, dtype=np.float32, copy=True).reshape(-1)
    if o.shape != (3,) or s.shape != (3,):
        raise ValueError("origin and step must have 3 entries each (x, y, z)")
    out = np.zeros(_ffi.RM_MASS_PROPS, dtype=np.float64)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = _ffi.hip_lib().rm_mass_from_moments(m.ctypes.data_as(C.POINTER(C.c_uint64)), len(m), fp(o), fp(s), float(density),
                                             out.ctypes.data_as(C.POINTER(C.c_double)), len(out))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, "rm_mass_from_moments: " + _ffi.hip_lib().rm_status_string(rc).decode())
    if raw:
        return out
    ixx, iyy, izz, ixy, iyz, ixz = (float(x) for x in out[_ffi.RM_MASS_IXX:_ffi.RM_MASS_IXZ + 1])
    return {"volume": float(out[_ffi.RM_MASS_VOLUME]), "mass": float(out[_ffi.RM_MASS_MASS]),
            "centroid": out[_ffi.RM_MASS_CX:_ffi.RM_MASS_CZ + 1].copy(),
            "inertia": np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]]),
            "bbox_lo": out[_ffi.RM_MASS_LO_X:_ffi.RM_MASS_LO_Z + 1].copy(), "bbox_hi": out[_ffi.RM_MASS_HI_X:_ffi.RM_MASS_HI_Z + 1].copy()}


def lighting_defaults():
    """rm_lighting_defaults: the 13 default lighting parameters in _ffi.LIGHT_NAMES order (pure host code, no GPU needed)."""
    out = (C.c_float * _ffi.RM_LIGHT_PARAMS)()
    rc = _ffi.hip_lib().rm_lighting_defaults(out, _ffi.RM_LIGHT_PARAMS)
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, _ffi.hip_lib().rm_status_string(rc).decode())
    return [float(v) for v in out]


def trace_defaults():
    """rm_trace_defaults: the 6 default traversal parameters in _ffi.TRACE_PARAM_NAMES order (pure host code, no GPU needed)."""
    out = (C.c_float * _ffi.RM_TRACE_PARAMS)()
    rc = _ffi.hip_lib().rm_trace_defaults(out, _ffi.RM_TRACE_PARAMS)
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, _ffi.hip_lib().rm_status_string(rc).decode())
    return [float(v) for v in out]


def validate_program(cmd_count, words):
    """rm_validate_program: (status, max_depth); pure host code, no GPU needed."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    depth = C.c_uint32(0)
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    rc = _ffi.hip_lib().rm_validate_program(int(cmd_count), ptr, int(w.size), C.byref(depth))
    return rc, depth.value


def program_subtree(cmd_count, words, index):
    """rm_program_subtree: (first, count), the range of command indices that produce the value command `index` leaves on
    the stack -- the selection of that graph node for draw_gbuffer (pure host code, no GPU needed)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    first, count = C.c_uint32(0), C.c_uint32(0)
    rc = _ffi.hip_lib().rm_program_subtree(int(cmd_count), ptr, int(w.size), int(index), C.byref(first), C.byref(count))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, _ffi.hip_lib().rm_status_string(rc).decode())
    return first.value, count.value


def program_lipschitz(cmd_count, words):
    """rm_program_lipschitz: L with |map_scene(p) - map_scene(q)| <= L |p - q| in real arithmetic, or inf when the program
    has no such bound (a parameter that is not finite, a Scale of 0); pure host code, no GPU needed."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    out = C.c_double(0.0)
    rc = _ffi.hip_lib().rm_program_lipschitz(int(cmd_count), ptr, int(w.size), C.byref(out))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, _ffi.hip_lib().rm_status_string(rc).decode())
    return out.value


def selection_overlay(image, selected_mask, n_samples, colour, alpha=0.5):
    """Highlights a selection (pure numpy): blends `colour` (r, g, b) into a copy of the RGBA32F `image` (rows, W, 4) by
    alpha * popcount(selected_mask) / n_samples per pixel, i.e. with the image's own anti-aliasing at the selection's edge.
    selected_mask: draw_gbuffer's, of the same rows; n_samples: 16 for RM_SAMPLE_ALL, 1 for a single sample."""
    img = np.array(image, dtype=np.float32, copy=True)
    m = np.asarray(selected_mask).astype(np.uint32)
    if img.ndim != 3 or img.shape[2] != 4 or m.shape != img.shape[:2]:
        raise ValueError("image must be (rows, W, 4) and selected_mask (rows, W)")
    bits = np.zeros(m.shape, dtype=np.float32)
    for b in range(17):   # sample ids 0..16
        bits += ((m >> np.uint32(b)) & np.uint32(1)).astype(np.float32)
    cover = (np.float32(alpha) * bits / np.float32(n_samples))[..., None]
    img[..., :3] = img[..., :3] * (np.float32(1.0) - cover) + np.asarray(colour, dtype=np.float32)[:3] * cover
    return img


PROGRAM_FACTS = ("records", "cones", "slabs", "subtracted_leaves", "groups", "spill_depth", "is_chain", "prunable", "bound_walk",
                 "has_xforms", "leaves", "auto_pruned")


def program_info(cmd_count, words):
    """rm_program_info: what the upload-time decoder makes of a command stream, as a dict (pure host code, no GPU needed)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    out = (C.c_uint32 * len(PROGRAM_FACTS))()
    rc = _ffi.hip_lib().rm_program_info(int(cmd_count), ptr, int(w.size), out, len(PROGRAM_FACTS))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, _ffi.hip_lib().rm_status_string(rc).decode())
    return dict(zip(PROGRAM_FACTS, [int(v) for v in out]))


def jit_source(cmd_count, words, waves_per_tile=4, prune=False, env=None):
    """rm_jit_source: the HIP source the structure specialiser generates for a command stream (no GPU needed).
    env: A/B knobs of the generator (RM_JIT_*), set in the process environment for this call only."""
    if env:
        import os
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return jit_source(cmd_count, words, waves_per_tile, prune)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    L = _ffi.hip_lib()
    need = C.c_size_t(0)
    waves_per_tile = int(waves_per_tile) | (_ffi.RM_JIT_PRUNE if prune else 0)
    rc = L.rm_jit_source(int(cmd_count), ptr, int(w.size), int(waves_per_tile), None, 0, C.byref(need))
    if rc != _ffi.RM_OK:
        raise _ffi.RmError(rc, L.rm_status_string(rc).decode())
    buf = C.create_string_buffer(need.value)
    L.rm_jit_source(int(cmd_count), ptr, int(w.size), int(waves_per_tile), buf, need.value, None)
    return buf.value.decode()


def jit_compile(cmd_count, words, waves_per_tile=4, prune=False, range_proved=False):
    """rm_jit_compile: compile the specialised kernel for gfx950 with hipRTC, without loading it (no GPU needed).
    range_proved: the variant without the per-lane range guards (RM_INFO_RANGE_PROOF), for the programs that get one.
    Returns (status, compile_ms, code_bytes, log)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    ptr = w.ctypes.data_as(C.POINTER(C.c_uint32)) if w.size else None
    ms, nbytes = C.c_double(0.0), C.c_size_t(0)
    log = C.create_string_buffer(1 << 16)
    waves_per_tile = int(waves_per_tile) | (_ffi.RM_JIT_PRUNE if prune else 0) | (_ffi.RM_JIT_RANGE_PROVED if range_proved else 0)
    rc = _ffi.hip_lib().rm_jit_compile(int(cmd_count), ptr, int(w.size), int(waves_per_tile), C.byref(ms),
                                       C.byref(nbytes), log, len(log))
    return rc, ms.value, nbytes.value, log.value.decode(errors="replace")
