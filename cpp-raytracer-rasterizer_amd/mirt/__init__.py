"""mirt -- thin ctypes binding of the C-ABI in include/mirt.h (libmirt.so, hand-written gfx950 kernels).

This module is plumbing for tests and bench.py: it marshals numpy arrays (or device pointers of torch
tensors) into the C entry points.  There is no Python/CPU implementation of the render path here and no
fallback: if libmirt.so is missing or no MI355X is visible, the calls raise MirtError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libmirt.so")

MAX_LIGHTS = 32
MAX_ORDERED_HITS = 8                  # hits per ray and call of intersect_ordered (MIRT_MAX_ORDERED_HITS)
MAX_LIGHT_POSITIONS = 256             # lights x soft-shadow samples (MIRT_MAX_LIGHT_POSITIONS: randomPositions[256], raytracer.cpp:84)
RT_AUTO, RT_BRUTE, RT_BINNED = 0, 1, 2
QUERY_AUTO, QUERY_BRUTE, QUERY_BINNED = 0, 1, 2
KERNEL_NAMES = ("prep", "bin", "trace", "dof", "raster_setup", "raster_frag", "raster_resolve", "clear")

# every symbol include/mirt.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = (
    "mirt_init", "mirt_shutdown", "mirt_last_error", "mirt_abi_version", "mirt_set_profiling", "mirt_sync",
    "mirt_stream", "mirt_scene_upload", "mirt_scene_set_culled", "mirt_scene_size", "mirt_scene_cornell",
    "mirt_scene_soup", "mirt_scene_load_stl", "mirt_cull", "mirt_cull_device", "mirt_scene_get_culled", "mirt_set_soft_shadows", "mirt_set_antialiasing", "mirt_set_depth_of_field", "mirt_set_frames_in_flight", "mirt_raytrace", "mirt_raytrace_device", "mirt_raytrace_ex", "mirt_raytrace_device_ex", "mirt_rasterise",
    "mirt_rasterise_device", "mirt_get_stats", "mirt_get_previous_kernel_ms", "mirt_surface_register", "mirt_surface_unregister", "mirt_raytrace_async", "mirt_rasterise_async",
    "mirt_band_of", "mirt_band_plan", "mirt_set_partition", "mirt_partition_segments", "mirt_partition_plan",
    "mirt_set_cost_histogram", "mirt_cost_histogram", "mirt_weighted_bounds", "mirt_partition_bounds", "mirt_bounds_plan", "mirt_comm_create_id", "mirt_comm_init", "mirt_comm_shutdown", "mirt_comm_selfcheck", "mirt_raytrace_sharded", "mirt_rasterise_sharded",
    "mirt_intersect", "mirt_intersect_device", "mirt_direct_light", "mirt_direct_light_device",
    "mirt_set_query_mode", "mirt_get_query_stats",
    "mirt_intersect_from", "mirt_intersect_from_device", "mirt_get_fan_stats",
    "mirt_intersect_fans", "mirt_intersect_fans_device",
    "mirt_occluded", "mirt_occluded_device", "mirt_occluded_fans", "mirt_occluded_fans_device", "mirt_get_occlusion_stats",
    "mirt_intersect_along", "mirt_intersect_along_device", "mirt_occluded_along", "mirt_occluded_along_device", "mirt_get_along_stats",
    "mirt_intersect_alongs", "mirt_intersect_alongs_device", "mirt_occluded_alongs", "mirt_occluded_alongs_device",
    "mirt_set_ray_grid", "mirt_get_ray_grid_stats",
    "mirt_intersect_ordered", "mirt_intersect_ordered_device",
    "mirt_intersect_ordered_along", "mirt_intersect_ordered_along_device", "mirt_intersect_ordered_alongs", "mirt_intersect_ordered_alongs_device",
    "mirt_intersect_ordered_from", "mirt_intersect_ordered_from_device", "mirt_intersect_ordered_fans", "mirt_intersect_ordered_fans_device",
    "mirt_count_hits", "mirt_count_hits_device", "mirt_count_hits_along", "mirt_count_hits_along_device", "mirt_count_hits_alongs", "mirt_count_hits_alongs_device",
    "mirt_shadow_mask", "mirt_shadow_mask_device", "mirt_direct_light_masked", "mirt_direct_light_masked_device", "mirt_get_shadow_mask_stats",
    "mirt_scene_upload_device", "mirt_scene_update_device", "mirt_scene_update", "mirt_scene_transform", "mirt_transform",
    "mirt_scene_download", "mirt_scene_info",
    "mirt_scene_set_objects", "mirt_scene_pose", "mirt_pose",
    "mirt_set_supersampled_many_lights", "mirt_get_supersample_stats",
    "mirt_get_shadowed",
)


_soft_samples = 1                     # samples per light of the last successful set_soft_shadows (1: hard shadows)


class MirtError(RuntimeError):
    pass


class View(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("rot", C.c_float * 9), ("focal", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class Light(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("color", C.c_float * 3), ("intensity", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("tests", C.c_uint64),
                ("gpu_ms", C.c_float), ("kernel_ms", C.c_float * 8), ("mode_used", C.c_int32), ("candidates", C.c_uint64),
                ("steps_primary", C.c_uint64), ("steps_shadow", C.c_uint64), ("drains", C.c_uint64),
                ("bins_reused", C.c_uint32), ("selected_triangles", C.c_uint32)]


class QueryStats(C.Structure):
    """mirt_query_stats: how the last DirectLight query was answered."""
    _fields_ = [("mode_used", C.c_int32), ("cube_source", C.c_int32), ("cube_bins", C.c_int32), ("shells", C.c_int32),
                ("shadow_rays", C.c_uint64), ("candidates", C.c_uint64), ("tests", C.c_uint64), ("fallback_records", C.c_uint64)]


class RayGridStats(C.Structure):
    """mirt_ray_grid_stats: how the last mirt_intersect* / mirt_occluded* call under set_ray_grid(True) was answered."""
    _fields_ = [("mode_used", C.c_int32), ("source", C.c_int32), ("gave_up", C.c_int32), ("cells", C.c_int32), ("plane_bins", C.c_int32),
                ("offset_bins", C.c_int32), ("pairs", C.c_uint32), ("plane_pairs", C.c_uint32), ("every_rows", C.c_uint32), ("reserved", C.c_uint32),
                ("rays", C.c_uint64), ("rows_cells", C.c_uint64), ("rows_planes", C.c_uint64), ("rows_every", C.c_uint64), ("tests", C.c_uint64),
                ("swept_rays", C.c_uint64)]


class Ray(C.Structure):
    """mirt_ray: the `start` and `dir` arguments of one ClosestIntersection call (24 bytes)."""
    _fields_ = [("start", C.c_float * 3), ("dir", C.c_float * 3)]


class Hit(C.Structure):
    """mirt_hit == struct Intersection (raytracer.cpp:91-96): position, distance, triangleIndex (20 bytes)."""
    _fields_ = [("position", C.c_float * 3), ("distance", C.c_float), ("index", C.c_int32)]


class SceneInfo(C.Structure):
    """struct mirt_scene_info: the values the library decides with (40 bytes)."""
    _fields_ = [("n", C.c_int32), ("finite", C.c_int32), ("bbox_lo", C.c_float * 3), ("bbox_hi", C.c_float * 3),
                ("version", C.c_uint64)]


class Object(C.Structure):
    """mirt_object: rest rows [rest_first, rest_first + count) pose into scene rows [scene_first, scene_first + count) (12 bytes)."""
    _fields_ = [("rest_first", C.c_int32), ("scene_first", C.c_int32), ("count", C.c_int32)]


# the same two layouts for numpy: arrays of rays / hit records travel as they are
RAY_DTYPE = np.dtype([("start", np.float32, 3), ("dir", np.float32, 3)])
HIT_DTYPE = np.dtype([("position", np.float32, 3), ("distance", np.float32), ("index", np.int32)])

_vp = C.c_void_p
_lib = None


def load():
    """Loads libmirt.so (raises MirtError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirtError("libmirt.so not built: run `make -C cpp-raytracer-rasterizer_amd` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    lib.mirt_last_error.restype = C.c_char_p
    lib.mirt_stream.restype = _vp
    lib.mirt_init.argtypes = [C.c_int]
    lib.mirt_set_profiling.argtypes = [C.c_int]
    lib.mirt_scene_upload.argtypes = [_vp, _vp, C.c_int]
    lib.mirt_scene_set_culled.argtypes = [_vp, C.c_int]
    lib.mirt_scene_cornell.argtypes = [_vp]
    lib.mirt_scene_soup.argtypes = [C.c_uint32, C.c_int, C.c_float, _vp]
    lib.mirt_cull.argtypes = [_vp, C.c_int, C.POINTER(View), C.c_int, _vp]
    lib.mirt_cull_device.argtypes = [C.POINTER(View), C.c_int]
    lib.mirt_scene_get_culled.argtypes = [_vp, C.c_int]
    lib.mirt_scene_load_stl.argtypes = [C.c_char_p, C.c_float, _vp, _vp, C.c_int]
    lib.mirt_set_soft_shadows.argtypes = [C.c_int, _vp, C.c_int]
    lib.mirt_set_depth_of_field.argtypes = [C.c_int, C.c_float]
    lib.mirt_set_supersampled_many_lights.argtypes = [C.c_int]
    lib.mirt_get_supersample_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mirt_set_frames_in_flight.argtypes = [C.c_int]
    lib.mirt_raytrace.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_raytrace_device.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _vp, C.c_int, _vp, _vp]
    lib.mirt_raytrace_ex.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]
    lib.mirt_raytrace_device_ex.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _vp, C.c_int, _vp, _vp, _vp, _vp]
    lib.mirt_rasterise.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_rasterise_device.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                          _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_get_stats.argtypes = [C.POINTER(Stats)]
    lib.mirt_get_previous_kernel_ms.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mirt_surface_register.argtypes = [_vp, C.c_size_t]
    lib.mirt_surface_unregister.argtypes = [_vp]
    lib.mirt_raytrace_async.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, C.c_int, _vp, C.c_int]
    lib.mirt_rasterise_async.argtypes = [C.POINTER(View), _vp, C.c_int, _vp, _vp, C.c_int]
    lib.mirt_band_of.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mirt_band_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int]
    lib.mirt_set_partition.argtypes = [C.c_int]
    lib.mirt_partition_segments.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int]
    lib.mirt_partition_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int]
    lib.mirt_set_cost_histogram.argtypes = [C.c_int]
    lib.mirt_cost_histogram.argtypes = [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mirt_weighted_bounds.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
    lib.mirt_partition_bounds.argtypes = [C.c_int, C.c_int, C.c_int, _vp]
    lib.mirt_bounds_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
    lib.mirt_comm_create_id.argtypes = [_vp]
    lib.mirt_comm_init.argtypes = [_vp, C.c_int, C.c_int]
    lib.mirt_comm_selfcheck.argtypes = [C.c_size_t]
    lib.mirt_raytrace_sharded.argtypes = [C.POINTER(View), C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int]
    lib.mirt_rasterise_sharded.argtypes = [C.POINTER(View), C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int]
    lib.mirt_intersect.argtypes = [_vp, C.c_int, _vp]
    lib.mirt_intersect_device.argtypes = [_vp, C.c_int, _vp]
    lib.mirt_direct_light.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp]
    lib.mirt_direct_light_device.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp]
    lib.mirt_set_query_mode.argtypes = [C.c_int]
    lib.mirt_get_query_stats.argtypes = [C.POINTER(QueryStats)]
    lib.mirt_intersect_from.argtypes = [_vp, _vp, C.c_int, _vp]
    lib.mirt_intersect_from_device.argtypes = [_vp, _vp, C.c_int, _vp]
    lib.mirt_get_fan_stats.argtypes = [C.POINTER(QueryStats)]
    lib.mirt_intersect_fans.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp]
    lib.mirt_intersect_fans_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp]
    lib.mirt_occluded.argtypes = [_vp, C.c_int, _vp, _vp]
    lib.mirt_occluded_device.argtypes = [_vp, C.c_int, _vp, _vp]
    lib.mirt_occluded_fans.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_occluded_fans_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_get_occlusion_stats.argtypes = [C.POINTER(QueryStats)]
    lib.mirt_intersect_along.argtypes = [_vp, _vp, C.c_int, _vp]
    lib.mirt_intersect_along_device.argtypes = [_vp, _vp, C.c_int, _vp]
    lib.mirt_occluded_along.argtypes = [_vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_occluded_along_device.argtypes = [_vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_get_along_stats.argtypes = [C.POINTER(QueryStats)]
    lib.mirt_set_ray_grid.argtypes = [C.c_int]
    lib.mirt_get_ray_grid_stats.argtypes = [C.POINTER(RayGridStats)]
    lib.mirt_intersect_ordered.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_device.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_along.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_along_device.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_alongs.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_alongs_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_from.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_from_device.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_fans.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_intersect_ordered_fans_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_count_hits.argtypes = [_vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_count_hits_device.argtypes = [_vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_count_hits_along.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_count_hits_along_device.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_count_hits_alongs.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_count_hits_alongs_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp]
    lib.mirt_intersect_alongs.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp]
    lib.mirt_intersect_alongs_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp]
    lib.mirt_occluded_alongs.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_occluded_alongs_device.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]
    lib.mirt_shadow_mask.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp]
    lib.mirt_shadow_mask_device.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp]
    lib.mirt_direct_light_masked.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_direct_light_masked_device.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.mirt_get_shadow_mask_stats.argtypes = [C.POINTER(QueryStats)]
    lib.mirt_get_shadowed.argtypes = [C.c_int, _vp, C.c_int]
    lib.mirt_scene_upload_device.argtypes = [_vp, _vp, C.c_int]
    lib.mirt_scene_update_device.argtypes = [C.c_int, C.c_int, _vp]
    lib.mirt_scene_update.argtypes = [C.c_int, C.c_int, _vp]
    lib.mirt_scene_transform.argtypes = [C.c_int, C.c_int, _vp, _vp]
    lib.mirt_transform.argtypes = [_vp, C.c_int, _vp, _vp]
    lib.mirt_scene_download.argtypes = [C.c_int, C.c_int, _vp]
    lib.mirt_scene_info.argtypes = [C.POINTER(SceneInfo)]
    lib.mirt_scene_set_objects.argtypes = [_vp, C.c_int, _vp, C.c_int]
    lib.mirt_scene_pose.argtypes = [_vp, C.c_int, _vp]
    lib.mirt_pose.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int]
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise MirtError("mirt error %d: %s" % (rc, load().mirt_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def make_view(pos, rot9, focal, W, H):
    v = View()
    v.pos[:] = [float(x) for x in pos]
    v.rot[:] = [float(x) for x in np.asarray(rot9, np.float32).ravel()]
    v.focal = float(focal)
    v.width, v.height = int(W), int(H)
    return v


def make_lights(lights7):
    """lights7: (k, 7) array {pos, color, intensity} -> (ctypes array or None, k)."""
    l = np.ascontiguousarray(lights7, np.float32).reshape(-1, 7)
    if len(l) == 0:
        return None, 0
    arr = (Light * len(l))()
    for i, r in enumerate(l):
        arr[i].pos[:] = r[0:3].tolist()
        arr[i].color[:] = r[3:6].tolist()
        arr[i].intensity = float(r[6])
    return arr, len(l)


def rot_from_yaw(yaw, m11):
    """cameraRot as the reference's Update() builds it (raytracer.cpp:377-382 / rasteriser.cpp:378-383)."""
    c, s = np.float32(np.cos(np.float32(yaw))), np.float32(np.sin(np.float32(yaw)))
    r = np.zeros(9, np.float32)
    r[4] = m11
    r[0], r[2], r[6], r[8] = c, s, -s, c
    return r


# ---- lifetime ---------------------------------------------------------------------------------------

def init(device=0):
    global _soft_samples
    _check(load().mirt_init(int(device)))
    _soft_samples = 1                 # (a fresh context: hard shadows)


def shutdown():
    global _soft_samples
    if _lib is not None:
        _lib.mirt_shutdown()
    _soft_samples = 1                 # (context state: mirt_shutdown puts it back)


def surface_register(arr):
    """Pins and maps a host surface (numpy array): frames rendered into it skip the staging copy (mirt_surface_register)."""
    _check(load().mirt_surface_register(_ptr(arr), arr.nbytes))


def surface_unregister(arr):
    _check(load().mirt_surface_unregister(_ptr(arr)))


def previous_kernel_ms():
    """kernel_ms (dict like stats()["kernel_ms"]) and gpu_ms of the call before the last one (two frames in flight, profiling on)."""
    k = (C.c_float * 8)()
    gms = C.c_float()
    _check(load().mirt_get_previous_kernel_ms(k, C.byref(gms)))
    return {name: float(k[i]) for i, name in enumerate(KERNEL_NAMES)}, float(gms.value)


def set_profiling(on):
    _check(load().mirt_set_profiling(1 if on else 0))


def sync():
    _check(load().mirt_sync())


def stats():
    s = Stats()
    _check(load().mirt_get_stats(C.byref(s)))
    return {"primary_rays": s.primary_rays, "shadow_rays": s.shadow_rays, "tests": s.tests, "gpu_ms": s.gpu_ms,
            "kernel_ms": dict(zip(KERNEL_NAMES, list(s.kernel_ms))), "mode_used": s.mode_used, "candidates": s.candidates,
            "steps_primary": s.steps_primary, "steps_shadow": s.steps_shadow, "drains": s.drains,
            "bins_reused": int(s.bins_reused), "selected_triangles": int(s.selected_triangles)}


# ---- scene ------------------------------------------------------------------------------------------

def scene_cornell():
    t = np.zeros((30, 15), np.float32)
    n = load().mirt_scene_cornell(_ptr(t))
    if n != 30:
        _check(n if n < 0 else -3)
    return t


def scene_soup(seed, n, s):
    t = np.zeros((n, 15), np.float32)
    rc = load().mirt_scene_soup(int(seed), int(n), float(s), _ptr(t))
    if rc != n:
        _check(rc if rc < 0 else -3)
    return t


def cull(tris, view, flags=3):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    c = np.zeros(len(tris), np.uint8)
    _check(load().mirt_cull(_ptr(tris), len(tris), C.byref(view), int(flags), _ptr(c)))
    return c


def cull_device(view, flags=3):
    """The cull step on the GPU for the uploaded scene (flags stay on the device)."""
    _check(load().mirt_cull_device(C.byref(view), int(flags)))


def scene_get_culled():
    c = np.zeros(load().mirt_scene_size(), np.uint8)
    _check(load().mirt_scene_get_culled(_ptr(c), len(c)))
    return c


def scene_load_stl(path, scale=0.05, colour=(0.5, 0.5, 0.5)):
    """LoadSTL::LoadSTLFile: (n, 15) triangles of an ASCII STL, scaled by -scale, one colour, normals recomputed."""
    col = np.asarray(colour, np.float32)
    n = load().mirt_scene_load_stl(str(path).encode(), float(scale), _ptr(col), None, 0)
    if n < 0:
        raise MirtError("cannot load %s (status %d)" % (path, n))
    t = np.zeros((n, 15), np.float32)
    if n:
        _check(min(0, load().mirt_scene_load_stl(str(path).encode(), float(scale), _ptr(col), _ptr(t), n)))
    return t


def scene_upload(tris, culled=None):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    culled = None if culled is None else np.ascontiguousarray(culled, np.uint8)
    _check(load().mirt_scene_upload(_ptr(tris), _ptr(culled), len(tris)))


def scene_set_culled(culled):
    culled = np.ascontiguousarray(culled, np.uint8)
    _check(load().mirt_scene_set_culled(_ptr(culled), len(culled)))


# ---- moving and device-resident scenes (device arrays: raw pointers, e.g. torch.Tensor.data_ptr()) --------

def scene_upload_device(d_tris, n, d_culled=None):
    """scene_upload with both arrays in device memory (mirt_scene_upload_device): n x 15 floats, and n bytes or None."""
    _check(load().mirt_scene_upload_device(d_tris, d_culled, int(n)))


def scene_update_device(first, count, d_tris):
    """Replaces triangles [first, first + count) with count x 15 floats in device memory (mirt_scene_update_device)."""
    _check(load().mirt_scene_update_device(int(first), int(count), d_tris))


def scene_update(first, tris):
    """Replaces triangles [first, first + len(tris)) with the rows of a host array (mirt_scene_update)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    _check(load().mirt_scene_update(int(first), len(tris), _ptr(tris)))


def scene_transform(first, count, rot9, translate3=(0.0, 0.0, 0.0)):
    """Moves triangles [first, first + count) in place on the device: v -> rot9 * v + translate3 (GLM column-major mat3), normals
    recomputed (mirt_scene_transform)."""
    r = np.ascontiguousarray(rot9, np.float32).reshape(9)
    t = np.ascontiguousarray(translate3, np.float32).reshape(3)
    _check(load().mirt_scene_transform(int(first), int(count), _ptr(r), _ptr(t)))


def transform(tris, rot9, translate3=(0.0, 0.0, 0.0)):
    """The arithmetic of scene_transform on a host array (mirt_transform; no device): a new (n, 15) array."""
    out = np.array(tris, np.float32, order="C").reshape(-1, 15)
    r = np.ascontiguousarray(rot9, np.float32).reshape(9)
    t = np.ascontiguousarray(translate3, np.float32).reshape(3)
    _check(load().mirt_transform(_ptr(out), len(out), _ptr(r), _ptr(t)))
    return out


def _as_objects(objects):
    """Objects as an (k, 3) int32 array {rest_first, scene_first, count}: the bytes of k mirt_object."""
    if isinstance(objects, C.Array):
        objects = [(o.rest_first, o.scene_first, o.count) for o in objects]
    else:
        objects = [(o.rest_first, o.scene_first, o.count) if isinstance(o, Object) else tuple(o) for o in objects]
    return np.ascontiguousarray(np.array(objects, np.int64).reshape(-1, 3), np.int32)


def _as_pose(xforms, which):
    x = np.ascontiguousarray(xforms, np.float32).reshape(-1, 12)
    w = None if which is None else np.ascontiguousarray(which, np.int32).reshape(-1)
    if w is not None and len(w) != len(x):
        raise ValueError("%d transforms for %d listed objects" % (len(x), len(w)))
    return x, w


def scene_set_objects(objects, rest=None):
    """Declares the objects of the uploaded scene -- rows (rest_first, scene_first, count) or Object instances -- and the rest pose they
    are posed from: an (nrest, 15) host array, or None for a snapshot of the scene as it is (mirt_scene_set_objects).  No objects:
    they and the rest pose are forgotten."""
    o = _as_objects(objects)
    rest = None if rest is None else np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    _check(load().mirt_scene_set_objects(_ptr(o), len(o), _ptr(rest), 0 if rest is None else len(rest)))


def scene_pose(xforms, which=None):
    """Poses objects from the rest pose in one call: xforms is (count, 12), {rot9 column-major, translate3} per object; which lists
    their indices (None: objects 0 .. count - 1) (mirt_scene_pose)."""
    x, w = _as_pose(xforms, which)
    _check(load().mirt_scene_pose(_ptr(w), len(x), _ptr(x)))


def pose(rest, objects, xforms, tris, which=None):
    """The arithmetic of scene_set_objects + scene_pose on host arrays (mirt_pose; no device): a new (n, 15) array, tris with the
    listed objects' rows posed from rest (None: from tris itself)."""
    out = np.array(tris, np.float32, order="C").reshape(-1, 15)
    o = _as_objects(objects)
    rest = None if rest is None else np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    x, w = _as_pose(xforms, which)
    _check(load().mirt_pose(_ptr(rest), 0 if rest is None else len(rest), _ptr(o), len(o), _ptr(w), len(x), _ptr(x), _ptr(out), len(out)))
    return out


def scene_download(first=0, count=None):
    """Triangles [first, first + count) of the uploaded scene (to its end when count is None): (count, 15) float32."""
    if count is None:
        count = load().mirt_scene_size() - int(first)
    out = np.zeros((max(int(count), 0), 15), np.float32)
    _check(load().mirt_scene_download(int(first), int(count), _ptr(out)))
    return out


def scene_info():
    """n, finite, bbox_lo, bbox_hi (float32 arrays) and version of the uploaded scene (mirt_scene_info)."""
    s = SceneInfo()
    _check(load().mirt_scene_info(C.byref(s)))
    return {"n": int(s.n), "finite": int(s.finite), "bbox_lo": np.array(list(s.bbox_lo), np.float32),
            "bbox_hi": np.array(list(s.bbox_hi), np.float32), "version": int(s.version)}


def set_depth_of_field(kernel_size, focal_length=0.0):
    """kernel_size x kernel_size blur before the pixels are stored (the reference: 8, FOCAL_LENGTH 1.3 / 1.9); <= 1: off."""
    _check(load().mirt_set_depth_of_field(int(kernel_size), float(focal_length)))


def set_frames_in_flight(frames):
    """1: device calls run in order on one stream; 2: they alternate between two streams (consecutive frames need
    different output planes)."""
    _check(load().mirt_set_frames_in_flight(int(frames)))


def set_antialiasing(samples):
    """samples x samples sub-rays per pixel (the reference's AA_SAMPLES = 3); <= 1 switches it off."""
    _check(load().mirt_set_antialiasing(int(samples)))


def set_supersampled_many_lights(on):
    """Supersampled frames of more than MAX_LIGHTS light positions (the reference's AA + soft shadows with a third light) are
    rendered, each record a pixel carries shaded once, bit for bit the reference's sum (mirt_set_supersampled_many_lights).  Off by
    default, and again after shutdown(): the frame is refused."""
    _check(load().mirt_set_supersampled_many_lights(1 if on else 0))


def supersample_stats():
    """The last such frame (mirt_get_supersample_stats; waits for it): "hit_subrays", the sub-rays that hit -- each shades the
    carried record in the reference --, and "records_shaded", the records DirectLight was actually asked for."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(load().mirt_get_supersample_stats(C.byref(a), C.byref(b)))
    return {"hit_subrays": int(a.value), "records_shaded": int(b.value)}


def set_soft_shadows(samples, positions=None):
    """samples <= 1 turns soft shadows off; otherwise positions is (nlights*samples, 3), at most MAX_LIGHT_POSITIONS rows: up to
    MAX_LIGHTS lights with nlights*samples <= MAX_LIGHT_POSITIONS.  Frames and direct_light* with more than MAX_LIGHTS positions run
    DirectLight in passes (bit-identical); such frames are combined with set_antialiasing only while
    set_supersampled_many_lights is on (off by default: the frame is refused)."""
    global _soft_samples
    if samples <= 1:
        _check(load().mirt_set_soft_shadows(1, None, 0))
        _soft_samples = 1
        return
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    _check(load().mirt_set_soft_shadows(int(samples), _ptr(p), len(p)))
    _soft_samples = int(samples)


# ---- render (host buffers) --------------------------------------------------------------------------

def raytrace(view, lights7, indirect=(0.2, 0.2, 0.2), mode=RT_AUTO, want_rgb=True, want_index=True, xrgb=None,
             want_intersection=False):
    """want_intersection adds "dist" and "pos": closestIntersections[].distance / .position (mirt_raytrace_ex)."""
    W, H = view.width, view.height
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32)
    out = {
        "xrgb": np.zeros((H, W), np.uint32) if xrgb is None else xrgb,
        "rgb": np.zeros((H, W, 3), np.float32) if want_rgb else None,
        "index": np.zeros((H, W), np.int32) if want_index else None,
    }
    if want_intersection:
        out["dist"] = np.zeros((H, W), np.float32)
        out["pos"] = np.zeros((H, W, 3), np.float32)
        _check(load().mirt_raytrace_ex(C.byref(view), larr, nl, _ptr(ind), int(mode), _ptr(out["xrgb"]),
                                       out["xrgb"].strides[0], _ptr(out["rgb"]), _ptr(out["index"]), _ptr(out["dist"]), _ptr(out["pos"])))
    else:
        _check(load().mirt_raytrace(C.byref(view), larr, nl, _ptr(ind), int(mode), _ptr(out["xrgb"]),
                                    out["xrgb"].strides[0], _ptr(out["rgb"]), _ptr(out["index"])))
    out["stats"] = stats()
    return out


def rasterise(view, lights7, indirect=(0.2, 0.2, 0.2), want_rgb=True, want_zinv=True, want_index=True, xrgb=None):
    W, H = view.width, view.height
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32)
    out = {
        "xrgb": np.full((H, W), 0xDEADBEEF, np.uint32) if xrgb is None else xrgb,
        "rgb": np.zeros((H, W, 3), np.float32) if want_rgb else None,
        "depth": np.zeros((H, W), np.float32) if want_zinv else None,
        "index": np.zeros((H, W), np.int32) if want_index else None,
    }
    _check(load().mirt_rasterise(C.byref(view), larr, nl, _ptr(ind), _ptr(out["xrgb"]), out["xrgb"].strides[0],
                                 _ptr(out["rgb"]), _ptr(out["depth"]), _ptr(out["index"])))
    out["stats"] = stats()
    return out


# ---- render (device buffers: raw pointers, e.g. torch.Tensor.data_ptr()) -----------------------------

def raytrace_device(view, lights7, indirect, mode, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb=None, d_index=None,
                    d_dist=None, d_pos=None):
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32)
    if d_dist is None and d_pos is None:
        _check(load().mirt_raytrace_device(C.byref(view), larr, nl, _ptr(ind), int(mode), int(y0), int(y1),
                                           int(row_origin), d_xrgb, int(pitch_bytes), d_rgb, d_index))
    else:
        _check(load().mirt_raytrace_device_ex(C.byref(view), larr, nl, _ptr(ind), int(mode), int(y0), int(y1),
                                              int(row_origin), d_xrgb, int(pitch_bytes), d_rgb, d_index, d_dist, d_pos))


def rasterise_device(view, lights7, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb=None, d_zinv=None,
                     d_index=None):
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32)
    _check(load().mirt_rasterise_device(C.byref(view), larr, nl, _ptr(ind), int(y0), int(y1), int(row_origin),
                                        d_xrgb, int(pitch_bytes), d_rgb, d_zinv, d_index))


def prepared_raytrace_device(view, lights7, indirect, mode, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb=None,
                             d_index=None):
    """Marshals the arguments once and returns a zero-argument callable that enqueues the frame: keeps the
    per-frame host cost of a render loop at one foreign call."""
    lib = load()
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32).copy()
    args = (C.byref(view), larr, nl, _ptr(ind), int(mode), int(y0), int(y1), int(row_origin), d_xrgb, int(pitch_bytes),
            d_rgb, d_index)
    fn = lib.mirt_raytrace_device

    def launch(_keep=(view, larr, ind)):
        rc = fn(*args)
        if rc:
            _check(rc)
    return launch


def prepared_rasterise_device(view, lights7, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb=None, d_zinv=None,
                              d_index=None):
    lib = load()
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32).copy()
    args = (C.byref(view), larr, nl, _ptr(ind), int(y0), int(y1), int(row_origin), d_xrgb, int(pitch_bytes), d_rgb,
            d_zinv, d_index)
    fn = lib.mirt_rasterise_device

    def launch(_keep=(view, larr, ind)):
        rc = fn(*args)
        if rc:
            _check(rc)
    return launch


def prepared_async(kind, view, lights7, indirect, mode, surface):
    """Zero-argument callable: one asynchronous frame into `surface`, a numpy array inside a registered surface
    (mirt_raytrace_async / mirt_rasterise_async); mirt.sync() completes it."""
    lib = load()
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32).copy()
    if kind == "rt":
        fn, args = lib.mirt_raytrace_async, (C.byref(view), larr, nl, _ptr(ind), int(mode), _ptr(surface), int(surface.strides[0]))
    else:
        fn, args = lib.mirt_rasterise_async, (C.byref(view), larr, nl, _ptr(ind), _ptr(surface), int(surface.strides[0]))

    def launch(_keep=(view, larr, ind, surface)):
        rc = fn(*args)
        if rc:
            _check(rc)
    return launch


# ---- ray queries: ClosestIntersection / DirectLight for the caller's own rays -------------------------

def make_rays(start, direction):
    """(n, 3) starts and directions (either may be one vector for all) -> n rays (RAY_DTYPE)."""
    s, d = np.asarray(start, np.float32), np.asarray(direction, np.float32)
    n = max(s.reshape(-1, 3).shape[0], d.reshape(-1, 3).shape[0])
    rays = np.zeros(n, RAY_DTYPE)
    rays["start"], rays["dir"] = s, d
    return rays


def fresh_hits(n):
    """n records as Update() resets them (raytracer.cpp:335-339): distance FLT_MAX, index -1, position 0."""
    hits = np.zeros(int(n), HIT_DTYPE)
    hits["distance"] = np.finfo(np.float32).max
    hits["index"] = -1
    return hits


def _as_rays(rays):
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6).view(RAY_DTYPE).reshape(-1)
    return np.ascontiguousarray(rays)


def intersect(rays, hits=None):
    """One ClosestIntersection call per ray against the uploaded scene (mirt_intersect).  rays: RAY_DTYPE or (n, 6) floats;
    hits: the in/out records (HIT_DTYPE; fresh ones when None).  Returns the records after the calls (a new array)."""
    rays = _as_rays(rays)
    hits = fresh_hits(len(rays)) if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).copy()
    if len(hits) != len(rays):
        raise ValueError("%d rays but %d hit records" % (len(rays), len(hits)))
    _check(load().mirt_intersect(_ptr(rays), len(rays), _ptr(hits)))
    return hits


def intersect_device(d_rays, nrays, d_hits):
    """The same on device arrays (raw pointers), queued like a *_device frame; mirt.sync() completes it."""
    _check(load().mirt_intersect_device(d_rays, int(nrays), d_hits))


def intersect_ordered(rays, max_hits, after=None):
    """The first max_hits triangles along every ray in the reference's order -- nearer first, the later index first among equal
    distances -- (mirt_intersect_ordered): (hits[n, max_hits] HIT_DTYPE, counts[n] int32); the slots behind a ray's count are fresh
    records.  after: one record per ray (HIT_DTYPE) behind which the ray continues -- the last record an earlier call wrote -- or None."""
    rays = _as_rays(rays)
    max_hits = int(max_hits)
    if after is not None:
        after = np.ascontiguousarray(after, HIT_DTYPE)
        if after.shape != (len(rays),):
            raise ValueError("%d rays but after has shape %s" % (len(rays), after.shape))
    hits = np.zeros((len(rays), max(max_hits, 0)), HIT_DTYPE)
    counts = np.zeros(len(rays), np.int32)
    _check(load().mirt_intersect_ordered(_ptr(rays), len(rays), _ptr(after), max_hits, _ptr(hits), _ptr(counts)))
    return hits, counts


def intersect_ordered_device(d_rays, nrays, d_after, max_hits, d_hits, d_counts):
    """The same on device arrays (raw pointers; d_after may be None, or d_hits itself when max_hits is 1), queued like
    intersect_device; mirt.sync() completes it."""
    _check(load().mirt_intersect_ordered_device(d_rays, int(nrays), d_after, int(max_hits), d_hits, d_counts))


def direct_light(hits, lights7):
    """DirectLight(hits[i]) for every record (mirt_direct_light): (n, 3) float32."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    larr, nl = make_lights(lights7)
    out = np.zeros((len(hits), 3), np.float32)
    _check(load().mirt_direct_light(_ptr(hits), len(hits), larr, nl, _ptr(out)))
    return out


def direct_light_device(d_hits, nhits, lights7, d_rgb):
    larr, nl = make_lights(lights7)
    _check(load().mirt_direct_light_device(d_hits, int(nhits), larr, nl, d_rgb))


def set_query_mode(mode):
    """QUERY_AUTO / QUERY_BRUTE / QUERY_BINNED: how direct_light* walks its shadow rays (mirt_set_query_mode)."""
    _check(load().mirt_set_query_mode(int(mode)))


def set_ray_grid(on):
    """True: intersect* and occluded* answer through the arbitrary-ray grid whenever it can be built, bit for bit as before
    (mirt_set_ray_grid); False, the default: they sweep."""
    _check(load().mirt_set_ray_grid(1 if on else 0))


def ray_grid_stats():
    """The last intersect* / occluded* call made under set_ray_grid(True) (mirt_get_ray_grid_stats) as a dict: mode_used (0 no such
    call), source (0 none, 1 built by the call, 2 kept), gave_up, cells, plane_bins, offset_bins, pairs, plane_pairs, every_rows and --
    with profiling on -- rays, rows_cells, rows_planes, rows_every, tests, swept_rays."""
    s = RayGridStats()
    _check(load().mirt_get_ray_grid_stats(C.byref(s)))
    return {name: int(getattr(s, name)) for name, _ in RayGridStats._fields_ if name != "reserved"}


def _read_query_stats(getter):
    """One mirt_query_stats through `getter` (mirt_get_query_stats, mirt_get_fan_stats, mirt_get_occlusion_stats) as a dict."""
    s = QueryStats()
    _check(getter(C.byref(s)))
    return {name: int(getattr(s, name)) for name, _ in QueryStats._fields_}


def query_stats():
    """The last DirectLight query (mirt_get_query_stats): mode_used, cube_source (0 none, 1 built by the call, 2 kept from an
    earlier query, 3 the frame path's), cube_bins, shells and -- with profiling on -- the binned kernel's counters."""
    return _read_query_stats(load().mirt_get_query_stats)


def intersect_from(origin, dirs, hits=None):
    """ClosestIntersection(origin, dirs[i]) for every direction (mirt_intersect_from): what intersect() returns for the rays
    {origin, dirs[i]}, bit for bit, each ray walking its bin of a cube around the origin where that pays (set_query_mode).
    dirs: (n, 3) floats, used as given; hits: the in/out records (HIT_DTYPE; fresh ones when None).  Returns a new array."""
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    hits = fresh_hits(len(dirs)) if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).copy()
    if len(hits) != len(dirs):
        raise ValueError("%d directions but %d hit records" % (len(dirs), len(hits)))
    _check(load().mirt_intersect_from(_ptr(origin), _ptr(dirs), len(dirs), _ptr(hits)))
    return hits


def intersect_from_device(origin, d_dirs, nrays, d_hits):
    """The same on device arrays (raw pointers; the origin is host data), queued like a *_device frame; mirt.sync() completes it."""
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    _check(load().mirt_intersect_from_device(_ptr(origin), d_dirs, int(nrays), d_hits))


def _as_fans(origins, origin_of, dirs):
    """The arrays of a many-origin call as the library takes them: origins (k, 3), origin_of one int32 per ray or None, dirs (n, 3)."""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if origin_of is not None:
        origin_of = np.ascontiguousarray(origin_of, np.int32).reshape(-1)
        if len(origin_of) != len(dirs):
            raise ValueError("%d directions but %d origin indices" % (len(dirs), len(origin_of)))
    return np.ascontiguousarray(origins, np.float32).reshape(-1, 3), origin_of, dirs


def intersect_fans(origins, origin_of, dirs, hits=None):
    """ClosestIntersection(origins[origin_of[i]], dirs[i]) for every ray (mirt_intersect_fans): what intersect() returns for the
    rays {origins[origin_of[i]], dirs[i]}, bit for bit, the origins sharing cubes of up to MAX_LIGHTS positions (set_query_mode).
    origins: (k, 3) floats; origin_of: one int32 per ray, or None for a single origin; dirs: (n, 3) floats, used as given; hits:
    the in/out records (HIT_DTYPE; fresh ones when None).  Returns a new array."""
    origins, origin_of, dirs = _as_fans(origins, origin_of, dirs)
    hits = fresh_hits(len(dirs)) if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).copy()
    if len(hits) != len(dirs):
        raise ValueError("%d directions but %d hit records" % (len(dirs), len(hits)))
    _check(load().mirt_intersect_fans(_ptr(origins), len(origins), _ptr(origin_of), _ptr(dirs), len(dirs), _ptr(hits)))
    return hits


def intersect_fans_device(origins, d_origin_of, d_dirs, nrays, d_hits):
    """The same on device arrays (raw pointers; the origins are host data, d_origin_of may be None for a single origin), queued like
    a *_device frame; mirt.sync() completes it."""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    _check(load().mirt_intersect_fans_device(_ptr(origins), len(origins), d_origin_of, d_dirs, int(nrays), d_hits))


def fan_stats():
    """The last intersect_from* / intersect_fans* / intersect_ordered_from* / intersect_ordered_fans* call (mirt_get_fan_stats), in mirt_query_stats' fields: mode_used, cube_source (0 none, 1 built by
    the call, 2 kept), cube_bins, shells and -- profiling on, binned -- shadow_rays = rays, candidates = rows stepped over, tests =
    rows tested, fallback_records = rays that swept the whole table."""
    return _read_query_stats(load().mirt_get_fan_stats)


# ---- occlusion queries: any-hit rays ---------------------------------------------------------------------

def _as_limits(max_distance, n, what):
    """None, or n float32 limits (one value stands for all)."""
    if max_distance is None:
        return None
    lim = np.asarray(max_distance, np.float32)
    lim = np.full(n, lim, np.float32) if lim.ndim == 0 else np.ascontiguousarray(lim).reshape(-1)
    if len(lim) != n:
        raise ValueError("%d %s but %d limits" % (n, what, len(lim)))
    return lim


def _occluded_out(out, n, what):
    """The uint8 array the bytes go to: a new one, or the caller's (C-contiguous uint8 of the rays' length)."""
    if out is None:
        return np.zeros(n, np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("the output must be a writeable C-contiguous uint8 array")
    if out.size != n:
        raise ValueError("%d %s but %d output bytes" % (n, what, out.size))
    return out


def occluded(rays, max_distance=None, out=None):
    """occluded[i] = 1 when some triangle ClosestIntersection accepts for rays[i] is nearer than max_distance[i], strictly; else 0
    (mirt_occluded).  rays: RAY_DTYPE or (n, 6) floats, dir used as given; max_distance: n floats, one for all, or None for +inf.
    Returns uint8 (`out` when given: every byte is written)."""
    rays = _as_rays(rays)
    lim = _as_limits(max_distance, len(rays), "rays")
    out = _occluded_out(out, len(rays), "rays")
    _check(load().mirt_occluded(_ptr(rays), len(rays), None if lim is None else _ptr(lim), _ptr(out)))
    return out


def occluded_device(d_rays, nrays, d_max_distance, d_occluded):
    """The same on device arrays (raw pointers; d_max_distance may be None), queued like a *_device frame; mirt.sync() completes it."""
    _check(load().mirt_occluded_device(d_rays, int(nrays), d_max_distance, d_occluded))


def occluded_fans(origins, origin_of, dirs, max_distance=None, out=None):
    """occluded() for the rays {origins[origin_of[i]], dirs[i]}, byte for byte, through the cubes of intersect_fans
    (mirt_occluded_fans; set_query_mode).  origins: (k, 3) floats; origin_of: one int32 per ray, or None for a single origin."""
    origins, origin_of, dirs = _as_fans(origins, origin_of, dirs)
    lim = _as_limits(max_distance, len(dirs), "directions")
    out = _occluded_out(out, len(dirs), "directions")
    if origin_of is not None:
        if len(origin_of) and (origin_of.min() < 0 or origin_of.max() >= len(origins)):
            bad = int(np.flatnonzero((origin_of < 0) | (origin_of >= len(origins)))[0])
            raise ValueError("origin_of[%d] = %d is outside [0, %d)" % (bad, int(origin_of[bad]), len(origins)))
    _check(load().mirt_occluded_fans(_ptr(origins), len(origins), _ptr(origin_of), _ptr(dirs), len(dirs), _ptr(lim), _ptr(out)))
    return out


def occluded_fans_device(origins, d_origin_of, d_dirs, nrays, d_max_distance, d_occluded):
    """The same on device arrays (raw pointers; the origins are host data, d_origin_of may be None for a single origin and
    d_max_distance for +inf), queued like a *_device frame; mirt.sync() completes it."""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    _check(load().mirt_occluded_fans_device(_ptr(origins), len(origins), d_origin_of, d_dirs, int(nrays), d_max_distance, d_occluded))


def occlusion_stats():
    """The last occluded* call (mirt_get_occlusion_stats), in mirt_query_stats' fields: mode_used, cube_source (0 - 4 as for
    intersect_fans), cube_bins, shells and -- profiling on, binned -- shadow_rays = rays, candidates = rows stepped over, tests =
    rows not beyond the limit, fallback_records = rays that swept their origin's table."""
    return _read_query_stats(load().mirt_get_occlusion_stats)


# ---- ray queries along one direction ------------------------------------------------------------------------

def _as_along(direction, origins):
    """The shared direction (3 floats) and the starts (n, 3) as the library takes them."""
    return np.ascontiguousarray(direction, np.float32).reshape(3), np.ascontiguousarray(origins, np.float32).reshape(-1, 3)


def intersect_along(direction, origins, hits=None):
    """ClosestIntersection(origins[i], direction) for every start (mirt_intersect_along): what intersect() returns for the rays
    {origins[i], direction}, bit for bit, each ray walking its cell of a grid across the direction where that pays
    (set_query_mode).  direction: 3 floats, used as given; origins: (n, 3) floats; hits: the in/out records (HIT_DTYPE; fresh ones
    when None).  Returns a new array."""
    direction, origins = _as_along(direction, origins)
    hits = fresh_hits(len(origins)) if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).copy()
    if len(hits) != len(origins):
        raise ValueError("%d origins but %d hit records" % (len(origins), len(hits)))
    _check(load().mirt_intersect_along(_ptr(direction), _ptr(origins), len(origins), _ptr(hits)))
    return hits


def intersect_along_device(direction, d_origins, nrays, d_hits):
    """The same on device arrays (raw pointers; the direction is host data), queued like a *_device frame; mirt.sync() completes it."""
    direction = np.ascontiguousarray(direction, np.float32).reshape(3)
    _check(load().mirt_intersect_along_device(_ptr(direction), d_origins, int(nrays), d_hits))


def occluded_along(direction, origins, max_distance=None, out=None):
    """occluded() for the rays {origins[i], direction}, byte for byte, through the grid of intersect_along (mirt_occluded_along).
    max_distance: n floats, one for all, or None for +inf.  Returns uint8 (`out` when given: every byte is written)."""
    direction, origins = _as_along(direction, origins)
    lim = _as_limits(max_distance, len(origins), "origins")
    out = _occluded_out(out, len(origins), "origins")
    _check(load().mirt_occluded_along(_ptr(direction), _ptr(origins), len(origins), None if lim is None else _ptr(lim), _ptr(out)))
    return out


def occluded_along_device(direction, d_origins, nrays, d_max_distance, d_occluded):
    """The same on device arrays (raw pointers; the direction is host data, d_max_distance may be None), queued like a *_device frame."""
    direction = np.ascontiguousarray(direction, np.float32).reshape(3)
    _check(load().mirt_occluded_along_device(_ptr(direction), d_origins, int(nrays), d_max_distance, d_occluded))


def along_stats():
    """The last intersect_along* / occluded_along* / intersect_alongs* / occluded_alongs* / intersect_ordered_along(s)* / count_hits_along(s)* call (mirt_get_along_stats), in
    mirt_query_stats' fields: mode_used, cube_source (0 no grid, 1 built by the call, 2 kept), cube_bins = cells per grid side, shells
    and -- profiling on, binned -- shadow_rays = rays, candidates = rows offered, tests = rows tested, fallback_records = rays that
    swept the scene.  For a call of several directions the counters are summed over its passes, and cube_source is 1 when some pass
    built its group, 2 when every pass's group was held."""
    return _read_query_stats(load().mirt_get_along_stats)


# ---- ray queries along several directions in one call ----------------------------------------------------------

def _as_alongs(directions, dir_of, origins):
    """The arrays of a call of several directions as the library takes them: directions (k, 3), dir_of one int32 per ray or None,
    origins (n, 3)."""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    if dir_of is not None:
        dir_of = np.ascontiguousarray(dir_of, np.int32).reshape(-1)
        if len(dir_of) != len(origins):
            raise ValueError("%d origins but %d direction indices" % (len(origins), len(dir_of)))
    return np.ascontiguousarray(directions, np.float32).reshape(-1, 3), dir_of, origins


def intersect_alongs(directions, dir_of, origins, hits=None):
    """ClosestIntersection(origins[i], directions[dir_of[i]]) for every start (mirt_intersect_alongs): what intersect() returns for
    the rays {origins[i], directions[dir_of[i]]}, bit for bit, the directions sharing groups of up to MAX_LIGHTS grids
    (set_query_mode).  directions: (k, 3) floats, used as given; dir_of: one int32 per ray, or None for a single direction; origins:
    (n, 3) floats; hits: the in/out records (HIT_DTYPE; fresh ones when None).  Returns a new array."""
    directions, dir_of, origins = _as_alongs(directions, dir_of, origins)
    hits = fresh_hits(len(origins)) if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).copy()
    if len(hits) != len(origins):
        raise ValueError("%d origins but %d hit records" % (len(origins), len(hits)))
    _check(load().mirt_intersect_alongs(_ptr(directions), len(directions), _ptr(dir_of), _ptr(origins), len(origins), _ptr(hits)))
    return hits


def intersect_alongs_device(directions, d_dir_of, d_origins, nrays, d_hits):
    """The same on device arrays (raw pointers; the directions are host data, d_dir_of may be None for a single direction), queued
    like a *_device frame; mirt.sync() completes it."""
    directions = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    _check(load().mirt_intersect_alongs_device(_ptr(directions), len(directions), d_dir_of, d_origins, int(nrays), d_hits))


def occluded_alongs(directions, dir_of, origins, max_distance=None, out=None):
    """occluded() for the rays {origins[i], directions[dir_of[i]]}, byte for byte, through the groups of intersect_alongs
    (mirt_occluded_alongs).  max_distance: n floats, one for all, or None for +inf.  Returns uint8 (`out` when given: every byte is
    written)."""
    directions, dir_of, origins = _as_alongs(directions, dir_of, origins)
    lim = _as_limits(max_distance, len(origins), "origins")
    out = _occluded_out(out, len(origins), "origins")
    _check(load().mirt_occluded_alongs(_ptr(directions), len(directions), _ptr(dir_of), _ptr(origins), len(origins), _ptr(lim), _ptr(out)))
    return out


def occluded_alongs_device(directions, d_dir_of, d_origins, nrays, d_max_distance, d_occluded):
    """The same on device arrays (raw pointers; the directions are host data, d_dir_of may be None for a single direction and
    d_max_distance for +inf), queued like a *_device frame."""
    directions = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    _check(load().mirt_occluded_alongs_device(_ptr(directions), len(directions), d_dir_of, d_origins, int(nrays), d_max_distance, d_occluded))


# ---- every hit along parallel rays, in order ------------------------------------------------------------------

def _ordered_arrays(n, max_hits, after):
    """max_hits, the `after` records (or None) and the outputs of an ordered call of n rays."""
    max_hits = int(max_hits)
    if after is not None:
        after = np.ascontiguousarray(after, HIT_DTYPE)
        if after.shape != (n,):
            raise ValueError("%d origins but after has shape %s" % (n, after.shape))
    return max_hits, after, np.zeros((n, max(max_hits, 0)), HIT_DTYPE), np.zeros(n, np.int32)


def intersect_ordered_along(direction, origins, max_hits, after=None):
    """intersect_ordered() for the rays {origins[i], direction}, byte for byte, through the grid of intersect_along where that pays
    (mirt_intersect_ordered_along; set_query_mode, along_stats): (hits[n, max_hits] HIT_DTYPE, counts[n] int32).  The thickness of a
    part along a beam is hits["distance"][:, 1] - hits["distance"][:, 0] where counts >= 2."""
    direction, origins = _as_along(direction, origins)
    max_hits, after, hits, counts = _ordered_arrays(len(origins), max_hits, after)
    _check(load().mirt_intersect_ordered_along(_ptr(direction), _ptr(origins), len(origins), _ptr(after), max_hits, _ptr(hits), _ptr(counts)))
    return hits, counts


def intersect_ordered_along_device(direction, d_origins, nrays, d_after, max_hits, d_hits, d_counts):
    """The same on device arrays (raw pointers; the direction is host data, d_after may be None, or d_hits itself when max_hits is
    1), queued like a *_device frame; mirt.sync() completes it."""
    direction = np.ascontiguousarray(direction, np.float32).reshape(3)
    _check(load().mirt_intersect_ordered_along_device(_ptr(direction), d_origins, int(nrays), d_after, int(max_hits), d_hits, d_counts))


def intersect_ordered_alongs(directions, dir_of, origins, max_hits, after=None):
    """intersect_ordered() for the rays {origins[i], directions[dir_of[i]]}, byte for byte, through the groups of intersect_alongs
    (mirt_intersect_ordered_alongs): (hits[n, max_hits], counts[n]).  dir_of: one int32 per ray, or None for a single direction."""
    directions, dir_of, origins = _as_alongs(directions, dir_of, origins)
    max_hits, after, hits, counts = _ordered_arrays(len(origins), max_hits, after)
    _check(load().mirt_intersect_ordered_alongs(_ptr(directions), len(directions), _ptr(dir_of), _ptr(origins), len(origins), _ptr(after), max_hits,
                                                _ptr(hits), _ptr(counts)))
    return hits, counts


def intersect_ordered_alongs_device(directions, d_dir_of, d_origins, nrays, d_after, max_hits, d_hits, d_counts):
    """The same on device arrays (raw pointers; the directions are host data, d_dir_of may be None for a single direction).  A ray
    whose index names no direction keeps its slots as they were and gets the count 0."""
    directions = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    _check(load().mirt_intersect_ordered_alongs_device(_ptr(directions), len(directions), d_dir_of, d_origins, int(nrays), d_after, int(max_hits),
                                                       d_hits, d_counts))


# ---- every hit along rays from shared origins, in order --------------------------------------------------------

def intersect_ordered_from(origin, dirs, max_hits, after=None):
    """intersect_ordered() for the rays {origin, dirs[i]}, byte for byte, through the cube of intersect_from where that pays
    (mirt_intersect_ordered_from; set_query_mode, fan_stats): (hits[n, max_hits] HIT_DTYPE, counts[n] int32).  The layers under a
    pixel of a perspective camera are hits[i, :counts[i]]."""
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    max_hits, after, hits, counts = _ordered_arrays(len(dirs), max_hits, after)
    _check(load().mirt_intersect_ordered_from(_ptr(origin), _ptr(dirs), len(dirs), _ptr(after), max_hits, _ptr(hits), _ptr(counts)))
    return hits, counts


def intersect_ordered_from_device(origin, d_dirs, nrays, d_after, max_hits, d_hits, d_counts):
    """The same on device arrays (raw pointers; the origin is host data, d_after may be None, or d_hits itself when max_hits is 1),
    queued like a *_device frame; mirt.sync() completes it."""
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    _check(load().mirt_intersect_ordered_from_device(_ptr(origin), d_dirs, int(nrays), d_after, int(max_hits), d_hits, d_counts))


def intersect_ordered_fans(origins, origin_of, dirs, max_hits, after=None):
    """intersect_ordered() for the rays {origins[origin_of[i]], dirs[i]}, byte for byte, through the cubes of intersect_fans
    (mirt_intersect_ordered_fans): (hits[n, max_hits], counts[n]).  origin_of: one int32 per ray, or None for a single origin."""
    origins, origin_of, dirs = _as_fans(origins, origin_of, dirs)
    max_hits, after, hits, counts = _ordered_arrays(len(dirs), max_hits, after)
    _check(load().mirt_intersect_ordered_fans(_ptr(origins), len(origins), _ptr(origin_of), _ptr(dirs), len(dirs), _ptr(after), max_hits,
                                              _ptr(hits), _ptr(counts)))
    return hits, counts


def intersect_ordered_fans_device(origins, d_origin_of, d_dirs, nrays, d_after, max_hits, d_hits, d_counts):
    """The same on device arrays (raw pointers; the origins are host data, d_origin_of may be None for a single origin).  A ray whose
    index names no origin keeps its slots as they were and gets the count 0."""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    _check(load().mirt_intersect_ordered_fans_device(_ptr(origins), len(origins), d_origin_of, d_dirs, int(nrays), d_after, int(max_hits),
                                                     d_hits, d_counts))


# ---- the number of hits along a ray ---------------------------------------------------------------------------

def _count_arrays(n, after, max_distance, what):
    """The `after` records (or None), the limits (or None) and the output of a count call of n rays."""
    if after is not None:
        after = np.ascontiguousarray(after, HIT_DTYPE)
        if after.shape != (n,):
            raise ValueError("%d %s but after has shape %s" % (n, what, after.shape))
    return after, _as_limits(max_distance, n, what), np.zeros(n, np.int32)


def count_hits(rays, after=None, max_distance=None):
    """The number of triangles along every ray (mirt_count_hits): those ClosestIntersection accepts at a distance a fresh record
    takes, behind after[i] when `after` is given (HIT_DTYPE, one record per ray: only distance and index are read) and strictly
    nearer than max_distance[i] when limits are given (n floats, or one for all).  Returns int32 counts.  A point lies inside a closed
    mesh when a ray from it crosses an odd number of triangles."""
    rays = _as_rays(rays)
    after, lim, counts = _count_arrays(len(rays), after, max_distance, "rays")
    _check(load().mirt_count_hits(_ptr(rays), len(rays), _ptr(after), _ptr(lim), _ptr(counts)))
    return counts


def count_hits_device(d_rays, nrays, d_after, d_max_distance, d_counts):
    """The same on device arrays (raw pointers; d_after and d_max_distance may be None), queued like intersect_device; mirt.sync()
    completes it."""
    _check(load().mirt_count_hits_device(d_rays, int(nrays), d_after, d_max_distance, d_counts))


def count_hits_along(direction, origins, after=None, max_distance=None):
    """count_hits() for the rays {origins[i], direction}, count for count, through the grid of intersect_along where that pays
    (mirt_count_hits_along; set_query_mode, along_stats).  The occupancy of a voxel line is the count's parity."""
    direction, origins = _as_along(direction, origins)
    after, lim, counts = _count_arrays(len(origins), after, max_distance, "origins")
    _check(load().mirt_count_hits_along(_ptr(direction), _ptr(origins), len(origins), _ptr(after), _ptr(lim), _ptr(counts)))
    return counts


def count_hits_along_device(direction, d_origins, nrays, d_after, d_max_distance, d_counts):
    """The same on device arrays (raw pointers; the direction is host data, d_after and d_max_distance may be None), queued like a
    *_device frame; mirt.sync() completes it."""
    direction = np.ascontiguousarray(direction, np.float32).reshape(3)
    _check(load().mirt_count_hits_along_device(_ptr(direction), d_origins, int(nrays), d_after, d_max_distance, d_counts))


def count_hits_alongs(directions, dir_of, origins, after=None, max_distance=None):
    """count_hits() for the rays {origins[i], directions[dir_of[i]]}, count for count, through the groups of intersect_alongs
    (mirt_count_hits_alongs).  dir_of: one int32 per ray, or None for a single direction."""
    directions, dir_of, origins = _as_alongs(directions, dir_of, origins)
    after, lim, counts = _count_arrays(len(origins), after, max_distance, "origins")
    _check(load().mirt_count_hits_alongs(_ptr(directions), len(directions), _ptr(dir_of), _ptr(origins), len(origins), _ptr(after), _ptr(lim),
                                         _ptr(counts)))
    return counts


def count_hits_alongs_device(directions, d_dir_of, d_origins, nrays, d_after, d_max_distance, d_counts):
    """The same on device arrays (raw pointers; the directions are host data, d_dir_of may be None for a single direction).  A ray
    whose index names no direction gets the count 0."""
    directions = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    _check(load().mirt_count_hits_alongs_device(_ptr(directions), len(directions), d_dir_of, d_origins, int(nrays), d_after, d_max_distance,
                                                d_counts))


# ---- shadow masks: DirectLight's shadow decisions, and DirectLight from them ---------------------------------

def mask_words(npositions):
    """Planes of a shadow mask of npositions light positions (MIRT_MASK_WORDS): one uint32 word per record and 32 positions."""
    return (int(npositions) + 31) // 32


def _light_positions(nlights):
    """lights x samples under the current set_soft_shadows state, as the library counts them (the samples of the last
    set_soft_shadows call that succeeded: the masks' shapes follow from them)."""
    return int(nlights) * _soft_samples


def shadow_mask(hits, lights7):
    """DirectLight's shadow decision per (record, light position) (mirt_shadow_mask): a (words, n) uint32 array, position j =
    light * samples + sample in bit j & 31 of row j >> 5; 1 where DirectLight sets D = 0 (raytracer.cpp:314).  Only the records'
    positions are read, so bare points with any index get their bits."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    larr, nl = make_lights(lights7)
    out = np.zeros((mask_words(_light_positions(nl)), len(hits)), np.uint32)
    _check(load().mirt_shadow_mask(_ptr(hits), len(hits), larr, nl, _ptr(out)))
    return out


def shadow_mask_device(d_hits, nhits, lights7, d_mask):
    """The same on device arrays (raw pointers; d_mask: mask_words(positions) x nhits words), queued like a *_device frame;
    mirt.sync() completes it."""
    larr, nl = make_lights(lights7)
    _check(load().mirt_shadow_mask_device(d_hits, int(nhits), larr, nl, d_mask))


def _as_mask(mask, nhits, nlights):
    """A (words, n) uint32 mask with at least the planes nlights lights need under the current soft-shadow state, C-contiguous (the
    plane stride is the record count: the mask of more lights serves a prefix of them)."""
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint32:
        raise ValueError("the mask must be a uint32 array")
    need = mask_words(_light_positions(nlights))
    if mask.ndim != 2 or mask.shape[1] != nhits or mask.shape[0] < need:
        raise ValueError("the mask must have shape (>= %d, %d), not %s" % (need, nhits, mask.shape))
    return np.ascontiguousarray(mask)


def direct_light_masked(hits, lights7, mask):
    """DirectLight(hits[i]) with every shadow ray replaced by its bit of `mask` (mirt_direct_light_masked): (n, 3) float32.  With the
    mask shadow_mask() returned for the same records, light positions and soft-shadow state it is direct_light() bit for bit,
    whatever the lights' colours and intensities are now; no ray is cast."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    larr, nl = make_lights(lights7)
    mask = _as_mask(mask, len(hits), nl)
    out = np.zeros((len(hits), 3), np.float32)
    _check(load().mirt_direct_light_masked(_ptr(hits), len(hits), larr, nl, _ptr(mask), _ptr(out)))
    return out


def direct_light_masked_device(d_hits, nhits, lights7, d_mask, d_rgb):
    """The same on device arrays (raw pointers), queued like a *_device frame; mirt.sync() completes it."""
    larr, nl = make_lights(lights7)
    _check(load().mirt_direct_light_masked_device(d_hits, int(nhits), larr, nl, d_mask, d_rgb))


def shadow_mask_stats():
    """The last shadow_mask* call (mirt_get_shadow_mask_stats), in mirt_query_stats' fields with DirectLight's meanings; with
    profiling on the counters are filled for a sweep as well: shadow_rays = records x positions."""
    return _read_query_stats(load().mirt_get_shadow_mask_stats)


def get_shadowed(position, n):
    """One byte per triangle (mirt_get_shadowed): 1 where one other triangle hides the whole triangle from light position `position`
    -- the binned frames cast no shadow ray from it.  MirtError while no shared light cube is held."""
    out = np.zeros(int(n), np.uint8)
    _check(load().mirt_get_shadowed(int(position), _ptr(out), int(n)))
    return out


# ---- several GPUs: band sharding with the gather inside the library ------------------------------------

COMM_ID_BYTES = 128


def band_of(rank, world, height):
    y0, y1 = C.c_int(), C.c_int()
    _check(load().mirt_band_of(int(rank), int(world), int(height), C.byref(y0), C.byref(y1)))
    return y0.value, y1.value


def band_plan(world, root, width, height, nviews):
    """[(root_offset, band_offset, bytes, peer)] of one gather (mirt_band_plan)."""
    n = load().mirt_band_plan(world, root, width, height, nviews, None, None, None, None, 0)
    if n < 0:
        _check(n)
    ro, bo, by, pe = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    load().mirt_band_plan(world, root, width, height, nviews, _ptr(ro), _ptr(bo), _ptr(by), _ptr(pe), n)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(ro, bo, by, pe)]


def set_partition(strip_rows):
    """0: contiguous bands; > 0: interleaved strips of that many rows (mirt_set_partition)."""
    _check(load().mirt_set_partition(int(strip_rows)))


def partition_segments(rank, world, height, strip_rows):
    """[(y0, y1)] of a rank's rows (mirt_partition_segments)."""
    n = load().mirt_partition_segments(rank, world, height, strip_rows, None, None, 0)
    if n < 0:
        _check(n)
    a, b = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    load().mirt_partition_segments(rank, world, height, strip_rows, _ptr(a), _ptr(b), n)
    return [(int(x), int(y)) for x, y in zip(a[:n], b[:n])]


def partition_plan(world, root, width, height, nviews, strip_rows):
    """[(root_offset, band_offset, bytes, peer)] of one gather for either partition (mirt_partition_plan)."""
    n = load().mirt_partition_plan(world, root, width, height, nviews, strip_rows, None, None, None, None, 0)
    if n < 0:
        _check(n)
    ro, bo, by, pe = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.int32)
    load().mirt_partition_plan(world, root, width, height, nviews, strip_rows, _ptr(ro), _ptr(bo), _ptr(by), _ptr(pe), n)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(ro[:n], bo[:n], by[:n], pe[:n])]


PARTITION_WEIGHTED = -1


def set_cost_histogram(on):
    """Binned ray-traced frames leave the cost histogram of the whole frame (mirt_set_cost_histogram)."""
    _check(load().mirt_set_cost_histogram(1 if on else 0))


def cost_histogram():
    """(hist, shift) of the latest binned frame -- estimated (tile, triangle) pairs per coarse tile row of (1 << shift) tile rows --
    or (None, 0)."""
    h = np.zeros(256, np.uint32)
    rows, shift = C.c_int(), C.c_int()
    n = load().mirt_cost_histogram(_ptr(h), 256, C.byref(rows), C.byref(shift))
    if n < 0:
        _check(n)
    return (h[:n].copy(), shift.value) if n > 0 else (None, 0)


def weighted_bounds(hist, shift, width, height, world):
    """world + 1 row boundaries of bands of equal estimated cost (mirt_weighted_bounds; pure arithmetic, no device)."""
    h = np.ascontiguousarray(hist if hist is not None else np.zeros(0), np.uint32)
    b = np.zeros(world + 1, np.int32)
    _check(load().mirt_weighted_bounds(_ptr(h) if len(h) else None, len(h), int(shift), int(width), int(height), int(world), _ptr(b)))
    return [int(x) for x in b]


def partition_bounds(world, width, height):
    """The boundaries the next sharded call will use (mirt_partition_bounds)."""
    b = np.zeros(world + 1, np.int32)
    _check(load().mirt_partition_bounds(int(world), int(width), int(height), _ptr(b)))
    return [int(x) for x in b]


def bounds_plan(world, root, width, height, nviews, bounds):
    """[(root_offset, band_offset, bytes, peer)] of one gather for explicit band boundaries (mirt_bounds_plan)."""
    bd = np.ascontiguousarray(bounds, np.int32)
    n = load().mirt_bounds_plan(world, root, width, height, nviews, _ptr(bd), None, None, None, None, 0)
    if n < 0:
        _check(n)
    ro, bo, by, pe = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.int32)
    load().mirt_bounds_plan(world, root, width, height, nviews, _ptr(bd), _ptr(ro), _ptr(bo), _ptr(by), _ptr(pe), n)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(ro[:n], bo[:n], by[:n], pe[:n])]


def comm_create_id():
    buf = (C.c_char * COMM_ID_BYTES)()
    _check(load().mirt_comm_create_id(buf))
    return bytes(buf)


def comm_init(comm_id, rank, world):
    buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(comm_id)
    _check(load().mirt_comm_init(buf, int(rank), int(world)))


def comm_shutdown():
    _check(load().mirt_comm_shutdown())


def comm_selfcheck(nbytes):
    _check(load().mirt_comm_selfcheck(C.c_size_t(int(nbytes))))


def view_array(views):
    arr = (View * len(views))()
    for i, v in enumerate(views):
        C.memmove(C.byref(arr[i]), C.byref(v), C.sizeof(View))
    return arr


def prepared_sharded(kind, views, lights7, indirect, mode, root, d_frames, pitch_bytes):
    """Zero-argument callable: this rank's band of len(views) frames + the gather on `root` (mirt_*_sharded)."""
    lib = load()
    arr = view_array(views)
    larr, nl = make_lights(lights7)
    ind = np.asarray(indirect, np.float32).copy()
    if kind == "rt":
        fn, args = lib.mirt_raytrace_sharded, (arr, len(views), larr, nl, _ptr(ind), int(mode), int(root), d_frames, int(pitch_bytes))
    else:
        fn, args = lib.mirt_rasterise_sharded, (arr, len(views), larr, nl, _ptr(ind), int(root), d_frames, int(pitch_bytes))

    def launch(_keep=(arr, larr, ind)):
        rc = fn(*args)
        if rc:
            _check(rc)
    return launch


def prepared_cull_device(view, flags=3):
    """Zero-argument callable that runs the cull step for `view` on the device (see prepared_raytrace_device)."""
    lib = load()
    ref = C.byref(view)
    fn = lib.mirt_cull_device

    def launch(_keep=(view,)):
        rc = fn(ref, int(flags))
        if rc:
            _check(rc)
    return launch


DEFAULT_LIGHT = np.array([[0.0, -0.5, -0.7, 1.0, 1.0, 1.0, 14.0]], np.float32)
