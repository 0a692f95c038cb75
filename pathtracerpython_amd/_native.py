"""ctypes binding of libpt_hip.so (include/pt_capi.h).

The HIP library is the only implementation of the hot path: there is no CPU
fallback.  If the library is missing or no gfx950 device is visible, calls
raise `NativeError` — loudly, never silently.
"""
import ctypes as C
import os

from ._abi import PtAccumBand, PtAdaptParams, PtDenoiseParams, PtLaunchInfo, PtLens, PtMesh, PtRenderParams, PtSceneDesc, PtStats  # noqa: F401 (PtMesh re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_HIP_LIB", os.path.join(HERE, "_lib", "libpt_hip.so"))

_lib = None


class NativeError(RuntimeError):
    pass


def _bind(lib):
    vp = C.c_void_p
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    sig = {
        "pt_api_version": ([], C.c_int),
        "pt_last_error": ([], C.c_char_p),
        "pt_build_id": ([], C.c_char_p),
        "pt_test_fault_inject": ([C.c_int32], C.c_int),
        "pt_device_count": ([ip], C.c_int),
        "pt_scene_create": ([C.POINTER(PtSceneDesc), C.POINTER(vp)], C.c_int),
        "pt_scene_create_on": ([C.POINTER(PtSceneDesc), C.c_int32, C.POINTER(vp)], C.c_int),
        "pt_scene_create_lens": ([C.POINTER(PtSceneDesc), C.c_int32, C.POINTER(PtLens), C.POINTER(vp)], C.c_int),
        "pt_scene_create_rays": ([C.POINTER(PtSceneDesc), C.c_int32, dp, C.POINTER(vp)], C.c_int),
        "pt_radiance_device": ([vp, vp, C.c_int64, C.POINTER(PtRenderParams), vp, vp, vp, vp], C.c_int),
        "pt_radiance": ([vp, vp, C.c_int64, C.POINTER(PtRenderParams), vp, vp, vp], C.c_int),
        "pt_render_multi": ([C.POINTER(vp), C.c_int32, C.POINTER(PtRenderParams), vp,
                             C.POINTER(PtStats)], C.c_int),
        "pt_scene_destroy": ([vp], None),
        "pt_band_rows": ([C.POINTER(PtRenderParams), ip], C.c_int),
        "pt_render_device": ([vp, C.POINTER(PtRenderParams), vp, vp, C.POINTER(PtStats)], C.c_int),
        "pt_render": ([vp, C.POINTER(PtRenderParams), vp, C.POINTER(PtStats)], C.c_int),
        "pt_last_kernel_ms": ([vp, C.POINTER(C.c_float)], C.c_int),
        "pt_last_launch_info": ([vp, C.POINTER(PtLaunchInfo)], C.c_int),
        "pt_intersect_objects": ([vp, dp, C.c_int64, ip, dp], C.c_int),
        "pt_compute_color": ([vp, ip, dp, dp, dp, C.c_int64, dp], C.c_int),
        "pt_image_u8_device": ([vp, C.c_int32, C.c_int32, C.c_uint32, vp, vp], C.c_int),
        "pt_image_u8": ([vp, C.c_int32, C.c_int32, C.c_uint32, vp], C.c_int),
        "pt_assemble_bands_device": ([vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                      vp, vp], C.c_int),
        "pt_host_map": ([vp, C.c_uint64, C.POINTER(vp)], C.c_int),
        "pt_host_unmap": ([vp], C.c_int),
        "pt_signal": ([vp, C.c_uint64, vp], C.c_int),
        "pt_wait_flags": ([vp, C.c_int32, C.c_int32, C.c_uint64, C.c_double], C.c_int),
        "pt_obj_load": ([C.c_char_p, C.POINTER(C.POINTER(PtMesh))], C.c_int),
        "pt_mesh_free": ([C.POINTER(PtMesh)], None),
        # adaptive sampling (v7, additive)
        "pt_accum_create": ([vp, C.c_int32, C.c_int32, C.POINTER(vp)], C.c_int),
        "pt_accum_destroy": ([vp], None),
        "pt_accum_reset": ([vp, vp], C.c_int),
        "pt_accum_select": ([vp, C.POINTER(PtAdaptParams), vp, C.POINTER(C.c_uint32),
                             C.POINTER(C.c_uint64)], C.c_int),
        "pt_accum_render": ([vp, C.POINTER(PtRenderParams), C.POINTER(PtAdaptParams), vp], C.c_int),
        "pt_accum_render_stats": ([vp, C.POINTER(PtRenderParams), C.POINTER(PtAdaptParams), vp,
                                   C.POINTER(PtStats)], C.c_int),
        "pt_accum_resolve_device": ([vp, C.c_uint32, vp, vp], C.c_int),
        "pt_accum_read": ([vp, dp, dp, C.POINTER(C.c_uint32), dp, C.POINTER(C.c_uint32), C.c_uint32,
                           C.POINTER(C.c_uint32)], C.c_int),
        # bands, band tiles, host restore (v7, additive)
        "pt_accum_set_band": ([vp, C.POINTER(PtAccumBand)], C.c_int),
        "pt_accum_tile_bytes": ([C.c_int32, C.c_int32, C.POINTER(C.c_uint64)], C.c_int),
        "pt_accum_export_band_device": ([vp, vp, vp], C.c_int),
        "pt_accum_import_band_device": ([vp, C.POINTER(PtAccumBand), vp, vp], C.c_int),
        "pt_accum_write": ([vp, dp, dp, C.POINTER(C.c_uint32)], C.c_int),
        # ray accumulators (v7, additive)
        "pt_accum_create_rays": ([vp, vp, C.c_int32, C.c_int32, C.POINTER(vp)], C.c_int),
        # denoising (additive)
        "pt_denoise_device": ([C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), vp, vp, vp, vp, vp,
                               C.c_uint32, vp, vp, vp], C.c_int),
        "pt_denoise": ([C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), vp, vp, vp, vp, vp,
                        C.c_uint32, vp, vp], C.c_int),
        "pt_denoise_times": ([C.c_int32, C.POINTER(C.c_float), C.c_int32, ip], C.c_int),
        "pt_accum_features": ([vp, vp], C.c_int),
        "pt_accum_read_features": ([vp, ip, ip, dp, dp], C.c_int),
        "pt_accum_denoise_device": ([vp, C.POINTER(PtDenoiseParams), C.c_uint32, vp, vp, vp], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


EXPORTS = ("pt_api_version", "pt_last_error", "pt_build_id", "pt_test_fault_inject",
           "pt_device_count", "pt_scene_create",
           "pt_scene_create_on", "pt_scene_create_lens", "pt_render_multi", "pt_scene_destroy", "pt_band_rows",
           "pt_render_device", "pt_render", "pt_last_kernel_ms", "pt_intersect_objects", "pt_compute_color",
           "pt_image_u8_device", "pt_image_u8", "pt_assemble_bands_device", "pt_host_map",
           "pt_host_unmap", "pt_signal", "pt_wait_flags", "pt_obj_load", "pt_mesh_free",
           "pt_accum_create", "pt_accum_destroy", "pt_accum_reset", "pt_accum_select",
           "pt_accum_render", "pt_accum_render_stats", "pt_accum_resolve_device", "pt_accum_read",
           "pt_denoise_device", "pt_denoise", "pt_denoise_times", "pt_accum_features", "pt_accum_read_features",
           "pt_accum_denoise_device", "pt_accum_set_band", "pt_accum_tile_bytes",
           "pt_accum_export_band_device", "pt_accum_import_band_device", "pt_accum_write",
           "pt_last_launch_info", "pt_scene_create_rays", "pt_radiance_device", "pt_radiance",
           "pt_accum_create_rays")


def lib():
    """Load libpt_hip.so once.  torch (if present) is imported first so the
    library binds to the same HIP runtime instance torch uses."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        import torch  # noqa: F401  (shares libamdhip64 with torch)
    except Exception:
        pass
    raw = C.CDLL(LIB_PATH)
    from ._abi import PT_API_VERSION
    if not hasattr(raw, "pt_build_id") or raw.pt_api_version() != PT_API_VERSION:
        raise NativeError(f"{LIB_PATH} has C-ABI version {raw.pt_api_version()}, this binding "
                          f"needs {PT_API_VERSION}: rebuild it (python __graft_entry__.py build)")
    lib_ = _bind(raw)
    got = lib_.pt_build_id().decode("ascii", "replace")
    want = source_sha()
    # a library built from other sources than those on disk is refused, so a
    # measurement never carries the wrong sources' name (build.py); dev
    # variants built from patched sources opt out explicitly and are still
    # named by their own id (bench.py reports build_id())
    if got != want and os.environ.get("PT_ALLOW_FOREIGN_BUILD") != "1":
        raise NativeError(f"{LIB_PATH} was built from sources {got}, the sources on disk are {want}: "
                          "rebuild it (python __graft_entry__.py build)")
    _lib = lib_
    return _lib


def source_sha():
    from .build import source_sha as sha
    return sha()


def build_id():
    """The loaded library's PT_BUILD_ID (the content hash of its sources)."""
    return lib().pt_build_id().decode("ascii", "replace")


def last_error():
    msg = lib().pt_last_error()
    return msg.decode() if msg else ""


def check(rc, what):
    if rc != 0:
        raise NativeError(f"{what} failed ({rc}): {last_error()}")


def device_count():
    n = C.c_int32(0)
    check(lib().pt_device_count(C.byref(n)), "pt_device_count")
    return n.value
