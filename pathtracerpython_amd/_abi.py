"""ctypes mirror of include/pt_capi.h (structs, flags, error codes)."""
import ctypes as C

PT_API_VERSION = 7

PT_OK = 0
PT_EINVAL = -1
PT_EHIP = -2
PT_ENOMEM = -3
PT_ENODEV = -4
PT_EUNSUPPORTED = -5
PT_ETIMEOUT = -6

PT_FLAG_RR = 1 << 0
PT_FLAG_FORCE_F64 = 1 << 1
PT_FLAG_COUNT = 1 << 2
PT_FLAG_OUT_F64 = 1 << 3
PT_FLAG_MEGAKERNEL = 1 << 4
PT_FLAG_WALK_COUNT = 1 << 5
PT_FLAG_KERNEL_TIMES = 1 << 6
# bit 7: reserved (v4's PT_FLAG_TREE_WALK, retired in v5)
PT_FLAG_AA = 1 << 8   # antialiasing: a jittered primary ray per sample
PT_FLAG_LENS = 1 << 9   # thin lens: a lens point per sample (a scene created with a lens)
PT_FLAG_RAYS_SINGLE = 1 << 10   # pt_radiance only: the single kernel k_render_rays whatever the scene

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class PtSceneDesc(C.Structure):
    _fields_ = [
        ("n_tri", C.c_int32), ("n_obj_tri", C.c_int32), ("n_obj", C.c_int32),
        ("reserved", C.c_int32),
        ("tri_v", _dp), ("tri_n", _dp), ("tri_area", _dp), ("tri_obj", _ip),
        ("mat", _dp),
        ("eye", C.c_double * 3), ("ortho", C.c_double * 4),
        ("ambient", C.c_double), ("light_rgb", C.c_double * 3),
    ]


class PtLens(C.Structure):
    """pt_lens (include/pt_capi.h): the aperture radius and the focal plane's z."""
    _fields_ = [("radius", C.c_double), ("focus_z", C.c_double)]


def make_lens(lens):
    """pt_lens of (R, zf)."""
    R, zf = lens
    L = PtLens()
    L.radius, L.focus_z = float(R), float(zf)
    return L


PT_PATH_NONE, PT_PATH_SINGLE, PT_PATH_WAVEFRONT = 0, 1, 2
PATH_NAMES = {PT_PATH_NONE: "none", PT_PATH_SINGLE: "single", PT_PATH_WAVEFRONT: "wavefront"}


class PtLaunchInfo(C.Structure):
    """pt_launch_info (include/pt_capi.h): which path a handle's last launch took."""
    _fields_ = [("path", C.c_int32), ("steps", C.c_int32), ("lanes_per_pixel", C.c_int32),
                ("flags", C.c_uint32)]


# pt_ray (include/pt_capi.h): a record of pt_radiance, 56 bytes
RAY_DTYPE = [("o", "<f8", (3,)), ("d", "<f8", (3,)), ("key", "<u4"), ("reserved", "<u4")]


def make_rays(origins, dirs, keys=None):
    """The pt_ray records of origins, dirs (n, 3) f64 and keys (n,) u32
    (None: 0..n-1), a numpy structured array."""
    import numpy as np
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError("origins and dirs must have the same length")
    if keys is None:
        k = np.arange(n, dtype=np.uint32)
    else:
        k = np.asarray(keys)
        if k.shape != (n,):
            raise ValueError("keys must be (n,)")
        if k.size and (k.min() < 0 or k.max() > 0xFFFFFFFF):
            raise ValueError("keys must fit 32 bits")
        k = k.astype(np.uint32)
    rec = np.zeros(n, dtype=np.dtype(RAY_DTYPE))
    assert rec.dtype.itemsize == 56
    rec["o"], rec["d"], rec["key"] = o, d, k
    return rec


class PtRenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
        ("bounces", C.c_int32), ("seed", C.c_uint64), ("flags", C.c_uint32),
        ("rr_depth", C.c_int32), ("row_begin", C.c_int32),
        ("row_end", C.c_int32), ("row_step", C.c_int32),
        ("row_phase", C.c_int32), ("sample_begin", C.c_int32),
        ("out_row_stride", C.c_int32), ("lanes_per_pixel", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PtAdaptParams(C.Structure):
    """pt_adapt_params (include/pt_capi.h): the stop rule of an adaptive run."""
    _fields_ = [("tol", C.c_double), ("floor", C.c_double), ("min_spp", C.c_int32),
                ("max_spp", C.c_int32), ("step_spp", C.c_int32), ("reserved", C.c_int32)]


def make_adapt(tol, max_spp, min_spp=8, step_spp=8, floor=0.01):
    a = PtAdaptParams()
    a.tol, a.floor = float(tol), float(floor)
    a.min_spp, a.max_spp, a.step_spp = int(min_spp), int(max_spp), int(step_spp)
    return a


class PtAccumBand(C.Structure):
    """pt_accum_band (include/pt_capi.h): the rows an accumulator works on and
    the fixed lanes per pixel of its passes."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("row_step", C.c_int32),
                ("row_phase", C.c_int32), ("lanes_per_pixel", C.c_int32), ("reserved", C.c_int32)]

    def rows(self):
        return (self.row_begin, self.row_end, self.row_step, self.row_phase)


def make_band(height, row_begin=0, row_end=None, row_step=1, row_phase=0, lanes_per_pixel=0):
    b = PtAccumBand()
    b.row_begin, b.row_end = int(row_begin), int(height if row_end is None else row_end)
    b.row_step, b.row_phase = int(row_step), int(row_phase)
    b.lanes_per_pixel = int(lanes_per_pixel)
    return b


def band_pixels(width, height, band):
    """numpy twin of band_pixel (pt_path.h): the whole-frame pixel indices
    e = (height-1-iy)*width + ix of the band's pixels, band rows top-first —
    an ascending int64 array of rows*width entries."""
    import numpy as np
    iy = np.array(band_rows(height, *band.rows())[::-1], dtype=np.int64)
    e = (height - 1 - iy)[:, None] * width + np.arange(width, dtype=np.int64)[None, :]
    return e.reshape(-1)


class PtDenoiseParams(C.Structure):
    """pt_denoise_params (include/pt_capi.h): the filter of a denoise."""
    _fields_ = [("sigma_l", C.c_double), ("sigma_z", C.c_double), ("eps", C.c_double),
                ("iters", C.c_int32), ("normal_sq", C.c_int32), ("reserved", C.c_int32)]


DENOISE_DEFAULTS = dict(iters=5, sigma_l=2.0, sigma_z=0.1, eps=1e-10, normal_sq=5)


def make_denoise(iters=5, sigma_l=2.0, sigma_z=0.1, eps=1e-10, normal_sq=5):
    d = PtDenoiseParams()
    d.sigma_l, d.sigma_z, d.eps = float(sigma_l), float(sigma_z), float(eps)
    d.iters, d.normal_sq = int(iters), int(normal_sq)
    return d


class PtMesh(C.Structure):
    """pt_mesh (include/pt_capi.h): a mesh read by pt_obj_load."""
    _fields_ = [("n_vert", C.c_int64), ("n_tri", C.c_int64), ("n_skip", C.c_int64),
                ("vert", C.POINTER(C.c_double)), ("face", C.POINTER(C.c_int64)),
                ("tri_v", C.POINTER(C.c_double)), ("tri_n", C.POINTER(C.c_double)),
                ("tri_area", C.POINTER(C.c_double)), ("skip_off", C.POINTER(C.c_int64)),
                ("skip_len", C.POINTER(C.c_int64))]


class PtStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "closest_tests", "shadow_tests", "ray_bounces", "shading_points",
        "light_hits", "escapes", "f64_fallbacks", "f64_rescans",
        "shadow_queries", "shadow_node_visits", "shadow_leaf_units",
        "closest_queries", "closest_node_visits", "closest_leaf_units")] + \
        [(n, C.c_double) for n in ("shade_ms", "shadow_ms", "closest_ms")] + \
        [(n, C.c_uint64) for n in ("shade_launches", "shadow_launches", "closest_launches")] + \
        [("sort_ms", C.c_double), ("sort_launches", C.c_uint64)]

    COUNTERS = ("closest_tests", "shadow_tests", "ray_bounces", "shading_points",
                "light_hits", "escapes", "f64_fallbacks", "f64_rescans")

    def as_dict(self, all_fields=False):
        """The reference-semantics counters (PT_FLAG_COUNT); all_fields adds
        the wavefront walk counts and per-kernel times."""
        names = [n for n, _ in self._fields_] if all_fields else self.COUNTERS
        return {n: (float if n.endswith("_ms") else int)(getattr(self, n)) for n in names}


def make_params(width, height, spp, bounces, seed, flags=0, rr_depth=3,
                row_begin=0, row_end=None, row_step=1, row_phase=0,
                sample_begin=0, out_row_stride=0, lanes_per_pixel=0):
    p = PtRenderParams()
    p.width, p.height, p.spp, p.bounces = int(width), int(height), int(spp), int(bounces)
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p.flags = int(flags)
    p.rr_depth = int(rr_depth)
    p.row_begin = int(row_begin)
    p.row_end = int(height if row_end is None else row_end)
    p.row_step = int(row_step)
    p.row_phase = int(row_phase)
    p.sample_begin = int(sample_begin)
    p.out_row_stride = int(out_row_stride)
    p.lanes_per_pixel = int(lanes_per_pixel)
    return p


def with_flags(p, add=0, **fields):
    """A copy of params p with flag bits `add` set and any fields replaced."""
    q = PtRenderParams()
    C.pointer(q)[0] = p
    q.flags = p.flags | int(add)
    for k, v in fields.items():
        setattr(q, k, int(v))
    return q


def band_rows(height, row_begin=0, row_end=None, row_step=1, row_phase=0):
    """Python twin of pt_band_rows: the iy values a launch renders, in order."""
    row_end = height if row_end is None else row_end
    return [iy for iy in range(row_begin, row_end) if iy % row_step == row_phase]
