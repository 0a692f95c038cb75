"""Adaptive sampling: render until every pixel's noise estimate is below a
target, within a per-pixel sample budget (build extension).

The reference spends `-r` samples on every pixel (main.py:186-271).  Here a
device-resident accumulator (`pt_accum`, include/pt_capi.h) keeps, per pixel,
the sum S of its sample colours, the per-channel sum of their squares Q and
the sample count n.  A run is a loop of passes: a select evaluates

    m_c = S_c / n
    v_c = max(0, Q_c - S_c*S_c / n) / (n - 1)
    err = sqrt((v_r + v_g + v_b) / n) / (|m_r| + |m_g| + |m_b| + floor)

(err = +inf below two samples), lists the pixels with
n < min_spp or (err > tol and n < max_spp), and a render pass adds
k = min(step_spp, (min_spp if n < min_spp else max_spp) - n) samples — the
sample indices n .. n+k-1 — to each listed pixel.  The run ends when the list
is empty.  The keyed RNG makes sample s of a pixel the same draw whichever
pass renders it, so a pixel that stopped at n samples holds what a uniform
render of n samples gives it (to ~1e-15 relative: the sum order).  The
list's length is the one value the host reads per pass.
"""
import ctypes as C
import weakref

import numpy as np

from . import _native
from ._abi import (PT_FLAG_FORCE_F64, PT_FLAG_MEGAKERNEL, PT_FLAG_OUT_F64, PT_FLAG_RR, PtStats,
                   make_adapt, make_denoise, make_params)


class AdaptiveResult:
    """fb (H, W, 3) f64 mean colours; counts (H, W) u32 samples per pixel;
    err (H, W) f64 the last error estimates; passes [(n_active,
    samples_added)]; samples the total.  After a run with denoise: denoised
    (H, W, 3) f64 the filtered frame, denoised_var (H, W, 3) f64 its variance
    estimate, features dict(tri, obj (H, W) i32; N, P (H, W, 3) f64) of the
    first hits; None otherwise."""

    def __init__(self, fb, counts, err, passes, denoised=None, denoised_var=None, features=None):
        self.fb, self.counts, self.err = fb, counts, err
        self.denoised, self.denoised_var, self.features = denoised, denoised_var, features
        self.passes = list(passes)
        self.samples = int(sum(s for _, s in self.passes))

    def __repr__(self):
        H, W = self.counts.shape
        return (f"AdaptiveResult({W}x{H}, {len(self.passes)} passes, {self.samples} samples, "
                f"{self.samples / max(1, W * H):.2f} spp mean)")


def check_rule(tol, max_spp, min_spp=8, step_spp=8, floor=0.01):
    """The argument checks of pt_adapt_params, before any device work."""
    if not (isinstance(min_spp, (int, np.integer)) and isinstance(max_spp, (int, np.integer))
            and isinstance(step_spp, (int, np.integer))):
        raise ValueError("min_spp, max_spp and step_spp must be integers")
    if not 2 <= min_spp <= max_spp:
        raise ValueError("need 2 <= min_spp <= max_spp")
    if step_spp < 1:
        raise ValueError("step_spp must be >= 1")
    if not tol >= 0:
        raise ValueError("tol must be >= 0")
    if not floor > 0:
        raise ValueError("floor must be > 0")


def pass_samples(n, min_spp, max_spp, step_spp):
    """k of the rule above for a pixel with n samples (0: at its goal)."""
    goal = min_spp if n < min_spp else max_spp
    return max(0, min(step_spp, goal - n))


class Accumulator:
    """A `pt_accum` of one (width, height) frame of a Renderer's scene."""

    def __init__(self, renderer, width, height):
        self._lib = renderer._lib
        self.renderer = renderer
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _native.check(self._lib.pt_accum_create(renderer._h, self.width, self.height, C.byref(h)),
                      "pt_accum_create")
        self._h = h
        # the accumulator must go before its scene: Renderer.close() closes
        # the accumulators still open on it first
        if not hasattr(renderer, "_accums"):
            renderer._accums = weakref.WeakSet()
        renderer._accums.add(self)

    def reset(self, stream=None):
        _native.check(self._lib.pt_accum_reset(self._h, C.c_void_p(stream or 0)), "pt_accum_reset")

    def select(self, adapt, stream=None):
        """(n_active, samples the pass will add)."""
        n, k = C.c_uint32(0), C.c_uint64(0)
        _native.check(self._lib.pt_accum_select(self._h, C.byref(adapt), C.c_void_p(stream or 0),
                                                C.byref(n), C.byref(k)), "pt_accum_select")
        return n.value, k.value

    def render(self, params, adapt, stream=None, stats=False):
        """One pass.  Scenes with a BVH take it through the wavefront kernels
        (PT_FLAG_MEGAKERNEL in params.flags: through the single kernel, the
        same S, Q, n bit for bit).  stats=True returns the pass's stats dict
        (pt_accum_render_stats): with PT_FLAG_WALK_COUNT / PT_FLAG_KERNEL_TIMES
        the walk counts / per-kernel launch counts and times of a wavefront
        pass, zeros after a single-kernel one."""
        if not stats:
            _native.check(self._lib.pt_accum_render(self._h, C.byref(params), C.byref(adapt),
                                                    C.c_void_p(stream or 0)), "pt_accum_render")
            return None
        st = PtStats()
        _native.check(self._lib.pt_accum_render_stats(self._h, C.byref(params), C.byref(adapt),
                                                      C.c_void_p(stream or 0), C.byref(st)),
                      "pt_accum_render_stats")
        return st.as_dict(all_fields=True)

    def resolve_device(self, out_ptr, f64=True, stream=None):
        _native.check(self._lib.pt_accum_resolve_device(self._h, PT_FLAG_OUT_F64 if f64 else 0,
                                                        C.c_void_p(out_ptr), C.c_void_p(stream or 0)),
                      "pt_accum_resolve_device")

    def read(self, S=False, Q=False, n=False, err=False, active=False):
        """The requested arrays as a dict: S, Q (H, W, 3) f64; n (H, W) u32;
        err (H, W) f64; list (the last select's active list, u32)."""
        H, W = self.height, self.width
        out = {}
        if S:
            out["S"] = np.zeros((H, W, 3), dtype=np.float64)
        if Q:
            out["Q"] = np.zeros((H, W, 3), dtype=np.float64)
        if n:
            out["n"] = np.zeros((H, W), dtype=np.uint32)
        if err:
            out["err"] = np.zeros((H, W), dtype=np.float64)
        lst = np.zeros(H * W, dtype=np.uint32) if active else None
        ln = C.c_uint32(0)

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        _native.check(self._lib.pt_accum_read(
            self._h, ptr("S", C.c_double), ptr("Q", C.c_double), ptr("n", C.c_uint32),
            ptr("err", C.c_double),
            lst.ctypes.data_as(C.POINTER(C.c_uint32)) if active else None,
            H * W if active else 0, C.byref(ln) if active else None), "pt_accum_read")
        if active:
            out["list"] = lst[:ln.value].copy()
        return out

    def features(self, stream=None):
        """The first-hit features of the frame (pt_accum_features, computed
        once and kept on the device): dict(tri, obj (H, W) i32 — -1 for an
        escape; N, P (H, W, 3) f64 the hit triangle's normal and the hit
        point, 0 for an escape)."""
        H, W = self.height, self.width
        _native.check(self._lib.pt_accum_features(self._h, C.c_void_p(stream or 0)), "pt_accum_features")
        out = dict(tri=np.zeros((H, W), dtype=np.int32), obj=np.zeros((H, W), dtype=np.int32),
                   N=np.zeros((H, W, 3), dtype=np.float64), P=np.zeros((H, W, 3), dtype=np.float64))
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        _native.check(self._lib.pt_accum_read_features(
            self._h, out["tri"].ctypes.data_as(ip), out["obj"].ctypes.data_as(ip),
            out["N"].ctypes.data_as(dp), out["P"].ctypes.data_as(dp)), "pt_accum_read_features")
        return out

    def denoise_device(self, out_ptr, var_ptr=None, f64=True, stream=None, **params):
        """The filtered frame of the present state into device buffers
        (pt_accum_denoise_device; params: make_denoise's)."""
        d = make_denoise(**params)
        _native.check(self._lib.pt_accum_denoise_device(
            self._h, C.byref(d), PT_FLAG_OUT_F64 if f64 else 0, C.c_void_p(out_ptr),
            C.c_void_p(var_ptr or 0), C.c_void_p(stream or 0)), "pt_accum_denoise_device")

    def denoise(self, f64=True, **params):
        """(filtered frame, its variance), (H, W, 3) f64 (f32 with f64=False):
        the edge-avoiding filter of include/pt_capi.h (pt_denoise_params) on
        the accumulator's present moments.  S, Q, n and the list stay as
        they are."""
        import torch
        H, W = self.height, self.width
        dt = torch.float64 if f64 else torch.float32
        dev = self.renderer.device
        with torch.cuda.device(torch.cuda.current_device() if dev is None else int(dev)):
            out = torch.empty((H, W, 3), dtype=dt, device="cuda")
            var = torch.empty((H, W, 3), dtype=dt, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            self.denoise_device(out.data_ptr(), var.data_ptr(), f64, s, **params)
            return out.cpu().numpy(), var.cpu().numpy()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pt_accum_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_passes(acc, params, adapt, on_pass=None, max_passes=None):
    """The pass loop on an accumulator (anything with select / render): select,
    stop on an empty list, render.  Returns [(n_active, samples_added)]."""
    passes = []
    # every pass adds at least one sample to each listed pixel, so a run has at
    # most max_spp passes (+1 for the closing select): a longer one is a bug
    limit = int(adapt.max_spp) + 1 if max_passes is None else int(max_passes)
    while True:
        n_active, k = acc.select(adapt)
        if n_active == 0:
            return passes
        if len(passes) >= limit:
            raise RuntimeError(f"adaptive run did not end within {limit} passes")
        acc.render(params, adapt)
        passes.append((int(n_active), int(k)))
        if on_pass is not None:
            on_pass(len(passes), int(n_active), int(k))


def render_adaptive(renderer, width=None, height=None, max_spp=64, bounces=1, seed=None, rr=False,
                    rr_depth=3, tol=0.05, min_spp=8, step_spp=8, floor=0.01, force_f64=False,
                    on_pass=None, megakernel=False, denoise=None):
    """Render until err <= tol everywhere or a pixel has max_spp samples.

    renderer: a render.Renderer.  on_pass(i, n_active, samples_added) after
    each pass.  megakernel=True: scenes with a BVH take their passes through
    the single kernel instead of the wavefront kernels (the same result, bit
    for bit).  denoise: None, True (the default filter) or a dict of
    make_denoise's parameters — the result then also holds the filtered
    frame, its variance and the first-hit features (Accumulator.denoise).
    Returns an AdaptiveResult."""
    check_rule(tol, max_spp, min_spp, step_spp, floor)
    if denoise is not None and denoise is not True and not isinstance(denoise, dict):
        raise ValueError("denoise: None, True or a dict of filter parameters")
    width = int(renderer.scene.width if width is None else width)
    height = int(renderer.scene.height if height is None else height)
    seed = renderer.scene.seed if seed is None else seed
    seed = 0 if seed is None else int(seed)
    flags = (PT_FLAG_RR if rr else 0) | (PT_FLAG_FORCE_F64 if force_f64 else 0) | \
        (PT_FLAG_MEGAKERNEL if megakernel else 0)
    params = make_params(width, height, max_spp, bounces, seed, flags, rr_depth)
    adapt = make_adapt(tol, max_spp, min_spp, step_spp, floor)
    with Accumulator(renderer, width, height) as acc:
        passes = run_passes(acc, params, adapt, on_pass)
        d = acc.read(S=True, n=True, err=True)
        den = var = feat = None
        if denoise is not None:
            den, var = acc.denoise(**(denoise if isinstance(denoise, dict) else {}))
            feat = acc.features()
    n = d["n"]
    fb = np.where(n[..., None] > 0, d["S"] / np.maximum(n, 1)[..., None], 0.0)
    return AdaptiveResult(fb, n, d["err"], passes, den, var, feat)
