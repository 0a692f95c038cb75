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

A pixel's trajectory through the passes depends on nothing but its own S, Q
and n.  So an accumulator can be restricted to a band of rows (set_band) and
N of them, one per device, run their own pass loops with no exchange until
the end (render.MultiRenderer.render_adaptive; band tiles move the state:
export_band / import_band); and a run can be cut between any two passes and
continued from its moments (AccumCheckpoint, Accumulator.write).

The same for rays the caller supplies (RayAccumulator, render_rays_adaptive;
pt_accum_create_rays): element e of the accumulator belongs to ray record e,
sample s of a record is pt_radiance's sample s, and everything above — the
rule, the bands, the checkpoints, the denoiser — works on the records' shape.
"""
import hashlib
import ctypes as C
import json
import os
import time
import weakref

import numpy as np

from . import _native
from ._abi import (PT_FLAG_AA, PT_FLAG_FORCE_F64, PT_FLAG_LENS, PT_FLAG_MEGAKERNEL, PT_FLAG_OUT_F64, PT_FLAG_RR, PtAccumBand,
                   PtStats, band_pixels, make_adapt, make_band, make_denoise, make_params, make_rays)
from .progressive import lens_of, scene_fingerprint


class AdaptiveResult:
    """fb (H, W, 3) f64 mean colours; counts (H, W) u32 samples per pixel;
    err (H, W) f64 the last error estimates; passes [(n_active,
    samples_added)]; samples the total.  After a run with denoise: denoised
    (H, W, 3) f64 the filtered frame, denoised_var (H, W, 3) f64 its variance
    estimate, features dict(tri, obj (H, W) i32; N, P (H, W, 3) f64) of the
    first hits; None otherwise.  After a run with moments=True: S, Q
    (H, W, 3) f64, the sums the run ended with; None otherwise."""

    def __init__(self, fb, counts, err, passes, denoised=None, denoised_var=None, features=None,
                 S=None, Q=None):
        self.fb, self.counts, self.err = fb, counts, err
        self.S, self.Q = S, Q
        self.denoised, self.denoised_var, self.features = denoised, denoised_var, features
        self.passes = list(passes)
        self.samples = int(sum(s for _, s in self.passes))

    def __repr__(self):
        shape = "x".join(str(v) for v in self.counts.shape[::-1])   # (a flat ray batch: its length)
        return (f"AdaptiveResult({shape}, {len(self.passes)} passes, {self.samples} samples, "
                f"{self.samples / max(1, self.counts.size):.2f} spp mean)")


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


def tile_bytes(width, rows):
    """Bytes of a band tile of rows*width pixels (pt_accum_tile_bytes)."""
    return 60 * int(rows) * int(width)


def tile_sections(buf, pixels):
    """The four sections of a band tile held in the uint8 array `buf`
    (include/pt_capi.h): views S, Q (P, 3) f64, err (P,) f64, n (P,) u32."""
    P = int(pixels)
    return dict(S=buf[:24 * P].view(np.float64).reshape(P, 3),
                Q=buf[24 * P:48 * P].view(np.float64).reshape(P, 3),
                err=buf[48 * P:56 * P].view(np.float64), n=buf[56 * P:60 * P].view(np.uint32))


class Accumulator:
    """A `pt_accum` of one (width, height) frame of a Renderer's scene; band
    (a PtAccumBand, _abi.make_band): the rows it works on and the fixed lanes
    per pixel of its passes (default: the whole frame, chosen per pass)."""

    def __init__(self, renderer, width, height, band=None):
        self._lib = renderer._lib
        self.renderer = renderer
        self.width, self.height = int(width), int(height)
        self._h = self._create(renderer)
        # the accumulator must go before its scene: Renderer.close() closes
        # the accumulators still open on it first
        if not hasattr(renderer, "_accums"):
            renderer._accums = weakref.WeakSet()
        renderer._accums.add(self)
        self.band = make_band(self.height)
        if band is not None:
            self.set_band(band)

    def _create(self, renderer):
        h = C.c_void_p()
        _native.check(self._lib.pt_accum_create(renderer._h, self.width, self.height, C.byref(h)),
                      "pt_accum_create")
        return h

    def set_band(self, band):
        """Restrict the selects, and so the passes, to the rows of `band`
        (pt_accum_set_band); make_band(height) is the whole frame again."""
        _native.check(self._lib.pt_accum_set_band(self._h, C.byref(band)), "pt_accum_set_band")
        b = PtAccumBand()
        C.pointer(b)[0] = band
        self.band = b

    def _device(self):
        import torch
        dev = self.renderer.device
        return torch.cuda.device(torch.cuda.current_device() if dev is None else int(dev))

    def export_band_device(self, ptr, stream=None):
        """The band's tile (include/pt_capi.h: S, Q, err, n of its pixels,
        top-first) into tile_bytes() of device memory at ptr, asynchronous."""
        _native.check(self._lib.pt_accum_export_band_device(self._h, C.c_void_p(ptr), C.c_void_p(stream or 0)),
                      "pt_accum_export_band_device")

    def export_band(self):
        """dict of numpy S, Q (P, 3) f64, err (P,) f64, n (P,) u32 for the P
        pixels of the band's rows, in the order of _abi.band_pixels."""
        import torch
        P = len(band_pixels(self.width, self.height, self.band))
        with self._device():
            tile = torch.empty(max(60 * P, 8), dtype=torch.uint8, device="cuda")
            self.export_band_device(tile.data_ptr(), torch.cuda.current_stream().cuda_stream)
            buf = tile.cpu().numpy()
        return {k: v.copy() for k, v in tile_sections(buf, P).items()}

    def import_band(self, band, tile, stream=None):
        """Overwrite S, Q, err and n of the rows of `band` with a tile: a
        device pointer (int) of this accumulator's device — asynchronous on
        `stream` — or the dict form of export_band (copied up first).  The
        accumulator's own band stays."""
        if isinstance(tile, dict):
            import torch
            P = len(band_pixels(self.width, self.height, band))
            buf = np.zeros(max(60 * P, 8), dtype=np.uint8)
            sec = tile_sections(buf, P)
            for k in ("S", "Q", "err", "n"):
                sec[k][...] = np.asarray(tile[k]).reshape(sec[k].shape)
            with self._device():
                dev = torch.from_numpy(buf).cuda()
                s = torch.cuda.current_stream().cuda_stream
                _native.check(self._lib.pt_accum_import_band_device(
                    self._h, C.byref(band), C.c_void_p(dev.data_ptr()), C.c_void_p(s)),
                    "pt_accum_import_band_device")
                torch.cuda.current_stream().synchronize()   # dev is freed on return
            return
        _native.check(self._lib.pt_accum_import_band_device(
            self._h, C.byref(band), C.c_void_p(int(tile)), C.c_void_p(stream or 0)),
            "pt_accum_import_band_device")

    def write(self, S, Q, n):
        """Replace the whole frame's S, Q (H, W, 3) f64 and n (H, W) u32
        (pt_accum_write, synchronous): err becomes +inf, the list is dropped."""
        H, W = self.height, self.width
        S = np.ascontiguousarray(S, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        if S.shape != (H, W, 3) or Q.shape != (H, W, 3) or n.shape != (H, W):
            raise ValueError("write: S, Q must be (H, W, 3) and n (H, W)")
        dp = C.POINTER(C.c_double)
        _native.check(self._lib.pt_accum_write(self._h, S.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                               n.ctypes.data_as(C.POINTER(C.c_uint32))), "pt_accum_write")

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
        with self._device():
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


def ray_records(o, d, keys=None, shape=None):
    """(records, (H, W)) of a ray accumulator: the pt_ray records of o, d
    (n, 3) f64 and keys (n,) u32 (None: 0..n-1) as element e's, and the shape
    they fill — (1, n) for a flat batch, shape=(H, W) with H*W = n for an image
    whose records are in image orientation, e = (H-1-iy)*W + ix."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    if shape is None:
        H, W = 1, n
    else:
        H, W = (int(v) for v in shape)
        if H < 1 or W < 1 or H * W != n:
            raise ValueError(f"shape {tuple(shape)} does not hold the {n} records")
    if not 1 <= n < 1 << 30:
        raise ValueError("a ray accumulator needs 1 <= n < 2^30 records")
    return rec, (H, W)


class RayAccumulator(Accumulator):
    """A `pt_accum` whose element e belongs to ray record e instead of a pixel
    of the scene's camera (pt_accum_create_rays): o, d (n, 3) f64 and keys
    (n,) u32 as for Renderer.render_rays; shape=None is a flat batch (height
    1, width n), shape=(H, W) an image of records in image orientation.  The
    records are uploaded and copied by the library at create.  Every method of
    Accumulator applies, on the arrays' (H, W) shape."""

    def __init__(self, renderer, o, d, keys=None, shape=None, band=None):
        self.records, (H, W) = ray_records(o, d, keys, shape)
        super().__init__(renderer, W, H, band)

    def _create(self, renderer):
        import torch
        h = C.c_void_p()
        with self._device():
            dev = torch.from_numpy(self.records.view(np.uint8)).cuda()
            torch.cuda.current_stream().synchronize()   # the upload has landed
            _native.check(self._lib.pt_accum_create_rays(renderer._h, C.c_void_p(dev.data_ptr()), self.width,
                                                         self.height, C.byref(h)), "pt_accum_create_rays")
        return h   # (the library made its own copy: dev may go)


def _pass_loop(acc, params, adapt, on_pass, limit, done=(), stop_after=None, after_pass=None):
    """select, stop on an empty list, render — continuing the passes `done`.
    Returns (passes, finished): finished False when stop_after passes were
    made in this call and the list is not empty."""
    passes = list(done)
    made = 0
    while True:
        n_active, k = acc.select(adapt)
        if n_active == 0:
            return passes, True
        if stop_after is not None and made >= stop_after:
            return passes, False
        if len(passes) >= limit:
            raise RuntimeError(f"adaptive run did not end within {limit} passes")
        acc.render(params, adapt)
        passes.append((int(n_active), int(k)))
        made += 1
        if after_pass is not None:
            after_pass(passes)
        if on_pass is not None:
            on_pass(len(passes), int(n_active), int(k))


def run_passes(acc, params, adapt, on_pass=None, max_passes=None):
    """The pass loop on an accumulator (anything with select / render): select,
    stop on an empty list, render.  Returns [(n_active, samples_added)]."""
    # every pass adds at least one sample to each listed pixel, so a run has at
    # most max_spp passes (+1 for the closing select): a longer one is a bug
    limit = int(adapt.max_spp) + 1 if max_passes is None else int(max_passes)
    return _pass_loop(acc, params, adapt, on_pass, limit)[0]


class AccumCheckpoint:
    """The moments of an adaptive run in one .npz file (written whole to a
    temporary name, then renamed over the old one, as progressive.Checkpoint):
    S, Q, n and the passes made so far.  The key is what defines a sample —
    scene, size, bounces, seed, rr, rr_depth, lanes_per_pixel, and "aa" when
    antialiasing is on (absent otherwise); the stop rule
    is stored beside it but is no part of it: resuming with a lower tol or a
    larger budget is the point of keeping moments."""

    def __init__(self, path):
        self.path = str(path)

    def load(self, key):
        """dict(S, Q, n, passes, rule) when the file holds a run with this
        key; None when there is no file.  A file of another render is an
        error, not a silent restart."""
        if not os.path.exists(self.path):
            return None
        with np.load(self.path, allow_pickle=False) as z:
            got = json.loads(str(z["key"]))
            if got != key:
                raise ValueError(f"checkpoint {self.path} belongs to another render: {got} != {key}")
            passes = [(int(a), int(k)) for a, k in np.array(z["passes"]).reshape(-1, 2)]
            return dict(S=np.array(z["S"], dtype=np.float64), Q=np.array(z["Q"], dtype=np.float64),
                        n=np.array(z["n"], dtype=np.uint32), passes=passes,
                        rule=json.loads(str(z["rule"])))

    def save(self, key, rule, S, Q, n, passes):
        tmp = self.path + ".tmp.npz"
        np.savez(tmp, key=np.array(json.dumps(key, sort_keys=True)),
                 rule=np.array(json.dumps(rule, sort_keys=True)), S=S, Q=Q, n=np.asarray(n, dtype=np.uint32),
                 passes=np.array(passes, dtype=np.int64).reshape(-1, 2))
        os.replace(tmp, self.path)

    def remove(self):
        if os.path.exists(self.path):
            os.remove(self.path)


def accum_key(packed, width, height, bounces, seed, rr, rr_depth, lanes_per_pixel, aa=False, lens=None,
              rays=None, shape=None):
    """AccumCheckpoint's key: what defines sample s of a pixel and the sum
    order of the moments.  "aa" is present only when antialiasing is on and
    "lens": [R, zf] only when the samples go through a lens, so the keys and
    files from before them stay valid.  rays: the pt_ray records of a ray
    accumulator — the key then holds "rays", the sha256 of their bytes, and
    "shape", the shape of the run's arrays ([n] or [H, W]); absent otherwise."""
    key = {"scene": scene_fingerprint(packed), "width": int(width), "height": int(height),
           "bounces": int(bounces), "seed": int(seed), "rr": bool(rr),
           "rr_depth": int(rr_depth), "lanes_per_pixel": int(lanes_per_pixel)}
    if aa:
        key["aa"] = True
    if lens is not None:
        key["lens"] = [float(lens[0]), float(lens[1])]
    if rays is not None:
        key["rays"] = hashlib.sha256(np.ascontiguousarray(rays).tobytes()).hexdigest()
        key["shape"] = [int(v) for v in (shape if shape is not None else (len(rays),))]
    return key


def render_adaptive(renderer, width=None, height=None, max_spp=64, bounces=1, seed=None, rr=False,
                    rr_depth=3, tol=0.05, min_spp=8, step_spp=8, floor=0.01, force_f64=False,
                    on_pass=None, megakernel=False, denoise=None, lanes_per_pixel=0, checkpoint=None,
                    checkpoint_every=1, max_passes=None, moments=False, aa=False, lens=None):
    """Render until err <= tol everywhere or a pixel has max_spp samples.

    renderer: a render.Renderer.  on_pass(i, n_active, samples_added) after
    each pass.  megakernel=True: scenes with a BVH take their passes through
    the single kernel instead of the wavefront kernels (the same result, bit
    for bit).  denoise: None, True (the default filter) or a dict of
    make_denoise's parameters — the result then also holds the filtered
    frame, its variance and the first-hit features (Accumulator.denoise).
    lanes_per_pixel: 0 lets the library choose per pass; a fixed power of two
    makes the moments independent of how the frame is split into bands
    (include/pt_capi.h, pt_accum_band).  checkpoint: a path (or
    AccumCheckpoint) to resume from and to write after every
    checkpoint_every-th pass and at the end.  max_passes: stop after this
    many passes in this call (returns None when passes remain, the
    checkpoint written).  moments=True: the result also holds S and Q.
    aa=True: antialiasing, every sample has its own jittered primary ray
    (PT_FLAG_AA); the features and the denoiser keep the centre ray.
    lens: the samples go through the renderer's lens (PT_FLAG_LENS; None: iff
    it has one); the features and the denoiser keep the pinhole's centre ray.
    Returns an AdaptiveResult."""
    check_rule(tol, max_spp, min_spp, step_spp, floor)
    if denoise is not None and denoise is not True and not isinstance(denoise, dict):
        raise ValueError("denoise: None, True or a dict of filter parameters")
    if int(checkpoint_every) < 1:
        raise ValueError("checkpoint_every must be >= 1")
    width = int(renderer.scene.width if width is None else width)
    height = int(renderer.scene.height if height is None else height)
    seed = renderer.scene.seed if seed is None else seed
    seed = 0 if seed is None else int(seed)
    through = lens_of(renderer, lens)
    flags = (PT_FLAG_RR if rr else 0) | (PT_FLAG_FORCE_F64 if force_f64 else 0) | \
        (PT_FLAG_MEGAKERNEL if megakernel else 0) | (PT_FLAG_AA if aa else 0) | \
        (PT_FLAG_LENS if through is not None else 0)
    params = make_params(width, height, max_spp, bounces, seed, flags, rr_depth)
    adapt = make_adapt(tol, max_spp, min_spp, step_spp, floor)
    ck = checkpoint if isinstance(checkpoint, AccumCheckpoint) or checkpoint is None \
        else AccumCheckpoint(checkpoint)
    key = None
    if ck is not None:
        key = accum_key(renderer.packed, width, height, bounces, params.seed, rr, rr_depth,
                        lanes_per_pixel, aa, through)
    # (the whole frame; a band only to carry the fixed lane count)
    kw = dict(band=make_band(height, lanes_per_pixel=lanes_per_pixel)) if lanes_per_pixel else {}
    return _run(lambda: Accumulator(renderer, width, height, **kw), width, height, params, adapt, ck, key,
                on_pass, max_passes, checkpoint_every, moments, denoise)


def _run(make_acc, width, height, params, adapt, ck, key, on_pass, max_passes, checkpoint_every, moments,
         denoise, shape=None):
    """The run of render_adaptive / render_rays_adaptive on the accumulator
    make_acc() opens: resume from the checkpoint ck (key: accum_key's), the
    pass loop, the closing read and the denoise.  shape: the shape the
    result's arrays get in place of (height, width) (a flat ray batch)."""
    rule = state = None
    if ck is not None:
        # (read back from the ctypes record: c_double and int32 fields, so the
        # values are the callers' arguments; a narrower field type in
        # make_adapt would change what the file records)
        rule = {"tol": float(adapt.tol), "min_spp": int(adapt.min_spp), "max_spp": int(adapt.max_spp),
                "step_spp": int(adapt.step_spp), "floor": float(adapt.floor)}
        state = ck.load(key)
        if state is not None and (state["S"].shape != (height, width, 3) or
                                  state["Q"].shape != (height, width, 3) or
                                  state["n"].shape != (height, width)):
            raise ValueError(f"checkpoint state does not fit the render: {state['S'].shape}")
    with make_acc() as acc:
        done = []
        if state is not None:
            acc.write(state["S"], state["Q"], state["n"])
            done = state["passes"]

        def save(passes):
            m = acc.read(S=True, Q=True, n=True)
            ck.save(key, rule, m["S"], m["Q"], m["n"], passes)

        def after_pass(passes):
            if (len(passes) - len(done)) % int(checkpoint_every) == 0:
                save(passes)
        # at most max_spp passes take a pixel from 0 to max_spp, whatever rule
        # the earlier part of a resumed run followed (+1: the closing select)
        limit = len(done) + int(adapt.max_spp) + 1
        passes, finished = _pass_loop(acc, params, adapt, on_pass, limit, done, max_passes,
                                      after_pass if ck is not None else None)
        if ck is not None and (len(passes) - len(done)) % int(checkpoint_every) != 0:
            save(passes)
        if not finished:
            return None
        d = acc.read(S=True, Q=bool(moments), n=True, err=True)
        den = var = feat = None
        if denoise is not None:
            den, var = acc.denoise(**(denoise if isinstance(denoise, dict) else {}))
            feat = acc.features()
    if shape is not None:   # (height, width, ...) -> shape + (...)
        def fit(x):
            return None if x is None else x.reshape(tuple(shape) + x.shape[2:])
        d = {k: fit(v) for k, v in d.items()}
        den, var = fit(den), fit(var)
        feat = None if feat is None else {k: fit(v) for k, v in feat.items()}
    n = d["n"]
    fb = np.where(n[..., None] > 0, d["S"] / np.maximum(n, 1)[..., None], 0.0)
    return AdaptiveResult(fb, n, d["err"], passes, den, var, feat,
                          *((d["S"], d["Q"]) if moments else ()))


def render_rays_adaptive(renderer, o, d, keys=None, shape=None, max_spp=64, bounces=1, tol=0.05, min_spp=8,
                         step_spp=8, floor=0.01, seed=None, rr=False, rr_depth=3, lanes_per_pixel=0,
                         denoise=False, checkpoint=None, force_f64=False, on_pass=None, checkpoint_every=1,
                         max_passes=None, moments=False, **denoise_params):
    """render_adaptive for caller-supplied rays: every record is sampled until
    its err <= tol or it has max_spp samples (a RayAccumulator; sample s of a
    record is Renderer.render_rays' sample s).  o, d (n, 3) f64, keys (n,) u32
    (None: 0..n-1) as for render_rays; shape=None: a flat batch, the result's
    fb, counts and err are (n, ...); shape=(H, W): the records of an image in
    image orientation (cameras.to_image_order), the result's arrays are
    (H, W, ...).  denoise=True (denoise_params: make_denoise's) also gives the
    filtered values, their variance and the records' first-hit features —
    neighbours are neighbours in the shape.  lanes_per_pixel: lanes per record,
    0 lets the library choose per pass; checkpoint, checkpoint_every,
    max_passes, moments, on_pass, force_f64: as for render_adaptive (a resumed
    run continues bit for bit at a fixed lanes_per_pixel).  The passes run the
    list kernel over ray records on every scene.  Returns an AdaptiveResult."""
    check_rule(tol, max_spp, min_spp, step_spp, floor)
    if denoise_params and not denoise:
        raise ValueError(f"{sorted(denoise_params)}: filter parameters need denoise=True")
    if int(checkpoint_every) < 1:
        raise ValueError("checkpoint_every must be >= 1")
    rec, (H, W) = ray_records(o, d, keys, shape)
    seed = renderer.scene.seed if seed is None else seed
    seed = 0 if seed is None else int(seed)
    flags = (PT_FLAG_RR if rr else 0) | (PT_FLAG_FORCE_F64 if force_f64 else 0)
    params = make_params(W, H, max_spp, bounces, seed, flags, rr_depth)
    adapt = make_adapt(tol, max_spp, min_spp, step_spp, floor)
    ck = checkpoint if isinstance(checkpoint, AccumCheckpoint) or checkpoint is None \
        else AccumCheckpoint(checkpoint)
    key = None
    if ck is not None:
        key = accum_key(renderer.packed, W, H, bounces, params.seed, rr, rr_depth, lanes_per_pixel,
                        rays=rec, shape=shape)
    kw = dict(band=make_band(H, lanes_per_pixel=lanes_per_pixel)) if lanes_per_pixel else {}
    return _run(lambda: RayAccumulator(renderer, rec["o"], rec["d"], rec["key"], (H, W), **kw), W, H, params,
                adapt, ck, key, on_pass, max_passes, checkpoint_every, moments,
                (denoise_params or True) if denoise else None,
                shape=None if shape is not None else (rec.shape[0],))


def transfer_band(src, dst, band):
    """The state of src's band (an Accumulator whose band is `band`) into the
    same rows of dst, device to device: export into a tile on src's device,
    one 1-D copy to dst's device (none when they share it), import."""
    import torch
    P = len(band_pixels(src.width, src.height, band))
    if P == 0:
        return
    with src._device():
        tile = torch.empty(60 * P, dtype=torch.uint8, device="cuda")
        src.export_band_device(tile.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
    with dst._device():
        there = tile.to(torch.device("cuda", torch.cuda.current_device()))
        stream = torch.cuda.current_stream()
        stream.synchronize()   # the copy has landed
        dst.import_band(band, there.data_ptr(), stream.cuda_stream)
        stream.synchronize()   # before the tiles are freed


def _drain(accs):
    """Wait for the accumulators' devices; the time afterwards."""
    import torch
    for a in accs:
        with a._device():
            torch.cuda.synchronize()
    return time.perf_counter()


def render_adaptive_multi(renderers, width=None, height=None, max_spp=64, bounces=1, seed=None, rr=False,
                          rr_depth=3, tol=0.05, min_spp=8, step_spp=8, floor=0.01, force_f64=False,
                          on_pass=None, megakernel=False, denoise=None, lanes_per_pixel=0,
                          moments=False, timings=None, aa=False, lens=None):
    """render_adaptive on the renderers of a render.MultiRenderer (one scene
    on N devices): device d gets a banded accumulator of the rows
    distributed.rank_band(H, d, N) and runs its own pass loop — a round-robin
    of select, then render, over the devices that still list pixels; the
    render is asynchronous, so the devices work at the same time.  At the end
    the tiles of bands 1..N-1 move into device 0's accumulator, which becomes
    whole-frame and is read (and denoised) there.  passes[i] is the sum over
    the devices of their pass i: the one-device run's.  With a fixed
    lanes_per_pixel the moments are the one-device run's bit for bit, with 0
    to the sum order (pt_accum_band).  on_pass is called once per round.
    timings: a dict that receives passes_ms and merge_ms (wall time; the
    devices are then drained between the two — scripts/bench_adaptive.py)."""
    from .distributed import rank_band
    check_rule(tol, max_spp, min_spp, step_spp, floor)
    if denoise is not None and denoise is not True and not isinstance(denoise, dict):
        raise ValueError("denoise: None, True or a dict of filter parameters")
    r0 = renderers[0]
    N = len(renderers)
    width = int(r0.scene.width if width is None else width)
    height = int(r0.scene.height if height is None else height)
    seed = r0.scene.seed if seed is None else seed
    seed = 0 if seed is None else int(seed)
    flags = (PT_FLAG_RR if rr else 0) | (PT_FLAG_FORCE_F64 if force_f64 else 0) | \
        (PT_FLAG_MEGAKERNEL if megakernel else 0) | (PT_FLAG_AA if aa else 0) | \
        (PT_FLAG_LENS if lens_of(r0, lens) is not None else 0)   # (every renderer of a MultiRenderer has the lens)
    params = make_params(width, height, max_spp, bounces, seed, flags, rr_depth)
    adapt = make_adapt(tol, max_spp, min_spp, step_spp, floor)
    bands = [make_band(height, *rank_band(height, d, N), lanes_per_pixel=lanes_per_pixel)
             for d in range(N)]
    accs = []
    try:
        for r, b in zip(renderers, bands):
            accs.append(Accumulator(r, width, height, band=b))
        rounds = []
        live = list(range(N))
        t0 = time.perf_counter()
        while live:
            if len(rounds) > int(adapt.max_spp):
                raise RuntimeError(f"adaptive run did not end within {int(adapt.max_spp) + 1} passes")
            still, n_sum, k_sum = [], 0, 0
            for d in live:   # a device whose list is empty has finished: it leaves the round-robin
                n_active, k = accs[d].select(adapt)
                if n_active == 0:
                    continue
                accs[d].render(params, adapt)
                still.append(d)
                n_sum, k_sum = n_sum + int(n_active), k_sum + int(k)
            live = still
            if live:
                rounds.append((n_sum, k_sum))
                if on_pass is not None:
                    on_pass(len(rounds), n_sum, k_sum)
        acc = accs[0]
        if timings is not None:
            t1 = _drain(accs)
        for d in range(1, N):
            transfer_band(accs[d], acc, bands[d])
        acc.set_band(make_band(height, lanes_per_pixel=lanes_per_pixel))
        if timings is not None:
            t2 = _drain(accs[:1])
            timings.update(passes_ms=(t1 - t0) * 1e3, merge_ms=(t2 - t1) * 1e3)
        # (the bands' last selects left err; the merged frame carries it)
        m = acc.read(S=True, Q=bool(moments), n=True, err=True)
        den = var = feat = None
        if denoise is not None:
            den, var = acc.denoise(**(denoise if isinstance(denoise, dict) else {}))
            feat = acc.features()
    finally:
        for a in accs:
            a.close()
    n = m["n"]
    fb = np.where(n[..., None] > 0, m["S"] / np.maximum(n, 1)[..., None], 0.0)
    return AdaptiveResult(fb, n, m["err"], rounds, den, var, feat,
                          *((m["S"], m["Q"]) if moments else ()))
